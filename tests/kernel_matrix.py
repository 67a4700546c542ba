"""The kernel-instantiation matrix: case generators, the launch plan each case
must produce and the set of instantiations the matrix has to reach.

Shared by tests/test_gpu_kernel_matrix.py (runs the cases on the device and
compares the library's launch record, nxec_debug_launch_log, with the plan
made here) and tests/test_kernel_matrix_plan.py (checks this file against the
kernel sources and the oracle on the CPU).

An instantiation is named by a tuple:
  ("k_mul_vec", k, R, gather, copy, full)    ("k_mul_perm", k, gather)
  ("k_mul_vec_dyn", gather)                  ("k_mul_bytes", gather)
  ("k_scrub_vec", kd, rows, full)            ("k_mul_ragged", k)
  ("k_mul_md5", k, hsrc)                     ("k_gather_md5", k, hsrc)
  ("k_files_md5", k, mask, tstore)           ("k_mul_mixed", k)
  ("k_decode_mixed", k)                      ("k_update_vec", r)
k_mul_list, k_scrub_bytes and k_update_bytes are not templates over k; their
launches are recorded and checked per case but are not part of the set.  The
plain MD5 launches (k_md5: launch_md5, launch_md5_list) are not recorded at
all; tests/digest_matrix.py covers that kernel by its results.  k_update_vec
takes k at run time, but k sizes its LDS and the updated chunk's index picks
the table, so group (h) still runs every k.

The constants below mirror nexoedge_amd/csrc (the CPU test reads the sources
and fails when one moves).
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nexoedge_amd", "csrc")

KBLOCK = 1024             # vectors (16 bytes) per tile
TILE = KBLOCK * 16
LDS_BYTES = 160 * 1024
RING_BYTES = 16
MAX_TEMPL_K = 20          # kMaxTemplK
PREFETCH_MAX_K = 10       # kPrefetchMaxK
PREFETCH_MAX_K_COPY = 8   # kPrefetchMaxKCopy
PERM_PREFETCH_MAX_K = 4   # kPermPrefetchMaxK
PERM_MAX_K = 13           # kPermMaxK
MAX_ROWS = 4              # kMaxRowsPerPass
RAGGED_MAX_K = 19         # kMaxRaggedK
SCRUB_MAX_K = 16          # kScrubMaxK
SCRUB_MAX_SRC = 20        # kScrubMaxSrc
MUL_MD5_MAX_K = 20        # kEncMd5MaxK
GATHER_MD5_MAX_K = 16     # kGatherMd5MaxK
FILES_MD5_MAX_K = 16      # kFilesMd5MaxK
UPDATE_MAX_K16 = 9        # kUpdateMaxK16
SENTINEL = 0xEE
MIXED_LOST = -1           # NXEC_RECOVER_LOST

SOURCE_CONSTANTS = {  # name in the sources -> (file, value here)
    "kBlock": ("nxec_kernels.hip", KBLOCK),
    "kMaxTemplK": ("nxec_kernels.hip", MAX_TEMPL_K),
    "kPrefetchMaxK": ("nxec_kernels.hip", PREFETCH_MAX_K),
    "kPrefetchMaxKCopy": ("nxec_kernels.hip", PREFETCH_MAX_K_COPY),
    "kPermPrefetchMaxK": ("nxec_kernels.hip", PERM_PREFETCH_MAX_K),
    "kPermMaxK": ("nxec_kernels.hip", PERM_MAX_K),
    "kRingBytes": ("nxec_kernels.hip", RING_BYTES),
    "kUpdateMaxK16": ("nxec_kernels.hip", UPDATE_MAX_K16),
    "kMaxRowsPerPass": ("nxec_internal.h", MAX_ROWS),
    "kMaxRaggedK": ("nxec_internal.h", RAGGED_MAX_K),
    "kScrubMaxK": ("nxec_internal.h", SCRUB_MAX_K),
    "kScrubMaxSrc": ("nxec_internal.h", SCRUB_MAX_SRC),
    "kEncMd5MaxK": ("nxec_internal.h", MUL_MD5_MAX_K),
    "kGatherMd5MaxK": ("nxec_internal.h", GATHER_MD5_MAX_K),
    "kFilesMd5MaxK": ("nxec_internal.h", FILES_MD5_MAX_K),
}


def source_constant(name):
    """The value of `constexpr int <name> = <int>;` in its source file."""
    path = os.path.join(CSRC, SOURCE_CONSTANTS[name][0])
    with open(path) as f:
        m = re.search(r"constexpr int %s = (\d+)\s*;" % re.escape(name), f.read())
    assert m, f"{name} not found in {path}"
    return int(m.group(1))


def rup(x, m=16):
    return (x + m - 1) // m * m


# ------------------------------------------------------------ dispatch model
def default_r(k):
    return 16 if k <= 9 else 8


def queue_fits(table_bytes):
    return table_bytes + RING_BYTES <= LDS_BYTES


def vec_prefetch(k, copy, full):
    return k <= (PREFETCH_MAX_K_COPY if (copy or not full) else PREFETCH_MAX_K)


def vec_queued(k, r):
    return queue_fits(k * 1024 * r)


def scrub_prefetch(nsrc, full):
    return nsrc <= (PREFETCH_MAX_K if full else PREFETCH_MAX_K_COPY)


def use_perm(k, rows, full, copy, gather):
    if rows != 1 or k > PERM_MAX_K or not full or copy:
        return False
    return not (k == 11 and not gather)  # the one instantiation the library keeps off the VALU kernel


def tiles_per_grab(k, rows, copies=0):
    return max(1, min(8, -(-12 // (k + rows + copies))))


def stripe_group(nvec, aliased):
    return 8 if (-(-nvec // KBLOCK) >= 128 and aliased) else 1


def mul_launches(k, rows, length, *, gather=False, copies=0, vec_ok=True, chunk_stride=0):
    """The launches nxec_stripes_mul / nxec_stripes_mul_ptrs make for one call, in
    order, as dicts of launch-record fields (grid and slot left out)."""
    out = []
    passes = 1 if rows == 0 else -(-rows // MAX_ROWS)
    nvec = length // 16 if vec_ok else 0
    for p in range(passes):
        pr = max(min(MAX_ROWS, rows - p * MAX_ROWS), 0)
        ncp = copies if p == 0 else 0
        copy = ncp > 0
        nfull = nvec // KBLOCK * KBLOCK
        sg = stripe_group(nvec, gather or chunk_stride % (1 << 20) == 0)
        for full, cnt in ((True, nfull), (False, nvec - nfull)):
            if cnt <= 0:
                continue
            tpg = tiles_per_grab(k, pr, ncp)
            base = dict(k=k, rows=pr, gather=int(gather), copy=int(copy), full=int(full))
            if use_perm(k, pr, full, copy, gather):
                out.append(dict(base, family="k_mul_perm", r=0, pf=int(k <= PERM_PREFETCH_MAX_K), q=1, tpg=tpg, sg=sg))
            elif k > MAX_TEMPL_K:
                out.append(dict(base, family="k_mul_vec_dyn", r=1, pf=0, q=0, tpg=0, sg=1))
            else:
                r = default_r(k)
                out.append(dict(base, family="k_mul_vec", r=r, pf=int(vec_prefetch(k, copy, full)),
                                q=int(vec_queued(k, r)), tpg=tpg, sg=sg))
        if nvec * 16 < length:
            out.append(dict(family="k_mul_bytes", k=k, rows=pr, r=1, gather=int(gather), copy=int(copy), full=0, pf=0,
                            q=0, tpg=0, sg=1, byte_begin=nvec * 16))
    return out


def scrub_launches(kd, rows, length, chunk_stride):
    """The detect-stage launches of nxec_rs_scrub_stripes(n = kd + rows, k = kd) on an aligned batch."""
    assert kd <= SCRUB_MAX_K and 1 <= rows <= MAX_ROWS and kd + rows <= SCRUB_MAX_SRC
    out = []
    nvec = length // 16
    nfull = nvec // KBLOCK * KBLOCK
    sg = stripe_group(nvec, chunk_stride % (1 << 20) == 0)
    for full, cnt in ((True, nfull), (False, nvec - nfull)):
        if cnt > 0:
            out.append(dict(family="k_scrub_vec", kd=kd, rows=rows, r=default_r(kd), full=int(full),
                            pf=int(scrub_prefetch(kd + rows, full)), q=1, tpg=tiles_per_grab(kd, rows), sg=sg))
    if nvec * 16 < length:
        out.append(dict(family="k_scrub_bytes", kd=kd, rows=rows, byte_begin=nvec * 16))
    return out


def mixed_launch(k, decode):
    """The one launch of nxec_rs_recover_stripes_mixed / nxec_rs_decode_stripes_mixed on an aligned batch with
    k <= RAGGED_MAX_K (launch_mixed): `rows` is always MAX_ROWS, the segment records carry the real counts."""
    assert 1 <= k <= RAGGED_MAX_K
    tpg = tiles_per_grab(k, 0, k) if decode else tiles_per_grab(k, MAX_ROWS)
    return dict(family="k_decode_mixed" if decode else "k_mul_mixed", k=k, rows=MAX_ROWS, r=default_r(k),
                pf=int(k <= PREFETCH_MAX_K_COPY), q=1, tpg=tpg)


def update_launches(n, k, rounds):
    """The launches of nxec_rs_update_stripes(n, k) in order; `rounds` lists (vector tiles, updates, byte items)
    per round.  Per round and per pass of <= MAX_ROWS parity rows: launch_update_vec, then launch_update_bytes
    (each left out when it has no work); only the last pass stores the new data."""
    out = []
    m = n - k
    passes = max(1, -(-m // MAX_ROWS))
    for rnd, (tiles, updates, items) in enumerate(rounds):
        for p in range(passes):
            rows = min(MAX_ROWS, m - p * MAX_ROWS)
            last = int(p == passes - 1)
            where = {"round": rnd, "pass": p, "last": last}
            if tiles > 0:
                assert k <= RAGGED_MAX_K
                out.append(dict(family="k_update_vec", k=k, rows=rows, r=default_r(k), pf=1, q=1,
                                tpg=tiles_per_grab(2 + last, 2 * rows), tiles=tiles, updates=updates, **where))
            if items > 0:
                out.append(dict(family="k_update_bytes", k=k, rows=rows, r=1, items=items, **where))
    return out


def update_counters(n, k, cs, ss, length, addr, ups):
    """(rounds, vector tiles, byte items) of a valid update list [(stripe, chunk, offset, length, d_new)],
    evaluated update by update: what nxec_rs_update_plan counts (nxec_update_host.cpp)."""
    live = [u for u in ups if u[3] > 0]
    # rounds: the most updates over one column of one stripe (sweep over the range ends)
    rounds = 0
    for stripe in {u[0] for u in live}:
        ev = sorted([(u[2], 1) for u in live if u[0] == stripe] + [(u[2] + u[3], -1) for u in live if u[0] == stripe])
        depth = 0
        for _, d in ev:  # at equal columns the -1 sorts first: adjacent ranges do not stack
            depth += d
            rounds = max(rounds, depth)
    vec_layout = k <= RAGGED_MAX_K and addr % 16 == 0 and cs % 16 == 0 and ss % 16 == 0
    tiles = items = 0
    for _, _, off, ln, p in live:
        b0, b1 = rup(off), (off + ln) // 16 * 16
        if vec_layout and b0 < b1 and (p + b0 - off) % 16 == 0:
            tiles += -(-((b1 - b0) // 16) // KBLOCK)
            items += (off < b0) + (b1 < off + ln)
        else:
            items += 1
    return rounds, tiles, items


def inst_of(rec):
    """Launch record (dict) -> instantiation tuple, or None for a kernel that is not a template over k."""
    f = rec["family"]
    if f in ("k_mul_mixed", "k_decode_mixed"):
        return (f, rec["k"])
    if f == "k_update_vec":
        return (f, rec["r"])
    if f == "k_mul_vec":
        return (f, rec["k"], rec["r"], rec["gather"], rec["copy"], rec["full"])
    if f == "k_mul_perm":
        return (f, rec["k"], rec["gather"])
    if f in ("k_mul_vec_dyn", "k_mul_bytes"):
        return (f, rec["gather"])
    if f == "k_scrub_vec":
        return (f, rec["kd"], rec["rows"], rec["full"])
    if f == "k_mul_ragged":
        return (f, rec["k"])
    if f in ("k_mul_md5", "k_gather_md5"):
        return (f, rec["k"], rec["hsrc"])
    if f == "k_files_md5":
        return (f, rec["k"], rec["mask"], rec["tstore"])
    return None


def matches(rec, want):
    """Every field of the planned launch `want` has that value in the recorded launch."""
    return all(rec.get(key) == v for key, v in want.items())


# Variants no public entry point reaches, taken out of the expected set.
# k_files_md5<1, MASK, !TSTORE>: nxec_encode_objects masks the data chunk that holds an object's last
# bytes when it is partial; with k = 1 the last stripe's chunk length is the remainder itself, so its one
# chunk is never partial and OBJECTS_TAIL_INPLACE launches the plain kernel.
UNREACHABLE = {("k_files_md5", 1, 1, 0)}


def expected_instantiations():
    s = set()
    for k in range(1, MAX_TEMPL_K + 1):
        for gather, copy in ((0, 0), (0, 1), (1, 0)):
            for full in (0, 1):
                s.add(("k_mul_vec", k, default_r(k), gather, copy, full))
        for hsrc in (0, 1):
            s.add(("k_mul_md5", k, hsrc))
    for k in range(1, PERM_MAX_K + 1):
        for gather in (0, 1):
            if use_perm(k, 1, True, False, bool(gather)):
                s.add(("k_mul_perm", k, gather))
    for gather in (0, 1):
        s.add(("k_mul_vec_dyn", gather))
        s.add(("k_mul_bytes", gather))
    for kd in range(1, SCRUB_MAX_K + 1):
        for rows in range(1, MAX_ROWS + 1):
            for full in (0, 1):
                s.add(("k_scrub_vec", kd, rows, full))
    for k in range(1, RAGGED_MAX_K + 1):
        s.add(("k_mul_ragged", k))
        s.add(("k_mul_mixed", k))
        s.add(("k_decode_mixed", k))
    for r in (16, 8):
        s.add(("k_update_vec", r))
    for k in range(1, GATHER_MD5_MAX_K + 1):
        for hsrc in (0, 1):
            s.add(("k_gather_md5", k, hsrc))
    for k in range(1, FILES_MD5_MAX_K + 1):
        for mask, tstore in ((0, 0), (1, 0), (1, 1)):
            s.add(("k_files_md5", k, mask, tstore))
    return s - UNREACHABLE


# ------------------------------------------------------------------ inputs
def coefficients(rows, k, seed):
    """Seeded random rows x k matrix with a 0, a 1 and a 0xFF forced into every row (as far as k allows)."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, size=(max(rows, 0), k), dtype=np.uint8)
    vals = (0, 1, 0xFF)
    for r in range(rows):
        if k >= 3:
            for i, v in enumerate(vals):
                c[r, (r + i) % k] = v
        else:  # too narrow for all three: the rows take turns
            for j in range(k):
                c[r, j] = vals[(r + j) % 3]
    return c


# ------------------------------------------------- (a) every instantiation
A_LEN = TILE + 48 + 5  # one complete tile, a 3-vector ragged launch, a 5-byte tail
A_STRIPES = 3
A_STRIDE = rup(A_LEN) + 48  # padded chunk stride
A_KS = list(range(1, MAX_TEMPL_K + 1)) + [21, 24]
A_FORMS = ("strided", "copy", "gather")


def a_cases():
    """(id, dict) of group (a): form x k x rows, then the specials."""
    out = []
    for form in A_FORMS:
        for k in A_KS:
            for rows in (1, 2, 3, 4):
                out.append(dict(form=form, k=k, rows=rows, length=A_LEN, base=0))
    for k in (3, 12, 21):  # copies only
        out.append(dict(form="copy", k=k, rows=0, length=A_LEN, base=0))
    out.append(dict(form="gather", k=5, rows=6, length=A_LEN, base=0))  # two passes: dst_ptr_row0 = 4
    # the byte kernel carries whole chunks: a strided layout 3 bytes off alignment; the gather form
    # (whose pointers must be aligned) with chunks shorter than one vector
    out.append(dict(form="strided", k=7, rows=3, length=A_LEN, base=3))
    out.append(dict(form="copy", k=7, rows=3, length=A_LEN, base=3))
    out.append(dict(form="gather", k=7, rows=3, length=13, base=0))
    return out


def a_copies(case):
    return min(2, case["k"]) if case["form"] == "copy" else 0


def a_plan(case):
    return mul_launches(case["k"], case["rows"], case["length"], gather=case["form"] == "gather",
                        copies=a_copies(case), vec_ok=case["base"] == 0, chunk_stride=A_STRIDE)


def case_id(case):
    return "-".join(f"{key}{v}" if not isinstance(v, str) else v for key, v in case.items())


# ------------------------------------------------ (b) queue steady state
B_CS = 65536  # 4 complete tiles per chunk


def b_cases():
    out = [dict(form="strided", k=k, rows=4) for k in range(1, 20)]
    out += [dict(form="strided", k=k, rows=1) for k in range(1, PERM_MAX_K + 1)]
    out += [dict(form="gather", k=k, rows=1) for k in (4, 5, 11, 13)]
    out += [dict(form="copy", k=k, rows=4) for k in (8, 9, 10)]
    out += [dict(form="strided", k=20, rows=4)]  # no room for the queue ring: static tile order
    return out


def b_copies(case):
    return 2 if case["form"] == "copy" else 0


def b_stripes(case, cus):
    """Enough stripes for >= 4 * cus * T tiles: at least half of all tiles come from published grabs
    (each workgroup's two initial grabs cover 2 * cus * T)."""
    t = tiles_per_grab(case["k"], case["rows"], b_copies(case))
    return -(-4 * cus * t // (B_CS // TILE))


def b_plan(case):
    return mul_launches(case["k"], case["rows"], B_CS, gather=case["form"] == "gather", copies=b_copies(case),
                        chunk_stride=B_CS)


def b_seed(case):
    return 77000 + 100 * case["k"] + 10 * case["rows"] + A_FORMS.index(case["form"])


# ------------------------------------------------------- (c) tile order
C_CS = (2 << 20) + 4096
C_STRIPES = (1, 9, 19)

# ---------------------------------------------------------- (d) scrub
D_LEN = TILE + 16
D_STRIPES = 2
D_STRIDE = D_LEN + 48
D_FLIP_POS = (5000, TILE + 7)  # inside the complete tile, inside the ragged vector


def d_cases():
    return [(kd, rows) for kd in range(1, SCRUB_MAX_K + 1) for rows in range(1, MAX_ROWS + 1)]


def d_flip_chunks(kd, rows):
    return sorted({0, kd - 1} | set(range(kd, kd + rows)))


def d_queue_cases():
    """(kd, rows) on each side of the scrub kernel's prefetch boundary (complete tiles)."""
    return [(PREFETCH_MAX_K - MAX_ROWS, MAX_ROWS), (PREFETCH_MAX_K - MAX_ROWS + 1, MAX_ROWS)]


# ------------------------------------------------------ (e) fused MD5
E_CS = 768  # three 256-byte steps
E_STRIPES = 17


def e_p(k):
    return 1 if k % 2 else 4  # alternates between 1 and 4


# ------------------------------------------- the mixed plan, in Python
def sentinel_bytes(nbytes):
    """A position-dependent fill of period 251 (a prime: no chunk or stripe stride here is a multiple)."""
    return np.resize(((np.arange(251, dtype=np.uint32) * 7 + 0x5A) % 251).astype(np.uint8), nbytes)


def mixed_model(n, k, sets, decode):
    """What mixed_plan and mixed_tables (nxec_mixed_host.cpp) make of one erased set per stripe, for sets whose
    first k alive chunks invert (the CPU test checks that with the oracle; SINGULAR is not modelled).
    Recover keys a plan by the erased set, rebuilds all of it and leaves a clean stripe unplanned; Decode keys
    a plan by the first k alive ids, rebuilds the lost data chunks and plans a clean stripe as a pure copy.
    More than n - k erasures: MIXED_LOST.  Plans become segments of <= MAX_ROWS rows in first-appearance
    order (a plan without rows is one segment of 0 rows); items run by segment, then ascending stripe.
    Returns dict(verdict per stripe, plans, segs, stripes planned, seg_rows per segment, order: stripe per item)."""
    index, plan_rows, plan_stripes, verdict = {}, [], [], []
    for s, e in enumerate(sets):
        e = sorted(set(e))
        assert all(0 <= c < n for c in e)
        if len(e) > n - k:
            verdict.append(MIXED_LOST)
            continue
        if decode:
            key = tuple([c for c in range(n) if c not in e][:k])
            rows = sum(c < k for c in e)
        else:
            key, rows = tuple(e), len(e)
            if not e:
                verdict.append(0)
                continue
        if key not in index:
            index[key] = len(plan_rows)
            plan_rows.append(rows)
            plan_stripes.append([])
        assert plan_rows[index[key]] == rows
        plan_stripes[index[key]].append(s)
        verdict.append(rows)
    seg_rows, order = [], []
    for rows, stripes in zip(plan_rows, plan_stripes):
        for r0 in range(0, max(rows, 1), MAX_ROWS):
            seg_rows.append(min(MAX_ROWS, rows - r0))
            order += stripes
    return dict(verdict=verdict, plans=len(plan_rows), segs=len(seg_rows), stripes=sum(map(len, plan_stripes)),
                seg_rows=seg_rows, order=order)


def first_alive(n, k, e):
    return [c for c in range(n) if c not in e][:k]


MIXED_MODES = ("recover", "decode")
MIXED_EXTRA = 6  # groups (f) and (g): n = k + 6, so plans of 5 and 6 erasures (two segments) exist for every k


def three_of(k):
    """Chunk 0, chunk 1 and the first parity chunk (k = 1 has no chunk 1: two ids)."""
    return tuple(sorted({0, min(1, k - 1), k}))


# ---------------------------------------- (f) every mixed instantiation
F_LEN = TILE + 48             # one complete tile and a tile of 3 vectors
F_STRIDE = F_LEN + 48         # source chunk stride; the stripe stride is one chunk more than n chunks
F_OUT_STRIDE = F_LEN + 32     # decode: output chunk stride; the stripe stride is one chunk more than k chunks


def f_cases():
    return [(mode, k) for mode in MIXED_MODES for k in range(1, RAGGED_MAX_K + 1)]


def f_lost(k):
    return tuple(range(MIXED_EXTRA + 1))


def f_sets(k, decode):
    """One erased set per stripe.  The first plans to appear have 4, 1, 2 and 3 rows (as far as k allows:
    the decode's rows are the lost data chunks, at most k), so a 4-row segment is followed by each shorter
    one; then every chunk as the only target, pairs and triples across the data/parity border, full sets of
    4, plans of 5 and 6 (two segments), the one LOST stripe, and a clean stripe at each end."""
    n = k + MIXED_EXTRA
    two = three_of(k) if decode else (0, n - 1)  # two lost data chunks / two erased chunks
    sets = [(), tuple(range(4)), (0,), two, tuple(range(3))]
    sets += [(c,) for c in range(1, n)]
    sets += [(0, n - 1), (k - 1, k), three_of(k), tuple(range(n - 4, n)), tuple(range(0, n, 2))[:4], tuple(range(5)),
             f_lost(k), tuple(range(n - 6, n)), tuple(range(k - 1, k + 5)), ()]
    return sets


def f_row_sequence(k, decode):
    """The rows of the segments that the first plans of f_sets make: 4, 1, 2, 3, but a decode has at most k
    lost data chunks (and at k = 2 the 2-row and the 3-row set are the same set)."""
    if not decode:
        return [4, 1, 2, 3]
    return [min(4, k), 1, min(2, k)] + ([3] if k >= 3 else [])


# ------------------------------------------- (g) mixed steady state
G_KS = (1, PREFETCH_MAX_K_COPY, UPDATE_MAX_K16, RAGGED_MAX_K)  # most tiles per grab, last prefetch, largest table, widest
G_CS = TILE  # one tile per chunk, packed


def g_cases():
    return [(mode, k) for mode in MIXED_MODES for k in G_KS]


def g_sets(k):
    """The patterns stripe s % len takes, for both modes: 4, 1, 0, 6, 2, 3, 4, 5 and 3 erased chunks.  Recover:
    a 4-row segment, then 1 row; 6 and 5 erasures are plans of two segments (4 + 2, 4 + 1); the clean stripes
    are unplanned.  Decode (rows = lost data chunks): 4, 1, then the clean plan, a pure-copy segment between
    coded ones that the parity-only set joins; range(5) is its plan of two segments where k >= 5."""
    n = k + MIXED_EXTRA
    return [tuple(range(4)), (k - 1,), (), tuple(range(k - 1, k + 5)), (0, n - 1), three_of(k), tuple(range(n - 4, n)),
            tuple(range(5)), tuple(range(3))]


def g_stripes(k, decode, cus):
    """4 * cus * T stripes of one tile: at least half of all tiles come from published grabs."""
    return 4 * cus * mixed_launch(k, decode)["tpg"]


def g_seed(k, decode):
    return 99000 + 10 * k + int(decode)


# ------------------------------------------------- (h) update sweep
H_ROWS = (4, 6, 1, 2, 5, 3)
H_OFF, H_BYTES = 3, TILE + 40  # a 13-byte head, 1025 vectors (a full tile and one more), an 11-byte tail


def h_p(k):
    return H_ROWS[(k - 1) % len(H_ROWS)]


def h_specs(k):
    """(stripe, chunk, offset, length): stripe s < k updates chunk s; stripe k stays untouched."""
    return [(s, s, H_OFF, H_BYTES) for s in range(k)]


def h_new_offset(i):
    """Where update i's new bytes start in the d_new buffer: 64-byte slots, aligned like the chunk offset."""
    return 64 + i * rup(H_BYTES + 64, 64) + H_OFF % 16


def h_plan(k, batch_addr=0, new_addr=0):
    """The launches of the (h) case of k; the addresses only matter modulo 16."""
    n, cs = k + h_p(k), F_STRIDE
    ups = [(s, c, off, ln, new_addr + h_new_offset(i)) for i, (s, c, off, ln) in enumerate(h_specs(k))]
    rounds, tiles, items = update_counters(n, k, cs, n * cs, F_LEN, batch_addr, ups)
    assert rounds == 1
    return update_launches(n, k, [(tiles, len(ups), items)])


def all_cases():
    """Every (group, instantiations the case's plan names) pair that can be planned without a device."""
    out = []
    for mode, k in f_cases():
        out.append(("f", [inst_of(mixed_launch(k, mode == "decode"))]))
    for mode, k in g_cases():
        out.append(("g", [inst_of(mixed_launch(k, mode == "decode"))]))
    for k in range(1, RAGGED_MAX_K + 1):
        out.append(("h", [i for i in map(inst_of, h_plan(k)) if i is not None]))
    for c in a_cases():
        out.append(("a", [inst_of(r) for r in a_plan(c)]))
    for c in b_cases():
        out.append(("b", [inst_of(r) for r in b_plan(c)]))
    for ns in C_STRIPES:
        out.append(("c", [inst_of(r) for r in mul_launches(2, 1, C_CS, gather=True)]))
    for kd, rows in d_cases():
        out.append(("d", [inst_of(r) for r in scrub_launches(kd, rows, D_LEN, D_STRIDE)]))
    for kd, rows in d_queue_cases():
        out.append(("d", [inst_of(r) for r in scrub_launches(kd, rows, B_CS, B_CS)]))
    for k in range(1, MUL_MD5_MAX_K + 1):
        out.append(("e", [("k_mul_md5", k, 1), ("k_mul_md5", k, 0)]))
    for k in range(1, GATHER_MD5_MAX_K + 1):
        out.append(("e", [("k_gather_md5", k, 0), ("k_gather_md5", k, 1)]))
    for k in range(1, FILES_MD5_MAX_K + 1):
        out.append(("e", [("k_files_md5", k, 0, 0), ("k_files_md5", k, int(k > 1), 0), ("k_files_md5", k, 1, 1)]))
    for k in range(1, RAGGED_MAX_K + 1):
        out.append(("e", [("k_mul_ragged", k)]))
    return out
