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
  ("k_files_md5", k, mask, tstore)
k_mul_list, k_scrub_bytes and the plain MD5 kernels are not templates over k;
their launches are recorded and checked per case but are not part of the set.

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
SENTINEL = 0xEE

SOURCE_CONSTANTS = {  # name in the sources -> (file, value here)
    "kBlock": ("nxec_kernels.hip", KBLOCK),
    "kMaxTemplK": ("nxec_kernels.hip", MAX_TEMPL_K),
    "kPrefetchMaxK": ("nxec_kernels.hip", PREFETCH_MAX_K),
    "kPrefetchMaxKCopy": ("nxec_kernels.hip", PREFETCH_MAX_K_COPY),
    "kPermPrefetchMaxK": ("nxec_kernels.hip", PERM_PREFETCH_MAX_K),
    "kPermMaxK": ("nxec_kernels.hip", PERM_MAX_K),
    "kRingBytes": ("nxec_kernels.hip", RING_BYTES),
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


def inst_of(rec):
    """Launch record (dict) -> instantiation tuple, or None for a kernel that is not a template over k."""
    f = rec["family"]
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


def all_cases():
    """Every (group, instantiations the case's plan names) pair that can be planned without a device."""
    out = []
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
