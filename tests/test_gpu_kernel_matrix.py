"""Parity matrix over every kernel instantiation (tests/kernel_matrix.py).

Every hot kernel is a template instantiated once per k and picked from a
table at launch, so each k is its own compiled code.  This module runs every
instantiation at the smallest shape that reaches it, compares every output
bit-exactly with the plain-C oracle (oracle.matmul / oracle.rs_encode, and
oracle.simd_encode -- pinned to the oracle by test_oracle_golden -- for the
large work-queue shapes) and hashlib.md5, and checks the library's launch
record (nxec_debug_launch_log) against the plan: a case that silently moved to
another kernel fails.  Output buffers are prefilled with 0xEE and compared
whole: bytes past the chunk length, unselected rows and stride padding must
stay untouched.  The last test asserts that the instantiations seen over the
module are exactly kernel_matrix.expected_instantiations(), so it needs the
whole module to have run.

Groups: (a) every multiply instantiation, (b) the work queue's steady state
(workgroups consuming published grabs) for every queued instantiation, (c) the
stripe-group tile order, (d) scrub detect for all 64 (KD, ROWS), (e) the fused
MD5 families and the ragged launch, (f) every mixed recover and mixed decode
instantiation on a batch whose stripes lost different chunks, (g) the mixed
kernels' steady state, where a workgroup's next tile is nearly always of
another segment than the one whose tables are resident, (h) the update
kernels at every k, every chunk index the updated one once.

In (f), (g) and (h) the batches are built on the host: data random (or the
fill stream), parity from oracle.rs_encode (oracle.simd_encode in (g)); the
expected verdicts and the launch's segment and stripe counts come from the
Python model of the plan in kernel_matrix.py, never from a library call.
"""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

import kernel_matrix as km
import oracle
from nexoedge_amd import _lib, nxec

pytestmark = pytest.mark.gpu

lib = _lib.lib
EE = km.SENTINEL
SEEN = set()  # instantiations recorded by the cases of this module


@pytest.fixture(scope="module", autouse=True)
def launch_record():
    nxec.launch_log(True)
    yield
    nxec.launch_log(False)


def note(recs):
    for r in recs:
        inst = km.inst_of(r)
        if inst is not None:
            SEEN.add(inst)
    return recs


def take(plan, only=None):
    """Reads the launch record; the launches (of the families in `only`, if given) must be the planned ones, in order."""
    recs = note(nxec.launch_log_read())
    mine = [r for r in recs if only is None or r["family"] in only]
    assert len(mine) == len(plan) and all(km.matches(r, w) for r, w in zip(mine, plan)), (mine, plan)
    return mine


def up(a):
    a = np.ascontiguousarray(a)
    b = nxec.DeviceBuffer(a.nbytes)
    b.upload(a)
    return b


def md5(a):
    return np.frombuffer(hashlib.md5(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def cus_of(ctx):
    return json.loads(ctx.describe_launch(4, 10, 65536, 8))["cus"]


# --------------------------------------------------------------------- (a)
def run_mul(ctx, form, k, rows, length, ns, stride, base, copies, seed):
    """One nxec_stripes_mul / _ptrs call on random data at a padded stride; returns nothing, asserts the
    whole output image."""
    rng = np.random.default_rng(seed)
    coeffs = km.coefficients(rows, k, seed)
    if form == "gather":
        nd = rows + 1  # one slot per stripe that no pointer names
        pool = rng.integers(0, 256, size=(ns * k * 2, stride), dtype=np.uint8)
        perm = rng.permutation(ns * k * 2)[: ns * k].reshape(ns, k)
        pb = up(pool)
        img = np.full((ns, nd, stride), EE, dtype=np.uint8)
        ob = up(img)
        sp = np.array([[pb.ptr + int(perm[s, j]) * stride for j in range(k)] for s in range(ns)], dtype=np.uint64)
        dp = np.array([[ob.ptr + (s * nd + rows - 1 - r) * stride for r in range(rows)] for s in range(ns)],
                      dtype=np.uint64)  # destination rows reversed
        spb, dpb = up(sp.view(np.uint8)), up(dp.view(np.uint8))
        ctx.stripes_mul_ptrs(coeffs, spb.ptr, dpb.ptr, length, ns)
        ctx.sync()
        got = ob.download().reshape(ns, nd, stride)
        for s in range(ns):
            w = oracle.matmul(coeffs, [pool[perm[s, j], :length] for j in range(k)])
            for r in range(rows):
                img[s, rows - 1 - r, :length] = w[r]
        bufs = (pb, ob, spb, dpb)
    else:
        nd = rows + copies + 1  # slot `copies` stays unselected
        src = rng.integers(0, 256, size=base + ns * k * stride + 16, dtype=np.uint8)
        sb = up(src)
        img = np.full(base + ns * nd * stride + 16, EE, dtype=np.uint8)
        ob = up(img)
        src_idx = list(reversed(range(k)))
        dst_idx = [nd - 1 - r for r in range(rows)]
        copy_idx = [-1] * k
        if copies:
            copy_idx[0] = 0
        if copies > 1:
            copy_idx[k - 1] = 1
        ctx.stripes_mul(coeffs, sb.ptr + base, ob.ptr + base, src_idx=src_idx, dst_idx=dst_idx if rows else None,
                        copy_idx=copy_idx if copies else None, src_chunk_stride=stride, src_stripe_stride=k * stride,
                        dst_chunk_stride=stride, dst_stripe_stride=nd * stride, length=length, nstripes=ns)
        ctx.sync()
        got = ob.download()
        sv = src[base: base + ns * k * stride].reshape(ns, k, stride)
        iv = img[base: base + ns * nd * stride].reshape(ns, nd, stride)
        for s in range(ns):
            if rows:
                w = oracle.matmul(coeffs, [sv[s, src_idx[j], :length] for j in range(k)])
                for r in range(rows):
                    iv[s, dst_idx[r], :length] = w[r]
            for j in range(k):
                if copy_idx[j] >= 0:
                    iv[s, copy_idx[j], :length] = sv[s, src_idx[j], :length]
        bufs = (sb, ob)
    for b in bufs:
        b.free()
    bad = np.flatnonzero(got.reshape(-1) != img.reshape(-1))
    assert bad.size == 0, (form, k, rows, "first differing output byte", int(bad[0]), "of", bad.size)


@pytest.mark.parametrize("case", km.a_cases(), ids=km.case_id)
def test_a_every_multiply_instantiation(gpu_ctx, case):
    nxec.launch_log_read()
    run_mul(gpu_ctx, case["form"], case["k"], case["rows"], case["length"], km.A_STRIPES, km.A_STRIDE, case["base"],
            km.a_copies(case), seed=1000 * case["k"] + 10 * case["rows"] + km.A_FORMS.index(case["form"]))
    take(km.a_plan(case))


# --------------------------------------------------------------------- (b)
def host_encode(coeffs, seed, ns, k, cs, src_of=None):
    """The device fill stream of a [ns][k][cs] buffer regenerated on the host (oracle.fill_bytes_at, the
    offset form of oracle.fill_bytes) and coeffs x the chunks of every stripe (oracle.simd_encode); source j
    of stripe s is chunk src_of(s, j) of that stripe.  Stripe ranges run on a few threads (both calls
    release the GIL): these shapes are hundreds of MiB.  Returns (data [ns][k][cs], rows [ns][rows][cs])."""
    from concurrent.futures import ThreadPoolExecutor
    rows = coeffs.shape[0]
    data = np.empty((ns, k, cs), dtype=np.uint8)
    want = np.empty((ns, rows, cs), dtype=np.uint8)

    def work(lo):
        hi = min(lo + step, ns)
        oracle.fill_bytes_at(data[lo:hi].reshape(-1), seed, lo * k * cs)
        for s in range(lo, hi):
            oracle.simd_encode(coeffs, [data[s, src_of(s, j) if src_of else j] for j in range(k)],
                               [want[s, r] for r in range(rows)])

    step = max(1, -(-ns // 16))
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(work, range(0, ns, step)))
    return data, want


def run_queue(ctx, form, k, rows, copies, cs, ns, seed, plan, cus=None, before_launch=None, wrong=None):
    """Complete tiles only, data filled on the device and regenerated on the host; the parity buffer is
    prefilled with 0xEE, so a skipped tile fails and a tile written twice with other data fails.  With a
    dict for `wrong`, the stripes whose row r differs are stored there as wrong[r] instead of failing."""
    coeffs = km.coefficients(rows, k, seed)
    nd = rows + copies
    src = nxec.DeviceBuffer(ns * k * cs)
    src.fill_random(seed)
    dst = nxec.DeviceBuffer(ns * nd * cs)
    dst.memset(EE)
    copy_idx = [-1] * k
    if copies:
        copy_idx[1], copy_idx[k - 1] = rows, rows + 1
    tabs = ()
    nxec.launch_log_read()
    if before_launch:
        before_launch()
    if form == "gather":  # chunk j of stripe s is pool chunk (j + s) % k of that stripe
        sp = np.array([[src.ptr + (s * k + (j + s) % k) * cs for j in range(k)] for s in range(ns)], dtype=np.uint64)
        dp = np.array([[dst.ptr + (s * nd + r) * cs for r in range(rows)] for s in range(ns)], dtype=np.uint64)
        tabs = (up(sp.view(np.uint8)), up(dp.view(np.uint8)))
        ctx.stripes_mul_ptrs(coeffs, tabs[0].ptr, tabs[1].ptr, cs, ns)
    else:
        ctx.stripes_mul(coeffs, src.ptr, dst.ptr, copy_idx=copy_idx if copies else None, src_chunk_stride=cs,
                        src_stripe_stride=k * cs, dst_chunk_stride=cs, dst_stripe_stride=nd * cs, length=cs,
                        nstripes=ns)
    ctx.sync()
    recs = take(plan)
    if cus is not None:  # one workgroup per CU, or the case does not reach the steady state it is about
        assert [r["grid"] for r in recs] == [cus] * len(recs), recs
    got = dst.download().reshape(ns, nd, cs)
    for b in (src, dst) + tabs:
        b.free()
    data, want = host_encode(coeffs, seed, ns, k, cs, (lambda s, j: (j + s) % k) if form == "gather" else None)
    for r in range(rows):
        bad = np.flatnonzero((got[:, r] != want[:, r]).any(axis=1))
        if wrong is not None:
            wrong[r] = bad.tolist()
            continue
        assert bad.size == 0, (form, k, rows, "row", r, "stripes with wrong or missing tiles", bad[:8], bad.size)
    for j in range(k):
        if copy_idx[j] >= 0:
            assert np.array_equal(got[:, copy_idx[j]], data[:, j]), (form, k, "copy of source", j)


@pytest.mark.parametrize("case", km.b_cases(), ids=km.case_id)
def test_b_queue_steady_state(gpu_ctx, case):
    cus = cus_of(gpu_ctx)
    plan = km.b_plan(case)
    assert len(plan) == 1
    if case["form"] == "strided" and case["rows"] == 1:  # the VALU kernel, but for the k the library keeps on LDS tables
        assert plan[0]["family"] == ("k_mul_vec" if case["k"] == 11 else "k_mul_perm")
    assert plan[0]["q"] == (0 if case["k"] == 20 else 1)
    run_queue(gpu_ctx, case["form"], case["k"], case["rows"], km.b_copies(case), km.B_CS, km.b_stripes(case, cus),
              km.b_seed(case), plan, cus)


def test_b_checker_sees_skipped_tiles(gpu_ctx):
    """Negative control: a launch whose queue counter starts at 5 (nxec_debug_poison_next_queue_slot) never
    runs tiles 0..4, and the steady-state check reports exactly the stripes those tiles belong to."""
    case = dict(form="strided", k=10, rows=4)
    cus = cus_of(gpu_ctx)
    assert km.b_plan(case)[0]["tpg"] == 1
    wrong = {}
    run_queue(gpu_ctx, "strided", 10, 4, 0, km.B_CS, km.b_stripes(case, cus), km.b_seed(case), km.b_plan(case), cus,
              before_launch=lambda: nxec.check(lib.nxec_debug_poison_next_queue_slot(5), "poison"), wrong=wrong)
    assert wrong == {r: [0, 1] for r in range(4)}  # tiles 0..4 = stripe 0 and the first tile of stripe 1


# --------------------------------------------------------------------- (c)
@pytest.mark.parametrize("ns", km.C_STRIPES)
def test_c_stripe_group_tile_order(gpu_ctx, ns):
    """Gather form, 2 MiB + 4 KiB chunks: tiles run column-major inside groups of 8 stripes, the last group partial."""
    plan = km.mul_launches(2, 1, km.C_CS, gather=True)
    assert [p["sg"] for p in plan] == [8] * len(plan) and plan[0]["family"] == "k_mul_perm"
    run_queue(gpu_ctx, "gather", 2, 1, 0, km.C_CS, ns, 4400 + ns, plan)


# --------------------------------------------------------------------- (d)
def scrub_batch(n, k, length, stride, ns, seed, slots=None):
    """Host image [ns][slots or n][stride] of oracle-encoded stripes (random bytes in the stride padding and
    in the slots past chunk n - 1)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(ns, slots or n, stride), dtype=np.uint8)
    for s in range(ns):
        img[s, :n, :length] = oracle.rs_encode(n, k, img[s, :k, :length].reshape(-1), length)
    return img


@pytest.mark.parametrize("kd,rows", km.d_cases())
def test_d_scrub_detect_every_instantiation(gpu_ctx, kd, rows):
    n, length, stride, ns = kd + rows, km.D_LEN, km.D_STRIDE, km.D_STRIPES
    clean, unloc = nxec.SCRUB_CLEAN, nxec.SCRUB_UNLOCATED
    img = scrub_batch(n, kd, length, stride, ns, 500 + 10 * kd + rows)
    buf = up(img)
    plan = km.scrub_launches(kd, rows, length, stride)
    assert [p["full"] for p in plan] == [1, 0]
    for flags in (0, nxec.SCRUB_LOCATE):
        nxec.launch_log_read()
        st, nbad = gpu_ctx.rs_scrub(n, kd, buf.ptr, stride, n * stride, length, ns, flags)
        take(plan)
        assert st.tolist() == [clean] * ns and nbad == 0, (flags, st, nbad)
    flip = 0
    for c in km.d_flip_chunks(kd, rows):
        for pos in km.D_FLIP_POS:
            s = flip % ns
            flip += 1
            at = (s * n + c) * stride + pos
            buf.upload(np.array([img[s, c, pos] ^ (1 << (flip % 8))], dtype=np.uint8), at)
            for flags in (0, nxec.SCRUB_LOCATE):
                st, nbad = gpu_ctx.rs_scrub(n, kd, buf.ptr, stride, n * stride, length, ns, flags)
                want = [clean] * ns
                want[s] = c if (flags and rows >= 2) else unloc
                assert st.tolist() == want and nbad == 1, (c, pos, flags, st, nbad)
            buf.upload(img[s, c, pos: pos + 1], at)
    note(nxec.launch_log_read())
    st, nbad = gpu_ctx.rs_scrub(n, kd, buf.ptr, stride, n * stride, length, ns, nxec.SCRUB_LOCATE)
    assert st.tolist() == [clean] * ns and nbad == 0  # every flip was put back
    assert np.array_equal(buf.download().reshape(img.shape), img)  # detect and locate write nothing
    buf.free()


@pytest.mark.parametrize("kd,rows", km.d_queue_cases())
def test_d_scrub_queue_steady_state(gpu_ctx, kd, rows):
    """Complete tiles, >= 4 * cus * T of them, on each side of the scrub kernel's prefetch boundary.  A tile
    the queue skipped would hide corruption: run t flips one byte in tile (s + t) % 4 of every stripe s, so
    over the four runs every tile of every stripe is the only corrupt one of its stripe once."""
    cus = cus_of(gpu_ctx)
    n, cs = kd + rows, km.B_CS
    tps = cs // km.TILE
    ns = -(-4 * cus * km.tiles_per_grab(kd, rows) // tps)
    plan = km.scrub_launches(kd, rows, cs, cs)
    assert len(plan) == 1 and plan[0]["pf"] == int(kd + rows <= km.PREFETCH_MAX_K)
    seed = 8800 + kd
    data, par = host_encode(oracle.gen_rs_matrix(n, kd)[kd:], seed, ns, kd, cs)
    img = np.concatenate([data, par], axis=1)
    buf = up(img)
    nxec.launch_log_read()
    st, nbad = gpu_ctx.rs_scrub(n, kd, buf.ptr, cs, n * cs, cs, ns, 0)
    recs = take(plan)
    assert recs[0]["grid"] == cus
    assert (st == nxec.SCRUB_CLEAN).all() and nbad == 0
    flat = img.reshape(-1)

    def poke(where, values):  # one byte each, one wait for all of them
        for w, v in zip(where, values):
            nxec.check(lib.nxec_memcpy_h2d(buf.addr(w), C.c_void_p(v.ctypes.data), 1, None), "h2d")
        nxec.check(lib.nxec_stream_sync(None), "sync")

    for t in range(tps):
        where = [((s * n + (s + t) % n) * cs + ((s + t) % tps) * km.TILE + (37 * s + t) % km.TILE) for s in range(ns)]
        poke(where, list((flat[where] ^ 0x10).reshape(-1, 1)))
        st, nbad = gpu_ctx.rs_scrub(n, kd, buf.ptr, cs, n * cs, cs, ns, 0)
        missed = np.flatnonzero(st != nxec.SCRUB_UNLOCATED)
        assert missed.size == 0 and nbad == ns, (t, "stripes whose corrupt tile was not scanned", missed[:8], nbad)
        poke(where, list(flat[where].reshape(-1, 1)))
    note(nxec.launch_log_read())
    buf.free()


# --------------------------------------------------------------------- (e)
@pytest.mark.parametrize("k", range(1, km.MUL_MD5_MAX_K + 1))
def test_e_mul_md5(gpu_ctx, k):
    """k_mul_md5<K, HSRC>: rs_encode_md5 hashes sources and parity, rs_recover_md5 the rebuilt chunks only."""
    p, cs, ns = km.e_p(k), km.E_CS, km.E_STRIPES
    n = k + p
    rng = np.random.default_rng(600 + k)
    want = np.empty((ns, n, cs), dtype=np.uint8)
    for s in range(ns):
        want[s] = oracle.rs_encode(n, k, rng.integers(0, 256, size=k * cs, dtype=np.uint8), cs)
    dig_want = np.stack([np.stack([md5(want[s, c]) for c in range(n)]) for s in range(ns)])
    img = want.copy()
    img[:, k:] = EE
    buf = up(img)
    dig = nxec.DeviceBuffer(ns * n * 16 + 16)
    dig.memset(EE)
    nxec.launch_log_read()
    gpu_ctx.rs_encode_md5(n, k, buf.ptr, cs, n * cs, cs, ns, dig.ptr)
    gpu_ctx.sync()
    take([dict(family="k_mul_md5", k=k, p=p, hsrc=1, hdst=1, product=1)])
    assert np.array_equal(buf.download().reshape(want.shape), want)
    d = dig.download()
    assert np.array_equal(d[: ns * n * 16].reshape(ns, n, 16), dig_want) and (d[ns * n * 16:] == EE).all()
    # recover: p chunks (data and parity) erased
    failed = sorted(list(dict.fromkeys([0, n - 1, k, k - 1, 1, 2]))[:p]) if p > 1 else [k // 2]
    assert len(failed) == p
    img = want.copy()
    img[:, failed] = EE
    buf.upload(img)
    dig.memset(EE)
    gpu_ctx.rs_recover_md5(n, k, failed, buf.ptr, cs, n * cs, cs, ns, dig.ptr)
    gpu_ctx.sync()
    take([dict(family="k_mul_md5", k=k, p=p, hsrc=0, hdst=1, product=1)])
    assert np.array_equal(buf.download().reshape(want.shape), want)
    d = dig.download()
    assert np.array_equal(d[: ns * p * 16].reshape(ns, p, 16), dig_want[:, failed]) and (d[ns * p * 16:] == EE).all()
    buf.free()
    dig.free()


class Arena:
    """nxec_host_alloc blocks (pinned, device-mapped) viewed as numpy arrays."""

    def __init__(self):
        self.blocks = []

    def array(self, nbytes):
        p = C.c_void_p()
        nxec.check(lib.nxec_host_alloc(nbytes, C.byref(p)), "nxec_host_alloc")
        self.blocks.append(p.value)
        return np.ctypeslib.as_array((C.c_ubyte * nbytes).from_address(p.value))

    def free(self):
        for b in self.blocks:
            lib.nxec_host_free(C.c_void_p(b))
        self.blocks = []


@pytest.mark.parametrize("hsrc", [0, 1])
@pytest.mark.parametrize("k", range(1, km.GATHER_MD5_MAX_K + 1))
def test_e_gather_md5(gpu_ctx, k, hsrc):
    """k_gather_md5<K, HSRC> through nxec_agent_encode_batch on pinned buffers: five requests of one matrix,
    chunks of three whole 256-byte steps and a partial one; HSRC when the request asks for its inputs' digests."""
    p, cs, nreq = km.e_p(k), 3 * 256 + 232, 5
    rng = np.random.default_rng(700 + k)
    m = km.coefficients(p, k, 700 + k)
    arena = Arena()
    try:
        reqs, bigs = [], []
        for r in range(nreq):
            ins = []
            for j in range(k):
                a = arena.array(cs)
                a[:] = rng.integers(0, 256, size=cs, dtype=np.uint8)
                ins.append(a)
            big = [arena.array(cs + 64) for _ in range(p)]
            for b in big:
                b[:] = EE
            bigs.append(big)
            reqs.append((m, ins, [b[:cs] for b in big], np.full((p, 16), EE, dtype=np.uint8),
                         np.full((k, 16), EE, dtype=np.uint8) if hsrc else None))
        nxec.launch_log_read()
        gpu_ctx.agent_encode_batch(reqs, cs)
        take([dict(family="k_gather_md5", k=k, p=p, hsrc=hsrc)])
        for r, (req, big) in enumerate(zip(reqs, bigs)):
            w = oracle.matmul(m, [x.copy() for x in req[1]])
            for o in range(p):
                assert np.array_equal(big[o][:cs], w[o]), (r, o)
                assert (big[o][cs:] == EE).all(), (r, o)
                assert np.array_equal(req[3][o], md5(w[o])), (r, o)
            if hsrc:
                for j in range(k):
                    assert np.array_equal(req[4][j], md5(req[1][j])), (r, j)
    finally:
        arena.free()


def run_objects(ctx, n, k, M, lengths, misalign, flags, seed, with_md5=True):
    """nxec_encode_objects on tiny objects; every parity chunk against a per-object oracle encode, every
    digest against hashlib, the tail arena against the zero-padded last-stripe chunks.  Returns the record."""
    p = n - k
    rng = np.random.default_rng(seed)
    offs, pos = [], 0
    for L in lengths:
        offs.append(pos + misalign)
        pos += km.rup(L + misalign) + 16
    host = rng.integers(0, 256, size=pos + 4096, dtype=np.uint8)
    arena = up(host)
    total, tail_bytes = nxec.objects_layout(n, k, lengths, M)
    par = nxec.DeviceBuffer(total * p * M)
    par.memset(EE)
    tail = nxec.DeviceBuffer(max(tail_bytes, 16) + 16)
    tail.memset(EE)
    dg = nxec.DeviceBuffer(total * n * 16 + 16)
    dg.memset(EE)
    nxec.launch_log_read()
    ctx.encode_objects(n, k, [arena.ptr + o for o in offs], lengths, M, par.ptr, tail.ptr, dg.ptr if with_md5 else None,
                       flags=flags)
    ctx.sync()
    recs = note(nxec.launch_log_read())
    gp = par.download().reshape(total, p, M)
    gt = tail.download()
    gd = dg.download()
    for b in (arena, par, tail, dg):
        b.free()
    assert (gt[tail_bytes:] == EE).all() and (gd[total * n * 16:] == EE).all()
    gd = gd[: total * n * 16].reshape(total, n, 16)
    g, toff = 0, 0
    for i, (o, L) in enumerate(zip(offs, lengths)):
        ns, nf, cl = nxec.object_layout(n, k, L, M)
        for s in range(ns):
            cs = M if s < nf else cl
            sd = np.zeros(k * cs, dtype=np.uint8)
            piece = host[o + s * k * M: o + min(L, s * k * M + k * cs)]
            sd[: len(piece)] = piece
            st = oracle.rs_encode(n, k, sd, cs)
            for r in range(p):
                assert np.array_equal(gp[g + s, r, :cs], st[k + r]), (i, s, r)
                assert (gp[g + s, r, km.rup(cs):] == EE).all(), (i, s, r)  # outputs are whole 16-byte vectors
            if with_md5:
                for c in range(n):
                    assert np.array_equal(gd[g + s, c], md5(st[c])), (i, s, c)
            if s >= nf:
                cls = km.rup(cl)
                slots = gt[toff: toff + k * cls].reshape(k, cls)
                rem = L - nf * k * M
                for j in range(k):
                    partial = j == rem // cl and rem % cl
                    if flags & nxec.OBJECTS_TAIL_INPLACE and not partial and (slots[j] == EE).all():
                        continue  # only the partial chunk has to be in the arena
                    assert np.array_equal(slots[j, :cl], st[j]) and not slots[j, cl:].any(), (i, j)
                toff += k * cls
        g += ns
    return recs


def files_only(recs):
    mine = [r for r in recs if r["family"] == "k_files_md5"]
    assert all(r["product"] == 1 for r in mine), mine
    return mine


@pytest.mark.parametrize("k", range(1, km.FILES_MD5_MAX_K + 1))
def test_e_files_md5(gpu_ctx, k):
    """k_files_md5<K, MASK, TSTORE>: aligned objects of whole stripes (plain), objects with ragged last
    stripes (masked chunks + whole tail arena), the same with OBJECTS_TAIL_INPLACE (masked chunks)."""
    p, M = km.e_p(k), 512
    n = k + p
    whole = [k * M, 2 * k * M, k * M]
    ragged = [k * M + (k * 48 - 1 if k > 1 else 47), 2 * k * M, k * 48 - 1 if k > 1 else 31, 5, k * M + k * 256,
              k * 100 + 3]
    recs = run_objects(gpu_ctx, n, k, M, whole, 0, 0, 800 + k)
    assert [km.inst_of(r) for r in files_only(recs)] == [("k_files_md5", k, 0, 0)] and len(recs) == 1, recs
    recs = run_objects(gpu_ctx, n, k, M, ragged, 0, 0, 820 + k)
    assert [km.inst_of(r) for r in files_only(recs)] == [("k_files_md5", k, 1, 1)], recs
    recs = run_objects(gpu_ctx, n, k, M, ragged, 0, nxec.OBJECTS_TAIL_INPLACE, 840 + k)
    # k = 1: the last stripe's only chunk is never partial, so no request masks a chunk (kernel_matrix.UNREACHABLE)
    assert [km.inst_of(r) for r in files_only(recs)] == [("k_files_md5", k, int(k > 1), 0)], recs


@pytest.mark.parametrize("k", range(1, km.RAGGED_MAX_K + 2))
def test_e_ragged_launch(gpu_ctx, k):
    """k_mul_ragged<K>: the last stripes of objects that take the separate launches -- misaligned objects
    (even k) or five parity rows (odd k: two passes); k = 20 has no ragged kernel and falls back to k_mul_list."""
    p, M = (2 if k % 2 == 0 else 5), km.TILE + 1024
    n = k + p
    # last stripes of two tiles (chunks of 16500 bytes), of one vector, of 7, 3 and 498 bytes per chunk or fewer
    lengths = [k * M + k * 16500 - 1, k * 64, 2 * k * M + 7, 3, k * 500 - 2]
    recs = run_objects(gpu_ctx, n, k, M, lengths, 3 if k % 2 == 0 else 0, 0, 900 + k)
    rag = [r for r in recs if r["family"] == "k_mul_ragged"]
    lst = [r for r in recs if r["family"] == "k_mul_list"]
    assert not files_only(recs), recs
    if k > km.RAGGED_MAX_K:
        assert not rag and lst, recs
        return
    want = [dict(family="k_mul_ragged", k=k, rows=min(p - r0, km.MAX_ROWS), r=km.default_r(k),
                 pf=int(k <= km.PREFETCH_MAX_K_COPY), q=1, tpg=km.tiles_per_grab(k, min(p - r0, km.MAX_ROWS)))
            for r0 in range(0, p, km.MAX_ROWS)]
    assert len(rag) == len(want) and all(km.matches(r, w) for r, w in zip(rag, want)), (rag, want)
    assert bool(lst) == (k % 2 == 0), recs  # misaligned objects: their full stripes through the list kernel


# --------------------------------------------------------------- (f), (g)
def first_difference(got, want, ns, tag, wrong=None):
    """Whole-image comparison of two [ns][...] arrays: fails naming the wrong stripes and the first differing
    byte, or, with a list for `wrong`, stores the wrong stripes there instead."""
    if wrong is None and got.shape == want.shape and got.nbytes % 8 == 0:  # the usual outcome, eight bytes at a time
        if np.array_equal(got.reshape(-1).view(np.uint64), want.reshape(-1).view(np.uint64)):
            return
    ne = (got != want).reshape(ns, -1)
    bad = np.flatnonzero(ne.any(axis=1))
    if wrong is not None:
        wrong += bad.tolist()
    if wrong is not None or bad.size == 0:
        return
    s = int(bad[0])
    pytest.fail(f"{tag}: {bad.size} wrong stripes {bad[:8].tolist()}, first differing byte in stripe {s} at stripe "
                f"byte {int(np.flatnonzero(ne[s])[0])} (stripe shape {got.shape[1:]})")


def run_mixed(ctx, decode, n, k, truth, length, sets, out_slots=None, out_stride=None, cus=None, before_launch=None,
              wrong=None):
    """One nxec_rs_recover_stripes_mixed / nxec_rs_decode_stripes_mixed call over the host image `truth`
    [ns][slots >= n][chunk stride] of oracle-encoded stripes, stripe s erased at sets[s].  The image is
    uploaded and the erased chunks alone are overwritten on the device, with garbage that differs from the
    truth in every byte.  Recover: the whole buffer comes back as the truth, but a stripe with a negative
    verdict keeps its garbage.  Decode: the output, prefilled with km.sentinel_bytes, holds the original data
    chunks of every stripe with a verdict >= 0 and the sentinel everywhere else; the source is unchanged.
    Verdicts, segments and stripes are the Python model's (km.mixed_model), the one launch km.mixed_launch's.
    `truth` is used up: the garbage the device must still hold is written into it before the comparison."""
    ns, slots, cs = truth.shape
    mode = km.MIXED_MODES[decode]
    model = km.mixed_model(n, k, sets, decode)
    verdict = np.array(model["verdict"])
    alive = np.ones((ns, n), dtype=np.uint8)
    mask = np.random.default_rng(31 * k + decode).integers(1, 256, size=length, dtype=np.uint8)  # no zero byte
    by_set = {}
    for s, e in enumerate(sets):
        by_set.setdefault(tuple(e), []).append(s)
    src = up(truth)
    junk = {}  # erased set -> the garbage of its stripes' erased chunks, [stripes][chunks][length]
    for e, idx in by_set.items():
        if e:
            alive[np.ix_(idx, e)] = 0
            junk[e] = j = truth[np.ix_(idx, e)][:, :, :length] ^ mask
            for a, s in enumerate(idx):
                for b, c in enumerate(e):  # one wait for all of them, below
                    nxec.check(lib.nxec_memcpy_h2d(src.addr((s * slots + c) * cs),
                                                   C.c_void_p(j.ctypes.data + (a * len(e) + b) * length), length, None), "h2d")
    nxec.check(lib.nxec_stream_sync(None), "sync")

    def keep_garbage(keep):  # keep: one bool per stripe
        for e, j in junk.items():
            idx = np.array(by_set[e])
            sel = keep[idx]
            for b, c in enumerate(e):
                truth[idx[sel], c, :length] = j[sel, b]

    out = None
    if decode:
        oslots, ocs = out_slots or k, out_stride or cs
        blank = km.sentinel_bytes(ns * oslots * ocs).reshape(ns, oslots, ocs)
        out = up(blank)
    nxec.launch_log_read()
    if before_launch:
        before_launch()
    if decode:
        res = ctx.rs_decode_mixed(n, k, alive, src.ptr, cs, slots * cs, out.ptr, ocs, oslots * ocs, length, ns)
    else:
        res = ctx.rs_recover_mixed(n, k, alive, src.ptr, cs, slots * cs, length, ns)
    ctx.sync()
    recs = note(nxec.launch_log_read())
    got = src.download().reshape(truth.shape)
    got_out = out.download().reshape(blank.shape) if decode else None
    src.free()
    if decode:
        out.free()
    assert res.tolist() == model["verdict"], (mode, k, res.tolist(), model["verdict"])
    plan = dict(km.mixed_launch(k, decode), segs=model["segs"], stripes=model["stripes"])
    assert len(recs) == 1 and km.matches(recs[0], plan), (recs, plan)
    if cus is not None:  # one workgroup per CU and >= 4 grabs each, or the case does not reach the steady state
        m = recs[0]
        assert m["grid"] == cus and ns * (-(-length // km.TILE)) >= 4 * m["grid"] * m["tpg"], (m, ns)
    if decode:
        np.copyto(blank[:, :k, :length], truth[:, :k, :length], where=(verdict >= 0)[:, None, None])
        first_difference(got_out, blank, ns, (mode, k, "output"), wrong)
        keep_garbage(np.ones(ns, dtype=bool))
        first_difference(got, truth, ns, (mode, k, "the source was written"))
    else:
        keep_garbage(verdict < 0)  # a LOST stripe is left as it was
        first_difference(got, truth, ns, (mode, k, "batch"), wrong)


@pytest.mark.parametrize("mode,k", km.f_cases(), ids=lambda v: str(v))
def test_f_every_mixed_instantiation(gpu_ctx, mode, k):
    """k_mul_mixed<K> / k_decode_mixed<K> for every K: a complete tile and a tile of 3 vectors, padded chunk
    and stripe strides with random bytes in the padding, every chunk the only target once, segments of 4, 1,
    2 and 3 rows in a row, plans of two segments, one LOST stripe."""
    decode = mode == "decode"
    n = k + km.MIXED_EXTRA
    sets = km.f_sets(k, decode)
    truth = scrub_batch(n, k, km.F_LEN, km.F_STRIDE, len(sets), 1200 + 10 * k + decode, slots=n + 1)
    run_mixed(gpu_ctx, decode, n, k, truth, km.F_LEN, sets, out_slots=k + 1, out_stride=km.F_OUT_STRIDE)


def g_batch(k, decode, cus):
    """(n, truth [ns][n][G_CS], sets).  The truth as host_encode makes it, but in one [ns][n] image: the data
    chunks of stripe s are the fill stream from byte s * k * cs on (oracle.fill_bytes_at), its parity is the
    generator's parity rows x those chunks (oracle.simd_encode); stripe ranges run on a few threads."""
    from concurrent.futures import ThreadPoolExecutor
    n, cs, seed = k + km.MIXED_EXTRA, km.G_CS, km.g_seed(k, decode)
    ns = km.g_stripes(k, decode, cus)
    enc = oracle.gen_rs_matrix(n, k)[k:]
    truth = np.empty((ns, n, cs), dtype=np.uint8)

    def work(lo):
        for s in range(lo, min(lo + step, ns)):
            oracle.fill_bytes_at(truth[s, :k].reshape(-1), seed, s * k * cs)
            oracle.simd_encode(enc, [truth[s, j] for j in range(k)], [truth[s, k + r] for r in range(n - k)])

    step = max(1, -(-ns // 16))
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(work, range(0, ns, step)))
    pats = km.g_sets(k)
    return n, truth, [pats[s % len(pats)] for s in range(ns)]


@pytest.mark.parametrize("mode,k", km.g_cases(), ids=lambda v: str(v))
def test_g_mixed_steady_state(gpu_ctx, mode, k):
    """>= 4 * cus * T one-tile stripes whose patterns interleave (km.g_sets): most tiles come from published
    grabs, and a workgroup's next tile is nearly always of another segment than the resident one -- under
    prefetch (k <= 8), after a 4-row segment, in the second segment of a plan, across the decode's pure copies."""
    decode = mode == "decode"
    cus = cus_of(gpu_ctx)
    n, truth, sets = g_batch(k, decode, cus)
    run_mixed(gpu_ctx, decode, n, k, truth, km.G_CS, sets, cus=cus)


def test_g_checker_sees_skipped_tiles(gpu_ctx):
    """Negative control: a launch whose queue counter starts at 5 (nxec_debug_poison_next_queue_slot) never
    runs items 0..4 (one tile each, one tile per grab at k = 9), and the steady-state check reports exactly
    their stripes."""
    k, cus = km.UPDATE_MAX_K16, cus_of(gpu_ctx)
    assert km.mixed_launch(k, False)["tpg"] == 1
    n, truth, sets = g_batch(k, False, cus)
    wrong = []
    run_mixed(gpu_ctx, False, n, k, truth, km.G_CS, sets, cus=cus, wrong=wrong,
              before_launch=lambda: nxec.check(lib.nxec_debug_poison_next_queue_slot(5), "poison"))
    assert wrong == sorted(km.mixed_model(n, k, sets, False)["order"][:5]) and len(set(wrong)) == 5


# --------------------------------------------------------------------- (h)
@pytest.mark.parametrize("k", range(1, km.RAGGED_MAX_K + 1))
def test_h_update_every_k(gpu_ctx, k):
    """k_update_vec<16> (k <= 9) and <8> with the LDS of every k: stripe s updates chunk s, so every table
    of the k, the last one right under the queue ring included, multiplies once; 1 to 6 parity rows."""
    n, length, cs, ns = k + km.h_p(k), km.F_LEN, km.F_STRIDE, k + 1
    img = scrub_batch(n, k, length, cs, ns, 1300 + k)
    specs = km.h_specs(k)
    new = np.random.default_rng(1400 + k).integers(0, 256, size=km.h_new_offset(len(specs)), dtype=np.uint8)
    want = img.copy()
    for i, (s, c, off, ln) in enumerate(specs):
        want[s, c, off: off + ln] = new[km.h_new_offset(i): km.h_new_offset(i) + ln]
        want[s, :, :length] = oracle.rs_encode(n, k, want[s, :k, :length].reshape(-1), length)
    buf, nb = up(img), up(new)
    nxec.launch_log_read()
    gpu_ctx.rs_update(n, k, buf.ptr, cs, n * cs, length, ns,
                      [(s, c, off, ln, nb.ptr + km.h_new_offset(i)) for i, (s, c, off, ln) in enumerate(specs)])
    gpu_ctx.sync()
    take(km.h_plan(k, buf.ptr, nb.ptr))
    got, new_after = buf.download().reshape(img.shape), nb.download()
    buf.free()
    nb.free()
    first_difference(got, want, ns, ("update", k))
    assert np.array_equal(new_after, new), (k, "d_new was written")


# ---------------------------------------------------------------- complete
def test_z_every_instantiation_was_launched():
    """The union of the instantiations recorded above is the whole expected set (needs the whole module)."""
    want = km.expected_instantiations()
    assert not (want - SEEN), ("never launched", sorted(want - SEEN))
    assert not (SEEN - want), ("launched but not in the expected set", sorted(SEEN - want))
    print(f"kernel matrix: {len(SEEN)} instantiations launched = the expected set")
