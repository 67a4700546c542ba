"""Mixed-pattern decode on the GPU (nxec_rs_decode_stripes_mixed,
nxec_decode_object_mixed): every stripe of a batch is decoded around its own
erased chunks into a separate output.

Method: encode a fill_random batch and keep its host copy as truth; overwrite
every erased chunk with fresh garbage; fill the output with a sentinel byte
pattern; call; download the output whole.  It must equal the original data
chunks wherever result >= 0 and the sentinel everywhere else (output padding,
LOST and SINGULAR stripes); the source must be unchanged; result must be the
CPU plan's; the launch record must show exactly one k_decode_mixed line with
the plan's segs and stripes, or only by-runs families.

Shapes, the smallest that reach each way the kernel can go wrong:
  geometry (6,4)    prefetch instantiation
           (14,10)  four rows, R = 8
           (12,6)   five lost data chunks (two segments, copies once), the
                    singular sets, a parity-only loss
           (10,4)   5 and 6 erased chunks: <= 4 targets, many masks one plan
           (23,19)  the widest instantiation
           (24,21)  k > 19: the by-runs path
  len      16 (one vector), 16384 (one full tile), 16384 + 16, 3 * 16384 + 48;
           4096 + 5 reaches the by-runs path through its tail, a source base
           offset of 3 and an output base offset of 3
  layouts  source and output each packed, chunk stride len + 48, stripe
           padded by one chunk
"""
import ctypes as C
import itertools
import json

import numpy as np
import pytest

from nexoedge_amd import _lib, nxec

pytestmark = pytest.mark.gpu

LOST, SINGULAR = nxec.RECOVER_LOST, nxec.RECOVER_SINGULAR
TILE = 16384
LENS = [16, 16384, 16384 + 16, 3 * 16384 + 48]
BY_RUNS = ("k_mul_vec", "k_mul_perm", "k_mul_bytes", "k_mul_vec_dyn")
MAX_K = 19  # the widest k_decode_mixed instantiation


def rup(x, m=16):
    return (x + m - 1) // m * m


def layouts(chunks, length):
    """(chunk stride, stripe stride): packed, padded chunks, stripes padded by one chunk"""
    return [(length, chunks * length), (length + 48, chunks * (length + 48)), (length, (chunks + 1) * length)]


def alive_of(n, sets):
    a = np.ones((len(sets), n), dtype=np.uint8)
    for s, e in enumerate(sets):
        a[s, list(e)] = 0
    return a


@pytest.fixture(scope="module", autouse=True)
def launch_record():
    nxec.launch_log(True)
    yield
    nxec.launch_log(False)


def sentinel(nbytes):
    return ((np.arange(nbytes, dtype=np.uint32) * 7 + 0x5A) % 251).astype(np.uint8)


class Source:
    """An encoded [ns][n] batch on the device and its host copy (truth)."""

    def __init__(self, ctx, n, k, length, ns, off=0, cs=None, ss=None, seed=3):
        self.ctx, self.n, self.k, self.len, self.ns, self.off = ctx, n, k, length, ns, off
        self.cs = cs if cs is not None else length
        self.ss = ss if ss is not None else n * self.cs
        self.buf = nxec.DeviceBuffer(off + ns * self.ss + 16)
        self.buf.fill_random(seed + 977 * n + length)
        ctx.rs_encode(n, k, self.buf.ptr + off, self.cs, self.ss, length, ns)
        ctx.sync()
        self.truth = self.buf.download()

    def free(self):
        self.buf.free()

    def at(self, s, c):
        return self.off + s * self.ss + c * self.cs

    def erase(self, alive, seed=5):
        """Garbage into every erased chunk, on the device; returns the host image of the damaged buffer."""
        rng = np.random.default_rng(seed)
        cur = self.truth.copy()
        for s, c in zip(*np.nonzero(np.asarray(alive).reshape(self.ns, self.n) == 0)):
            junk = rng.integers(0, 256, self.len, dtype=np.uint8)
            junk[0] = self.truth[self.at(s, c)] ^ 0xA5  # differs from the original for sure
            cur[self.at(s, c): self.at(s, c) + self.len] = junk
        self.buf.upload(cur)
        return cur


class Output:
    """The output buffer under a sentinel pattern."""

    def __init__(self, src, off=0, ocs=None, oss=None):
        self.src, self.off = src, off
        self.ocs = ocs if ocs is not None else src.len
        self.oss = oss if oss is not None else src.k * self.ocs
        self.buf = nxec.DeviceBuffer(off + src.ns * self.oss + 16)
        self.blank = sentinel(self.buf.nbytes)

    def free(self):
        self.buf.free()

    def reset(self):
        self.buf.upload(self.blank)

    def expected(self, result):
        """the sentinel, but the k data chunks of every stripe with result >= 0 are the originals"""
        b, want = self.src, self.blank.copy()
        for s in np.flatnonzero(np.asarray(result) >= 0):
            for j in range(b.k):
                o = self.off + s * self.oss + j * self.ocs
                want[o: o + b.len] = b.truth[b.at(s, j): b.at(s, j) + b.len]
        return want

    def decode(self, alive, stream=None):
        b = self.src
        return b.ctx.rs_decode_mixed(b.n, b.k, alive, b.buf.ptr + b.off, b.cs, b.ss, self.buf.ptr + self.off, self.ocs,
                                     self.oss, b.len, b.ns, stream)


def one_launch_shape(b, o):
    return (b.k <= MAX_K and b.len % 16 == 0 and b.off % 16 == 0 and o.off % 16 == 0 and
            all(x % 16 == 0 for x in (b.cs, b.ss, o.ocs, o.oss)))


def check(b, o, alive, tag):
    """Damage, decode, compare the whole output, the source and the verdicts; returns the call's launch records."""
    alive = np.ascontiguousarray(alive, dtype=np.uint8)
    want_res, nplans, nseg, ndec = nxec.rs_decode_mixed_plan(b.n, b.k, alive)
    damaged = b.erase(alive)
    o.reset()
    nxec.launch_log_read()
    res = o.decode(alive)
    b.ctx.sync()
    recs = nxec.launch_log_read()
    got = o.buf.download()
    assert np.array_equal(res, want_res), (tag, res, want_res)
    want = o.expected(want_res)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        first = int(bad[0]) - o.off
        pytest.fail(f"{tag}: {bad.size} output bytes differ, first in stripe {first // o.oss} at stripe byte "
                    f"{first % o.oss} (out chunk stride {o.ocs}, len {b.len})")
    assert np.array_equal(b.buf.download(), damaged), (tag, "the source was written")
    mixed = [r for r in recs if r["family"] == "k_decode_mixed"]
    if ndec == 0 or b.len == 0:
        assert recs == [], (tag, recs)
    elif one_launch_shape(b, o):
        assert len(mixed) == 1 and len(recs) == 1, (tag, recs)
        m = mixed[0]
        assert (m["k"], m["rows"], m["q"], m["segs"], m["stripes"]) == (b.k, 4, 1, nseg, ndec), (tag, m)
        assert m["pf"] == int(b.k <= 8) and m["r"] == (16 if b.k <= 9 else 8), (tag, m)
    else:
        assert not mixed and recs and all(r["family"] in BY_RUNS for r in recs), (tag, recs)
    return recs


def pattern_sets(n, k):
    """The stripes of the mixed recover's test (clean, single, scattered, full n-k, geometry specials, lost),
    plus clean stripes repeated so that clean items dominate one segment."""
    m = n - k
    sets = [(), (0,), (n - 1,), tuple(range(m)), tuple(range(n - m, n)), (1, k)[:m], tuple(range(0, n, 2))[:m]]
    if (n, k) == (10, 4):
        sets += [(0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 9), (2, 4, 5, 6, 8, 9), (0, 1, 2, 3, 4)]  # 5 and 6 erased, <= 4 targets
    if (n, k) == (12, 6):
        # the first two are singular; the last loses five data chunks: two segments, copies once
        sets += [(0, 2, 5, 7, 8), (0, 3, 5, 8, 9), (0, 2, 5, 7, 9), (1, 2, 3, 4, 5, 6)]
    sets += [tuple(range(m + 1)), tuple(range(n))]  # lost
    return sets + [()] * 6


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("n,k", [(6, 4), (14, 10), (10, 4), (12, 6), (23, 19), (24, 21)])
def test_geometries(gpu_ctx, n, k, length):
    sets = pattern_sets(n, k)
    if (n, k) == (12, 6):
        res, _, nseg, _ = nxec.rs_decode_mixed_plan(n, k, alive_of(n, sets))
        assert res[sets.index((0, 2, 5, 7, 8))] == SINGULAR and res[sets.index((1, 2, 3, 4, 5, 6))] == 5
        assert res[sets.index(tuple(range(6, 12)))] == 0  # parity-only loss
    if (n, k) == (10, 4):
        res, nplans, _, ndec = nxec.rs_decode_mixed_plan(n, k, alive_of(n, sets))
        assert res.max() == 4 and nplans < ndec - 6  # many masks share a plan
    src_layouts, out_layouts = layouts(n, length), layouts(k, length)
    for i, (cs, ss) in enumerate(src_layouts):
        b = Source(gpu_ctx, n, k, length, len(sets), cs=cs, ss=ss)
        try:
            for ocs, oss in (out_layouts[i], out_layouts[(i + 1) % 3]):
                o = Output(b, ocs=ocs, oss=oss)
                try:
                    check(b, o, alive_of(n, sets), (n, k, length, cs, ss, ocs, oss))
                finally:
                    o.free()
        finally:
            b.free()
    # 1 and 5 stripes, every stripe with a loss
    for ns in (1, 5):
        b = Source(gpu_ctx, n, k, length, ns, cs=length + 48)
        o = Output(b, ocs=length + 48)
        try:
            some = [e for e in sets if 0 < len(e) <= n - k][:ns]
            check(b, o, alive_of(n, (some * ns)[:ns]), (n, k, length, ns))
        finally:
            o.free()
            b.free()


@pytest.mark.parametrize("n,k", [(6, 4), (14, 10)])
def test_all_clean_batch_is_one_pure_copy_launch(gpu_ctx, n, k):
    length, ns = 16384 + 16, 5
    b = Source(gpu_ctx, n, k, length, ns, cs=length + 48)
    o = Output(b, oss=(k + 1) * length)
    try:
        for alive in (np.ones((ns, n), np.uint8), np.full((ns, n), 0xFF, np.uint8)):
            recs = check(b, o, alive, ("clean", n, k))
            assert recs[0]["segs"] == 1 and recs[0]["stripes"] == ns
        # nothing to launch: no stripe, no byte, nothing decodable
        nxec.launch_log_read()
        assert gpu_ctx.rs_decode_mixed(n, k, np.zeros((0, n), np.uint8), b.buf.ptr, b.cs, b.ss, o.buf.ptr, o.ocs, o.oss,
                                       length, 0).size == 0
        assert gpu_ctx.rs_decode_mixed(n, k, alive_of(n, [(1,)] * ns), b.buf.ptr, b.cs, b.ss, o.buf.ptr, o.ocs, o.oss, 0,
                                       ns).tolist() == [1] * ns
        assert gpu_ctx.rs_decode_mixed(n, k, alive_of(n, [tuple(range(n))] * ns), b.buf.ptr, b.cs, b.ss, o.buf.ptr, o.ocs,
                                       o.oss, length, ns).tolist() == [LOST] * ns
        gpu_ctx.sync()
        assert nxec.launch_log_read() == []
    finally:
        o.free()
        b.free()


@pytest.mark.parametrize("route", ["tail", "source base", "output base"])
@pytest.mark.parametrize("n,k", [(6, 4), (14, 10), (10, 4)])
def test_by_runs_through_tail_and_layout(gpu_ctx, n, k, route):
    """len = 4096 + 5: a sub-16-byte tail on an aligned layout, or a source / an output base at offset 3."""
    length = 4096 + 5
    sets = pattern_sets(n, k)
    sets = sets + sets[1:4]  # runs of equal plans and repeats further on
    sets.insert(2, sets[1])
    b = Source(gpu_ctx, n, k, length, len(sets), off=3 if route == "source base" else 0, cs=rup(length))
    o = Output(b, off=3 if route == "output base" else 0, ocs=rup(length))
    try:
        assert not one_launch_shape(b, o)
        check(b, o, alive_of(n, sets), (n, k, route))
    finally:
        o.free()
        b.free()


@pytest.mark.parametrize("length,cs,ocs", [(16, 16, 16), (16384 + 16, 16384 + 64, 16384 + 16),
                                           (3 * 16384 + 48, 3 * 16384 + 48, 3 * 16384 + 96)])
def test_every_small_set_of_6_4_with_clean_and_lost(gpu_ctx, length, cs, ocs):
    n, k = 6, 4
    sets = [e for size in (0, 1, 2) for e in itertools.combinations(range(n), size)]
    assert len(sets) == 22
    sets = sets[:10] + [(0, 1, 2), ()] + sets[10:] + [(3, 4, 5), (0, 1, 2, 3, 4, 5), ()] + sets[::-1][:4]
    b = Source(gpu_ctx, n, k, length, len(sets), cs=cs)
    o = Output(b, ocs=ocs)
    try:
        recs = check(b, o, alive_of(n, sets), (length, cs, ocs))
        # input sets: the clean one (no loss, or parity only), 4 + 4 with one data chunk lost, 6 with two
        assert recs[0]["segs"] == 1 + 8 + 6 and recs[0]["stripes"] == len(sets) - 3
    finally:
        o.free()
        b.free()


@pytest.mark.parametrize("seed", [1, 2])
def test_random_maps_14_10(gpu_ctx, seed):
    """0..6 erased chunks per stripe: some stripes are LOST, plans repeat and interleave."""
    n, k, length, ns = 14, 10, 16384 + 16, 96
    rng = np.random.default_rng(seed)
    alive = rng.integers(1, 256, size=(ns, n), dtype=np.uint8)  # any non-zero byte is alive
    for s in range(ns):
        alive[s, rng.choice(n, size=rng.integers(0, 7), replace=False)] = 0
    res = nxec.rs_decode_mixed_plan(n, k, alive)[0]
    assert (res == LOST).any() and (res == 0).any() and (res >= 3).any()  # result: the lost data chunks
    b = Source(gpu_ctx, n, k, length, ns, cs=length + 48, ss=(n + 1) * (length + 48))
    o = Output(b, ocs=length + 48, oss=(k + 1) * (length + 48))
    try:
        check(b, o, alive, ("random", seed))
    finally:
        o.free()
        b.free()


@pytest.mark.parametrize("n,k,erased", [(6, 4, (1, 4)), (14, 10, (1, 4, 11, 13)), (12, 6, (1, 2, 3, 4, 5, 6)),
                                        (24, 21, (2, 20, 23))])
def test_one_shared_pattern_equals_rs_decode(gpu_ctx, n, k, erased):
    length, ns = 16384 + 16, 5
    alive = alive_of(n, [erased] * ns)
    b = Source(gpu_ctx, n, k, length, ns)
    o = Output(b, ocs=length + 48)
    ref = nxec.DeviceBuffer(o.buf.nbytes)
    try:
        recs = check(b, o, alive, (n, k, erased))
        if k <= MAX_K:
            nt = sum(c < k for c in erased)
            assert recs[0]["segs"] == max(1, (nt + 3) // 4) and recs[0]["stripes"] == ns
        ref.upload(o.blank)
        gpu_ctx.rs_decode(n, k, list(erased), b.buf.ptr, b.cs, b.ss, ref.ptr, o.ocs, o.oss, length, ns)
        gpu_ctx.sync()
        assert np.array_equal(o.buf.download(), ref.download())
    finally:
        ref.free()
        o.free()
        b.free()


def test_queue_steady_state_with_interleaved_segments(gpu_ctx):
    """(14,10), two tiles per chunk, the erased id s % n: the plans' stripes interleave, and at least four
    tiles per workgroup of the launch's grid, so most tiles come from published grabs and every workgroup
    crosses segment boundaries, pure-copy segments (a parity chunk lost) among them."""
    n, k, length = 14, 10, 2 * TILE
    # sized for a grid of one workgroup per CU; the launch record below shows the grid that ran
    grid = json.loads(gpu_ctx.describe_launch(4, k, length, 8))["cus"]
    ns = -(-4 * grid // (length // TILE))
    b = Source(gpu_ctx, n, k, length, ns, seed=9)
    o = Output(b)
    try:
        recs = check(b, o, alive_of(n, [(s % n,) for s in range(ns)]), ("queue", ns))
        m = recs[0]
        # ten plans with one lost data chunk, and the clean plan for the four parity ids
        assert m["segs"] == k + 1 and m["stripes"] == ns and m["grid"] == grid
        assert ns * (length // TILE) >= 4 * m["grid"] * m["tpg"]
    finally:
        o.free()
        b.free()


def test_stream_ordering_and_alive_reuse(gpu_ctx):
    """On a caller's stream: the alive map is overwritten as soon as the call returns, and the download
    follows on the same stream without a device synchronise."""
    n, k, length, ns = 14, 10, 16384 + 16, 40
    sets = [(s % n, (s * 5 + 3) % n) if s % 3 else (s % n,) for s in range(ns)]
    sets = [tuple(sorted(set(e))) for e in sets]
    alive = alive_of(n, sets)
    b = Source(gpu_ctx, n, k, length, ns, cs=length + 48)
    o = Output(b, ocs=length + 48)
    sp = C.c_void_p()
    _lib.check(_lib.lib.nxec_stream_create(C.byref(sp)), "nxec_stream_create")
    try:
        want_res = nxec.rs_decode_mixed_plan(n, k, alive)[0]
        b.erase(alive)
        o.reset()
        want = o.expected(want_res)
        gpu_ctx.sync()
        work = alive.copy()
        for _ in range(3):  # again and again on the stream: each call's tables live in a slot of their own
            res = o.decode(work, stream=sp)
            work[:] = 1  # the call has read it
            work[:, 0] = 0
            assert np.array_equal(res, want_res)
            work[:] = alive
        got = o.buf.download(stream=sp)
        assert np.array_equal(got, want)
    finally:
        _lib.lib.nxec_stream_sync(sp)
        _lib.lib.nxec_stream_destroy(sp)
        o.free()
        b.free()


def object_chunks(ctx, n, k, M, obj, with_md5=False):
    """[ns][n][M] chunks as the agents store them: data chunks cut from the object (the last stripe zero
    padded), parity from nxec_encode_object; with_md5: its [ns][n][16] digests too."""
    length = obj.size
    ns, nf, cl = nxec.object_layout(n, k, length, M)
    ob = nxec.DeviceBuffer(length)
    ob.upload(obj)
    par = nxec.DeviceBuffer(max(ns * (n - k) * M, 1))
    tail = nxec.DeviceBuffer(k * M)
    md5 = nxec.DeviceBuffer(ns * n * 16) if with_md5 else None
    ctx.encode_object(n, k, ob.ptr, length, M, par.ptr, tail.ptr, md5.ptr if md5 else None)
    ctx.sync()
    hp = par.download().reshape(ns, n - k, M)
    ch = np.zeros((ns, n, M), dtype=np.uint8)
    for s in range(ns):
        cs = M if s < nf else cl
        sd = np.zeros(k * cs, dtype=np.uint8)
        piece = obj[s * k * M: s * k * M + k * cs]
        sd[:len(piece)] = piece
        ch[s, :k, :cs] = sd.reshape(k, cs)
        ch[s, k:, :cs] = hp[s, :, :cs]
    for x in (ob, par, tail):
        x.free()
    return ch, md5


def rotating_sets(n, k, ns, lost=None):
    """Different chunks erased per stripe, the last stripe included: stripe s loses 1 + s % (n-k) chunks from
    id s % n on (wrapping); stripe `lost` loses n-k+1."""
    sets = [tuple(sorted({(s + i) % n for i in range(1 + s % (n - k))})) for s in range(ns)]
    if lost is not None:
        sets[lost] = tuple(range(n - k + 1))
    return sets


@pytest.mark.parametrize("n,k,M,full,rem", [
    (6, 4, 16384 + 16, 4, 0),            # a multiple of k*M, one launch
    (6, 4, 16384 + 16, 3, 4 * 1000 + 3),  # a remainder not divisible by k
    (6, 4, 16384 + 16, 0, 4 * 777 + 1),   # only a last stripe
    (14, 10, 16384 + 16, 5, 10 * 512 + 7),
    (6, 4, 4096 + 5, 4, 4 * 100 + 2),     # by-runs
])
def test_objects(gpu_ctx, n, k, M, full, rem):
    length = full * k * M + rem
    ns, nf, cl = nxec.object_layout(n, k, length, M)
    assert (nf, ns) == (full, full + (rem > 0))
    obj = np.random.default_rng(length).integers(0, 256, length, dtype=np.uint8)
    ch, _ = object_chunks(gpu_ctx, n, k, M, obj)
    lost = 1 if full >= 3 else None
    sets = rotating_sets(n, k, ns, lost)
    alive = alive_of(n, sets)
    want_res = nxec.rs_decode_mixed_plan(n, k, alive)[0]
    assert [s for s in range(ns) if want_res[s] < 0] == ([] if lost is None else [lost])
    assert lost is None or want_res[lost] == LOST
    for s, e in enumerate(sets):
        ch[s, list(e)] = 0xEE
    cb = nxec.DeviceBuffer(ch.nbytes)
    cb.upload(ch)
    out = nxec.DeviceBuffer(length)
    blank = sentinel(length)
    out.upload(blank)
    tail = nxec.DeviceBuffer(k * M)
    try:
        nxec.launch_log_read()
        res = gpu_ctx.decode_object_mixed(n, k, alive, cb.ptr, M, n * M, length, M, out.ptr, tail.ptr)
        gpu_ctx.sync()
        recs = nxec.launch_log_read()
        assert np.array_equal(res, want_res)
        want = obj.copy()
        if lost is not None:  # a LOST full stripe leaves its k*M object bytes alone
            want[lost * k * M:(lost + 1) * k * M] = blank[lost * k * M:(lost + 1) * k * M]
        assert np.array_equal(out.download(), want)
        assert np.array_equal(cb.download(), ch.reshape(-1))
        mixed = [r for r in recs if r["family"] == "k_decode_mixed"]
        if M % 16 == 0 and nf > 0:
            assert len(mixed) == 1 and mixed[0]["stripes"] == nf - (lost is not None)
        else:
            assert not mixed
        assert all(r["family"] in BY_RUNS for r in recs if r not in mixed)
    finally:
        for x in (cb, out, tail):
            x.free()


def test_lost_last_stripe_is_skipped_and_reported(gpu_ctx):
    n, k, M = 6, 4, 16384 + 16
    length = 2 * k * M + 4 * 300 + 1
    obj = np.random.default_rng(7).integers(0, 256, length, dtype=np.uint8)
    ch, _ = object_chunks(gpu_ctx, n, k, M, obj)
    alive = alive_of(n, [(5,), (), (0, 2, 4)])
    cb = nxec.DeviceBuffer(ch.nbytes)
    cb.upload(ch)
    out = nxec.DeviceBuffer(length)
    blank = sentinel(length)
    out.upload(blank)
    tail = nxec.DeviceBuffer(k * M)
    try:
        res = gpu_ctx.decode_object_mixed(n, k, alive, cb.ptr, M, n * M, length, M, out.ptr, tail.ptr)
        gpu_ctx.sync()
        assert res.tolist() == [0, 0, LOST]
        want = obj.copy()
        want[2 * k * M:] = blank[2 * k * M:]
        assert np.array_equal(out.download(), want)
    finally:
        for x in (cb, out, tail):
            x.free()


def test_verify_then_decode_around_the_bad_chunks(gpu_ctx):
    """Closing the loop: nxec_decode_object_verify with no failed chunk flags the corrupted data chunks in
    d_ok (preset to 1, so chunks it did not read stay trusted); the downloaded map is the alive map of
    nxec_decode_object_mixed, which returns the original object."""
    n, k, M = 14, 10, 4096
    length = 6 * k * M + 10 * 123 + 4
    ns, nf, cl = nxec.object_layout(n, k, length, M)
    obj = np.random.default_rng(99).integers(0, 256, length, dtype=np.uint8)
    ch, md5 = object_chunks(gpu_ctx, n, k, M, obj, with_md5=True)
    bad = {0: 3, 2: 0, 3: 9, 5: 7, ns - 1: 4}  # stripe -> corrupted data chunk, the last stripe included
    for s, c in bad.items():
        ch[s, c, 17] ^= 0x40
    cb = nxec.DeviceBuffer(ch.nbytes)
    cb.upload(ch)
    out = nxec.DeviceBuffer(length)
    tail = nxec.DeviceBuffer(k * M)
    ok = nxec.DeviceBuffer(ns * n)
    ok.memset(1)
    try:
        gpu_ctx.decode_object_verify(n, k, [], cb.ptr, length, M, md5.ptr, out.ptr, tail.ptr, ok.ptr)
        gpu_ctx.sync()
        assert not np.array_equal(out.download(), obj)  # the flagged stripes decoded to undefined bytes
        alive = ok.download().reshape(ns, n)
        assert np.array_equal(alive, alive_of(n, [(bad[s],) if s in bad else () for s in range(ns)]))
        out.upload(sentinel(length))
        res = gpu_ctx.decode_object_mixed(n, k, alive, cb.ptr, M, n * M, length, M, out.ptr, tail.ptr)
        gpu_ctx.sync()
        assert res.tolist() == [1 if s in bad else 0 for s in range(ns)]
        assert np.array_equal(out.download(), obj)
    finally:
        for x in (cb, out, tail, ok, md5):
            x.free()
