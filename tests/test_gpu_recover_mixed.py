"""Mixed-pattern recover on the GPU (nxec_rs_recover_stripes_mixed): every
stripe of a batch rebuilds its own erased chunks.

Method: encode a fill_random batch and keep its host copy as truth; overwrite
every erased chunk with fresh garbage; call; download the whole buffer.  It
must equal truth everywhere except in the erased chunks of stripes whose
result is negative (LOST, SINGULAR), which keep their garbage: that checks the
rebuilt bytes and that nothing else was written, stride padding included.
The result array must be the CPU plan's.

Shapes, the smallest that reach each way the kernel can go wrong:
  geometry (6,4)    prefetch instantiation
           (14,10)  four rows, R = 8
           (10,4)   sets of 5 and 6 erasures: two segments over the same sources
           (12,6)   {0,2,5,7,8} is singular: reported, stripe untouched
           (23,19)  the widest instantiation
           (24,21)  k > 19: the by-runs path
  len      16 (one vector), 16384 (one full tile), 16384 + 16, 3 * 16384 + 48;
           4096 + 5 reaches the by-runs path through its tail (base 0, chunk
           stride rounded up to 16) and through the layout (base offset 3)
  strides  packed, chunk_stride = len + 48, stripe_stride padded by one chunk
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


def rup(x, m=16):
    return (x + m - 1) // m * m


def strides(n, length):
    """(chunk stride, stripe stride): packed, padded chunks, stripes padded by one chunk"""
    return [(length, n * length), (length + 48, n * (length + 48)), (length, (n + 1) * length)]


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


class Batch:
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

    def expected(self, damaged, alive, result):
        """truth, but the erased chunks of stripes with a negative result keep their garbage"""
        want = self.truth.copy()
        a = np.asarray(alive).reshape(self.ns, self.n)
        for s in np.flatnonzero(np.asarray(result) < 0):
            for c in np.flatnonzero(a[s] == 0):
                want[self.at(s, c): self.at(s, c) + self.len] = damaged[self.at(s, c): self.at(s, c) + self.len]
        return want

    def recover(self, alive, stream=None):
        return self.ctx.rs_recover_mixed(self.n, self.k, alive, self.buf.ptr + self.off, self.cs, self.ss, self.len,
                                         self.ns, stream)


def check(b, alive, tag, one_launch):
    """Damage, recover, compare the whole buffer and the verdicts; returns the launch records of the call."""
    alive = np.ascontiguousarray(alive, dtype=np.uint8)
    want_res, npat, nseg, ncoded = nxec.rs_recover_mixed_plan(b.n, b.k, alive)
    damaged = b.erase(alive)
    nxec.launch_log_read()
    res = b.recover(alive)
    b.ctx.sync()
    recs = nxec.launch_log_read()
    got = b.buf.download()
    assert np.array_equal(res, want_res), (tag, res, want_res)
    want = b.expected(damaged, alive, want_res)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        first = int(bad[0]) - b.off
        pytest.fail(f"{tag}: {bad.size} bytes differ, first in stripe {first // b.ss} at stripe byte {first % b.ss} "
                    f"(chunk stride {b.cs}, len {b.len})")
    mixed = [r for r in recs if r["family"] == "k_mul_mixed"]
    if ncoded == 0 or b.len == 0:
        assert recs == [], (tag, recs)
    elif one_launch:
        assert len(mixed) == 1 and len(recs) == 1, (tag, recs)
        m = mixed[0]
        assert (m["k"], m["rows"], m["q"], m["segs"], m["stripes"]) == (b.k, 4, 1, nseg, ncoded), (tag, m)
        assert m["pf"] == int(b.k <= 8) and m["r"] == (16 if b.k <= 9 else 8), (tag, m)
    else:
        assert not mixed and recs and all(r["family"] in BY_RUNS for r in recs), (tag, recs)
    return recs


def pattern_sets(n, k):
    """A handful of stripes per geometry: clean, single, scattered, full n-k, geometry specials, lost."""
    m = n - k
    sets = [(), (0,), (n - 1,), tuple(range(m)), tuple(range(n - m, n)), (1, k)[:m], tuple(range(0, n, 2))[:m]]
    if (n, k) == (10, 4):
        sets += [(0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 9), (2, 4, 5, 6, 8, 9), (0, 1, 2, 3, 4)]  # two segments each
    if (n, k) == (12, 6):
        sets += [(0, 2, 5, 7, 8), (0, 3, 5, 8, 9), (0, 2, 5, 7, 9), (1, 2, 3, 4, 5, 6)]  # the first two are singular
    sets += [tuple(range(m + 1)), tuple(range(n))]  # lost
    return sets


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("n,k", [(6, 4), (14, 10), (10, 4), (12, 6), (23, 19), (24, 21)])
def test_geometries(gpu_ctx, n, k, length):
    sets = pattern_sets(n, k)
    if (n, k) == (12, 6):
        res = nxec.rs_recover_mixed_plan(n, k, alive_of(n, sets))[0]
        assert res[sets.index((0, 2, 5, 7, 8))] == SINGULAR and res[sets.index((0, 2, 5, 7, 9))] == 5
    for cs, ss in strides(n, length):
        b = Batch(gpu_ctx, n, k, length, len(sets), cs=cs, ss=ss)
        try:
            check(b, alive_of(n, sets), (n, k, length, cs, ss), one_launch=k <= 19)
        finally:
            b.free()
    # 1 and 5 stripes, every stripe coded
    for ns in (1, 5):
        b = Batch(gpu_ctx, n, k, length, ns, cs=length + 48)
        try:
            some = [e for e in sets if 0 < len(e) <= n - k][:ns]
            check(b, alive_of(n, (some * ns)[:ns]), (n, k, length, ns), one_launch=k <= 19)
        finally:
            b.free()


@pytest.mark.parametrize("off,cs", [(0, rup(4096 + 5)), (3, 4096 + 5), (3, 4096 + 5 + 48)])
@pytest.mark.parametrize("n,k", [(6, 4), (14, 10), (10, 4)])
def test_by_runs_through_tail_and_layout(gpu_ctx, n, k, off, cs):
    """len = 4096 + 5: a sub-16-byte tail (aligned base and strides) or an unaligned layout (base offset 3)."""
    length = 4096 + 5
    sets = pattern_sets(n, k)
    sets = sets + sets[1:4]  # runs of equal patterns and repeats further on
    sets.insert(2, sets[1])
    b = Batch(gpu_ctx, n, k, length, len(sets), off=off, cs=cs)
    try:
        check(b, alive_of(n, sets), (n, k, off, cs), one_launch=False)
    finally:
        b.free()


@pytest.mark.parametrize("length,cs", [(16, 16), (16384 + 16, 16384 + 64), (3 * 16384 + 48, 3 * 16384 + 48)])
def test_every_pattern_of_6_4_with_clean_and_lost(gpu_ctx, length, cs):
    n, k = 6, 4
    sets = [e for size in (1, 2) for e in itertools.combinations(range(n), size)]
    assert len(sets) == 21
    sets = [()] + sets[:10] + [(0, 1, 2), ()] + sets[10:] + [(3, 4, 5), (0, 1, 2, 3, 4, 5)] + sets[::-1][:4]
    b = Batch(gpu_ctx, n, k, length, len(sets), cs=cs)
    try:
        recs = check(b, alive_of(n, sets), (length, cs), one_launch=True)
        assert recs[0]["segs"] == 21 and recs[0]["stripes"] == 25
    finally:
        b.free()


@pytest.mark.parametrize("seed", [1, 2])
def test_random_maps_14_10(gpu_ctx, seed):
    """0..6 erased chunks per stripe: some stripes are LOST, patterns repeat and interleave."""
    n, k, length, ns = 14, 10, 16384 + 16, 96
    rng = np.random.default_rng(seed)
    alive = rng.integers(1, 256, size=(ns, n), dtype=np.uint8)  # any non-zero byte is alive
    for s in range(ns):
        alive[s, rng.choice(n, size=rng.integers(0, 7), replace=False)] = 0
    res = nxec.rs_recover_mixed_plan(n, k, alive)[0]
    assert (res == LOST).any() and (res == 0).any() and (res == 4).any()
    b = Batch(gpu_ctx, n, k, length, ns, cs=length + 48, ss=(n + 1) * (length + 48))
    try:
        check(b, alive, ("random", seed), one_launch=True)
    finally:
        b.free()


@pytest.mark.parametrize("n,k,erased", [(6, 4, (1, 4)), (14, 10, (1, 4, 11, 13)), (10, 4, (0, 2, 3, 5, 7, 9)),
                                        (23, 19, (0, 7, 19, 22)), (24, 21, (2, 20, 23))])
def test_one_shared_pattern_equals_rs_recover(gpu_ctx, n, k, erased):
    length, ns = 16384 + 16, 5
    alive = alive_of(n, [erased] * ns)
    b = Batch(gpu_ctx, n, k, length, ns)
    ref = nxec.DeviceBuffer(b.buf.nbytes)
    try:
        recs = check(b, alive, (n, k, erased), one_launch=k <= 19)
        if k <= 19:
            assert recs[0]["segs"] == (len(erased) + 3) // 4 and recs[0]["stripes"] == ns
        ref.upload(b.erase(alive))
        gpu_ctx.rs_recover(n, k, list(erased), ref.ptr, b.cs, b.ss, length, ns)
        gpu_ctx.sync()
        b.recover(alive)
        gpu_ctx.sync()
        assert np.array_equal(b.buf.download(), ref.download())
    finally:
        ref.free()
        b.free()


def test_all_clean_launches_nothing(gpu_ctx):
    n, k, length, ns = 14, 10, 16384, 5
    b = Batch(gpu_ctx, n, k, length, ns)
    try:
        nxec.launch_log_read()
        for alive in (np.ones((ns, n), np.uint8), np.full((ns, n), 0xFF, np.uint8)):
            assert b.recover(alive).tolist() == [0] * ns
        assert gpu_ctx.rs_recover_mixed(n, k, np.zeros((0, n), np.uint8), b.buf.ptr, b.cs, b.ss, length, 0).size == 0
        assert b.ctx.rs_recover_mixed(n, k, alive_of(n, [(1,)] * ns), b.buf.ptr, b.cs, b.ss, 0, ns).tolist() == [1] * ns
        assert gpu_ctx.rs_recover_mixed(4, 4, alive_of(4, [(1,), ()]), b.buf.ptr, 64, 256, 64, 2).tolist() == [LOST, 0]
        gpu_ctx.sync()
        assert nxec.launch_log_read() == []
        assert np.array_equal(b.buf.download(), b.truth)
    finally:
        b.free()


def test_queue_steady_state_with_interleaved_segments(gpu_ctx):
    """(14,10), two tiles per chunk, the erased id s % n: 14 segments whose stripes interleave, and at least
    four tiles per workgroup of the launch's grid, so most tiles come from published grabs and every
    workgroup rebuilds its tables at each segment boundary it crosses."""
    n, k, length = 14, 10, 2 * TILE
    # sized for a grid of one workgroup per CU; the launch record below shows the grid that ran
    grid = json.loads(gpu_ctx.describe_launch(4, k, length, 8))["cus"]
    ns = -(-4 * grid // (length // TILE))
    b = Batch(gpu_ctx, n, k, length, ns, seed=9)
    try:
        recs = check(b, alive_of(n, [(s % n,) for s in range(ns)]), ("queue", ns), one_launch=True)
        m = recs[0]
        assert m["segs"] == n and m["stripes"] == ns and m["grid"] == grid
        assert ns * (length // TILE) >= 4 * m["grid"] * m["tpg"]
    finally:
        b.free()


def test_stream_ordering_and_alive_reuse(gpu_ctx):
    """On a caller's stream: the alive map is overwritten as soon as the call returns, and the download
    follows on the same stream without a device synchronise."""
    n, k, length, ns = 14, 10, 16384 + 16, 40
    sets = [(s % n, (s * 5 + 3) % n) if s % 3 else (s % n,) for s in range(ns)]
    sets = [tuple(sorted(set(e))) for e in sets]
    alive = alive_of(n, sets)
    b = Batch(gpu_ctx, n, k, length, ns, cs=length + 48)
    sp = C.c_void_p()
    _lib.check(_lib.lib.nxec_stream_create(C.byref(sp)), "nxec_stream_create")
    try:
        want_res = nxec.rs_recover_mixed_plan(n, k, alive)[0]
        damaged = b.erase(alive)
        want = b.expected(damaged, alive, want_res)
        gpu_ctx.sync()
        work = alive.copy()
        for _ in range(3):  # again and again on the stream: each call's tables live in a slot of their own
            res = b.recover(work, stream=sp)
            work[:] = 1  # the call has read it
            work[:, 0] = 0
            assert np.array_equal(res, want_res)
            work[:] = alive
        got = b.buf.download(stream=sp)
        assert np.array_equal(got, want)
    finally:
        _lib.lib.nxec_stream_sync(sp)
        _lib.lib.nxec_stream_destroy(sp)
        b.free()
