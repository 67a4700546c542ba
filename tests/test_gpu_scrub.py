"""Parity scrub on the GPU (nxec_rs_scrub_stripes): detect, locate, heal.

Batches are encoded with rs_encode from fill_random data; every expected
status follows from where the test flips bytes, so no model is needed.  The
shapes are the smallest that reach each code path:

  geometry (6,4)    two parity rows, prefetch instantiation (6 sources)
           (14,10)  four rows, 14 sources
           (20,16)  k + rows = 20, the widest vector kernel
           (12,6)   six rows: two passes flagging one status word
           (5,4)    one row: detect only
           (24,21)  k > 16: the byte kernel
  len      16 (one vector), 16384 (one full tile), 16384 + 16 (full tile +
           ragged launch), 4096 + 5 (ragged launch + sub-16 tail; with the base
           offset by 3 bytes everything goes through the byte kernel)
  strides  packed and chunk_stride = len + 48; 1 and 5 stripes
"""
import ctypes as C

import numpy as np
import pytest

from nexoedge_amd import _lib, nxec

pytestmark = pytest.mark.gpu

CLEAN, UNLOCATED = nxec.SCRUB_CLEAN, nxec.SCRUB_UNLOCATED
LOCATE, REPAIR = nxec.SCRUB_LOCATE, nxec.SCRUB_REPAIR
GEOMS = [(6, 4), (14, 10), (20, 16), (12, 6), (5, 4), (24, 21)]
LENS = [16, 16384, 16384 + 16, 4096 + 5]
TILE = 16384
NBAD0 = 1000  # the counter's value before each call: the call adds, never resets


def rup(x, m=16):
    return (x + m - 1) // m * m


def layouts(length):
    """(base offset, chunk stride) pairs for one chunk length."""
    if length % 16 == 0:
        return [(0, length), (0, length + 48)]
    # byte kernel (nothing aligned), the same padded, and the aligned layout whose last 5 bytes are the sub-16 tail
    return [(3, length), (3, length + 48), (0, rup(length))]


class Batch:
    """An encoded [ns][n] batch on the device, its host copy, and a status / counter pair."""

    def __init__(self, ctx, n, k, length, ns, off=0, cs=None, seed=7):
        self.ctx, self.n, self.k, self.len, self.ns, self.off = ctx, n, k, length, ns, off
        self.cs = cs if cs is not None else length
        self.ss = n * self.cs
        self.buf = nxec.DeviceBuffer(off + ns * self.ss + 16)
        self.buf.fill_random(seed + 131 * n + length)
        ctx.rs_encode(n, k, self.buf.ptr + off, self.cs, self.ss, length, ns)
        ctx.sync()
        self.aux = nxec.DeviceBuffer(ns * 4 + 16)
        self.cnt = rup(ns * 4, 8)

    def free(self):
        self.buf.free()
        self.aux.free()

    def at(self, s, c, pos=0):
        return self.off + s * self.ss + c * self.cs + pos

    def host(self):
        return self.buf.download()

    def put(self, s, c, pos, data):
        self.buf.upload(np.asarray(data, dtype=np.uint8), self.at(s, c, pos))

    def scrub(self, flags=0, count=True, stream=None, wait=True):
        """(statuses, growth of the counter)"""
        self.aux.upload(np.full(self.ns, 12345, dtype=np.int32))  # stale statuses: the call resets them
        self.aux.upload(np.array([NBAD0], dtype=np.uint64), self.cnt)
        self.ctx.rs_scrub_stripes(self.n, self.k, self.buf.ptr + self.off, self.cs, self.ss, self.len, self.ns,
                                  self.aux.ptr, flags, self.aux.ptr + self.cnt if count else None, stream)
        if not wait:
            return None
        if stream is None:
            self.ctx.sync()
        return self.result(stream)

    def result(self, stream=None):
        raw = self.aux.download(stream=stream)
        return raw[: self.ns * 4].view(np.int32).copy(), int(raw[self.cnt: self.cnt + 8].view(np.uint64)[0]) - NBAD0


def stripes_of(ns):
    return sorted({0, ns // 2, ns - 1})


def positions(length):
    """offset 0, the last byte of the full-tile region, inside the ragged remainder, inside the sub-16 tail"""
    pos = {0}
    full = length // TILE * TILE
    if full:
        pos.add(full - 1)
    if length // 16 * 16 > full:
        pos.add(full + (length // 16 * 16 - full) // 2)
    if length % 16:
        pos.add(length - 1)
        pos.add(length // 16 * 16)
    return sorted(p for p in pos if p < length)


def chunks_of(n, k):
    c = {0, k - 1, k, n - 1}
    if (n, k) == (12, 6):
        c.add(k + 5)  # parity row 5: the second pass
    return sorted(c)


def expect(ns, bad, value):
    e = np.full(ns, CLEAN, dtype=np.int32)
    e[list(bad)] = value
    return e


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("n,k", GEOMS)
def test_scrub_shapes(gpu_ctx, n, k, length):
    m = n - k
    for off, cs in layouts(length):
        for ns in (1, 5):
            b = Batch(gpu_ctx, n, k, length, ns, off, cs)
            try:
                orig = b.host()
                tag = (n, k, length, off, cs, ns)
                # 1. clean batch: every status CLEAN, counter and bytes unchanged
                for flags in (0, LOCATE, REPAIR):
                    st, grew = b.scrub(flags)
                    assert np.array_equal(st, expect(ns, [], 0)) and grew == 0, (tag, flags, st, grew)
                st, _ = b.scrub(LOCATE, count=False)
                assert np.array_equal(st, expect(ns, [], 0)), tag
                assert np.array_equal(b.host(), orig), tag
                # 2. one flipped byte per chosen stripe
                bad = stripes_of(ns)
                for c in chunks_of(n, k):
                    for pos in positions(length):
                        cur = orig.copy()
                        for s in bad:
                            cur[b.at(s, c, pos)] ^= 0x40 + s
                            b.put(s, c, pos, cur[b.at(s, c, pos): b.at(s, c, pos) + 1])
                        st, grew = b.scrub(0)
                        assert np.array_equal(st, expect(ns, bad, UNLOCATED)) and grew == len(bad), (tag, c, pos, st)
                        st, grew = b.scrub(LOCATE)
                        want = c if m >= 2 else UNLOCATED
                        assert np.array_equal(st, expect(ns, bad, want)) and grew == len(bad), (tag, c, pos, st)
                        st, _ = b.scrub(0, count=False)  # detect only, no counter: no second stage at all
                        assert np.array_equal(st, expect(ns, bad, UNLOCATED)), (tag, c, pos, st)
                        assert np.array_equal(b.host(), cur), (tag, c, pos)  # nothing written without REPAIR
                        for s in bad:
                            b.put(s, c, pos, orig[b.at(s, c, pos): b.at(s, c, pos) + 1])
                # 3. a whole chunk overwritten: located, healed, clean afterwards
                s = ns // 2
                rng = np.random.default_rng(1000 * n + length + ns)
                for c in (1 % k, n - 1):
                    junk = rng.integers(0, 256, length, dtype=np.uint8)
                    junk[0] = orig[b.at(s, c)] ^ 1  # differs from the original for sure
                    cur = orig.copy()
                    cur[b.at(s, c): b.at(s, c) + length] = junk
                    b.put(s, c, 0, junk)
                    st, grew = b.scrub(LOCATE)
                    want = c if m >= 2 else UNLOCATED
                    assert np.array_equal(st, expect(ns, [s], want)) and grew == 1, (tag, c, st)
                    assert np.array_equal(b.host(), cur), (tag, c)
                    st, grew = b.scrub(REPAIR)
                    assert np.array_equal(st, expect(ns, [s], want)) and grew == 1, (tag, c, st)
                    if m >= 2:
                        assert np.array_equal(b.host(), orig), (tag, c, "not healed")
                        st, grew = b.scrub(REPAIR)
                        assert np.array_equal(st, expect(ns, [], 0)) and grew == 0, (tag, c, st)
                    else:
                        assert np.array_equal(b.host(), cur), (tag, c, "detect-only code wrote")
                        b.put(s, c, 0, orig[b.at(s, c): b.at(s, c) + length])
                # 4. two chunks of one stripe at different offsets: not one chunk's doing
                s = ns - 1
                cur = orig.copy()
                for c, pos in ((0, 0), (n - 1, length - 1)):
                    cur[b.at(s, c, pos)] ^= 0x5A
                    b.put(s, c, pos, cur[b.at(s, c, pos): b.at(s, c, pos) + 1])
                for flags in (LOCATE, REPAIR):
                    st, grew = b.scrub(flags)
                    assert np.array_equal(st, expect(ns, [s], UNLOCATED)) and grew == 1, (tag, flags, st)
                    assert np.array_equal(b.host(), cur), (tag, flags, "an unlocated stripe was written")
                for c, pos in ((0, 0), (n - 1, length - 1)):
                    b.put(s, c, pos, orig[b.at(s, c, pos): b.at(s, c, pos) + 1])
                # 5. two chunks at the same offset: never mistaken for a third chunk when n-k >= 3
                if m >= 3:
                    pos = length // 2
                    for pair, errs in (((1, k + 1), (1, 1)), ((0, k - 1), (0x53, 0xCA)), ((k, n - 1), (7, 9))):
                        cur = orig.copy()
                        for c, e in zip(pair, errs):
                            cur[b.at(s, c, pos)] ^= e
                            b.put(s, c, pos, cur[b.at(s, c, pos): b.at(s, c, pos) + 1])
                        st, grew = b.scrub(REPAIR)
                        assert np.array_equal(st, expect(ns, [s], UNLOCATED)) and grew == 1, (tag, pair, st)
                        assert np.array_equal(b.host(), cur), (tag, pair)
                        for c in pair:
                            b.put(s, c, pos, orig[b.at(s, c, pos): b.at(s, c, pos) + 1])
                assert np.array_equal(b.host(), orig), tag
            finally:
                b.free()


def test_same_offset_pair_on_rs_14_10(gpu_ctx):
    """Every pair of chunks of RS(14,10) corrupted at one offset reports UNLOCATED (distance 5)."""
    n, k, length, ns = 14, 10, 4096, 3
    b = Batch(gpu_ctx, n, k, length, ns)
    try:
        orig = b.host()
        pos, s = 1027, 1
        for a in range(n):
            for c in range(a + 1, n):
                one = orig[b.at(s, a, pos): b.at(s, a, pos) + 1] ^ 0x53
                two = orig[b.at(s, c, pos): b.at(s, c, pos) + 1] ^ 0xCA
                b.put(s, a, pos, one)
                b.put(s, c, pos, two)
                st, grew = b.scrub(LOCATE)
                assert np.array_equal(st, expect(ns, [s], UNLOCATED)) and grew == 1, (a, c, st)
                b.put(s, a, pos, orig[b.at(s, a, pos): b.at(s, a, pos) + 1])
                b.put(s, c, pos, orig[b.at(s, c, pos): b.at(s, c, pos) + 1])
    finally:
        b.free()


def test_stream_ordering(gpu_ctx):
    """encode -> erase one chunk (memset2d) -> scrub on one stream, no host sync in between."""
    n, k, length, ns, gone = 14, 10, 16384 + 16, 5, 3
    cs = length + 48
    buf = nxec.DeviceBuffer(ns * n * cs)
    aux = nxec.DeviceBuffer(rup(ns * 4, 8) + 8)
    sp = C.c_void_p()
    _lib.check(_lib.lib.nxec_stream_create(C.byref(sp)), "nxec_stream_create")
    try:
        buf.fill_random(99)
        aux.upload(np.zeros(aux.nbytes, dtype=np.uint8))
        gpu_ctx.rs_encode(n, k, buf.ptr, cs, n * cs, length, ns, stream=sp)
        buf.memset2d(0, gone * cs, n * cs, length, ns, stream=sp)
        gpu_ctx.rs_scrub_stripes(n, k, buf.ptr, cs, n * cs, length, ns, aux.ptr, REPAIR, aux.ptr + rup(ns * 4, 8),
                                 stream=sp)
        raw = aux.download(stream=sp)
        st = raw[: ns * 4].view(np.int32)
        assert np.array_equal(st, np.full(ns, gone, dtype=np.int32)), st
        assert int(raw[rup(ns * 4, 8):].view(np.uint64)[0]) == ns
        # healed: a second scrub on the same stream is clean
        gpu_ctx.rs_scrub_stripes(n, k, buf.ptr, cs, n * cs, length, ns, aux.ptr, LOCATE, None, stream=sp)
        st = aux.download(stream=sp)[: ns * 4].view(np.int32)
        assert np.array_equal(st, np.full(ns, CLEAN, dtype=np.int32)), st
    finally:
        _lib.lib.nxec_stream_sync(sp)
        _lib.lib.nxec_stream_destroy(sp)
        buf.free()
        aux.free()


def test_queue_run(gpu_ctx):
    """More tiles than workgroups: queue grabs and both ping-pong buffers run.
    (6,4), 64 KiB + 16 chunks, 160 stripes (about 60 MiB): 5 tiles per stripe."""
    n, k, length, ns = 6, 4, 65536 + 16, 160
    b = Batch(gpu_ctx, n, k, length, ns)
    try:
        total = b.off + ns * b.ss
        sum0 = b.buf.checksum(total)
        st, grew = b.scrub(REPAIR)
        assert np.array_equal(st, expect(ns, [], 0)) and grew == 0
        assert b.buf.checksum(total) == sum0
        # one byte in each of the five tiles of a stripe, different stripes and chunks
        flips = {0: (0, 0), 1: (1, TILE - 1), 57: (3, TILE), 80: (4, 2 * TILE + 5), 121: (5, 4 * TILE - 1),
                 158: (2, 4 * TILE + 3), 159: (5, length - 1)}
        saved = {}
        for s, (c, pos) in flips.items():
            saved[s] = b.buf.download(1, b.at(s, c, pos))
            b.put(s, c, pos, saved[s] ^ 0x21)
        sum1 = b.buf.checksum(total)
        assert sum1 != sum0
        want = np.full(ns, CLEAN, dtype=np.int32)
        for s, (c, _) in flips.items():
            want[s] = c
        st, grew = b.scrub(0)
        assert np.array_equal(st, np.where(want == CLEAN, CLEAN, UNLOCATED)) and grew == len(flips), st
        st, grew = b.scrub(LOCATE)
        assert np.array_equal(st, want) and grew == len(flips), st
        assert b.buf.checksum(total) == sum1  # nothing written without REPAIR
        st, grew = b.scrub(REPAIR)
        assert np.array_equal(st, want) and grew == len(flips), st
        assert b.buf.checksum(total) == sum0  # healed
        st, grew = b.scrub(LOCATE)
        assert np.array_equal(st, expect(ns, [], 0)) and grew == 0
    finally:
        b.free()


def test_empty_calls_reset_the_statuses(gpu_ctx):
    """len == 0 launches nothing and reports CLEAN; n == k has nothing to check."""
    aux = nxec.DeviceBuffer(4 * 8)
    buf = nxec.DeviceBuffer(4096)
    try:
        for n, k, length in ((6, 4, 0), (4, 4, 64)):
            aux.upload(np.full(8, 77, dtype=np.int32))
            gpu_ctx.rs_scrub_stripes(n, k, buf.ptr, 64, n * 64, length, 6, aux.ptr, LOCATE)
            gpu_ctx.sync()
            st = aux.download().view(np.int32)
            assert np.array_equal(st, [CLEAN] * 6 + [77, 77]), (n, k, length, st)
        st, nbad = gpu_ctx.rs_scrub(6, 4, buf.ptr, 64, 6 * 64, 0, 3, REPAIR)
        assert st.tolist() == [CLEAN] * 3 and nbad == 0
    finally:
        aux.free()
        buf.free()
