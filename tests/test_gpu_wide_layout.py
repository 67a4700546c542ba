"""Every strided kernel at chunk offsets up to the 4 GiB stripe limit.

The strided calls keep a chunk's byte offset inside its stripe in 32 bits
(include/nxec.h: "chunks of a stripe must lie within 4 GiB", checked on the host
as (n-1)*chunk_stride + len <= 2^32 - 1).  Here the kernels run at the largest
layouts that contract accepts, so a sign-extended offset, a 32-bit product or an
offset sum that wraps computes a wrong byte that these tests see.

One ~10 GiB device buffer serves the whole module: 2 GiB of guard, then two
stripes SS = 2^32 + 2^20 apart, then 1 MiB.  The guard and the space between the
chunks keep a wrong address inside the allocation: a kernel that sign-extended
or wrapped an offset changes a byte some check here reads instead of faulting.
Per case the buffer is set to 0xEE, only the chunk windows are uploaded, the
call runs, every window comes back with 64 bytes either side and is compared
byte for byte with the host oracle's result on packed copies, and everything
between the windows is covered by DeviceBuffer.checksum before and after the call.
The kernel work per case is a few tiles.
"""
import functools
import hashlib

import numpy as np
import pytest

import oracle
from helpers import fill_bytes
from nexoedge_amd import _lib, nxec

pytestmark = pytest.mark.gpu

G4 = 1 << 32
BASE = 1 << 31               # the batch starts behind 2 GiB of guard
SS = G4 + (1 << 20)          # stripe 1 from stripe 0
NBYTES = BASE + 2 * SS + (1 << 20)
MARGIN = 64
FILL = 0xEE
INVALID = _lib.NXEC_ERR_INVALID


def top_stride(nchunks, length):
    """The largest multiple of 16 with (nchunks-1)*cs + length <= 2^32 - 16."""
    cs = (G4 - 16 - length) // (nchunks - 1) // 16 * 16
    assert (nchunks - 1) * cs + length <= G4 - 16 < (nchunks - 1) * (cs + 16) + length
    return cs


class Layout:
    def __init__(self, name, n, k, length, cs, ss=SS, base=BASE):
        self.name, self.n, self.k, self.len, self.cs, self.ss, self.base = name, n, k, length, cs, ss, base
        assert cs >= length and (n - 1) * cs + length <= G4 - 1  # what the contract accepts
        assert base >= BASE and base + ss + (n - 1) * cs + length <= NBYTES - (1 << 20) + 16

    def off(self, s, c):
        return self.base + s * self.ss + c * self.cs

    def out_stride(self):
        """The chunk stride of a wide decode output: the same rule with k in place of n."""
        if self.base % 16 == 0:
            return top_stride(self.k, self.len)
        return (G4 - 1 - self.len) // (self.k - 1)

    def __repr__(self):
        return self.name


def top(n, k, length=16384 + 16):
    return Layout(f"top-{n}-{k}" + ("" if length == 16400 else f"-{length}"), n, k, length, top_stride(n, length))


TOPS = [top(6, 4), top(14, 10), top(12, 6), top(5, 4), top(24, 21)]
STRADDLE = Layout("straddle", 3, 2, 16400, (1 << 31) - 8208)
BYTES = Layout("bytes", 6, 4, 4105, (G4 - 1 - 4105) // 5, ss=SS + 5, base=BASE + 3)
LAYOUTS = TOPS + [STRADDLE, BYTES]
# the fused multiply + MD5 kernels walk chunks in 256-byte steps
FUSED = [Layout("straddle-256", 3, 2, 16384, (1 << 31) - 8208), top(6, 4, 16384), top(14, 10, 16384), top(5, 4, 16384)]


def test_layouts_are_what_they_claim():
    t64 = TOPS[0]
    assert (t64.cs, 5 * t64.cs + t64.len) == (858990176, G4 - 16)  # RS(6,4): the last chunk ends exactly at 2^32 - 16
    t = TOPS[1]
    assert [c for c in range(14) if (c * t.cs) >> 31] == list(range(7, 14))  # RS(14,10): bit 31 set from chunk 7
    for lay in TOPS + FUSED:
        assert lay.cs % 16 == 0 and lay.ss % 16 == 0 and lay.base % 16 == 0
        assert G4 - 16 - 16 * lay.n < (lay.n - 1) * lay.cs + lay.len <= G4 - 16
    for lay in (STRADDLE, FUSED[0]):
        assert lay.cs <= 1 << 31 < lay.cs + lay.len  # chunk 1 covers byte 2^31 of the stripe
        assert G4 - 32 <= 2 * lay.cs + lay.len <= G4 - 16
    assert 2 * STRADDLE.cs + STRADDLE.len == G4 - 16
    assert 5 * BYTES.cs + BYTES.len == G4 - 1 and BYTES.cs == 858992638  # the largest layout the contract accepts
    assert BYTES.cs % 16 and BYTES.ss % 16 and BYTES.base % 16
    assert all(lay.len % 256 == 0 for lay in FUSED)
    assert NBYTES == (1 << 31) + 2 * SS + (1 << 20)


@functools.lru_cache(maxsize=None)
def coded(n, k, length):
    """Two coded stripes [2][n][length] from the host oracle, computed once and read-only."""
    data = fill_bytes(2 * k * length, 1000003 * n + 10007 * k + length).reshape(2, k * length)
    code = np.stack([oracle.rs_encode(n, k, data[s], length) for s in range(2)])
    code.setflags(write=False)
    return code


def md5(a):
    return np.frombuffer(hashlib.md5(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


class Wide:
    """The module's buffer with the windows of one case: what was uploaded and what the call must leave."""

    def __init__(self, ctx, buf):
        self.ctx, self.buf = ctx, buf
        self.want = {}

    def reset(self):
        self.buf.memset(FILL)
        self.want = {}
        return self

    def put(self, off, data):
        """Upload a window; unless expect() says otherwise the call must leave it as it is."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        self.buf.upload(data, off)
        self.want[off] = data

    def hole(self, off, length):
        """A window that stays 0xEE before the call."""
        self.want[off] = np.full(length, FILL, dtype=np.uint8)

    def expect(self, off, data):
        assert off in self.want and len(self.want[off]) == len(data)
        self.want[off] = np.ascontiguousarray(data, dtype=np.uint8)

    def spans(self):
        """The windows with their margins, 8-byte aligned and merged: [(begin, end)] ascending."""
        out = []
        for off in sorted(self.want):
            a = max(0, (off - MARGIN) // 8 * 8)
            b = min(self.buf.nbytes, (off + len(self.want[off]) + MARGIN + 7) // 8 * 8)
            if out and a <= out[-1][1]:
                out[-1] = (out[-1][0], max(b, out[-1][1]))
            else:
                out.append((a, b))
        return out

    def gap_sums(self):
        sums, at = [], 0
        for a, b in self.spans() + [(self.buf.nbytes, self.buf.nbytes)]:
            if a > at:
                sums.append((at, a, self.buf.checksum(a - at, at)))
            at = b
        assert sum(b - a for a, b, _ in sums) + sum(b - a for a, b in self.spans()) == self.buf.nbytes
        return sums

    def snapshot(self):
        """Just before the call: the checksum of everything outside the windows, the guard included."""
        self.before = self.gap_sums()

    def verify(self, what=""):
        """After the call: every window and its margins byte for byte, every gap by checksum."""
        self.ctx.sync()
        for a, b in self.spans():
            image = np.full(b - a, FILL, dtype=np.uint8)
            for off, data in self.want.items():
                if a <= off < b:
                    image[off - a: off - a + len(data)] = data
            got = self.buf.download(b - a, a)
            if not np.array_equal(got, image):
                i = int(np.flatnonzero(got != image)[0])
                pytest.fail(f"{what}: first differing byte at buffer offset {a + i} (batch offset {a + i - BASE}, "
                            f"{(a + i - BASE) % SS} past its stripe): got {got[i]:#04x}, want {image[i]:#04x}")
        after = self.gap_sums()
        for (a, b, s0), (_, _, s1) in zip(self.before, after):
            assert s0 == s1, f"{what}: bytes outside the windows changed in [{a}, {b}) of the buffer"


@pytest.fixture(scope="module")
def wide(gpu_ctx):
    import torch

    free = torch.cuda.mem_get_info(0)[0]
    if free < 12 << 30:
        pytest.skip(f"{free >> 20} MiB of device memory free, the wide-layout buffer needs 12 GiB")
    buf = nxec.DeviceBuffer(NBYTES)
    yield Wide(gpu_ctx, buf)
    buf.free()


@pytest.fixture(scope="module", autouse=True)
def launch_record():
    nxec.launch_log(True)
    yield
    nxec.launch_log(False)


def put_stripes(w, lay, chunks, skip=()):
    """Upload chunks [2][*][len] at the layout's places; (s, c) in `skip` stays 0xEE."""
    for s in range(2):
        for c in range(chunks.shape[1]):
            if (s, c) in skip:
                w.hole(lay.off(s, c), lay.len)
            else:
                w.put(lay.off(s, c), chunks[s, c])


def expect_stripes(w, lay, chunks):
    for s in range(2):
        for c in range(chunks.shape[1]):
            w.expect(lay.off(s, c), chunks[s, c])


def erasure_sets(n, k):
    """Erasures with the first and the last chunk: together where n - k allows two, else one after the other."""
    return [[0, n - 1]] if n - k >= 2 else [[0], [n - 1]]


def alive_maps(n, k):
    """Stripe 0 loses chunks {0, n-1} ({0} where n - k == 1: two would be lost for good), stripe 1 loses chunk k."""
    a = np.ones((2, n), dtype=np.uint8)
    a[0, [0, n - 1] if n - k >= 2 else [0]] = 0
    a[1, k] = 0
    return a


def lost(alive):
    return {(s, c) for s in range(alive.shape[0]) for c in range(alive.shape[1]) if not alive[s, c]}


def small(nbytes, data=None):
    b = nxec.DeviceBuffer(nbytes + 64)
    b.memset(FILL)
    if data is not None:
        b.upload(data)
    return b


def packed_equal(buf, want, what):
    got = buf.download()
    want = np.ascontiguousarray(want).reshape(-1)
    assert np.array_equal(got[:want.size], want), f"{what}: first differing byte {int(np.flatnonzero(got[:want.size] != want)[0])}"
    assert (got[want.size:] == FILL).all(), f"{what}: bytes past the packed result changed"


# the full tile of a one-row pass goes to k_mul_perm and its ragged rest to k_mul_vec
ENCODE_PATHS = {"top-5-4": {"k_mul_perm", "k_mul_vec"}, "top-24-21": {"k_mul_vec_dyn"}, "bytes": {"k_mul_bytes"}}


@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_encode(wide, lay):
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    w = wide.reset()
    put_stripes(w, lay, code, skip={(s, c) for s in range(2) for c in range(k, n)})
    w.snapshot()
    nxec.launch_log_read()
    w.ctx.rs_encode(n, k, w.buf.ptr + lay.base, lay.cs, lay.ss, lay.len, 2)
    recs = nxec.launch_log_read()
    fams = {r["family"] for r in recs}
    # the code paths the geometries are here for
    assert ENCODE_PATHS.get(lay.name, {"k_mul_vec"}) <= fams, recs
    if lay.name == "top-12-6":
        assert {r["rows"] for r in recs} == {4, 2}, recs  # six rows: two passes
    expect_stripes(w, lay, code)
    w.verify("rs_encode")


@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_recover_in_place(wide, lay):
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    for failed in erasure_sets(n, k):
        w = wide.reset()
        put_stripes(w, lay, code, skip={(s, c) for s in range(2) for c in failed})
        w.snapshot()
        w.ctx.rs_recover(n, k, failed, w.buf.ptr + lay.base, lay.cs, lay.ss, lay.len, 2)
        expect_stripes(w, lay, code)
        w.verify(f"rs_recover {failed}")


@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_decode_wide_source_into_packed_output(wide, lay):
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    for failed in erasure_sets(n, k):
        w = wide.reset()
        put_stripes(w, lay, code, skip={(s, c) for s in range(2) for c in failed})
        out = small(2 * k * lay.len)
        w.snapshot()
        w.ctx.rs_decode(n, k, failed, w.buf.ptr + lay.base, lay.cs, lay.ss, out.ptr, lay.len, k * lay.len, lay.len, 2)
        w.verify(f"rs_decode {failed}: the source")
        packed_equal(out, code[:, :k], f"rs_decode {failed}")
        out.free()


@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_decode_packed_source_into_wide_output(wide, lay):
    """The copy-through form: surviving data chunks pass through to copy offsets near the top."""
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    olay = Layout(lay.name + "-out", k, k, lay.len, lay.out_stride(), lay.ss, lay.base)
    for failed in erasure_sets(n, k):
        src_img = code.copy()
        src_img[:, failed] = FILL
        src = small(2 * n * lay.len, src_img)
        w = wide.reset()
        put_stripes(w, olay, code[:, :k], skip={(s, c) for s in range(2) for c in range(k)})
        w.snapshot()
        w.ctx.rs_decode(n, k, failed, src.ptr, lay.len, n * lay.len, w.buf.ptr + olay.base, olay.cs, olay.ss, lay.len, 2)
        expect_stripes(w, olay, code[:, :k])
        w.verify(f"rs_decode {failed}: the output")
        packed_equal(src, src_img, "the packed source")
        src.free()


@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_scrub(wide, lay):
    """Clean; then one flipped byte at the last byte of the last chunk, in stripe 0 and then in stripe 1: detected,
    located, healed, clean again."""
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    CLEAN, UNLOC = nxec.SCRUB_CLEAN, nxec.SCRUB_UNLOCATED
    base, args = wide.buf.ptr + lay.base, (lay.cs, lay.ss, lay.len, 2)
    w = wide.reset()
    put_stripes(w, lay, code)
    w.snapshot()
    st, nbad = w.ctx.rs_scrub(n, k, base, *args)
    assert st.tolist() == [CLEAN, CLEAN] and nbad == 0
    located = n - 1 if n - k >= 2 else UNLOC  # one parity byte per column cannot say which chunk is wrong
    for s in range(2):
        bad = code[s, n - 1].copy()
        bad[-1] ^= 0x5A
        w.put(lay.off(s, n - 1), bad)
        want = [CLEAN, CLEAN]
        want[s] = UNLOC
        st, nbad = w.ctx.rs_scrub(n, k, base, *args)
        assert st.tolist() == want and nbad == 1, "detect"
        want[s] = located
        st, nbad = w.ctx.rs_scrub(n, k, base, *args, flags=nxec.SCRUB_LOCATE)
        assert st.tolist() == want and nbad == 1, "locate"
        w.verify(f"scrub detect and locate, stripe {s}")  # neither writes into the batch
        st, nbad = w.ctx.rs_scrub(n, k, base, *args, flags=nxec.SCRUB_REPAIR)
        assert st.tolist() == want and nbad == 1, "repair"
        if n - k >= 2:
            w.expect(lay.off(s, n - 1), code[s, n - 1])
        else:
            w.put(lay.off(s, n - 1), code[s, n - 1])  # nothing could be healed: put the byte back
        w.verify(f"scrub repair, stripe {s}")
        st, nbad = w.ctx.rs_scrub(n, k, base, *args)
        assert st.tolist() == [CLEAN, CLEAN] and nbad == 0
    w.verify("scrub")


@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_recover_mixed(wide, lay):
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    alive = alive_maps(n, k)
    w = wide.reset()
    put_stripes(w, lay, code, skip=lost(alive))
    w.snapshot()
    nxec.launch_log_read()
    res = w.ctx.rs_recover_mixed(n, k, alive, w.buf.ptr + lay.base, lay.cs, lay.ss, lay.len, 2)
    assert res.tolist() == [int((alive[s] == 0).sum()) for s in range(2)]
    fams = {r["family"] for r in nxec.launch_log_read()}
    one_launch = k <= 19 and lay.base % 16 == 0
    assert ("k_mul_mixed" in fams) == one_launch, fams  # (24,21) and the byte layout go by runs
    expect_stripes(w, lay, code)
    w.verify("rs_recover_mixed")


@pytest.mark.parametrize("wide_side", ["source", "output"])
@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_decode_mixed(wide, lay, wide_side):
    """Each stripe around its own erased chunks, and a clean map (the decode's pure-copy segment); the wide side is
    the source (packed output) or the output (packed source, out_chunk_stride by the same rule with k for n)."""
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    olay = Layout(lay.name + "-out", k, k, lay.len, lay.out_stride(), lay.ss, lay.base)
    for alive in (alive_maps(n, k), np.ones((2, n), dtype=np.uint8)):
        w = wide.reset()
        src_img = code.copy()
        for s, c in lost(alive):
            src_img[s, c] = FILL
        if wide_side == "source":
            put_stripes(w, lay, code, skip=lost(alive))
            other = small(2 * k * lay.len)
            call = (w.buf.ptr + lay.base, lay.cs, lay.ss, other.ptr, lay.len, k * lay.len)
        else:
            put_stripes(w, olay, code[:, :k], skip={(s, c) for s in range(2) for c in range(k)})
            other = small(2 * n * lay.len, src_img)
            call = (other.ptr, lay.len, n * lay.len, w.buf.ptr + olay.base, olay.cs, olay.ss)
        w.snapshot()
        nxec.launch_log_read()
        res = w.ctx.rs_decode_mixed(n, k, alive, *call, lay.len, 2)
        assert res.tolist() == [int((alive[s, :k] == 0).sum()) for s in range(2)]
        fams = {r["family"] for r in nxec.launch_log_read()}
        assert ("k_decode_mixed" in fams) == (k <= 19 and lay.base % 16 == 0), fams
        if wide_side == "source":
            w.verify("rs_decode_mixed: the source")
            packed_equal(other, code[:, :k], "rs_decode_mixed")
        else:
            expect_stripes(w, olay, code[:, :k])
            w.verify("rs_decode_mixed: the output")
            packed_equal(other, src_img, "the packed source")
        other.free()


@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_update(wide, lay):
    """Three updates: a range that ends at the last byte of data chunk k-1 (16-aligned where the layout is), five
    unaligned bytes in chunk 0, and a whole chunk of stripe 1.  Data and parity against the oracle's re-encode."""
    n, k, L, code = lay.n, lay.k, lay.len, coded(lay.n, lay.k, lay.len)
    ups = [(0, k - 1, L - 4096, 4096), (0, 0, 3, 5), (1, k // 2, 0, L)]
    new = fill_bytes(sum(u[3] for u in ups) + 64, 77 + n).copy()
    # every update's new bytes aligned like its offset in the chunk (a vector body needs that)
    places, at = [], 0
    for s, c, off, ln in ups:
        at = (at + 15) // 16 * 16 + off % 16
        places.append(at)
        at += ln
    d_new = small(at, new[:at])
    data = code[:, :k].copy()
    for (s, c, off, ln), p in zip(ups, places):
        data[s, c, off:off + ln] = new[p:p + ln]
    want = np.stack([oracle.rs_encode(n, k, data[s].reshape(-1), L) for s in range(2)])
    w = wide.reset()
    put_stripes(w, lay, code)
    w.snapshot()
    w.ctx.rs_update(n, k, w.buf.ptr + lay.base, lay.cs, lay.ss, L, 2,
                    [(s, c, off, ln, d_new.ptr + p) for (s, c, off, ln), p in zip(ups, places)])
    expect_stripes(w, lay, want)
    w.verify("rs_update")
    packed_equal(d_new, new[:at], "the new bytes")
    d_new.free()


@pytest.mark.parametrize("lay", LAYOUTS, ids=repr)
def test_md5_chunks_and_verify(wide, lay):
    n, code = lay.n, coded(lay.n, lay.k, lay.len)
    want = np.stack([md5(code[s, c]) for s in range(2) for c in range(n)])
    w = wide.reset()
    put_stripes(w, lay, code)
    dig, ok, nb = small(2 * n * 16), small(2 * n), small(8, np.zeros(8, dtype=np.uint8))
    w.snapshot()
    w.ctx.md5_chunks(w.buf.ptr + lay.base, lay.cs, lay.ss, n, lay.len, 2, dig.ptr)
    w.ctx.sync()
    packed_equal(dig, want, "md5_chunks")
    exp = want.copy()
    exp[2 * n - 1, 0] ^= 1  # the digest on record for the last chunk of stripe 1 is another one
    dig.upload(exp)
    w.ctx.md5_verify_chunks(w.buf.ptr + lay.base, lay.cs, lay.ss, n, lay.len, 2, dig.ptr, ok.ptr, nb.ptr)
    w.verify("md5_chunks and md5_verify_chunks")
    packed_equal(ok, np.array([1] * (2 * n - 1) + [0], dtype=np.uint8), "md5_verify_chunks")
    assert int(nb.download(8).view(np.uint64)[0]) == 1
    for b in (dig, ok, nb):
        b.free()


def fused_records():
    recs = nxec.launch_log_read()
    assert [r["family"] for r in recs] == ["k_mul_md5"] and recs[0]["product"] == 1, recs
    return recs[0]


@pytest.mark.parametrize("lay", FUSED, ids=repr)
def test_fused_encode_md5(wide, lay):
    """Parity and digests from the fused kernel against the oracle and hashlib, and against the two-kernel path
    (rs_encode, then md5_chunks) on the same buffer."""
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    want = np.stack([md5(code[s, c]) for s in range(2) for c in range(n)])
    base = wide.buf.ptr + lay.base
    dig = small(2 * n * 16)
    for fused in (True, False):
        w = wide.reset()
        dig.memset(FILL)
        put_stripes(w, lay, code, skip={(s, c) for s in range(2) for c in range(k, n)})
        w.snapshot()
        nxec.launch_log_read()
        if fused:
            w.ctx.rs_encode_md5(n, k, base, lay.cs, lay.ss, lay.len, 2, dig.ptr)
            assert fused_records()["hsrc"] == 1
        else:
            w.ctx.rs_encode(n, k, base, lay.cs, lay.ss, lay.len, 2)
            w.ctx.md5_chunks(base, lay.cs, lay.ss, n, lay.len, 2, dig.ptr)
        expect_stripes(w, lay, code)
        w.verify("rs_encode_md5" if fused else "rs_encode + md5_chunks")
        packed_equal(dig, want, "digests, " + ("fused" if fused else "two kernels"))
    dig.free()


@pytest.mark.parametrize("lay", FUSED, ids=repr)
def test_fused_recover_md5(wide, lay):
    n, k, code = lay.n, lay.k, coded(lay.n, lay.k, lay.len)
    base = wide.buf.ptr + lay.base
    for failed in erasure_sets(n, k):
        want = np.stack([md5(code[s, c]) for s in range(2) for c in failed])
        dig = small(2 * len(failed) * 16)
        for fused in (True, False):
            w = wide.reset()
            dig.memset(FILL)
            put_stripes(w, lay, code, skip={(s, c) for s in range(2) for c in failed})
            w.snapshot()
            nxec.launch_log_read()
            if fused:
                w.ctx.rs_recover_md5(n, k, failed, base, lay.cs, lay.ss, lay.len, 2, dig.ptr)
                assert fused_records()["hsrc"] == 0
            else:
                w.ctx.rs_recover(n, k, failed, base, lay.cs, lay.ss, lay.len, 2)
                for r, c in enumerate(failed):  # digest (s, r) at (s*nfailed + r)*16: one launch per rebuilt chunk
                    one = small(2 * 16)
                    w.ctx.md5_chunks(base + c * lay.cs, lay.cs, lay.ss, 1, lay.len, 2, one.ptr)
                    w.ctx.sync()
                    d = one.download(32).reshape(2, 16)
                    for s in range(2):
                        dig.upload(d[s], (s * len(failed) + r) * 16)
                    one.free()
            expect_stripes(w, lay, code)
            w.verify(f"rs_recover_md5 {failed}" if fused else f"rs_recover + md5_chunks {failed}")
            packed_equal(dig, want, f"digests {failed}, " + ("fused" if fused else "two kernels"))
        dig.free()


def refused(w, call, what):
    """`call` gives NXEC_ERR_INVALID, launches nothing and changes no byte of the buffer."""
    w.snapshot()
    nxec.launch_log_read()
    with pytest.raises(nxec.NxecError) as e:
        call()
    assert e.value.code == INVALID, what
    assert nxec.launch_log_read() == [], what
    w.verify(what)


@pytest.mark.parametrize("extra", [0, 16], ids=["len-256s", "len-plus-16"])
def test_fused_encode_md5_refuses_a_chunk_that_ends_past_4gib(wide, extra):
    """RS(20,16), one stripe, data chunk 15 at 2^32 - 256 with 512-byte chunks: the chunk starts below 2^32 and
    ends above it.  The fused kernel used to take this layout (only the chunk starts were checked) and add the
    second step's 256 to the chunk offset in 32 bits, which reads chunk 0's bytes; the two-kernel path (len + 16)
    always refused it.  Both refuse it now."""
    n, k, L, cs = 20, 16, 512 + extra, 286331136
    assert 15 * cs == G4 - 256 and BASE + 19 * cs + L <= NBYTES
    data = fill_bytes(k * L, 2016).reshape(k, L)
    w = wide.reset()
    for c in range(n):
        w.put(BASE + c * cs, data[c]) if c < k else w.hole(BASE + c * cs, L)
    dig = small(n * 16)
    refused(w, lambda: w.ctx.rs_encode_md5(n, k, w.buf.ptr + BASE, cs, SS, L, 1, dig.ptr), "rs_encode_md5 RS(20,16)")
    packed_equal(dig, np.zeros(0, dtype=np.uint8), "the digests")
    dig.free()


@pytest.mark.parametrize("extra", [0, 16], ids=["len-256s", "len-plus-16"])
def test_fused_recover_md5_refuses_a_chunk_that_ends_past_4gib(wide, extra):
    """RS(17,16), failed = [16], chunk 16 at 2^32 - 512 with 768-byte chunks: the rebuilt chunk would end past 2^32."""
    n, k, L, cs = 17, 16, 768 + extra, 268435424
    assert 16 * cs == G4 - 512
    data = fill_bytes(k * L, 1716).reshape(k, L)
    w = wide.reset()
    for c in range(n):
        w.put(BASE + c * cs, data[c]) if c < k else w.hole(BASE + c * cs, L)
    dig = small(16)
    refused(w, lambda: w.ctx.rs_recover_md5(n, k, [16], w.buf.ptr + BASE, cs, SS, L, 1, dig.ptr), "rs_recover_md5 RS(17,16)")
    packed_equal(dig, np.zeros(0, dtype=np.uint8), "the digests")
    dig.free()
