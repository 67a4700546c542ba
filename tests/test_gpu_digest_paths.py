"""The digest paths on the device, bit-exact against hashlib's MD5 and the oracle's coding.

  * k_md5 over the digest matrix (tests/digest_matrix.py): every length of three periods of the aligned
    ring at every chunk alignment, plain and in verify mode;
  * nxec_rs_recover_md5_stripes with more rebuilt chunks than one MD5 launch has regions;
  * each condition of the fused / two-kernel rule (mul_md5_layout_ok), both sides of its edge through
    nxec_rs_encode_md5_stripes and nxec_rs_recover_md5_stripes, with the launch record naming the side.

The plain MD5 launches are not in the launch record; what the record shows here is which multiply kernels ran.
"""
import functools
import hashlib

import numpy as np
import pytest

import digest_matrix as dm
import oracle
from helpers import fill_bytes
from nexoedge_amd import nxec

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE
EMPTY_MD5 = hashlib.md5(b"").digest()


def md5(a):
    return np.frombuffer(hashlib.md5(a).digest(), dtype=np.uint8)


# ------------------------------------------------------ the digest matrix
@functools.lru_cache(maxsize=None)
def _matrix(layout):
    """(host bytes of the one buffer every length reuses, hashlib digests [length][lane][16]); read-only."""
    host = fill_bytes(dm.buffer_bytes(layout), 20240 + dm.LAYOUTS.index(layout))
    view = memoryview(host)
    want = np.empty((len(dm.LENGTHS), dm.LANES, 16), dtype=np.uint8)
    for i, length in enumerate(dm.LENGTHS):
        cs, ss = dm.strides(layout, length)
        want[i] = np.frombuffer(b"".join(
            hashlib.md5(view[s * ss + c * cs:s * ss + c * cs + length]).digest()
            for s in range(dm.NSTRIPES) for c in range(dm.NCHUNKS)), dtype=np.uint8).reshape(dm.LANES, 16)
    host.setflags(write=False)
    want.setflags(write=False)
    return host, want


def _slots(raw, first, slot, nbytes):
    """The per-length slices of a downloaded buffer: (payload [length][nbytes], guard [length][slot - nbytes])."""
    a = raw[first:first + len(dm.LENGTHS) * slot].reshape(len(dm.LENGTHS), slot)
    return a[:, :nbytes], a[:, nbytes:]


def _first_difference(layout, got, want):
    i, lane = (int(x[0]) for x in np.nonzero((got != want).any(axis=-1)))
    length = dm.LENGTHS[i]
    return f"length {length} lane {lane}: {dm.path(dm.chunk_offset(layout, length, lane), length)}"


@pytest.mark.parametrize("layout", dm.LAYOUTS)
def test_md5_every_length_and_alignment(gpu_ctx, layout):
    """One nxec_md5_chunks call per length over the same random buffer (a chunk's neighbours are random bytes,
    so a stray byte read into a digest shows); every digest equals hashlib's, every guard keeps its fill."""
    host, want = _matrix(layout)
    buf = nxec.DeviceBuffer(host.nbytes)
    dig = nxec.DeviceBuffer(dm.digest_bytes())
    try:
        buf.upload(host)
        dig.memset(SENTINEL)
        for length in dm.LENGTHS:
            cs, ss = dm.strides(layout, length)
            gpu_ctx.md5_chunks(buf.ptr, cs, ss, dm.NCHUNKS, length, dm.NSTRIPES,
                               dig.ptr + dm.digest_offset(layout, length))
        gpu_ctx.sync()
        raw = dig.download()
        assert np.array_equal(buf.download(), host)
    finally:
        buf.free()
        dig.free()
    first = dm.digest_offset(layout, dm.LENGTHS[0])
    got, guards = _slots(raw, first, dm.DIGEST_SLOT, dm.LANES * 16)
    got = got.reshape(len(dm.LENGTHS), dm.LANES, 16)
    assert np.array_equal(got, want), _first_difference(layout, got, want)
    assert (guards == SENTINEL).all(), np.nonzero((guards != SENTINEL).any(axis=1))[0][:8]
    assert (raw[:first] == SENTINEL).all() and (raw[first + len(dm.LENGTHS) * dm.DIGEST_SLOT:] == SENTINEL).all()


@pytest.mark.parametrize("layout", dm.LAYOUTS)
def test_md5_verify_every_length_and_alignment(gpu_ctx, layout):
    """The same matrix through nxec_md5_verify_chunks: hashlib's digests as the expected ones, one bit flipped
    in a third of them (every byte position of a digest in turn).  ok is 0 exactly there and 1 elsewhere, the
    counter -- zeroed once -- ends at the number of altered lanes, and the expected digests are not written."""
    host, want = _matrix(layout)
    nl = len(dm.LENGTHS)
    lanes = np.arange(dm.LANES)[None, :] + np.asarray(dm.LENGTHS)[:, None]  # lane + length
    bad = lanes % 3 == 0
    assert all(bad[i, lane] == dm.altered(lane, length) and lanes[i, lane] % 16 == dm.altered_byte(lane, length)
               for i, length in ((0, dm.LENGTHS[0]), (nl - 1, dm.LENGTHS[-1])) for lane in range(dm.LANES))
    exp = want.copy()
    li, la = np.nonzero(bad)
    exp[li, la, lanes[li, la] % 16] ^= (1 << (lanes[li, la] % 8)).astype(np.uint8)
    first = dm.digest_offset(layout, dm.LENGTHS[0])
    exp_raw = np.full(dm.digest_bytes(), SENTINEL, dtype=np.uint8)
    exp_raw[first:first + nl * dm.DIGEST_SLOT].reshape(nl, dm.DIGEST_SLOT)[:, :dm.LANES * 16] = exp.reshape(nl, -1)
    buf = nxec.DeviceBuffer(host.nbytes)
    dig = nxec.DeviceBuffer(exp_raw.nbytes)
    ok = nxec.DeviceBuffer(nl * dm.OK_SLOT)
    nbad = nxec.DeviceBuffer(8)
    try:
        buf.upload(host)
        dig.upload(exp_raw)
        ok.memset(0x77)
        nbad.memset(0)
        for i, length in enumerate(dm.LENGTHS):
            cs, ss = dm.strides(layout, length)
            gpu_ctx.md5_verify_chunks(buf.ptr, cs, ss, dm.NCHUNKS, length, dm.NSTRIPES,
                                      dig.ptr + dm.digest_offset(layout, length), ok.ptr + i * dm.OK_SLOT, nbad.ptr)
        gpu_ctx.sync()
        ok_raw = ok.download()
        count = int(nbad.download().view(np.uint64)[0])
        assert np.array_equal(dig.download(), exp_raw)  # verify mode reads the digests, never writes them
    finally:
        for b in (buf, dig, ok, nbad):
            b.free()
    flags, guards = _slots(ok_raw, 0, dm.OK_SLOT, dm.LANES)
    expect = np.where(bad, 0, 1).astype(np.uint8)
    assert np.array_equal(flags, expect), _first_difference(layout, flags[..., None], expect[..., None])
    assert (guards == 0x77).all()
    assert count == int(bad.sum())


# --------------------------------------- coded batches with sentinel padding
def _coded_batch(n, k, length, cs, ss, ns, base, seed):
    """(host image of a buffer of base + ns * ss + 16 bytes holding the oracle's encode of seeded data, sentinel
    everywhere else; the chunks [ns][n][length])."""
    data = fill_bytes(ns * k * length, seed).reshape(ns, k * length)
    image = np.full(base + ns * ss + 16, SENTINEL, dtype=np.uint8)
    chunks = np.zeros((ns, n, length), dtype=np.uint8)
    for s in range(ns):
        if length:
            chunks[s] = oracle.rs_encode(n, k, data[s], length).reshape(n, length)
        for c in range(n):
            o = base + s * ss + c * cs
            image[o:o + length] = chunks[s, c]
    return image, chunks


def _erase(image, ids, length, cs, ss, ns, base):
    out = image.copy()
    for s in range(ns):
        for c in ids:
            o = base + s * ss + c * cs
            out[o:o + length] = SENTINEL
    return out


def _digests(chunks, ids):
    ns = chunks.shape[0]
    return np.stack([md5(chunks[s, c].tobytes()) for s in range(ns) for c in ids]).reshape(ns, len(ids), 16)


def _run_md5_call(gpu_ctx, call, n, k, failed, image, start, length, cs, ss, ns, base):
    """Uploads `start`, runs the call with the launch record read around it; returns (records, buffer,
    digests [ns][hashed chunks][16]) after checking the digest guard."""
    nh = n if call == "rs_encode_md5" else len(failed)
    buf = nxec.DeviceBuffer(image.nbytes)
    dig = nxec.DeviceBuffer(ns * nh * 16 + 16)
    try:
        buf.upload(start)
        dig.memset(SENTINEL)
        nxec.launch_log_read()
        if call == "rs_encode_md5":
            gpu_ctx.rs_encode_md5(n, k, buf.ptr + base, cs, ss, length, ns, dig.ptr)
        else:
            gpu_ctx.rs_recover_md5(n, k, failed, buf.ptr + base, cs, ss, length, ns, dig.ptr)
        gpu_ctx.sync()
        recs = nxec.launch_log_read()
        got, draw = buf.download(), dig.download()
    finally:
        buf.free()
        dig.free()
    assert (draw[ns * nh * 16:] == SENTINEL).all(), "digest guard"
    return recs, got, draw[:ns * nh * 16].reshape(ns, nh, 16)


def _families(recs):
    return [r["family"] for r in recs]


def _is_multiply(family):
    return family.startswith("k_mul_") and family != "k_mul_md5"


@pytest.mark.parametrize("length", [768, 1000])
@pytest.mark.parametrize("n,k,failed", [(10, 4, [1, 4, 6, 8, 9]), (10, 4, [0, 2, 3, 5, 7, 9]),
                                        (12, 6, [1, 2, 3, 4, 5, 6])])
def test_recover_md5_more_failures_than_regions(gpu_ctx, n, k, failed, length):
    """More rebuilt chunks than kMaxMd5Regions: recover, then one MD5 launch per four rebuilt chunks -- the
    second starts at rebuilt chunk 4, its digests 4 * 16 bytes into a stripe's, its stripes nfailed * 16 apart."""
    assert len(failed) > dm.MAX_MD5_REGIONS and len(failed) > dm.MAX_ROWS
    ns, cs, base = 9, dm.rup(length) + 16, 0
    ss = n * cs + 16
    image, chunks = _coded_batch(n, k, length, cs, ss, ns, base, 5100 + n + length + len(failed))
    start = _erase(image, failed, length, cs, ss, ns, base)
    nxec.launch_log(True)
    try:
        recs, got, dig = _run_md5_call(gpu_ctx, "rs_recover_md5", n, k, failed, image, start, length, cs, ss, ns, base)
    finally:
        nxec.launch_log(False)
    assert np.array_equal(got, image)  # every chunk rebuilt, all padding intact
    assert np.array_equal(dig, _digests(chunks, failed))
    fam = _families(recs)
    assert "k_mul_md5" not in fam and any(map(_is_multiply, fam)), fam


def _boundary_cases(call):
    """(id, n, k, length, base offset, chunk stride or None for rup16(length) + 16, fused)."""
    n, k = 6, 4
    cases = [(f"len{length}", n, k, length, 0, None, True) for length in (256, 512)]
    cases += [(f"len{length}", n, k, length, 0, None, False) for length in (0, 1, 16, 240, 272)]
    cases += [("base+16", n, k, 512, 16, None, True), ("base+8", n, k, 512, 8, None, False),
              ("stride520", n, k, 512, 0, 520, False),
              ("k20", 24, 20, 512, 0, None, True), ("k21", 25, 21, 512, 0, None, False)]
    if call == "rs_encode_md5":
        cases += [("p4", 14, 10, 512, 0, None, True), ("p5", 15, 10, 512, 0, None, False)]
    return cases


@pytest.mark.parametrize("call", ["rs_encode_md5", "rs_recover_md5"])
def test_fused_boundaries(gpu_ctx, call):
    """Both sides of each condition of mul_md5_layout_ok give the oracle's bytes and hashlib's digests; the
    launch record names the side: one k_mul_md5 line and no other multiply, or multiply lines and no k_mul_md5."""
    assert (dm.ENC_MD5_STEP, dm.ENC_MD5_MAX_K, dm.MAX_ROWS) == (256, 20, 4)  # the edges the cases sit on
    ns = 5
    nxec.launch_log(True)
    try:
        for name, n, k, length, base, cs, fused in _boundary_cases(call):
            cs = cs or dm.rup(length) + 16
            ss = n * cs
            image, chunks = _coded_batch(n, k, length, cs, ss, ns, base, 6200 + n + length + base + cs)
            if call == "rs_encode_md5":
                failed, hashed = None, list(range(n))
                start = _erase(image, range(k, n), length, cs, ss, ns, base)
            else:
                failed = hashed = [1, n - 1]
                start = _erase(image, failed, length, cs, ss, ns, base)
            recs, got, dig = _run_md5_call(gpu_ctx, call, n, k, failed, image, start, length, cs, ss, ns, base)
            fam = _families(recs)
            if fused:
                assert fam == ["k_mul_md5"], (name, fam)
            else:
                assert "k_mul_md5" not in fam, (name, fam)
                assert length == 0 or any(map(_is_multiply, fam)), (name, fam)
            assert np.array_equal(got, image), name  # coded / rebuilt bytes, and every padding byte
            if length == 0:
                assert all(bytes(d) == EMPTY_MD5 for d in dig.reshape(-1, 16)), name
            else:
                assert np.array_equal(dig, _digests(chunks, hashed)), name
    finally:
        nxec.launch_log(False)
