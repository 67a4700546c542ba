"""Delta update on the GPU (nxec_rs_update_stripes): byte ranges of data chunks
are overwritten and the parity follows by c(r,j) * (new ^ old).

Method: encode a fill_random batch and keep its host copy; build the expected
image on the host (data bytes patched with numpy, the parity of every touched
stripe from the plain-C oracle); upload the new bytes to a separate device
buffer that is random elsewhere and compared afterwards (d_new is only read);
call; download the whole batch buffer and compare it whole, which checks
untouched stripes and stride padding too; check the launch record against
rs_update_plan's counters.  Every comparison is bit-exact.

Shapes, the smallest that reach each way the kernel can go wrong:
  geometry (6,4)    R = 16, prefetch
           (5,4)    one parity row: the short pass
           (14,10)  four rows, R = 8
           (10,4)   six rows: two passes, the new data stored by the second only
           (23,19)  the widest vector shape
           (24,21)  k > 19: byte kernel only
  len      16 (one vector), 16384 (one full tile), 16384 + 16, 3 * 16384 + 48;
           4096 + 5 reaches the byte kernel through the layout (packed chunks
           are not 16-byte aligned) and, at an aligned stride, through tails
  strides  packed, chunk_stride = len + 48, stripe_stride padded by one chunk
  ranges   whole chunk, first and last vector, one byte, head only, head and
           one vector, head + a full tile + tail, head + 1025 vectors + tail,
           a full tile off the chunk's start, an empty range, and a d_new
           that is off by 4 bytes (the whole update by bytes)
"""
import ctypes as C
import json

import numpy as np
import pytest

import oracle
from nexoedge_amd import _lib, nxec

pytestmark = pytest.mark.gpu

TILE = 16384
LENS = [16, 16384, 16384 + 16, 3 * 16384 + 48]
GEOMETRIES = [(6, 4), (5, 4), (14, 10), (10, 4), (23, 19), (24, 21)]


def rup(x, m=16):
    return (x + m - 1) // m * m


def strides(n, length):
    """(chunk stride, stripe stride): packed, padded chunks, stripes padded by one chunk"""
    return [(length, n * length), (length + 48, n * (length + 48)), (length, (n + 1) * length)]


@pytest.fixture(scope="module", autouse=True)
def launch_record():
    nxec.launch_log(True)
    yield
    nxec.launch_log(False)


class Batch:
    """An encoded [ns][n] batch on the device and its host image."""

    def __init__(self, ctx, n, k, length, ns, off=0, cs=None, ss=None, seed=3):
        self.ctx, self.n, self.k, self.len, self.ns, self.off = ctx, n, k, length, ns, off
        self.cs = cs if cs is not None else length
        self.ss = ss if ss is not None else n * self.cs
        self.buf = nxec.DeviceBuffer(off + ns * self.ss + 16)
        self.buf.fill_random(seed + 977 * n + length)
        ctx.rs_encode(n, k, self.buf.ptr + off, self.cs, self.ss, length, ns)
        ctx.sync()
        self.image = self.buf.download()

    @property
    def ptr(self):
        return self.buf.ptr + self.off

    def free(self):
        self.buf.free()

    def at(self, s, c):
        return self.off + s * self.ss + c * self.cs

    def plan(self, ups):
        return nxec.rs_update_plan(self.n, self.k, self.cs, self.ss, self.len, self.ns, self.ptr, ups)

    def expected(self, image, specs, new):
        """`image` with the updates' bytes patched in and the parity of every touched stripe encoded afresh."""
        want = image.copy()
        for (s, c, off, ln, _), nb in zip(specs, new):
            want[self.at(s, c) + off: self.at(s, c) + off + ln] = nb
        for s in sorted({u[0] for u in specs if u[3] > 0}):
            data = np.concatenate([want[self.at(s, j): self.at(s, j) + self.len] for j in range(self.k)])
            if self.n > self.k:
                st = oracle.rs_encode(self.n, self.k, data, self.len)
                for r in range(self.k, self.n):
                    want[self.at(s, r): self.at(s, r) + self.len] = st[r]
        return want


class NewBytes:
    """The new bytes of a list of (stripe, chunk, offset, length, shift) in one device buffer that is random
    everywhere: update i reads `length` bytes at a 64-byte slot + offset % 16 + shift (shift 0: the body's
    vectors are 16-byte aligned in d_new, 4: they are not)."""

    def __init__(self, specs, seed):
        pos, at = [], 64
        for _, _, off, ln, shift in specs:
            pos.append(at + off % 16 + shift)
            at = rup(at + off % 16 + shift + ln, 64) + 64
        self.host = np.random.default_rng(seed).integers(0, 256, at, dtype=np.uint8)
        self.dev = nxec.DeviceBuffer(at)
        self.dev.upload(self.host)
        self.new = [self.host[p: p + u[3]] for p, u in zip(pos, specs)]
        self.ups = [(s, c, off, ln, self.dev.ptr + p) for (s, c, off, ln, _), p in zip(specs, pos)]

    def untouched(self):
        return np.array_equal(self.dev.download(), self.host)

    def free(self):
        self.dev.free()


def check_records(recs, n, k, plan, tag):
    """The launch record of one call against the plan's counters: per round and per pass of <= 4 parity rows
    the vector launch, then the byte launch; `last` on the last pass only."""
    nrounds, ntiles, nitems = plan
    passes = max(1, -(-(n - k) // 4))
    assert all(r["family"] in ("k_update_vec", "k_update_bytes") for r in recs), (tag, recs)
    vec = [r for r in recs if r["family"] == "k_update_vec"]
    byt = [r for r in recs if r["family"] == "k_update_bytes"]
    assert sum(r["tiles"] for r in vec if r["pass"] == 0) == ntiles, (tag, recs)
    assert sum(r["items"] for r in byt if r["pass"] == 0) == nitems, (tag, recs)
    assert {r["round"] for r in recs} == set(range(nrounds)), (tag, recs)
    key = [(r["round"], r["pass"], r["family"] == "k_update_bytes") for r in recs]
    assert key == sorted(set(key)), (tag, key)  # stream order, nothing twice
    for r in recs:
        assert r["k"] == k and r["rows"] == min(4, n - k - 4 * r["pass"]), (tag, r)
        assert r["last"] == int(r["pass"] == passes - 1), (tag, r)
        same = [q for q in recs if q["round"] == r["round"] and q["family"] == r["family"]]
        assert [q["pass"] for q in same] == list(range(passes)), (tag, same)  # every pass over the same work
        assert len({q.get("tiles", q.get("items")) for q in same}) == 1, (tag, same)
    for r in vec:
        assert k <= 19 and r["r"] == (16 if k <= 9 else 8) and r["pf"] == 1 and r["q"] == 1, (tag, r)
        assert 1 <= r["grid"] <= r["tiles"] and r["updates"] >= 1, (tag, r)


def run(b, specs, tag, seed=7):
    """One call over `specs` [(stripe, chunk, offset, length, shift)]: whole-buffer comparison, d_new
    untouched, launch record; returns (records, plan).  b.image follows the batch."""
    nb = NewBytes(specs, seed)
    try:
        plan = b.plan(nb.ups)
        want = b.expected(b.image, specs, nb.new)
        nxec.launch_log_read()
        b.ctx.rs_update(b.n, b.k, b.ptr, b.cs, b.ss, b.len, b.ns, nb.ups)
        b.ctx.sync()
        recs = nxec.launch_log_read()
        got = b.buf.download()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            first = int(bad[0]) - b.off
            pytest.fail(f"{tag}: {bad.size} bytes differ, first in stripe {first // b.ss} at stripe byte {first % b.ss} "
                        f"(chunk stride {b.cs}, len {b.len})")
        assert nb.untouched(), tag
        check_records(recs, b.n, b.k, plan, tag)
        b.image = want
        return recs, plan
    finally:
        nb.free()


def range_specs(k, length, ns):
    """The update ranges of the module docstring that fit `length`, one per stripe, chunks in turn."""
    ranges = [(0, length, 0), (0, 16, 0), (length - 16, 16, 0), (5, 1, 0), (5, 11, 0), (5, 27, 0),
              (3, 16384 + 20, 0), (3, 16384 + 40, 0), (16, 16384, 0), (7, 0, 0), (16, min(length - 16, 4096), 4),
              (0, length, 4)]
    fit = [r for r in ranges if r[0] >= 0 and r[0] + r[1] <= length and (r[1] > 0 or r[0] == 7)]
    assert len(fit) <= ns
    return [(i, (i * 3 + 1) % k, off, ln, shift) for i, (off, ln, shift) in enumerate(fit)]


NS = 12


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("n,k", GEOMETRIES)
def test_geometries(gpu_ctx, n, k, length):
    specs = range_specs(k, length, NS)
    for cs, ss in strides(n, length):
        b = Batch(gpu_ctx, n, k, length, NS, cs=cs, ss=ss)
        try:
            recs, plan = run(b, specs, (n, k, length, cs, ss))
            assert plan[0] == 1  # one update per stripe: one round
            if k > 19:
                assert plan[1] == 0 and all(r["family"] == "k_update_bytes" for r in recs)
            else:
                assert plan[1] > 0 and any(r["family"] == "k_update_vec" for r in recs)
            if (n, k) == (10, 4):  # six rows: the new data goes out with the second pass only
                assert [(r["pass"], r["rows"], r["last"]) for r in recs if r["family"] == "k_update_vec"] == [(0, 4, 0), (1, 2, 1)]
            if (n, k) == (5, 4):
                assert all(r["rows"] == 1 and r["last"] == 1 for r in recs)
        finally:
            b.free()


@pytest.mark.parametrize("off,cs", [(0, 4096 + 5), (0, rup(4096 + 5)), (3, rup(4096 + 5)), (0, 4096 + 5 + 48)])
@pytest.mark.parametrize("n,k", [(6, 4), (14, 10), (10, 4), (24, 21)])
def test_unaligned_layouts_and_tails(gpu_ctx, n, k, off, cs):
    """len = 4096 + 5: packed chunks or a base offset of 3 leave no vector work; at an aligned stride the
    bodies run in the vector kernel and the chunk's last 5 bytes as tails."""
    length = 4096 + 5
    specs = range_specs(k, length, NS) + [(NS - 1, k - 1, length - 21, 21, 0), (NS - 2, 0, length - 5, 5, 0)]
    b = Batch(gpu_ctx, n, k, length, NS, off=off, cs=cs)
    try:
        recs, plan = run(b, specs, (n, k, off, cs))
        vec = k <= 19 and off % 16 == 0 and cs % 16 == 0
        assert (plan[1] > 0) == vec and plan[2] > 0
        if not vec:
            assert plan[2] == sum(1 for u in specs if u[3] > 0)
    finally:
        b.free()


def test_n_equals_k_overwrites_data_only(gpu_ctx):
    n = k = 4
    length = 16384 + 16
    b = Batch(gpu_ctx, n, k, length, 4, cs=length + 48)
    try:
        recs, _ = run(b, [(0, 0, 0, length, 0), (1, 3, 5, 27, 0), (2, 2, 3, 16384 + 5, 0), (3, 1, 16, 160, 4)], "n == k")
        assert all(r["rows"] == 0 and r["last"] == 1 and r["pass"] == 0 for r in recs) and recs
    finally:
        b.free()


@pytest.mark.parametrize("n,k", GEOMETRIES)
def test_interactions(gpu_ctx, n, k):
    length, ns = 16384 + 16, 5
    b = Batch(gpu_ctx, n, k, length, ns, cs=length + 48, ss=(n + 1) * (length + 48))
    try:
        # chunks 0 and k-1 of one stripe over the same columns: two rounds, both applied
        _, plan = run(b, [(1, 0, 32, 4096, 0), (1, k - 1, 32, 4096, 0)], (n, k, "same columns"))
        assert plan[0] == 2
        # two updates on different chunks that split one 16-byte vector at byte 8
        _, plan = run(b, [(2, 0, 64, 40, 0), (2, 1, 104, 56, 0)], (n, k, "split vector"), seed=8)
        assert plan[0] == 1
        # ... and that meet in one column of that vector
        _, plan = run(b, [(2, 0, 64, 41, 0), (2, 1, 104, 56, 0)], (n, k, "one shared column"), seed=9)
        assert plan[0] == 2
        # adjacent same-chunk ranges
        _, plan = run(b, [(3, 2, 0, 100, 0), (3, 2, 100, 16384 - 100, 0), (3, 2, 16384, 16, 0)], (n, k, "adjacent"), seed=10)
        assert plan[0] == 1
        # all k chunks of a stripe over the whole length: k rounds, a fresh encode of the new data
        _, plan = run(b, [(0, j, 0, length, 0) for j in range(k)], (n, k, "all chunks"), seed=11)
        assert plan[0] == k
        # updates only in the last stripe, up to its last byte (their columns meet in 16384 .. 16395)
        _, plan = run(b, [(ns - 1, 1, 3, 16384 + 9, 0), (ns - 1, 0, 16384, 16, 0)], (n, k, "last stripe"), seed=12)
        assert plan[0] == 2
    finally:
        b.free()


def test_empty_work_launches_nothing(gpu_ctx):
    b = Batch(gpu_ctx, 6, 4, 4096, 3)
    nb = NewBytes([(0, 0, 0, 16, 0)], 1)
    try:
        nxec.launch_log_read()
        gpu_ctx.rs_update(6, 4, b.ptr, b.cs, b.ss, b.len, b.ns, [])
        gpu_ctx.rs_update(6, 4, b.ptr, b.cs, b.ss, b.len, b.ns, [(0, 1, 5, 0, nb.dev.ptr), (2, 3, 4096, 0, None)])
        gpu_ctx.sync()
        assert nxec.launch_log_read() == []
        assert np.array_equal(b.buf.download(), b.image)
        with pytest.raises(_lib.NxecError):  # d_new inside the batch
            gpu_ctx.rs_update(6, 4, b.ptr, b.cs, b.ss, b.len, b.ns, [(0, 1, 0, 16, b.ptr + 4096)])
        with pytest.raises(_lib.NxecError):  # same-chunk intersection
            gpu_ctx.rs_update(6, 4, b.ptr, b.cs, b.ss, b.len, b.ns, [(0, 1, 0, 16, nb.dev.ptr), (0, 1, 15, 1, nb.dev.ptr)])
        gpu_ctx.sync()
        assert nxec.launch_log_read() == [] and np.array_equal(b.buf.download(), b.image)
    finally:
        nb.free()
        b.free()


def test_queue_steady_state(gpu_ctx):
    """(6,4), one 16384-byte update per stripe over at least 4 x CUs x tiles-per-grab stripes: one tile per
    update, so most tiles come from published grabs."""
    n, k, length = 6, 4, TILE
    grid = json.loads(gpu_ctx.describe_launch(2, k, length, 8))["cus"]
    ns = 4 * grid * 2
    b = Batch(gpu_ctx, n, k, length, ns, seed=9)
    try:
        recs, plan = run(b, [(s, (s * 7 + s // 5) % k, 0, length, 0) for s in range(ns)], ("queue", ns))
        assert plan == (1, ns, 0) and len(recs) == 1
        m = recs[0]
        assert m["grid"] == grid and m["tiles"] == ns >= 4 * m["grid"] * m["tpg"]
    finally:
        b.free()


def test_syndrome_is_preserved(gpu_ctx):
    """A stripe that is not a codeword keeps its syndrome: one flipped parity byte in one stripe, one flipped
    data byte in another, updates over those columns on other chunks of the same stripes.  The expected
    image is the re-encode of the patched data with the two flips XORed back in, and the scrub names the
    same chunks before and after."""
    n, k, length, ns = 10, 4, 16384 + 16, 4
    b = Batch(gpu_ctx, n, k, length, ns, cs=length + 48)
    try:
        flips = [(b.at(1, k + 4) + 1000, 0x5A), (b.at(2, 1) + 77, 0x81)]
        damaged = b.image.copy()
        for pos, x in flips:
            damaged[pos] ^= x
        b.buf.upload(damaged)
        before, nbad = gpu_ctx.rs_scrub(n, k, b.ptr, b.cs, b.ss, length, ns, nxec.SCRUB_LOCATE)
        assert before.tolist() == [nxec.SCRUB_CLEAN, k + 4, 1, nxec.SCRUB_CLEAN] and nbad == 2
        specs = [(1, 0, 992, 32, 0), (1, 3, 5, 16384, 0), (2, 0, 64, 32, 0), (2, 2, 70, 9, 0), (2, 3, 0, length, 0),
                 (3, 1, 0, 16, 0)]
        nb = NewBytes(specs, 21)
        try:
            want = b.expected(b.image, specs, nb.new)  # of the undamaged batch
            for pos, x in flips:
                want[pos] ^= x
            gpu_ctx.rs_update(n, k, b.ptr, b.cs, b.ss, length, ns, nb.ups)
            gpu_ctx.sync()
            assert np.array_equal(b.buf.download(), want)
        finally:
            nb.free()
        after, nbad = gpu_ctx.rs_scrub(n, k, b.ptr, b.cs, b.ss, length, ns, nxec.SCRUB_LOCATE)
        assert after.tolist() == before.tolist() and nbad == 2
    finally:
        b.free()


def fuzz_case(seed):
    rng = np.random.default_rng(4000 + seed)
    n, k = GEOMETRIES[seed % len(GEOMETRIES)]
    length = int(rng.choice(LENS + [4096 + 5]))
    cs = int(rng.choice([length, rup(length), rup(length) + 48]))
    ss = (n + int(rng.integers(0, 2))) * cs
    ns = 6
    sizes = [0, 1, 11, 16, 27, 100, 1024, 4096, 16384, 16384 + 20, length]
    specs, taken = [], {}
    want = int(rng.integers(1, 41))
    while len(specs) < want:  # rejection sampling: no two same-chunk ranges intersect
        s, c = int(rng.integers(ns)), int(rng.integers(k))
        ln = min(int(rng.choice(sizes)), length)
        off = int(rng.integers(length - ln + 1))
        if rng.random() < 0.4:
            off = off // 16 * 16
        if ln > 0 and any(off < o + l and o < off + ln for o, l in taken.get((s, c), [])):
            continue
        taken.setdefault((s, c), []).append((off, ln))
        specs.append((s, c, off, ln, 4 if rng.random() < 0.15 else 0))
    return n, k, length, cs, ss, ns, specs


@pytest.mark.parametrize("seed", range(24))
def test_seeded_fuzz(gpu_ctx, seed):
    n, k, length, cs, ss, ns, specs = fuzz_case(seed)
    b = Batch(gpu_ctx, n, k, length, ns, cs=cs, ss=ss, seed=seed)
    try:
        run(b, specs, ("fuzz", seed, n, k, length, cs, ss), seed=seed)
        run(b, specs[::-1], ("fuzz again", seed), seed=seed + 100)  # the same ranges over the updated batch
    finally:
        b.free()


def test_two_streams_and_update_list_reuse(gpu_ctx):
    """Two calls on two streams over disjoint stripe ranges of one buffer; each call's update array is
    overwritten as soon as the call returns, and the download follows both streams."""
    n, k, length, ns = 14, 10, 16384 + 16, 16
    b = Batch(gpu_ctx, n, k, length, ns, cs=length + 48)
    half = [[(s, (s * 3) % k, 3, 16384 + 9, 0) for s in range(0, ns // 2)] + [(1, 7, 100, 64, 0)],
            [(s, (s * 5) % k, 16, 16384, 0) for s in range(ns // 2, ns)] + [(ns - 1, 2, 0, 5, 0)]]
    sp = [C.c_void_p(), C.c_void_p()]
    nbs = []
    try:
        for p in sp:
            _lib.check(_lib.lib.nxec_stream_create(C.byref(p)), "nxec_stream_create")
        nbs = [NewBytes(h, 30 + i) for i, h in enumerate(half)]
        want = b.image
        for h, nb in zip(half, nbs):
            want = b.expected(want, h, nb.new)
        gpu_ctx.sync()
        for p, nb in zip(sp, nbs):
            arr, nu = nxec._update_list(nb.ups)
            _lib.check(_lib.lib.nxec_rs_update_stripes(C.c_void_p(gpu_ctx.ptr), n, k, C.c_void_p(b.ptr), b.cs, b.ss,
                                                       length, ns, arr, nu, p), "nxec_rs_update_stripes")
            C.memset(arr, 0xFF, C.sizeof(arr))  # the call has read it
        for p in sp:
            _lib.check(_lib.lib.nxec_stream_sync(p), "nxec_stream_sync")
        assert np.array_equal(b.buf.download(), want)
        assert all(nb.untouched() for nb in nbs)
    finally:
        for p in sp:
            if p:
                _lib.lib.nxec_stream_sync(p)
                _lib.lib.nxec_stream_destroy(p)
        for nb in nbs:
            nb.free()
        b.free()
