"""Agent service, fused form (k_gather_md5): nxec_agent_encode_batch codes and
hashes each batch in one kernel straight from and into pinned host memory.
Inputs / outputs that are arena (pinned, device-mapped) buffers are used in
place; pageable or misaligned ones go through the staging slot.  Every shape
the agent sends (container_manager.cc:221-258 partial encodes, agent.cc:240-415
CAR / non-CAR repairs) and every buffer mix is checked bit-exactly against the
oracle's CodingUtils::encode and hashlib MD5 (agent.cc:342)."""
import ctypes as C
import hashlib
import zlib

import numpy as np
import pytest

import oracle
from nexoedge_amd import _lib, nxec

lib = _lib.lib


class Arena:
    """nxec_host_alloc blocks viewed as numpy arrays (the agent's Chunk buffers)."""

    def __init__(self):
        self.blocks = []

    def array(self, nbytes, offset=0):
        p = C.c_void_p()
        nxec.check(lib.nxec_host_alloc(nbytes + offset, C.byref(p)), "nxec_host_alloc")
        self.blocks.append(p.value)
        return np.ctypeslib.as_array((C.c_ubyte * nbytes).from_address(p.value + offset))

    def free(self):
        for b in self.blocks:
            lib.nxec_host_free(C.c_void_p(b))
        self.blocks = []


def make_buf(arena, kind, cs, i):
    if kind == "pageable":
        return np.zeros(cs, dtype=np.uint8)
    if kind == "arena":
        return arena.array(cs)
    if kind == "misaligned":  # inside a pinned block but not 16-byte aligned: staged
        return arena.array(cs, offset=8)
    return make_buf(arena, ("arena", "pageable", "misaligned")[i % 3], cs, i)  # mixed


def run_batch(gpu_ctx, shapes, cs, in_kind, out_kind, nreq, seed, with_md5=lambda r: True, batch_bytes=0):
    rng = np.random.default_rng(seed)
    arena = Arena()
    reqs, want = [], []
    try:
        for r in range(nreq):
            ni, no = shapes[r % len(shapes)]
            m = rng.integers(0, 256, size=(no, ni), dtype=np.uint8)
            ins = []
            for j in range(ni):
                a = make_buf(arena, in_kind, cs, r * 7 + j)
                a[:] = rng.integers(0, 256, size=cs, dtype=np.uint8)
                ins.append(a)
            outs = [make_buf(arena, out_kind, cs, r * 5 + o) for o in range(no)]
            for o in outs:
                o[:] = 0xEE
            md5 = np.zeros((no, 16), dtype=np.uint8) if with_md5(r) else None
            reqs.append((m, ins, outs, md5))
            want.append(oracle.matmul(m, [x.copy() for x in ins]))
        gpu_ctx.agent_encode_batch(reqs, cs, batch_bytes)
        for r, ((m, ins, outs, md5), w) in enumerate(zip(reqs, want)):
            for o in range(m.shape[0]):
                assert np.array_equal(outs[o], w[o]), (r, o)
                if md5 is not None:
                    assert md5[o].tobytes().hex() == hashlib.md5(w[o].tobytes()).hexdigest(), (r, o)
    finally:
        arena.free()


# (ninputs, noutputs): ENC partial encodes of racks of 1-4 chunks, CAR XOR of
# G partials, non-CAR repairs of 1-4 lost chunks from k = 10 / 12 / 16 inputs
SHAPES = [(4, 1), (3, 1), (1, 1), (2, 1), (12, 2), (10, 4), (16, 4), (16, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("in_kind,out_kind", [("pageable", "pageable"), ("arena", "arena"), ("arena", "pageable"),
                                              ("mixed", "mixed"), ("misaligned", "arena")])
def test_agent_fused_buffer_kinds(gpu_ctx, in_kind, out_kind):
    for ni_no in SHAPES:
        run_batch(gpu_ctx, [ni_no], 65536, in_kind, out_kind, nreq=5, seed=zlib.crc32(repr((in_kind, out_kind, ni_no)).encode()))


@pytest.mark.gpu
@pytest.mark.parametrize("cs", [256, 4096, 1 << 20])
def test_agent_fused_chunk_sizes_and_grouping(gpu_ctx, cs):
    """Interleaved shapes (one launch per matrix group), the smallest step
    (256 B), 1 MiB chunks; requests without a digest pointer in a hashed group."""
    nreq = 24 if cs == 1 << 20 else 60
    run_batch(gpu_ctx, SHAPES[:4], cs, "mixed", "mixed", nreq=nreq, seed=cs, with_md5=lambda r: r % 5 != 3)


@pytest.mark.gpu
def test_agent_fused_many_requests_packed_per_workgroup(gpu_ctx):
    """More requests than CUs: several per workgroup (S > 1) and a partial last
    workgroup; a small batch_bytes splits them over rotating staging slots."""
    run_batch(gpu_ctx, [(4, 1)], 4096, "arena", "arena", nreq=1100, seed=17)
    run_batch(gpu_ctx, [(3, 1), (12, 2)], 8192, "pageable", "arena", nreq=700, seed=18, batch_bytes=3 << 20)


@pytest.mark.gpu
@pytest.mark.parametrize("cs", [1, 15, 16, 17, 100, 255, 257, 319, 5000, 65536 + 16, (1 << 20) - 3])
def test_agent_fused_any_chunk_size(gpu_ctx, cs):
    """Chunk sizes that are not a multiple of the 256-byte step (a file's last
    stripe, ceil(rem/k) bytes): the partial last step reads and writes nothing
    past a chunk's end -- every output sits in a larger buffer whose bytes past
    cs must keep their sentinel -- and the MD5 padding is built in registers."""
    rng = np.random.default_rng(cs)
    arena = Arena()
    try:
        reqs, want, guards = [], [], []
        for r in range(6):
            ni, no = [(4, 1), (12, 2), (3, 1)][r % 3]
            m = rng.integers(0, 256, size=(no, ni), dtype=np.uint8)
            ins = []
            for j in range(ni):
                a = make_buf(arena, ("arena", "pageable")[(r + j) % 2], cs, r)
                a[:] = rng.integers(0, 256, size=cs, dtype=np.uint8)
                ins.append(a)
            outs, g = [], []
            for o in range(no):
                big = arena.array(cs + 64) if (r + o) % 2 == 0 else np.zeros(cs + 64, dtype=np.uint8)
                big[:] = 0xEE
                outs.append(big[:cs])
                g.append(big)
            md5 = np.zeros((no, 16), dtype=np.uint8)
            reqs.append((m, ins, outs, md5))
            want.append(oracle.matmul(m, [x.copy() for x in ins]))
            guards.append(g)
        gpu_ctx.agent_encode_batch(reqs, cs)
        for r, ((m, ins, outs, md5), w, g) in enumerate(zip(reqs, want, guards)):
            for o in range(m.shape[0]):
                assert np.array_equal(outs[o], w[o]), (r, o)
                assert md5[o].tobytes().hex() == hashlib.md5(w[o].tobytes()).hexdigest(), (r, o)
                assert (g[o][cs:] == 0xEE).all(), (r, o)  # nothing written past the chunk
    finally:
        arena.free()


@pytest.mark.gpu
@pytest.mark.parametrize("in_kind,out_kind", [("arena", "arena"), ("pageable", "pageable"), ("mixed", "mixed"),
                                              ("misaligned", "arena")])
@pytest.mark.parametrize("cs", [65536, 65536 + 16, 5000, 1])
def test_agent_without_digests_zero_copy(gpu_ctx, in_kind, out_kind, cs):
    """Groups that want no digest (ENC_CHUNK_REQ: getEncodedChunks computes
    none) run the gather form of the multiply kernel over the same pointer
    tables -- mapped buffers in place, the others through the slot."""
    run_batch(gpu_ctx, SHAPES, cs, in_kind, out_kind, nreq=10, seed=cs + 7, with_md5=lambda r: False)


# ----------------------------------------------------------------------------
# The staged form with digests (H2D -> multiply -> k_md5 -> D2H): what a group
# takes with more than kGatherMd5MaxK (16) inputs, more than kMaxRowsPerPass (4)
# outputs, or with zero copy switched off (NXEC_HOST_DIRECT=0).

def run_digest_batch(gpu_ctx, shapes, cs, in_kind, out_kind, nreq, seed, hash_inputs, batch_bytes=0,
                     without_md5=lambda r: False):
    """One nxec_agent_encode_batch call of `nreq` requests cycling through `shapes`; the requests of a shape
    share its matrix, so they form one group and travel in batches of several.  Outputs are the first cs bytes
    of larger sentinel-filled buffers and the digest arrays carry a sentinel row behind them.  Checks outputs
    against the oracle, output and input digests against hashlib, and that nothing past cs or past the digests
    was written.  Returns the call's launch record."""
    rng = np.random.default_rng(seed)
    arena = Arena()
    mats = {sh: rng.integers(0, 256, size=(sh[1], sh[0]), dtype=np.uint8) for sh in dict.fromkeys(shapes)}
    reqs, want, guards = [], [], []
    try:
        for r in range(nreq):
            ni, no = shapes[r % len(shapes)]
            ins = []
            for j in range(ni):
                a = make_buf(arena, in_kind, cs, r * 7 + j)
                a[:] = rng.integers(0, 256, size=cs, dtype=np.uint8)
                ins.append(a)
            big = [make_buf(arena, out_kind, cs + 64, r * 5 + o) for o in range(no)]
            for b in big:
                b[:] = 0xEE
            md5 = None if without_md5(r) else np.full((no + 1, 16), 0xEE, dtype=np.uint8)
            md5_in = np.full((ni + 1, 16), 0xEE, dtype=np.uint8) if hash_inputs else None
            reqs.append((mats[(ni, no)], ins, [b[:cs] for b in big], md5[:no] if md5 is not None else None,
                         md5_in[:ni] if md5_in is not None else None))
            want.append(oracle.matmul(mats[(ni, no)], [x.copy() for x in ins]))
            guards.append((big, md5, md5_in))
        nxec.launch_log(True)
        try:
            gpu_ctx.agent_encode_batch(reqs, cs, batch_bytes)
            recs = nxec.launch_log_read()
        finally:
            nxec.launch_log(False)
        for r, ((m, ins, outs, _, _), w, (big, md5, md5_in)) in enumerate(zip(reqs, want, guards)):
            for o in range(m.shape[0]):
                assert np.array_equal(outs[o], w[o]), (r, o)
                assert (big[o][cs:] == 0xEE).all(), (r, o)  # nothing written past the chunk
                if md5 is not None:
                    assert md5[o].tobytes() == hashlib.md5(w[o].tobytes()).digest(), (r, o)
            if md5 is not None:
                assert (md5[-1] == 0xEE).all(), r
            if md5_in is not None:
                for j in range(m.shape[1]):
                    assert md5_in[j].tobytes() == hashlib.md5(ins[j].tobytes()).digest(), (r, "input", j)
                assert (md5_in[-1] == 0xEE).all(), r
        return recs
    finally:
        arena.free()


def gather_shapes(recs):
    return [(r["k"], r["p"]) for r in recs if r["family"] == "k_gather_md5"]


@pytest.mark.gpu
@pytest.mark.parametrize("hash_inputs", [False, True])
@pytest.mark.parametrize("cs", [1, 255, 256, 5000, 65536 + 16])
def test_agent_staged_with_digests(gpu_ctx, cs, hash_inputs):
    """Shapes past the fused kernel's limits (more than 16 inputs, more than 4 outputs, both): the staged form,
    whose MD5 launch hashes the outputs alone or -- with md5_inputs -- two regions, the inputs' digests first
    in a request's digest row and the outputs' behind them.  A request without an md5 pointer shares the batch
    when the inputs are not hashed."""
    for ni, no in [(17, 1), (20, 4), (4, 5), (4, 6), (20, 6)]:
        recs = run_digest_batch(gpu_ctx, [(ni, no)], cs, "mixed", "mixed", nreq=5,
                                seed=zlib.crc32(repr((ni, no, cs, hash_inputs)).encode()), hash_inputs=hash_inputs,
                                without_md5=lambda r: not hash_inputs and r == 2)
        fam = [r["family"] for r in recs]
        assert "k_gather_md5" not in fam and any(f.startswith("k_mul_") for f in fam), ((ni, no), fam)


@pytest.mark.gpu
@pytest.mark.parametrize("hash_inputs", [False, True])
def test_agent_round_mixing_fused_and_staged_groups(gpu_ctx, hash_inputs):
    """One call whose groups alternate between the fused form ((4, 1), (16, 4)) and the staged form ((17, 1),
    (4, 5)), split into many batches: the three rotating slots are each handed from one form to the other."""
    shapes = [(4, 1), (17, 1), (4, 5), (16, 4)]
    cs, per_shape, batch_bytes = 8192, 6, 100000
    # the staged groups alone: (ni + no) * cs exceeds half of batch_bytes for both, so one request per batch
    assert all((ni + no) * cs > batch_bytes // 2 for ni, no in ((17, 1), (4, 5)))
    recs = run_digest_batch(gpu_ctx, shapes, cs, "mixed", "mixed", nreq=per_shape * len(shapes), seed=4100 + hash_inputs,
                            hash_inputs=hash_inputs, batch_bytes=batch_bytes)
    gathered = gather_shapes(recs)
    assert set(gathered) == {(4, 1), (16, 4)}, gathered  # the two narrow shapes only
    staged = [r for r in recs if r["family"] != "k_gather_md5"]
    assert {r["k"] for r in staged} == {17, 4} and all(r["family"].startswith("k_mul_") for r in staged), staged
    assert len(gathered) + 2 * per_shape >= 7  # batches of the round: every slot is used at least twice
    # groups run in key order (4, 1), (4, 5), (16, 4), (17, 1): fused, staged, fused, staged
    form = ["F" if r["family"] == "k_gather_md5" else "S" for r in recs]
    runs = [f for i, f in enumerate(form) if i == 0 or form[i - 1] != f]
    assert runs == ["F", "S", "F", "S"], runs


@pytest.mark.gpu
@pytest.mark.parametrize("hash_inputs", [False, True])
@pytest.mark.parametrize("kind", ["arena", "pageable"])
@pytest.mark.parametrize("cs", [5000, 65536])
def test_agent_staged_when_zero_copy_is_off(gpu_ctx, monkeypatch, cs, kind, hash_inputs):
    """NXEC_HOST_DIRECT=0 (a deployment setting, read at every call): every shape takes the staged form, and
    outputs and digests come back by a plain device-to-host copy instead of the copy kernel."""
    monkeypatch.setenv("NXEC_HOST_DIRECT", "0")
    for ni_no in SHAPES:
        recs = run_digest_batch(gpu_ctx, [ni_no], cs, kind, kind, nreq=5,
                                seed=zlib.crc32(repr((ni_no, cs, kind, hash_inputs)).encode()), hash_inputs=hash_inputs)
        fam = [r["family"] for r in recs]
        assert "k_gather_md5" not in fam and any(f.startswith("k_mul_") for f in fam), (ni_no, fam)
