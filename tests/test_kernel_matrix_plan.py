"""The kernel matrix's plan (tests/kernel_matrix.py), checked without a device:
its constants against the kernel sources, the expected set against the sizes
the dispatch tables imply, every generated case against that set, and the
reference side alone at the shapes tests/test_gpu_kernel_matrix.py runs."""
import numpy as np
import pytest

import kernel_matrix as km
import oracle
from nexoedge_amd import nxec


@pytest.mark.parametrize("name", sorted(km.SOURCE_CONSTANTS))
def test_constants_mirror_the_sources(name):
    assert km.source_constant(name) == km.SOURCE_CONSTANTS[name][1]


def test_use_perm_exclusion_matches_the_source():
    """The model's single excluded instantiation is the one use_perm() names."""
    with open(km.os.path.join(km.CSRC, "nxec_kernels.hip")) as f:
        src = f.read()
    assert "if (k == 11 && !gather) return false;" in src
    assert [(k, g) for k in range(1, km.PERM_MAX_K + 1) for g in (False, True)
            if not km.use_perm(k, 1, True, False, g)] == [(11, False)]
    assert not km.use_perm(km.PERM_MAX_K + 1, 1, True, False, True)
    assert not km.use_perm(4, 2, True, False, False) and not km.use_perm(4, 1, False, False, False)
    assert not km.use_perm(4, 1, True, True, False)


def test_queue_and_prefetch_thresholds():
    assert [km.default_r(k) for k in (9, 10)] == [16, 8]
    assert km.vec_queued(19, 8) and not km.vec_queued(20, 8)  # k = 20: the tables fill the LDS, static tile order
    assert km.vec_prefetch(10, False, True) and not km.vec_prefetch(11, False, True)
    assert km.vec_prefetch(8, True, True) and not km.vec_prefetch(9, True, True)
    assert km.vec_prefetch(8, False, False) and not km.vec_prefetch(9, False, False)
    assert [km.tiles_per_grab(k, r, c) for k, r, c in ((1, 1, 0), (1, 4, 0), (10, 4, 0), (19, 4, 0), (8, 4, 2))] == \
        [6, 3, 1, 1, 1]
    assert [km.scrub_prefetch(kd + r, True) for kd, r in km.d_queue_cases()] == [True, False]


def test_expected_set_has_the_size_the_tables_imply():
    want = km.expected_instantiations()
    count = {}
    for inst in want:
        count[inst[0]] = count.get(inst[0], 0) + 1
    # k_files_md5<1, MASK, !TSTORE> is unreachable: a one-chunk last stripe has no partial chunk to mask
    assert km.UNREACHABLE == {("k_files_md5", 1, 1, 0)}
    assert count == {"k_mul_vec": 120, "k_mul_perm": 25, "k_mul_vec_dyn": 2, "k_mul_bytes": 2, "k_scrub_vec": 128,
                     "k_mul_ragged": 19, "k_mul_md5": 40, "k_gather_md5": 32, "k_files_md5": 48 - 1}
    assert len(want) == 120 + 25 + 2 + 2 + 128 + 19 + 40 + 32 + 48 - len(km.UNREACHABLE)


def test_every_case_maps_into_the_expected_set_and_covers_it():
    want = km.expected_instantiations()
    seen = set()
    for group, insts in km.all_cases():
        for inst in insts:
            assert inst in want | km.UNREACHABLE, (group, inst)
            seen.add(inst)
    assert seen - km.UNREACHABLE == want, sorted(want - seen)


def test_group_a_reaches_every_multiply_instantiation():
    seen = {km.inst_of(r) for c in km.a_cases() for r in km.a_plan(c)}
    want = {i for i in km.expected_instantiations() if i[0] in ("k_mul_vec", "k_mul_perm", "k_mul_vec_dyn", "k_mul_bytes")}
    assert seen == want
    ids = [km.case_id(c) for c in km.a_cases()]
    assert len(set(ids)) == len(ids)
    # the regular shape: a complete tile, a ragged launch of 3 vectors, a 5-byte tail
    plan = km.a_plan(dict(form="strided", k=10, rows=4, length=km.A_LEN, base=0))
    assert [p["family"] for p in plan] == ["k_mul_vec", "k_mul_vec", "k_mul_bytes"]
    assert [p["full"] for p in plan] == [1, 0, 0] and plan[2]["byte_begin"] == km.TILE + 48


def test_group_b_shapes_and_plans():
    for case in km.b_cases():
        plan = km.b_plan(case)
        assert len(plan) == 1 and plan[0]["full"] == 1, case
        t = km.tiles_per_grab(case["k"], case["rows"], km.b_copies(case))
        assert plan[0]["tpg"] == t
        for cus in (1, 64, 256, 304):
            ns = km.b_stripes(case, cus)
            assert ns * (km.B_CS // km.TILE) >= 4 * cus * t > (ns - 1) * (km.B_CS // km.TILE)
    fams = {(c["form"], c["k"], c["rows"]): km.b_plan(c)[0]["family"] for c in km.b_cases()}
    assert fams[("strided", 11, 1)] == "k_mul_vec" and fams[("gather", 11, 1)] == "k_mul_perm"
    assert all(f == "k_mul_perm" for (form, k, rows), f in fams.items() if rows == 1 and (form, k) != ("strided", 11))


def test_coefficients_force_the_special_values():
    for rows in (1, 4, 6):
        for k in (1, 2, 3, 4, 11, 20, 24):
            c = km.coefficients(rows, k, 5)
            assert c.shape == (rows, k)
            if k >= 3:
                assert all({0, 1, 0xFF} <= set(c[r].tolist()) for r in range(rows))
    assert np.array_equal(km.coefficients(4, 10, 9), km.coefficients(4, 10, 9))


@pytest.mark.parametrize("case", km.b_cases(), ids=km.case_id)
def test_references_agree_on_the_queue_shapes(case):
    """oracle.simd_encode (the reference of the large shapes) equals the plain-C oracle.matmul on the
    coefficients, chunk length and data stream of every (b) case: its first and last stripe for 256 CUs."""
    k, rows, cs, seed = case["k"], case["rows"], km.B_CS, km.b_seed(case)
    coeffs = km.coefficients(rows, k, seed)
    ns = km.b_stripes(case, 256)
    for s in (0, ns - 1):
        data = oracle.fill_bytes_at(np.empty(k * cs, dtype=np.uint8), seed, s * k * cs).reshape(k, cs)
        outs = [np.empty(cs, dtype=np.uint8) for _ in range(rows)]
        oracle.simd_encode(coeffs, [data[j] for j in range(k)], outs)
        want = oracle.matmul(coeffs, [data[j] for j in range(k)])
        assert all(np.array_equal(outs[r], want[r]) for r in range(rows))
    if case["k"] == 1 and case["rows"] == 1:
        assert np.array_equal(oracle.fill_bytes(4096, seed)[1024:2048],
                              oracle.fill_bytes_at(np.empty(1024, dtype=np.uint8), seed, 1024))


@pytest.mark.parametrize("kd,rows", km.d_cases())
def test_scrub_flips_change_the_oracle_syndrome(kd, rows):
    """Every flip of group (d) leaves a non-zero syndrome byte under the oracle's arithmetic, and with two
    or more parity rows the host rule names the flipped chunk."""
    n, length = kd + rows, km.D_LEN
    rng = np.random.default_rng(500 + 10 * kd + rows)
    stripe = oracle.rs_encode(n, kd, rng.integers(0, 256, size=kd * length, dtype=np.uint8), length)
    enc = oracle.gen_rs_matrix(n, kd)[kd:]

    def syndrome(st, pos):
        par = oracle.matmul(enc, [st[j, pos: pos + 1] for j in range(kd)])
        return [int(par[r][0] ^ st[kd + r, pos]) for r in range(rows)]

    for c in km.d_flip_chunks(kd, rows):
        for i, pos in enumerate(km.D_FLIP_POS):
            assert pos < length and (pos < km.TILE) == (i == 0)
            assert not any(syndrome(stripe, pos))
            bad = stripe.copy()
            bad[c, pos] ^= 1 << (c % 8)
            syn = syndrome(bad, pos)
            assert any(syn), (c, pos)
            chunk, _ = nxec.syndrome_locate(n, kd, syn)
            assert chunk == (c if rows >= 2 else nxec.SCRUB_UNLOCATED), (c, pos, syn)


def test_launch_record_is_off_by_default_and_reads_empty():
    assert nxec.launch_log_read() == []
    nxec.launch_log(True)
    try:
        assert nxec.launch_log_read() == []
    finally:
        nxec.launch_log(False)
    buf = nxec.C.create_string_buffer(4)
    assert nxec.lib.nxec_debug_launch_log_read(buf, 4) == 0 and buf.value == b""
