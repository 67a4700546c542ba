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
                     "k_mul_ragged": 19, "k_mul_md5": 40, "k_gather_md5": 32, "k_files_md5": 48 - 1,
                     "k_mul_mixed": 19, "k_decode_mixed": 19, "k_update_vec": 2}
    assert len(want) == 120 + 25 + 2 + 2 + 128 + 19 + 40 + 32 + 48 - len(km.UNREACHABLE) + 19 + 19 + 2 == 455


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


# ------------------------------------------------- groups (f), (g) and (h)
def alive_of(n, sets):
    a = np.ones((len(sets), n), dtype=np.uint8)
    for s, e in enumerate(sets):
        a[s, list(e)] = 0
    return a


def check_sets(n, k, sets, decode, lost=()):
    """Every stripe but the placed LOST ones is decodable under the oracle's arithmetic (so none is left out
    of the GPU comparison), and the Python plan model agrees with the library's host planner."""
    enc = oracle.gen_rs_matrix(n, k)
    for s, e in enumerate(sets):
        if s in lost:
            assert len(set(e)) > n - k
            continue
        assert len(set(e)) == len(e) <= n - k, (k, e)
        rc, _ = oracle.invert_matrix(enc[km.first_alive(n, k, e)])
        assert rc == 0, (n, k, e, "the first k alive rows of the generator do not invert")
    model = km.mixed_model(n, k, sets, decode)
    plan = (nxec.rs_decode_mixed_plan if decode else nxec.rs_recover_mixed_plan)(n, k, alive_of(n, sets))
    assert plan[0].tolist() == model["verdict"], (n, k, decode)
    assert plan[1:] == (model["plans"], model["segs"], model["stripes"]), (n, k, decode, plan[1:], model)
    assert [s for s, v in enumerate(model["verdict"]) if v < 0] == sorted(lost)
    assert len(model["order"]) >= model["stripes"] == len(set(model["order"]))
    return model


def holds(seq, sub):
    return any(seq[i: i + len(sub)] == sub for i in range(len(seq) - len(sub) + 1))


def test_mixed_model_constants_and_launch_plan():
    assert km.MIXED_LOST == nxec.RECOVER_LOST
    assert km.MAX_ROWS + 2 == km.MIXED_EXTRA  # plans of 5 and 6 erasures are the two-segment ones
    for k in range(1, km.RAGGED_MAX_K + 1):
        rec, dec = km.mixed_launch(k, False), km.mixed_launch(k, True)
        assert (rec["family"], dec["family"]) == ("k_mul_mixed", "k_decode_mixed")
        assert rec["rows"] == dec["rows"] == 4 and rec["q"] == dec["q"] == 1 and "full" not in rec
        assert rec["pf"] == dec["pf"] == int(k <= 8) and rec["r"] == dec["r"] == (16 if k <= 9 else 8)
        assert rec["tpg"] == km.tiles_per_grab(k, 4) and dec["tpg"] == km.tiles_per_grab(k, 0, k)
        assert km.queue_fits(k * 1024 * rec["r"])
    assert [km.mixed_launch(k, False)["tpg"] for k in km.G_KS] == [3, 1, 1, 1]
    assert [km.mixed_launch(k, True)["tpg"] for k in km.G_KS] == [6, 1, 1, 1]
    # the model on a hand-made batch of (10,4): decode shares one plan between every set with equal first k alive
    sets = [(), (9,), (0,), (0, 9), (0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5, 6)]
    m = km.mixed_model(10, 4, sets, False)
    assert (m["verdict"], m["plans"], m["seg_rows"]) == ([0, 1, 1, 2, 5, km.MIXED_LOST], 4, [1, 1, 2, 4, 1])
    assert m["order"] == [1, 2, 3, 4, 4] and m["stripes"] == 4
    m = km.mixed_model(10, 4, sets, True)
    assert (m["verdict"], m["plans"], m["seg_rows"]) == ([0, 0, 1, 1, 4, km.MIXED_LOST], 3, [0, 1, 4])
    assert m["order"] == [0, 1, 2, 3, 4] and m["stripes"] == 5


@pytest.mark.parametrize("mode,k", km.f_cases())
def test_group_f_sets(mode, k):
    decode = mode == "decode"
    n = k + km.MIXED_EXTRA
    sets = km.f_sets(k, decode)
    lost = [sets.index(km.f_lost(k))]
    assert sets.count(km.f_lost(k)) == 1 and sets.count(()) == 2 and sets[0] == sets[-1] == ()
    model = check_sets(n, k, sets, decode, lost)
    # every chunk is the only erased one once; the pairs, the full sets and the two-segment plans are there
    for e in [(c,) for c in range(n)] + [(0, n - 1), (k - 1, k), km.three_of(k), tuple(range(4)), tuple(range(n - 4, n)),
                                         tuple(range(0, n, 2))[:4], tuple(range(5)), tuple(range(n - 6, n)),
                                         tuple(range(k - 1, k + 5))]:
        assert e in sets, (k, e)
    # a 4-row segment is followed by a 1-row, a 2-row and a 3-row one (the decode's rows: lost data chunks <= k)
    assert holds(model["seg_rows"], km.f_row_sequence(k, decode)), (mode, k, model["seg_rows"])
    if not decode or k >= 4:
        assert km.f_row_sequence(k, decode) == [4, 1, 2, 3]
    if not decode or k >= 5:  # range(5) and, in place, range(n - 6, n): second segments of 1 and 2 rows
        assert holds(model["seg_rows"], [4, 1]) and (decode or holds(model["seg_rows"], [4, 2]))
    assert km.F_LEN % 16 == 0 and km.F_LEN // 16 == km.KBLOCK + 3
    assert len(sets) * (n + 1) * km.F_STRIDE <= 17 << 20  # about 16 MB at the widest


@pytest.mark.parametrize("mode,k", km.g_cases())
def test_group_g_patterns(mode, k):
    decode = mode == "decode"
    n = k + km.MIXED_EXTRA
    pats = km.g_sets(k)
    assert len(pats) >= 6 and {4, 1, 6, 2, 3, 5} <= {len(e) for e in pats}
    assert () in pats and tuple(range(n - 4, n)) in pats  # clean and parity-only
    rows = check_sets(n, k, pats * 3, decode)["seg_rows"]  # repeats add stripes, not plans
    assert rows == check_sets(n, k, pats, decode)["seg_rows"]
    if decode:
        # the clean plan is one pure-copy segment between coded ones; the parity-only set has the same first k
        # alive chunks and joins it
        z = rows.index(0)
        assert rows.count(0) == 1 and 0 < z < len(rows) - 1 and rows[z - 1] > 0 and rows[z + 1] > 0
        both = km.mixed_model(n, k, [(), tuple(range(n - 4, n))], True)
        assert (both["plans"], both["seg_rows"], both["verdict"]) == (1, [0], [0, 0])
    if decode and k < 5:
        # at most k data chunks can be lost: k = 1 has no 4-row segment and no plan of two segments
        assert k == 1 and set(rows) == {0, 1}
    else:
        assert any(a == 4 and b < 4 for a, b in zip(rows, rows[1:])), (mode, k, rows)
        two = km.mixed_model(n, k, [tuple(range(5))], decode)
        assert two["plans"] == 1 and two["seg_rows"] == [4, 1]
    if not decode:
        assert km.mixed_model(n, k, [tuple(range(k - 1, k + 5))], False)["seg_rows"] == [4, 2]
        assert 3 in rows and 2 in rows and 1 in rows
    for cus in (1, 64, 256, 304):
        ns = km.g_stripes(k, decode, cus)
        model = km.mixed_model(n, k, [pats[s % len(pats)] for s in range(ns)], decode)
        tiles = len(model["order"]) * (km.G_CS // km.TILE)
        assert tiles >= ns >= 4 * cus * km.mixed_launch(k, decode)["tpg"]


def test_group_g_poisoned_items_are_the_first_pattern():
    """The negative control skips items 0..4 of the recover at k = 9: five stripes of the first pattern."""
    k = km.UPDATE_MAX_K16
    pats = km.g_sets(k)
    assert km.mixed_launch(k, False)["tpg"] == 1
    ns = km.g_stripes(k, False, 256)
    model = km.mixed_model(k + km.MIXED_EXTRA, k, [pats[s % len(pats)] for s in range(ns)], False)
    assert model["order"][:5] == [0, 9, 18, 27, 36] and len(pats) == 9


@pytest.mark.parametrize("mode", km.MIXED_MODES)
def test_reference_alone_on_a_group_f_case(mode):
    """The truth image of group (f) is a codeword under the oracle's own arithmetic: the inverse of the first
    k alive rows of the generator (oracle.invert_matrix), applied with oracle.matmul, gives back the data,
    and the generator's rows of the erased chunks applied to that give back every erased chunk."""
    k, decode = 11, mode == "decode"
    n, length = k + km.MIXED_EXTRA, km.F_LEN
    enc = oracle.gen_rs_matrix(n, k)
    rng = np.random.default_rng(4100 + decode)
    stripe = oracle.rs_encode(n, k, rng.integers(0, 256, size=k * length, dtype=np.uint8), length)
    assert np.array_equal(stripe[:k], np.stack(oracle.matmul(enc[:k], list(stripe[:k]))))  # systematic
    for e in km.f_sets(k, decode):
        if e == km.f_lost(k) or not e:
            continue
        ids = km.first_alive(n, k, e)
        rc, inv = oracle.invert_matrix(enc[ids])
        assert rc == 0
        data = oracle.matmul(inv, [stripe[c] for c in ids])
        assert all(np.array_equal(data[j], stripe[j]) for j in range(k)), (mode, e)
        back = oracle.matmul(enc[list(e)], data)
        assert all(np.array_equal(back[i], stripe[c]) for i, c in enumerate(e)), (mode, e)


def test_group_h_table_and_plan():
    assert sorted(km.H_ROWS) == [1, 2, 3, 4, 5, 6]
    assert {km.h_p(k) for k in range(1, km.RAGGED_MAX_K + 1)} == set(range(1, 7))
    assert km.h_p(km.RAGGED_MAX_K) == 4 and km.h_p(km.UPDATE_MAX_K16) == 1
    assert km.H_OFF + km.H_BYTES <= km.F_LEN
    batch, new = 0x7000_0000_0000, 0x7100_0000_0000  # addresses only: the planner touches no memory
    for k in range(1, km.RAGGED_MAX_K + 1):
        n, p, cs = k + km.h_p(k), km.h_p(k), km.F_STRIDE
        specs = km.h_specs(k)
        assert [(s, c) for s, c, _, _ in specs] == [(j, j) for j in range(k)]  # every chunk index once, stripe k untouched
        ups = [(s, c, off, ln, new + km.h_new_offset(i)) for i, (s, c, off, ln) in enumerate(specs)]
        for (_, _, _, ln, a), (_, _, _, _, b) in zip(ups, ups[1:]):
            assert a + ln <= b  # the new bytes of two updates do not overlap
        want = km.update_counters(n, k, cs, n * cs, km.F_LEN, batch, ups)
        assert want == nxec.rs_update_plan(n, k, cs, n * cs, km.F_LEN, k + 1, batch, ups)
        assert want == (1, 2 * k, 2 * k)  # a head, a full tile + a one-vector tile, a tail
        plan = km.h_plan(k, batch, new)
        passes = -(-p // km.MAX_ROWS)
        assert [r["family"] for r in plan] == ["k_update_vec", "k_update_bytes"] * passes
        assert [r["last"] for r in plan] == [0, 0, 1, 1][-2 * passes:]
        assert [r["rows"] for r in plan[::2]] == ([4, p - 4] if p > 4 else [p])
        for r in plan[::2]:
            assert r["r"] == (16 if k <= km.UPDATE_MAX_K16 else 8) and (r["pf"], r["q"]) == (1, 1)
            assert r["tpg"] == km.tiles_per_grab(2 + r["last"], 2 * r["rows"]) and r["tiles"] == 2 * k
        assert km.queue_fits(k * 1024 * km.default_r(k))  # update_lds(k): the ring lies right above the k tables


def test_launch_record_is_off_by_default_and_reads_empty():
    assert nxec.launch_log_read() == []
    nxec.launch_log(True)
    try:
        assert nxec.launch_log_read() == []
    finally:
        nxec.launch_log(False)
    buf = nxec.C.create_string_buffer(4)
    assert nxec.lib.nxec_debug_launch_log_read(buf, 4) == 0 and buf.value == b""
