"""The digest matrix's plan (tests/digest_matrix.py), checked without a device:
its constants against the sources, and that its range of lengths and its two
layouts reach every state of k_md5's streaming loops for the ring shapes in
the sources -- so widening a ring without widening the range fails here."""
import pytest

import digest_matrix as dm


@pytest.mark.parametrize("name", sorted(dm.SOURCE_CONSTANTS))
def test_constants_mirror_the_sources(name):
    assert dm.source_constant(name) == dm.SOURCE_CONSTANTS[name]


def test_ring_shapes_mirror_the_sources():
    assert dm.source_ring_defaults() == (dm.MD5_DEPTH, dm.MD5_GROUP) == (2, 8)
    assert dm.source_misaligned_ring() == [(dm.MD5_U_DEPTH, dm.MD5_U_GROUP)] == [(2, 4)]


def test_length_range_spans_three_periods_of_the_aligned_ring():
    period = dm.MD5_DEPTH * dm.MD5_GROUP
    assert dm.LENGTHS == range(0, 64 * (3 * period + 1))
    assert len(dm.LENGTHS) >= 64 * (6 * dm.MD5_U_DEPTH * dm.MD5_U_GROUP + 1)  # six periods of the misaligned ring
    assert (dm.LENGTHS[0], dm.LENGTHS[-1]) == (0, 3135)


def _classes(layout):
    """path (without the shift) -> set of rem, and the shifts seen per misaligned state, over the whole matrix."""
    rems, shifts = {}, {}
    for length in dm.LENGTHS:
        for lane in range(dm.LANES):
            p = dm.path(dm.chunk_offset(layout, length, lane), length)
            key = p[:4] if p[0] == "misaligned" else p
            rems.setdefault(key, set()).add(length % 64)
            if p[0] == "misaligned":
                shifts.setdefault(key, set()).add(p[4])
    return rems, shifts


@pytest.fixture(scope="module")
def ragged():
    return _classes("ragged")


@pytest.mark.parametrize("layout", dm.LAYOUTS)
def test_aligned_path_meets_every_ring_state_with_every_tail(layout, ragged):
    rems = ragged[0] if layout == "ragged" else _classes(layout)[0]
    want = dm.all_ring_states(dm.MD5_DEPTH, dm.MD5_GROUP)
    assert len(want) == dm.MD5_DEPTH * 3 * dm.MD5_GROUP
    seen = {key[1:] for key in rems if key[0] == "aligned"}
    assert seen == want, sorted(want - seen)
    for key, r in rems.items():
        if key[0] == "aligned":
            assert r == set(range(64)), key
    if layout == "aligned":
        assert {key[0] for key in rems} == {"aligned"}  # whole waves on md5_stream


def test_misaligned_path_meets_every_ring_state_tail_and_shift(ragged):
    rems, shifts = ragged
    want = dm.all_ring_states(dm.MD5_U_DEPTH, dm.MD5_U_GROUP) - {(0, 0, 0)}  # nblk >= 1
    seen = {key[1:] for key in rems if key[0] == "misaligned"}
    assert seen == want, sorted(want ^ seen)
    assert {key for key in rems if key[0] == "bytes"} == {("bytes", 0), ("bytes", 1)}
    for key, r in rems.items():
        assert r == set(range(64)), key
    for key, s in shifts.items():
        assert s == {0, 8, 16, 24}, key  # shift 0: an address that is 4, 8 or 12 mod 16


def test_padding_edges_follow_streamed_blocks():
    """rem = 55 (one padding block), 56 and 63 (two) behind every count of streamed blocks in the range."""
    for nfull in range(0, dm.LENGTHS[-1] // 64):
        for rem in (0, 55, 56, 63):
            assert nfull * 64 + rem in dm.LENGTHS


def test_ragged_layout_shows_every_alignment_in_every_stripe():
    for length in dm.LENGTHS:
        cs, ss = dm.strides("ragged", length)
        assert cs >= length + 1 and cs % 16 == 1 and cs - 16 < length + 1 and ss == dm.NCHUNKS * cs + 5
        for s in range(dm.NSTRIPES):
            al = {dm.chunk_offset("ragged", length, s * dm.NCHUNKS + c) % 16 for c in range(dm.NCHUNKS)}
            assert al == set(range(16)), (length, s)


@pytest.mark.parametrize("layout", dm.LAYOUTS)
def test_layout_keeps_every_chunk_apart_and_inside_the_buffer(layout):
    size = dm.buffer_bytes(layout)
    for length in dm.LENGTHS:
        offs = [dm.chunk_offset(layout, length, lane) for lane in range(dm.LANES)]
        assert offs == sorted(offs) and offs[0] == 0
        assert all(b - a >= length + 1 for a, b in zip(offs, offs[1:])), length  # a byte between neighbours
        # the misaligned path reads whole dwords around a chunk: up to 3 bytes past its last streamed block
        assert offs[-1] + length + 3 < size, length
        if layout == "aligned":
            cs, ss = dm.strides(layout, length)
            assert cs == dm.rup(length) + 16 and ss == dm.NCHUNKS * cs and all(o % 16 == 0 for o in offs)


def test_digest_slots_do_not_overlap_and_ragged_ones_are_odd():
    for layout in dm.LAYOUTS:
        offs = [dm.digest_offset(layout, length) for length in dm.LENGTHS]
        assert all(b - a == dm.LANES * 16 + dm.DIGEST_GUARD for a, b in zip(offs, offs[1:]))
        assert offs[-1] + dm.DIGEST_SLOT <= dm.digest_bytes()
        assert all(o % 2 == (layout == "ragged") for o in offs)


def test_verify_alterations_take_every_digest_byte():
    hit = {dm.altered_byte(lane, length) for length in dm.LENGTHS for lane in range(dm.LANES)
           if dm.altered(lane, length)}
    assert hit == set(range(16))
    n = sum(dm.altered(lane, length) for length in dm.LENGTHS for lane in range(dm.LANES))
    assert 0 < n < len(dm.LENGTHS) * dm.LANES
