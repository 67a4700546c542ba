"""Delta update, host side (CPU only): the plan counters of nxec_rs_update_plan
against a brute-force evaluation in Python (rounds as the most updates over one
column of one stripe, which is what an interval colouring needs; the split of
every update into a 16-byte-aligned body and byte heads and tails), the
argument validation of the plan call and of nxec_rs_update_stripes, and the two
stand-alone C++ programs (tests/cpp/update_plan_test.cc under ASan + UBSan,
tests/cpp/update_registry_test.cc against libnxec).

No device memory is touched here: the batch and the new bytes are addresses only.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import kernel_matrix
from nexoedge_amd import _lib, nxec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 0x7000_0000_0000  # a 16-byte aligned stand-in for the batch's device address
NEW = 0x7100_0000_0000    # new bytes live far from it
TILE_VECS = 1024
INVALID, NODEV, OK = _lib.NXEC_ERR_INVALID, _lib.NXEC_ERR_NODEV, _lib.NXEC_OK


def rup(x, m=16):
    return (x + m - 1) // m * m


# the brute-force evaluation lives with the kernel matrix, whose update group plans its launches from it
brute = kernel_matrix.update_counters
assert kernel_matrix.KBLOCK == TILE_VECS and kernel_matrix.RAGGED_MAX_K == 19


def draw(rng, k, length, ns, count, misalign=0.2):
    """A seeded list without same-chunk intersections (rejection sampling); every update has its own
    d_new region, aligned like its offset unless drawn misaligned."""
    ups, taken = [], {}
    sizes = [0, 1, 11, 16, 27, 100, 1024, 16384, 16384 + 20, length]
    while len(ups) < count:
        s, c = int(rng.integers(ns)), int(rng.integers(k))
        ln = min(int(rng.choice(sizes)), length)
        off = int(rng.integers(length - ln + 1))
        if rng.random() < 0.4:
            off = off // 16 * 16
        if any(off < o + l and o < off + ln for o, l in taken.get((s, c), [])) and ln > 0:
            continue
        taken.setdefault((s, c), []).append((off, ln))
        p = NEW + (len(ups) << 24) + off % 16 + (4 if rng.random() < misalign else 0)
        ups.append((s, c, off, ln, p))
    return ups


@pytest.mark.parametrize("n,k", [(6, 4), (14, 10), (10, 4), (23, 19), (24, 21)])
def test_plan_counters_against_python(n, k):
    rng = np.random.default_rng(1000 * n + k)
    some_vec = False
    for length in (16, 100, 16384 + 16, 3 * 16384 + 48):
        for cs, ss in ((length, n * length), (rup(length) + 48, n * (rup(length) + 48)), (rup(length), (n + 1) * rup(length))):
            for case in range(6):
                ups = draw(rng, k, length, 5, int(rng.integers(1, 41)))
                got = nxec.rs_update_plan(n, k, cs, ss, length, 5, BATCH, ups)
                want = brute(n, k, cs, ss, length, BATCH, ups)
                assert got == want, (n, k, length, cs, ss, case)
                live = [u for u in ups if u[3] > 0]
                if k > 19 or cs % 16:
                    assert got[1:] == (0, len(live))  # everything is byte items
                else:
                    some_vec |= got[1] > 0
                    # whole vectors with matching d_new: nothing is left to the byte kernel
                    whole = [(s, c, rup(off), max(0, (off + ln) // 16 * 16 - rup(off)), p // 16 * 16)
                             for s, c, off, ln, p in live if rup(off) < (off + ln) // 16 * 16]
                    _, tiles, items = nxec.rs_update_plan(n, k, cs, ss, length, 5, BATCH, whole)
                    assert items == 0 and tiles == sum(-(-u[3] // 16384) for u in whole)
                assert got[0] <= k
    assert some_vec == (k <= 19)


def test_plan_unaligned_batch_address_is_byte_items_only():
    ups = [(0, 0, 0, 16384, NEW), (1, 2, 16, 4096, NEW + (1 << 24))]
    assert nxec.rs_update_plan(6, 4, 16384, 6 * 16384, 16384, 2, BATCH, ups) == (1, 2, 0)
    assert nxec.rs_update_plan(6, 4, 16384, 6 * 16384, 16384, 2, BATCH + 3, ups) == (1, 0, 2)
    assert nxec.rs_update_plan(6, 4, 16384 + 8, 6 * (16384 + 8), 16384, 2, BATCH, ups) == (1, 0, 2)


def test_plan_body_head_tail_split():
    plan = lambda ups, k=4, n=6: nxec.rs_update_plan(n, k, 65536, n * 65536, 65536, 3, BATCH, ups)  # noqa: E731
    assert plan([(0, 0, 0, 65536, NEW)]) == (1, 4, 0)
    assert plan([(0, 0, 0, 16, NEW)]) == (1, 1, 0)
    assert plan([(0, 0, 65536 - 16, 16, NEW)]) == (1, 1, 0)
    assert plan([(0, 0, 5, 1, NEW + 5)]) == (1, 0, 1)
    assert plan([(0, 0, 5, 11, NEW + 5)]) == (1, 0, 1)  # head only
    assert plan([(0, 0, 5, 27, NEW + 5)]) == (1, 1, 1)  # head, one vector, no tail
    assert plan([(0, 0, 3, 16384 + 20, NEW + 3)]) == (1, 1, 2)  # head, 1024 vectors, tail
    assert plan([(0, 0, 3, 16384 + 40, NEW + 3)]) == (1, 2, 2)  # head, 1025 vectors, tail
    assert plan([(0, 0, 16, 16384, NEW)]) == (1, 1, 0)
    assert plan([(0, 0, 16, 16384, NEW + 4)]) == (1, 0, 1)  # d_new off by 4: the whole update by bytes
    assert plan([(0, 0, 5, 27, NEW)]) == (1, 0, 1)  # d_new aligned where the offset is not
    assert plan([(0, 0, 100, 0, NEW)]) == (0, 0, 0)
    assert plan([]) == (0, 0, 0)
    assert plan([(0, 0, 16, 16384, NEW)], k=19, n=23) == (1, 1, 0)
    assert plan([(0, 0, 16, 16384, NEW)], k=20, n=24) == (1, 0, 1)


def test_rounds():
    plan = lambda ups: nxec.rs_update_plan(6, 4, 4096, 6 * 4096, 4096, 4, BATCH, ups)  # noqa: E731
    a, b, c, d = NEW, NEW + (1 << 24), NEW + (2 << 24), NEW + (3 << 24)
    # no column intersections: exactly one round
    assert plan([(s, s % 4, 256 * s, 256, a + (s << 24)) for s in range(4)])[0] == 1
    assert plan([(0, 0, 0, 128, a), (0, 1, 128, 128, b), (0, 2, 256, 128, c), (0, 0, 384, 128, d)])[0] == 1
    # chunks 0 and 1 over the same columns: two rounds
    assert plan([(2, 0, 64, 64, a), (2, 1, 64, 64, b)]) == (2, 2, 0)
    assert plan([(2, 0, 64, 64, a), (3, 1, 64, 64, b)])[0] == 1  # other stripes do not meet
    assert plan([(2, 0, 64, 64, a), (2, 1, 127, 64, b + 15)])[0] == 2  # one shared column
    assert plan([(2, 0, 64, 64, a), (2, 1, 128, 64, b)])[0] == 1  # adjacent
    # all k chunks over the whole length: k rounds
    assert plan([(1, j, 0, 4096, a + (j << 24)) for j in range(4)]) == (4, 4, 0)
    # a chain a-b, b-c overlapping pairwise but not all three: two rounds are enough
    assert plan([(0, 0, 0, 100, a), (0, 1, 50, 100, b + 2), (0, 2, 120, 100, c + 8)])[0] == 2


def update_call(ctx, ups="one", n=6, k=4, stripes=BATCH, cs=64, ss=6 * 64, length=64, ns=2, count=None):
    if isinstance(ups, str):
        ups = [(0, 1, 8, 16, NEW)]
    arr = (_lib.Update * max(len(ups), 1))()
    for u, (s, c, off, ln, p, *rest) in zip(arr, ups):
        u.stripe, u.chunk, u.offset, u.length, u.d_new = s, c, off, ln, p
        u.reserved = rest[0] if rest else 0
    return _lib.lib.nxec_rs_update_stripes(ctx, n, k, ctypes.c_void_p(stripes), cs, ss, length, ns, arr,
                                           len(ups) if count is None else count, None)


def plan_call(ups, n=6, k=4, stripes=BATCH, cs=64, ss=6 * 64, length=64, ns=2, count=None):
    arr = (_lib.Update * max(len(ups), 1))()
    for u, (s, c, off, ln, p, *rest) in zip(arr, ups):
        u.stripe, u.chunk, u.offset, u.length, u.d_new = s, c, off, ln, p
        u.reserved = rest[0] if rest else 0
    cnt = ctypes.c_int64(7)
    rc = _lib.lib.nxec_rs_update_plan(n, k, cs, ss, length, ns, stripes, arr, len(ups) if count is None else count,
                                      cnt, cnt, cnt)
    assert rc == OK or cnt.value == 7  # refused calls write nothing
    return rc


REJECTED = {
    "invalid (n,k) 4,5": dict(n=4, k=5),
    "invalid (n,k) 0,0": dict(n=0, k=0),
    "invalid (n,k) 129,4": dict(n=129, k=4),
    "negative chunk stride": dict(cs=-64),
    "negative stripe stride": dict(ss=-1),
    "negative len": dict(length=-1),
    "negative nstripes": dict(ns=-1),
    "negative nupdates": dict(count=-1),
    "stripe past the batch": dict(ups=[(2, 1, 8, 16, NEW)]),
    "negative stripe": dict(ups=[(-1, 1, 8, 16, NEW)]),
    "a parity chunk": dict(ups=[(0, 4, 8, 16, NEW)]),
    "negative chunk": dict(ups=[(0, -1, 8, 16, NEW)]),
    "negative offset": dict(ups=[(0, 1, -1, 16, NEW)]),
    "negative length": dict(ups=[(0, 1, 8, -1, NEW)]),
    "range past the chunk": dict(ups=[(0, 1, 49, 16, NEW)]),
    "length that overflows": dict(ups=[(0, 1, 8, 2 ** 63 - 1, NEW)]),
    "reserved != 0": dict(ups=[(0, 1, 8, 16, NEW, 1)]),
    "same chunk, one shared byte": dict(ups=[(0, 1, 8, 16, NEW), (0, 1, 23, 4, NEW + 64)]),
    "same chunk, one shared byte, listed the other way": dict(ups=[(0, 1, 23, 4, NEW + 64), (0, 1, 8, 16, NEW)]),
    "same chunk, same range, far apart in the list": dict(ups=[(0, 1, 8, 16, NEW), (1, 1, 8, 16, NEW), (0, 2, 8, 16, NEW),
                                                              (0, 1, 8, 16, NEW)]),
    "d_new inside the batch": dict(ups=[(0, 1, 8, 16, BATCH + 100)]),
    "d_new reaching into the batch": dict(ups=[(0, 1, 8, 16, BATCH - 15)]),
    "d_new on the batch's last byte": dict(ups=[(0, 1, 8, 16, BATCH + 2 * 6 * 64 - 1)]),
    "null d_new": dict(ups=[(0, 1, 8, 16, None)]),
    "chunks beyond 4 GiB": dict(cs=1 << 30, ss=6 << 30),
}


@pytest.mark.parametrize("what", sorted(REJECTED))
def test_rejections_before_any_device_use(what):
    """Both calls refuse the same arguments; the batch call with a context that is never valid here."""
    kw = dict(REJECTED[what])
    ups = kw.pop("ups", [(0, 1, 8, 16, NEW)])
    assert plan_call(ups, **kw) == INVALID, what
    assert update_call(ctypes.c_void_p(1), ups, **kw) == INVALID, what


def test_null_list_and_null_context_and_null_batch():
    L = _lib.lib
    cnt = ctypes.c_int64(7)
    assert L.nxec_rs_update_plan(6, 4, 64, 384, 64, 2, BATCH, None, 1, cnt, cnt, cnt) == INVALID and cnt.value == 7
    assert L.nxec_rs_update_stripes(ctypes.c_void_p(1), 6, 4, ctypes.c_void_p(BATCH), 64, 384, 64, 2, None, 1, None) == INVALID
    assert update_call(None) == INVALID  # no context, even with valid work
    assert update_call(None, ups=[]) == INVALID
    assert update_call(ctypes.c_void_p(1), stripes=None) == INVALID  # work to do, no buffer
    assert L.nxec_rs_update_plan(6, 4, 64, 384, 64, 2, BATCH, None, 0, None, None, None) == OK  # everything optional


def test_legal_neighbours_of_the_rejections():
    assert plan_call([(0, 1, 8, 16, NEW), (0, 1, 24, 4, NEW + 64), (0, 1, 0, 8, NEW + 128)]) == OK  # adjacent ranges
    assert plan_call([(0, 1, 8, 16, NEW), (0, 2, 8, 16, NEW), (1, 1, 8, 16, NEW)]) == OK  # d_new may be shared
    assert plan_call([(0, 1, 48, 16, NEW)]) == OK and plan_call([(0, 1, 64, 0, NEW)]) == OK  # up to the chunk's end
    assert plan_call([(0, 1, 8, 16, BATCH - 16)]) == OK and plan_call([(0, 1, 8, 16, BATCH + 2 * 384)]) == OK
    assert plan_call([(0, 1, 8, 0, None)]) == OK  # an empty update needs no bytes
    assert plan_call([(0, 1, 8, 0, NEW)], cs=1 << 30, ss=6 << 30) == OK  # nothing to do: any layout
    assert plan_call([(0, 1, 8, 16, NEW), (0, 1, 10, 0, NEW)]) == OK  # an empty update inside another


def test_empty_work_needs_no_device():
    fake = ctypes.c_void_p(1)
    assert update_call(fake, ups=[]) == OK
    assert update_call(fake, ups=[(0, 1, 8, 0, NEW), (1, 3, 64, 0, None)]) == OK
    assert update_call(fake, ups=[(0, 1, 8, 0, NEW)], stripes=None) == OK
    assert update_call(fake, ups=[], ns=0) == OK and update_call(fake, ups=[], length=0) == OK


@pytest.mark.skipif(nxec.device_count() > 0, reason="a GPU is visible")
def test_valid_work_without_a_device_fails_loudly():
    """No CPU fallback for either kind of work item: with work to do and no usable device the call reports
    NXEC_ERR_NODEV.  A zeroed block stands in for a context (the call reads its device index and fails at
    the device check)."""
    stand_in = ctypes.create_string_buffer(8192)
    ctx = ctypes.cast(stand_in, ctypes.c_void_p)
    assert nxec.rs_update_plan(6, 4, 64, 384, 64, 2, BATCH, [(0, 1, 16, 32, NEW)]) == (1, 1, 0)
    assert update_call(ctx, ups=[(0, 1, 16, 32, NEW)]) == NODEV  # a vector shape
    assert nxec.rs_update_plan(6, 4, 64, 384, 64, 2, BATCH, [(0, 1, 5, 3, NEW)]) == (1, 0, 1)
    assert update_call(ctx, ups=[(0, 1, 5, 3, NEW)]) == NODEV  # a byte shape
    assert update_call(ctx, ups=[(0, 1, 16, 32, NEW)], n=24, k=21, ss=24 * 64) == NODEV  # k > 19
    assert update_call(ctx, ups=[(0, 1, 16, 32, NEW)], n=4, k=4, ss=256) == NODEV  # n == k still overwrites data


def run_program(name, marker, sanitized):
    exe = os.path.join(ROOT, "build", name)
    assert os.path.exists(exe), f"build/{name} missing: run make (or __graft_entry__.build())"
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert ("__asan_init" in syms and "__ubsan_handle" in syms) == sanitized
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert marker in r.stdout


def test_standalone_planner_program_under_sanitizers():
    """tests/cpp/update_plan_test.cc: the planner and the device tables it builds as a plain host program built
    with -fsanitize=address,undefined (its own main; nothing is preloaded here)."""
    run_program("update_plan_test", "update_plan_test ok", sanitized=True)


def test_every_update_kernel_is_prepared():
    """tests/cpp/update_registry_test.cc: for k = 1..19 the kernel the vector launch picks, and for every k the
    byte kernel, is in the per-device preparation list with at least the LDS the launch asks for."""
    run_program("update_registry_test", "update_registry_test ok", sanitized=False)
