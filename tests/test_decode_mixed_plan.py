"""Mixed-pattern decode, host side (CPU only): the per-stripe verdicts and
plan counters of nxec_rs_decode_mixed_plan against a brute force built from
nxec_rs_plan(is_repair=0) + nxec_rs_decode_matrix (the steps of
nxec_rs_decode_stripes) and against nxec_rs_recover_mixed_plan, the argument
validation of the plan call, of nxec_rs_decode_stripes_mixed and of
nxec_decode_object_mixed, and the two stand-alone C++ programs
(tests/cpp/decode_mixed_plan_test.cc under ASan + UBSan,
tests/cpp/mixed_registry_test.cc against libnxec).

Every erasure set of 0..n-k chunks is one stripe.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from nexoedge_amd import _lib, nxec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOST, SINGULAR = nxec.RECOVER_LOST, nxec.RECOVER_SINGULAR
GEOMETRIES = [(6, 4), (14, 10), (10, 4), (12, 6), (23, 19)]


def erasure_sets(n, lo, hi):
    return [e for size in range(lo, hi + 1) for e in itertools.combinations(range(n), size)]


def alive_map(n, sets):
    a = np.ones((len(sets), n), dtype=np.uint8)
    for s, e in enumerate(sets):
        a[s, list(e)] = 0
    return a


def brute(n, k, e):
    """(verdict, first k alive ids) of one stripe, the way nxec_rs_decode_stripes plans it."""
    if len(e) > n - k:
        return LOST, None
    f = (ctypes.c_int32 * max(len(e), 1))(*e)
    inputs = (ctypes.c_int32 * n)()
    ni, mi = ctypes.c_int(), ctypes.c_int()
    rc = _lib.lib.nxec_rs_plan(n, k, f, len(e), 0, inputs, ctypes.byref(ni), ctypes.byref(mi), None)
    assert rc == _lib.NXEC_OK and ni.value == n - len(e)
    targets = [c for c in e if c < k]
    if targets:
        t = (ctypes.c_int32 * len(targets))(*targets)
        m = (ctypes.c_ubyte * (len(targets) * k))()
        rc = _lib.lib.nxec_rs_decode_matrix(n, k, inputs, t, len(targets), m)
        assert rc in (_lib.NXEC_OK, _lib.NXEC_ERR_SINGULAR), rc
        if rc != _lib.NXEC_OK:
            return SINGULAR, None
    return len(targets), tuple(inputs[:k])


@pytest.mark.parametrize("n,k", GEOMETRIES)
def test_plan_against_brute_force(n, k):
    sets = erasure_sets(n, 0, n - k)
    both = [brute(n, k, e) for e in sets]
    want = np.array([v for v, _ in both], dtype=np.int32)
    a = alive_map(n, sets)
    res, nplans, nseg, ndec = nxec.rs_decode_mixed_plan(n, k, a)
    assert np.array_equal(res, want)
    # negative exactly where the recover's plan is: both invert the same input matrix
    rec = nxec.rs_recover_mixed_plan(n, k, a)[0]
    assert np.array_equal(res < 0, rec < 0) and np.array_equal(res[res < 0], rec[rec < 0])
    ok = want >= 0
    assert np.array_equal(res[ok], np.array([sum(c < k for c in e) for e, good in zip(sets, ok) if good], dtype=np.int32))
    # plans are keyed by the first k alive ids, computed here from the map alone
    tuples = {tuple(np.flatnonzero(row)[:k]): r for row, r in zip(a[ok], want[ok])}
    assert tuples.keys() == {inp for (_, inp), good in zip(both, ok) if good}
    assert nplans == len(tuples) and ndec == int(ok.sum())
    assert nseg == sum(max(1, -(-int(t) // 4)) for t in tuples.values())
    assert tuple(range(k)) in tuples  # the clean plan counts
    # the batch twice over: no new plan
    res2, nplans2, nseg2, ndec2 = nxec.rs_decode_mixed_plan(n, k, np.concatenate([a, a]))
    assert np.array_equal(res2, np.concatenate([res, res])) and (nplans2, nseg2, ndec2) == (nplans, nseg, 2 * ndec)


@pytest.mark.parametrize("n,k", GEOMETRIES + [(5, 4), (4, 4)])
def test_lost_stripes(n, k):
    sets = erasure_sets(n, n - k + 1, n - k + 1) + [tuple(range(n))]
    res, nplans, nseg, ndec = nxec.rs_decode_mixed_plan(n, k, alive_map(n, sets))
    assert res.tolist() == [LOST] * len(sets) and (nplans, nseg, ndec) == (0, 0, 0)


def test_specials_of_rs_12_6():
    sets = [(0, 2, 5, 7, 8), (6, 7, 8, 9, 10, 11), (0, 2, 5, 7, 9), (1, 2, 3, 4, 5, 6), ()]
    res, nplans, nseg, ndec = nxec.rs_decode_mixed_plan(12, 6, alive_map(12, sets))
    assert res.tolist() == [SINGULAR, 0, 3, 5, 0]
    # the parity-only loss and the clean stripe share the clean plan; five lost data chunks are two segments
    assert (nplans, nseg, ndec) == (3, 1 + 1 + 2, 4)


def test_masks_beyond_the_kth_alive_chunk_share_a_plan():
    """(10,4): inputs are the first 4 alive ids, so erasures past the fourth alive chunk do not make a new plan."""
    sets = [(0, 1), (0, 1, 9), (0, 1, 6, 7, 8, 9), (0, 1, 7), ()]
    res, nplans, nseg, ndec = nxec.rs_decode_mixed_plan(10, 4, alive_map(10, sets))
    assert res.tolist() == [2, 2, 2, 2, 0] and (nplans, nseg, ndec) == (2, 2, 5)
    a = np.full((3, 10), 0xFF, dtype=np.uint8)  # any non-zero byte is alive
    a[1, 2] = 0
    assert nxec.rs_decode_mixed_plan(10, 4, a)[0].tolist() == [0, 1, 0]
    assert nxec.rs_decode_mixed_plan(6, 4, np.zeros((0, 6), dtype=np.uint8))[1:] == (0, 0, 0)


def test_plan_call_validates():
    L = _lib.lib
    a = (ctypes.c_ubyte * 12)(*([1] * 12))
    res = (ctypes.c_int32 * 2)(7, 7)
    cnt = ctypes.c_int64(7)
    for n, k in ((0, 0), (4, 5), (6, 0), (129, 4), (130, 128)):
        assert L.nxec_rs_decode_mixed_plan(n, k, a, 1, res, cnt, cnt, cnt) == _lib.NXEC_ERR_INVALID, (n, k)
    assert L.nxec_rs_decode_mixed_plan(6, 4, None, 1, res, cnt, cnt, cnt) == _lib.NXEC_ERR_INVALID
    assert L.nxec_rs_decode_mixed_plan(6, 4, a, -1, res, cnt, cnt, cnt) == _lib.NXEC_ERR_INVALID
    assert list(res) == [7, 7] and cnt.value == 7  # refused calls write nothing
    assert L.nxec_rs_decode_mixed_plan(6, 4, None, 0, None, None, None, None) == _lib.NXEC_OK  # everything optional
    assert L.nxec_rs_decode_mixed_plan(6, 4, a, 2, res, None, None, None) == _lib.NXEC_OK and list(res) == [0, 0]


SRC, OUT = 1 << 20, 1 << 24  # fake device addresses, never touched


def mixed_call(ctx, n=6, k=4, alive="one", stripes=SRC, cs=64, ss=6 * 64, out=OUT, ocs=64, oss=4 * 64, length=64, ns=1,
               result=None):
    if isinstance(alive, str):
        row = [0] + [1] * (n - 1) if alive == "one" else [1] * n
        alive = (ctypes.c_ubyte * (n * max(ns, 1)))(*(row * max(ns, 1)))
    vp = ctypes.c_void_p
    return _lib.lib.nxec_rs_decode_stripes_mixed(ctx, n, k, alive, vp(stripes), cs, ss, vp(out), ocs, oss, length, ns,
                                                 result, None)


def test_batch_call_rejects_arguments_before_device_use():
    """Bad arguments are refused before the context or any device pointer is touched (neither is ever valid
    here), and a call with nothing to launch returns its verdicts without a device."""
    fake = ctypes.c_void_p(1)
    res = (ctypes.c_int32 * 4)(9, 9, 9, 9)
    bad = _lib.NXEC_ERR_INVALID
    assert mixed_call(None, result=res) == bad  # no context
    for n, k in ((0, 0), (4, 5), (6, 0), (129, 4), (130, 128)):
        assert mixed_call(fake, n=n, k=k, alive=(ctypes.c_ubyte * 256)(), result=res) == bad, (n, k)
    assert mixed_call(fake, alive=None, result=res) == bad
    assert mixed_call(fake, length=-1, result=res) == bad
    assert mixed_call(fake, ns=-1, result=res) == bad
    assert mixed_call(fake, cs=-64, result=res) == bad
    assert mixed_call(fake, ss=-64, result=res) == bad
    assert mixed_call(fake, stripes=None, result=res) == bad  # work to do, no source
    assert mixed_call(fake, out=None, result=res) == bad  # work to do, no output
    assert mixed_call(fake, cs=1 << 30, ss=6 << 30, out=1 << 40, result=res) == bad  # source chunks beyond 4 GiB
    assert mixed_call(fake, ocs=1 << 31, oss=4 << 31, out=1 << 40, result=res) == bad  # output chunks beyond 4 GiB
    assert mixed_call(fake, ocs=48, result=res) == bad  # out_chunk_stride < len
    assert mixed_call(fake, ocs=-64, oss=0, length=0, result=res) == bad
    assert mixed_call(fake, oss=3 * 64 + 63, result=res) == bad  # out_stripe_stride too small for k chunks
    # the output intersects the source: its start, its last byte, around it, and the far end of a batch
    assert mixed_call(fake, out=SRC, result=res) == bad
    assert mixed_call(fake, out=SRC + 6 * 64 - 1, result=res) == bad
    assert mixed_call(fake, out=SRC - 4 * 64 + 1, result=res) == bad
    assert mixed_call(fake, out=SRC - 64, oss=1 << 16, ns=3, result=res) == bad
    assert mixed_call(fake, out=SRC + 2 * 6 * 64 + 17, ns=3, result=res) == bad
    assert list(res) == [9, 9, 9, 9]  # refused calls write nothing
    # nothing to launch: the verdicts are still filled, and no device is needed
    assert mixed_call(fake, alive=None, ns=0) == _lib.NXEC_OK
    assert mixed_call(fake, length=0, stripes=None, out=None, result=res) == _lib.NXEC_OK and res[0] == 1
    lost = (ctypes.c_ubyte * 18)(*([0, 0, 0, 1, 1, 1] * 3))
    assert mixed_call(fake, alive=lost, stripes=None, out=None, ns=3, result=res) == _lib.NXEC_OK
    assert list(res) == [LOST, LOST, LOST, 9]
    assert mixed_call(fake, n=4, k=4, alive=(ctypes.c_ubyte * 4)(1, 0, 1, 1), stripes=None, out=None, cs=64, ss=256,
                      result=res) == _lib.NXEC_OK and res[0] == LOST  # n == k: an erased chunk is lost
    sing = (ctypes.c_ubyte * 12)(*[0 if c in (0, 2, 5, 7, 8) else 1 for c in range(12)])
    assert mixed_call(fake, n=12, k=6, alive=sing, stripes=None, out=None, ss=12 * 64, oss=6 * 64,
                      result=res) == _lib.NXEC_OK and res[0] == SINGULAR
    # touching ranges do not intersect: refused only at the device check or not at all
    assert mixed_call(fake, alive=lost, out=SRC + 3 * 6 * 64, ns=3, result=res) == _lib.NXEC_OK
    assert mixed_call(fake, alive=lost, out=SRC - 3 * 4 * 64, ns=3, result=res) == _lib.NXEC_OK


def object_call(ctx, n=6, k=4, alive="one", chunks=SRC, cs=64, ss=6 * 64, length=4 * 64, M=64, obj=OUT, tail=OUT + 4096,
                result=None):
    if isinstance(alive, str):
        alive = (ctypes.c_ubyte * (n * 4))(*([0] + [1] * (n - 1)) * 4)
    vp = ctypes.c_void_p
    return _lib.lib.nxec_decode_object_mixed(ctx, n, k, alive, vp(chunks), cs, ss, length, M, vp(obj), vp(tail), result,
                                             None)


def test_object_call_rejects_arguments_before_device_use():
    fake = ctypes.c_void_p(1)
    res = (ctypes.c_int32 * 4)(9, 9, 9, 9)
    bad = _lib.NXEC_ERR_INVALID
    assert object_call(None, result=res) == bad
    assert object_call(fake, n=4, k=5, result=res) == bad
    assert object_call(fake, length=-1, result=res) == bad
    assert object_call(fake, M=0, result=res) == bad
    assert object_call(fake, alive=None, result=res) == bad
    assert object_call(fake, chunks=None, result=res) == bad
    assert object_call(fake, obj=None, result=res) == bad
    assert object_call(fake, length=4 * 64 + 5, tail=None, result=res) == bad  # a last stripe needs the scratch
    assert object_call(fake, cs=48, result=res) == bad
    assert object_call(fake, ss=5 * 64, result=res) == bad
    assert object_call(fake, obj=SRC + 64, result=res) == bad  # the object intersects the chunks
    assert list(res) == [9, 9, 9, 9]
    assert object_call(fake, length=0, result=res) == _lib.NXEC_OK and list(res) == [9, 9, 9, 9]  # no stripe at all
    lost = (ctypes.c_ubyte * 12)(*([0, 0, 0, 1, 1, 1] * 2))
    assert object_call(fake, alive=lost, length=4 * 64 + 5, result=res) == _lib.NXEC_OK  # both stripes skipped
    assert list(res) == [LOST, LOST, 9, 9]


@pytest.mark.skipif(nxec.device_count() > 0, reason="a GPU is visible")
def test_calls_without_a_device_fail_loudly():
    """No CPU fallback on either path: with work to do and no usable device the call reports NXEC_ERR_NODEV.
    A zeroed block stands in for a context (the call reads its device index and fails at the device check)."""
    stand_in = ctypes.create_string_buffer(8192)
    ctx = ctypes.cast(stand_in, ctypes.c_void_p)
    assert mixed_call(ctx) == _lib.NXEC_ERR_NODEV  # one-launch shape
    assert mixed_call(ctx, alive="none") == _lib.NXEC_ERR_NODEV  # a clean batch is work too: k copies
    assert mixed_call(ctx, length=61) == _lib.NXEC_ERR_NODEV  # by-runs shape: the tail
    assert mixed_call(ctx, out=OUT + 3) == _lib.NXEC_ERR_NODEV  # by-runs shape: the output base
    assert mixed_call(ctx, n=24, k=21, cs=64, ss=24 * 64, oss=21 * 64) == _lib.NXEC_ERR_NODEV  # by-runs shape: k > 19
    assert object_call(ctx) == _lib.NXEC_ERR_NODEV
    assert object_call(ctx, alive=(ctypes.c_ubyte * 6)(1, 0, 1, 1, 1, 1), length=5) == _lib.NXEC_ERR_NODEV  # only a last stripe


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
    """tests/cpp/decode_mixed_plan_test.cc: the planner and the device tables it builds as a plain host
    program built with -fsanitize=address,undefined (its own main; nothing is preloaded here)."""
    run_program("decode_mixed_plan_test", "decode_mixed_plan_test ok", sanitized=True)


def test_every_decode_mixed_kernel_is_prepared():
    """tests/cpp/mixed_registry_test.cc: every k_decode_mixed instantiation is in the per-device
    preparation list with at least the LDS its launch asks for."""
    run_program("mixed_registry_test", "mixed_registry_test ok", sanitized=False)
