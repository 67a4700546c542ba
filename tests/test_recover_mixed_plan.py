"""Mixed-pattern recover, host side (CPU only): the per-stripe verdicts and
plan counters of nxec_rs_recover_mixed_plan against a brute-force evaluation
with nxec_rs_plan, the argument validation of the plan call and of
nxec_rs_recover_stripes_mixed, and the two stand-alone C++ programs
(tests/cpp/recover_mixed_plan_test.cc under ASan + UBSan,
tests/cpp/mixed_registry_test.cc against libnxec).

Every erasure set of 1..n-k chunks is one stripe.  The pinned counts are the
number of such sets, sum_{e=1..n-k} C(n, e), and the number of them whose first
k alive chunks do not invert (only RS(12,6) has any: ten sets of 5 or 6 chunks).
"""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from nexoedge_amd import _lib, nxec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOST, SINGULAR = nxec.RECOVER_LOST, nxec.RECOVER_SINGULAR
# (n, k): (sets of 1..n-k chunks, singular ones)
PINNED = {(6, 4): (21, 0), (14, 10): (1470, 0), (10, 4): (847, 0), (23, 19): (10902, 0), (12, 6): (2509, 10)}


def erasure_sets(n, lo, hi):
    return [e for size in range(lo, hi + 1) for e in itertools.combinations(range(n), size)]


def alive_map(n, sets):
    a = np.ones((len(sets), n), dtype=np.uint8)
    for s, e in enumerate(sets):
        a[s, list(e)] = 0
    return a


def brute(n, k, e):
    """The verdict of one stripe from nxec_rs_plan itself."""
    if not e:
        return 0
    if len(e) > n - k:
        return LOST
    f = (ctypes.c_int32 * len(e))(*e)
    inputs = (ctypes.c_int32 * n)()
    rm = (ctypes.c_ubyte * (len(e) * k))()
    ni, mi = ctypes.c_int(), ctypes.c_int()
    rc = _lib.lib.nxec_rs_plan(n, k, f, len(e), 1, inputs, ctypes.byref(ni), ctypes.byref(mi), rm)
    assert rc in (_lib.NXEC_OK, _lib.NXEC_ERR_SINGULAR), rc
    return len(e) if rc == _lib.NXEC_OK else SINGULAR


@pytest.mark.parametrize("n,k", sorted(PINNED))
def test_plan_against_brute_force(n, k):
    sets = erasure_sets(n, 1, n - k)
    want = np.array([brute(n, k, e) for e in sets], dtype=np.int32)
    res, npat, nseg, ncoded = nxec.rs_recover_mixed_plan(n, k, alive_map(n, sets))
    assert np.array_equal(res, want)
    assert len(sets) == PINNED[(n, k)][0] == sum(math.comb(n, e) for e in range(1, n - k + 1))
    assert int((want == SINGULAR).sum()) == PINNED[(n, k)][1]
    ok = want > 0
    assert npat == ncoded == int(ok.sum())  # every stripe its own pattern
    assert nseg == int(((want[ok] + 3) // 4).sum())


def test_singular_sets_of_rs_12_6():
    sets = erasure_sets(12, 1, 6)
    res, _, _, _ = nxec.rs_recover_mixed_plan(12, 6, alive_map(12, sets))
    bad = [e for e, r in zip(sets, res) if r == SINGULAR]
    assert len(bad) == 10 and all(len(e) in (5, 6) for e in bad)
    assert (0, 2, 5, 7, 8) in bad and (0, 3, 5, 8, 9) in bad


@pytest.mark.parametrize("n,k", [(6, 4), (14, 10), (10, 4), (12, 6), (5, 4), (4, 4)])
def test_lost_and_clean_stripes(n, k):
    sets = erasure_sets(n, n - k + 1, n - k + 1) + [tuple(range(n)), ()]
    res, npat, nseg, ncoded = nxec.rs_recover_mixed_plan(n, k, alive_map(n, sets))
    assert res.tolist() == [LOST] * (len(sets) - 1) + [0]
    assert (npat, nseg, ncoded) == (0, 0, 0)


def test_counters_match_numpy_and_patterns_count_once():
    n, k, ns = 14, 10, 3000
    rng = np.random.default_rng(11)
    a = rng.integers(1, 256, size=(ns, n), dtype=np.uint8)  # any non-zero byte is alive
    for s in range(ns):
        a[s, rng.integers(0, n, size=rng.integers(0, 7))] = 0  # 0..6 erased: some are lost
    res, npat, nseg, ncoded = nxec.rs_recover_mixed_plan(n, k, a)
    ne = (a == 0).sum(axis=1)
    assert np.array_equal(res, np.where(ne > n - k, LOST, ne))  # RS(14,10) has no singular set
    coded = res > 0
    pats = {tuple(np.flatnonzero(row == 0)) for row in a[coded]}
    assert ncoded == int(coded.sum()) and npat == len(pats) < ncoded
    assert nseg == sum((len(p) + 3) // 4 for p in pats)
    # the batch twice over: no new pattern
    res2, npat2, nseg2, ncoded2 = nxec.rs_recover_mixed_plan(n, k, np.concatenate([a, a]))
    assert np.array_equal(res2, np.concatenate([res, res])) and (npat2, nseg2, ncoded2) == (npat, nseg, 2 * ncoded)
    # one pattern of six erased chunks on RS(10,4): two segments, however many stripes share it
    one = alive_map(10, [(0, 1, 2, 3, 4, 5)] * 7)
    assert nxec.rs_recover_mixed_plan(10, 4, one)[1:] == (1, 2, 7)
    assert nxec.rs_recover_mixed_plan(6, 4, np.zeros((0, 6), dtype=np.uint8))[1:] == (0, 0, 0)


def test_plan_call_validates():
    L = _lib.lib
    a = (ctypes.c_ubyte * 12)(*([1] * 12))
    res = (ctypes.c_int32 * 2)(7, 7)
    cnt = ctypes.c_int64(7)
    for n, k in ((0, 0), (4, 5), (6, 0), (129, 4), (130, 128)):
        assert L.nxec_rs_recover_mixed_plan(n, k, a, 1, res, cnt, cnt, cnt) == _lib.NXEC_ERR_INVALID, (n, k)
    assert L.nxec_rs_recover_mixed_plan(6, 4, None, 1, res, cnt, cnt, cnt) == _lib.NXEC_ERR_INVALID
    assert L.nxec_rs_recover_mixed_plan(6, 4, a, -1, res, cnt, cnt, cnt) == _lib.NXEC_ERR_INVALID
    assert list(res) == [7, 7] and cnt.value == 7  # refused calls write nothing
    assert L.nxec_rs_recover_mixed_plan(6, 4, None, 0, None, None, None, None) == _lib.NXEC_OK  # everything optional
    assert L.nxec_rs_recover_mixed_plan(6, 4, a, 2, res, None, None, None) == _lib.NXEC_OK and list(res) == [0, 0]


def mixed_call(ctx, n=6, k=4, alive="one", stripes=ctypes.c_void_p(4096), cs=64, ss=6 * 64, length=64, ns=1,
               result=None):
    if isinstance(alive, str):
        row = [0] + [1] * (n - 1) if alive == "one" else [1] * n
        alive = (ctypes.c_ubyte * (n * max(ns, 1)))(*(row * max(ns, 1)))
    return _lib.lib.nxec_rs_recover_stripes_mixed(ctx, n, k, alive, stripes, cs, ss, length, ns, result, None)


def test_batch_call_rejects_arguments_before_device_use():
    """Bad arguments are refused before the context or any device pointer is touched (neither is ever valid
    here), and a call with nothing to code returns its verdicts without a device."""
    fake = ctypes.c_void_p(1)
    res = (ctypes.c_int32 * 4)(9, 9, 9, 9)
    assert mixed_call(None) == _lib.NXEC_ERR_INVALID  # no context
    for n, k in ((0, 0), (4, 5), (6, 0), (129, 4), (130, 128)):
        assert mixed_call(fake, n=n, k=k, alive=(ctypes.c_ubyte * 256)()) == _lib.NXEC_ERR_INVALID, (n, k)
    assert mixed_call(fake, alive=None) == _lib.NXEC_ERR_INVALID
    assert mixed_call(fake, length=-1) == _lib.NXEC_ERR_INVALID
    assert mixed_call(fake, ns=-1) == _lib.NXEC_ERR_INVALID
    assert mixed_call(fake, stripes=None, result=res) == _lib.NXEC_ERR_INVALID  # work to do, no buffer
    assert mixed_call(fake, cs=-16, result=res) == _lib.NXEC_ERR_INVALID
    assert mixed_call(fake, cs=1 << 30, ss=6 << 30, result=res) == _lib.NXEC_ERR_INVALID  # chunks beyond 4 GiB
    assert list(res) == [9, 9, 9, 9]  # refused calls write nothing
    # nothing to launch: the verdicts are still filled, and no device is needed
    assert mixed_call(fake, alive=None, ns=0) == _lib.NXEC_OK
    assert mixed_call(fake, length=0, stripes=None, result=res) == _lib.NXEC_OK and res[0] == 1
    assert mixed_call(fake, alive="none", stripes=None, ns=3, result=res) == _lib.NXEC_OK and list(res) == [0, 0, 0, 9]
    lost = (ctypes.c_ubyte * 6)(0, 0, 0, 1, 1, 1)
    assert mixed_call(fake, alive=lost, stripes=None, result=res) == _lib.NXEC_OK and res[0] == LOST
    assert mixed_call(fake, n=4, k=4, alive=(ctypes.c_ubyte * 4)(1, 0, 1, 1), stripes=None, cs=64, ss=256,
                      result=res) == _lib.NXEC_OK and res[0] == LOST  # n == k: nothing can be rebuilt
    sing = (ctypes.c_ubyte * 12)(*[0 if c in (0, 2, 5, 7, 8) else 1 for c in range(12)])
    assert mixed_call(fake, n=12, k=6, alive=sing, stripes=None, ss=12 * 64, result=res) == _lib.NXEC_OK
    assert res[0] == SINGULAR


@pytest.mark.skipif(nxec.device_count() > 0, reason="a GPU is visible")
def test_batch_call_without_a_device_fails_loudly():
    """No CPU fallback on either path: with work to do and no usable device the call reports NXEC_ERR_NODEV.
    A zeroed block stands in for a context (the call reads its device index and fails at the device check)."""
    stand_in = ctypes.create_string_buffer(8192)
    ctx = ctypes.cast(stand_in, ctypes.c_void_p)
    assert mixed_call(ctx) == _lib.NXEC_ERR_NODEV  # one-launch shape
    assert mixed_call(ctx, length=61) == _lib.NXEC_ERR_NODEV  # by-runs shape


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
    """tests/cpp/recover_mixed_plan_test.cc: the planner and the device tables it builds as a plain host
    program built with -fsanitize=address,undefined (its own main; nothing is preloaded here)."""
    run_program("recover_mixed_plan_test", "recover_mixed_plan_test ok", sanitized=True)


def test_every_mixed_kernel_is_prepared():
    """tests/cpp/mixed_registry_test.cc: for k = 1..19 the kernel the mixed launch picks is in the
    per-device preparation list with at least the LDS the launch asks for."""
    run_program("mixed_registry_test", "mixed_registry_test ok", sanitized=False)
