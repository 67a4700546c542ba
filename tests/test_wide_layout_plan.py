"""The 4 GiB stripe limit on the host (CPU only): "(n-1)*chunk_stride + len <= 2^32 - 1" at its boundary.

The largest layout the contract accepts passes the plan calls and the argument checks of every device call that
checks its layout before it uses a device (scrub, mixed recover, mixed decode on its source and on its output
side, update); one byte more gives NXEC_ERR_INVALID.  Two shapes: a 16-byte aligned layout whose last chunk ends
at 2^32 - 16, and an unaligned one that ends exactly at 2^32 - 1.  No device memory is touched: every buffer is an
address only.  That the accepted layouts also compute the right bytes is tests/test_gpu_wide_layout.py.

A call that passes its checks goes on to the device.  So the accepted half of the device calls runs where no GPU is
visible: a zeroed block stands in for the context, and the call fails at the device check with NXEC_ERR_NODEV -- past
the layout check and before any pointer is used.  The refused half runs everywhere.
"""
import ctypes
import os
import subprocess

import pytest

from nexoedge_amd import _lib, nxec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NODEV, OK = _lib.NXEC_ERR_INVALID, _lib.NXEC_ERR_NODEV, _lib.NXEC_OK
G4 = 1 << 32
BATCH = 0x7000_0000_0000  # 16-byte aligned stand-ins for device addresses, far from each other
OTHER = 0x7400_0000_0000
NEW = 0x7800_0000_0000
SS = G4 + (1 << 20)

# (n, k, chunk stride, len, the smallest len past the limit that keeps the shape)
ALIGNED = (6, 4, 858990176, 16400, 16416)
EXACT = (6, 4, 858992638, 4105, 4106)
WIDE_CODE = (24, 21, 186736992, 16464, 16480)  # k > 19: the by-runs and byte paths of mixed and update
SHAPES = {"aligned": ALIGNED, "exact": EXACT, "k21": WIDE_CODE}


def test_shapes_sit_on_the_limit():
    for n, k, cs, ln, over in SHAPES.values():
        assert (n - 1) * cs + ln <= G4 - 1 < (n - 1) * cs + over
    n, k, cs, ln, _ = EXACT
    assert (n - 1) * cs + ln == G4 - 1
    n, k, cs, ln, _ = ALIGNED
    assert (n - 1) * cs + ln == G4 - 16 and cs % 16 == 0


def out_limit(k, ln):
    """The output side of a decode at its limit, k chunks: (out chunk stride, the largest len it takes, the
    smallest it refuses), 16-byte aligned when `ln` is.  The largest len is `ln` or a little more."""
    step = 16 if ln % 16 == 0 else 1
    ocs = (G4 - step - ln) // (k - 1) // step * step
    at = G4 - step - (k - 1) * ocs
    assert ln <= at <= ocs and (k - 1) * ocs + at <= G4 - 1 < (k - 1) * ocs + at + step
    return ocs, at, at + step


def updates(k, ln):
    """The last bytes of data chunk k-1, five unaligned bytes of chunk 0, a whole chunk of stripe 1."""
    return [(0, k - 1, ln - 2048, 2048, NEW), (0, 0, 3, 5, NEW + (1 << 24) + 3), (1, k // 2, 0, ln, NEW + (2 << 24))]


def update_list(ups):
    arr = (_lib.Update * len(ups))()
    for u, (s, c, off, ln, p) in zip(arr, ups):
        u.stripe, u.chunk, u.reserved, u.offset, u.length, u.d_new = s, c, 0, off, ln, p
    return arr


def update_plan(n, k, cs, ln, base=BATCH):
    cnt = [ctypes.c_int64(-7) for _ in range(3)]
    ups = updates(k, ln)
    rc = _lib.lib.nxec_rs_update_plan(n, k, cs, SS, ln, 2, base, update_list(ups), len(ups), *cnt)
    return rc, tuple(c.value for c in cnt)


def update_call(ctx, n, k, cs, ln, base=BATCH):
    ups = updates(k, ln)
    return _lib.lib.nxec_rs_update_stripes(ctx, n, k, ctypes.c_void_p(base), cs, SS, ln, 2, update_list(ups), len(ups), None)


def alive(n, k):
    a = [1] * (2 * n)
    a[0] = a[n + k] = 0  # stripe 0 lost chunk 0, stripe 1 chunk k
    return (ctypes.c_ubyte * (2 * n))(*a)


def recover_mixed_call(ctx, n, k, cs, ln, base=BATCH):
    res = (ctypes.c_int32 * 2)(9, 9)
    rc = _lib.lib.nxec_rs_recover_stripes_mixed(ctx, n, k, alive(n, k), ctypes.c_void_p(base), cs, SS, ln, 2, res, None)
    return rc, list(res)


def decode_mixed_call(ctx, n, k, cs, ss, ocs, oss, ln, src=BATCH, out=OTHER):
    res = (ctypes.c_int32 * 2)(9, 9)
    rc = _lib.lib.nxec_rs_decode_stripes_mixed(ctx, n, k, alive(n, k), ctypes.c_void_p(src), cs, ss,
                                               ctypes.c_void_p(out), ocs, oss, ln, 2, res, None)
    return rc, list(res)


def scrub_call(ctx, n, k, cs, ln, flags=0, base=BATCH):
    return _lib.lib.nxec_rs_scrub_stripes(ctx, n, k, ctypes.c_void_p(base), cs, SS, ln, 2, flags, ctypes.c_void_p(OTHER),
                                          None, None)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_update_plan_takes_the_limit_and_refuses_one_byte_more(shape):
    n, k, cs, ln, over = SHAPES[shape]
    rc, (rounds, tiles, items) = update_plan(n, k, cs, ln)
    assert rc == OK and rounds == 1
    if shape == "aligned":
        assert (tiles, items) == (1 + 2, 1)  # 2048 bytes and a chunk of 1025 vectors in tiles of 1024; 5 loose bytes
    else:
        assert (tiles, items) == (0, 3)  # unaligned strides, or k > 19: everything by bytes
    assert update_plan(n, k, cs, over) == (INVALID, (-7, -7, -7))  # refused calls write nothing
    # the base address does not enter the rule
    assert update_plan(n, k, cs, ln, base=BATCH + 3)[0] == OK and update_plan(n, k, cs, over, base=BATCH + 3)[0] == INVALID


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_calls_refuse_one_byte_more_before_any_device_use(shape):
    """The context and the buffers are never valid here: the refusal comes before either is touched."""
    n, k, cs, ln, over = SHAPES[shape]
    fake = ctypes.c_void_p(1)
    assert update_call(fake, n, k, cs, over) == INVALID
    assert recover_mixed_call(fake, n, k, cs, over) == (INVALID, [9, 9])
    for flags in (0, nxec.SCRUB_LOCATE, nxec.SCRUB_REPAIR):
        assert scrub_call(fake, n, k, cs, over, flags) == INVALID
    # mixed decode, the source side: a packed output is fine, the wide source is one byte too long
    assert decode_mixed_call(fake, n, k, cs, SS, over, k * over, over) == (INVALID, [9, 9])
    # the output side: a packed source is fine, the k output chunks end one byte too far
    ocs, _, over = out_limit(k, ln)
    assert decode_mixed_call(fake, n, k, over, n * over, ocs, SS, over) == (INVALID, [9, 9])
    assert b"4 GiB" in _lib.lib.nxec_last_error()


@pytest.mark.parametrize("n,k", [(6, 4), (24, 21), (128, 124)])
def test_a_stride_whose_product_overflows_int64_is_refused(n, k):
    """chunk_stride = 2^57: (n-1) * chunk_stride is merely huge for the small codes and wraps a signed 64-bit product
    for n = 128, to -2^57, which passes for a layout within 4 GiB.  The recover, the scrub and the update used to
    multiply before they compared; all three refuse the stride by the 4 GiB rule, before the context or a buffer
    is touched."""
    cs, ln, fake = 1 << 57, 4096, ctypes.c_void_p(1)
    assert (n - 1) * cs + ln > G4 - 1 and (n < 128 or (n - 1) * cs >= 1 << 63)
    last_error = _lib.lib.nxec_last_error
    assert update_plan(n, k, cs, ln) == (INVALID, (-7, -7, -7)) and b"4 GiB" in last_error()
    assert update_call(fake, n, k, cs, ln) == INVALID and b"update" in last_error() and b"4 GiB" in last_error()
    assert recover_mixed_call(fake, n, k, cs, ln) == (INVALID, [9, 9])
    assert b"mixed recover" in last_error() and b"4 GiB" in last_error()
    for flags in (0, nxec.SCRUB_LOCATE, nxec.SCRUB_REPAIR):
        assert scrub_call(fake, n, k, cs, ln, flags) == INVALID
        assert b"scrub" in last_error() and b"4 GiB" in last_error()


@pytest.mark.skipif(nxec.device_count() > 0, reason="a GPU is visible")
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_calls_take_the_limit(shape):
    """At the limit every one of them passes its layout check and fails at the device check."""
    n, k, cs, ln, _ = SHAPES[shape]
    stand_in = ctypes.create_string_buffer(8192)
    ctx = ctypes.cast(stand_in, ctypes.c_void_p)
    assert update_call(ctx, n, k, cs, ln) == NODEV
    assert recover_mixed_call(ctx, n, k, cs, ln)[0] == NODEV
    for flags in (0, nxec.SCRUB_LOCATE, nxec.SCRUB_REPAIR):
        assert scrub_call(ctx, n, k, cs, ln, flags) == NODEV
    assert decode_mixed_call(ctx, n, k, cs, SS, ln, k * ln, ln)[0] == NODEV
    ocs, at, _ = out_limit(k, ln)
    assert decode_mixed_call(ctx, n, k, at, n * at, ocs, SS, at)[0] == NODEV


def test_standalone_layout_rules_program_under_sanitizers():
    """tests/cpp/md5_layout_test.cc: chunk_off32, the fused multiply + MD5 eligibility and the stripes-per-group
    cap of its launch as a plain host program built with -fsanitize=address,undefined (its own main; nothing is
    preloaded here)."""
    exe = os.path.join(ROOT, "build", "md5_layout_test")
    assert os.path.exists(exe), "build/md5_layout_test missing: run make (or __graft_entry__.build())"
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "not a sanitizer build"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "md5_layout_test ok" in r.stdout
