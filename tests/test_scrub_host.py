"""Parity scrub, host side (CPU only): the per-byte rule behind
nxec_rs_scrub_stripes -- which single chunk explains an (n-k)-byte syndrome --
through nxec_rs_syndrome_locate, the batch call's argument validation, and the
stand-alone sanitizer build of the same rule (tests/cpp/scrub_host_test.cc).

Expected results follow from the construction: the syndrome of an error e in
chunk c is e times column c of H = [C | I], C the parity rows of
gf_gen_rs_matrix.  Any two columns of H are independent (n-k >= 2), any three
when n-k >= 3, so one bad chunk is always located and two are never mistaken
for one.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from nexoedge_amd import _lib, nxec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERRORS = (1, 0x53, 0xFF)


def gf_mul_table():
    """256 x 256 products over 0x11d, from the library's own gf_mul (checked against the goldens elsewhere)."""
    exp = np.zeros(512, dtype=np.int64)
    log = np.zeros(256, dtype=np.int64)
    v = 1
    for i in range(255):
        exp[i] = v
        log[v] = i
        v <<= 1
        if v & 0x100:
            v ^= 0x11D
    exp[255:510] = exp[:255]
    t = exp[(log[:, None] + log[None, :])]
    t[0, :] = 0
    t[:, 0] = 0
    return t.astype(np.uint8)


MUL = gf_mul_table()


def columns(n, k):
    """H = [C | I] as an (n-k) x n array: column c is the syndrome of a unit error in chunk c."""
    c = nxec.gen_rs_matrix(n, k)[k:]
    return np.concatenate([c, np.eye(n - k, dtype=np.uint8)], axis=1)


def syndrome(h, c, e):
    return MUL[h[:, c], e]


def geometries(golden, pred):
    seen = sorted({(m["n"], m["k"]) for m in golden["matrices"]})
    return [g for g in seen if pred(*g)]


def test_mul_table_is_the_librarys_field():
    for a, b in [(2, 0x80), (0x53, 0xCA), (0xFF, 0xFF), (1, 0x1D), (0, 7)]:
        assert MUL[a, b] == nxec.gf_mul(a, b)


def test_single_error_is_located_with_its_value(golden):
    geoms = geometries(golden, lambda n, k: n - k >= 2)
    assert geoms
    for n, k in geoms:
        h = columns(n, k)
        assert nxec.syndrome_locate(n, k, np.zeros(n - k, np.uint8)) == (nxec.SCRUB_CLEAN, 0)
        for c in range(n):
            for e in ERRORS:
                assert nxec.syndrome_locate(n, k, syndrome(h, c, e)) == (c, e), (n, k, c, e)


def test_two_errors_are_never_mistaken_for_one(golden):
    geoms = geometries(golden, lambda n, k: n - k >= 3 and n <= 20)
    assert geoms
    for n, k in geoms:
        h = columns(n, k)
        for a, b in itertools.combinations(range(n), 2):
            for ea, eb in ((1, 1), (0x53, 0xCA)):
                s = syndrome(h, a, ea) ^ syndrome(h, b, eb)
                assert nxec.syndrome_locate(n, k, s) == (nxec.SCRUB_UNLOCATED, 0), (n, k, a, b, ea, eb)


def test_one_parity_row_detects_only(golden):
    geoms = geometries(golden, lambda n, k: n - k == 1) + [(5, 4), (128, 127)]
    for n, k in geoms:
        assert nxec.syndrome_locate(n, k, [0]) == (nxec.SCRUB_CLEAN, 0)
        for e in (1, 2, 0x53, 0xFF):
            assert nxec.syndrome_locate(n, k, [e]) == (nxec.SCRUB_UNLOCATED, 0), (n, k, e)


def test_wider_codes_than_the_goldens():
    """(24,21) and (26,22): the byte-fallback shapes of the GPU scrub."""
    for n, k in ((24, 21), (26, 22)):
        h = columns(n, k)
        for c in range(n):
            for e in ERRORS:
                assert nxec.syndrome_locate(n, k, syndrome(h, c, e)) == (c, e)
        for a, b in itertools.combinations(range(n), 2):
            s = syndrome(h, a, 0x53) ^ syndrome(h, b, 0xCA)
            assert nxec.syndrome_locate(n, k, s)[0] == nxec.SCRUB_UNLOCATED, (n, k, a, b)


def test_syndrome_locate_validates():
    L = _lib.lib
    chunk, err = ctypes.c_int32(7), ctypes.c_ubyte(7)
    syn = (ctypes.c_ubyte * 4)()
    for n, k in ((0, 0), (4, 5), (6, 0), (129, 4), (130, 128)):
        assert L.nxec_rs_syndrome_locate(n, k, syn, ctypes.byref(chunk), ctypes.byref(err)) == _lib.NXEC_ERR_INVALID
    assert L.nxec_rs_syndrome_locate(6, 4, None, ctypes.byref(chunk), ctypes.byref(err)) == _lib.NXEC_ERR_INVALID
    assert L.nxec_rs_syndrome_locate(6, 4, syn, None, ctypes.byref(err)) == _lib.NXEC_ERR_INVALID
    assert chunk.value == 7  # refused calls write nothing
    assert L.nxec_rs_syndrome_locate(6, 4, syn, ctypes.byref(chunk), None) == _lib.NXEC_OK  # error is optional
    assert chunk.value == nxec.SCRUB_CLEAN


def scrub_call(ctx, n=6, k=4, stripes=ctypes.c_void_p(4096), cs=64, ss=6 * 64, length=64, ns=1, flags=0,
               status=ctypes.c_void_p(8192), nbad=None):
    return _lib.lib.nxec_rs_scrub_stripes(ctx, n, k, stripes, cs, ss, length, ns, flags, status, nbad, None)


def test_scrub_arguments_rejected_before_device_use():
    """Bad n, k, flags, sizes and a NULL status array are refused before the
    context or any pointer is touched (the pointers here are never valid)."""
    fake = ctypes.c_void_p(1)
    assert scrub_call(None) == _lib.NXEC_ERR_INVALID  # no context
    for n, k in ((0, 0), (4, 5), (6, 0), (129, 4), (130, 128)):
        assert scrub_call(fake, n=n, k=k) == _lib.NXEC_ERR_INVALID, (n, k)
    for flags in (4, 8, -1, nxec.SCRUB_LOCATE | 4, 1 << 16):
        assert scrub_call(fake, flags=flags) == _lib.NXEC_ERR_INVALID, flags
    assert scrub_call(fake, status=None) == _lib.NXEC_ERR_INVALID
    assert scrub_call(fake, status=None, ns=0) == _lib.NXEC_ERR_INVALID
    assert scrub_call(fake, length=-1) == _lib.NXEC_ERR_INVALID
    assert scrub_call(fake, ns=-1) == _lib.NXEC_ERR_INVALID
    assert scrub_call(fake, stripes=None) == _lib.NXEC_ERR_INVALID
    assert scrub_call(fake, cs=-16) == _lib.NXEC_ERR_INVALID
    assert scrub_call(fake, cs=1 << 30, ss=6 << 30) == _lib.NXEC_ERR_INVALID  # chunks of a stripe beyond 4 GiB
    assert b"scrub" in _lib.lib.nxec_last_error() or b"invalid" in _lib.lib.nxec_last_error()
    # no stripes: nothing to reset, nothing launched, no device needed
    assert scrub_call(fake, ns=0) == _lib.NXEC_OK


@pytest.mark.skipif(nxec.device_count() > 0, reason="a GPU is visible")
def test_scrub_without_a_device_fails_loudly():
    """No CPU fallback: with valid arguments and no usable device the batch
    call reports NXEC_ERR_NODEV.  A context cannot be created without a device,
    so a zeroed block stands in for one: the call reads its device index (0)
    and fails at the device check, before anything else of it is used."""
    stand_in = ctypes.create_string_buffer(8192)
    ctx = ctypes.cast(stand_in, ctypes.c_void_p)
    for flags in (0, nxec.SCRUB_LOCATE, nxec.SCRUB_REPAIR):
        assert scrub_call(ctx, flags=flags) == _lib.NXEC_ERR_NODEV
    assert scrub_call(ctx, length=0) == _lib.NXEC_ERR_NODEV  # the statuses would still be reset on the device


def test_standalone_rule_program_under_sanitizers():
    """tests/cpp/scrub_host_test.cc: the rule and the matrix generator as a
    plain host program built with -fsanitize=address,undefined (its own main;
    nothing is preloaded into this interpreter)."""
    exe = os.path.join(ROOT, "build", "scrub_host_test")
    assert os.path.exists(exe), "build/scrub_host_test missing: run make (or __graft_entry__.build())"
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "not a sanitizer build"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scrub_host_test ok" in r.stdout
