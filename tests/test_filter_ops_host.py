"""CPU tier of the filter algebra (cph_filters_combine): the host statement of the device pass.

tests/filter_ops_host/filter_ops_host.cpp includes csrc/host_index.h and is built with plain g++ and
-fsanitize=address,undefined, the way tests/test_labels_host.py builds its driver (a stand-alone program; nothing loaded
into Python runs under a sanitizer).  `eval` runs filter_combine_host on data written by this test, on exact-size buffers
pre-filled with garbage, and the results are compared with numpy (tests/filter_ops_model.py); `self` compares them with a
bit-by-bit loop.  cph_host_filter_combine (the library's host-only hook, no HIP call) is compared with numpy on the same
cases, and the argument errors of the hooks and of cph_filters_combine that need no device are checked."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from filter_ops_model import OPS, cases, expect, nwords, operands

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "filter_ops_host", "filter_ops_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]

SIZES = [0, 1, 31, 32, 33, 127, 128, 129, 2047, 2049, 4100]
FILTER_COUNTS = [1, 3, 70]


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("filter_ops_host")), "filter_ops_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(cmd, timeout=600):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    return r.stdout


def test_combine_statement_against_a_loop_under_asan_ubsan(asan_exe):
    assert "self: ok" in _run([asan_exe, "self"])


@pytest.mark.parametrize("n_bits", SIZES)
def test_combine_statement_against_numpy_under_asan_ubsan(asan_exe, tmp_path, n_bits):
    """filter_combine_host, every m, op and form of b, against numpy: words and counts; dirty tails do not leak."""
    nw = nwords(n_bits)
    for m in FILTER_COUNTS:
        a, b = operands(n_bits, m, 1000 * n_bits + m)
        for op, bc in cases():
            bb = None if op == "not" else b[:1] if bc else b
            fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(fin, "wb") as f:
                f.write(np.array([OPS[op], n_bits, m, int(bc)], np.uint64).tobytes() + a.tobytes() + (b"" if bb is None else bb.tobytes()))
            assert "eval: ok" in _run([asan_exe, "eval", fin, fout])
            raw = open(fout, "rb").read()
            assert len(raw) == m * nw * 4 + m * 8
            words = np.frombuffer(raw, np.uint32, m * nw).reshape(m, nw)
            counts = np.frombuffer(raw, np.uint64, m, m * nw * 4)
            ew, ec = expect(op, a, bb, n_bits)
            assert np.array_equal(words, ew), (op, bc, m)      # every word written, tail bits of the last word clear
            assert np.array_equal(counts, ec), (op, bc, m)


def _ptr(x):
    return None if x is None or x.size == 0 else x.ctypes.data


@pytest.mark.parametrize("n_bits", SIZES)
@pytest.mark.parametrize("m", FILTER_COUNTS)
def test_host_filter_combine_hook_matches_numpy(n_bits, m):
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    a, b = operands(n_bits, m, 1000 * n_bits + m)
    for op, bc in cases():
        bb = None if op == "not" else np.ascontiguousarray(b[:1]) if bc else b
        words = np.full((m, nwords(n_bits)), 0xDEADBEEF, np.uint32)
        counts = np.full(m, 12345, np.uint64)
        _lib.check(L.cph_host_filter_combine(OPS[op], _ptr(a), _ptr(bb), int(bc), n_bits, m, _ptr(words), counts.ctypes.data))
        ew, ec = expect(op, a, bb, n_bits)
        assert np.array_equal(words, ew), (op, bc)
        assert np.array_equal(counts, ec), (op, bc)


def test_host_filter_combine_hook_edges():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    assert L.cph_version() >= 108
    assert L.cph_host_filter_combine(0, None, None, 0, 64, 0, None, None) == _lib.OK          # m == 0: nothing to do
    w = np.zeros((1, 2), np.uint32)
    c = np.zeros(1, np.uint64)
    ok = (w.ctypes.data, w.ctypes.data, 0, 64, 1, w.ctypes.data, c.ctypes.data)
    assert L.cph_host_filter_combine(0, *ok) == _lib.OK
    for bad_op in (-1, 5, 99):
        assert L.cph_host_filter_combine(bad_op, *ok) == _lib.INVALID_ARGUMENT
    assert L.cph_host_filter_combine(0, None, w.ctypes.data, 0, 64, 1, w.ctypes.data, c.ctypes.data) == _lib.INVALID_ARGUMENT
    assert L.cph_host_filter_combine(0, w.ctypes.data, None, 0, 64, 1, w.ctypes.data, c.ctypes.data) == _lib.INVALID_ARGUMENT
    assert L.cph_host_filter_combine(0, w.ctypes.data, w.ctypes.data, 0, 64, 1, None, c.ctypes.data) == _lib.INVALID_ARGUMENT
    assert L.cph_host_filter_combine(0, w.ctypes.data, w.ctypes.data, 0, 64, 1, w.ctypes.data, None) == _lib.INVALID_ARGUMENT
    assert L.cph_host_filter_combine(4, w.ctypes.data, w.ctypes.data, 0, 64, 1, w.ctypes.data, c.ctypes.data) == _lib.INVALID_ARGUMENT  # NOT with b
    assert L.cph_host_filter_combine(4, w.ctypes.data, None, 0, 64, 1, w.ctypes.data, c.ctypes.data) == _lib.OK
    assert L.cph_host_filter_combine(0, w.ctypes.data, w.ctypes.data, 0, 2 ** 32, 1, w.ctypes.data, c.ctypes.data) == _lib.INVALID_ARGUMENT
    with pytest.raises(ValueError):
        _lib.check(L.cph_host_filter_combine(7, *ok))


def test_filters_combine_argument_errors_need_no_device():
    """What cph_filters_combine and its parts form refuse before they look at a filter."""
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    out = (C.c_void_p * 2)(1, 1)
    one = (C.c_void_p * 2)(None, None)
    for fn in (L.cph_filters_combine, L.cph_parts_filters_combine):
        assert fn(0, None, 0, None, 0, None) == _lib.OK                      # m == 0 touches nothing
        assert fn(0, one, 0, one, 5, out) == _lib.OK and out[0] == 1
        assert fn(0, one, 2, one, 2, None) == _lib.INVALID_ARGUMENT          # no out
        assert fn(0, None, 2, one, 2, out) == _lib.INVALID_ARGUMENT and out[0] is None and out[1] is None
        assert fn(9, one, 2, one, 2, out) == _lib.INVALID_ARGUMENT           # unknown op
        assert fn(-1, one, 2, one, 2, out) == _lib.INVALID_ARGUMENT
        assert fn(0, one, 2, one, 0, out) == _lib.INVALID_ARGUMENT           # n_b not in {m, 1}
        assert fn(0, one, 2, None, 2, out) == _lib.INVALID_ARGUMENT          # no b for a binary op
        assert fn(4, one, 2, one, 2, out) == _lib.INVALID_ARGUMENT           # NOT with b
        assert fn(4, one, 2, None, 1, out) == _lib.INVALID_ARGUMENT          # NOT with n_b
        assert fn(0, one, 2, one, 2, out) == _lib.INVALID_ARGUMENT           # null entries
        assert b"null filter" in L.cph_last_error()
        out[0] = out[1] = 1


def test_column_slot_arguments_need_no_device():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    f = C.c_int(0)
    assert L.cph_set_column(None, 0, None, 0, 0) == _lib.INVALID_ARGUMENT
    assert L.cph_has_column(None, 0, C.byref(f)) == _lib.INVALID_ARGUMENT
    assert L.cph_get_column(None, 8, 0, 0, None) == _lib.INVALID_ARGUMENT
    assert L.cph_filters_from_column(None, 0, None, None, 0, None) == _lib.OK
    assert L.cph_multi_set_column(None, 0, None, 0, 0) == _lib.INVALID_ARGUMENT
    assert L.cph_parts_set_column(None, 8, None, 0) == _lib.INVALID_ARGUMENT
    assert L.cph_parts_filters_from_column(None, 0, None, None, 0, None) == _lib.OK
