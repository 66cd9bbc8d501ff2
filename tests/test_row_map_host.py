"""CPU tier of the row map (input row of every internal id): the native file's `rows` section and the host statement
of the row-space filter.

tests/row_map_san/row_map_san.cpp includes csrc/host_index.h and csrc/native_file.h and is built with plain g++ and
-fsanitize=address,undefined, the way tests/test_host_san.py builds its driver: a HostIndex with a map survives
write_native -> read_native as format 2 (and the file still meets everything a format-1 reader checks, so that an
older library loads it); without a map the file is format 1 and byte for byte the documented format-1 layout; a
`rows` section that is truncated, holds an entry >= n or repeats one, or whose offset points
anywhere else, is rejected with an exception and no sanitizer report.  cph_host_rows_filter (the library's host-only
hook, no HIP call) is compared with numpy's `mask_input[rows]`."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from golden_util import fixture_path

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "row_map_san", "row_map_san.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("row_map_san")), "row_map_san_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(cmd, timeout=600):
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    return r.stdout


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g16", 1), ("g1024", 2), ("sift96", 4), ("g256", 4)])
def test_native_file_rows_section_under_asan_ubsan(asan_exe, tmp_path, name, bits):
    assert "files: ok" in _run([asan_exe, "files", fixture_path(name, bits), str(tmp_path)])


def test_rows_filter_host_under_asan_ubsan(asan_exe):
    assert "filter: ok" in _run([asan_exe, "filter"])


def _pack(mask):
    from cphnsw_mi355x.index import pack_allowed_bits
    return pack_allowed_bits(mask)


def _unpack(words, n):
    return np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 96, 100, 128, 1000, 4096, 100_003])
def test_host_rows_filter_matches_numpy(n):
    """cph_host_rows_filter against `mask_internal = mask_input[rows]`: n that is and is not a multiple of 32 and of
    64; all-zero, all-one, 50 % and 1 % masks."""
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    rng = np.random.default_rng(n)
    rows = rng.permutation(n).astype(np.uint32)
    masks = [np.zeros(n, bool), np.ones(n, bool), rng.random(n) < 0.5, rng.random(n) < 0.01]
    for mask_input in masks:
        w_in = _pack(mask_input)
        if n % 32:
            w_in[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)   # bits behind n must not leak into the result
        w_out = np.full((n + 31) // 32, 0xDEADBEEF, np.uint32)
        _lib.check(L.cph_host_rows_filter(w_in.ctypes.data, rows.ctypes.data, n, w_out.ctypes.data))
        mask_internal = mask_input[rows]
        assert np.array_equal(_unpack(w_out, n), mask_internal)
        assert np.array_equal(w_out, _pack(mask_internal))                # tail bits of the last word clear
        assert int(np.unpackbits(w_out.view(np.uint8)).sum()) == int(mask_input.sum())


def test_host_rows_filter_rejects_rows_out_of_range():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    rows = np.array([0, 1, 70, 3], np.uint32)
    w = np.zeros(1, np.uint32)
    with pytest.raises(ValueError, match="row out of range"):
        _lib.check(L.cph_host_rows_filter(w.ctypes.data, rows.ctypes.data, 4, w.ctypes.data))
    _lib.check(L.cph_host_rows_filter(None, None, 0, None))               # nothing to do
    assert C.c_int(L.cph_version()).value >= 102
