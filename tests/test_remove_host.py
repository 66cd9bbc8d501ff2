"""CPU tier of removed rows (cph_remove): the host statement of the effective filter F & ~R and the native file's
`removed` section.

tests/remove_host/remove_host.cpp includes csrc/host_index.h and csrc/native_file.h and is built with plain g++ and
-fsanitize=address,undefined, the way tests/test_row_map_host.py builds its driver: a HostIndex with removed rows
survives write_native -> read_native as format 3, with and without a row map; without removed rows the file is byte
for byte the format-1 / format-2 file; what a reader of formats 1 and 2 finds behind the upper layers of a format-3
file is something it refuses; a `removed` section that is truncated, whose stored count is wrong, that holds a bit at
an id >= n or whose offset points anywhere else is rejected with the reader's usual errors and no sanitizer report.
cph_host_live_filter (the library's host-only hook, no HIP call) is compared with numpy."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from golden_util import fixture_path

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "remove_host", "remove_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("remove_host")), "remove_host_asan")
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


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g16", 1), ("g1024", 2)])
def test_native_file_removed_section_under_asan_ubsan(asan_exe, tmp_path, name, bits):
    assert "files: ok" in _run([asan_exe, "files", fixture_path(name, bits), str(tmp_path)])


def test_native_writer_against_files_of_the_older_library(asan_exe, tmp_path):
    """Independent of this tree's writer and reader: tests/golden/remove_g16_b1_parent_native_f2.cphn.gz was written by
    write_native of the commit before removed rows existed (g16 1-bit fixture, row map (7 i + 3) mod n) -- an index
    without removed rows must still be written as exactly those bytes; remove_g16_b1_native_f3_{plain,rows}.cphn.gz are
    format-3 files (R = every fifth id and the last) that read_native of that commit was run on and refused ("Corrupt
    index: unknown data behind the upper layers") -- this writer must still produce exactly those bytes.  (The format-1
    bytes of an index without a map are pinned by the layout statement in tests/row_map_san.)"""
    import gzip
    gold = tmp_path / "gold"
    gold.mkdir()
    for name in ("parent_native_f2", "native_f3_plain", "native_f3_rows"):
        with gzip.open(os.path.join(HERE, "golden", f"remove_g16_b1_{name}.cphn.gz"), "rb") as f:
            (gold / f"{name}.cphn").write_bytes(f.read())
    out = tmp_path / "out"
    out.mkdir()
    assert "golden: ok" in _run([asan_exe, "golden", fixture_path("g16", 1), str(gold), str(out)])


def test_live_filter_host_under_asan_ubsan(asan_exe):
    assert "filter: ok" in _run([asan_exe, "filter"])


def _pack(mask):
    from cphnsw_mi355x.index import pack_allowed_bits
    return pack_allowed_bits(mask)


def _tail(n):
    return np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 300, 8193])
@pytest.mark.parametrize("with_f", [False, True])
def test_host_live_filter_matches_numpy(n, with_f):
    """cph_host_live_filter against `F & ~R`: n that is and is not a multiple of 32, F null and not, tail bits of the
    last word set in both inputs (ignored, and clear in the output), the count."""
    from cphnsw_mi355x import _lib
    import ctypes as C
    L = _lib.lib()
    rng = np.random.default_rng(n * 2 + with_f)
    for F, R in [(np.ones(n, bool), np.zeros(n, bool)), (rng.random(n) < 0.5, rng.random(n) < 0.5),
                 (rng.random(n) < 0.9, rng.random(n) < 0.1), (rng.random(n) < 0.5, np.ones(n, bool))]:
        wf, wr = _pack(F), _pack(R)
        if n % 32:
            wf[-1] |= _tail(n)
            wr[-1] |= _tail(n)
        out = np.full((n + 31) // 32, 0xDEADBEEF, np.uint32)
        cnt = C.c_uint64(12345)
        _lib.check(L.cph_host_live_filter(wf.ctypes.data if with_f else None, wr.ctypes.data, n, out.ctypes.data, C.byref(cnt)))
        want = (F if with_f else np.ones(n, bool)) & ~R
        assert np.array_equal(out, _pack(want))            # tail bits of the last word clear
        assert cnt.value == int(want.sum())
    _lib.check(L.cph_host_live_filter(None, None, 0, None, None))          # nothing to do
    assert L.cph_version() >= 104
