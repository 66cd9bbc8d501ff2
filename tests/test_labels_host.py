"""CPU tier of the label column (cph_set_labels, cph_filters_from_labels): the host statements of the device pass.

tests/labels_host/labels_host.cpp includes csrc/host_index.h and is built with plain g++ and
-fsanitize=address,undefined, the way tests/test_remove_host.py builds its driver (a stand-alone program; nothing loaded
into Python runs under a sanitizer).  `eval` runs label_filters_host and labels_to_internal_host on data written by this
test, on exact-size buffers, and the results are compared with numpy; `self` compares them with a bit-by-bit loop.
cph_host_label_filters (the library's host-only hook, no HIP call) is compared with numpy on the same cases."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "labels_host", "labels_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]

SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4100]
FILTER_COUNTS = [1, 3, 70]
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
SPECIAL = np.array([I32_MIN, -1, 0, 1, 5, I32_MAX], np.int32)


def _pack(mask):
    from cphnsw_mi355x.index import pack_allowed_bits
    return pack_allowed_bits(mask)


def _case(n, m):
    """labels from SPECIAL plus random values; m filters cycling through: equality, a range, lo > hi (empty), the full
    range (all ones), a value nobody has, a range overlapping the first one, a random pair."""
    rng = np.random.default_rng(1000 * n + m)
    labels = np.where(rng.random(n) < 0.7, SPECIAL[rng.integers(0, 6, n)], rng.integers(I32_MIN, I32_MAX, n, endpoint=True)).astype(np.int32)
    nobody = 123456789
    labels[labels == nobody] = 0
    lo, hi = np.empty(m, np.int32), np.empty(m, np.int32)
    for j in range(m):
        kind = j % 7
        if kind == 0:
            lo[j] = hi[j] = SPECIAL[(j // 7) % 6]
        elif kind == 1:
            lo[j], hi[j] = -1, 5
        elif kind == 2:
            lo[j], hi[j] = 5, -1
        elif kind == 3:
            lo[j], hi[j] = I32_MIN, I32_MAX
        elif kind == 4:
            lo[j] = hi[j] = nobody
        elif kind == 5:
            lo[j], hi[j] = 0, I32_MAX
        else:
            lo[j], hi[j] = rng.integers(I32_MIN, I32_MAX, 2, endpoint=True)
    return labels, lo, hi


def _expect(labels, lo, hi):
    n, m, nw = labels.size, lo.size, (labels.size + 31) // 32
    words = np.zeros((m, nw), np.uint32)
    counts = np.zeros(m, np.uint64)
    x = labels.astype(np.int64)
    for j in range(m):
        mask = (x >= int(lo[j])) & (x <= int(hi[j]))
        words[j] = _pack(mask)
        counts[j] = mask.sum()
        kind = j % 7
        if kind == 2 or kind == 4:
            assert counts[j] == 0
        if kind == 3:
            assert counts[j] == n
    return words, counts


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("labels_host")), "labels_host_asan")
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


def test_label_statements_against_a_loop_under_asan_ubsan(asan_exe):
    assert "self: ok" in _run([asan_exe, "self"])


@pytest.mark.parametrize("n", SIZES)
def test_label_statements_against_numpy_under_asan_ubsan(asan_exe, tmp_path, n):
    """label_filters_host (every m) and labels_to_internal_host against numpy: words, counts, labels[rows]."""
    for m in FILTER_COUNTS:
        labels, lo, hi = _case(n, m)
        rows = np.random.default_rng(n + 7).permutation(n).astype(np.uint32)
        fin, fout = str(tmp_path / f"in{m}.bin"), str(tmp_path / f"out{m}.bin")
        with open(fin, "wb") as f:
            f.write(np.array([n, m], np.uint64).tobytes() + labels.tobytes() + lo.tobytes() + hi.tobytes() + rows.tobytes())
        assert "eval: ok" in _run([asan_exe, "eval", fin, fout])
        raw = open(fout, "rb").read()
        nw = (n + 31) // 32
        assert len(raw) == m * nw * 4 + m * 8 + n * 4
        words = np.frombuffer(raw, np.uint32, m * nw).reshape(m, nw)
        counts = np.frombuffer(raw, np.uint64, m, m * nw * 4)
        internal = np.frombuffer(raw, np.int32, n, m * nw * 4 + m * 8)
        ew, ec = _expect(labels, lo, hi)
        assert np.array_equal(words, ew)                     # every word written, tail bits of the last word clear
        assert np.array_equal(counts, ec)
        assert np.array_equal(internal, labels[rows])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("m", FILTER_COUNTS)
def test_host_label_filters_hook_matches_numpy(n, m):
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    labels, lo, hi = _case(n, m)
    nw = (n + 31) // 32
    words = np.full((m, nw), 0xDEADBEEF, np.uint32)
    counts = np.full(m, 12345, np.uint64)
    _lib.check(L.cph_host_label_filters(labels.ctypes.data if n else None, n, lo.ctypes.data, hi.ctypes.data, m,
                                        words.ctypes.data if n else None, counts.ctypes.data))
    ew, ec = _expect(labels, lo, hi)
    assert np.array_equal(words, ew)
    assert np.array_equal(counts, ec)


def test_host_label_filters_hook_edges():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    _lib.check(L.cph_host_label_filters(None, 0, None, None, 0, None, None))           # m == 0: nothing to do
    one = np.zeros(1, np.int32)
    with pytest.raises(ValueError):
        _lib.check(L.cph_host_label_filters(None, 5, one.ctypes.data, one.ctypes.data, 1, None, None))
    assert L.cph_version() >= 105
