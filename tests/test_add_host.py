"""CPU tier of added rows (cph_add): the host statement of the tail fold and the capacity rule of the resident arrays.

tests/add_host/add_host.cpp includes csrc/host_tail.h and is built with plain g++ and -fsanitize=address,undefined, the
way tests/test_remove_host.py builds its driver: tail_fold_host on exact-size buffers against a stable sort of the
concatenated row, out of place and in place, and tail_capacity.  cph_host_tail_fold and cph_host_tail_capacity (the
library's host-only hooks, no HIP call) are compared with the numpy statement in tests/tail_model.py:
argsort(concatenate([G_i, T_i]), kind="stable")[:k]."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tail_model import FMAX, FOLD_KS, FOLD_N, FOLD_PS, fold_case, fold_model, keys_of, pool_capacity

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "add_host", "add_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("add_host")), "add_host_asan")
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


def test_tail_fold_host_under_asan_ubsan(asan_exe):
    assert "fold: ok (18 cases)" in _run([asan_exe, "fold"])


def test_tail_capacity_under_asan_ubsan(asan_exe):
    assert "capacity: ok" in _run([asan_exe, "capacity"])


def _host_fold(g_ids, g_dist, pools, counts, k, C_, in_place=False):
    from cphnsw_mi355x import _lib
    P, n, _ = pools.shape
    gi, gd = g_ids.copy(), g_dist.copy()
    oi, od = (gi, gd) if in_place else (np.full_like(gi, -7), np.full_like(gd, -7.0))
    _lib.check(_lib.lib().cph_host_tail_fold(gi.ctypes.data, gd.ctypes.data, n, k, pools.ctypes.data, counts.ctypes.data, P, C_,
                                             oi.ctypes.data, od.ctypes.data))
    return oi, od


@pytest.mark.parametrize("P", FOLD_PS)
@pytest.mark.parametrize("k", FOLD_KS)
def test_host_tail_fold_matches_numpy_stable_argsort(k, P):
    g_ids, g_dist, pools, counts, C_ = fold_case(k, P, seed=k * 7 + P)
    assert g_ids.shape == (FOLD_N, k) and C_ == pool_capacity(k) and int(counts.max()) <= k
    # the shapes the case promises: tail counts 0, 1, < k, == k and more than k over the lists; rows that are partly and
    # all padding; a duplicate id
    tot = counts.sum(axis=0)
    assert tot[0] == 1 and tot[3] == 0 and tot[2] == k and tot[5] == P * k and (k < 3 or 0 < tot[1] < k)
    assert (g_ids[2] == -1).all() and (g_dist[2] == FMAX).all() and (k < 2 or (g_ids[1] == -1).any())
    assert k < 2 or g_ids[3, 0] == g_ids[3, 1]
    want_i, want_d = fold_model(g_ids, g_dist, pools, counts, k)
    for in_place in (False, True):
        oi, od = _host_fold(g_ids, g_dist, pools, counts, k, C_, in_place)
        assert np.array_equal(oi, want_i), (k, P, in_place)
        assert od.tobytes() == want_d.tobytes(), (k, P, in_place)
    # padding sorts last and stays padding; an empty tail leaves the row as it was
    assert ((want_i >= 0) == (want_d != FMAX)).all()
    assert np.array_equal(want_i[3], g_ids[3]) and np.array_equal(want_i[6], g_ids[6])


def test_host_tail_fold_ties():
    """Equal float values between a graph entry and a tail entry: the graph's entry first (also +0.0 against -0.0, which
    are equal as floats and differ in their bits); equal distance bits inside the tail: by id, across the lists."""
    k, P, C_ = 6, 2, 128
    g_ids = np.array([[5, 9, 11, -1, -1, -1]], np.int64)
    g_dist = np.array([[-0.0, 1.0, 2.0, FMAX, FMAX, FMAX]], np.float32)
    pools = np.full((P, 1, C_), 0xFFFFFFFFFFFFFFFF, np.uint64)
    pools[0, 0, :2] = keys_of(np.array([0.0, 1.0], np.float32), np.array([1002, 1007]))
    pools[1, 0, :3] = keys_of(np.array([1.0, 1.0, 2.0], np.float32), np.array([1001, 1009, 1000]))
    counts = np.array([[2], [3]], np.uint32)
    oi, od = _host_fold(g_ids, g_dist, pools, counts, k, C_)
    assert oi.tolist() == [[5, 1002, 9, 1001, 1007, 1009]]
    assert od.tobytes() == np.array([[-0.0, 0.0, 1.0, 1.0, 1.0, 1.0]], np.float32).tobytes()
    wi, wd = fold_model(g_ids, g_dist, pools, counts, k)
    assert np.array_equal(oi, wi) and od.tobytes() == wd.tobytes()


def test_host_tail_fold_refuses_bad_shapes():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    g_ids, g_dist, pools, counts, C_ = fold_case(10, 2, seed=1)
    oi, od = np.empty_like(g_ids), np.empty_like(g_dist)
    args = lambda k, P, Cc, cnt: (g_ids.ctypes.data, g_dist.ctypes.data, FOLD_N, k, pools.ctypes.data, cnt.ctypes.data, P, Cc,
                                  oi.ctypes.data, od.ctypes.data)
    assert L.cph_host_tail_fold(*args(10, 2, C_, counts)) == _lib.OK
    for bad in (args(1025, 2, 4096, counts), args(10, 0, C_, counts), args(10, 257, C_, counts), args(10, 2, 96, counts),
                args(10, 2, 16, counts), args(0, 2, C_, counts), args(10, 2, C_, counts + np.uint32(11))):
        assert L.cph_host_tail_fold(*bad) == _lib.INVALID_ARGUMENT
    assert L.cph_host_tail_fold(None, g_dist.ctypes.data, FOLD_N, 10, pools.ctypes.data, counts.ctypes.data, 2, C_, oi.ctypes.data,
                                od.ctypes.data) == _lib.INVALID_ARGUMENT


def test_host_tail_capacity_rule():
    from cphnsw_mi355x import _lib
    L = _lib.lib()

    def cap(c, need):
        out = C.c_uint64(0)
        _lib.check(L.cph_host_tail_capacity(c, need, C.byref(out)))
        return out.value
    assert cap(300, 300) == 300 and cap(300, 0) == 300                  # while the rows fit: no change
    assert cap(300, 301) == 1324                                          # 1,024 rows at least
    assert cap(1_000_000, 1_000_001) == 1_500_000                         # half as much again
    assert cap(1_000_000, 5_000_000) == 5_000_000                         # never below the need
    assert cap(4_000_000_000, 4_000_000_001) == 0xFFFFFFFF                # never beyond the id space
    c, growths = 300, 0
    for size in range(300, 300 + 3000):                                   # single-row adds: amortised
        if size + 1 > c:
            c, growths = cap(c, size + 1), growths + 1
    assert growths == 3 and c >= 3300


def test_new_symbols_are_declared_with_the_issue_s_signatures():
    """cph_add / cph_tail_count / the fold hooks exist in the library, the header and the ctypes table; ABI minor 6."""
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    txt = open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", txt)
    fold = ("const int64_t* g_ids, const float* g_dist, uint64_t n, uint64_t k, const uint64_t* pools, const uint32_t* counts, "
            "uint32_t P, uint32_t C, int64_t* out_ids, float* out_dist);")
    for decl in ("int cph_add(cph_index* h, const float* vectors, uint64_t m, const int32_t* labels, int64_t* first_id);",
                 "int cph_tail_count(cph_index* h, uint64_t* t);",
                 "int cph_tail_fold_hook(int device, " + fold,
                 "int cph_host_tail_fold(" + fold):
        assert decl in flat, decl
    for name in ("cph_add", "cph_tail_count", "cph_tail_fold_hook", "cph_host_tail_fold", "cph_host_tail_capacity"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    assert _lib.SYMBOLS["cph_add"][1] == [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int64)]
    assert L.cph_version() >= 106
    # without a handle nothing is touched: the argument check answers
    assert L.cph_add(None, None, 0, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_tail_count(None, None) == _lib.INVALID_ARGUMENT
