"""CPU tier of the inner-product metric: the host statement of its arithmetic.

tests/ip_model.py is the statement in numpy.  cph_host_ip_augment / cph_host_ip_epilogue (csrc/host_ip.h behind the
library's host-only hooks, no HIP call) are compared with the model byte for byte: dims on both sides of the 64-lane
stride and in the multi-pass loop, 1, 3 and 130 rows, per-row scales 2^-10 .. 2^10; the extra coordinate of the longest
row; the caller's bound at the exact maximum and one ulp below it; bad and over-bound rows at the first, a middle and the
last row; zero rows; queries and their c; the epilogue on padded, sorted rows.  tests/ip_host/ip_host.cpp includes
csrc/host_ip.h and csrc/native_file.h, is built with plain g++, -fsanitize=address,undefined and -ffp-contract=off and
runs the same cases as a child process on buffers of exactly the stated sizes, and pins the version check that makes a
format-4 reader refuse the format-5 metric record.  No sanitizer touches code loaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ip_model import (BAD_KINDS, DIMS, NO_ROW, NS, bad_cases, bad_row, case_rows, cases, epilogue_case, epilogue_model, max_model,
                      queries_model, rows_model, sq_norm_model)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "ip_host", "ip_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]
A5 = np.frombuffer(b"\xa5" * 4, np.float32)[0]
FLT_MAX = np.finfo(np.float32).max


def host_augment(x, mode, m2=0.0):
    """mode 0: rows against m2, 1: rows, bound from the data, 2: queries -> (out, c, m2 used, (bad, over, first))."""
    from cphnsw_mi355x import _lib
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    out = np.full((n, dim + 1), A5, np.float32)
    c = np.full(n, A5, np.float32)
    used = C.c_float(-1.0)
    cnt = (C.c_uint64 * 3)(77, 77, 77)
    _lib.check(_lib.lib().cph_host_ip_augment(x.ctypes.data, n, dim, mode, float(m2), out.ctypes.data,
                                              c.ctypes.data if mode == 2 else None, C.byref(used), cnt))
    return out, c, np.float32(used.value), (int(cnt[0]), int(cnt[1]), int(cnt[2]))


def host_epilogue(ids, dist, c):
    from cphnsw_mi355x import _lib
    ids = np.ascontiguousarray(ids, np.int64)
    d = np.ascontiguousarray(dist, np.float32).copy()
    c = np.ascontiguousarray(c, np.float32)
    _lib.check(_lib.lib().cph_host_ip_epilogue(ids.ctypes.data, d.ctypes.data, ids.shape[0], ids.shape[1], c.ctypes.data))
    return d


def test_case_list_covers_what_the_issue_names():
    assert set(DIMS) == {8, 63, 64, 65, 127, 128, 130, 960} and set(NS) == {1, 3, 130}
    assert len(cases()) == len(DIMS) * len(NS) and set(BAD_KINDS) == {"nan", "inf", "overflow"}
    x = case_rows(130, 64)
    norms = np.linalg.norm(x.astype(np.float64), axis=1)
    assert norms.max() / norms.min() > 2.0 ** 18            # scales from 2^-10 to 2^10 are really there
    kinds = {(k, p) for k, p, _, _ in bad_cases(65)}
    assert kinds == {(k, p) for k in BAD_KINDS + ("over",) for p in (0, 3, 6)}


@pytest.mark.parametrize("n,dim", cases())
def test_host_twin_has_the_model_s_bytes(n, dim):
    x = case_rows(n, dim)
    want, m2, cnt = rows_model(x)
    assert cnt == (0, 0, NO_ROW) and m2 == sq_norm_model(x).max()
    got, _, used, gcnt = host_augment(x, 1)
    assert used.tobytes() == m2.tobytes() and gcnt == cnt and got.tobytes() == want.tobytes()
    assert got[:, :dim].tobytes() == x.tobytes()                          # the caller's coordinates, bit for bit
    # the longest row sits on the sphere: its extra coordinate is exactly +0
    top = int(np.argmax(sq_norm_model(x)))
    assert got[top, dim].tobytes() == np.float32(0.0).tobytes()
    assert (got[:, dim] >= 0).all() and np.isfinite(got).all()
    # the caller's bound: the exact maximum gives the same bytes, one ulp below refuses exactly the longest rows
    got2, _, used2, cnt2 = host_augment(x, 0, m2)
    assert got2.tobytes() == want.tobytes() and cnt2 == cnt and used2 == m2
    below = np.nextafter(m2, np.float32(0.0))
    want3, _, cnt3 = rows_model(x, below)
    got3, _, _, gcnt3 = host_augment(x, 0, below)
    assert cnt3[0] == 0 and cnt3[1] >= 1 and cnt3[2] <= top and gcnt3 == cnt3 and got3.tobytes() == want3.tobytes()
    assert got3[top].tobytes() == np.zeros(dim + 1, np.float32).tobytes()
    # a generous bound: every row good, every extra coordinate positive
    big = np.float32(4.0) * m2
    got4, _, _, cnt4 = host_augment(x, 0, big)
    assert cnt4 == (0, 0, NO_ROW) and got4.tobytes() == rows_model(x, big)[0].tobytes() and (got4[:, dim] > 0).all()


@pytest.mark.parametrize("n,dim", cases())
def test_stored_rows_turn_squared_l2_into_the_inner_product(n, dim):
    """|q~ - x~|^2 = |q|^2 + M2 - 2 q.x on the stored rows, in float64, up to the rounding of the extra coordinate."""
    x = case_rows(n, dim)
    q = case_rows(3, dim, seed=5)
    rows, _, m2, _ = host_augment(x, 1)
    qa, c, _, qcnt = host_augment(q, 2, m2)
    assert qcnt == (0, 0, NO_ROW)
    r64, q64 = rows.astype(np.float64), qa.astype(np.float64)
    d = ((q64[:, None, :] - r64[None, :, :]) ** 2).sum(axis=2)
    want = -(q.astype(np.float64) @ x.astype(np.float64).T)
    scale = float(m2) + (q.astype(np.float64) ** 2).sum(axis=1)
    err = np.abs(0.5 * (d - c.astype(np.float64)[:, None]) - want) / scale[:, None]
    assert err.max() <= (dim + 8) * 2.0 ** -24, err.max()


@pytest.mark.parametrize("dim", (8, 64, 65, 130))
def test_bad_and_over_bound_rows_are_zeroed_counted_and_leave_their_neighbours_alone(dim):
    for kind, pos, x, m2 in bad_cases(dim):
        want, wm2, wcnt = rows_model(x, m2)
        assert wcnt == ((0, 1, pos) if kind == "over" else (1, 0, pos)), (kind, pos)
        got, _, used, cnt = host_augment(x, 1 if m2 is None else 0, 0.0 if m2 is None else m2)
        assert cnt == wcnt and used.tobytes() == wm2.tobytes(), (kind, pos)
        assert got.tobytes() == want.tobytes(), (kind, pos)
        assert got[pos].tobytes() == np.zeros(dim + 1, np.float32).tobytes()             # +0.0, every slot
        others = np.arange(len(x)) != pos
        assert got[others].tobytes() == rows_model(x[others], wm2)[0].tobytes()          # the neighbours are untouched
    # several: all counted, kinds apart, the lowest reported
    x = case_rows(9, dim)
    keep = [0, 1, 3, 4, 6, 7]
    m2 = max_model(x[keep])
    x[5] = x[keep][int(np.argmax(sq_norm_model(x[keep])))] * np.float32(2)
    x[2] = np.nan
    x[8, 0] = np.inf
    assert rows_model(x, m2)[2] == (2, 1, 2)
    assert host_augment(x, 0, m2)[3] == (2, 1, 2)


def test_a_zero_row_is_a_good_row():
    x = case_rows(5, 65)
    x[2] = 0.0
    x[2, ::2] = -0.0
    got, _, m2, cnt = host_augment(x, 1)
    assert cnt == (0, 0, NO_ROW) and got.tobytes() == rows_model(x)[0].tobytes()
    assert got[2, :65].tobytes() == x[2].tobytes() and got[2, 65] == np.sqrt(m2)
    z = np.zeros((3, 8), np.float32)                      # nothing but zero rows: M2 = 0, every extra coordinate +0
    got, _, m2, cnt = host_augment(z, 1)
    assert cnt == (0, 0, NO_ROW) and m2 == 0 and got.tobytes() == np.zeros((3, 9), np.float32).tobytes()


@pytest.mark.parametrize("n,dim", cases())
def test_queries_and_their_c(n, dim):
    q = case_rows(n, dim, seed=3)
    m2 = np.float32(37.5)
    want, wc, wcnt = queries_model(q, m2)
    got, c, _, cnt = host_augment(q, 2, m2)
    assert got.tobytes() == want.tobytes() and c.tobytes() == wc.tobytes() and cnt == wcnt == (0, 0, NO_ROW)
    assert got[:, :dim].tobytes() == q.tobytes() and got[:, dim].tobytes() == np.zeros(n, np.float32).tobytes()
    # a query is never over the bound; a bad one is the zero vector with c = M2
    for kind in BAD_KINDS:
        q2 = q.copy()
        q2[n // 2] = bad_row(kind, dim, np.random.default_rng(dim))
        want, wc, wcnt = queries_model(q2, m2)
        got, c, _, cnt = host_augment(q2, 2, m2)
        assert got.tobytes() == want.tobytes() and c.tobytes() == wc.tobytes() and cnt == wcnt == (1, 0, n // 2)
        assert got[n // 2].tobytes() == np.zeros(dim + 1, np.float32).tobytes() and c[n // 2] == m2


@pytest.mark.parametrize("n,k", [(1, 1), (3, 10), (130, 7), (64, 100)])
def test_epilogue_keeps_padding_and_order(n, k):
    ids, dist, c = epilogue_case(n, k)
    want = epilogue_model(ids, dist, c)
    got = host_epilogue(ids, dist, c)
    assert got.tobytes() == want.tobytes()
    pad = ids < 0
    assert pad.any() or n == 1
    assert got[pad].tobytes() == dist[pad].tobytes() and (got[pad] == FLT_MAX).all()         # padding keeps its bytes
    for i in range(n):                                                                       # sorted rows stay ascending
        live = got[i][~pad[i]]
        assert (np.diff(live) >= 0).all()
    # ties stay ties, and neighbours one ulp apart never swap
    d2 = np.repeat(np.float32(3.0), k)[None, :].copy()
    d2[0, k // 2:] = np.nextafter(np.float32(3.0), np.float32(4.0))
    g2 = host_epilogue(np.zeros((1, k), np.int64), d2, np.array([1.0 / 3], np.float32))
    assert (np.diff(g2[0]) >= 0).all() and len(set(g2[0][:k // 2].tolist())) <= 1


def test_host_hooks_validate_their_arguments():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    x = np.ones((2, 8), np.float32)
    o = np.zeros((2, 9), np.float32)
    c = np.zeros(2, np.float32)
    assert L.cph_host_ip_augment(None, 2, 8, 0, 1.0, o.ctypes.data, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_host_ip_augment(x.ctypes.data, 2, 8, 0, 1.0, None, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_host_ip_augment(x.ctypes.data, 2, 0, 0, 1.0, o.ctypes.data, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_host_ip_augment(x.ctypes.data, 2, 8, 3, 1.0, o.ctypes.data, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_host_ip_augment(x.ctypes.data, 2, 8, 2, 1.0, o.ctypes.data, None, None, None) == _lib.INVALID_ARGUMENT      # queries need c
    assert L.cph_host_ip_augment(x.ctypes.data, 2, 8, 0, float("nan"), o.ctypes.data, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_host_ip_augment(x.ctypes.data, 2, 8, 0, -1.0, o.ctypes.data, None, None, None) == _lib.INVALID_ARGUMENT
    assert (o == 0).all()
    assert L.cph_host_ip_augment(x.ctypes.data, 2, 8, 0, 8.0, o.ctypes.data, None, None, None) == _lib.OK        # null counters are allowed
    assert o.tobytes() == rows_model(x, 8.0)[0].tobytes()
    assert L.cph_host_ip_epilogue(None, c.ctypes.data, 1, 2, c.ctypes.data) == _lib.INVALID_ARGUMENT
    # the other new entry points answer before they touch a device
    assert L.cph_set_metric_ip(None) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_set_metric_ip(None) == _lib.INVALID_ARGUMENT
    assert L.cph_set_ip_bound(None, 1.0) == _lib.INVALID_ARGUMENT
    assert L.cph_get_ip_bound(None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_set_ip_bound(None, 1.0) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_get_ip_bound(None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_ip_augment_hook(0, None, 1, 8, 0, 1.0, None, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_ip_epilogue_hook(0, None, None, 1, 1, None, 0) == _lib.INVALID_ARGUMENT


def test_new_symbols_are_declared_with_the_issue_s_signatures():
    from cphnsw_mi355x import _lib
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    for decl in ("enum { CPH_METRIC_IP = 2 };", "int cph_set_metric_ip(cph_index* h);", "int cph_multi_set_metric_ip(cph_multi* m);",
                 "int cph_set_ip_bound(cph_index* h, float max_sq_norm);",
                 "int cph_get_ip_bound(cph_index* h, float* m2);", "int cph_multi_set_ip_bound(cph_multi* m, float max_sq_norm);",
                 "int cph_multi_get_ip_bound(cph_multi* m, float* m2);"):
        assert decl in flat, decl
    assert _lib.METRIC_IP == 2
    assert _lib.lib().cph_version() >= 112


def test_python_arguments_are_checked_before_any_device_is_touched():
    import cphnsw_mi355x
    with pytest.raises(ValueError, match="partition"):
        cphnsw_mi355x.CPIndex(24, 4, devices=[0, 0], partition=True, metric="ip")
    with pytest.raises(ValueError, match="max_norm"):
        cphnsw_mi355x.CPIndex(24, 4, metric="l2", max_norm=3.0)
    with pytest.raises(ValueError, match="max_norm"):
        cphnsw_mi355x.CPIndex(24, 4, metric="ip", max_norm=-1.0)
    with pytest.raises(ValueError, match="max_norm"):
        cphnsw_mi355x.CPIndex(24, 4, metric="ip", max_norm=float("inf"))


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("ip_host")), "ip_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_ip_host_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases as above, through the stand-alone program: exact-size buffers, every output byte compared there;
    and the native file's metric record as a format-4 and a format-5 reader take it."""
    path = os.path.join(str(tmp_path), "cases.bin")
    blobs = []

    def rows_case(x, m2):
        want, wm2, cnt = rows_model(x, m2)
        blobs.append(np.array([1 if m2 is None else 0, x.shape[0], x.shape[1], *cnt], np.uint64).tobytes() +
                     np.float32(wm2).tobytes() + x.tobytes() + want.tobytes())

    for n, dim in cases():
        x = case_rows(n, dim)
        rows_case(x, None)
        rows_case(x, np.nextafter(max_model(x), np.float32(0.0)))
        q = case_rows(n, dim, seed=3)
        q[n // 2, 0] = np.nan if dim % 2 else q[n // 2, 0]
        want, wc, cnt = queries_model(q, np.float32(37.5))
        blobs.append(np.array([2, n, dim, *cnt], np.uint64).tobytes() + np.float32(37.5).tobytes() + q.tobytes() +
                     want.tobytes() + wc.tobytes())
    for dim in (8, 64, 65, 130):
        for _, _, x, m2 in bad_cases(dim):
            rows_case(x, m2)
    z = case_rows(5, 65)
    z[2] = 0.0
    rows_case(z, None)
    for n, k in [(1, 1), (3, 10), (130, 7), (64, 100)]:
        ids, dist, c = epilogue_case(n, k)
        blobs.append(np.array([3, n, k, 0, 0, 0], np.uint64).tobytes() + np.float32(0).tobytes() + ids.tobytes() +
                     dist.tobytes() + c.tobytes() + epilogue_model(ids, dist, c).tobytes())
    with open(path, "wb") as f:
        f.write(np.uint64(len(blobs)).tobytes())
        for b in blobs:
            f.write(b)
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"ip: ok ({len(blobs)} cases)" in r.stdout
