"""CPU tier of two-stage search (make_rescore_vectors, search_rescored): the host statement of rows-in and of the rescoring pass.

tests/rescore_model.py is the statement in numpy.  cph_host_rescore_rows_in and cph_host_rescore_rows (csrc/host_rescore.h
behind the library's host-only hooks, no HIP call) are compared with it byte for byte: the (C, k, dim_full, dtype, metric) of
rescore_model.cases() on the candidate-row kinds of diverse_model.synth_row plus a row whose candidates outnumber k by one,
each with and without a row map.  The model itself is held against float64 with the standard bound for dim_full + 2
roundings, and the float16 rounding against numpy.astype(float16).  tests/rescore_host/rescore_host.cpp includes
csrc/host_rescore.h, is built with plain g++, -fsanitize=address,undefined and -ffp-contract=off and runs the same cases as a
child process on buffers of exactly the stated sizes.  No sanitizer touches code loaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from diverse_model import FMAX, N_DUP, N_IDS, N_RANDOM
from rescore_model import (CS, DIMS, DTYPES, KINDS, KS, METRICS, Layout, cases, host_rescore_rows, host_rows_in, model_scores, model_sum,
                           rescore_model_batch, rows_in_model, same_bytes, stored_values, synth_full, synth_queries, synth_rows)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "rescore_host", "rescore_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]

_OBJ, _WANT = {}, {}
_ROW_MAP = np.random.default_rng(99).permutation(N_IDS).astype(np.uint32)
IN_DIMS = DIMS[:-1] + (1032,)
N_IN, N_IN_MAP = 37, 30


def _object(dim, dtype):
    """The object over synth_full(dim) as the model stores it: (L, stored, norms, X).  Cached."""
    if (dim, dtype) not in _OBJ:
        stored, norms, bad = rows_in_model(synth_full(dim), dtype)
        assert bad.size == 0
        L = Layout(dim, dtype)
        for a in (stored, norms):
            a.setflags(write=False)
        _OBJ[(dim, dtype)] = (L, stored, norms, stored_values(stored, L))
    return _OBJ[(dim, dtype)]


def _case(case):
    """The batch of a case and what the model says, without and with the row map: computed once, shared by the tests."""
    if case not in _WANT:
        Cn, k, dim, dtype, metric = case
        L, stored, norms, X = _object(dim, dtype)
        ids, dist, kinds = synth_rows(Cn, k, seed=1)
        fq = synth_queries(ids.shape[0], dim, seed=Cn + k)
        want = rescore_model_batch(ids, dist, k, fq, X, norms, L, metric, N_IDS)
        want_rows = rescore_model_batch(ids, dist, k, fq, X, norms, L, metric, N_IDS, _ROW_MAP)
        for w in want + want_rows:
            w.setflags(write=False)
        _WANT[case] = (ids, dist, kinds, fq, want, want_rows)
    return _WANT[case]


def _rows_in_case(dim, dtype, with_map):
    rows = synth_full(dim)[:N_IN]
    rm = np.random.default_rng(dim).permutation(N_IN_MAP).astype(np.uint32) if with_map else None
    return rows, rm, rows_in_model(rows, dtype, rm)


def test_case_list_covers_what_it_promises():
    cs = cases()
    assert {c[0] for c in cs} == set(CS) and {c[2] for c in cs} == set(DIMS)
    for Cn in CS:
        assert {c[1] for c in cs if c[0] == Cn} == {k for k in KS + (Cn,) if k <= Cn}
    assert {(c[2], c[3], c[4]) for c in cs} == {(d, t, m) for d in DIMS for t in DTYPES for m in METRICS}
    # every G, a row below one piece, a row that is no whole number of pieces, more than one pass of the widest group
    assert {Layout(d, t).G for d in DIMS for t in DTYPES} == {1, 2, 4, 8, 16, 32, 64}
    assert Layout(1, "float16").pieces == 1 and Layout(7, "float32").padded == 8 and Layout(72, "float16").pieces == 9
    assert Layout(520, "float16").pieces == 65 and Layout(8192, "float32").pieces == 32 * 64
    assert Layout(64, "float16").stride == 128 and Layout(64, "float16").G == 8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", IN_DIMS)
def test_host_rows_in_matches_the_model(dim, dtype):
    for with_map in (False, True):
        rows, rm, (w_stored, w_norms, w_bad) = _rows_in_case(dim, dtype, with_map)
        stored, norms, bad, first = host_rows_in(rows, dtype, rm)
        assert w_bad.size == 0 and bad == 0 and first is None
        assert stored.tobytes() == w_stored.tobytes() and norms.tobytes() == w_norms.tobytes()
        L = Layout(dim, dtype)
        assert stored.shape == (N_IN, L.stride) and L.stride % 16 == 0
        assert (stored.view(L.np_dtype).reshape(N_IN, L.padded)[:, dim:] == 0).all()            # the padding is zeros
        if with_map:
            plain = rows_in_model(rows, dtype)[0]
            assert stored[:N_IN_MAP].tobytes() == plain[rm].tobytes() and stored[N_IN_MAP:].tobytes() == plain[N_IN_MAP:].tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_objects_match_the_model(dtype):
    for dim in (8, 72, 520):
        L, w_stored, w_norms, _ = _object(dim, dtype)
        stored, norms, bad, _ = host_rows_in(synth_full(dim), dtype)
        assert bad == 0 and stored.tobytes() == w_stored.tobytes() and norms.tobytes() == w_norms.tobytes()


def test_float16_rounding_is_numpy_s():
    """Ties to even, subnormals, the largest finite value and the first one that overflows; then 2^18 random bit patterns."""
    e = np.float64(2.0)
    special = np.array([1 + e ** -11, 1 + 3 * e ** -11, 1 + e ** -11 + e ** -20, 1 + e ** -11 - e ** -20, 2047.5, 2048.5, 2049.0,
                        e ** -24, e ** -25, e ** -25 * (1 + e ** -20), 3 * e ** -25, e ** -26, 5 * e ** -25, e ** -14, e ** -14 - e ** -25,
                        e ** -14 - e ** -26, 1023.5 * e ** -24, 65504.0, 65519.99, -65504.0, 0.0, -0.0, 1e-10, -1e-10, 0.1, -3.14159],
                       np.float32)
    rng = np.random.default_rng(5)
    rnd = rng.integers(0, 2 ** 32, 2 ** 18, dtype=np.uint64).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        rnd = np.where(np.abs(rnd) < 65520.0, rnd, np.float32(0.5))      # (NaN and everything that overflows: refused, below)
    vals = np.concatenate([special, rnd[:2 ** 18 - special.size]]).reshape(32, 8192)
    stored, norms, bad, _ = host_rows_in(vals, "float16")
    assert bad == 0
    got = stored.view(np.uint16)
    assert got.tobytes() == vals.astype(np.float16).view(np.uint16).tobytes()
    assert got[0, 0] == 0x3C00 and got[0, 1] == 0x3C02 and got[0, 2] == 0x3C01 and got[0, 3] == 0x3C00       # ties go to even
    assert got[0, 7] == 1 and got[0, 8] == 0 and got[0, 9] == 1 and got[0, 10] == 2 and got[0, 17] == 0x7BFF and got[0, 18] == 0x7BFF
    # float32 storage keeps the bits
    stored32, _, bad32, _ = host_rows_in(vals, "float32")
    assert bad32 == 0 and stored32.tobytes() == vals.tobytes()


def test_bad_rows_are_counted_with_the_lowest_row():
    rows = synth_full(24)[:20].copy()
    assert host_rows_in(rows, "float16")[2:] == (0, None)
    rows[11, 3] = np.float32(65520.0)                    # rounds to an infinity in float16
    rows[5, 23] = np.nan
    rows[17, 0] = -np.inf
    for dtype, want in (("float16", [5, 11, 17]), ("float32", [5, 17])):
        _, _, bad, first = host_rows_in(rows, dtype)
        assert (bad, first) == (len(want), want[0])
        assert rows_in_model(rows, dtype)[2].tolist() == want
    rows = synth_full(24)[:20].copy()
    rows[2, 1] = np.float32(70000.0)
    assert host_rows_in(rows, "float16")[2:] == (1, 2) and host_rows_in(rows, "float32")[2:] == (0, None)
    rows[2, 1] = np.float32(65504.0)
    assert host_rows_in(rows, "float16")[2:] == (0, None)
    rows[9, :] = np.float32(3e19)                        # finite values, an overflowing squared norm
    assert host_rows_in(rows, "float32")[2:] == (1, 9) and rows_in_model(rows, "float32")[2].tolist() == [9]
    # under a row map the row is still named in the caller's numbering
    rm = np.arange(20, dtype=np.uint32)[::-1].copy()
    assert host_rows_in(rows, "float32", rm)[2:] == (1, 9)


def _check_batch_promises(case, ids, dist, kinds, want):
    Cn, k, dim, dtype, metric = case
    w_ids, w_score, w_first = want
    at = {kind: kinds.index(kind) for kind in KINDS}
    valid = [len(set(i for i in ids[q].tolist() if 0 <= i < N_IDS)) for q in range(ids.shape[0])]
    r = at["all_padding"]
    assert valid[r] == 0 and (w_ids[r] == -1).all() and (w_score[r] == FMAX).all() and (w_first[r] == FMAX).all()
    r = at["partly_padding"]
    assert 0 < valid[r] and (k == 1 or valid[r] < k) and (Cn < 3 or (ids[r] >= N_IDS).any())
    if Cn >= 6:
        _, c = np.unique(ids[at["repeated_ids"]], return_counts=True)
        assert 2 in c and 3 in c
    r = at["dup_vectors"]
    if Cn >= 2:
        assert ids[r, 1] == ids[r, 0] + N_RANDOM and ids[r, 0] < N_DUP
        if k == Cn:                                       # both twins are returned: equal scores, the lower id first
            a, b = int(np.flatnonzero(w_ids[r] == ids[r, 0])[0]), int(np.flatnonzero(w_ids[r] == ids[r, 1])[0])
            assert b == a + 1 and w_score[r, a].tobytes() == w_score[r, b].tobytes()
    if Cn >= 63:
        d = dist[at["equal_relevance"]]
        assert np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
    r = at["one_more_than_k"]
    assert valid[r] == min(Cn, k + 1) and (w_ids[r] >= 0).all()
    for q in range(ids.shape[0]):
        got = w_ids[q][w_ids[q] >= 0]
        assert len(set(got.tolist())) == len(got) == min(k, valid[q])
        m = len(got)
        assert (w_ids[q, m:] == -1).all() and (w_score[q, m:] == FMAX).all() and (w_first[q, m:] == FMAX).all()
        s = w_score[q, :m]
        assert (np.diff(s) >= 0).all()
        ties = np.flatnonzero(np.diff(s) == 0)
        assert (got[ties] < got[ties + 1]).all()
        for t in range(m):                                # first = the bytes at the id's first position in the row
            j = int(np.flatnonzero(ids[q] == got[t])[0])
            assert w_first[q, t].tobytes() == dist[q, j].tobytes()
        if metric == "l2":
            assert (s >= 0).all() and not np.signbit(s).any()
        else:
            assert not ((s == 0) & ~np.signbit(s)).any()


@pytest.mark.parametrize("case", cases(), ids=lambda c: "C%d-k%d-dim%d-%s-%s" % c)
def test_host_rescore_rows_matches_the_model(case):
    Cn, k, dim, dtype, metric = case
    ids, dist, kinds, fq, want, want_rows = _case(case)
    L, stored, norms, X = _object(dim, dtype)
    assert ids.shape == (len(KINDS), Cn) and stored.shape == (N_IDS, L.stride)
    _check_batch_promises(case, ids, dist, kinds, want)
    assert same_bytes(host_rescore_rows(ids, dist, k, fq, stored, norms, dtype, metric), want)
    assert same_bytes(host_rescore_rows(ids, dist, k, fq, stored, norms, dtype, metric, _ROW_MAP), want_rows)
    # the row map only renames the answers
    assert want_rows[1].tobytes() == want[1].tobytes() and want_rows[2].tobytes() == want[2].tobytes()
    m = want[0] >= 0
    assert np.array_equal(want_rows[0][m], _ROW_MAP[want[0][m]]) and (want_rows[0][~m] == -1).all()


def test_a_query_without_a_finite_norm_gets_padding():
    L, stored, norms, X = _object(24, "float16")
    ids, dist, _ = synth_rows(65, 3, seed=2)
    fq = synth_queries(ids.shape[0], 24)
    fq[0, 5], fq[1, 0], fq[2, :] = np.nan, np.inf, np.float32(3e19)
    for metric in METRICS:
        want = rescore_model_batch(ids, dist, 3, fq, X, norms, L, metric, N_IDS)
        assert (want[0][:3] == -1).all() and (want[1][:3] == FMAX).all() and (want[0][3] >= 0).all()
        assert same_bytes(host_rescore_rows(ids, dist, 3, fq, stored, norms, "float16", metric), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", DIMS)
def test_model_is_within_the_rounding_bound_of_float64(dim, dtype):
    """|score - exact| <= (dim_full + 2) 2^-23 (qn + xn + 2 sum |q_j x_j|) for "l2", the same with sum |q_j x_j| alone for
    "ip": the standard bound for dim_full + 2 roundings, with a factor of two in hand."""
    L, stored, norms, X = _object(dim, dtype)
    fq = synth_queries(4, dim, seed=3)
    pick = np.r_[0:40, N_RANDOM:N_IDS]
    x64 = X[pick, :dim].astype(np.float64)
    for q in fq:
        q64 = q.astype(np.float64)
        dot, qn, xn, ab = x64 @ q64, q64 @ q64, (x64 * x64).sum(axis=1), np.abs(x64 * q64).sum(axis=1)
        for metric in METRICS:
            s = model_scores(q, X[pick], norms[pick], L, metric)[0].astype(np.float64)
            exact = -dot if metric == "ip" else np.maximum(0.0, qn + xn - 2 * dot)
            bound = (dim + 2) * 2.0 ** -23 * (ab if metric == "ip" else qn + xn + 2 * ab)
            assert (np.abs(s - exact) <= bound).all(), (metric, np.abs(s - exact).max())
    # and a sum worked by hand: 2 pieces of float32, G = 2: lane 0 = 1 + 2 + 3 + 4, lane 1 = 5 + 6 + 7
    L7 = Layout(7, "float32")
    assert (L7.G, L7.pieces, L7.padded) == (2, 2, 8)
    assert model_sum(np.arange(1, 9, dtype=np.float32) * (np.arange(8) < 7), np.ones(8, np.float32), L7)[0] == 28.0


def test_host_entries_refuse_bad_arguments():
    from cphnsw_mi355x import _lib
    Lb = _lib.lib()
    L, stored, norms, X = _object(24, "float16")
    ids, dist, _ = synth_rows(65, 3, seed=3)
    fq = synth_queries(ids.shape[0], 24)
    n = ids.shape[0]
    o = (np.full((n, 65), -7, np.int64), np.full((n, 65), -7, np.float32), np.full((n, 65), -7, np.float32))
    po = [x.ctypes.data for x in o]
    stored, norms = np.ascontiguousarray(stored), np.ascontiguousarray(norms)

    def call(i=ids, d=dist, nn=n, Cn=65, f=fq, dim=24, s=stored, nm=norms, ni=N_IDS, dt=0, mt=0, k=3, out=po):
        p = [None if x is None else x.ctypes.data for x in (i, d, f, s, nm)]
        return Lb.cph_host_rescore_rows(p[0], p[1], nn, Cn, p[2], dim, p[3], p[4], ni, dt, mt, None, k, *out)
    assert call() == _lib.OK
    for bad in (dict(i=None), dict(d=None), dict(f=None), dict(s=None), dict(nm=None), dict(k=0), dict(k=66), dict(Cn=0), dict(nn=0),
                dict(ni=0), dict(dim=0), dict(dim=8193), dict(dt=2), dict(mt=2), dict(out=[None] + po[1:]), dict(out=po[:2] + [None])):
        before = [x.copy() for x in o]
        assert call(**bad) == _lib.INVALID_ARGUMENT, bad
        assert Lb.cph_last_error()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o, before))      # nothing written
    big = np.zeros((1, 1025), np.int64)
    assert call(i=big, d=np.zeros((1, 1025), np.float32), nn=1, Cn=1025, k=1) == _lib.INVALID_ARGUMENT
    assert b"1024" in Lb.cph_last_error()
    # the other new entry points answer before they touch a device
    out = C.c_void_p()
    assert Lb.cph_rescore_vectors_create(None, None, 0, 8, 0, 0, 0, C.byref(out)) == _lib.INVALID_ARGUMENT and not out.value
    assert Lb.cph_rescore_vectors_create(None, None, 0, 8, 0, 0, 0, None) == _lib.INVALID_ARGUMENT
    assert Lb.cph_rescore_vectors_destroy(None) == _lib.OK
    assert Lb.cph_rescore_vectors_get(None, 0, 0, None, None) == _lib.INVALID_ARGUMENT
    assert Lb.cph_search_rescored(None, None, 0, None, 8, 1, 64, None, None, 0, None, 0, None, None, None) == _lib.INVALID_ARGUMENT
    assert Lb.cph_search_rescored_device(None, None, 0, None, 8, 1, 64, None, None, 0, None, 0, None, None, None, None) == _lib.INVALID_ARGUMENT
    assert Lb.cph_multi_search_rescored(None, None, 0, None, 8, 1, 64, None, None, 0, None, 0, None, None, None) == _lib.INVALID_ARGUMENT
    assert Lb.cph_rescore_rows_hook(None, None, None, 1, 64, None, None, 1, None, None, None) == _lib.INVALID_ARGUMENT
    assert Lb.cph_debug_time_rescored(None, 1) == _lib.INVALID_ARGUMENT
    assert Lb.cph_debug_last_rescored_us(None, None) == _lib.INVALID_ARGUMENT


def test_new_symbols_are_declared():
    from cphnsw_mi355x import _lib
    Lb = _lib.lib()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    call = ("uint64_t n, const float* full_queries, uint64_t dim_full, uint64_t k, uint64_t candidates, ")
    for decl in ("int cph_search_rescored(cph_index* h, const float* queries, " + call + "const cph_rescore_vectors* vectors, ",
                 "int cph_multi_search_rescored(cph_multi* m, const float* queries, " + call + "const cph_rescore_vectors* const* vectors, ",
                 "int cph_rescore_vectors_get(const cph_rescore_vectors* rv, uint64_t first, uint64_t count, void* rows_out, float* norms_out);",
                 "int cph_debug_time_rescored(cph_index* h, int on);", "int cph_debug_last_rescored_us(cph_index* h, double* us);"):
        assert decl in flat, decl
    for name in ("cph_rescore_vectors_create", "cph_rescore_vectors_destroy", "cph_rescore_vectors_info", "cph_rescore_vectors_get",
                 "cph_search_rescored", "cph_search_rescored_device", "cph_multi_search_rescored", "cph_debug_time_rescored",
                 "cph_debug_last_rescored_us", "cph_rescore_rows_hook", "cph_host_rescore_rows", "cph_host_rescore_rows_in"):
        assert hasattr(Lb, name) and name in _lib.SYMBOLS, name
    assert Lb.cph_version() >= 114


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("rescore_host")), "rescore_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_rescore_host_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases as above, through the stand-alone program: exact-size buffers, every output byte compared there."""
    path = os.path.join(str(tmp_path), "cases.bin")
    n_cases = 0
    u64 = lambda *v: np.array(v, np.uint64).tobytes()
    with open(path, "wb") as f:
        f.write(u64(0))
        for dim in IN_DIMS:
            for dtype in DTYPES:
                for with_map in (False, True):
                    rows, rm, (w_stored, w_norms, w_bad) = _rows_in_case(dim, dtype, with_map)
                    f.write(u64(0, rows.shape[0], dim, int(dtype == "float32"), int(with_map), N_IN_MAP if with_map else 0))
                    for a in (rows,) + ((rm,) if with_map else ()) + (w_stored, w_norms):
                        f.write(np.ascontiguousarray(a).tobytes())
                    f.write(u64(w_bad.size, 2 ** 64 - 1))
                    n_cases += 1
        bad_rows = synth_full(24)[:20].copy()
        bad_rows[7, 2], bad_rows[3, 0] = 70000.0, np.nan
        w_stored, w_norms, w_bad = rows_in_model(bad_rows, "float16")
        f.write(u64(0, 20, 24, 0, 0, 0) + bad_rows.tobytes() + w_stored.tobytes() + w_norms.tobytes() + u64(2, 3))
        n_cases += 1
        for case in cases():
            Cn, k, dim, dtype, metric = case
            ids, dist, kinds, fq, want, want_rows = _case(case)
            L, stored, norms, X = _object(dim, dtype)
            f.write(u64(1, ids.shape[0], Cn, k, N_IDS, dim, int(dtype == "float32"), int(metric == "ip")))
            for a in (ids, dist, fq, stored, norms, _ROW_MAP) + want + want_rows:
                f.write(np.ascontiguousarray(a).tobytes())
            n_cases += 1
        f.seek(0)
        f.write(u64(n_cases))
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"rescore: ok ({n_cases} cases)" in r.stdout and n_cases > 2 * len(IN_DIMS) * len(DTYPES)
