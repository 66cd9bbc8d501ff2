"""CPU tier of diversified search (search_diverse): the host statement of the MMR pass.

tests/diverse_model.py is the statement in numpy; its pair distance is a callable built from the oracle's free-array dot
(orc_dot), first tied, byte for byte, to OracleIndex.exact_l2 on a golden index file -- the distance bytes every search
reports.  cph_host_diverse_rows (csrc/host_diverse.h behind the library's host-only hook, no HIP call) is compared with the
model byte for byte in all three outputs on synthetic vectors and rows: the (C, k, D, lam) of diverse_model.cases(), each
with and without a row map.  tests/diverse_host/diverse_host.cpp includes csrc/host_diverse.h, is built with plain g++,
-fsanitize=address,undefined and -ffp-contract=off and runs the same cases as a child process on buffers of exactly the
stated sizes, the way tests/test_group_host.py runs its driver.  No sanitizer touches code loaded into Python."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from diverse_model import (CS, DS, FMAX, ID_X, ID_Y, ID_Z, KS, LAMS, N_DUP, N_IDS, N_RANDOM, ROW_KINDS, OraclePairs, cases,
                           diverse_model, diverse_model_batch, host_diverse_rows, read_v2_vectors, same_bytes, synth_batch,
                           synth_vectors)
from golden_util import DATASETS, fixture_path

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "diverse_host", "diverse_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]

_WANT = {}


def _case(case):
    """The batch of a case and what the model says, without and with the row map: computed once, shared by the tests."""
    if case not in _WANT:
        Cn, k, D, dim, lam = case
        raw, norm, pairs = synth_vectors(D, dim)
        ids, dist, rows, kinds = synth_batch(Cn, k, seed=1)
        want = diverse_model_batch(ids, dist, k, lam, pairs, N_IDS)
        want_rows = diverse_model_batch(ids, dist, k, lam, pairs, N_IDS, rows)
        for w in want + want_rows:
            w.setflags(write=False)
        _WANT[case] = (ids, dist, rows, kinds, raw, norm, pairs, want, want_rows)
    return _WANT[case]


def test_case_list_covers_what_it_promises():
    cs = cases()
    assert {c[0] for c in cs} == set(CS) and {c[2] for c in cs} == set(DS) and {c[4] for c in cs} == set(LAMS)
    for Cn in CS:
        assert {c[1] for c in cs if c[0] == Cn} == {k for k in KS + (Cn,) if k <= Cn}
        assert len({c[2] for c in cs if c[0] == Cn}) >= min(3, len([c for c in cs if c[0] == Cn]))
    assert any(c[3] < c[2] for c in cs)
    assert N_IDS % 2 == 1


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g16", 1)])
def test_pair_callable_has_the_bytes_of_exact_l2(oracle, name, bits):
    """(qn + n) - 2 dot from orc_dot on the rows of a golden index file == OracleIndex.exact_l2(row s, [j]), both ways round."""
    spec = DATASETS[name]
    path = fixture_path(name, bits)
    raw, norm = read_v2_vectors(path, spec["n"], spec["dim"], spec["D"])
    assert (raw[:, spec["dim"]:] == 0).all() and norm.min() > 0
    oi = oracle.load(path)
    pairs = OraclePairs(raw, norm)
    rng = np.random.default_rng(spec["seed"])
    for s in rng.integers(0, spec["n"], 12):
        js = rng.integers(0, spec["n"], 4)
        js[0] = s
        got = pairs(int(s), js)
        want = oi.exact_l2(raw[s, :spec["dim"]], js)
        assert got.tobytes() == want.tobytes(), (s, js)
        back = np.array([pairs(int(j), [s])[0] for j in js], np.float32)
        assert back.tobytes() == np.array([oi.exact_l2(raw[j, :spec["dim"]], [s])[0] for j in js], np.float32).tobytes()


def _check_batch_promises(case, ids, dist, kinds, raw, pairs, want):
    """The batch holds what the case list promises (so that a generator that quietly stopped producing a case fails here)."""
    Cn, k, D, dim, lam = case
    w_ids, w_dist, w_gap = want
    at = {kind: kinds.index(kind) for kind in ROW_KINDS}
    valid = ((ids >= 0) & (ids < N_IDS)).sum(axis=1)
    assert valid[at["all_padding"]] == 0 and (w_ids[at["all_padding"]] == -1).all()
    assert (w_dist[at["all_padding"]] == FMAX).all() and (w_gap[at["all_padding"]] == FMAX).all()
    r = at["partly_padding"]
    assert 0 < valid[r] and (k == 1 or valid[r] < k) and (Cn < 3 or (ids[r] >= N_IDS).any())
    assert (w_ids[r, :valid[r]] >= 0).all() and (w_ids[r, valid[r]:] == -1).all() and (w_gap[r, valid[r]:] == FMAX).all()
    if Cn >= 6:
        _, c = np.unique(ids[at["repeated_ids"]], return_counts=True)
        assert 2 in c and 3 in c
    r = at["dup_vectors"]
    if Cn >= 2:
        assert ids[r, 0] != ids[r, 1] and (raw[ids[r, 0]] == raw[ids[r, 1]]).all()
        assert pairs(int(ids[r, 0]), ids[r, 1:2])[0] == 0                    # m = 0 occurs at pick 1
        if k >= Cn:
            assert (w_gap[r] == 0).any()
    if Cn >= 63:
        d = dist[at["equal_relevance"]]
        zeros = d[d == 0]
        assert np.signbit(zeros).any() and not np.signbit(zeros).all()       # +0.0 and -0.0 side by side
        assert (np.diff(d) >= 0).all() and (np.diff(d) == 0).sum() > Cn // 2
    r = at["score_tie"]
    if Cn >= 3:
        px, py = int(np.flatnonzero(ids[r] == ID_X)[0]), int(np.flatnonzero(ids[r] == ID_Y)[0])
        assert ids[r, 0] == ID_Z and px < py and ID_X > ID_Y and dist[r, px] == dist[r, py]
        assert pairs(ID_Z, [ID_X]).tobytes() == pairs(ID_Z, [ID_Y]).tobytes()
        if lam < 1 and k >= 3:       # X and Y tie at pick 1, far ahead of the rest; the lower position wins, then Y
            assert w_ids[r, :3].tolist() == [ID_Z, ID_X, ID_Y], w_ids[r, :3]
            assert w_gap[r, 1] == w_gap[r, 2] == np.float32(10000.0)
    # invariants: distinct picks, gap[0], padding behind the picks
    for q in range(ids.shape[0]):
        got = w_ids[q][w_ids[q] >= 0]
        assert len(set(got.tolist())) == len(got) == min(k, len(set(ids[q][(ids[q] >= 0) & (ids[q] < N_IDS)].tolist())))
        assert w_gap[q, 0] == FMAX
        assert (w_dist[q, len(got):] == FMAX).all() and (w_gap[q, 1:len(got)] < FMAX).all()
    if lam == 1:
        for q in range(ids.shape[0]):
            first = [int(i) for i in dict.fromkeys(ids[q].tolist()) if 0 <= i < N_IDS][:k]
            assert w_ids[q, :len(first)].tolist() == first
            assert w_dist[q, :len(first)].tobytes() == np.array(
                [dist[q, int(np.flatnonzero(ids[q] == i)[0])] for i in first], np.float32).tobytes()
    if lam == 0.5 and k >= 2 and Cn >= 3:
        r = at["dup_vectors"]
        assert w_ids[r, 1] != ids[r, 1], "pick 1 is row entry 1: the row does not show a reordering"


@pytest.mark.parametrize("case", cases(), ids=lambda c: "C%d-k%d-D%d-dim%d-lam%g" % c)
def test_host_diverse_rows_matches_the_model(case):
    Cn, k, D, dim, lam = case
    ids, dist, rows, kinds, raw, norm, pairs, want, want_rows = _case(case)
    assert ids.shape == (len(ROW_KINDS), Cn) and raw.shape == (N_IDS, D) and sorted(rows.tolist()) == list(range(N_IDS))
    assert (raw[:N_RANDOM, dim:] == 0).all() and (raw[:N_RANDOM, :dim] != 0).all()
    _check_batch_promises(case, ids, dist, kinds, raw, pairs, want)
    assert same_bytes(host_diverse_rows(ids, dist, raw, norm, k, lam), want)
    assert same_bytes(host_diverse_rows(ids, dist, raw, norm, k, lam, rows), want_rows)
    # the row map only renames the picks
    assert want_rows[1].tobytes() == want[1].tobytes() and want_rows[2].tobytes() == want[2].tobytes()
    m = want[0] >= 0
    assert np.array_equal(want_rows[0][m], rows[want[0][m]]) and (want_rows[0][~m] == -1).all()


def test_model_on_a_row_worked_by_hand():
    """Four points on a line, exact arithmetic: 0, 1, 1 (a twin under another id) and 10."""
    raw = np.zeros((5, 8), np.float32)
    raw[:, 0] = [0, 1, 1, 10, 3]
    norm = (raw ** 2).sum(axis=1)
    pairs = OraclePairs(raw, norm)
    assert pairs(1, [0, 2, 3]).tolist() == [1.0, 0.0, 81.0]
    ids = np.array([1, 2, 1, -1, 0, 3, 9], np.int64)            # 1 twice; padding; 9 is beyond the five vectors
    dist = np.array([0.0, 0.0, 0.0, FMAX, 1.0, 81.0, 90.0], np.float32)
    # lam = 0.5: pick 0 = id 1.  Pick 1: scores 2: 0 - 0 = 0; 0: 0.5 - 0.5 = 0; 3: 40.5 - 40.5 = 0 -> a three-way tie: id 2
    # (lowest position).  Pick 2: m unchanged (2 is 1's twin): again a tie, id 0.  Pick 3: id 3, m = min(81, 81, 100).
    w = diverse_model(ids, dist, 5, 0.5, pairs, 5)
    assert w[0].tolist() == [1, 2, 0, 3, -1]
    assert w[1].tobytes() == np.array([0.0, 0.0, 1.0, 81.0, FMAX], np.float32).tobytes()
    assert w[2].tobytes() == np.array([FMAX, 0.0, 1.0, 81.0, FMAX], np.float32).tobytes()
    # lam = 0: the farthest point first
    assert diverse_model(ids, dist, 3, 0.0, pairs, 5)[0].tolist() == [1, 3, 0]
    # lam = 1: the row, repeats skipped
    assert diverse_model(ids, dist, 4, 1.0, pairs, 5)[0].tolist() == [1, 2, 0, 3]
    for k, lam in ((5, 0.5), (3, 0.0), (4, 1.0), (1, 0.3)):
        got = host_diverse_rows(ids[None], dist[None], raw, norm, k, lam)
        assert same_bytes(got, diverse_model_batch(ids[None], dist[None], k, lam, pairs, 5))


def test_host_diverse_rows_refuses_bad_arguments():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    raw, norm, _ = synth_vectors(16)
    ids, dist, rows, _ = synth_batch(65, 3, seed=3)
    n = ids.shape[0]
    o = (np.full((n, 65), -7, np.int64), np.full((n, 65), -7, np.float32), np.full((n, 65), -7, np.float32))
    po = [x.ctypes.data for x in o]

    def call(i=ids, d=dist, nn=n, Cn=65, rw=raw, nm=norm, ni=N_IDS, D=16, k=3, lam=0.5, out=po):
        p = [None if x is None else x.ctypes.data for x in (i, d, rw, nm)]
        return L.cph_host_diverse_rows(p[0], p[1], nn, Cn, p[2], p[3], ni, D, None, k, lam, *out)
    assert call() == _lib.OK
    for bad in (dict(i=None), dict(d=None), dict(rw=None), dict(nm=None), dict(k=0), dict(k=66), dict(Cn=0), dict(nn=0), dict(ni=0),
                dict(D=0), dict(D=12), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")),
                dict(out=[None] + po[1:]), dict(out=po[:2] + [None])):
        before = [x.copy() for x in o]
        assert call(**bad) == _lib.INVALID_ARGUMENT, bad
        assert L.cph_last_error()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(o, before))      # nothing written
    big = np.zeros((1, 1025), np.int64)
    assert call(i=big, d=np.zeros((1, 1025), np.float32), nn=1, Cn=1025, k=1) == _lib.INVALID_ARGUMENT
    assert b"1024" in L.cph_last_error()
    # the other new entry points answer before they touch a device
    assert L.cph_search_diverse(None, None, 0, 1, 0.5, 64, None, 0, None, 0, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_search_diverse_device(None, None, 0, 1, 0.5, 64, None, 0, None, 0, None, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_search_diverse(None, None, 0, 1, 0.5, 64, None, 0, None, 0, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_diverse_rows_hook(None, None, None, 1, 64, 1, 0.5, None, None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_debug_time_diverse(None, 1) == _lib.INVALID_ARGUMENT
    assert L.cph_debug_last_diverse_rows_us(None, None) == _lib.INVALID_ARGUMENT


def test_new_symbols_are_declared_with_the_issue_s_signatures():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    call = ("uint64_t n, uint64_t k, float lam, uint64_t candidates, const cph_filter* const* filters, uint32_t n_filters, "
            "const int32_t* filter_of, int exact, ")
    for decl in ("int cph_search_diverse(cph_index* h, const float* queries, " + call + "int64_t* ids, float* dist, float* gap);",
                 "int cph_search_diverse_device(cph_index* h, const float* d_queries, " + call +
                 "int64_t* d_ids, float* d_dist, float* d_gap, void* stream);",
                 "int cph_multi_search_diverse(cph_multi* m, const float* queries, " + call + "int64_t* ids, float* dist, float* gap);",
                 "int cph_diverse_rows_hook(cph_index* h, const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, "
                 "uint64_t k, float lam, int64_t* out_ids, float* out_dist, float* out_gap);",
                 "int cph_host_diverse_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const float* raw, "
                 "const float* norm_sq, uint64_t n_ids, uint64_t D, const uint32_t* rows, uint64_t k, float lam, int64_t* out_ids, "
                 "float* out_dist, float* out_gap);",
                 "int cph_debug_time_diverse(cph_index* h, int on);", "int cph_debug_last_diverse_rows_us(cph_index* h, double* us);"):
        assert decl in flat, decl
    p, u64, f32 = C.c_void_p, C.c_uint64, C.c_float
    diverse = [p, p, u64, u64, f32, u64, p, C.c_uint32, p, C.c_int, p, p, p]
    want = {"cph_search_diverse": diverse, "cph_search_diverse_device": diverse + [p], "cph_multi_search_diverse": diverse,
            "cph_diverse_rows_hook": [p, p, p, u64, u64, u64, f32, p, p, p],
            "cph_host_diverse_rows": [p, p, u64, u64, p, p, u64, u64, p, u64, f32, p, p, p],
            "cph_debug_time_diverse": [p, C.c_int], "cph_debug_last_diverse_rows_us": [p, C.POINTER(C.c_double)]}
    for name, args in want.items():
        assert hasattr(L, name) and _lib.SYMBOLS[name] == (C.c_int, args), name
    assert L.cph_version() >= 109


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("diverse_host")), "diverse_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_diverse_rows_host_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases as above, through the stand-alone program: exact-size buffers, every output byte compared there."""
    path = os.path.join(str(tmp_path), "cases.bin")
    n_cases = 0
    with open(path, "wb") as f:
        f.write(np.uint64(0).tobytes())
        for case in cases():
            Cn, k, D, dim, lam = case
            ids, dist, rows, kinds, raw, norm, pairs, want, want_rows = _case(case)
            for rm, w in ((None, want), (rows, want_rows)):
                f.write(np.array([ids.shape[0], Cn, k, N_IDS, D, int(rm is not None)], np.uint64).tobytes())
                f.write(np.float32(lam).tobytes())
                for a in (ids, dist, raw, norm) + (() if rm is None else (rm,)) + w:
                    f.write(np.ascontiguousarray(a).tobytes())
                n_cases += 1
        f.seek(0)
        f.write(np.uint64(n_cases).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"diverse: ok ({n_cases} cases)" in r.stdout and n_cases == 2 * len(cases())
