"""CPU tier of fused search (search_fused: several query vectors per query, exact weighted-sum top-k).

cph_host_fused_rows (csrc/host_fused.h behind the library's host-only hook, no HIP call) is compared, byte for byte in all
three outputs, with tests/fused_model.py over the oracle's eight-chain dot on the synthetic batch of that file: T = 1, 2, 5 and
64; unions of 0, 1, 63, 64 and 65 ids and T * C = 8192; k = 1, 3, 65 and 67 (U and U + 2 of the 65-id query); D = 16 and 128 with
dim < D; each case with and without a row map.  The pair distance of the model is tied to OracleIndex.exact_l2 on a golden
index file.  tests/fused_host/fused_host.cpp includes the header, is built with plain g++ and
-fsanitize=address,undefined -ffp-contract=off and runs the same cases as a child process on buffers of exactly the stated
sizes.  No sanitizer touches code loaded into Python."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from diverse_model import read_v2_vectors
from fused_model import (BIG, FMAX, _orderable, KINDS, TWIN_HI, TWIN_LO, U_SIZES, OracleQueryDists, check_batch_promises, fused_model,
                         fused_model_batch, host_fused_rows, same_bytes, synth_batch, synth_index, union_sizes)
from golden_util import DATASETS, fixture_path

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "fused_host", "fused_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]

# name: (D, dim, T, C, ks)
CASES = {
    "t1": (16, 10, 1, 70, (1, 3, 65, 67)),
    "t2": (16, 10, 2, 40, (1, 3, 65, 67)),
    "t5": (128, 100, 5, 14, (1, 3, 65, 67)),
    "t5_c1": (16, 10, 5, 1, (1, 5)),
    "t64": (16, 10, 64, 128, (3, 1024)),
    "t64_d128": (128, 100, 64, 2, (67,)),
}
TWINS = (TWIN_LO, TWIN_HI)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of one case and the distances of the model: computed once, shared by the tests and the sanitizer driver."""
    D, dim, T, C_, ks = CASES[name]
    raw, norm = synth_index(D, dim)
    batch = synth_batch(raw, dim, T, C_, TWINS, seed=len(name))
    dist = OracleQueryDists(raw, norm, batch["Q"])
    rows = np.random.default_rng(T * C_).permutation(len(raw)).astype(np.uint32)
    return raw, norm, batch, dist, rows


@functools.lru_cache(maxsize=None)
def _want(name, k, with_rows):
    raw, norm, batch, dist, rows = _case(name)
    return fused_model_batch(batch["cand"], batch["n_vectors"], batch["weights"], dist, len(raw), k, rows if with_rows else None)


def test_pair_distance_is_exact_l2_of_a_golden_index():
    """The model's d_t(x) for a FREE query vector has the bytes OracleIndex.exact_l2 returns on the index file."""
    from oracle_lib import Oracle
    for name, bits in (("g16", 1), ("g128", 4)):
        spec = DATASETS[name]
        path = fixture_path(name, bits)
        oi = Oracle().load(path)
        raw, norm = read_v2_vectors(path, spec["n"], spec["dim"], spec["D"])
        rng = np.random.default_rng(spec["n"])
        dist = OracleQueryDists(raw, norm)
        ids = np.arange(spec["n"])
        for q in (rng.standard_normal(spec["dim"]).astype(np.float32), raw[3, :spec["dim"]].copy(),
                  (raw[9, :spec["dim"]] * np.float32(1e3)).astype(np.float32)):
            assert dist.one(q, ids).tobytes() == oi.exact_l2(q, ids.astype(np.uint32)).tobytes(), name


def test_cases_hold_what_they_promise():
    seen_u, seen_kinds = set(), set()
    for name, (D, dim, T, C_, ks) in CASES.items():
        raw, norm, batch, dist, rows = _case(name)
        assert raw[TWIN_LO].tobytes() == raw[TWIN_HI].tobytes() and norm[TWIN_LO].tobytes() == norm[TWIN_HI].tobytes() and dim < D
        check_batch_promises(batch, dist, len(raw), TWINS)
        seen_u |= set(union_sizes(batch, len(raw)))
        seen_kinds |= set(batch["kinds"])
    assert seen_u >= set(U_SIZES) and seen_kinds >= set(KINDS)
    assert {c[2] for c in CASES.values()} == {1, 2, 5, 64} and any(c[2] * c[3] == 8192 for c in CASES.values())
    assert {c[0] for c in CASES.values()} == {16, 128} and {1, 3, 65, 67} <= {k for c in CASES.values() for k in c[4]}


@pytest.mark.parametrize("with_rows", (False, True))
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_matches_the_model(name, with_rows):
    raw, norm, batch, dist, rows = _case(name)
    D, dim, T, C_, ks = CASES[name]
    for k in ks:
        want = _want(name, k, with_rows)
        got = host_fused_rows(batch["cand"], batch["n_vectors"], batch["weights"], dist.q, raw, norm, k, rows if with_rows else None)
        assert same_bytes(got, want), (name, k)
        found = (want[0] >= 0).sum(axis=1)
        for q, U in enumerate(union_sizes(batch, len(raw))):           # the shape of every answer
            f = found[q]
            assert f <= min(k, U) and (want[0][q, f:] == -1).all() and (want[1][q, f:] == FMAX).all() and (want[2][q, f:] == 0).all()
            assert (want[2][q, :f] >= 1).all() and (want[2][q, :f] <= batch["n_vectors"][q]).all()
            assert (np.diff(_orderable(want[1][q, :f])) >= 0).all()
            if batch["kinds"][q] != "nan":
                assert f == min(k, U)
    ones = np.ones_like(batch["weights"])                              # weights = NULL is every weight 1
    k = ks[0]
    assert same_bytes(host_fused_rows(batch["cand"], batch["n_vectors"], None, dist.q, raw, norm, k),
                      host_fused_rows(batch["cand"], batch["n_vectors"], ones, dist.q, raw, norm, k))
    live = batch["n_vectors"] == T                                     # n_vectors = NULL is every vector live
    assert same_bytes([o[live] for o in host_fused_rows(batch["cand"], None, batch["weights"], dist.q, raw, norm, k)],
                      [o[live] for o in _want(name, k, False)])


def test_union_order_does_not_matter():
    """Every row permuted inside itself (the union forms in another order): same bytes."""
    raw, norm, batch, dist, rows = _case("t5")
    rng = np.random.default_rng(8)
    cand, Q, W = batch["cand"].copy(), dist.q.copy(), batch["weights"].copy()
    for q in range(len(cand)):
        for t in range(cand.shape[1]):
            cand[q, t] = cand[q, t, rng.permutation(cand.shape[2])]
    k = 20
    got = host_fused_rows(cand, batch["n_vectors"], W, Q, raw, norm, k)
    assert same_bytes(got, _want("t5", k, False))


def test_a_row_worked_by_hand():
    """D = 8, integers: every product and sum is exact.  Rows: x0 = 0, x1 = e1, x2 = 2 e1, x3 = 2 e2, x4 = x1 (a twin).
    q0 = 0, q1 = 3 e1, q2 = garbage (dead).  d_0 = (0, 1, 4, 4, 1), d_1 = (9, 4, 1, 13, 4).  w = (2, -0.5):
    s = (-4.5, 0, 7.5, 1.5, 0) -> order x0, x1, x4 (tie: the lower id), x3, x2."""
    raw = np.zeros((5, 8), np.float32)
    raw[1, 0] = raw[4, 0] = 1
    raw[2, 0] = 2
    raw[3, 1] = 2
    norm = (raw ** 2).sum(axis=1).astype(np.float32)
    qpad = np.zeros((1, 3, 8), np.float32)
    qpad[0, 1, 0] = 3
    qpad[0, 2] = 1e30
    cand = np.array([[[4, 2, -1, 2], [0, 3, 4, 1], [0, 0, 0, 0]]], np.int64)      # x4: rows 0 and 1; x2: twice in row 0
    w = np.array([[2.0, -0.5, 100.0]], np.float32)
    nv = np.array([2], np.int32)
    ids, score, hits = host_fused_rows(cand, nv, w, qpad, raw, norm, 6)
    assert ids.tolist() == [[0, 1, 4, 3, 2, -1]]
    assert score[0, :5].tolist() == [-4.5, 0.0, 0.0, 1.5, 7.5] and score[0, 5] == FMAX and not np.signbit(score[0, 1:3]).any()
    assert hits.tolist() == [[1, 1, 2, 1, 1, 0]]
    m = fused_model(cand[0], 2, w[0], lambda t, js: ((qpad[0, t][None, :] - raw[js]) ** 2).sum(axis=1).astype(np.float32), 5, 6)
    assert same_bytes(m, (ids[0], score[0], hits[0]))
    rows = np.array([40, 30, 20, 10, 0], np.uint32)
    assert host_fused_rows(cand, nv, w, qpad, raw, norm, 3, rows)[0].tolist() == [[40, 30, 0]]
    # overflow with both signs: 3e38 * 4 = +inf and -3e38 * d_1 = -inf for d_1 >= 4.  x3 (d = 4, 13) is inf + -inf, a NaN, and
    # is dropped; x0, x1, x4 (d_0 <= 1) end at -inf and tie down to the id; x2 (d = 4, 1) ends at +inf, a real slot in front of
    # the padding
    wb = np.array([[BIG, -BIG, 0.0]], np.float32)
    ids, score, hits = host_fused_rows(cand, nv, wb, qpad, raw, norm, 6)
    assert ids.tolist() == [[0, 1, 4, 2, -1, -1]] and (score[0, :3] == -np.inf).all() and score[0, 3] == np.inf
    assert (score[0, 4:] == FMAX).all() and hits.tolist() == [[1, 1, 2, 1, 0, 0]]


def test_refusals_write_nothing():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    raw, norm, batch, dist, rows = _case("t2")
    cand, nv, w = batch["cand"], batch["n_vectors"], batch["weights"]
    n, T, C_ = cand.shape
    k = 10
    out = [np.full((n, k), -7, np.int64), np.full((n, k), -7, np.float32), np.full((n, k), -7, np.int32)]
    before = [o.copy() for o in out]
    po = [o.ctypes.data for o in out]

    def call(cand_=cand, nn=n, T_=T, nv_=nv, w_=w, C__=C_, q_=dist.q, raw_=raw, n_ids=len(raw), D_=raw.shape[1], k_=k, out_=po):
        p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        return L.cph_host_fused_rows(p(cand_), nn, T_, p(nv_), p(w_), C__, p(q_), p(raw_), norm.ctypes.data, n_ids, D_, None, k_, *out_)
    bad_w, bad_w2, bad_nv, bad_nv2 = w.copy(), w.copy(), nv.copy(), nv.copy()
    bad_w[1, 0] = np.inf
    bad_w2[2, 1] = np.nan
    bad_nv[1] = 0
    bad_nv2[3] = T + 1
    for bad, names in ((dict(cand_=None), b"null"), (dict(q_=None), b"null"), (dict(raw_=None), b"null"), (dict(out_=po[:2] + [None]), b"null"),
                       (dict(nn=0), b"sizes"), (dict(n_ids=0), b"sizes"), (dict(D_=12), b"multiple of 8"),
                       (dict(T_=0), b"1 <= vectors <= 64"), (dict(T_=65), b"1 <= vectors <= 64"),
                       (dict(C__=0), b"1 <= candidates <= 1024"), (dict(C__=1025), b"1 <= candidates <= 1024"),
                       (dict(T_=9, C__=1024), b"vectors * candidates <= 8192"),
                       (dict(k_=0), b"1 <= k <= min(1024"), (dict(k_=T * C_ + 1), b"1 <= k <= min(1024"),
                       (dict(T_=8, C__=1024, k_=1025), b"1 <= k <= min(1024"),
                       (dict(nn=2 ** 31, T_=1), b"n * vectors <= 2147483647"), (dict(nn=2 ** 30, T_=2), b"n * vectors <= 2147483647"),
                       (dict(nn=2 ** 24, T_=8, C__=1024), b"n * ceil(vectors * candidates / 64)"),
                       (dict(w_=bad_w), b"weights[1][0] is not finite"), (dict(w_=bad_w2), b"weights[2][1] is not finite"),
                       (dict(nv_=bad_nv), b"n_vectors[1] = 0 is outside [1, 2]"), (dict(nv_=bad_nv2), b"n_vectors[3] = 3 is outside [1, 2]")):
        assert call(**bad) == _lib.INVALID_ARGUMENT, bad
        assert names in L.cph_last_error(), (bad, L.cph_last_error())
        assert same_bytes(out, before), bad
    assert call() == _lib.OK and not same_bytes(out, before)
    # the other new entry points answer before they touch a device
    none3 = [None] * 3
    assert L.cph_search_fused(None, None, 0, 1, None, None, 1, 32, None, 0, None, 0, *none3) == _lib.INVALID_ARGUMENT
    assert L.cph_search_fused_device(None, None, 0, 1, None, None, 1, 32, None, 0, None, 0, *none3, None) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_search_fused(None, None, 0, 1, None, None, 1, 32, None, 0, None, 0, *none3) == _lib.INVALID_ARGUMENT
    assert L.cph_debug_time_fused(None, 1) == _lib.INVALID_ARGUMENT
    assert L.cph_debug_last_fused_us(None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_fused_rows_hook(None, None, None, 1, 1, None, None, 1, 1, *none3) == _lib.INVALID_ARGUMENT


def test_new_symbols_are_declared():
    from cphnsw_mi355x import _lib
    import cphnsw_mi355x
    import inspect
    L = _lib.lib()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    for name in ("cph_search_fused", "cph_search_fused_device", "cph_multi_search_fused", "cph_debug_time_fused", "cph_debug_last_fused_us",
                 "cph_fused_rows_hook", "cph_host_fused_rows"):
        assert f"int {name}(" in flat and hasattr(L, name) and name in _lib.SYMBOLS, name
    assert L.cph_version() >= 115
    ix = cphnsw_mi355x.CPIndex
    assert (ix.FUSED_MAX_VECTORS, ix.FUSED_MAX_CANDIDATES, ix.FUSED_MAX_ENTRIES, ix.FUSED_MAX_K) == \
        (ix.MAXSIM_MAX_TOKENS, ix.MAXSIM_MAX_CANDIDATES, ix.MAXSIM_MAX_ENTRIES, ix.MAXSIM_MAX_K) == (64, 1024, 8192, 1024)
    names = list(inspect.signature(ix.search_fused).parameters)
    assert names == ["self", "queries", "k", "weights", "n_vectors", "candidates", "filter", "exact", "filter_of", "label"]
    for name in ("search_fused_device", "time_fused", "last_fused_us"):
        assert callable(getattr(ix, name))


# ---- the stand-alone program under sanitizers ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("fused_host")), "fused_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_host_twin_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases through the stand-alone program: exact-size buffers, every output byte compared there."""
    path = os.path.join(str(tmp_path), "cases.bin")
    count = 0
    with open(path, "wb") as f:
        f.write(np.uint64(sum(2 * len(c[4]) for c in CASES.values())).tobytes())
        for name in sorted(CASES):
            raw, norm, batch, dist, rows = _case(name)
            n, T, C_ = batch["cand"].shape
            n_ids, D = raw.shape
            for k in CASES[name][4]:
                for with_rows in (False, True):
                    want = _want(name, k, with_rows)
                    f.write(np.array([n, T, C_, n_ids, D, k, int(with_rows)], np.uint64).tobytes())
                    for a in (batch["cand"], batch["n_vectors"], batch["weights"], dist.q, raw, norm) + ((rows,) if with_rows else ()) + want:
                        f.write(np.ascontiguousarray(a).tobytes())
                    count += 1
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"fused: ok ({count} cases)" in r.stdout
