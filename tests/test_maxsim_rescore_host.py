"""CPU tier of the exact rescoring stage of multi-vector search (search_maxsim(..., rescore=R)).

cph_host_maxsim_rescore (csrc/host_maxsim_rescore.h behind the library's host-only hook, no HIP call) is compared, byte for
byte in all six outputs, with tests/maxsim_rescore_model.py over the oracle's eight-chain dot on synthetic vectors: D = 16,
128 and 2048; key segments of 1, 63, 64, 65, 200 and more than 2,000 rows; n_tokens = 1, 7, 8, 9 and T = 64; R = 1, R = k and
R = 1024; found < R; a duplicated vector under two ids of one key; two keys with identical rows; a bitmap that leaves a key
one allowed row; a bitmap per query; a row map.  cph_host_key_rows is compared with a stable numpy argsort.  A property test
runs the lower-bound statement (maxsim_model.py) on brute-force candidate rows made in numpy and checks the rescored answer
against it.  tests/maxsim_rescore_host/maxsim_rescore_host.cpp includes the header, is built with plain g++ and
-fsanitize=address,undefined -ffp-contract=off and runs the same cases as a child process on buffers of exactly the stated
sizes.  No sanitizer touches code loaded into Python."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from maxsim_model import maxsim_model_batch
from maxsim_rescore_model import (FMAX, I32_MAX, I32_MIN, KEY_BIG, KEY_DUP, KEY_HALF, SEG_KEYS, OracleTokenDists, bitmap_words,
                                  host_key_rows, host_maxsim_rescore, key_rows_model, rescore_model_batch, same_bytes,
                                  synth_candidates, synth_index, synth_tokens)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "maxsim_rescore_host", "maxsim_rescore_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]

# name: (D, dim, big, T, n_tokens, R, k, found per query, allow kind, row map)
CASES = {
    "edges16": (16, 10, 2100, 9, (1, 7, 8, 9, 9, 9), 48, 10, (48, 48, 30, 5, 48, 1), None, False),
    "one_row_left": (16, 10, 0, 9, (9, 8, 1), 48, 10, (48, 40, 48), "one", False),
    "twins": (16, 10, 0, 9, (9, 8), 20, 20, (20, 20), None, False),
    "per_query": (16, 10, 0, 9, (9, 7, 9, 1), 32, 32, (32, 32, 20, 32), "each", True),
    "t64_r1": (128, 100, 0, 64, (64, 33), 1, 1, (1, 1), None, False),
    "t64_rk": (128, 100, 0, 64, (64, 1), 7, 7, (7, 3), "one", True),
    "r1024": (16, 10, 0, 3, (3, 2), 1024, 10, (52, 9), None, False),
    "r1024_k1024": (16, 10, 0, 2, (2,), 1024, 1024, (52,), "each", False),
    "chunked2048": (2048, 1536, 0, 3, (3, 1), 16, 4, (16, 2), None, False),
}
MUST = tuple(SEG_KEYS.values()) + (KEY_DUP, -5, 900, KEY_HALF, I32_MIN, I32_MAX, -1)


def _allow(kind, ix, n, seed):
    """None; "one": one bitmap for the batch, in which key 13 (64 rows) keeps ONE allowed row and every other key at least
    one; "each": a bitmap of that kind per query."""
    if kind is None:
        return None
    key_of = ix["key_of"]
    rng = np.random.default_rng(seed)

    def one():
        a = rng.random(len(key_of)) < 0.5
        for key in np.unique(key_of):
            members = np.flatnonzero(key_of == key)
            if key == SEG_KEYS[64]:
                a[members] = False
            if not a[members].any():
                a[rng.choice(members)] = True
        return a
    return one() if kind == "one" else np.stack([one() for _ in range(n)])


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of one case and the model's answer: computed once, shared by the twin test and the sanitizer driver."""
    D, dim, big, T, n_tokens, R, k, founds, akind, with_rows = CASES[name]
    ix = synth_index(D, dim, big)
    n = len(n_tokens)
    nt = np.array(n_tokens, np.int32)
    tok = synth_tokens(ix, n_tokens, T, seed=len(name))
    if name == "twins":
        tok[:, 0] = ix["raw"][ix["dup"][0], :dim]           # token 0 IS the duplicated vector: both ids tie, the lower one wins
    must = tuple(m for m in MUST + ((KEY_BIG,) if big else ()))
    ck, lb, cf = synth_candidates(ix["key_of"], n, R, founds, seed=len(name), must=must)
    allow = _allow(akind, ix, n, seed=R + T)
    rows = np.random.default_rng(R).permutation(len(ix["key_of"])).astype(np.uint32) if with_rows else None
    dists = OracleTokenDists(ix["raw"], ix["norm_sq"], tok)
    want = rescore_model_batch(ck, lb, cf, nt, T, ix["key_of"], dists, allow, k, rows)
    return ix, tok, nt, ck, lb, cf, allow, rows, want


def test_cases_hold_what_they_promise():
    ix = synth_index(16, 10, 2100)
    key_of = ix["key_of"]
    sizes = {int(key): int((key_of == key).sum()) for key in np.unique(key_of)}
    assert all(sizes[key] == length for length, key in SEG_KEYS.items()) and sizes[KEY_BIG] >= 2000
    assert sizes[KEY_HALF] * 2 == len(key_of) and {I32_MIN, I32_MAX, -1} <= set(sizes) and sum(1 for v in sizes.values() if v == 1) >= 41
    lo, hi = ix["dup"]
    assert lo < hi and key_of[lo] == key_of[hi] == KEY_DUP and ix["raw"][lo].tobytes() == ix["raw"][hi].tobytes()
    a, b = (np.flatnonzero(key_of == key) for key in ix["same"])
    assert ix["raw"][a].tobytes() == ix["raw"][b].tobytes() and ix["norm_sq"][a].tobytes() == ix["norm_sq"][b].tobytes()
    assert {c[5] for c in CASES.values()} >= {1, 1024} and any(c[5] == c[6] > 1 for c in CASES.values())
    assert {t for c in CASES.values() for t in c[4]} >= {1, 7, 8, 9, 64} and {c[0] for c in CASES.values()} == {16, 128, 2048}
    assert any(f < c[5] for c in CASES.values() for f in c[7])
    # the duplicated vector: the lower id is reported; the twin keys: equal scores, the smaller key first
    ix, tok, nt, ck, lb, cf, allow, rows, want = _case("twins")
    lo, hi = ix["dup"]
    for q in range(len(nt)):                                  # (R = k and every special key is a candidate: all are answered)
        slots = {int(key): j for j, key in enumerate(want[0][q, :want[4][q]])}
        assert want[3][q, slots[KEY_DUP], 0] == lo and hi not in want[3][q, slots[KEY_DUP]]
        assert slots[900] == slots[-5] + 1 and want[1][q, slots[900]].tobytes() == want[1][q, slots[-5]].tobytes()
    ix, tok, nt, ck, lb, cf, allow, rows, want = _case("one_row_left")
    members = np.flatnonzero(ix["key_of"] == SEG_KEYS[64])
    assert allow[members].sum() == 1
    q = 0
    slot = want[0][q, :want[4][q]].tolist()
    if SEG_KEYS[64] in slot:
        assert set(want[3][q, slot.index(SEG_KEYS[64]), :nt[q]].tolist()) == {int(members[allow[members]][0])}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_matches_the_model(name):
    ix, tok, nt, ck, lb, cf, allow, rows, want = _case(name)
    D, dim, big, T, n_tokens, R, k, founds, akind, with_rows = CASES[name]
    got = host_maxsim_rescore(ck, lb, cf, tok, nt, ix["raw"], ix["norm_sq"], ix["key_of"], allow, k, rows)
    assert same_bytes(got, want), name
    n = len(nt)
    for q in range(n):                                        # the shape of every answer
        f = want[4][q]
        assert f == min(k, founds[q]) and (want[2][q, :f] == nt[q]).all() and (want[3][q, :f, :nt[q]] >= 0).all()
        assert (want[3][q, :, nt[q]:] == -1).all() and (want[0][q, f:] == 0).all() and (want[1][q, f:] == FMAX).all()
        assert (want[2][q, f:] == 0).all() and (want[3][q, f:] == -1).all() and 0 <= want[5][q] <= f
        assert founds[q] == R or want[5][q] == f
        assert (np.diff(want[1][q, :f].view(np.uint32).astype(np.int64)) >= 0).all()
    if np.all(nt == T):                                       # n_tokens = NULL is every token live
        assert same_bytes(host_maxsim_rescore(ck, lb, cf, tok, None, ix["raw"], ix["norm_sq"], ix["key_of"], allow, k, rows), want)


def test_certified_follows_the_last_lower_bound():
    """R found: the leading slots strictly below lb_{R-1}; every value of the bound from 'below all' to 'above all'."""
    ix, tok, nt, ck, lb, cf, allow, rows, want = _case("per_query")
    R, k = ck.shape[1], want[0].shape[1]
    seen = set()
    for q in np.flatnonzero(cf == R):
        scores = want[1][q, :want[4][q]]
        for bound in (np.float32(0.0), scores[0], scores[3], np.nextafter(scores[3], np.float32(np.inf)), FMAX):
            lb2 = lb.copy()
            lb2[q, R - 1] = bound
            got = host_maxsim_rescore(ck, lb2, cf, tok, nt, ix["raw"], ix["norm_sq"], ix["key_of"], allow, k, rows)
            expect = int((scores < bound).sum())                    # (scores ascend)
            assert got[5][q] == expect and same_bytes(got[:5], want[:5])
            seen.add(expect)
    assert {0, k} <= seen and any(0 < c < k for c in seen)


def test_host_key_rows_matches_a_stable_argsort():
    rng = np.random.default_rng(5)
    n = 4001
    keys = rng.integers(-50, 50, n).astype(np.int64)
    keys[rng.random(n) < 0.5] = 7                              # one key owns half the rows
    keys[:6] = [I32_MIN, I32_MAX, -1, I32_MAX, I32_MIN, -1]
    keys[100:140] = 10 ** 6 + np.arange(40)                    # singletons
    for col in (keys, keys[:1], keys[:0], np.full(65, 3), np.arange(64)[::-1] - 32):
        ids, ukeys, offs = host_key_rows(col)
        want = key_rows_model(col)
        assert np.array_equal(ids[:len(col)], want[0]) and np.array_equal(ukeys, want[1]) and np.array_equal(offs, want[2])
    ids, ukeys, offs = host_key_rows(keys)
    assert ukeys[0] == I32_MIN and ukeys[-1] == I32_MAX and -1 in ukeys and (np.diff(ukeys.astype(np.int64)) > 0).all()
    u = int(np.searchsorted(ukeys, 7))
    assert offs[u + 1] - offs[u] >= n // 2 and (np.diff(offs.astype(np.int64)) == 1).sum() >= 40
    for u in range(len(ukeys)):
        seg = ids[offs[u]:offs[u + 1]]
        assert (keys[seg] == ukeys[u]).all() and (np.diff(seg.astype(np.int64)) > 0).all()


# ---- the claims: lower bound, equality on full hits, exactness --------------------------------------------------------------
def _documents():
    """240 documents of five rows around their own centre plus 300 rows in one tight cluster (documents of five too), 16
    dimensions; queries of T = 4 tokens, each query around ONE document's centre: that document is found by every token,
    its neighbours by some."""
    rng = np.random.default_rng(77)
    n_docs, per, dim = 240, 5, 16
    centre = rng.standard_normal((n_docs, dim)).astype(np.float32)
    X = (np.repeat(centre, per, axis=0) + np.float32(0.3) * rng.standard_normal((n_docs * per, dim))).astype(np.float32)
    tight = (np.float32(6.0) + np.float32(0.05) * rng.standard_normal((300, dim))).astype(np.float32)
    raw = np.concatenate([X, tight])
    key_of = (np.arange(len(raw)) // per - 7).astype(np.int32)
    norm = (raw.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    T, n = 4, 6
    target = rng.integers(0, n_docs, n)
    tok = (centre[target][:, None, :] + np.float32(0.3) * rng.standard_normal((n, T, dim))).astype(np.float32)
    tok[-1] = np.float32(6.0) + np.float32(0.05) * rng.standard_normal((T, dim)).astype(np.float32)      # one query inside the cluster
    n_tokens = np.array([4, 4, 3, 4, 1, 4], np.int32)
    return raw, norm, key_of, tok, n_tokens


def _top_c(dists, n, T, C_, allow):
    """Brute-force candidate rows: per token the C smallest (distance bits, id) over the allowed ids."""
    ids, dist = np.full((n, T, C_), -1, np.int64), np.full((n, T, C_), FMAX, np.float32)
    for q in range(n):
        for t in range(T):
            d = dists(q, t)
            pool = np.arange(len(d)) if allow is None else np.flatnonzero(allow)
            o = pool[np.lexsort((pool, d[pool].view(np.uint32)))[:C_]]
            ids[q, t, :len(o)], dist[q, t, :len(o)] = o, d[o]
    return ids, dist


@pytest.mark.parametrize("filtered", (False, True))
def test_properties_on_brute_force_candidate_rows(filtered):
    raw, norm, key_of, tok, n_tokens = _documents()
    n, T, _ = tok.shape
    n_ids, k, C_ = len(raw), 10, 16
    allow = (np.random.default_rng(3).random(n_ids) < 0.7) if filtered else None
    dists = OracleTokenDists(raw, norm, tok)
    ids, dist = _top_c(dists, n, T, C_, allow)
    full = slots_low = rose = 0
    for R in (10, 24):
        lower = maxsim_model_batch(ids, dist, n_tokens, key_of, n_ids, R)
        ck, lb, hits, cf = lower[0], lower[1], lower[2], lower[4]
        got = host_maxsim_rescore(ck, lb, cf, tok, n_tokens, raw, norm, key_of, allow, k)
        assert same_bytes(got, rescore_model_batch(ck, lb, cf, n_tokens, T, key_of, dists, allow, k))
        for q in range(n):
            slot_of = {int(key): j for j, key in enumerate(ck[q, :cf[q]])}
            for o in range(got[4][q]):
                j = slot_of[int(got[0][q, o])]
                assert got[1][q, o] >= lb[q, j], (R, q, o)                       # a lower bound it was
                if hits[q, j] == n_tokens[q]:
                    assert got[1][q, o].tobytes() == lb[q, j].tobytes(), (R, q, o)
                    full += 1
                else:
                    slots_low += 1
                rose += int(got[1][q, o] > lb[q, j])
            assert got[5][q] <= got[4][q]
    assert full > 0 and slots_low > 0 and rose > 0, (full, slots_low, rose)
    # R at least the number of distinct keys of the rows a query's tokens returned, over rows that hold EVERY allowed id:
    # the brute-force MaxSim top-k, all of it certified
    pool = np.arange(n_ids) if allow is None else np.flatnonzero(allow)
    ids_all, dist_all = _top_c(dists, n, T, len(pool), allow)
    ukeys = np.unique(key_of[pool])
    R = len(ukeys)
    assert k <= R <= 1024
    lower = maxsim_model_batch(ids_all, dist_all, n_tokens, key_of, n_ids, R)
    got = host_maxsim_rescore(lower[0], lower[1], lower[4], tok, n_tokens, raw, norm, key_of, allow, k)
    for q in range(n):
        score = np.zeros(R, np.float32)
        for t in range(int(n_tokens[q])):
            best = np.full(R, np.inf, np.float32)
            np.minimum.at(best, np.searchsorted(ukeys, key_of[pool]), dists(q, t)[pool])
            score = (score + best).astype(np.float32)
        o = np.lexsort((ukeys, score))[:k]
        assert lower[4][q] == R and got[4][q] == k and got[5][q] == k
        assert np.array_equal(got[0][q], ukeys[o]) and got[1][q].tobytes() == score[o].tobytes()
        assert same_bytes([x[q] for x in got[:4]], [x[q, :k] for x in lower[:4]])       # every hit was full: the bound was the score


# ---- refusals and declarations -----------------------------------------------------------------------------------------------
def test_host_twin_refuses_bad_arguments():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    ix, tok, nt, ck, lb, cf, allow, rows, want = _case("one_row_left")
    n, R = ck.shape
    T, dim = tok.shape[1], tok.shape[2]
    k = 10
    out = [np.empty_like(w) for w in want]
    po = [o.ctypes.data for o in out]
    raw, norm, key_of = ix["raw"], ix["norm_sq"], ix["key_of"]

    def call(ck_=ck, cf_=cf, nn=n, R_=R, T_=T, nt_=nt, k_=k, D_=raw.shape[1], dim_=dim, out_=po, raw_=raw):
        return L.cph_host_maxsim_rescore(None if ck_ is None else ck_.ctypes.data, lb.ctypes.data, cf_.ctypes.data, nn, R_, tok.ctypes.data,
                                         T_, dim_, None if nt_ is None else nt_.ctypes.data, None if raw_ is None else raw_.ctypes.data,
                                         norm.ctypes.data, len(key_of), D_, key_of.ctypes.data, None, None, k_, *out_)
    assert call() == _lib.OK
    for bad, names in ((dict(ck_=None), b"null"), (dict(raw_=None), b"null"), (dict(out_=po[:5] + [None]), b"null"), (dict(nn=0), b"sizes"),
                       (dict(R_=k - 1), b"k <= rescore <= 1024"), (dict(R_=1025), b"k <= rescore <= 1024"), (dict(k_=0), b"k <= 1024"),
                       (dict(T_=65), b"tokens <= 64"), (dict(D_=12), b"multiple of 8"), (dict(dim_=17), b"dim <= D"),
                       (dict(nn=2 ** 22, R_=1024), b"n * rescore"),
                       (dict(cf_=np.array([48, 49, 48], np.int32)), b"cand_found[1] = 49 is outside [0, 48]"),
                       (dict(nt_=np.array([9, 0, 1], np.int32)), b"n_tokens[1] = 0 is outside [1, 9]")):
        assert call(**bad) == _lib.INVALID_ARGUMENT, bad
        assert names in L.cph_last_error(), (bad, L.cph_last_error())
    nk = C.c_uint64()
    assert L.cph_host_key_rows(None, 3, None, None, None, C.byref(nk)) == _lib.INVALID_ARGUMENT
    # the other new entry points answer before they touch a device
    none6 = [None] * 6
    assert L.cph_search_maxsim_rescored(None, None, 0, 1, None, 1, 32, 8, None, None, 0, None, 0, *none6) == _lib.INVALID_ARGUMENT
    assert L.cph_search_maxsim_rescored_device(None, None, 0, 1, None, 1, 32, 8, None, None, 0, None, 0, *none6, None) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_search_maxsim_rescored(None, None, 0, 1, None, 1, 32, 8, None, None, 0, None, 0, *none6) == _lib.INVALID_ARGUMENT
    assert L.cph_prepare_maxsim_rescore(None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_debug_time_maxsim_rescore(None, 1) == _lib.INVALID_ARGUMENT
    assert L.cph_debug_last_maxsim_rescore_us(None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_maxsim_rescore_hook(None, None, None, None, 1, 1, None, 1, None, None, None, 1, *none6) == _lib.INVALID_ARGUMENT


def test_new_symbols_are_declared():
    from cphnsw_mi355x import _lib
    import cphnsw_mi355x
    import inspect
    L = _lib.lib()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    for name in ("cph_search_maxsim_rescored", "cph_search_maxsim_rescored_device", "cph_multi_search_maxsim_rescored",
                 "cph_prepare_maxsim_rescore", "cph_debug_time_maxsim_rescore", "cph_debug_last_maxsim_rescore_us",
                 "cph_maxsim_rescore_hook", "cph_host_maxsim_rescore", "cph_host_key_rows"):
        assert f"int {name}(" in flat and hasattr(L, name) and name in _lib.SYMBOLS, name
    assert L.cph_version() >= 113
    ix = cphnsw_mi355x.CPIndex
    assert ix.MAXSIM_MAX_RESCORE == 1024
    for fn in (ix.search_maxsim, ix.search_maxsim_device):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "rescore" and params[-1].default is None          # appended: no positional call moved
    for name in ("prepare_maxsim_rescore", "time_maxsim_rescore", "last_maxsim_rescore_us"):
        assert callable(getattr(ix, name))


# ---- the stand-alone program under sanitizers ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("maxsim_rescore_host")), "maxsim_rescore_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_host_twin_and_key_rows_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases through the stand-alone program: exact-size buffers, every output byte compared there; then the key
    columns of test_host_key_rows_matches_a_stable_argsort."""
    path = os.path.join(str(tmp_path), "cases.bin")
    with open(path, "wb") as f:
        f.write(np.uint64(len(CASES)).tobytes())
        for name in sorted(CASES):
            ix, tok, nt, ck, lb, cf, allow, rows, want = _case(name)
            n, R = ck.shape
            T, dim = tok.shape[1], tok.shape[2]
            n_ids, D = ix["raw"].shape
            k = want[0].shape[1]
            words = None if allow is None else bitmap_words(np.broadcast_to(allow, (n, n_ids)) if allow.ndim == 1 else allow, n_ids)
            f.write(np.array([n, R, T, dim, n_ids, D, k, int(words is not None), int(rows is not None)], np.uint64).tobytes())
            for a in (ck, lb, cf, tok, nt, ix["raw"], ix["norm_sq"], ix["key_of"]) + (() if words is None else (words,)) + \
                    (() if rows is None else (rows,)) + want:
                f.write(np.ascontiguousarray(a).tobytes())
        rng = np.random.default_rng(9)
        cols = [rng.integers(-9, 9, 777).astype(np.int32), np.array([I32_MAX, I32_MIN, -1, I32_MIN], np.int32), np.zeros(0, np.int32),
                np.where(rng.random(1500) < 0.5, 4, rng.integers(-2 ** 31, 2 ** 31, 1500)).astype(np.int32)]
        f.write(np.uint64(len(cols)).tobytes())
        for col in cols:
            ids, ukeys, offs = key_rows_model(col)
            f.write(np.array([len(col), len(ukeys)], np.uint64).tobytes())
            for a in (col, ids, ukeys, offs):
                f.write(np.ascontiguousarray(a).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"maxsim rescore: ok ({len(CASES)} cases, {len(cols)} key columns)" in r.stdout
