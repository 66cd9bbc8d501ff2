"""CPU tier of multi-vector (MaxSim) search (search_maxsim): the host statement of the pass over the candidate rows.

cph_host_maxsim_rows (csrc/host_maxsim.h behind the library's host-only hook, no HIP call) is compared, byte for byte in all
five outputs, with tests/maxsim_model.py on synthetic queries: every (T, C) of maxsim_model.TCS -- every power-of-two
boundary of the kernel's sort -- with k in {1, 10, 1024}, each with and without a row map, 39 queries per case: the 13 kinds
of maxsim_model.KINDS under n_tokens = T, 1 and T - 1 each, garbage in the ignored rows.  tests/maxsim_host/maxsim_host.cpp
includes csrc/host_maxsim.h, is built with plain g++ and -fsanitize=address,undefined and runs the same cases as a child
process on buffers of exactly the stated sizes.  No sanitizer touches code loaded into Python."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from maxsim_model import (FMAX, KINDS, KS, N_IDS, R_SOLO, SPECIAL, TCS, TIE_HI, TIE_LO, host_maxsim_rows, maxsim_model,
                          maxsim_model_batch, same_bytes, shapes, synth_batch)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "maxsim_host", "maxsim_host.cpp")
COMMON = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror"]


@functools.lru_cache(maxsize=None)
def _case(T, Cn):
    """The batch of one (T, C) and the model's answers at every k, with and without the row map: computed once."""
    ids, dist, n_tokens, key_of, rows, kinds = synth_batch(T, Cn, seed=1)
    want = {(k, rm): maxsim_model_batch(ids, dist, n_tokens, key_of, N_IDS, k, rows if rm else None) for k in KS for rm in (False, True)}
    return ids, dist, n_tokens, key_of, rows, kinds, want


def _check_batch_promises(T, Cn, ids, dist, n_tokens, key_of, kinds, want):
    """The batch holds what the case list promises (so that a generator that quietly stopped producing a case fails here).
    want: the model's answers at k = 1, 10, 1024 without a row map."""
    n = ids.shape[0]
    assert n == 3 * len(KINDS) and set(kinds) == set(KINDS)
    assert set(n_tokens.tolist()) == {1, max(1, T - 1), T}
    full = {kind: next(i for i in range(n) if kinds[i] == kind and n_tokens[i] == T) for kind in KINDS}
    every = {kind: [i for i in range(n) if kinds[i] == kind] for kind in KINDS}
    assert all({int(n_tokens[i]) for i in qs} == {1, max(1, T - 1), T} for qs in every.values())
    w1, w10, wk = want[1], want[10], want[1024]
    valid = (ids >= 0) & (ids < N_IDS)
    for q in range(n):
        valid[q, n_tokens[q]:] = False                                      # the live rows only
    keys = np.where(valid, key_of[np.where(valid, ids, 0)], 0)

    def live_keys(q):
        return keys[q][valid[q]]
    q = full["one_key"]
    assert valid[q].all() and set(live_keys(q)) == {7} and wk[4][q] == 1 and wk[2][q, 0] == T
    q = full["distinct_keys"]
    assert len(set(live_keys(q))) == T * Cn and wk[4][q] == min(1024, T * Cn) and (wk[2][q, :wk[4][q]] == 1).all()
    q = full["special_keys"]
    assert set(live_keys(q)) <= set(SPECIAL) and (T * Cn < 40 or set(live_keys(q)) == set(SPECIAL))
    if T * Cn >= 40:
        assert wk[4][q] == 5 and sorted(wk[0][q, :5].tolist()) == sorted(SPECIAL)
    if Cn >= 6:
        q = full["repeated_ids"]
        for t in range(T):
            c = np.unique(ids[q, t], return_counts=True)[1]
            assert 2 in c and 3 in c
    if T >= 2:
        q = full["padding_token"]
        assert not valid[q, 1].any() and valid[q, 0].all() and (wk[2][q, :wk[4][q]] <= T - 1).all() and (wk[3][q, :, 1] == -1).all()
    if Cn >= 2:
        q = full["partly_padded"]
        per_row = valid[q].sum(axis=1)
        assert 0 < valid[q].sum() < T * Cn and (per_row < Cn).all()
        if Cn >= T + 1:
            assert (per_row > 0).all()
        if Cn >= 4 and T == 1:
            assert not valid[q, 0, 1] and valid[q, 0, 0]                    # the hole in front of valid entries
    for q in every["all_padded"]:                                           # found = 0, whatever the ignored rows hold
        assert not valid[q].any() and wk[4][q] == 0 and w1[4][q] == 0
        if n_tokens[q] < T:
            assert ((ids[q, n_tokens[q]:] >= 0) & (ids[q, n_tokens[q]:] < N_IDS)).any(), "the garbage must hold ids that look valid"
    if Cn >= 2:
        q = full["equal_distances"]
        d = dist[q]
        assert np.signbit(d[0, 0]) and d[0, 0] == 0 and not np.signbit(d[0, 1]) and d[0, 1] == 0       # -0.0 next to +0.0
        assert (np.diff(d, axis=1) == 0).sum() > T * Cn // 3
    q = full["negative_distances"]
    assert (dist[q] < 0).any() and (dist[q] > -1e-5).all() and w1[1][q, 0] <= wk[1][q, wk[4][q] - 1]
    if Cn >= 2:
        for q in every["tied_scores"]:
            # the larger key sits in front in every row; the answer puts the smaller first, with the same score bytes
            assert key_of[ids[q, 0, 0]] == TIE_HI and key_of[ids[q, 0, 1]] == TIE_LO and ids[q, 0, 0] == R_SOLO
            assert w1[0][q, 0] == TIE_LO and wk[0][q, :2].tolist() == [TIE_LO, TIE_HI]
            assert wk[1][q, 0].tobytes() == wk[1][q, 1].tobytes() and (wk[2][q, :2] == n_tokens[q]).all()
    q = full["few_keys"]
    assert 0 < w10[4][q] < 10 and w10[4][q] == min(3, T * Cn) and (w10[0][q, w10[4][q]:] == 0).all()
    if T >= 2 and Cn >= 2:
        q = full["one_token_key"]
        solo = int(key_of[R_SOLO + 2])
        at = wk[0][q, :wk[4][q]].tolist().index(solo)
        # nearer than every other entry of the query, on one token only: the floors of the others put it behind
        assert dist[q, 0, 0] < dist[q].ravel()[1:].min() and wk[2][q, at] == 1 and at > 0
        assert wk[3][q, at, 0] == ids[q, 0, 0] and (wk[3][q, at, 1:] == -1).all()
    # padding: every slot behind the last key; the ignored tokens have no rows
    for k in KS:
        w = want[k]
        for q in range(n):
            f = w[4][q]
            assert (w[0][q, f:] == 0).all() and (w[1][q, f:] == FMAX).all() and (w[2][q, f:] == 0).all() and (w[3][q, f:] == -1).all()
            assert (w[3][q, :, n_tokens[q]:] == -1).all() and (w[2][q, :f] >= 1).all() and (w[2][q, :f] <= n_tokens[q]).all()
            assert ((w[3][q, :f] >= 0).sum(axis=1) == w[2][q, :f]).all()


@pytest.mark.parametrize("T,Cn", TCS)
def test_host_maxsim_rows_matches_the_model(T, Cn):
    ids, dist, n_tokens, key_of, rows, kinds, want = _case(T, Cn)
    assert ids.shape == (3 * len(KINDS), T, Cn) and key_of.shape == (N_IDS,) and sorted(rows.tolist()) == list(range(N_IDS))
    _check_batch_promises(T, Cn, ids, dist, n_tokens, key_of, kinds, {k: want[k, False] for k in KS})
    for k in KS:
        assert same_bytes(host_maxsim_rows(ids, dist, n_tokens, key_of, k), want[k, False]), k
        assert same_bytes(host_maxsim_rows(ids, dist, n_tokens, key_of, k, rows), want[k, True]), (k, "rows")
        # the row map only renames rows
        a, b = want[k, False], want[k, True]
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3] + a[4:], b[:3] + b[4:]))
        m = a[3] >= 0
        assert np.array_equal(b[3][m], rows[a[3][m]]) and (b[3][~m] == -1).all()
    # n_tokens = NULL is every token live
    full = np.flatnonzero(n_tokens == T)
    got = host_maxsim_rows(ids[full], dist[full], None, key_of, 10)
    assert same_bytes(got, tuple(x[full] for x in want[10, False]))


def test_model_on_a_query_worked_by_hand():
    key_of = np.array([5, 5, -1, 9, -2 ** 31, 9], np.int32)
    #           token 0: ids 3 (key 9), 0 (key 5), 2 (key -1), padding      token 1: ids 1 (key 5), 5 (key 9), 1 again, 4 (INT32_MIN)
    ids = np.array([[3, 0, 2, -1], [1, 5, 1, 4], [7, 7, 7, 7]], np.int64)        # token 2: ids outside [0, 6): all invalid
    dist = np.array([[0.5, 1.0, 2.0, FMAX], [0.25, 0.75, 1.5, 3.0], [0.0, 0.0, 0.0, 0.0]], np.float32)
    keys, score, hits, rows, found = maxsim_model(ids, dist, 3, key_of, 6, 5)
    # floors: 2.0, 3.0, +0.0.  key 5: 1.0 + 0.25 + 0; key 9: 0.5 + 0.75 + 0; key -1: 2.0 + 3.0 + 0; INT32_MIN: 2.0 + 3.0 + 0
    assert found == 4 and keys.tolist() == [5, 9, -2 ** 31, -1, 0]              # 5.0 twice: the smaller key first
    assert score.tolist() == [1.25, 1.25, 5.0, 5.0, float(FMAX)] and hits.tolist() == [2, 2, 1, 1, 0]
    assert rows.tolist() == [[0, 1, -1], [3, 5, -1], [-1, 4, -1], [2, -1, -1], [-1, -1, -1]]
    # one live token: the other rows, floors included, are not read
    keys, score, hits, rows, found = maxsim_model(ids, dist, 1, key_of, 6, 2)
    assert found == 2 and keys.tolist() == [9, 5] and score.tolist() == [0.5, 1.0] and rows.tolist() == [[3, -1, -1], [0, -1, -1]]
    got = host_maxsim_rows(ids[None], dist[None], np.array([3], np.int32), key_of[:6], 5)
    assert same_bytes(got, maxsim_model_batch(ids[None], dist[None], [3], key_of, 6, 5))


def test_host_maxsim_rows_refuses_bad_arguments():
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    ids, dist, n_tokens, key_of, rows, _, _ = _case(3, 65)
    n = ids.shape[0]
    o = (np.empty((n, 1024), np.int32), np.empty((n, 1024), np.float32), np.empty((n, 1024), np.int32), np.empty((n, 1024, 64), np.int64),
         np.empty(n, np.int32))
    po = [x.ctypes.data for x in o]
    big_i, big_d = np.full(n * 9 * 1024, -1, np.int64), np.zeros(n * 9 * 1024, np.float32)       # room for the largest refused shape

    def call(i=ids, d=dist, nn=n, T=3, nt=n_tokens, Cn=65, ko=key_of, nk=N_IDS, k=3, out=po):
        return L.cph_host_maxsim_rows(None if i is None else i.ctypes.data, None if d is None else d.ctypes.data, nn, T,
                                      None if nt is None else nt.ctypes.data, Cn, None if ko is None else ko.ctypes.data, nk, None, k, *out)
    assert call() == _lib.OK and call(nt=None) == _lib.OK
    for bad, names in ((dict(i=None), b"null"), (dict(d=None), b"null"), (dict(ko=None), b"null"), (dict(out=[None] + po[1:]), b"null"),
                       (dict(out=po[:4] + [None]), b"null"), (dict(nn=0), b"sizes"), (dict(nk=0), b"sizes"),
                       (dict(i=big_i, d=big_d, T=0), b"tokens <= 64"), (dict(i=big_i, d=big_d, T=65, Cn=1), b"tokens <= 64"),
                       (dict(Cn=0), b"candidates <= 1024"), (dict(i=big_i, d=big_d, T=1, Cn=1025), b"candidates <= 1024"),
                       (dict(i=big_i, d=big_d, T=9, Cn=1024), b"tokens * candidates <= 8192"), (dict(k=0), b"k <= 1024"),
                       (dict(k=1025), b"k <= 1024"), (dict(nn=2 ** 31, T=1), b"2147483647"), (dict(nn=2 ** 30, T=2), b"2147483647"),
                       (dict(nt=np.where(np.arange(n) == 5, 0, n_tokens).astype(np.int32)), b"n_tokens[5] = 0 is outside [1, 3]"),
                       (dict(nt=np.where(np.arange(n) == 7, 4, n_tokens).astype(np.int32)), b"n_tokens[7] = 4 is outside [1, 3]")):
        assert call(**bad) == _lib.INVALID_ARGUMENT, bad
        assert names in L.cph_last_error(), (bad, L.cph_last_error())
    # the other new entry points answer before they touch a device
    none5 = [None] * 5
    assert L.cph_search_maxsim(None, None, 0, 1, None, 1, 32, None, None, 0, None, 0, *none5) == _lib.INVALID_ARGUMENT
    assert L.cph_search_maxsim_device(None, None, 0, 1, None, 1, 32, None, None, 0, None, 0, *none5, None) == _lib.INVALID_ARGUMENT
    assert L.cph_multi_search_maxsim(None, None, 0, 1, None, 1, 32, None, None, 0, None, 0, *none5) == _lib.INVALID_ARGUMENT
    assert L.cph_debug_time_maxsim(None, 1) == _lib.INVALID_ARGUMENT
    assert L.cph_debug_last_maxsim_rows_us(None, None) == _lib.INVALID_ARGUMENT
    assert L.cph_maxsim_rows_hook(0, None, None, 1, 1, None, 32, None, 1, None, 1, *none5) == _lib.INVALID_ARGUMENT


def test_new_symbols_are_declared_with_the_issue_s_signatures():
    from cphnsw_mi355x import _lib
    import cphnsw_mi355x
    L = _lib.lib()
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read())
    call = ("uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k, uint64_t candidates, const cph_group_keys* keys, "
            "const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact, ")
    outs = "int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows, int32_t* out_found);"
    rows_args = ("const int64_t* ids, const float* dist, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t candidates, "
                 "const int32_t* key_of, uint64_t n_keys, const uint32_t* rows, uint64_t k, " + outs)
    for decl in ("int cph_search_maxsim(cph_index* h, const float* queries, " + call + outs,
                 "int cph_search_maxsim_device(cph_index* h, const float* d_queries, " + call +
                 "int32_t* d_keys, float* d_score, int32_t* d_hits, int64_t* d_rows, int32_t* d_found, void* stream);",
                 "int cph_multi_search_maxsim(cph_multi* m, const float* queries, " +
                 call.replace("cph_group_keys* keys", "cph_group_keys* const* keys") + outs,
                 "int cph_debug_time_maxsim(cph_index* h, int on);", "int cph_debug_last_maxsim_rows_us(cph_index* h, double* us);",
                 "int cph_maxsim_rows_hook(int device, " + rows_args, "int cph_host_maxsim_rows(" + rows_args):
        assert decl in flat, decl
    p, u64 = C.c_void_p, C.c_uint64
    entry = [p, p, u64, u64, p, u64, u64, p, p, C.c_uint32, p, C.c_int, p, p, p, p, p]
    rows_sig = [p, p, u64, u64, p, u64, p, u64, p, u64, p, p, p, p, p]
    want = {"cph_search_maxsim": entry, "cph_search_maxsim_device": entry + [p], "cph_multi_search_maxsim": entry,
            "cph_debug_time_maxsim": [p, C.c_int], "cph_debug_last_maxsim_rows_us": [p, C.POINTER(C.c_double)],
            "cph_maxsim_rows_hook": [C.c_int] + rows_sig, "cph_host_maxsim_rows": rows_sig}
    for name, args in want.items():
        assert hasattr(L, name) and _lib.SYMBOLS[name] == (C.c_int, args), name
    assert L.cph_version() >= 111
    ix = cphnsw_mi355x.CPIndex
    assert (ix.MAXSIM_MAX_TOKENS, ix.MAXSIM_MAX_CANDIDATES, ix.MAXSIM_MAX_ENTRIES, ix.MAXSIM_MAX_K) == (64, 1024, 8192, 1024)
    for name in ("search_maxsim", "search_maxsim_device", "time_maxsim", "last_maxsim_rows_us"):
        assert callable(getattr(ix, name))
    for T, Cn in TCS:                                      # every tested shape is inside the limits
        assert 1 <= T <= 64 and 1 <= Cn <= 1024 and T * Cn <= 8192


@pytest.fixture(scope="module")
def asan_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    exe = os.path.join(str(tmp_path_factory.mktemp("maxsim_host")), "maxsim_host_asan")
    cmd = [cxx] + COMMON + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_maxsim_rows_host_under_asan_ubsan(asan_exe, tmp_path):
    """The same cases as above, through the stand-alone program: exact-size buffers, every output byte compared there."""
    path = os.path.join(str(tmp_path), "cases.bin")
    n_cases = 0
    with open(path, "wb") as f:
        f.write(np.uint64(0).tobytes())
        for (T, Cn, k) in shapes():
            ids, dist, n_tokens, key_of, rows, _, want = _case(T, Cn)
            for rm, nt in ((False, n_tokens), (True, n_tokens), (False, None)):
                sel = slice(None) if nt is not None else np.flatnonzero(n_tokens == T)
                w = tuple(x[sel] for x in want[k, rm])
                f.write(np.array([ids[sel].shape[0], T, Cn, k, key_of.size, int(rm), int(nt is not None)], np.uint64).tobytes())
                for a in (ids[sel], dist[sel]) + (() if nt is None else (nt,)) + (key_of,) + ((rows,) if rm else ()) + w:
                    f.write(np.ascontiguousarray(a).tobytes())
                n_cases += 1
        f.seek(0)
        f.write(np.uint64(n_cases).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:allocator_may_return_null=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([asan_exe, path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert f"maxsim: ok ({n_cases} cases)" in r.stdout and n_cases == 3 * len(shapes())
