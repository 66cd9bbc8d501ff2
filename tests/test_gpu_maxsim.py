"""Multi-vector (MaxSim) search on the GPU (CPIndex.search_maxsim / search_maxsim_device, cph_maxsim_rows_hook).

The yardstick is tests/maxsim_model.py: the kernel hook is compared with it and with the host twin on synthetic queries; an
end-to-end call is compared with the model applied to the rows search_batch(tokens.reshape(n * T, dim), C, ...) returns in
internal ids on the same handle, under every option the underlying search takes."""
import functools

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path
from maxsim_model import (FMAX, I32_MAX, I32_MIN, KINDS, KS, N_IDS, TCS, hook_maxsim_rows, host_maxsim_rows, maxsim_model_batch,
                          same_bytes, synth_batch)

pytestmark = pytest.mark.gpu

FIXTURES = [("g16", 1), ("g1024", 2), ("g2048", 1)]
STATES = ("plain", "input", "removed", "added")
TC = ((1, 70), (3, 65), (32, 40))                       # (T, C) of the end-to-end calls


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


# ---- the kernel against the host twin and the model -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch(T, Cn, n, first):
    return synth_batch(T, Cn, n=n, seed=n, first=first)


@pytest.mark.parametrize("T,Cn", TCS)
def test_kernel_hook_matches_host_twin_and_model(T, Cn):
    """39 queries (more than one workgroup; every kind under n_tokens = T, 1 and T - 1) at k = 1, 10, 1024; 1 and 3 queries
    at k = 10."""
    for n, first in ((1, 3), (3, 7), (3 * len(KINDS), 0)):
        ids, dist, n_tokens, key_of, rows, kinds = _batch(T, Cn, n, first)
        assert ids.shape == (n, T, Cn) and (n < len(KINDS) or set(kinds) == set(KINDS))
        for k in (KS if n > 3 else (10,)):
            want = maxsim_model_batch(ids, dist, n_tokens, key_of, N_IDS, k)
            assert same_bytes(host_maxsim_rows(ids, dist, n_tokens, key_of, k), want), (T, Cn, k, n)
            assert same_bytes(hook_maxsim_rows(0, ids, dist, n_tokens, key_of, k), want), (T, Cn, k, n)
            if k == 10:
                twin = host_maxsim_rows(ids, dist, n_tokens, key_of, k, rows)
                m = want[3] >= 0                             # (the row map only renames rows: checked on the CPU tier)
                assert np.array_equal(twin[3][m], rows[want[3][m]]) and same_bytes(twin[:3] + twin[4:], want[:3] + want[4:])
                assert same_bytes(hook_maxsim_rows(0, ids, dist, n_tokens, key_of, k, rows), twin), (T, Cn, k, n, "rows")
        full = np.flatnonzero(n_tokens == T)                 # n_tokens = NULL: every token is live
        assert same_bytes(hook_maxsim_rows(0, ids[full], dist[full], None, key_of, 10),
                          maxsim_model_batch(ids[full], dist[full], None, key_of, N_IDS, 10)), (T, Cn, n, "no n_tokens")


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _keys_for(n, seed):
    """Some keys own many rows, some one row; the ends of int32 occur."""
    rng = np.random.default_rng(seed)
    a = rng.random(n)
    keys = np.where(a < 0.5, 0, np.where(a < 0.8, rng.integers(1, 4, n), 1000 + np.arange(n)))
    keys[rng.integers(0, n, 3)] = [I32_MIN, I32_MAX, -1]
    return keys.astype(np.int64)


def _tokens(Q, n, T, seed):
    """n queries of T token vectors around the rows of Q, and ragged lengths that hold 1 and T."""
    rng = np.random.default_rng(seed)
    base = Q[rng.integers(0, len(Q), (n, T))]
    tok = (base + np.float32(0.1) * np.abs(base).mean() * rng.standard_normal(base.shape)).astype(np.float32)
    n_tokens = rng.integers(1, T + 1, n).astype(np.int32)
    n_tokens[0], n_tokens[-1] = T, 1
    tok[-1, 1:] = np.float32(1e3)                           # garbage in the ignored rows of the last query
    return tok, n_tokens


def _rows_internal(ix, tok, C_, **kw):
    """The candidate rows of the statement: search_batch over the n * T token rows at k = C, in internal ids, on the same
    handle; a per-query argument serves the T tokens of its query."""
    n, T, dim = tok.shape
    for name in ("filter_of", "label"):
        if name in kw and np.ndim(kw[name]) == 1:
            kw[name] = np.repeat(np.asarray(kw[name]), T)
    was = ix.result_ids
    ix.result_ids = "internal"
    try:
        ids, dist = ix.search_batch(tok.reshape(n * T, dim), C_, **kw)
    finally:
        ix.result_ids = was
    return ids.reshape(n, T, C_), dist.reshape(n, T, C_)


def _expect(ix, tok, n_tokens, k, C_, key_of, **kw):
    ids, dist = _rows_internal(ix, tok, C_, **kw)
    rows = ix.row_map() if ix.result_ids == "input" else None
    return maxsim_model_batch(ids, dist, n_tokens, np.asarray(key_of, np.int32), ix.size, k, rows)


@pytest.fixture(scope="module")
def built(cph, tmp_path_factory):
    """8,230 x 16 at 1 bit, as tests/test_gpu_grouped.py builds it, saved once; every test loads its own copy."""
    rng = np.random.default_rng(77)
    n, dim = 8230, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[:2000] = np.float32(6.0) + np.float32(0.05) * X[:2000]
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    path = str(tmp_path_factory.mktemp("maxsim") / "built.cphn")
    ix.save_native(path)
    Q = rng.standard_normal((12, dim)).astype(np.float32)
    Q[:4] = np.float32(6.0) + np.float32(0.05) * Q[:4]
    return dict(path=path, X=X, Q=Q, dim=dim)


def _open(cph, gold, built, name, bits):
    if name == "built":
        ix = cph.CPIndex(built["dim"], bits)
        ix.load_native(built["path"])
        return ix, built["Q"]
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits))
    ix.set_row_map(np.random.default_rng(5).permutation(ix.size))      # (a v2 file carries none)
    return ix, gold[f"Q/{name}"][:12]


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name,bits", FIXTURES + [("built", 1)])
def test_end_to_end_options(cph, gold, built, name, bits, state):
    ix, Q = _open(cph, gold, built, name, bits)
    n0 = ix.size
    rng = np.random.default_rng(n0 + len(state))
    key_of = _keys_for(n0, n0)
    ix.set_labels(key_of, ids="internal")
    if state == "input":
        ix.result_ids = "input"
    if state in ("removed", "added"):
        gone = rng.choice(n0, n0 // 5, replace=False)
        assert ix.remove(gone, ids="internal") == len(gone)
    if state == "added":
        twin = ix.get_vectors(5, 1)
        extra = np.concatenate([twin, twin + np.float32(0.25), rng.standard_normal((6, ix.dim)).astype(np.float32)])
        extra_keys = np.array([777777, int(key_of[5]), 0, 0, 1, 424242, I32_MIN, -1], np.int64)
        ix.add(extra, labels=extra_keys)
        key_of = np.concatenate([key_of, extra_keys])
    n = ix.size
    mask = rng.random(n) < 0.4
    small = rng.random(n) < 0.08
    f = ix.make_filter(mask, ids="internal")
    f2 = ix.make_filter(small, ids="internal")
    empty = ix.make_filter(np.zeros(n, bool), ids="internal")
    nq = 5
    fo = rng.integers(-1, 3, nq)
    lab = key_of[rng.integers(0, n, nq)]
    variants = [dict(), dict(exact=True), dict(filter=f), dict(filter=f, exact=True), dict(filter=empty), dict(label=0),
                dict(label=lab, exact=True), dict(filter=[f, f2, empty], filter_of=fo, exact=True)]
    if state != "added":        # (inherited: per-query filters would walk the graph of an index with a tail)
        variants += [dict(label=lab), dict(filter=[f, f2, empty], filter_of=fo)]
    other = (key_of * 7 + 3) % 11                         # a second column: other keys
    gk_other = ix.make_group_keys(other, ids="internal")
    for (T, C_) in TC:
        tok, n_tokens = _tokens(Q, nq, T, n0 + T)
        assert set(n_tokens.tolist()) >= {1, T}
        for k in (1, 10):
            for kw in variants:
                got = ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=C_, **kw)
                assert got[0].shape == (nq, k) and got[3].shape == (nq, k, T) and got[4].shape == (nq,)
                assert same_bytes(got, _expect(ix, tok, n_tokens, k, C_, key_of, **kw)), (name, state, T, k, sorted(kw))
        # every token live without n_tokens; a keys object gives other keys
        tok[-1, 1:] = tok[0, :T - 1]
        assert same_bytes(ix.search_maxsim(tok, 10, candidates=C_), _expect(ix, tok, None, 10, C_, key_of))
        got_o = ix.search_maxsim(tok, 10, n_tokens=n_tokens, candidates=C_, keys=gk_other, filter=f)
        assert same_bytes(got_o, _expect(ix, tok, n_tokens, 10, C_, other, filter=f))
    if state == "added":
        with pytest.raises(NotImplementedError):
            ix.search_maxsim(tok, 3, candidates=17, label=lab)
    for x in (f, f2, empty, gk_other):
        x.close()


def test_cosine_metric(cph):
    rng = np.random.default_rng(11)
    n, dim = 2500, 24
    X = (rng.standard_normal((n, dim)) * rng.uniform(0.2, 5.0, (n, 1))).astype(np.float32)
    ix = cph.CPIndex(dim, 4, metric="cosine")
    ix.build(X)
    ix.finalize()
    key_of = np.arange(n) // 5 - 7                        # documents of five chunks
    ix.set_labels(key_of, ids="internal")
    Q = rng.standard_normal((8, dim)).astype(np.float32)
    for (T, C_) in TC:
        tok, n_tokens = _tokens(Q, 4, T, T)
        tok[:-1] *= np.float32(3.0)                       # (the length of a query vector does not matter)
        for kw in (dict(), dict(exact=True)):
            got = ix.search_maxsim(tok, 10, n_tokens=n_tokens, candidates=C_, **kw)
            assert same_bytes(got, _expect(ix, tok, n_tokens, 10, C_, key_of, **kw)), (T, sorted(kw))
            f = got[4][0]
            sim = n_tokens[0] - got[1][0, :f]             # MaxSim similarity = n_tokens - score
            assert f > 0 and (sim <= n_tokens[0] + 1e-3).all() and (np.diff(sim) <= 0).all()


# ---- the exactness claim ----------------------------------------------------------------------------------------------------
def _brute_force(ids, dist, n_tokens, key_of, size, k):
    """MaxSim over ALL rows from exact rows that hold every id: per token the distance of every id, per key the minimum
    over its rows, the sequential float32 sum, the k smallest (score, key) -> (keys [n, k], score [n, k], {key: score})."""
    n, T, _ = ids.shape
    ukeys = np.unique(key_of)
    out_k, out_s, every = np.zeros((n, k), np.int32), np.full((n, k), FMAX, np.float32), []
    for q in range(n):
        score = np.zeros(len(ukeys), np.float32)
        for t in range(int(n_tokens[q])):
            d = np.full(size, np.inf, np.float32)
            d[ids[q, t]] = dist[q, t]
            assert np.isfinite(d).all()
            best = np.full(len(ukeys), np.inf, np.float32)
            np.minimum.at(best, np.searchsorted(ukeys, key_of), d)
            score = (score + best).astype(np.float32)
        o = np.lexsort((ukeys, score))[:k]
        out_k[q, :len(o)], out_s[q, :len(o)] = ukeys[o], score[o]
        every.append(dict(zip(ukeys.tolist(), score)))
    return out_k, out_s, every


def test_exactness_and_lower_bound(cph, gold):
    ix, Q = _open(cph, gold, None, "g16", 1)
    size = ix.size
    assert size <= 1024
    key_of = (np.arange(size) * 7 % 41 - 3).astype(np.int32)            # 41 documents of seven or eight rows
    ix.set_labels(key_of, ids="internal")
    T, k = 8, 10
    tok, n_tokens = _tokens(Q, 6, T, 3)
    tok[-1, 1:] = tok[0, :T - 1]                                           # (search_batch below reads every row)
    ids, dist = _rows_internal(ix, tok, size, exact=True)
    assert (np.sort(ids, axis=2) == np.arange(size)).all()
    want_k, want_s, every = _brute_force(ids, dist, n_tokens, key_of, size, k)
    got = ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=size, exact=True)
    assert (got[4] == k).all() and (got[2] == n_tokens[:, None]).all()     # every hits == n_tokens
    assert np.array_equal(got[0], want_k) and got[1].tobytes() == want_s.tobytes()
    # C = 16: a lower bound of the true score of every returned key, equal where every token found a row of it
    low = ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=16, exact=True)
    assert (low[4] == k).all() and (low[2] < n_tokens[:, None]).any() and (low[2] == n_tokens[:, None]).any()
    for q in range(len(tok)):
        for j in range(low[4][q]):
            true = every[q][int(low[0][q, j])]
            assert low[1][q, j] <= true, (q, j)
            if low[2][q, j] == n_tokens[q]:
                assert low[1][q, j].tobytes() == np.float32(true).tobytes(), (q, j)


def test_one_token_and_distinct_keys_is_the_plain_search(cph, gold):
    """T = 1 with every row its own key: the answer is the row of search_batch(q, k) with repeated ids dropped.  The exact
    route returns no id twice and, on this fixture, distinct distances: there the two calls agree slot for slot.  The graph
    rows of the fixtures hold ids twice (the reference's rows do), so there the first occurrences are what is compared."""
    ix, Q = _open(cph, gold, None, "g16", 1)
    Q = gold["Q/g16"]
    size, k = ix.size, 10
    gk = ix.make_group_keys(np.arange(size), ids="internal")
    for space in ("internal", "input"):
        ix.result_ids = space
        for kw in (dict(), dict(exact=True)):
            plain = ix.search_batch(Q, k, **kw)
            got = ix.search_maxsim(Q[:, None, :], k, candidates=k, keys=gk, **kw)
            assert (plain[0] >= 0).all() and not (np.signbit(plain[1]) & (plain[1] == 0)).any()
            if kw:
                assert (np.diff(plain[1], axis=1) > 0).all()                     # distinct distances: (score, key) is the row's order
                assert np.array_equal(got[3][:, :, 0], plain[0]) and got[1].tobytes() == plain[1].tobytes() and (got[4] == k).all()
            for q in range(len(Q)):
                first = np.sort(np.unique(plain[0][q], return_index=True)[1])    # an id's first position in the row
                f = len(first)
                assert got[4][q] == f and (got[2][q, :f] == 1).all() and (np.diff(plain[1][q, first]) > 0).all()
                assert np.array_equal(got[3][q, :f, 0], plain[0][q, first]) and got[1][q, :f].tobytes() == plain[1][q, first].tobytes()
                ids = got[3][q, :f, 0] if space == "internal" else np.argsort(ix.row_map())[got[3][q, :f, 0]]
                assert np.array_equal(got[0][q, :f], ids)                        # the key of a row is its internal id
                assert (got[0][q, f:] == 0).all() and (got[1][q, f:] == FMAX).all() and (got[3][q, f:] == -1).all()
    gk.close()


# ---- the device variant ------------------------------------------------------------------------------------------------------
def test_device_variant(cph, gold):
    import torch
    ix, Q = _open(cph, gold, None, "g16", 1)
    n = ix.size
    key_of = _keys_for(n, 3)
    ix.set_labels(key_of, ids="internal")
    dev = torch.device("cuda", 0)
    T, k, C_ = 5, 6, 40
    tok, n_tokens = _tokens(Q, 7, T, 9)
    nq = len(tok)
    Td = torch.from_numpy(tok).to(dev)
    f = ix.make_filter(np.arange(n) % 3 != 0, ids="internal")
    fo = np.arange(nq) % 2 - 1
    cases = [dict(), dict(n_tokens=n_tokens), dict(n_tokens=n_tokens, exact=True), dict(n_tokens=n_tokens, filter=f),
             dict(n_tokens=n_tokens, filter=[f], filter_of=fo), dict(n_tokens=n_tokens, label=0)]
    st1, st2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for st in (st1, st2):
        st.wait_stream(torch.cuda.current_stream(dev))

    def fresh_out(nn, kk, TT):
        return (torch.full((nn, kk), -9, dtype=torch.int32, device=dev), torch.full((nn, kk), -9.0, device=dev),
                torch.full((nn, kk), -9, dtype=torch.int32, device=dev), torch.full((nn, kk, TT), -9, dtype=torch.int64, device=dev),
                torch.full((nn,), -9, dtype=torch.int32, device=dev))
    for kw in cases:
        want = ix.search_maxsim(tok, k, candidates=C_, **kw)
        got = ix.search_maxsim_device(Td, k, candidates=C_, **kw)
        torch.cuda.synchronize()
        assert same_bytes([t.cpu().numpy() for t in got], want), sorted(kw)
        # out= and a side stream; the results are used in stream order, with no host wait in between
        out = fresh_out(nq, k, T)
        st1.wait_stream(torch.cuda.current_stream(dev))
        res = ix.search_maxsim_device(Td, k, candidates=C_, out=out, stream=st1, **kw)
        with torch.cuda.stream(st1):
            copies = [t.clone() for t in res]
        st1.synchronize()
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
        assert same_bytes([t.cpu().numpy() for t in copies], want), sorted(kw)
    # default candidates: the single pass at C0 = min(1024, 8192 // T, max(32, 4 k))
    got = ix.search_maxsim_device(Td, k, n_tokens=n_tokens)
    torch.cuda.synchronize()
    assert same_bytes([t.cpu().numpy() for t in got], ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=32))
    assert same_bytes(ix.search_maxsim(tok, 20, n_tokens=n_tokens), ix.search_maxsim(tok, 20, n_tokens=n_tokens, candidates=80))
    # non-contiguous input: every second token of a longer tensor
    wide = torch.zeros((nq, 2 * T, tok.shape[2]), device=dev)
    wide[:, ::2] = Td
    view = wide[:, ::2]
    assert not view.is_contiguous()
    got = ix.search_maxsim_device(view, k, n_tokens=n_tokens, candidates=C_)
    torch.cuda.synchronize()
    assert same_bytes([t.cpu().numpy() for t in got], ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=C_))
    with pytest.raises(ValueError, match="out must be"):
        ix.search_maxsim_device(Td, k, candidates=C_, out=fresh_out(nq, k, T + 1))
    # two batches on two streams
    tok_b, nt_b = _tokens(Q[::-1].copy(), 4, 3, 10)
    want_a = ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=C_)
    want_b = ix.search_maxsim(tok_b, 3, n_tokens=nt_b, candidates=90, exact=True)
    Tb = torch.from_numpy(tok_b).to(dev)
    torch.cuda.synchronize()
    for _ in range(2):
        a = ix.search_maxsim_device(Td, k, n_tokens=n_tokens, candidates=C_, stream=st1)
        b = ix.search_maxsim_device(Tb, 3, n_tokens=nt_b, candidates=90, exact=True, stream=st2)
        with torch.cuda.stream(st1):
            ca = [t.clone() for t in a]
        with torch.cuda.stream(st2):
            cb = [t.clone() for t in b]
        st1.synchronize()
        st2.synchronize()
        assert same_bytes([t.cpu().numpy() for t in ca], want_a) and same_bytes([t.cpu().numpy() for t in cb], want_b)
    ix.synchronize()
    f.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(cph, gold):
    ix, Q = _open(cph, gold, None, "g16", 1)
    n, dim = ix.size, ix.dim
    tok, n_tokens = _tokens(Q, 4, 3, 1)
    with pytest.raises(ValueError, match="set_labels"):
        ix.search_maxsim(tok, 3)                           # no label column, no keys
    gk = ix.make_group_keys(np.arange(n) % 7)

    def zeros(nq, T):
        return np.zeros((nq, T, dim), np.float32)
    for bad, what in ((dict(queries=zeros(1, 65)), "tokens <= 64"), (dict(queries=zeros(1, 0)), "tokens <= 64"),
                      (dict(candidates=0), r"\[1, 1024\]"), (dict(candidates=1025), r"\[1, 1024\]"),
                      (dict(queries=zeros(1, 9), candidates=1024), "tokens \\* candidates <= 8192"),
                      (dict(queries=zeros(1, 64), candidates=129), "tokens \\* candidates <= 8192"),
                      (dict(k=0), "k <= 1024"), (dict(k=1025), "k <= 1024"),
                      (dict(queries=tok[0]), "tokens, dim"), (dict(queries=zeros(4, 3)[:, :, :dim - 1]), "tokens, dim"),
                      (dict(n_tokens=[3, 3, 3]), "length 4"), (dict(n_tokens=[3, 0, 3, 3]), r"\[1, 3\]"),
                      (dict(n_tokens=[3, 4, 3, 3]), r"\[1, 3\]"), (dict(n_tokens=np.ones((4, 1), np.int32)), "length 4"),
                      (dict(n_tokens=np.ones(4, np.float32)), "integer"), (dict(keys=np.arange(n)), "GroupKeys"),
                      (dict(label=0, filter=np.ones(n, bool)), "exclude")):
        kw = dict(queries=tok, k=3, candidates=20, keys=gk)
        kw.update(bad)
        if "label" in bad:
            ix.set_labels(np.arange(n) % 7, ids="internal")
        with pytest.raises(ValueError, match=what):
            ix.search_maxsim(kw.pop("queries"), **kw)
    # the library's own refusals name the limit too (the Python checks are in front of them)
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    o = (np.empty((1, 4), np.int32), np.empty((1, 4), np.float32), np.empty((1, 4), np.int32), np.empty((1, 4, 65), np.int64), np.empty(1, np.int32))
    po = [x.ctypes.data for x in o]
    q = zeros(1, 65)
    nt = np.array([4], np.int32)
    for args, what in (((1, 65, None, 4, 16), b"tokens <= 64"), ((1, 3, None, 4, 1025), b"candidates <= 1024"),
                       ((1, 64, None, 4, 129), b"tokens * candidates <= 8192"), ((1, 3, None, 1025, 16), b"k <= 1024"),
                       ((1, 3, nt.ctypes.data, 4, 16), b"n_tokens[0] = 4 is outside [1, 3]"), ((2 ** 30, 2, None, 4, 16), b"2147483647")):
        nq, T, ntp, k, C_ = args
        assert L.cph_search_maxsim(ix._h, q.ctypes.data, nq, T, ntp, k, C_, gk._hs[0], None, 0, None, 0, *po) == _lib.INVALID_ARGUMENT
        assert what in L.cph_last_error(), (args, L.cph_last_error())
    assert ix.search_maxsim(zeros(0, 3), 3, candidates=20, keys=gk)[0].shape == (0, 3)          # an empty batch is no error
    other, _ = _open(cph, gold, None, "g16", 1)
    with pytest.raises(ValueError, match="another index"):
        other.search_maxsim(tok, 3, candidates=20, keys=gk)
    gk.close()
    with pytest.raises(ValueError, match="closed"):
        ix.search_maxsim(tok, 3, candidates=20, keys=gk)
    with pytest.raises(ValueError, match="no timed maxsim search"):
        ix.last_maxsim_rows_us()
    ix.time_maxsim(True)
    ix.search_maxsim(tok, 3, n_tokens=n_tokens, candidates=20)
    assert ix.last_maxsim_rows_us() > 0
    ix.time_maxsim(False)


# ---- replicas and parts ------------------------------------------------------------------------------------------------------
def test_replicas_equal_one_device_and_parts_are_refused(cph, gold):
    name, bits = "g16", 1
    one, _ = _open(cph, gold, None, name, bits)
    Q = gold[f"Q/{name}"]
    m = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0])
    m.set_min_shard(1)
    m.load(fixture_path(name, bits))
    m.set_row_map(one.row_map())
    n = one.size
    key_of = _keys_for(n, 9)
    other = (key_of * 5 + 1) % 13
    mask = np.arange(n) % 4 != 1
    tok, n_tokens = _tokens(Q, 9, 4, 2)                    # nine queries over two replicas: shards of five and four
    fo = np.arange(len(tok)) % 3 - 1
    for ix in (one, m):
        ix.set_labels(key_of, ids="internal")
    for ids in ("internal", "input"):
        one.result_ids = m.result_ids = ids
        gk1, gkm = one.make_group_keys(other, ids="internal"), m.make_group_keys(other, ids="internal")
        f1, fm = one.make_filter(mask, ids="internal"), m.make_filter(mask, ids="internal")
        e1, em = one.make_filter(~mask, ids="internal"), m.make_filter(~mask, ids="internal")
        for kw1, kwm in ((dict(), dict()), (dict(exact=True), dict(exact=True)), (dict(filter=f1), dict(filter=fm)),
                         (dict(keys=gk1, filter=f1, exact=True), dict(keys=gkm, filter=fm, exact=True)),
                         (dict(filter=[f1, e1], filter_of=fo), dict(filter=[fm, em], filter_of=fo)), (dict(label=0), dict(label=0))):
            for cand in (40, None):
                assert same_bytes(m.search_maxsim(tok, 6, n_tokens=n_tokens, candidates=cand, **kwm),
                                  one.search_maxsim(tok, 6, n_tokens=n_tokens, candidates=cand, **kw1)), (ids, sorted(kw1), cand)
        for x in (gk1, gkm, f1, fm, e1, em):
            x.close()
    p = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0], partition=True)
    with pytest.raises(ValueError, match="partitioned"):
        p.search_maxsim(tok, 6)
    import torch
    with pytest.raises(ValueError, match="partitioned"):
        p.search_maxsim_device(torch.from_numpy(tok).to("cuda:0"), 6)


# ---- nothing else moved ------------------------------------------------------------------------------------------------------
def test_other_searches_are_untouched(cph, gold):
    """search_batch and search_grouped return the same bytes before and after maxsim calls on the handle: the scratch rows
    are shared with grouped search."""
    ix, Q = _open(cph, gold, None, "g16", 1)
    ix.set_labels(_keys_for(ix.size, 1), ids="internal")
    tok, n_tokens = _tokens(Q, 6, 7, 4)
    for space in ("internal", "input"):
        ix.result_ids = space
        before = ix.search_batch(Q, 10)
        grouped_before = ix.search_grouped(Q, 4, 2, candidates=50)
        for _ in range(5):                                 # (more calls than the handle has scratch sets)
            ix.search_maxsim(tok, 4, n_tokens=n_tokens, candidates=50)
            ix.search_maxsim(tok, 4, candidates=90, exact=True)
        assert ix.result_ids == space
        assert same_bytes(ix.search_grouped(Q, 4, 2, candidates=50), grouped_before)
        assert same_bytes(ix.search_batch(Q, 10), before)
    ix.result_ids = "internal"
    assert np.array_equal(ix.search_batch(Q, 10)[0], gold["S/g16/b1/plain/k10/ids"][:len(Q)])       # (Q: the first 12 queries)


def test_rerankers_share_scratch_at_growing_shapes(cph, gold):
    """Grouped, maxsim and diverse calls take turns on the scratch sets of ONE handle, four calls each (one per set), at shapes
    chosen so that a later call needs a longer buffer in one output slot while every other size a call could compare is
    already long enough: with n = 4, grouped (k=2, g=1) leaves 8 slots per output, maxsim (T=8, k=8) 256 rows but 32 scores,
    grouped (k=8, g=8) then needs 256 distances with n * k = 32 and n = 4 unchanged.  Every answer is the model's, byte for
    byte; then the same sequence in the _device forms into preallocated outputs on one stream."""
    import torch
    from diverse_model import diverse_model_batch
    from group_model import group_model_batch
    ix, _ = _open(cph, gold, None, "g16", 1)
    Q = gold["Q/g16"][:4]
    key_of = _keys_for(ix.size, 2).astype(np.int32)
    ix.set_labels(key_of, ids="internal")
    tok, _ = _tokens(Q, 4, 8, 5)
    tok[-1, 1:] = tok[0, :7]                                # (every token is live: no n_tokens)
    C_ = 64
    was, ix.result_ids = ix.result_ids, "internal"
    rows, rows_tok = ix.search_batch(Q, C_), ix.search_batch(tok.reshape(32, -1), C_)
    ix.result_ids = was

    def pair(s, js):
        return ix.exact_l2(ix.get_vectors(s, 1)[0], np.asarray(js, np.int64))
    want = {("grouped", 2, 1): group_model_batch(*rows, key_of, 2, 1), ("grouped", 8, 8): group_model_batch(*rows, key_of, 8, 8),
            ("maxsim", 8): maxsim_model_batch(rows_tok[0].reshape(4, 8, C_), rows_tok[1].reshape(4, 8, C_), None, key_of, ix.size, 8),
            ("diverse", 16): diverse_model_batch(*rows, 16, 0.5, pair, ix.size)}
    sequence = [("grouped", 2, 1), ("maxsim", 8), ("grouped", 8, 8), ("diverse", 16), ("grouped", 8, 8)]
    dev = torch.device("cuda", 0)
    Qd, Td, st = torch.from_numpy(Q).to(dev), torch.from_numpy(tok).to(dev), torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    for device_form in (False, True):
        for step, call in enumerate(sequence):
            for rep in range(4):
                if device_form:
                    out = [torch.full(w.shape, 9, dtype=getattr(torch, w.dtype.name), device=dev) for w in want[call]]
                    st.wait_stream(torch.cuda.current_stream(dev))
                    fn = getattr(ix, f"search_{call[0]}_device")
                    got = fn(Td if call[0] == "maxsim" else Qd, *call[1:], candidates=C_, out=out, stream=st)
                    st.synchronize()
                    got = [t.cpu().numpy().view(w.dtype) for t, w in zip(got, want[call])]
                else:
                    got = getattr(ix, f"search_{call[0]}")(tok if call[0] == "maxsim" else Q, *call[1:], candidates=C_)
                    got = [np.asarray(g).view(w.dtype) for g, w in zip(got, want[call])]
                assert same_bytes(got, want[call]), (device_form, step, call, rep)
