"""Exhaustive MaxSim on the GPU: search_maxsim(candidates="all", rescore=R), search_maxsim_device and cph_maxsim_all_hook.

One index of 2,600 Gaussian rows per dim (10, 24, 96: D = 16 with the zero-filled K chunk, one chunk, four chunks).  The key
column, in the order of the inverted column: a document of 1 row, documents of 2 .. 40 rows, one of 300 rows (three column
tiles), one of 32 rows that ends exactly on column 1,152 = 9 x 128, then documents of 37 rows -- at dim 24 single-row
documents instead, 1,490 keys in all, more than R = 1,024.  The ids of every document are scattered over the id space.

The reference is the byte-exact statement of the rescoring stage (tests/maxsim_rescore_model.py over exact_l2 of the handle)
with EVERY key that has an allowed row as a candidate.  The tightness bound is the one derived in csrc/host_maxsim_all.h:
score - lb <= sum over live tokens of 2 eps_t + (6 + 2 L) 2^-24 score / (1 - L 2^-24), eps from cph_host_exact_matrix_slack."""
import numpy as np
import pytest

from exact_matrix_model import slack_of
from maxsim_rescore_model import bitmap_words, rescore_model_batch, same_bytes
from test_gpu_maxsim_rescore import Dists

pytestmark = pytest.mark.gpu

DIMS = {10: 16, 24: 32, 96: 128}
N = 2600
SHAPES = ((1, 37), (3, 37), (32, 5), (64, 5))          # (T, queries): T = 3 pads to 4; the last query tile is partial
FILTERS = ("none", "half", "each", "removed", "added")
NONE = 0xFFFFFFFF
_W = {}


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _doc_sizes(dim):
    sizes = [1] + list(range(2, 41)) + [300, 32]
    assert sum(sizes) == 1152
    rest = N - 1152
    return sizes + ([1] * rest if dim == 24 else [37] * (rest // 37) + [rest % 37])


def _world(cph, dim, cosine=False, singles=False):
    """Once per module, dim and metric: the index with its label column, and the documents (singles: 2,600 of one row)."""
    if (dim, cosine, singles) not in _W:
        rng = np.random.default_rng(9100 + dim)
        X = rng.standard_normal((N, dim)).astype(np.float32)
        sizes = [1] * N if singles else _doc_sizes(dim)
        key_of = np.empty(N, np.int32)
        key_of[rng.permutation(N)] = np.repeat(np.arange(len(sizes)), sizes) * 3 - 50
        ix = cph.CPIndex(dim, 4, metric="cosine") if cosine else cph.CPIndex(dim, 4)
        ix.build(X)
        ix.finalize()
        ix.set_labels(key_of[ix.row_map()], ids="internal")
        _W[dim, cosine, singles] = dict(ix=ix, X=X, key_in=key_of, key_of=key_of[ix.row_map()].copy(), live=np.ones(N, bool))
    return _W[dim, cosine, singles]


def _tokens(w, T, n, seed, ragged=True):
    rng = np.random.default_rng(seed)
    V = w["ix"].get_vectors(0, w["ix"].size)
    tok = (V[rng.integers(0, len(V), (n, T))] + np.float32(0.3) * rng.standard_normal((n, T, V.shape[1]))).astype(np.float32)
    nt = rng.integers(1, T + 1, n).astype(np.int32) if ragged else np.full(n, T, np.int32)
    nt[0] = T
    for q, L in enumerate(nt):
        tok[q, L:] = np.float32(1e30)                         # garbage in the ignored rows
    return tok, nt


def _state(w, kind, n, seed):
    """The filter situation -> (allow bool [n, size] as the kernels see it, the keyword arguments of the search)."""
    ix, rng = w["ix"], np.random.default_rng(seed)
    if kind == "removed" and w["live"].all():
        gone = rng.choice(N, 40, replace=False)
        assert ix.remove(gone, ids="internal") == 40
        w["live"][gone] = False
    if kind == "added" and ix.size == N:
        extra = rng.standard_normal((9, ix.dim)).astype(np.float32)
        labels = np.array([-50, -50, 70, 70, 70, 9001, 9001, 9002, 73], np.int32)     # old documents and three new ones
        ix.add(extra, labels=labels)
        w["key_of"] = np.concatenate([w["key_of"], labels])
        w["live"] = np.concatenate([w["live"], np.ones(9, bool)])
    size, key_of = ix.size, w["key_of"]
    allow = np.broadcast_to(w["live"], (n, size)).copy()
    kw = {}
    if kind == "half":
        one = rng.random(size) < 0.5
        allow &= one
        kw = dict(filter=ix.make_filter(one, ids="internal"))
    if kind == "each":
        each = rng.random((n, size)) < 0.5
        each[1, key_of == key_of[0]] = False                  # query 1: a whole document is disallowed
        each[2] = False                                       # query 2: an empty filter
        allow &= each
        kw = dict(filter=[ix.make_filter(e, ids="internal") for e in each], filter_of=np.arange(n))
    return allow, kw


def _hook(w, tok, nt, allow, R):
    from cphnsw_mi355x import _lib
    ix, (n, T, _) = w["ix"], tok.shape
    nk = len(np.unique(w["key_of"]))
    words = bitmap_words(allow, ix.size)
    table = np.zeros((n, nk), np.uint32)
    ck, lb, cf = np.zeros((n, R), np.int32), np.zeros((n, R), np.float32), np.zeros(n, np.int32)
    _lib.check(_lib.lib().cph_maxsim_all_hook(ix._h, tok.ctypes.data, n, T, nt.ctypes.data, None, words.ctypes.data, R, table.ctypes.data,
                                              ck.ctypes.data, lb.ctypes.data, cf.ctypes.data))
    return table, ck, lb, cf


def _scores(w, tok, nt, allow, cosine=False):
    """Every (query, key rank): the model's score over the key's allowed rows (float32, token order), inf without one."""
    d = Dists(w["ix"], tok, cosine)
    ukeys, rank = np.unique(w["key_of"], return_inverse=True)
    out = np.full((len(tok), len(ukeys)), np.inf, np.float32)
    for q in range(len(tok)):
        s = np.zeros(len(ukeys), np.float32)
        for t in range(nt[q]):
            m = np.full(len(ukeys), np.inf, np.float32)
            np.minimum.at(m, rank[allow[q]], d(q, t)[allow[q]])
            s = (s + m).astype(np.float32)
        out[q] = s
    return ukeys, out


def _all_keys_model(w, tok, nt, allow, k, cosine=False):
    """The statement with every key that has an allowed row as a candidate."""
    ukeys = np.unique(w["key_of"])
    n, R = len(tok), len(ukeys) + 1
    ck, cf = np.zeros((n, R), np.int32), np.zeros(n, np.int32)
    for q in range(n):
        have = np.unique(w["key_of"][allow[q]])
        ck[q, :len(have)], cf[q] = have, len(have)
    return rescore_model_batch(ck, np.zeros((n, R), np.float32), cf, nt, tok.shape[1], w["key_of"], Dists(w["ix"], tok, cosine), allow, k)


def _tightness(w, tok, nt, scores):
    D = DIMS[w["ix"].dim]
    flat = tok.reshape(-1, tok.shape[2])
    eps = slack_of(np.where(np.abs(flat) < 1e20, flat, 0), w["ix"].get_vectors(0, w["ix"].size), D)      # (ignored rows: unused)
    eps = eps.reshape(tok.shape[:2])
    out = np.empty(scores.shape)
    for q, L in enumerate(nt):
        out[q] = 2 * eps[q, :L].sum() + (6 + 2 * L) * 2.0 ** -24 * scores[q].astype(np.float64) / (1 - L * 2.0 ** -24)
    return out


def _check_candidates(table, has, ukeys, R, ck, clb, cf):
    """cand_* are the R smallest of every table row by (lb, key)."""
    lb = table.view(np.float32)
    for q in range(len(table)):
        order = np.flatnonzero(has[q])[np.argsort(table[q, has[q]], kind="stable")][:R]
        assert cf[q] == len(order) and (ck[q, :cf[q]] == ukeys[order]).all() and clb[q, :cf[q]].tobytes() == lb[q, order].tobytes()


@pytest.mark.parametrize("kind", FILTERS)
@pytest.mark.parametrize("T,n", SHAPES)
@pytest.mark.parametrize("dim", sorted(DIMS))
def test_bounds_and_answer(cph, dim, T, n, kind):
    w = _world(cph, dim)
    ix = w["ix"]
    tok, nt = _tokens(w, T, n, seed=dim + T)
    allow, kw = _state(w, kind, n, seed=T)
    from cphnsw_mi355x import _lib
    small = (T, kind) == (3, "each")                          # this point: a table of 20 queries, so two chunks of the 37
    _lib.check(_lib.lib().cph_debug_maxsim_all_budget(ix._h, 20 * 4 * len(np.unique(w["key_of"])) if small else 0))
    ukeys, s = _scores(w, tok, nt, allow)
    has = np.isfinite(s)
    # 1. the bound table and the candidates, through the hook
    R = 1024 if dim == 24 else 128
    table, ck, clb, cf = _hook(w, tok, nt, allow, R)
    assert (table[~has] == NONE).all() and (table[has] != NONE).all()
    lb = table.view(np.float32)
    slack = s.astype(np.float64) - lb
    worst = float((slack[has] / _tightness(w, tok, nt, s)[has]).max()) if has.any() else 0.0
    print(f"dim {dim} T {T} {kind}: largest (score - lb) / bound = {worst:.3f}")
    assert (lb[has] <= s[has]).all() and worst <= 1.0
    _check_candidates(table, has, ukeys, R, ck, clb, cf)
    # 2. the answer
    k = 10
    got = ix.search_maxsim(tok, k, n_tokens=nt, candidates="all", rescore=R, **kw)
    if dim != 24:
        assert has.sum(1).max() < R and same_bytes(got, _all_keys_model(w, tok, nt, allow, k)) and (got[5] == got[4]).all()
    else:
        want = _all_keys_model(w, tok, nt, allow, k)
        for q in range(n):
            c = got[5][q]
            assert all(g[q, :c].tobytes() == m[q, :c].tobytes() for g, m in zip(got[:4], want[:4])) and got[4][q] == want[4][q]
            if has[q].sum() < R:
                assert c == got[4][q]
                continue
            # the fixture, not the kernel: the R-th smallest score less the bound clears at least k scores (the tokens sit
            # 0.3 sigma from rows of the index, so a query's best documents score far below its 1,024th; seed 9100 + dim)
            sq = np.sort(s[q][has[q]].astype(np.float64))
            limit = sq[R - 1] - _tightness(w, tok, nt, s)[q][has[q]].max()
            c_i = int((sq < limit).sum())
            assert c_i >= k and c >= min(k, c_i)
    made = kw.get("filter", [])
    for f in made if isinstance(made, list) else [made]:
        f.close()


def test_streaming_selection_and_unbounded_query(cph):
    """2,600 keys against a select buffer of 2,048 words: the cuts inside the stream and the threshold run (with 1,490 keys
    only the final cut does).  Then a token whose squared norm overflows: that query's bounds are +0 for every key, its
    candidates the R smallest keys, certified 0; the other queries keep their bytes."""
    w = _world(cph, 10, singles=True)
    tok, nt = _tokens(w, 3, 5, seed=5)
    allow = np.ones((5, N), bool)
    ukeys, s = _scores(w, tok, nt, allow)
    table, ck, clb, cf = _hook(w, tok, nt, allow, 1024)
    assert (table.view(np.float32) <= s).all() and (cf == 1024).all()
    _check_candidates(table, np.ones_like(table, bool), ukeys, 1024, ck, clb, cf)
    bad = tok.copy()
    bad[4, 0, 0] = np.float32(3e38)
    table2, ck2, clb2, cf2 = _hook(w, bad, nt, allow, 1024)
    assert table2[:4].tobytes() == table[:4].tobytes() and ck2[:4].tobytes() == ck[:4].tobytes() and (table2[4] == 0).all()
    assert (ck2[4] == ukeys[:1024]).all() and (clb2[4] == 0).all() and cf2[4] == 1024
    got = w["ix"].search_maxsim(bad, 10, n_tokens=nt, candidates="all", rescore=1024)
    assert got[5][4] == 0 and (got[5][:4] == 10).all()


def test_plumbing(cph):
    import torch
    w = _world(cph, 10)
    ix = w["ix"]
    tok, nt = _tokens(w, 3, 6, seed=1)
    host = ix.search_maxsim(tok, 10, n_tokens=nt, candidates="all", rescore=128)
    side = torch.cuda.Stream()
    dev = ix.search_maxsim_device(torch.from_numpy(tok).cuda(), 10, n_tokens=nt, candidates="all", rescore=128, stream=side)
    side.synchronize()
    assert same_bytes(tuple(t.cpu().numpy() for t in dev), host)
    assert same_bytes(ix.search_maxsim(tok, 10, n_tokens=nt, candidates="all"), ix.search_maxsim(tok, 10, n_tokens=nt, candidates="all", rescore=64))
    lab = w["key_of"][:6].copy()
    filt = [ix.make_filter(w["key_of"] == v, ids="internal") for v in lab]
    assert same_bytes(ix.search_maxsim(tok, 10, n_tokens=nt, candidates="all", rescore=128, label=lab),
                      ix.search_maxsim(tok, 10, n_tokens=nt, candidates="all", rescore=128, filter=filt, filter_of=np.arange(6)))
    ix.result_ids = "input"
    try:
        mapped = ix.search_maxsim(tok, 10, n_tokens=nt, candidates="all", rescore=128)
    finally:
        ix.result_ids = "internal"
    rows = np.concatenate([ix.row_map(), np.arange(N, ix.size)])
    assert same_bytes(mapped[:3] + mapped[4:], host[:3] + host[4:]) and (mapped[3] == np.where(host[3] < 0, -1, rows[host[3]])).all()
    with pytest.raises(ValueError):
        ix.search_maxsim(tok, 10, candidates="every")


def test_cosine_equals_l2_over_normalised_rows(cph):
    wc = _world(cph, 10, cosine=True)
    tok, nt = _tokens(wc, 3, 5, seed=2, ragged=False)      # (the cosine model of the tests takes no rows without a direction)
    got = wc["ix"].search_maxsim(tok, 10, n_tokens=nt, candidates="all", rescore=128)
    assert same_bytes(got, _all_keys_model(wc, tok, nt, np.ones((5, N), bool), 10, cosine=True)) and (got[5] == got[4]).all()


def test_refusals(cph):
    rng = np.random.default_rng(3)
    X = rng.standard_normal((600, 10)).astype(np.float32)
    tok = X[:6].reshape(2, 3, 10)
    ip = cph.CPIndex(10, 4, metric="ip")
    ip.build(X)
    ip.finalize()
    ip.set_labels(np.arange(600) // 7, ids="internal")
    with pytest.raises(ValueError, match="inner-product"):
        ip.search_maxsim(tok, 5, candidates="all")
    parts = cph.CPIndex(10, 4, devices=[0, 0], partition=True)
    parts.build(X)
    parts.finalize()
    with pytest.raises(ValueError, match="partitioned"):
        parts.search_maxsim(tok, 5, candidates="all")


def test_two_replicas_equal_one(cph):
    rng = np.random.default_rng(4)
    X = rng.standard_normal((900, 24)).astype(np.float32)
    tok = (X[rng.integers(0, 900, (7, 4))] + np.float32(0.2)).astype(np.float32)
    outs = []
    for devices in (None, [0, 0]):                            # (two replicas on one device: the fan-out is the same)
        ix = cph.CPIndex(24, 4) if devices is None else cph.CPIndex(24, 4, devices=devices)
        ix.build(X)
        ix.finalize()
        ix.set_labels(np.arange(900) // 11, ids="input")
        outs.append(ix.search_maxsim(tok, 10, candidates="all", rescore=128))
    assert same_bytes(*outs)
