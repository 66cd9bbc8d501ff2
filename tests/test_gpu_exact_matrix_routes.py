"""Every route INTEGRATION.md sends through the exact scan, under the matrix engine (index.exact_engine = "matrix"): each
call runs under both engines on one handle and every returned array must have the vector engine's bytes; the batch must
have gone through the matrix launches (matrix_parts > 0) and been certified there (matrix_redo == 0: no scenario here
is built on duplicates, except the twin of a base row, whose pair fits any pool).  Where a route's rows have a plain
model -- the ORACLE's exact_l2 on the file, or the library's distance hook exact_l2 for rows no file holds -- they are
compared with it as well; cosine and inner product against the oracle on their L2 twin; each re-ranker against the model
of its own test file.

And bn_max, the one number of the engine no output byte shows: a stale value that is too small never changes a result, it
only voids the proof.  cph_debug_matrix_bn_max against the largest float64 row norm after every change of the index."""
import ctypes as C

import numpy as np
import pytest

from golden_util import fixture_path
from exact_matrix_model import DEFAULT_BUDGET_MB, U, may_flag, plan, slack_of
from test_gpu_exact import _all_distances, _allowed, _beq, _load, _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _same(a, b):
    a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    return len(a) == len(b) and all(np.asarray(x).shape == np.asarray(y).shape and np.asarray(x).tobytes() == np.asarray(y).tobytes()
                                    for x, y in zip(a, b))


def _both(ix, call, what, redo=0):
    """call() under the vector engine, then under the matrix engine: the same bytes, through the matrix launches."""
    ix.exact_engine = "vector"
    want = call()
    assert "matrix_parts" not in ix.last_search_stats(), what
    ix.exact_engine = "matrix"
    got = call()
    st = ix.last_search_stats()
    assert _same(got, want), what
    assert st.get("matrix_parts", 0) > 0, (what, st)
    if redo is not None:
        assert st["matrix_redo"] == redo, (what, st)
    return got


def _hook_model(ix, Q, allowed, k):
    """Rows from the library's own distance hook (rows of a tail or of another metric are in no file the oracle reads)."""
    return _model(np.stack([ix.exact_l2(q, allowed) for q in Q]), allowed, k)


def test_threshold_removed_rows_and_input_rows(cph, oracle, gold):
    ix = _load(cph, "g128", 4)
    oi = oracle.load(fixture_path("g128", 4))
    Q, n = gold["Q/g128"], ix.size
    rng = np.random.default_rng(31)
    mask = rng.random(n) < 0.4
    f = ix.make_filter(mask)
    # the cut-over of a filtered call that does not ask for the exact path
    ix.exact_threshold = f.count
    allowed = _allowed(mask, n)
    dist = _all_distances(oi, Q, allowed)
    for k in (1, 10, 100):
        ids, d = _both(ix, lambda: ix.search_batch(Q, k, filter=f), ("threshold", k))
        assert ix.last_search_stats()["expansions"] == 0
        want_ids, want_d = _model(dist, allowed, k)
        assert np.array_equal(ids, want_ids) and _beq(d, want_d), k
    ix.exact_threshold = 0
    # removed rows: the list is F & ~R, or ~R alone
    gone = rng.choice(n, 90, replace=False)
    ix.remove(gone)
    live = np.ones(n, bool)
    live[gone] = False
    for what, flt, m in (("removed", None, live), ("removed, filtered", f, live & mask)):
        allowed = _allowed(m, n)
        ids, d = _both(ix, lambda: ix.search_batch(Q, 10, filter=flt, exact=True), what)
        want_ids, want_d = _model(_all_distances(oi, Q, allowed), allowed, 10)
        assert np.array_equal(ids, want_ids) and _beq(d, want_d), what
    # result_ids = "input": the certify kernel's row translation
    rx = cph.CPIndex(24, 4)
    X = np.random.default_rng(32).standard_normal((500, 24)).astype(np.float32)
    rx.build(X)
    rx.finalize()
    rm = rx.row_map()
    Q24 = X[:30] + np.float32(0.01)
    rx.result_ids = "input"
    ids, d = _both(rx, lambda: rx.search_batch(Q24, 10, exact=True), "input rows")
    rx.result_ids = "internal"
    want_ids, want_d = _hook_model(rx, Q24, _allowed(None, 500), 10)
    assert np.array_equal(ids, rm[want_ids]) and _beq(d, want_d)
    assert (ids[:, 0] == np.arange(30)).all()                      # query i is input row i, moved a little


def test_tail_rows_a_twin_and_compact(cph, oracle, gold, tmp_path):
    ix = _load(cph, "g128", 4)
    Q, n = gold["Q/g128"], ix.size
    rng = np.random.default_rng(41)
    X = ix.get_vectors()
    new = ix.add(np.concatenate([X[5:6], rng.standard_normal((70, 128)).astype(np.float32)]))   # a twin of id 5, then 70 rows
    size = n + 71
    assert ix.size == size and ix.tail_size == 71
    Qt = np.concatenate([Q, X[5:6], ix.get_vectors(n + 3, 2)])
    for k in (1, 10, 100):
        ids, d = _both(ix, lambda: ix.search_batch(Qt, k, exact=True), ("tail", k))
        want_ids, want_d = _hook_model(ix, Qt, _allowed(None, size), k)
        assert np.array_equal(ids, want_ids) and _beq(d, want_d), k
    ids, d = ix.search_batch(Qt, 2, exact=True)
    assert ids[24].tolist() == [5, int(new[0])] and d[24, 0] == d[24, 1]          # the twin ties with its base row, ids ascending
    assert ids[25, 0] == n + 3 and ids[26, 0] == n + 4
    mask = rng.random(size) < 0.3
    mask[new[:3]] = True
    ids, d = _both(ix, lambda: ix.search_batch(Qt, 10, filter=ix.make_filter(mask), exact=True), "tail, filtered")
    want_ids, want_d = _hook_model(ix, Qt, _allowed(mask, size), 10)
    assert np.array_equal(ids, want_ids) and _beq(d, want_d)
    # compact(): a new graph over the live rows; the oracle reads its file
    ix.remove(np.arange(0, size, 7))
    ix.compact()
    assert ix.tail_size == 0 and ix.exact_engine == "matrix"
    p = str(tmp_path / "compacted.idx")
    ix.save(p)
    oi = oracle.load(p)
    allowed = _allowed(None, ix.size)
    ids, d = _both(ix, lambda: ix.search_batch(Qt, 10, exact=True), "compacted")
    want_ids, want_d = _model(_all_distances(oi, Qt, allowed), allowed, 10)
    assert np.array_equal(ids, want_ids) and _beq(d, want_d)


def _built(cph, dim, rows, **kw):
    ix = cph.CPIndex(dim, 4, **kw)
    ix.build(rows)
    ix.finalize()
    return ix


@pytest.mark.parametrize("metric,dim", (("cosine", 24), ("ip", 16)))
def test_other_metrics(cph, oracle, metric, dim, tmp_path):
    """Cosine at dim 24 and inner product at dim 16 (one coordinate more: D = pad(17) = 32), against the L2 twin of
    tests/test_gpu_cosine.py and tests/test_gpu_ip.py: a plain index B built from the rows the metric's model stores
    (cosine_model.model, ip_model.model), asked with the model's queries.  The expected rows are the ORACLE's on B's file --
    every id and every distance byte, at k = 1, 10 and 100, with and without a filter; for the inner product the distance
    bytes go through ip_model.epilogue_model."""
    import cosine_model
    import ip_model
    rng = np.random.default_rng(51)
    n = 700
    X = (rng.standard_normal((n, dim)) * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32)
    Q = (rng.standard_normal((40, dim)) * rng.uniform(0.5, 2.0, (40, 1))).astype(np.float32)
    if metric == "cosine":
        mX, mQ, c = cosine_model.model(X), cosine_model.model(Q), None
    else:
        m2 = ip_model.max_model(X)
        mX = ip_model.model(X)
        mQ, c, _ = ip_model.queries_model(Q, m2)
    A = _built(cph, dim, X, metric=metric)
    B = _built(cph, mX.shape[1], mX)
    # the builder is reproducible: A stores B's rows under B's ids
    assert np.array_equal(A.row_map(), B.row_map()) and _beq(A.get_vectors(stored=True), B.get_vectors())
    p = str(tmp_path / "twin.idx")
    B.save(p)
    oi = oracle.load(p)
    mask = rng.random(n) < 0.5
    f = A.make_filter(mask, ids="internal")
    D = 32
    eps = slack_of(mQ, mX, D)
    for m, flt in ((None, None), (mask, f)):
        allowed = _allowed(m, n)
        dist = _all_distances(oi, mQ, allowed)
        for k in (1, 10, 100):
            # (the reference's verdict first: no query of this input may need the fallback)
            assert not may_flag(dist, k, eps, plan(len(allowed), len(Q), k, DEFAULT_BUDGET_MB)).any(), ("bad input", metric, k)
            want_ids, want_d = _model(dist, allowed, k)
            if metric == "ip":
                want_d = ip_model.epilogue_model(want_ids, want_d, c)
            ids, d = _both(A, lambda: A.search_batch(Q, k, filter=flt, exact=True), (metric, k, m is not None))
            assert np.array_equal(ids, want_ids) and _beq(d, want_d), (metric, k, m is not None)


# ---- the re-rankers: each against the model of its own test file, over candidate rows of the vector engine ---------------
def _vector_expect(ix, expect):
    """A route's own statement of its result -- the _expect of its test file: the route's model over the candidate rows that
    search_batch(..., candidates, exact=True) returns on the same handle -- with those rows taken under the VECTOR engine,
    which tests/test_gpu_exact.py pins to the oracle."""
    ix.exact_engine = "vector"
    try:
        return expect()
    finally:
        ix.exact_engine = "matrix"


def _strict(got, want):
    return len(got) == len(want) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
                                         for x, y in zip(got, want))


def _variants(ix, seed):
    """With exact=True, over all rows and under a filter of 40 % of them; the mask of each."""
    mask = np.random.default_rng(seed).random(ix.size) < 0.4
    return ((dict(exact=True), np.ones(ix.size, bool)), (dict(filter=ix.make_filter(mask, ids="internal"), exact=True), mask))


def test_grouped(cph, gold):
    import test_gpu_grouped as t
    ix, Q = t._open(cph, gold, None, "g16", 1)
    key_of = t._keys_for(ix.size, ix.size)
    ix.set_labels(key_of, ids="internal")
    for kw, _ in _variants(ix, 61):
        for (k, g, C_) in ((3, 2, 17), (10, 3, 70)):
            want = _vector_expect(ix, lambda: t._expect(ix, Q, k, g, C_, key_of, **kw))
            got = _both(ix, lambda: ix.search_grouped(Q, k, g, candidates=C_, **kw), ("grouped", k, g, C_, sorted(kw)))
            assert t._same(got, want), (k, g, C_, sorted(kw))


def test_diverse(cph, gold):
    import test_gpu_diverse as t
    ix = _load(cph, "g128", 4)
    Q = gold["Q/g128"][:12]
    pairs = t.IndexPairs(ix)
    for kw, _ in _variants(ix, 62):
        for (k, lam, C_) in ((3, 0.3, 17), (10, 0.5, 70)):
            want = _vector_expect(ix, lambda: t._expect(ix, pairs, Q, k, lam, C_, **kw))
            got = _both(ix, lambda: ix.search_diverse(Q, k, lam, candidates=C_, **kw), ("diverse", k, lam, C_, sorted(kw)))
            assert _strict(got, want), (k, lam, C_, sorted(kw))


def _maxsim_scene(cph, gold):
    import test_gpu_maxsim as t
    ix, Q = t._open(cph, gold, None, "g16", 1)
    key_of = t._keys_for(ix.size, ix.size)
    ix.set_labels(key_of, ids="internal")
    return ix, Q, key_of


def _tokens(Q, nq, T, seed):
    """The tokens of tests/test_gpu_maxsim.py; its garbage rows (1e3, ignored by n_tokens, but scanned) are ordinary
    vectors here, as that file makes them for its every-token-live call: a query of that length is no Gaussian input."""
    import test_gpu_maxsim as t
    tok, n_tokens = t._tokens(Q, nq, T, seed)
    tok[-1, 1:] = tok[0, :T - 1]
    return tok, n_tokens


def test_maxsim(cph, gold):
    import test_gpu_maxsim as t
    ix, Q, key_of = _maxsim_scene(cph, gold)
    tok, n_tokens = _tokens(Q, 5, 3, ix.size + 3)
    for kw, _ in _variants(ix, 63):
        for k in (1, 10):
            want = _vector_expect(ix, lambda: t._expect(ix, tok, n_tokens, k, 65, key_of, **kw))
            got = _both(ix, lambda: ix.search_maxsim(tok, k, n_tokens=n_tokens, candidates=65, **kw), ("maxsim", k, sorted(kw)))
            assert _strict(got, want), (k, sorted(kw))


def test_maxsim_rescored(cph, gold):
    import test_gpu_maxsim_rescore as t
    ix, Q, key_of = _maxsim_scene(cph, gold)
    tok, n_tokens = _tokens(Q, 4, 9, ix.size + 9)
    for kw, allow in _variants(ix, 64):
        want = _vector_expect(ix, lambda: t._expect(ix, tok, n_tokens, 3, 24, 40, key_of, allow, **kw))
        got = _both(ix, lambda: ix.search_maxsim(tok, 3, n_tokens=n_tokens, candidates=40, rescore=24, **kw),
                    ("maxsim rescored", sorted(kw)))
        assert _strict(got, want), sorted(kw)


def test_fused(cph, gold):
    import test_gpu_fused as t
    ix, Q0 = t._open(cph, gold)
    Q = t._queries(Q0, t.N, t.T, ix.size)
    for kw, _ in _variants(ix, 65):
        for weights, nv in ((t.WEIGHTS, t.NV), (None, None)):
            want, _ = _vector_expect(ix, lambda: t._expect(ix, Q, t.K, t.C0, weights, nv, **kw))
            got = _both(ix, lambda: ix.search_fused(Q, t.K, weights=weights, n_vectors=nv, candidates=t.C0, **kw),
                        ("fused", weights is None, sorted(kw)))
            assert _strict(got, want), (weights is None, sorted(kw))


def test_two_stage_rescored(cph):
    import test_gpu_rescore as t
    ix = _load(cph, "g128", 4)
    full, FQ = t._prefix_data(ix, 200, 12, 7)
    Q = np.ascontiguousarray(FQ[:, :ix.dim])
    cases = (((10, 70), t._object_over(ix, full, "float16", "l2")), ((8, 130), t._object_over(ix, full, "float32", "ip")))
    for kw, _ in _variants(ix, 66):
        for (k, C_), obj in cases:
            want = _vector_expect(ix, lambda: t._expect(ix, obj, Q, FQ, k, C_, **kw))
            got = _both(ix, lambda: ix.search_rescored(Q, k, obj[0], full_queries=FQ, candidates=C_, **kw),
                        ("rescored", k, C_, sorted(kw)))
            assert _strict(got, want), (k, C_, sorted(kw))


def test_replicas_parts_and_views(cph, oracle, gold):
    """Replicas and a partitioned index (both on one device, as their own files run them), and part(i), which inherits the
    engine."""
    Q = gold["Q/g128"]
    ix = _load(cph, "g128", 4)
    n = ix.size
    mask = np.random.default_rng(71).random(n) < 0.5
    mx = _load(cph, "g128", 4, devices=[0, 0])
    mx.set_min_shard(8)
    for flt, mflt in ((None, None), (ix.make_filter(mask), mx.make_filter(mask))):
        want = ix.search_batch(Q, 10, filter=flt, exact=True)
        got = _both(mx, lambda: mx.search_batch(Q, 10, filter=mflt, exact=True), "replicas")
        assert _same(got, want)
    X = np.random.default_rng(72).standard_normal((900, 24)).astype(np.float32)
    Q24 = X[:40] + np.float32(0.02)
    px = cph.CPIndex(24, 4, devices=[0, 0], partition=True)
    px.build(X)
    px.finalize()
    pmask = np.random.default_rng(73).random(900) < 0.5
    for flt in (None, px.make_filter(pmask)):
        ids, d = _both(px, lambda: px.search_batch(Q24, 10, filter=flt, exact=True), "partitioned")
        rows = np.arange(900) if flt is None else np.flatnonzero(pmask)
        d64 = ((Q24[:, None, :].astype(np.float64) - X[rows][None].astype(np.float64)) ** 2).sum(2)
        assert (ids[:, 0] == rows[d64.argmin(1)]).all()              # query i is row i moved a little: far from any tie
    px.exact_engine = "matrix"
    v = px.part(1)
    assert v.exact_engine == "matrix"
    lo, hi = px.parts[1]
    ids, d = v.search_batch(Q24, 10, exact=True)
    st = v.last_search_stats()
    assert st["matrix_parts"] > 0 and st["matrix_redo"] == 0
    want_ids, want_d = _hook_model(v, Q24, _allowed(None, hi - lo), 10)
    assert np.array_equal(ids, v.row_map()[want_ids]) and _beq(d, want_d)


def _bn_max(ix):
    from cphnsw_mi355x import _lib
    out = C.c_float()
    _lib.check(_lib.lib().cph_debug_matrix_bn_max(ix._h, C.byref(out)))
    return float(out.value)


def _check_bn(ix, Q, D, rows, what):
    """One matrix batch on the handle's state, then bn_max against the largest float64 norm of `rows` (the stored rows):
    the stored norm is a float32 reduction of at most D terms, within gamma(D + 3) of the real one (device_exact_mfma.h)."""
    ix.search_batch(Q, 5, exact=True)
    assert ix.last_search_stats()["matrix_parts"] > 0
    want = float((np.asarray(rows, np.float64) ** 2).sum(1).max())
    g = (D + 3) * U / (1 - (D + 3) * U)
    got = _bn_max(ix)
    print(what, "bn_max", got, "float64", want)
    assert abs(got - want) <= g * want, (what, got, want)
    return got


def test_bn_max_follows_the_index_state(cph, tmp_path):
    rng = np.random.default_rng(81)
    X1 = rng.standard_normal((300, 10)).astype(np.float32)
    X2 = (0.5 * rng.standard_normal((300, 10))).astype(np.float32)
    Q = rng.standard_normal((8, 10)).astype(np.float32)
    paths = []
    for i, X in enumerate((X1, X2)):
        b = cph.CPIndex(10, 4)
        b.build(X)
        b.finalize()
        paths.append(str(tmp_path / f"bn{i}.idx"))
        b.save(paths[-1])
    ix = cph.CPIndex(10, 4)
    ix.load(paths[0])
    ix.exact_engine = "matrix"
    with pytest.raises(ValueError):
        _bn_max(ix)                                                  # no matrix batch has run on this state
    base = _check_bn(ix, Q, 16, X1, "fresh load")
    big = 10 * X1[(X1.astype(np.float64) ** 2).sum(1).argmax()]      # 100 times the largest norm
    new = ix.add(big[None, :])
    with pytest.raises(ValueError):
        _bn_max(ix)
    grown = _check_bn(ix, Q, 16, np.concatenate([X1, big[None, :]]), "after add")
    assert grown > 50 * base
    ix.remove(new)
    assert _check_bn(ix, Q, 16, np.concatenate([X1, big[None, :]]), "after remove: a tombstone keeps its norm") == grown
    ix.compact()
    assert ix.size == 300
    assert _check_bn(ix, Q, 16, X1, "after compact") == base
    ix.load(paths[1])                                                # another file, the same size()
    assert ix.size == 300
    assert _check_bn(ix, Q, 16, X2, "after load") < base
    ip = cph.CPIndex(16, 4, metric="ip")
    Xi = rng.standard_normal((300, 16)).astype(np.float32)
    ip.build(Xi)
    ip.finalize()
    ip.exact_engine = "matrix"
    stored = ip.get_vectors(stored=True)
    assert stored.shape[1] == 17
    m2 = _check_bn(ip, rng.standard_normal((8, 16)).astype(np.float32), 32, stored, "inner product: the bound M2")
    assert m2 >= float((Xi.astype(np.float64) ** 2).sum(1).max()) * (1 - 1e-6)


def test_first_use_from_two_streams(cph, gold):
    """A fresh handle, two device batches back to back on two streams with nothing between them: the first makes bn_max, the
    second uses it.  Both must have the host call's bytes.  (What this shows is that the second batch runs and is right
    beside the first one's reduction; that it WAITS for bn_max is not visible here -- a slack from a too-small bn_max
    almost never changes a byte -- and the value itself is test_bn_max_follows_the_index_state's.)"""
    import torch
    ix = _load(cph, "g128", 4)
    ix.exact_engine = "matrix"
    dev = torch.device("cuda", 0)
    Qa = torch.from_numpy(gold["Q/g128"]).to(dev)
    Qb = torch.from_numpy(np.ascontiguousarray(ix.get_vectors()[:200])).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    s1.wait_stream(torch.cuda.current_stream(dev))
    s2.wait_stream(torch.cuda.current_stream(dev))
    a_ids, a_d = ix.search_batch_device(Qa, 10, stream=s1, exact=True)
    b_ids, b_d = ix.search_batch_device(Qb, 10, stream=s2, exact=True)
    ix.synchronize()
    for (ids, d), Qh in (((a_ids, a_d), Qa), ((b_ids, b_d), Qb)):
        want_ids, want_d = ix.search_batch(Qh.cpu().numpy(), 10, exact=True)
        assert ix.last_search_stats()["matrix_redo"] == 0
        assert np.array_equal(ids.cpu().numpy(), want_ids) and _beq(d.cpu().numpy(), want_d)
    ix.exact_engine = "vector"
    want_ids, want_d = ix.search_batch(gold["Q/g128"], 10, exact=True)
    assert np.array_equal(a_ids.cpu().numpy(), want_ids) and _beq(a_d.cpu().numpy(), want_d)
