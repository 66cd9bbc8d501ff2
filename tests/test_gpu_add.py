"""Added rows on the GPU (CPIndex.add / tail_size; cph_add): a tail of flat fp32 rows behind the graph.

The model of a graph-routed search on an index with a tail: row i = the first k entries of the stable merge of G_i, the
row the call returns without the tail (taken on the same handle BEFORE the add, or on an untouched twin of the same
file), and T_i, the exact top-k of the allowed tail rows, ascending by (distance bits, id).  The tail distances do not
come from the library: a helper index is built here from [64 filler rows; A], saved, opened with the oracle
(oracle/cph_oracle.cpp), and exact_l2(q, id of A_j) is taken there -- the builder gives A_j the norm cph_add must give
it, the oracle the dot.  No tolerance anywhere: ids and distance bytes must be equal."""
import ctypes as C
import zlib

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path, sift_like
from tail_model import FMAX, FOLD_KS, FOLD_PS, fold_case

pytestmark = pytest.mark.gpu

KS = (1, 10, 100, 550, 1024)
TAILS = (1, 63, 64, 65, 200)              # around the 64-lane block of the scan


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _load(cph, name, bits):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits))
    return ix


def _rows_like(name, rng, m):
    s = DATASETS[name]
    if s["kind"] == "sift":
        return sift_like(rng, m, s["dim"])
    return rng.standard_normal((m, s["dim"])).astype(np.float32)


def oracle_tail_dist(cph, oracle, dim, bits, A, Q, tmp):
    """float32 [nq][t]: exact_l2(Q_i, A_j) as the ORACLE computes it on a helper index built from [64 filler rows; A]."""
    rng = np.random.default_rng(len(A) * 1000 + dim)
    base = np.concatenate([rng.standard_normal((64, dim)).astype(np.float32) * np.float32(3.0), A])
    hx = cph.CPIndex(dim, bits)
    hx.build(base)
    hx.finalize()
    path = str(tmp / f"helper_{dim}_{bits}_{len(A)}.idx")
    hx.save(path)
    id_of_row = np.argsort(hx.row_map())
    assert np.array_equal(hx.get_vectors()[id_of_row[64:]], A)
    oi = oracle.load(path)
    return np.stack([oi.exact_l2(q, id_of_row[64:]) for q in Q])


def fold(g_ids, g_dist, t_dist, t_ids, allowed, k):
    """The model: g_* [nq][k]; t_dist [nq][t] of the tail ids t_ids [t]; allowed: bool [t]."""
    out_i, out_d = np.empty_like(g_ids), np.empty_like(g_dist)
    for q in range(len(g_ids)):
        d, i = t_dist[q][allowed], t_ids[allowed]
        order = np.lexsort((i, d.view(np.uint32)))[:k]             # (distance bits, id)
        cat_d, cat_i = np.concatenate([g_dist[q], d[order]]), np.concatenate([g_ids[q], i[order]])
        pick = np.argsort(cat_d, kind="stable")[:k]
        out_i[q], out_d[q] = cat_i[pick], cat_d[pick]
    return out_i, out_d


def _stats(ix, nq):
    return ix.last_search_stats(), ix.last_query_expansions(nq)


# ---- 1. the fold kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", FOLD_PS)
@pytest.mark.parametrize("k", FOLD_KS)
def test_fold_kernel_equals_host_statement(cph, k, P):
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    g_ids, g_dist, pools, counts, C_ = fold_case(k, P, seed=k * 7 + P)
    n = len(g_ids)
    hi, hd = np.empty_like(g_ids), np.empty_like(g_dist)
    _lib.check(L.cph_host_tail_fold(g_ids.ctypes.data, g_dist.ctypes.data, n, k, pools.ctypes.data, counts.ctypes.data, P, C_,
                                    hi.ctypes.data, hd.ctypes.data))
    di, dd = np.full_like(g_ids, -7), np.full_like(g_dist, -7.0)
    _lib.check(L.cph_tail_fold_hook(cph.index._default_device(), g_ids.ctypes.data, g_dist.ctypes.data, n, k, pools.ctypes.data,
                                    counts.ctypes.data, P, C_, di.ctypes.data, dd.ctypes.data))
    assert np.array_equal(di, hi) and _beq(dd, hd), (k, P)


# ---- 2. every fixture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(enumerate(DATASETS)), ids=lambda c: c[1])
def test_every_fixture_graph_route_equals_model(cph, oracle, gold, tmp_path, case):
    j, name = case
    bits, t = max(DATASETS[name]["bits"]), TAILS[j % len(TAILS)]
    A_ix, B_ix = _load(cph, name, bits), _load(cph, name, bits)          # B: the untouched twin, same calls in the same order
    nb = A_ix.size
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    A = _rows_like(name, rng, t)
    hits = min(4, t)
    Q = np.concatenate([gold[f"Q/{name}"], A[:hits]])                    # ... plus zero-distance hits on tail rows
    nq = len(Q)
    before = {}
    for k in KS:
        ids, d = A_ix.search_batch(Q, k)
        before[k] = (ids, d) + _stats(A_ix, nq)
        B_ix.search_batch(Q, k)
    new = A_ix.add(A)
    assert np.array_equal(new, np.arange(nb, nb + t)) and A_ix.size == nb + t and A_ix.tail_size == t and B_ix.tail_size == 0
    T = oracle_tail_dist(cph, oracle, DATASETS[name]["dim"], bits, A, Q, tmp_path)
    assert _beq(np.stack([A_ix.exact_l2(q, new) for q in Q]), T)         # the scan's bytes are cph_exact_l2's: the oracle's
    for k in KS:
        g_ids, g_d, st0, work0 = before[k]
        ids, d = A_ix.search_batch(Q, k)
        st, work = _stats(A_ix, nq)
        bi, bd = B_ix.search_batch(Q, k)
        stb, workb = _stats(B_ix, nq)
        assert np.array_equal(bi, g_ids) and _beq(bd, g_d), (name, k)    # the twin is the handle before the add
        wi, wd = fold(g_ids, g_d, T, new, np.ones(t, bool), k)
        assert np.array_equal(ids, wi), (name, k)
        assert _beq(d, wd), (name, k)
        # the graph launch is the one a handle without a tail makes: its per-query work and every counter
        assert np.array_equal(work, work0) and np.array_equal(work, workb), (name, k)
        for key in st:
            if key == "kernel_us":
                continue
            grown = nq * t if key == "exact_l2" else 0
            assert st[key] == st0[key] + grown == stb[key] + grown, (name, k, key, st, st0, stb)
        for r in range(hits):                                            # a query that IS a tail row: that row leads the graph's
            assert ids[nq - hits + r, 0] == nb + r, (name, k)
    with pytest.raises(ValueError, match="compact"):
        A_ix.search_batch(Q, 1025)


@pytest.mark.parametrize("name", ("g16", "g1024"))
def test_filtered_tail_scan_generic_and_1024(cph, oracle, gold, tmp_path, name):
    """The tail scan's candidate source (the allowed bit of the effective filter) in the instantiations the `built` index
    (D = 128) does not reach: the generic one (g16) and <1024, 64> (g1024).  65 tail rows: one past the 64-lane block."""
    bits, t = max(DATASETS[name]["bits"]), 65
    A_ix, B_ix = _load(cph, name, bits), _load(cph, name, bits)          # B: the untouched twin
    nb = A_ix.size
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 1)
    A = _rows_like(name, rng, t)
    Q = gold[f"Q/{name}"]
    new = A_ix.add(A)
    assert np.array_equal(new, np.arange(nb, nb + t))
    T = oracle_tail_dist(cph, oracle, DATASETS[name]["dim"], bits, A, Q, tmp_path)
    M = rng.random(nb + t) < 0.5                                         # internal ids
    no_tail = M.copy()
    no_tail[nb:] = False
    assert M[nb:].any() and not M[nb:].all() and M[:nb].any()
    for where, mask in (("mask", M), ("no tail row allowed", no_tail)):
        fa, fb = A_ix.make_filter(mask), B_ix.make_filter(mask[:nb])
        for k in (1, 100):
            g_ids, g_d = B_ix.search_batch(Q, k, filter=fb)
            wi, wd = fold(g_ids, g_d, T, new, mask[nb:], k)
            ids, d = A_ix.search_batch(Q, k, filter=fa)
            assert A_ix.last_search_stats()["expansions"] > 0            # the graph route: the tail is scanned by its own kernel
            assert np.array_equal(ids, wi), (name, where, k)
            assert _beq(d, wd), (name, where, k)
            if not mask[nb:].any():                                      # the twin's rows
                assert np.array_equal(ids, g_ids) and _beq(d, g_d), (name, where, k)


# ---- 3. growth -------------------------------------------------------------------------------------------------------------
def test_growth_in_five_calls_equals_one_call(cph, gold):
    name, bits = "g16", 4
    Q = gold[f"Q/{name}"]
    rng = np.random.default_rng(16)
    steps = (1, 31, 32, 1000, 1200)         # crosses a bitmap word, a 2,048-id compaction block and two reallocations
    rows = _rows_like(name, rng, sum(steps))
    labs = rng.integers(0, 5, 300 + sum(steps)).astype(np.int32)

    def start():
        ix = _load(cph, name, bits)
        ix.set_row_map((np.arange(300) * 7 + 3) % 300)
        ix.set_labels(labs[:300], ids="internal")
        ix.remove([5, 299])
        return ix
    ix, done = start(), 0
    for m in steps:
        ids = ix.add(rows[done:done + m], labels=labs[300 + done:300 + done + m])
        assert np.array_equal(ids, np.arange(300 + done, 300 + done + m))
        done += m
        ix.remove([300 + done - 1])                                      # the newest row goes again: R grows with the tail
        twin = start()
        twin.add(rows[:done], labels=labs[300:300 + done])
        twin.remove(np.cumsum(steps)[:steps.index(m) + 1] + 299)
        assert ix.size == twin.size == 300 + done and ix.tail_size == done
        for kw in (dict(), dict(exact=True), dict(label=3), dict(label=3, exact=True)):
            a, b = ix.search_batch(Q, 10, **kw), twin.search_batch(Q, 10, **kw)
            assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]), (m, kw)
        assert _beq(ix.get_vectors(300, done), rows[:done]) and _beq(ix.get_vectors(), twin.get_vectors())
        assert np.array_equal(ix.row_map(), np.concatenate([(np.arange(300) * 7 + 3) % 300, np.arange(300, 300 + done)]))
        assert np.array_equal(ix.labels(ids="internal"), labs[:300 + done])
        assert np.array_equal(ix.labels(ids="input")[300:], labs[300:300 + done])
        want_removed = np.zeros(300 + done, bool)
        want_removed[[5, 299] + list(np.cumsum(steps)[:steps.index(m) + 1] + 299)] = True
        assert np.array_equal(ix.removed_mask(ids="internal"), want_removed)
        assert ix.live_count == 300 + done - int(want_removed.sum())


# ---- 4 .. 9 share one index built here ---------------------------------------------------------------------------------
NB, DIM, BITS, T = 2000, 128, 4, 300


@pytest.fixture(scope="module")
def built(cph, oracle, tmp_path_factory):
    """A 2,000 x 128 4-bit index built here and saved natively (every handle below loads that file: the same bytes), its
    rows X, the tail rows A, queries, and the oracle's tail distances."""
    tmp = tmp_path_factory.mktemp("add")
    rng = np.random.default_rng(2000)
    X = rng.standard_normal((NB, DIM)).astype(np.float32)
    A = rng.standard_normal((T, DIM)).astype(np.float32)
    Q = np.concatenate([rng.standard_normal((36, DIM)).astype(np.float32), A[:2], X[:2]])
    ix = cph.CPIndex(DIM, BITS)
    ix.build(X)
    ix.finalize()
    path = str(tmp / "base.cphn")
    ix.save_native(path)
    Tq = oracle_tail_dist(cph, oracle, DIM, BITS, A, Q, tmp)
    return dict(path=path, X=X, A=A, Q=Q, T=Tq, tmp=tmp)


def _open(cph, built, tail=True, labels=None):
    ix = cph.CPIndex(DIM, BITS)
    ix.load_native(built["path"])
    if labels is not None:
        ix.set_labels(labels[:NB], ids="internal")
    if tail:
        ix.add(built["A"], labels=None if labels is None else labels[NB:])
    return ix


def _check(built, A_ix, B_ix, allowed, k, where, a_kw, b_kw):
    """A_ix (with the tail) under a_kw against the model: B_ix (no tail) under b_kw, folded with the allowed tail rows;
    graph route and exact=True (exact: (distance bits, id) over all allowed ids -- base ids lie below tail ids, so the
    same fold of the base's exact row)."""
    Q, tids = built["Q"], np.arange(NB, NB + T)
    for exact in (False, True):
        g_ids, g_d = B_ix.search_batch(Q, k, exact=exact, **b_kw)
        wi, wd = fold(g_ids, g_d, built["T"], tids, allowed, k)
        ids, d = A_ix.search_batch(Q, k, exact=exact, **a_kw)
        assert np.array_equal(ids, wi), (where, k, exact)
        assert _beq(d, wd), (where, k, exact)
    return ids, d


def test_filters_removed_rows_and_id_spaces(cph, built):
    rng = np.random.default_rng(4)
    labs = rng.integers(0, 4, NB + T).astype(np.int32)
    A_ix, B_ix = _open(cph, built, labels=labs), _open(cph, built, tail=False, labels=labs)
    old = B_ix.make_filter(np.ones(NB, bool))
    rm = B_ix.row_map()                                                  # input row of every base id
    assert np.array_equal(A_ix.row_map(), np.concatenate([rm, np.arange(NB, NB + T)]))
    every = np.ones(T, bool)
    for k in (10, 100):
        _check(built, A_ix, B_ix, every, k, "unfiltered", {}, {})
        M = rng.random(NB + T) < 0.5                                      # internal ids
        _check(built, A_ix, B_ix, M[NB:], k, "mask", dict(filter=A_ix.make_filter(M)), dict(filter=B_ix.make_filter(M[:NB])))
        Mr = rng.random(NB + T) < 0.3                                     # input rows: bit r < NB is base id argsort(rm)[r]
        _check(built, A_ix, B_ix, Mr[NB:], k, "mask, input rows", dict(filter=A_ix.make_filter(Mr, ids="input")),
               dict(filter=B_ix.make_filter(Mr[:NB], ids="input")))
        _check(built, A_ix, B_ix, labs[NB:] == 2, k, "label", dict(label=2), dict(label=2))
        only_tail = np.zeros(NB + T, bool)
        only_tail[NB + 7:NB + 12] = True
        ids, d = _check(built, A_ix, B_ix, only_tail[NB:], k, "tail only", dict(filter=A_ix.make_filter(only_tail)),
                        dict(filter=B_ix.make_filter(np.zeros(NB, bool))))
        assert (np.sort(ids[:, :5], axis=1) == np.arange(NB + 7, NB + 12)).all() and (ids[:, 5:] == -1).all() and (d[:, 5:] == FMAX).all()
    A_ix.result_ids = B_ix.result_ids = "input"
    _check(built, A_ix, B_ix, every, 10, "input rows", {}, {})
    Mr = rng.random(NB + T) < 0.4
    _check(built, A_ix, B_ix, Mr[NB:], 10, "input rows, mask", dict(filter=A_ix.make_filter(Mr)), dict(filter=B_ix.make_filter(Mr[:NB])))
    A_ix.result_ids = B_ix.result_ids = "internal"
    with pytest.raises(ValueError, match=rf"filter covers {NB} ids, the index holds {NB + T}"):
        A_ix.search_batch(built["Q"], 10, filter=old)
    # removed rows, base and tail
    R = np.zeros(NB + T, bool)
    R[rng.choice(NB, 200, replace=False)] = True
    R[NB + rng.choice(T, 60, replace=False)] = True
    assert A_ix.remove(np.flatnonzero(R)) == 260 and A_ix.live_count == NB + T - 260
    assert np.array_equal(A_ix.removed_mask(), R)
    notR = B_ix.make_filter(~R[:NB])
    M = rng.random(NB + T) < 0.5
    for k in (10, 100):
        _check(built, A_ix, B_ix, ~R[NB:], k, "removed", {}, dict(filter=notR))
        _check(built, A_ix, B_ix, (M & ~R)[NB:], k, "removed, mask", dict(filter=A_ix.make_filter(M)),
               dict(filter=B_ix.make_filter((M & ~R)[:NB])))
        _check(built, A_ix, B_ix, ((labs == 1) & ~R)[NB:], k, "removed, label", dict(label=1),
               dict(filter=B_ix.make_filter(((labs == 1) & ~R)[:NB])))
    # every tail row removed: the rows from before the add
    C_ix = _open(cph, built)
    g = B_ix.search_batch(built["Q"], 10)
    assert C_ix.remove(np.arange(NB, NB + T)) == T
    got = C_ix.search_batch(built["Q"], 10)
    assert np.array_equal(got[0], g[0]) and _beq(got[1], g[1])


# ---- 5. twins ----------------------------------------------------------------------------------------------------------------
def test_twins_of_base_rows(cph, built):
    X, Q = built["X"], built["Q"]
    ix = cph.CPIndex(DIM, BITS)
    ix.load_native(built["path"])
    base_id = np.argsort(ix.row_map())[:40]                               # internal id of input rows 0..39
    new = ix.add(X[:40])
    for q in Q:
        assert _beq(ix.exact_l2(q, base_id), ix.exact_l2(q, new))         # the distance BITS of the base row
    for j in (0, 17, 39):
        ids, d = ix.search_batch(Q, 2, filter=ix.make_filter(np.array([base_id[j], new[j]])), exact=True)
        assert (ids == [base_id[j], new[j]]).all() and _beq(d[:, 0], d[:, 1])
        ids, d = ix.search_batch(X[j][None, :], 8)                         # the graph route: the graph's entry first
        dups = int((ids[0] == base_id[j]).sum())                           # (the graph search may report an id in two slots)
        assert 1 <= dups < 8 and (ids[0, :dups] == base_id[j]).all() and ids[0, dups] == new[j], (j, ids)
        assert _beq(d[0, :dups], np.repeat(d[0, dups], dups)), (j, d)


# ---- 6. exact paths ------------------------------------------------------------------------------------------------------
def test_exact_threshold_range_and_per_query_filters(cph, built):
    rng = np.random.default_rng(6)
    A_ix, B_ix = _open(cph, built), _open(cph, built, tail=False)
    Q, Tq, tids = built["Q"], built["T"], np.arange(NB, NB + T)
    nq, k = len(Q), 10
    M = rng.random(NB + T) < 0.2
    c = int(M.sum())
    fa, fb = A_ix.make_filter(M), B_ix.make_filter(M[:NB])
    for thr, scanned in ((c, True), (c - 1, False)):                      # compared with |E| over ALL ids
        A_ix.exact_threshold = thr
        g = B_ix.search_batch(Q, k, filter=fb, exact=scanned)
        wi, wd = fold(g[0], g[1], Tq, tids, M[NB:], k)
        ids, d = A_ix.search_batch(Q, k, filter=fa)
        assert (A_ix.last_search_stats()["expansions"] == 0) == scanned
        assert np.array_equal(ids, wi) and _beq(d, wd), thr
    A_ix.exact_threshold = 0
    # exact range search: every allowed id below the radius, tail ids included, by (distance bits, id)
    radius = np.float32(np.median(Tq))
    lb, ib, db = B_ix.range_search(Q, radius, filter=fb)
    la, ia, da = A_ix.range_search(Q, radius, filter=fa)
    for q in range(nq):
        hit = M[NB:] & (Tq[q] < radius)
        wi = np.concatenate([ib[lb[q]:lb[q + 1]], tids[hit]])
        wd = np.concatenate([db[lb[q]:lb[q + 1]], Tq[q][hit]])
        order = np.lexsort((wi, wd.view(np.uint32)))
        assert np.array_equal(ia[la[q]:la[q + 1]], wi[order]) and _beq(da[la[q]:la[q + 1]], wd[order]), q
    assert A_ix.last_search_stats()["exact_l2"] == 2 * nq * c
    # the graph route of the range search: the cut of the folded rows
    K = 40
    rows_i, rows_d = A_ix.search_batch(Q, K, filter=fa)
    la, ia, da = A_ix.range_search(Q, radius, filter=fa, exact=False, max_results=K)
    for q in range(nq):
        keep = (rows_i[q] >= 0) & (rows_d[q] < radius)
        assert np.array_equal(ia[la[q]:la[q + 1]], rows_i[q][keep]) and _beq(da[la[q]:la[q + 1]], rows_d[q][keep]), q
    # per-query filters: scanned queries are served, a query for the graph is not
    M2 = rng.random(NB + T) < 0.6
    fo = rng.integers(-1, 2, nq).astype(np.int32)
    fo[:3] = (-1, 0, 1)
    ids, d = A_ix.search_batch(Q, k, filter=[fa, A_ix.make_filter(M2)], filter_of=fo, exact=True)
    for f, mask in ((-1, np.ones(NB + T, bool)), (0, M), (1, M2)):
        g = B_ix.search_batch(Q, k, filter=B_ix.make_filter(mask[:NB]), exact=True)
        wi, wd = fold(g[0], g[1], Tq, tids, mask[NB:], k)
        assert np.array_equal(ids[fo == f], wi[fo == f]) and _beq(d[fo == f], wd[fo == f]), f
    with pytest.raises(NotImplementedError, match="compact"):
        A_ix.search_batch(Q, k, filter=[fa, A_ix.make_filter(M2)], filter_of=fo)
    A_ix.exact_threshold = NB + T                                          # every filter scanned, but -1 still walks the graph
    with pytest.raises(NotImplementedError, match="compact"):
        A_ix.search_batch(Q, k, filter=[fa, A_ix.make_filter(M2)], filter_of=fo)
    fo01 = np.where(fo < 0, 0, fo).astype(np.int32)
    ids, d = A_ix.search_batch(Q, k, filter=[fa, A_ix.make_filter(M2)], filter_of=fo01)
    ide, de = A_ix.search_batch(Q, k, filter=[fa, A_ix.make_filter(M2)], filter_of=fo01, exact=True)
    assert np.array_equal(ids, ide) and _beq(d, de)


# ---- 7. device entry and rotation ----------------------------------------------------------------------------------------
def test_device_entry_two_streams_and_single_query(cph, built):
    import torch
    A_ix, B_ix = _open(cph, built), _open(cph, built, tail=False)
    A_ix.set_batch_sets(2)
    dev = f"cuda:{A_ix.devices[0]}"
    rng = np.random.default_rng(7)
    Q8 = built["Q"][:8]
    Q100 = np.concatenate([built["Q"], rng.standard_normal((60, DIM)).astype(np.float32)])
    assert len(Q100) == 100
    # 100 queries leave the small-batch path: D = 128 at 4 bits is the probe-first launch, and the batch stays on it --
    # every counter (the stage-2 ones among them) and the per-query work are those of the handle without a tail
    A_ix.search_batch(Q100, 10)
    sa, wa = _stats(A_ix, 100)
    B_ix.search_batch(Q100, 10)
    sb, wb = _stats(B_ix, 100)
    assert np.array_equal(wa, wb) and sa["exact_l2"] == sb["exact_l2"] + 100 * T
    assert {k: v for k, v in sa.items() if k not in ("exact_l2", "kernel_us")} == {k: v for k, v in sb.items() if k not in ("exact_l2", "kernel_us")}
    M = rng.random(NB + T) < 0.5
    f = A_ix.make_filter(M)
    for kw in (dict(), dict(filter=f)):
        want8, want100 = A_ix.search_batch(Q8, 10, **kw), A_ix.search_batch(Q100, 10, **kw)
        d8, d100 = torch.from_numpy(Q8).to(dev), torch.from_numpy(Q100).to(dev)
        s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        torch.cuda.synchronize(dev)
        r100 = A_ix.search_batch_device(d100, 10, stream=s1, **kw)       # two batches in flight on two streams
        r8 = A_ix.search_batch_device(d8, 10, stream=s2, **kw)
        r100b = A_ix.search_batch_device(d100, 10, stream=s2, **kw)
        A_ix.synchronize()
        torch.cuda.synchronize(dev)
        for got, want in ((r8, want8), (r100, want100), (r100b, want100)):
            assert np.array_equal(got[0].cpu().numpy(), want[0]) and _beq(got[1].cpu().numpy(), want[1]), kw
    rows_i, rows_d = A_ix.search_batch(built["Q"], 10)
    for q in (0, 36, 39):                                                 # 36: a zero-distance hit on a tail row
        ids, d = A_ix.search(built["Q"][q], 10)
        m = int((rows_i[q] >= 0).sum())
        assert np.array_equal(ids, rows_i[q, :m]) and _beq(d, rows_d[q, :m]), q
    assert rows_i[36, 0] == NB


# ---- 8. compact() ----------------------------------------------------------------------------------------------------------
def test_compact_folds_the_tail_into_a_new_graph(cph, built):
    rng = np.random.default_rng(8)
    labs = rng.integers(0, 4, NB + T).astype(np.int32)
    A_ix = _open(cph, built, labels=labs)
    A_ix.result_ids = "input"
    R = np.zeros(NB + T, bool)                                            # in input rows
    R[rng.choice(NB, 100, replace=False)] = True
    R[NB + rng.choice(T, 30, replace=False)] = True
    A_ix.remove(np.flatnonzero(R))
    Q, k = built["Q"], 10
    before_i, before_d = A_ix.search_batch(Q, k, exact=True)              # (pinned against the model in the tests above)
    labs_by_row = labs.copy()
    labs_by_row[A_ix.row_map()[:NB]] = labs[:NB]                          # (_open set the base labels in internal ids)
    live = NB + T - 130
    old_to_new = A_ix.compact()
    assert A_ix.size == A_ix.live_count == live and A_ix.tail_size == 0 and A_ix.result_ids == "input"
    assert old_to_new.shape == (NB + T,) and (old_to_new[R] == -1).all()
    assert np.array_equal(old_to_new[~R], np.arange(live))                # a bijection that keeps the input-row order
    assert np.array_equal(A_ix.labels(), labs_by_row[~R])                 # labels follow the rows
    rows = np.concatenate([built["X"], built["A"]])[~R]
    assert _beq(A_ix.get_vectors()[np.argsort(A_ix.row_map())], rows)
    ids, d = A_ix.search_batch(Q, k, exact=True)
    assert np.array_equal(ids, np.where(before_i >= 0, old_to_new[np.maximum(before_i, 0)], -1)) and _beq(d, before_d)
    p = str(built["tmp"] / "compacted.cphn")
    A_ix.save_native(p)                                                   # works again
    A_ix.save(str(built["tmp"] / "compacted.idx"))
    A_ix.add(built["A"][:3], labels=[1, 2, 3])                            # ... and the index takes rows again
    assert A_ix.tail_size == 3 and A_ix.size == live + 3


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals(cph, built):
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    A_ix = _open(cph, built)
    with pytest.raises(RuntimeError, match="compact"):
        A_ix.save(str(built["tmp"] / "no.idx"))
    with pytest.raises(RuntimeError, match="compact"):
        A_ix.save_native(str(built["tmp"] / "no.cphn"))
    with pytest.raises(ValueError, match="compact"):
        A_ix.set_row_map(np.arange(NB + T))
    with pytest.raises(ValueError, match="compact"):
        A_ix.set_row_map(None)
    with pytest.raises(ValueError, match="no label column"):
        A_ix.add(built["A"][:2], labels=[1, 2])
    with pytest.raises(ValueError):
        A_ix.add(built["A"][:2, :5])
    with pytest.raises(ValueError, match="vertex out of range"):
        A_ix.fastscan_block(np.zeros((DIM // 4, 16), np.uint8), np.ones(7, np.float32), NB, 1.0)
    blk = np.zeros(1 << 16, np.uint8)
    assert L.cph_export_blocks(A_ix._h, NB, 1, 0, blk.ctypes.data) == _lib.INVALID_ARGUMENT
    # add of 0 rows changes nothing
    ref = A_ix.search_batch(built["Q"], 10)
    assert A_ix.add(np.zeros((0, DIM), np.float32)).size == 0 and A_ix.size == NB + T and A_ix.tail_size == T
    got = A_ix.search_batch(built["Q"], 10)
    assert np.array_equal(ref[0], got[0]) and _beq(ref[1], got[1])
    # a label column asks for labels
    Lx = _open(cph, built, tail=False, labels=np.zeros(NB + T, np.int32))
    with pytest.raises(ValueError, match="need labels"):
        Lx.add(built["A"][:2])
    with pytest.raises(ValueError):
        Lx.add(built["A"][:2], labels=[1, 2, 3])
    assert Lx.tail_size == 0 and Lx.size == NB
    # before finalize
    fresh = cph.CPIndex(DIM, BITS)
    with pytest.raises(ValueError, match="finalized"):
        fresh.add(built["A"][:2])
    fresh.build(built["X"][:100])
    with pytest.raises(ValueError, match="finalized"):
        fresh.add(built["A"][:2])
    # replicas, parts, borrowed handles
    dev = A_ix.devices[0]
    multi = cph.CPIndex(DIM, BITS, devices=[dev, dev])
    multi.load_native(built["path"])
    with pytest.raises(NotImplementedError):
        multi.add(built["A"][:2])
    first = C.c_int64(-1)
    v = np.ascontiguousarray(built["A"][:2])
    assert L.cph_add(multi._reps[0], v.ctypes.data, 2, None, C.byref(first)) == _lib.INVALID_ARGUMENT      # a borrowed replica
    assert multi.size == NB
    parts = cph.CPIndex(DIM, BITS, devices=[dev, dev], partition=True)
    parts.build(built["X"][:400])
    parts.finalize()
    with pytest.raises(NotImplementedError):
        parts.add(built["A"][:2])
    with pytest.raises(NotImplementedError):
        parts.part(0).add(built["A"][:2])
    assert L.cph_add(parts._part_handles[0], v.ctypes.data, 2, None, C.byref(first)) == _lib.INVALID_ARGUMENT
    assert parts.size == 400
