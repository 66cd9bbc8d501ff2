"""Per-query filters on the GPU: search_batch(q, k, filter=[...], filter_of=which) against the single-filter path it
replaces.  The yardstick is never the new code: for every case the expected rows come from one call of today's
search_batch(q[sel], k, filter=f, exact=...) per distinct filter (the plain call for the rows with -1), scattered back
into row order; ids and distance bytes of EVERY query must be equal.  Graph route, exact route (the grouped scan),
mixed routing with the statistics contract, input-row ids, the device entry, two replicas, the overflow re-run, errors."""
import ctypes as C

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

CASES = [(n, b, v) for n, s in DATASETS.items() for b in s["bits"] for v in s["variants"]]
KS = (1, 10, 100)


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _load(cph, name, bits, variant="plain", **kw):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits, **kw)
    ix.load(fixture_path(name, bits, variant))
    return ix


def _masks(n, seed):
    """The F = 6 filters of the issue: all ones, ~50 %, ~5 %, a handful, one id, empty."""
    rng = np.random.default_rng(seed)
    hand = np.zeros(n, bool)
    hand[rng.choice(n, 6, replace=False)] = True
    one = np.zeros(n, bool)
    one[int(rng.integers(0, n))] = True
    return [np.ones(n, bool), rng.random(n) < 0.5, rng.random(n) < 0.05, hand, one, np.zeros(n, bool)]


def _assign(nq, F, seed, lone=3, heavy=None):
    """filter_of at random: every filter and -1 occur, filter `lone` on exactly one query; `heavy`: a value that takes
    about 45 % of the queries."""
    rng = np.random.default_rng(seed)
    others = np.array([f for f in range(-1, F) if f != lone])
    fo = others[rng.integers(0, len(others), nq)]
    if heavy is not None:
        fo[rng.random(nq) < 0.45] = heavy
    spots = rng.permutation(nq)
    fo[spots[:len(others)]] = others                          # every other value at least once
    fo[spots[len(others)]] = lone
    assert set(fo.tolist()) == set(range(-1, F)) and np.count_nonzero(fo == lone) == 1
    return fo.astype(np.int64)


def _expected(ix, Q, k, filters, fo, exact=False, stats=False):
    """Row i = today's single-filter call for query i and its filter; with stats also the per-query expansions and the
    sums of the separate calls' counters."""
    n = len(Q)
    ids = np.full((n, k), -7, np.int64)
    dist = np.full((n, k), np.nan, np.float32)
    work = np.zeros(n, np.uint64)
    tot = {"expansions": 0, "exact_l2": 0, "scan_l2": 0, "rerun_queries": 0}
    for f in sorted(set(fo.tolist())):
        sel = np.flatnonzero(fo == f)
        if f < 0:
            i, d = ix.search_batch(Q[sel], k, exact=exact)
        else:
            i, d = ix.search_batch(Q[sel], k, filter=filters[f], exact=exact)
        ids[sel], dist[sel] = i, d
        if stats:
            st = ix.last_search_stats()
            w = ix.last_query_expansions(len(sel))
            work[sel] = w
            tot["expansions"] += st["expansions"]
            tot["exact_l2"] += st["exact_l2"]
            tot["rerun_queries"] += st["rerun_queries"]
            if st["expansions"] == 0:
                tot["scan_l2"] += st["exact_l2"]
    return ids, dist, work, tot


def _same(got, want, where):
    ids, dist = got
    assert ids.shape == want[0].shape and dist.shape == want[1].shape, where
    assert np.array_equal(ids, want[0]), where
    assert np.array_equal(dist.view(np.uint32), want[1].view(np.uint32)), where


# ---- 1. graph route -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bits,variant", CASES)
def test_graph_route_equals_single_filter_calls(cph, gold, name, bits, variant):
    ix = _load(cph, name, bits, variant)
    Q = gold[f"Q/{name}"]
    filters = [ix.make_filter(m) for m in _masks(ix.size, 11)]
    fo = _assign(len(Q), len(filters), 12)
    for k in KS:
        want = _expected(ix, Q, k, filters, fo)
        _same(ix.search_batch(Q, k, filter=filters, filter_of=fo), want, (name, bits, variant, k, "random"))
        # every query names the same filter: the single-filter call itself
        for f in range(len(filters)):
            one = np.full(len(Q), f)
            _same(ix.search_batch(Q, k, filter=filters, filter_of=one), ix.search_batch(Q, k, filter=filters[f]),
                  (name, bits, variant, k, "all", f))
        _same(ix.search_batch(Q, k, filter=filters, filter_of=np.full(len(Q), -1)), ix.search_batch(Q, k),
              (name, bits, variant, k, "all unfiltered"))
    # filters given as masks / id arrays are made and freed by the call
    _same(ix.search_batch(Q, 10, filter=_masks(ix.size, 11), filter_of=fo.tolist()), _expected(ix, Q, 10, filters, fo),
          (name, bits, variant, "masks"))


# ---- 2. exact route, 3. mixed routing: one index built here ------------------------------------------------------------
N_BUILT, DIM_BUILT, NQ_BUILT = 3000, 128, 400


@pytest.fixture(scope="module")
def built(cph):
    rng = np.random.default_rng(2024)
    X = rng.standard_normal((N_BUILT, DIM_BUILT)).astype(np.float32)
    Q = (X[rng.integers(0, N_BUILT, NQ_BUILT)] + 0.3 * rng.standard_normal((NQ_BUILT, DIM_BUILT))).astype(np.float32)
    ix = cph.CPIndex(DIM_BUILT, 4, device=0)
    ix.build(X)
    ix.finalize()
    return ix, X, Q


def _group_plan(seg_m, seg_q, k, budget=1 << 30):
    """The work items cph_host_exact_group_plan states for these segments on this device, rows of 8 words."""
    import torch
    from cphnsw_mi355x import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m, q = np.ascontiguousarray(seg_m, np.uint64), np.ascontiguousarray(seg_q, np.uint64)
    out = (C.c_uint64 * 6)()
    _lib.check(_lib.lib().cph_host_exact_group_plan(m.ctypes.data, q.ctypes.data, len(m), k, cus, budget, None, 0, out))
    items = np.zeros((int(out[0]), 8), np.uint32)
    _lib.check(_lib.lib().cph_host_exact_group_plan(m.ctypes.data, q.ctypes.data, len(m), k, cus, budget, items.ctypes.data,
                                                    len(items), out))
    return items


@pytest.mark.parametrize("k", [1, 10, 100, 1024])
def test_exact_route_equals_single_filter_calls(built, k):
    ix, X, Q = built
    masks = _masks(ix.size, 21)
    filters = [ix.make_filter(m) for m in masks]
    fo = _assign(len(Q), len(filters), 22 + k, heavy=1)
    # the batch really is cut: some segment into several parts, some segment's queries into at least two groups
    segs = [f for f in sorted(set(fo.tolist())) if f < 0 or masks[f].any()]
    items = _group_plan([ix.size if f < 0 else int(masks[f].sum()) for f in segs], [int((fo == f).sum()) for f in segs], k)
    assert items[:, 1].max() >= 1, "no segment was cut into parts"
    assert any(len(set(items[items[:, 0] == s][:, 4])) >= 2 for s in range(len(segs))), "no segment has two query groups"
    want = _expected(ix, Q, k, filters, fo, exact=True)
    _same(ix.search_batch(Q, k, filter=filters, filter_of=fo, exact=True), want, (k, "random"))
    for f in (1, 3, 5):
        _same(ix.search_batch(Q, k, filter=filters, filter_of=np.full(len(Q), f), exact=True),
              ix.search_batch(Q, k, filter=filters[f], exact=True), (k, "all", f))
    _same(ix.search_batch(Q, k, filter=filters, filter_of=np.full(len(Q), -1), exact=True), ix.search_batch(Q, k, exact=True),
          (k, "all unfiltered"))


@pytest.mark.parametrize("k", [10, 100])
def test_exact_route_cut_into_several_launches(cph, built, tmp_path, monkeypatch, k):
    """A pool budget of 1 MiB (CPH_EXACT_SCRATCH_MB, read when a handle is made): the grouped scan no longer fits one
    launch, so the descriptor table is walked from an offset, the pool indices start again at 0 and every launch merges
    its own rows.  Asserted on the planner's answer; the expected rows come from the handle with the default budget."""
    ix, X, Q = built
    p = str(tmp_path / "built.idx")
    ix.save(p)
    monkeypatch.setenv("CPH_EXACT_SCRATCH_MB", "1")
    small = cph.CPIndex(DIM_BUILT, 4, device=0)
    small.load(p)
    monkeypatch.delenv("CPH_EXACT_SCRATCH_MB")
    masks = _masks(ix.size, 25)
    filters = [ix.make_filter(m) for m in masks]
    sf = [small.make_filter(m) for m in masks]
    fo = _assign(len(Q), len(filters), 26 + k, heavy=1)
    segs = [f for f in sorted(set(fo.tolist())) if f < 0 or masks[f].any()]
    items = _group_plan([ix.size if f < 0 else int(masks[f].sum()) for f in segs], [int((fo == f).sum()) for f in segs], k,
                        budget=1 << 20)
    launches = int(items[:, 7].max()) + 1
    print("k", k, "work items", len(items), "launches", launches)
    assert launches >= 2, "the batch still fits one launch"
    assert all(items[items[:, 7] == l][:, 6].min() == 0 for l in range(launches))      # pool indices restart per launch
    want = _expected(ix, Q, k, filters, fo, exact=True)
    _same(small.search_batch(Q, k, filter=sf, filter_of=fo, exact=True), want, (k, "1 MiB"))
    # mixed routing under the same budget: the scanned rows among graph-searched and padded ones
    ix.exact_threshold = small.exact_threshold = 500
    try:
        want = _expected(ix, Q, k, filters, fo)
        _same(small.search_batch(Q, k, filter=sf, filter_of=fo), want, (k, "1 MiB, mixed"))
    finally:
        ix.exact_threshold = 0


def test_exact_route_on_the_fixtures(cph, gold):
    """The generic-dimension and D = 1024 instantiations of the grouped scan."""
    for name, bits in (("g16", 2), ("g1024", 2), ("sift96", 4), ("g256", 4)):
        ix = _load(cph, name, bits)
        Q = gold[f"Q/{name}"]
        filters = [ix.make_filter(m) for m in _masks(ix.size, 31)]
        fo = _assign(len(Q), len(filters), 32)
        for k in KS:
            _same(ix.search_batch(Q, k, filter=filters, filter_of=fo, exact=True), _expected(ix, Q, k, filters, fo, exact=True),
                  (name, bits, k))


@pytest.mark.parametrize("k", [10, 100])
def test_mixed_routing_and_statistics(built, k):
    """exact_threshold between the filter sizes: one call holds scanned, graph-searched, padded and unfiltered rows, and
    its statistics are those of the separate calls."""
    ix, X, Q = built
    masks = _masks(ix.size, 41)
    filters = [ix.make_filter(m) for m in masks]
    fo = _assign(len(Q), len(filters), 42)
    sizes = [int(m.sum()) for m in masks]
    ix.exact_threshold = 500
    try:
        assert sizes[0] > 500 and sizes[1] > 500 and 0 < sizes[2] <= 500 and 0 < sizes[3] <= 500 and sizes[5] == 0
        want_ids, want_d, want_work, tot = _expected(ix, Q, k, filters, fo, stats=True)
        got = ix.search_batch(Q, k, filter=filters, filter_of=fo)
        st = ix.last_search_stats()
        work = ix.last_query_expansions(len(Q))
        _same(got, (want_ids, want_d), (k, "mixed"))
        print("mixed routing stats:", st, "separate calls:", tot)
        assert tot["expansions"] > 0 and tot["scan_l2"] > 0            # both the graph and the scan did work
        assert st["expansions"] == tot["expansions"]
        assert st["exact_l2"] == tot["exact_l2"]
        assert np.array_equal(work.astype(np.uint64), want_work)
        scanned_or_padded = np.isin(fo, [2, 3, 4, 5])
        assert (work[scanned_or_padded] == 0).all() and (work[~scanned_or_padded] > 0).all()
    finally:
        ix.exact_threshold = 0


# ---- 4. the same equality through four more paths ----------------------------------------------------------------------
def test_input_row_ids_and_input_row_filters(built):
    ix, X, Q = built
    masks = _masks(ix.size, 51)
    fo = _assign(len(Q), len(masks), 52)
    ix.result_ids = "input"
    try:
        filters = [ix.make_filter(m, ids="input") for m in masks]
        for exact, thr in ((False, 0), (False, 500), (True, 0)):
            ix.exact_threshold = thr
            want = _expected(ix, Q, 10, filters, fo, exact=exact)
            _same(ix.search_batch(Q, 10, filter=filters, filter_of=fo, exact=exact), want, ("input rows", exact, thr))
            # the rows really are input rows: every returned id is allowed by its query's mask
            ids = want[0]
            for i in range(len(Q)):
                if fo[i] >= 0:
                    assert masks[fo[i]][ids[i][ids[i] >= 0]].all()
    finally:
        ix.exact_threshold = 0
        ix.result_ids = "internal"


def test_device_entry(cph, gold, built):
    import torch
    ix, X, Q = built
    filters = [ix.make_filter(m) for m in _masks(ix.size, 61)]
    fo = _assign(len(Q), len(filters), 62)
    qt = torch.from_numpy(Q).cuda()
    try:
        for exact, thr in ((False, 0), (False, 500), (True, 0)):
            ix.exact_threshold = thr
            want = _expected(ix, Q, 10, filters, fo, exact=exact)
            for rep in range(3):                                   # the batch sets take turns: tables are rewritten
                ids_t, dist_t = ix.search_batch_device(qt, 10, filter=filters, filter_of=fo, exact=exact)
                ix.synchronize()
                _same((ids_t.cpu().numpy(), dist_t.cpu().numpy()), want, ("device", exact, thr, rep))
    finally:
        ix.exact_threshold = 0
    name, bits = "g128", 4
    small = _load(cph, name, bits)
    Qs = gold[f"Q/{name}"]
    fs = [small.make_filter(m) for m in _masks(small.size, 63)]
    fos = _assign(len(Qs), len(fs), 64)
    ids_t, dist_t = small.search_batch_device(torch.from_numpy(Qs).cuda(), 10, filter=fs, filter_of=fos.tolist())
    small.synchronize()
    _same((ids_t.cpu().numpy(), dist_t.cpu().numpy()), _expected(small, Qs, 10, fs, fos), "device, fixture")


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g128", 1), ("g16", 2), ("g1024", 2)])
def test_two_replicas(cph, gold, name, bits):
    ix = _load(cph, name, bits, devices=[0, 0])
    ix.set_min_shard(4)                                            # 24 queries: split into two shards
    Q = gold[f"Q/{name}"]
    filters = [ix.make_filter(m) for m in _masks(ix.size, 71)]
    fo = _assign(len(Q), len(filters), 72)
    for exact, thr in ((False, 0), (False, 30), (True, 0)):
        ix.exact_threshold = thr
        want = _expected(ix, Q, 10, filters, fo, exact=exact)
        _same(ix.search_batch(Q, 10, filter=filters, filter_of=fo, exact=exact), want, (name, bits, exact, thr))
    # the same rows as one device ...
    single = _load(cph, name, bits)
    masks = _masks(ix.size, 71)
    sf = [single.make_filter(m) for m in masks]
    _same(ix.search_batch(Q, 10, filter=filters, filter_of=fo, exact=True), single.search_batch(Q, 10, filter=sf, filter_of=fo, exact=True),
          (name, bits, "against one device"))
    # ... and the shards were two: after that exact call each replica's own counter holds the candidates of ITS half of the
    # batch (a scanned query costs its filter's size, an unfiltered one the index; which replica took which half rotates)
    from cphnsw_mi355x import _lib
    cost = np.array([ix.size if f < 0 else int(masks[f].sum()) for f in fo], np.uint64)
    half = (len(Q) + 1) // 2
    seen = []
    for h in ix._reps:
        out = (C.c_uint64 * 12)()
        _lib.check(_lib.lib().cph_last_search_stats(h, out))
        seen.append(int(out[1]))                                   # exact_l2
    print("exact_l2 per replica:", seen, "halves:", int(cost[:half].sum()), int(cost[half:].sum()))
    assert len(seen) == 2 and min(seen) > 0
    assert sorted(seen) == sorted([int(cost[:half].sum()), int(cost[half:].sum())])


@pytest.mark.parametrize("name,bits,variant", [(n, b, "plain") for n, s in DATASETS.items() for b in s["bits"]])
def test_overflow_rerun_carries_the_table(cph, gold, name, bits, variant):
    ix = _load(cph, name, bits, variant)
    Q = gold[f"Q/{name}"]
    filters = [ix.make_filter(m) for m in _masks(ix.size, 81)]
    fo = _assign(len(Q), len(filters), 82)
    for k in (10, 100):
        ix.set_search_params(slots=0, beam_capacity=0)
        want = _expected(ix, Q, k, filters, fo)
        ix.set_search_params(slots=8, beam_capacity=64)
        _same(ix.search_batch(Q, k, filter=filters, filter_of=fo), want, (name, bits, k, "overflow"))
        reruns = ix.last_search_stats()["rerun_queries"]
        # the separate calls under the same small capacity say how many queries overflow: the one call re-runs as many
        small_ids, small_d, _, tot = _expected(ix, Q, k, filters, fo, stats=True)
        print(name, bits, k, "re-run queries:", reruns, "separate calls:", tot["rerun_queries"])
        assert reruns == tot["rerun_queries"], (name, bits, k)
        if ix.size >= 300:
            assert reruns > 0, "nothing overflowed: the re-run launch was not exercised"
        _same(ix.search_batch(Q, k, filter=filters, filter_of=fo), (small_ids, small_d), (name, bits, k, "both small"))


# ---- 5. errors ---------------------------------------------------------------------------------------------------------
def test_errors_leave_the_index_usable(cph, gold):
    ix = _load(cph, "g128", 4)
    other = _load(cph, "g16", 4)                                   # another size
    multi = _load(cph, "g128", 4, devices=[0, 0])
    Q = gold["Q/g128"]
    n = len(Q)
    filters = [ix.make_filter(m) for m in _masks(ix.size, 91)]
    fo = _assign(n, len(filters), 92)
    want = _expected(ix, Q, 10, filters, fo)
    closed = ix.make_filter(np.ones(ix.size, bool))
    closed.close()
    bad = [
        dict(filter=filters[0], filter_of=fo),                     # filter_of without a sequence
        dict(filter=None, filter_of=fo),
        dict(filter=np.ones(ix.size, bool), filter_of=fo),
        dict(filter=filters, filter_of=None),                      # a sequence without filter_of
        dict(filter=_masks(ix.size, 91), filter_of=None),          # ... of masks
        dict(filter=[np.array([1, 2, 3]), np.array([4, 5])], filter_of=None),               # ... of id arrays
        dict(filter=([1, 2, 3], [4, 5]), filter_of=None),          # ... of id lists
        dict(filter=[filters[0], np.ones(ix.size, bool)], filter_of=None),
        dict(filter=filters, filter_of=fo[:-1]),                   # wrong length
        dict(filter=filters, filter_of=np.zeros((n, 1), np.int64)),
        dict(filter=filters, filter_of=np.zeros(n, np.float32)),
        dict(filter=filters, filter_of=np.where(np.arange(n) == 5, len(filters), fo)),      # outside [-1, F)
        dict(filter=filters, filter_of=np.where(np.arange(n) == 5, -2, fo)),
        dict(filter=filters[:2] + [closed], filter_of=np.zeros(n, np.int64)),               # a closed filter
        dict(filter=[other.make_filter(np.ones(other.size, bool))], filter_of=np.zeros(n, np.int64)),   # another size
        dict(filter=[multi.make_filter(np.ones(multi.size, bool))], filter_of=np.zeros(n, np.int64)),   # another replica count
        dict(filter=[np.ones(ix.size + 1, bool)], filter_of=np.zeros(n, np.int64)),          # what make_filter refuses
    ]
    for kw in bad:
        for exact in (False, True):
            with pytest.raises(ValueError):
                ix.search_batch(Q, 10, exact=exact, **kw)
            _same(ix.search_batch(Q, 10, filter=filters, filter_of=fo), want, ("after", sorted(kw), exact))
    # a flat list of ids without filter_of is still ONE filter
    _same(ix.search_batch(Q, 10, filter=[1, 2, 3]), ix.search_batch(Q, 10, filter=np.array([1, 2, 3])), "flat id list")
    with pytest.raises(ValueError, match="k <= 1024"):
        ix.search_batch(Q, 1025, filter=filters, filter_of=fo, exact=True)
    # the C entry checks the values itself
    from cphnsw_mi355x import _lib
    ids = np.empty((n, 10), np.int64)
    dist = np.empty((n, 10), np.float32)
    hs = (C.c_void_p * len(filters))(*[f._h.value for f in filters])
    for v in (len(filters), -2):
        raw = fo.astype(np.int32)
        raw[3] = v
        rc = _lib.lib().cph_search_batch_filters(ix._h, Q.ctypes.data, n, 10, hs, len(filters), raw.ctypes.data, 0, ids.ctypes.data,
                                                 dist.ctypes.data)
        assert rc == _lib.INVALID_ARGUMENT
    import torch
    with pytest.raises(ValueError):
        ix.search_batch_device(torch.from_numpy(Q).cuda(), 10, filter=filters, filter_of=fo[:-1])
    with pytest.raises(ValueError):
        multi.search_batch(Q, 10, filter=filters, filter_of=fo)    # single-device filters on two replicas
    _same(ix.search_batch(Q, 10, filter=filters, filter_of=fo), want, "at the end")
