"""Per-query filters under exact_engine = "matrix" (device_exact_mfma_groups.h): every call under the vector engine, then the
matrix engine, on one handle -- the same bytes, through the grouped matrix launches (matrix_parts > 0) with the expected
matrix_redo; on file rows also the oracle model per query under its own filter.  Queries are index rows moved a little;
matrix segments have at least 128 queries, vector-routed ones at most 16: nothing depends on the measured cut-over."""
import ctypes as C

import numpy as np
import pytest

from golden_util import fixture_path
from test_gpu_exact import _all_distances, _allowed, _beq, _load, _model
from test_gpu_exact_matrix_routes import _both

pytestmark = pytest.mark.gpu

FIXTURES = (("g16", 4), ("g128", 4), ("g2048", 1))           # D = 16: one chunk per tile; 128; 2048: 64 chunks
NQ = 640
_W = {}


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _queries(X, n, seed):
    rng = np.random.default_rng(seed)
    return (X[rng.integers(0, len(X), n)] + 0.01 * rng.standard_normal((n, X.shape[1]))).astype(np.float32)


def _world(cph, oracle, name, bits):
    """Once per fixture: the handle, NQ queries and the oracle's distance of every query to every id."""
    if name not in _W:
        ix = _load(cph, name, bits)
        Q = _queries(ix.get_vectors(), NQ, 11)
        _W[name] = ix, Q, _all_distances(oracle.load(fixture_path(name, bits)), Q, _allowed(None, ix.size))
    return _W[name]


def _masks_of(n, pops, seed):
    rng = np.random.default_rng(seed)
    masks = []
    for p in pops:
        m = np.zeros(n, bool)
        m[rng.choice(n, min(p, n), replace=False)] = True
        masks.append(m)
    return masks


def _check(ix, Q, dist, masks, fo, k, what, redo=0):
    filters = [ix.make_filter(m) for m in masks]
    ids, d = _both(ix, lambda: ix.search_batch(Q, k, filter=filters, filter_of=fo, exact=True), what, redo)
    for f in sorted(set(fo.tolist())):
        sel = np.flatnonzero(fo == f)
        allowed = _allowed(None if f < 0 else masks[f], ix.size)
        want_ids, want_d = _model(dist[sel][:, allowed], allowed, k)
        assert np.array_equal(ids[sel], want_ids) and _beq(d[sel], want_d), (what, f)


@pytest.mark.parametrize("k", (1, 10, 100))
@pytest.mark.parametrize("name,bits", FIXTURES)
def test_segments_of_both_routes_in_one_call(cph, oracle, name, bits, k):
    """Three filters and -1, with 128, 300, 5 and 129 queries: a LIST and the non-LIST segment on the matrix kernels, a second
    tile with one live row, and a vector-routed segment, in one call."""
    ix, Q, dist = _world(cph, oracle, name, bits)
    n = ix.size
    masks = _masks_of(n, (n // 2, n // 3, n // 4), 21)
    fo = np.random.default_rng(22).permutation(np.repeat([0, 1, 2, -1], [128, 300, 5, 129]))
    _check(ix, Q[:len(fo)], dist[:len(fo)], masks, fo, k, (name, k))


@pytest.mark.parametrize("k", (1, 10, 100))
@pytest.mark.parametrize("name,bits", FIXTURES)
def test_list_sizes_at_the_tile_edge(cph, oracle, name, bits, k):
    """Filters of 1, 127, 128, 129 and k - 1 allowed ids (padded rows; none at k = 1: the padding route), 128 queries each."""
    ix, Q, dist = _world(cph, oracle, name, bits)
    masks = _masks_of(ix.size, (1, 127, 128, 129, k - 1), 31)
    fo = np.random.default_rng(32).permutation(np.repeat(np.arange(5), 128))
    _check(ix, Q, dist, masks, fo, k, (name, k))


def _groups_plan(seg_m, seg_q, k, budget):
    import torch
    from cphnsw_mi355x import _lib
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m, q = np.ascontiguousarray(seg_m, np.uint64), np.ascontiguousarray(seg_q, np.uint64)
    out = (C.c_uint64 * 6)()
    _lib.check(_lib.lib().cph_host_exact_matrix_groups_plan(m.ctypes.data, q.ctypes.data, len(m), k, cus, budget, None, 0, out))
    return dict(zip(("items", "launches", "tile", "C", "bytes", "parts"), [int(x) for x in out]))


def test_small_scratch_budget(cph, oracle, monkeypatch):
    """A budget of 1 MiB, read when the handle is made: several parts per segment and several launches, by the planner's word."""
    _, Q, dist = _world(cph, oracle, "g128", 4)
    monkeypatch.setenv("CPH_EXACT_SCRATCH_MB", "1")
    ix = _load(cph, "g128", 4)
    monkeypatch.delenv("CPH_EXACT_SCRATCH_MB")
    n = ix.size
    masks = _masks_of(n, (n - 1, 267), 41)
    fo = np.random.default_rng(42).permutation(np.repeat([0, 1, -1], [300, 140, 200]))
    pl = _groups_plan([n - 1, 267, n], [300, 140, 200], 100, 1 << 20)
    assert pl["launches"] > 1 and pl["parts"] > 1, pl
    _check(ix, Q, dist, masks, fo, 100, "1 MiB")
    assert ix.last_search_stats()["matrix_parts"] == pl["parts"]


def test_removed_rows_an_added_row_and_input_rows(cph, oracle):
    ix0, Q, dist = _world(cph, oracle, "g128", 4)
    ix = _load(cph, "g128", 4)
    n = ix.size
    Q = Q[:400]
    masks = _masks_of(n, (n // 2, n // 3), 51)
    filters = [ix.make_filter(m) for m in masks]
    fo = np.random.default_rng(52).permutation(np.repeat([0, 1, -1], [130, 10, 260]))
    gone = np.unique(dist[:400].argmin(1))[:60]                       # true nearest neighbours among them
    ix.remove(gone)
    call = lambda: ix.search_batch(Q, 10, filter=filters, filter_of=fo, exact=True)
    ids, d = _both(ix, call, "removed")                              # F & ~R, and -1 sent to ~R: every segment is a list
    assert not np.isin(ids, gone).any()
    new = int(ix.add(Q[fo == -1][:1])[0])                           # a twin of an unfiltered query: its nearest row
    filters = [ix.make_filter(np.append(m, True)) for m in masks]   # (a filter speaks of the size it was made for)
    ids, d = _both(ix, call, "added")
    assert (ids[np.flatnonzero(fo == -1)[0], 0] == new) and not np.isin(ids, gone).any()
    # result_ids = "input": the certify kernel's row translation, on an index that keeps its builder's row map
    X = np.random.default_rng(53).standard_normal((500, 24)).astype(np.float32)
    rx = cph.CPIndex(24, 4)
    rx.build(X)
    rx.finalize()
    rx.result_ids = "input"
    mask = np.random.default_rng(54).random(500) < 0.5
    Q24 = X[:200] + np.float32(0.01)
    fo = np.repeat([0, -1], [130, 70])
    ids, d = _both(rx, lambda: rx.search_batch(Q24, 10, filter=[rx.make_filter(mask)], filter_of=fo, exact=True), "input rows")
    assert mask[ids[:130]].all() and (ids[130:, 0] == np.arange(130, 200)).all()     # query i is input row i, moved a little


def test_threshold_route_beside_the_graph(cph, oracle):
    """exact_threshold without exact=True: the small filter's 140 queries are scanned on the matrix kernels, the large
    filter's 20 walk the graph, in one call."""
    ix, Q, dist = _world(cph, oracle, "g128", 4)
    masks = _masks_of(ix.size, (150, 350), 61)
    filters = [ix.make_filter(m) for m in masks]
    fo = np.random.default_rng(62).permutation(np.repeat([0, 1], [140, 20]))
    ix.exact_threshold = 200
    try:
        ids, d = _both(ix, lambda: ix.search_batch(Q[:160], 10, filter=filters, filter_of=fo), "threshold")
        assert ix.last_search_stats()["expansions"] > 0
    finally:
        ix.exact_threshold = 0


def test_two_replicas_and_the_device_entry(cph, oracle):
    import torch
    ix, Q, dist = _world(cph, oracle, "g128", 4)
    masks = _masks_of(ix.size, (200, 90), 71)
    fo = np.arange(NQ) % 2                                           # either half of the batch: 160 queries of each filter
    mx = _load(cph, "g128", 4, devices=[0, 0])
    mx.set_min_shard(8)
    _check(mx, Q, dist, masks, fo, 10, "replicas")
    filters = [ix.make_filter(m) for m in masks]
    qt = torch.from_numpy(Q).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def device_call():
        out = ix.search_batch_device(qt, 10, stream=side, filter=filters, filter_of=fo, exact=True)
        ix.synchronize()
        return tuple(t.cpu().numpy() for t in out)
    _both(ix, device_call, "device entry")


def test_fallback_and_a_re_ranker(cph):
    """A filter that allows 300 copies of one row, more than a pool of k = 10 holds (C = 128): its queries are flagged and
    answered by the grouped vector plan behind the matrix launches; the other segment's are not.  And search_grouped with
    filter_of, which rides on the same scan, against its vector-engine result."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((600, 24)).astype(np.float32)
    X[300:] = X[0]
    ix = cph.CPIndex(24, 4)
    ix.build(X)
    ix.finalize()
    Xi = ix.get_vectors()
    twins = (Xi == Xi[np.flatnonzero((Xi == X[0]).all(1))[0]]).all(1)
    assert twins.sum() == 301
    Q = np.concatenate([(X[0] + 0.01 * rng.standard_normal((128, 24))).astype(np.float32), _queries(X[1:300], 130, 6)])
    fo = np.repeat([0, 1], [128, 130])
    filters = [ix.make_filter(twins | (rng.random(600) < 0.2), ids="internal"), ix.make_filter(~twins, ids="internal")]
    _both(ix, lambda: ix.search_batch(Q, 10, filter=filters, filter_of=fo, exact=True), "duplicates", redo=None)
    st = ix.last_search_stats()
    assert st["matrix_redo"] == 128, st                              # every query of the first segment, none of the second
    ix.set_labels(np.arange(600) % 7, ids="internal")
    _both(ix, lambda: ix.search_grouped(Q, 3, 2, candidates=40, filter=filters, filter_of=fo, exact=True), "grouped", redo=None)
