"""Range search on the GPU (CPIndex.range_search / range_search_device) against the ORACLE, not the library: the model of
a segment is the oracle's exact_l2(query, allowed ids) on the same index file, cut at `dist < np.float32(r)` and ordered by
np.lexsort((ids, dist)).  lims, ids and distance BYTES must be equal -- no tolerance: both sides run the same eight FMA
chains and the same reduction tree, and the comparison with the radius is a float32 comparison on both."""
import ctypes as C
import zlib

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path
from test_gpu_exact import _all_distances, _allowed, _filters

pytestmark = pytest.mark.gpu

CASES = [(n, s["bits"][-1]) for n, s in DATASETS.items()]
COUNTS = (0, 1, 63, 64, 65, None)                # hits asked for; None: all
ZERO_STATS = ("expansions", "new_neighbours", "beam_pushes", "stage2_skipped", "rerun_queries", "kernel_us",
              "expansions_nothing_new", "slots", "capacity", "stage2_reruns", "stage2_undecided")


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _load(cph, name, bits, **kw):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits, **kw)
    ix.load(fixture_path(name, bits))
    return ix


def _model(dist, allowed, radius):
    """(lims, ids, dist) of the exact range search from the distance matrix [nq, m] and the radii [nq]."""
    allowed = np.asarray(allowed, np.int64)
    lims, ids, d = [0], [], []
    for i in range(dist.shape[0]):
        hit = dist[i] < np.float32(radius[i])
        a, x = allowed[hit], dist[i][hit]
        order = np.lexsort((a, x))
        ids.append(a[order])
        d.append(x[order])
        lims.append(lims[-1] + len(order))
    return (np.asarray(lims, np.int64), np.concatenate(ids).astype(np.int64) if ids else np.zeros(0, np.int64),
            np.concatenate(d).astype(np.float32) if d else np.zeros(0, np.float32))


def _same(got, want):
    return (np.array_equal(np.asarray(got[0]), want[0]) and np.array_equal(np.asarray(got[1]), want[1])
            and np.asarray(got[2]).dtype == np.float32 and np.asarray(got[2]).tobytes() == want[2].tobytes())


def _radius_for(s, c, above):
    """From a query's ascending model distances s: (radius, hits) with hits = c, or the next count at which two
    neighbours in s differ.  above: the float just above the last hit's distance; else exactly the distance of the first
    id that is NOT a hit, which the strict `<` excludes.  c = None (all): above = just over the farthest; else exactly
    the farthest distance, which drops it (and its ties)."""
    m = len(s)
    if m == 0:
        return np.float32(1.0), 0
    if c is None or c >= m:
        if above:
            return np.nextafter(s[-1], np.float32(np.inf)), m
        return s[-1], int((s < s[-1]).sum())
    while c > 0 and s[c] == s[c - 1]:
        c += 1
        if c == m:
            return _radius_for(s, None, above)
    if c == 0:
        return s[0], 0
    return (np.nextafter(s[c - 1], np.float32(np.inf)) if above else s[c]), c


def _check_stats(ix, nq, m):
    st = ix.last_search_stats()
    assert st["exact_l2"] == 2 * nq * m, st
    for key in ZERO_STATS:
        assert st[key] == 0, (key, st)


@pytest.mark.parametrize("name,bits", CASES)
def test_range_matches_oracle_on_every_fixture(cph, oracle, gold, name, bits):
    ix = _load(cph, name, bits)
    oi = oracle.load(fixture_path(name, bits))
    Q = gold[f"Q/{name}"]
    nq, n = len(Q), ix.size
    assert nq == 24
    for fname, mask in _filters(n, zlib.crc32(f"x{name}{bits}".encode())).items():
        allowed = _allowed(mask, n)
        dist = _all_distances(oi, Q, allowed)
        srt = np.sort(dist, axis=1)
        f = None if mask is None else ix.make_filter(mask)
        for above in (True, False):
            for shift in range(len(COUNTS)):
                picks = [_radius_for(srt[i], COUNTS[(i + shift) % len(COUNTS)], above) for i in range(nq)]
                radius = np.array([p[0] for p in picks], np.float32)
                want = _model(dist, allowed, radius)
                assert np.array_equal(np.diff(want[0]), [p[1] for p in picks]), (name, fname, above, shift)   # the model count
                got = ix.range_search(Q, radius, filter=f)
                print(name, bits, fname, "above" if above else "boundary", shift, "hits", int(want[0][-1]))
                assert _same(got, want), (name, fname, above, shift)
                _check_stats(ix, nq, len(allowed))
        for r, all_of_them in ((0.0, False), (-1.0, False), (float("nan"), False), (float("inf"), True)):
            got = ix.range_search(Q, r, filter=f)
            want = _model(dist, allowed, np.full(nq, r, np.float32))
            assert int(want[0][-1]) == (nq * len(allowed) if all_of_them else 0)
            assert _same(got, want), (name, fname, r)
            _check_stats(ix, nq, len(allowed))
    # a mixed vector: NaN, -0, inf and a finite radius next to each other
    radius = np.array([np.nan, -0.0, np.inf, srt[3][min(5, len(srt[3]) - 1)]] * 6, np.float32)
    assert _same(ix.range_search(Q, radius), _model(dist, allowed, radius))


def _range_plan(cph, m, nq):
    import torch
    from cphnsw_mi355x import _lib
    out = (C.c_uint64 * 5)()
    _lib.check(_lib.lib().cph_host_range_plan(m, nq, torch.cuda.get_device_properties(0).multi_processor_count, out))
    return dict(zip(("parts", "part", "group", "run", "query_rows"), [int(x) for x in out]))


def _n_tiles(lims, budget):
    from cphnsw_mi355x import _lib
    lims = np.ascontiguousarray(lims, np.int64)
    starts = np.zeros(len(lims) + 1, np.uint64)
    nt = C.c_uint64(0)
    _lib.check(_lib.lib().cph_host_range_tiles(lims.ctypes.data, len(lims) - 1, budget, starts.ctypes.data, C.byref(nt)))
    return nt.value


def test_long_segments_merge_runs_and_tile(cph, oracle, tmp_path, monkeypatch):
    """2 RUN + 809 rows: segments of RUN keys (the LDS sort at its limit), RUN + 1 and 2 RUN (two runs, one merge pass),
    2 RUN + 1 and all n (three runs with a short last one, two passes, an unpaired run copied), with empty segments
    between the long ones; several candidate parts.  Then the same call under a 1 MiB scratch budget: several tiles."""
    run = _range_plan(cph, 1000, 24)["run"]
    n, dim = 2 * run + 809, 128
    rng = np.random.default_rng(20250)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((24, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 4)
    ix.build(X)
    ix.finalize()
    p = str(tmp_path / "long.idx")
    ix.save(p)
    oi = oracle.load(p)
    allowed = np.arange(n, dtype=np.uint32)
    dist = _all_distances(oi, Q, allowed)
    srt = np.sort(dist, axis=1)
    assert _range_plan(cph, n, 24)["parts"] > 1
    targets = [run, 0, run + 1, 2 * run, 0, 2 * run + 1, n, 0] * 3
    picks = [_radius_for(srt[i], targets[i], i % 2 == 0) for i in range(24)]
    radius = np.array([x[0] for x in picks], np.float32)
    want = _model(dist, allowed, radius)
    counts = np.diff(want[0])
    assert np.array_equal(counts, [x[1] for x in picks])
    assert all(0 <= int(c) - t <= 2 for c, t in zip(counts, targets)), counts       # (a tie at a boundary moves it by one)
    assert (counts == run).any() and (counts > 2 * run).any() and (counts == n).any() and (counts == 0).any()
    got = ix.range_search(Q, radius)
    assert _same(got, want)
    _check_stats(ix, 24, n)
    ix.result_ids = "input"
    rm = ix.row_map()
    got = ix.range_search(Q, radius)
    ix.result_ids = "internal"
    assert _same(got, (want[0], rm[want[1]], want[2]))
    # a filter: the id list instead of 0..n-1, long segments all the same
    mask = rng.random(n) < 0.97
    al = _allowed(mask, n)
    fd = dist[:, mask]
    r2 = np.array([np.inf, 0.0, srt[2][run]] * 8, np.float32)
    assert _same(ix.range_search(Q, r2, filter=mask), _model(fd, al, r2))
    # 1 MiB of scratch: the batch is tiled inside finish
    monkeypatch.setenv("CPH_EXACT_SCRATCH_MB", "1")
    small = cph.CPIndex(dim, 4)
    small.load(p)
    monkeypatch.delenv("CPH_EXACT_SCRATCH_MB")
    assert _n_tiles(want[0], 1 << 20) > 1 and _n_tiles(want[0], 1 << 30) == 1
    assert _same(small.range_search(Q, radius), want)


def test_ties_leave_in_internal_id_order(cph, oracle, tmp_path):
    """The 300-row index of test_ties_come_out_in_internal_id_order (the last 40 rows repeat the first 40)."""
    rng = np.random.default_rng(77)
    X = rng.standard_normal((300, 128)).astype(np.float32)
    X[260:] = X[:40]
    Q = np.concatenate([X[:8], X[270:274], rng.standard_normal((12, 128)).astype(np.float32)])
    ix = cph.CPIndex(128, 4)
    ix.build(X)
    ix.finalize()
    p = str(tmp_path / "ties.idx")
    ix.save(p)
    oi = oracle.load(p)
    allowed = np.arange(300, dtype=np.uint32)
    dist = _all_distances(oi, Q, allowed)
    rm = ix.row_map()
    for radius in (np.inf, np.float32(np.median(dist)), np.sort(dist, axis=1)[:, 81]):
        radius = np.broadcast_to(np.asarray(radius, np.float32), (len(Q),))
        want = _model(dist, allowed, radius)
        lims, ids, d = ix.range_search(Q, radius)
        assert _same((lims, ids, d), want)
        ix.result_ids = "input"
        got = ix.range_search(Q, radius)
        ix.result_ids = "internal"
        assert _same(got, (want[0], rm[want[1]], want[2]))
    lims, ids, d = ix.range_search(Q, np.inf)
    ties = 0
    for i in range(len(Q)):
        si, sd = ids[lims[i]:lims[i + 1]], d[lims[i]:lims[i + 1]]
        assert len(set(si.tolist())) == 300                              # no id twice
        t = sd[1:] == sd[:-1]
        ties += int(t.sum())
        assert (si[1:][t] > si[:-1][t]).all()
    assert ties >= 40 * len(Q)


def test_removed_rows_leave_the_answer(cph, oracle, gold):
    ix = _load(cph, "g128", 4)
    oi = oracle.load(fixture_path("g128", 4))
    Q = gold["Q/g128"]
    n = ix.size
    rng = np.random.default_rng(31)
    mask = rng.random(n) < 0.5
    f = ix.make_filter(mask)                                             # made BEFORE the remove
    R = np.zeros(n, bool)
    R[rng.choice(n, int(0.3 * n), replace=False)] = True
    assert ix.remove(np.flatnonzero(R)) == int(R.sum())
    full = _all_distances(oi, Q, np.arange(n, dtype=np.uint32))
    radius = np.sort(full, axis=1)[:, n // 3].astype(np.float32)
    for m, flt in ((~R, None), (mask & ~R, f)):
        al = _allowed(m, n)
        for r in (radius, np.float32(np.inf)):
            r = np.broadcast_to(np.asarray(r, np.float32), (len(Q),))
            assert _same(ix.range_search(Q, r, filter=flt), _model(full[:, m], al, r))
            _check_stats(ix, len(Q), len(al))
    # the graph route on such a handle is the search on such a handle
    ids, d = ix.search_batch(Q, 10, filter=f)
    lims, gi, gd = ix.range_search(Q, np.inf, filter=f, exact=False, max_results=10)
    keep = ids >= 0
    assert np.array_equal(lims, np.concatenate([[0], np.cumsum(keep.sum(axis=1))])) and np.array_equal(gi, ids[keep])
    assert gd.tobytes() == d[keep].tobytes() and not R[gi].any()


def test_graph_route_cuts_the_search_rows(cph, gold):
    ix = _load(cph, "g128", 4)
    Q = gold["Q/g128"]
    n = ix.size
    mask = np.random.default_rng(9).random(n) < 0.2
    f = ix.make_filter(mask)
    for K in (10, 100):
        for flt in (f, None):
            ids, d = ix.search_batch(Q, K, filter=flt)
            st0 = ix.last_search_stats()
            assert st0["expansions"] > 0
            fin = np.where(ids >= 0, d, np.nan)
            for radius in (np.nanmedian(fin, axis=1).astype(np.float32), d[:, 0].copy(), np.float32(np.inf), np.float32(0)):
                radius = np.broadcast_to(np.asarray(radius, np.float32), (len(Q),))
                keep = (ids >= 0) & (d < radius[:, None])
                lims, gi, gd = ix.range_search(Q, radius, filter=flt, exact=False, max_results=K)
                assert np.array_equal(lims, np.concatenate([[0], np.cumsum(keep.sum(axis=1))])), K
                assert np.array_equal(gi, ids[keep]) and gd.tobytes() == d[keep].tobytes(), K
                st = ix.last_search_stats()
                assert all(st[k] == st0[k] for k in st if k != "kernel_us"), (st, st0)     # those of the underlying search
    with pytest.raises(ValueError, match="max_results"):
        ix.range_search(Q, 1.0, exact=False)
    with pytest.raises(ValueError, match="max_results"):
        ix.range_search(Q, 1.0, exact=False, max_results=0)


def test_entry_points(cph, gold):
    import torch
    ix = _load(cph, "g128", 4)
    Q = gold["Q/g128"]
    n = ix.size
    mask = np.random.default_rng(5).random(n) < 0.3
    f = ix.make_filter(mask)
    _, d64 = ix.search_batch(Q, 64, exact=True)
    radius = d64[:, 40].copy()
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    for flt in (f, None):
        for kw in (dict(), dict(exact=False, max_results=50)):
            want = ix.range_search(Q, radius, filter=flt, **kw)
            for r in (radius, torch.from_numpy(radius).to(dev)):
                lims, ids, d = ix.range_search_device(Qd, r, filter=flt, stream=side, **kw)
                assert lims.device.type == "cpu" and lims.dtype == torch.int64 and ids.is_cuda and d.is_cuda
                assert _same((lims.numpy(), ids.cpu().numpy(), d.cpu().numpy()), want)
            got = ix.range_search_device(Qd, radius, filter=flt, **kw)                       # torch's current stream
            assert _same((got[0].numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()), want)
    # a filter closed right after the device call: the call has waited for its kernels
    want = ix.range_search(Q, radius, filter=f)
    h = ix.make_filter(mask)
    got = ix.range_search_device(Qd, radius, filter=h, stream=side)
    h.close()
    assert _same((got[0].numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()), want)
    with pytest.raises(ValueError):
        ix.range_search(Q, radius, filter=h)                                                # closed
    # nothing to search
    lims, ids, d = ix.range_search(Q[:0], 1.0)
    assert np.array_equal(lims, [0]) and len(ids) == 0 and len(d) == 0
    lims, ids, d = ix.range_search(Q, np.inf, filter=np.zeros(n, bool))
    assert not lims.any() and len(lims) == len(Q) + 1 and len(ids) == 0
    # two replicas on one GPU, shards of at least 8 queries: the bytes of one device
    mx = _load(cph, "g128", 4, devices=[0, 0])
    mx.set_min_shard(8)
    mf = mx.make_filter(mask)
    for nq in (1, 7, 24):
        for flt, mflt in ((f, mf), (None, None)):
            for kw in (dict(), dict(exact=False, max_results=50)):
                want = ix.range_search(Q[:nq], radius[:nq], filter=flt, **kw)
                assert _same(mx.range_search(Q[:nq], radius[:nq], filter=mflt, **kw), want), (nq, kw)
            assert _same(mx.range_search(Q[:nq], radius[:nq], filter=mflt), ix.range_search(Q[:nq], radius[:nq], filter=flt))
            m = int(mask.sum()) if flt is not None else n
            assert mx.last_search_stats()["exact_l2"] == 2 * nq * m and mx.last_search_stats()["expansions"] == 0
    for _ in range(2):                                                                       # the device form: whole, on one replica, alternating
        got = mx.range_search_device(Qd, radius, filter=mf)
        assert _same((got[0].numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()), ix.range_search(Q, radius, filter=f))


def test_refusals(cph, gold):
    ix = _load(cph, "g128", 4)
    other = _load(cph, "g16", 4)
    Q = gold["Q/g128"]
    n = ix.size
    with pytest.raises(ValueError, match="radius"):
        ix.range_search(Q, np.ones(len(Q) - 1, np.float32))
    with pytest.raises(ValueError, match="radius"):
        ix.range_search(Q, np.ones((len(Q), 1), np.float32))
    with pytest.raises(ValueError, match="radius"):
        ix.range_search(Q, "near")
    with pytest.raises(ValueError, match="queries"):
        ix.range_search(Q[:, :100], 1.0)
    fa, fb = ix.make_filter(np.arange(0, n, 2)), ix.make_filter(np.arange(1, n, 2))
    with pytest.raises(ValueError, match="per-query"):
        ix.range_search(Q, 1.0, filter=[fa, fb], filter_of=np.arange(len(Q)) % 2)
    with pytest.raises(ValueError, match="per-query"):
        ix.range_search(Q, 1.0, filter=[fa, fb])
    with pytest.raises(ValueError):
        ix.range_search(Q, 1.0, filter=other.make_filter(np.ones(other.size, bool)))          # another index size
    # a fresh handle: the error of search_batch
    fresh = cph.CPIndex(128, 4)
    with pytest.raises(RuntimeError) as e1:
        fresh.search_batch(Q, 10)
    with pytest.raises(RuntimeError) as e2:
        fresh.range_search(Q, 1.0)
    with pytest.raises(RuntimeError) as e3:
        fresh.range_search(Q, 1.0, exact=False, max_results=10)
    assert str(e1.value) == str(e2.value) == str(e3.value)
    # a partitioned index points at its parts, whose range search works
    rng = np.random.default_rng(12)
    X = rng.standard_normal((600, 32)).astype(np.float32)
    px = cph.CPIndex(32, 4, devices=[0, 0], partition=True)
    px.build(X)
    px.finalize()
    with pytest.raises(ValueError, match=r"part\(i\)\.range_search"):
        px.range_search(X[:4], 1.0)
    part = px.part(1)
    lo, hi = px.parts[1]
    lims, ids, d = part.range_search(X[lo:lo + 4], 1e-2)
    assert np.array_equal(lims, np.arange(5)) and np.array_equal(ids, np.arange(4))            # each row finds itself (slice-local rows)


def test_remove_between_begin_and_finish_does_not_change_the_answer(cph, oracle, gold):
    """The two-step protocol holds the filter it began under: a remove() between cph_range_search_begin and
    cph_range_search_finish leaves the counted answer; an index swap makes finish fail instead of reading a new index."""
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    oi = oracle.load(fixture_path("g128", 4))
    Q = np.ascontiguousarray(gold["Q/g128"], np.float32)
    nq = len(Q)
    for with_filter in (False, True):
        ix = _load(cph, "g128", 4)
        n = ix.size
        mask = np.random.default_rng(3).random(n) < 0.6 if with_filter else np.ones(n, bool)
        f = ix.make_filter(mask) if with_filter else None
        allowed = _allowed(mask, n)
        dist = _all_distances(oi, Q, allowed)
        radius = np.sort(dist, axis=1)[:, 70].copy()
        want = _model(dist, allowed, radius)
        obj, total = C.c_void_p(), C.c_uint64(0)
        _lib.check(L.cph_range_search_begin(ix._h, Q.ctypes.data, 0, nq, radius.ctypes.data, None if f is None else f._h, 1, 0, None,
                                            C.byref(obj), C.byref(total)))
        try:
            assert total.value == int(want[0][-1])
            assert ix.remove(allowed[::2]) == len(allowed[::2])
            lims = np.zeros(nq + 1, np.int64)
            ids = np.empty(total.value, np.int64)
            d = np.empty(total.value, np.float32)
            _lib.check(L.cph_range_search_finish(obj, lims.ctypes.data, ids.ctypes.data, d.ctypes.data, 0))
            assert _same((lims, ids, d), want)
            with pytest.raises(ValueError):                                              # once per object
                _lib.check(L.cph_range_search_finish(obj, lims.ctypes.data, ids.ctypes.data, d.ctypes.data, 0))
        finally:
            L.cph_range_destroy(obj)
        # the next call sees the remove
        keep = np.ones(len(allowed), bool)
        keep[::2] = False
        assert _same(ix.range_search(Q, radius, filter=f), _model(dist[:, keep], allowed[keep], radius))
    ix = _load(cph, "g128", 4)
    obj, total = C.c_void_p(), C.c_uint64(0)
    radius = np.full(nq, np.inf, np.float32)
    _lib.check(L.cph_range_search_begin(ix._h, Q.ctypes.data, 0, nq, radius.ctypes.data, None, 1, 0, None, C.byref(obj), C.byref(total)))
    try:
        ix.load(fixture_path("g128", 4))
        lims, ids, d = np.zeros(nq + 1, np.int64), np.empty(total.value, np.int64), np.empty(total.value, np.float32)
        with pytest.raises(RuntimeError, match="changed"):
            _lib.check(L.cph_range_search_finish(obj, lims.ctypes.data, ids.ctypes.data, d.ctypes.data, 0))
    finally:
        L.cph_range_destroy(obj)
