"""Exact search on the GPU (search_batch(..., exact=True), exact_threshold) against the ORACLE, not the library: the
model of a row is the oracle's exact_l2(query, allowed ids) on the same index file, ordered by np.lexsort((ids, dist)),
cut at k and padded with -1 / FLT_MAX.  Ids and distance BYTES must be equal -- no tolerance: both sides run the same
eight FMA chains and the same reduction tree."""
import gc
import zlib

import numpy as np
import pytest

from filtered_model_lib import ModelIndex
from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
KS = (1, 10, 100, 550, 1024)
# every fixture (every padded dimension 16..2048), its widest code
CASES = [(n, s["bits"][-1]) for n, s in DATASETS.items()]


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _load(cph, name, bits, **kw):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits, **kw)
    ix.load(fixture_path(name, bits))
    return ix


def _filters(n, seed):
    rng = np.random.default_rng(seed)
    out = {"p0.5": rng.random(n) < 0.5, "p0.1": rng.random(n) < 0.1}
    r = np.zeros(n, bool)
    r[n // 4:n // 4 + max(1, n // 5)] = True
    out["range"] = r
    one = np.zeros(n, bool)
    one[7] = True
    out["single"] = one
    out["empty"] = np.zeros(n, bool)
    out["none"] = None
    return out


def _all_distances(oi, Q, allowed):
    """[nq, m] float32: the oracle's exact L2 of every query against the allowed ids (ascending)."""
    return np.stack([oi.exact_l2(q, allowed) for q in Q]) if len(allowed) else np.zeros((len(Q), 0), np.float32)


def _model(dist, allowed, k):
    """Rows of the exact search from the distance matrix: lexsort by (distance, id), cut at k, pad."""
    nq = dist.shape[0]
    ids = np.full((nq, k), -1, np.int64)
    d = np.full((nq, k), FMAX, np.float32)
    allowed = np.asarray(allowed, np.int64)
    for i in range(nq):
        order = np.lexsort((allowed, dist[i]))[:k]
        ids[i, :len(order)] = allowed[order]
        d[i, :len(order)] = dist[i][order]
    return ids, d


def _plan(cph, m, nq, k, scratch_bytes=1 << 30):
    """The cut the library's planner makes for such a batch on this GPU (cph_host_exact_plan): parts, candidates per part,
    queries per group, queries per launch, keys per pool, pool bytes."""
    import ctypes as C
    import torch
    from cphnsw_mi355x import _lib
    out = (C.c_uint64 * 6)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.check(_lib.lib().cph_host_exact_plan(m, nq, k, cus, scratch_bytes, out))
    return dict(zip(("parts", "part", "group", "tile_q", "pool_keys", "pool_bytes"), [int(x) for x in out]))


def _allowed(mask, n):
    return np.arange(n, dtype=np.uint32) if mask is None else np.flatnonzero(mask).astype(np.uint32)


@pytest.mark.parametrize("name,bits", CASES)
def test_exact_matches_oracle_on_every_fixture(cph, oracle, gold, name, bits):
    ix = _load(cph, name, bits)
    oi = oracle.load(fixture_path(name, bits))
    Q = gold[f"Q/{name}"]
    n = ix.size
    mism = 0
    for fname, mask in _filters(n, zlib.crc32(f"x{name}{bits}".encode())).items():
        allowed = _allowed(mask, n)
        dist = _all_distances(oi, Q, allowed)
        f = None if mask is None else ix.make_filter(mask)
        for k in KS:
            want_ids, want_d = _model(dist, allowed, k)
            ids, d = ix.search_batch(Q, k, filter=f, exact=True)
            bad = int((ids != want_ids).sum()) + int((d.view(np.uint32) != want_d.view(np.uint32)).sum())
            print(name, bits, fname, k, "mismatches:", bad)
            mism += bad
            st = ix.last_search_stats()
            assert st["expansions"] == 0 and (ix.last_query_expansions(len(Q)) == 0).all(), (name, fname, k)
            assert st["exact_l2"] == len(Q) * len(allowed), (name, fname, k, st)
            for key in ("new_neighbours", "beam_pushes", "stage2_skipped", "rerun_queries", "expansions_nothing_new", "slots",
                        "capacity", "stage2_reruns", "stage2_undecided"):
                assert st[key] == 0, (name, fname, k, st)
            if mask is None:
                # Q[0] = X[7]: a zero distance, up to the cancellation of qnorm + norm - 2 dot in float32
                assert want_d[0, 0] <= 1e-5 * float(np.dot(Q[0], Q[0])) and d[0, 0] == want_d[0, 0], (name, k)
        with pytest.raises(ValueError, match="1024"):
            ix.search_batch(Q, 1025, filter=f, exact=True)
    assert mism == 0


def test_ties_come_out_in_internal_id_order(cph, oracle, tmp_path):
    """300 rows of which the last 40 repeat the first 40: equal distance bits leave in ascending INTERNAL id, each id
    once; under result_ids = "input" the rows are row_map()[those internal ids], in the same order."""
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
    for k in (1, 10, 300):
        want_ids, want_d = _model(dist, allowed, k)
        ids, d = ix.search_batch(Q, k, exact=True)
        assert np.array_equal(ids, want_ids) and _beq(d, want_d), k
        ix.result_ids = "input"
        rids, rd = ix.search_batch(Q, k, exact=True)
        ix.result_ids = "internal"
        assert np.array_equal(rids, rm[want_ids]) and _beq(rd, want_d), k
    ids, d = ix.search_batch(Q, 300, exact=True)
    assert all(len(set(r)) == 300 for r in ids.tolist())                 # no id twice
    ties = (d[:, 1:] == d[:, :-1])
    assert ties.sum() >= 40 * len(Q)                                      # every repeated row ties with its twin
    assert (ids[:, 1:][ties] > ids[:, :-1][ties]).all()
    # a filter in input rows is an internal-id filter once made: nothing changes for the exact path
    rows_allowed = np.arange(0, 300, 3)
    f = ix.make_filter(rows_allowed, ids="input")
    inv = np.empty(300, np.int64)
    inv[rm] = np.arange(300)
    allowed_i = np.sort(inv[rows_allowed]).astype(np.uint32)
    want_ids, want_d = _model(_all_distances(oi, Q, allowed_i), allowed_i, 20)
    ids, d = ix.search_batch(Q, 20, filter=f, exact=True)
    assert np.array_equal(ids, want_ids) and _beq(d, want_d)


def test_exact_at_scale_merges_parts(cph, oracle, tmp_path, monkeypatch):
    """The 70,000 x 128 GPU-built index of test_filtered_search_at_scale, saved to v2 and opened by the oracle; the 1 %
    random mask (about 700 ids), a contiguous 10 % id range (7,000 ids) and no filter.  Every case must be cut into several
    candidate parts, so that every row is folded from several workgroups' lists by the merge kernel: asserted on the
    planner's own answer for this GPU.  Then the same index under a pool budget of 8 MiB (CPH_EXACT_SCRATCH_MB, read when
    a handle is made): 200 queries at k = 550 no longer fit one launch, the batch is tiled inside the call (a second
    scan + merge launch with q_first > 0 over the reused pools) and the parts are cut down to what the budget holds."""
    rng = np.random.default_rng(4242)
    n, dim = 70000, 128
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((200, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 4)
    ix.build(X)
    ix.finalize()
    p = str(tmp_path / "scale.idx")
    ix.save(p)
    oi = oracle.load(p)
    mask = rng.random(n) < 0.01
    rmask = np.zeros(n, bool)
    rmask[21000:28000] = True
    for label, m, q in (("1 %", mask, Q), ("range 10 %", rmask, Q), ("none", None, Q[:24])):
        allowed = _allowed(m, n)
        dist = _all_distances(oi, q, allowed)
        f = None if m is None else ix.make_filter(m)
        for k in (10, 550):
            want_ids, want_d = _model(dist, allowed, k)
            pl = _plan(cph, len(allowed), len(q), k)
            assert pl["parts"] > 1 and pl["tile_q"] == len(q), (label, k, pl)
            ids, d = ix.search_batch(q, k, filter=f, exact=True)
            st = ix.last_search_stats()
            bad = int((ids != want_ids).sum()) + int((d.view(np.uint32) != want_d.view(np.uint32)).sum())
            print(label, "k", k, "mismatches", bad, pl, st)
            assert bad == 0, (label, k)
            assert st["exact_l2"] == len(q) * len(allowed) and st["expansions"] == 0
    # a small pool budget: the batch is tiled inside the call
    monkeypatch.setenv("CPH_EXACT_SCRATCH_MB", "8")
    small = cph.CPIndex(dim, 4)
    small.load(p)
    monkeypatch.delenv("CPH_EXACT_SCRATCH_MB")
    allowed = _allowed(rmask, n)
    dist = _all_distances(oi, Q, allowed)
    sf = small.make_filter(rmask)
    for k in (10, 550):
        pl = _plan(cph, len(allowed), len(Q), k, 8 << 20)
        if k == 550:
            assert 1 < pl["parts"] < _plan(cph, len(allowed), len(Q), k)["parts"] and pl["tile_q"] < len(Q), pl
        want_ids, want_d = _model(dist, allowed, k)
        ids, d = small.search_batch(Q, k, filter=sf, exact=True)
        bad = int((ids != want_ids).sum()) + int((d.view(np.uint32) != want_d.view(np.uint32)).sum())
        print("8 MiB budget, k", k, "mismatches", bad, pl)
        assert bad == 0, k
        assert small.last_search_stats()["exact_l2"] == len(Q) * len(allowed)


def test_threshold_routes_filtered_calls(cph, oracle, gold):
    ix = _load(cph, "g128", 4)
    oi = oracle.load(fixture_path("g128", 4))
    mi = ModelIndex(fixture_path("g128", 4))
    Q = gold["Q/g128"]
    n = ix.size
    mask = np.random.default_rng(9).random(n) < 0.2
    allowed = _allowed(mask, n)
    f = ix.make_filter(mask)
    assert ix.exact_threshold == 0 and f.count == len(allowed)
    for k in (10, 100):
        ex_ids, ex_d = _model(_all_distances(oi, Q, allowed), allowed, k)
        g_ids, g_d, _, _ = mi.search_batch(Q, k, mask, nthreads=16)
        # default: the graph path, as before
        ids, d = ix.search_batch(Q, k, filter=f)
        assert np.array_equal(ids, g_ids) and _beq(d, g_d) and ix.last_search_stats()["expansions"] > 0
        ix.exact_threshold = f.count
        ids, d = ix.search_batch(Q, k, filter=f)
        assert np.array_equal(ids, ex_ids) and _beq(d, ex_d), k
        assert ix.last_search_stats()["expansions"] == 0
        si, sd = ix.search(Q[3], k, filter=f)                       # the single-query form follows the threshold too
        m = int((ex_ids[3] >= 0).sum())
        assert np.array_equal(si, ex_ids[3, :m]) and _beq(sd, ex_d[3, :m])
        ix.exact_threshold = f.count - 1
        ids, d = ix.search_batch(Q, k, filter=f)
        assert np.array_equal(ids, g_ids) and _beq(d, g_d), k
        assert ix.last_search_stats()["expansions"] > 0
        # the empty filter keeps its padding path
        ix.exact_threshold = n
        ids, d = ix.search_batch(Q, k, filter=np.zeros(n, bool))
        assert (ids == -1).all() and (d == FMAX).all()
        ix.exact_threshold = 0
    # a distance of the exact path is the distance the graph path reports for the same id
    ids, d = ix.search_batch(Q, 10, filter=f)
    xi, xd = ix.search_batch(Q, len(allowed), filter=f, exact=True)
    for i in range(len(Q)):
        look = dict(zip(xi[i].tolist(), xd[i].view(np.uint32).tolist()))
        for j, v in zip(ids[i].tolist(), d[i].view(np.uint32).tolist()):
            assert j < 0 or look[j] == v


def test_entry_points(cph, oracle, gold):
    import torch
    ix = _load(cph, "g128", 4)
    Q = gold["Q/g128"]
    n = ix.size
    mask = np.random.default_rng(5).random(n) < 0.3
    f = ix.make_filter(mask)
    for flt in (f, None):
        for k in (1, 10, 500):
            ids, d = ix.search_batch(Q, k, filter=flt, exact=True)
            for i in (0, 5, 23):
                si, sd = ix.search(Q[i], k, filter=flt, exact=True)
                m = int((ids[i] >= 0).sum())
                assert len(si) == m and np.array_equal(si, ids[i, :m]) and _beq(sd, d[i, :m]), (k, i)
    # device batches on a side stream
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    for flt in (f, None):
        for k in (10, 200):
            ids, d = ix.search_batch(Q, k, filter=flt, exact=True)
            did, dd = ix.search_batch_device(Qd, k, stream=side, filter=flt, exact=True)
            ix.synchronize()
            assert np.array_equal(did.cpu().numpy(), ids) and _beq(dd.cpu().numpy(), d), k
    # the device entry follows the threshold as well
    ix.exact_threshold = n
    ids, d = ix.search_batch(Q, 10, filter=f, exact=True)
    did, dd = ix.search_batch_device(Qd, 10, stream=side, filter=f)
    ix.synchronize()
    assert np.array_equal(did.cpu().numpy(), ids) and _beq(dd.cpu().numpy(), d)
    assert ix.last_search_stats()["expansions"] == 0
    # two replicas on one GPU, shards of at least 8 queries: the same rows as one device
    mx = _load(cph, "g128", 4, devices=[0, 0])
    mx.set_min_shard(8)
    mf = mx.make_filter(mask)
    for nq in (1, 7, 24):
        for flt, mflt in ((f, mf), (None, None)):
            ids, d = ix.search_batch(Q[:nq], 10, filter=flt, exact=True)
            mids, md = mx.search_batch(Q[:nq], 10, filter=mflt, exact=True)
            assert np.array_equal(mids, ids) and _beq(md, d), nq
            assert mx.last_search_stats()["expansions"] == 0
    mx.exact_threshold = n
    ids, d = ix.search_batch(Q, 10, filter=f, exact=True)
    mids, md = mx.search_batch(Q, 10, filter=mf)
    assert np.array_equal(mids, ids) and _beq(md, d) and mx.last_search_stats()["expansions"] == 0


def test_filter_lifetime_and_errors(cph, gold):
    import torch
    ix = _load(cph, "g128", 4)
    other = _load(cph, "g16", 4)
    Q = gold["Q/g128"]
    n = ix.size
    allowed = np.arange(0, n, 3)
    want_ids, want_d = ix.search_batch(Q, 100, filter=ix.make_filter(allowed), exact=True)
    # closed or collected while an exact device batch that reads its id list is in flight
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    h = ix.make_filter(allowed)
    ids1, d1 = ix.search_batch_device(Qd, 100, stream=st, filter=h, exact=True)
    h.close()
    h2 = ix.make_filter(allowed)
    ids2, d2 = ix.search_batch_device(Qd, 100, stream=st, filter=h2, exact=True)
    del h2
    gc.collect()
    ix.synchronize()
    for ids, d in ((ids1, d1), (ids2, d2)):
        assert np.array_equal(ids.cpu().numpy(), want_ids) and _beq(d.cpu().numpy(), want_d)
    # errors
    with pytest.raises(ValueError):
        ix.search_batch(Q, 10, filter=other.make_filter(np.ones(other.size, bool)), exact=True)   # another index size
    with pytest.raises(ValueError):
        ix.search_batch(Q, 10, filter=h, exact=True)                                               # closed
    fresh = cph.CPIndex(128, 4)
    with pytest.raises(RuntimeError) as e1:
        fresh.search_batch(Q, 10)
    with pytest.raises(RuntimeError) as e2:
        fresh.search_batch(Q, 10, exact=True)
    assert str(e1.value) == str(e2.value)
