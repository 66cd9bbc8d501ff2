"""The matrix engine of the exact range search (index.exact_engine = "matrix"; csrc/device_range_mfma.h) against the ORACLE
model of tests/test_gpu_range.py: lims, ids and distance BYTES equal, no tolerance -- the matrix cores only discard pairs
that provably are not hits, the vector arithmetic forms every distance and decides every hit.

What the statistics must say: matrix_parts is the exported plan's, exact_l2 == matrix_survivors, and
hits <= survivors <= #{pairs with oracle d < lim + eps}: a survivor has d^ < lim (or a d^ that is not finite, which the
fixtures do not produce), and d <= d^ + eps.  eps: the slack of tests/exact_matrix_model.py, from float64 norms rounded up, so
it is at least the device's, and with it lim."""
import ctypes as C
import zlib

import numpy as np
import pytest

from exact_matrix_model import slack_of
from golden_util import DATASETS, fixture_path
from test_gpu_exact import _all_distances, _allowed
from test_gpu_range import CASES, COUNTS, _load, _model, _radius_for, _range_plan, _same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _matrix(cph, name, bits, **kw):
    ix = _load(cph, name, bits, **kw)
    ix.exact_engine = "matrix"
    return ix


def _parts(m, nq):
    import torch
    from cphnsw_mi355x import _lib
    out = (C.c_uint64 * 2)()
    _lib.check(_lib.lib().cph_host_range_matrix_plan(m, nq, torch.cuda.get_device_properties(0).multi_processor_count, out))
    return int(out[0])


def _limits(radius, eps):
    from cphnsw_mi355x import _lib
    out = C.c_float()
    lim = np.empty(len(radius))
    for i, (r, e) in enumerate(zip(radius, eps)):
        _lib.check(_lib.lib().cph_host_range_matrix_limit(float(r), float(e), C.byref(out)))
        lim[i] = out.value
    return lim


def _check(ix, got, want, dist, radius, eps, where):
    """Bytes, then the statistics of a matrix range search over the distance matrix `dist` [nq, m]."""
    assert _same(got, want), where
    st = ix.last_search_stats()
    nq, m = dist.shape
    hits = int(want[0][-1])
    lim = _limits(np.broadcast_to(np.asarray(radius, np.float32), (nq,)), eps)
    with np.errstate(invalid="ignore"):
        bound = int((dist.astype(np.float64) < (lim + eps)[:, None]).sum())     # (lim = -1: nothing need survive; NaN: never here)
    print(where, "hits", hits, "survivors", st.get("matrix_survivors"), "bound", bound)
    assert hits <= bound, ("bad input", where)
    assert st["matrix_parts"] == _parts(m, nq) and st["matrix_redo"] == 0, (where, st)
    assert st["exact_l2"] == st["matrix_survivors"] and hits <= st["matrix_survivors"] <= bound, (where, st, hits, bound)
    assert st["expansions"] == 0 and st["kernel_us"] == 0, (where, st)


@pytest.mark.parametrize("name,bits", CASES)
def test_range_matches_oracle_on_every_fixture(cph, oracle, gold, name, bits):
    ix = _matrix(cph, name, bits)
    oi = oracle.load(fixture_path(name, bits))
    Q = gold[f"Q/{name}"]
    nq, n = len(Q), ix.size
    assert nq == 24
    eps = slack_of(Q, ix.get_vectors(), DATASETS[name]["D"])
    rng = np.random.default_rng(zlib.crc32(f"r{name}{bits}".encode()))
    one = np.zeros(n, bool)
    one[7] = True
    for fname, mask in (("none", None), ("p0.5", rng.random(n) < 0.5), ("p0.1", rng.random(n) < 0.1), ("single", one)):
        allowed = _allowed(mask, n)
        dist = _all_distances(oi, Q, allowed)
        srt = np.sort(dist, axis=1)
        f = None if mask is None else ix.make_filter(mask)
        for above in (True, False):
            for shift in range(len(COUNTS)):
                radius = np.array([_radius_for(srt[i], COUNTS[(i + shift) % len(COUNTS)], above)[0] for i in range(nq)], np.float32)
                _check(ix, ix.range_search(Q, radius, filter=f), _model(dist, allowed, radius), dist, radius, eps, (name, fname, above, shift))
        for r in (0.0, -1.0, float("nan"), float("inf")):
            _check(ix, ix.range_search(Q, r, filter=f), _model(dist, allowed, np.full(nq, r, np.float32)), dist, r, eps, (name, fname, r))
        radius = np.array([np.nan, -0.0, np.inf, srt[3][min(5, len(srt[3]) - 1)]] * 6, np.float32)
        _check(ix, ix.range_search(Q, radius, filter=f), _model(dist, allowed, radius), dist, radius, eps, (name, fname, "mixed"))
        if name == "g128" and mask is None:
            assert ix.last_search_stats()["matrix_parts"] > 1


def test_four_query_tiles_of_near_ties(cph, oracle):
    """400 queries, three full query tiles and a ragged one: query i is the float32 midpoint of row i and its nearest
    neighbour, the radius exactly the larger of its two distances -- a hit and a survivor that is none, a few ulp apart."""
    import torch
    ix = _matrix(cph, "g128", 4)
    oi = oracle.load(fixture_path("g128", 4))
    X = np.ascontiguousarray(ix.get_vectors())
    n = len(X)
    allowed = _allowed(None, n)
    dx = _all_distances(oi, X, allowed)
    np.fill_diagonal(dx, np.inf)
    nn = dx.argmin(1)
    Q = ((X.astype(np.float64) + X[nn]) / 2).astype(np.float32)
    dist = _all_distances(oi, Q, allowed)
    radius = np.maximum(dist[np.arange(n), np.arange(n)], dist[np.arange(n), nn]).astype(np.float32)
    want = _model(dist, allowed, radius)
    assert (np.diff(want[0]) <= 1).all() and int(want[0][-1]) >= n // 2
    _check(ix, ix.range_search(Q, radius), want, dist, radius, slack_of(Q, X, 128), "midpoints")
    st = ix.last_search_stats()
    assert st["matrix_parts"] > 1 and st["matrix_survivors"] >= 2 * n
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    Qd = torch.from_numpy(Q).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    lims, ids, d = ix.range_search_device(Qd, radius, stream=side)
    assert _same((lims.numpy(), ids.cpu().numpy(), d.cpu().numpy()), want)


@pytest.fixture(scope="module")
def copies(cph, oracle, tmp_path_factory):
    """2 RUN + 809 rows of dim 128 of which 2 RUN + 1 are one vector v; 48 queries: Gaussian rows plus 1 % noise."""
    run = _range_plan(cph, 1000, 24)["run"]
    n, dim = 2 * run + 809, 128
    rng = np.random.default_rng(20251)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    is_copy = np.zeros(n, bool)
    is_copy[rng.choice(n, 2 * run + 1, replace=False)] = True
    v = X[np.flatnonzero(is_copy)[0]]
    X[is_copy] = v
    Q = (X[np.flatnonzero(~is_copy)[:48]] * (1 + 0.01 * rng.standard_normal((48, dim)))).astype(np.float32)
    ix = cph.CPIndex(dim, 4)
    ix.build(X)
    ix.finalize()
    p = str(tmp_path_factory.mktemp("copies") / "copies.idx")
    ix.save(p)
    internal = ix.get_vectors()
    is_copy = (internal == v).all(1)                                     # (internal id order)
    assert int(is_copy.sum()) == 2 * run + 1
    dist = _all_distances(oracle.load(p), Q, np.arange(n, dtype=np.uint32))
    dv = dist[:, np.flatnonzero(is_copy)[0]].copy()
    assert (dist[:, is_copy] == dv[:, None]).all()
    return dict(run=run, n=n, path=p, Q=Q, dist=dist, dv=dv, is_copy=is_copy, eps=slack_of(Q, internal, dim))


@pytest.mark.parametrize("k_run,extra", ((1, 0), (1, 1), (2, 0), (2, 1)))
def test_long_segments_with_non_hits_inside(cph, copies, monkeypatch, k_run, extra):
    """Segments of RUN, RUN + 1, 2 RUN and 2 RUN + 1 copies of v (a filter admits that many of them and every other row),
    empty segments between them.  Radius exactly d(q, v): every copy survives and none is a hit; one float above: all of them
    hit, with tied distances in id order.  Then the same call on a handle with 1 MiB of scratch: the vector route answers."""
    c = copies
    count = k_run * c["run"] + extra
    mask = ~c["is_copy"]
    mask[np.flatnonzero(c["is_copy"])[:count]] = True
    allowed = _allowed(mask, c["n"])
    dist = c["dist"][:, mask]
    radius = np.zeros(48, np.float32)
    radius[0::4] = c["dv"][0::4]
    radius[2::4] = np.nextafter(c["dv"][2::4], np.float32(np.inf))
    want = _model(dist, allowed, radius)
    got_counts = np.diff(want[0])
    assert (got_counts[0::4] < 809).all() and (got_counts[2::4] >= count).all() and not got_counts[1::2].any()
    ix = cph.CPIndex(128, 4)
    ix.load(c["path"])
    ix.exact_engine = "matrix"
    f = ix.make_filter(mask)
    _check(ix, ix.range_search(c["Q"], radius, filter=f), want, dist, radius, c["eps"], ("copies", count))
    assert ix.last_search_stats()["matrix_survivors"] >= 24 * count
    monkeypatch.setenv("CPH_EXACT_SCRATCH_MB", "1")
    small = cph.CPIndex(128, 4)
    small.load(c["path"])
    monkeypatch.delenv("CPH_EXACT_SCRATCH_MB")
    small.exact_engine = "matrix"
    assert _same(small.range_search(c["Q"], radius, filter=small.make_filter(mask)), want)
    st = small.last_search_stats()
    assert st["exact_l2"] == 2 * 48 * len(allowed) and not [key for key in st if key.startswith("matrix")], st


@pytest.mark.parametrize("route", ("cosine", "remove_add", "input_ids"))
def test_routes(cph, gold, route):
    """No oracle serves these routes: bytes equal to the vector engine on the same index; under result_ids = "input" the unfiltered
    answer also to the internal-id answer through the row map."""
    Q = gold["Q/g128"]
    rng = np.random.default_rng(8)
    if route == "remove_add":
        ix = _load(cph, "g128", 4)
        n = ix.size
        assert ix.remove(rng.choice(n, n // 4, replace=False)) == n // 4
        ix.add(rng.standard_normal((200, 128)).astype(np.float32))
    else:
        X = rng.standard_normal((1500, 128)).astype(np.float32) * rng.uniform(0.1, 10, (1500, 1)).astype(np.float32)
        ix = cph.CPIndex(128, 4, **(dict(metric="cosine") if route == "cosine" else {}))
        ix.build(X)
        ix.finalize()
    if route == "input_ids":
        ix.result_ids = "input"
    mask = rng.random(ix.size) < 0.6
    for flt in (None, mask):
        _, d = ix.search_batch(Q, 70, filter=flt, exact=True)
        for radius in (d[:, 64].copy(), np.nextafter(d[:, 64], np.float32(np.inf)), np.float32(np.inf)):
            radius = np.broadcast_to(np.asarray(radius, np.float32), (len(Q),))
            ix.exact_engine = "vector"
            want = ix.range_search(Q, radius, filter=flt)
            if route == "input_ids" and flt is None:                 # (a mask under "input" names input rows: another filter)
                ix.result_ids = "internal"
                internal = ix.range_search(Q, radius)
                ix.result_ids = "input"
                assert _same(want, (internal[0], ix.row_map()[internal[1]], internal[2]))
            ix.exact_engine = "matrix"
            got = ix.range_search(Q, radius, filter=flt)
            st = ix.last_search_stats()
            assert _same(got, want), (route, flt is None)
            assert st["matrix_parts"] >= 1 and int(want[0][-1]) <= st["matrix_survivors"] == st["exact_l2"], (route, st)
