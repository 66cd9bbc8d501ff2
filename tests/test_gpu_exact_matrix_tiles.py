"""The matrix engine of the exact scan where a part of the candidate list is SEVERAL candidate tiles and the prefilter
prunes: 2,597 rows under a pool budget of 1 MiB are cut into parts of three tiles (k <= 64) or six (k = 65, 100), the last
part ragged, 400 queries into four launches with all four waves of a workgroup live.  That is the machinery no fixture
of 400 rows reaches: the ids fetched two tiles ahead and their hand-over, the column norms by tile parity, a limit carried
from tile to tile, a compaction in the middle of a part and the cut at its end.  The reference is the ORACLE on the saved
index, as in tests/test_gpu_exact_matrix.py: ids and distance BYTES equal, no tolerance.

matrix_redo.  A flagged query is answered by the vector scan, so equal bytes alone would pass a prefilter that flags
everything.  Every case therefore first derives from the REFERENCE distances which queries may need the fallback at all
(tests/exact_matrix_model.py: need() is the largest number of candidates within 4 eps of the k-th that any prefix a
compaction sees can hold; a query is flagged only if need + 64 > C).  At k = 1, 10, 65, 100
no query may be near that (asserted: an input that needs the fallback is a bad input, not a kernel bug) and matrix_redo
must be 0.  At k = 64 a pool is C = 128 = k + 64 keys and has room for NO candidate beside the k: a single one within
the band flags the query, which Gaussian rows produce for most queries; there matrix_redo may not exceed the number of
queries the reference marks."""
import itertools

import numpy as np
import pytest

from exact_matrix_model import need as _need
from exact_matrix_model import plan as _plan
from exact_matrix_model import slack_of
from test_gpu_exact import _all_distances, _allowed, _beq, _model

pytestmark = pytest.mark.gpu

DIMS = {10: 16, 24: 32, 96: 128}           # dim -> padded D: one chunk of half a K stage, one whole chunk, four chunks
KS = (1, 10, 64, 65, 100)
NQ = 400
SIZES = (2597, 2469, 2341)                 # rows, and what to fall back to where a device's CU count breaks the geometry
BUDGETS_MB = (1, 2, 3, 4)
_W = {}


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _multi_tile(pl, m, ragged):
    last = m - (pl["P"] - 1) * pl["part"]
    return pl["P"] >= 2 and pl["part"] >= 3 * 128 and pl["tile_q"] == 128 and (not ragged or last % 128 != 0)


def _geometry():
    """(n, budget in MiB): the first of SIZES x BUDGETS_MB at which every k cuts the whole index into parts of at least three
    tiles with a ragged last part, and the queries into launches of 128."""
    for n, mb in itertools.product(SIZES, BUDGETS_MB):
        if all(_multi_tile(_plan(n, NQ, k, mb), n, True) for k in KS):
            return n, mb
    raise AssertionError("no size and budget give multi-tile parts on this device")


def _build(cph, monkeypatch, tmp_path_factory, X, dim, mb):
    """A handle made under a pool budget of `mb` MiB (read when the handle is made), built, saved; its path."""
    import time
    monkeypatch.setenv("CPH_EXACT_SCRATCH_MB", str(mb))
    ix = cph.CPIndex(dim, 4)
    t0 = time.perf_counter()
    ix.build(X)
    ix.finalize()
    print(f"build of {len(X)} x {dim}: {time.perf_counter() - t0:.2f} s")
    p = str(tmp_path_factory.mktemp("mx") / f"tiles{dim}_{len(X)}.idx")
    ix.save(p)
    ix.exact_engine = "matrix"
    return ix, p


def _world(cph, oracle, monkeypatch, tmp_path_factory, dim):
    """Once per module and dim: the index, the oracle on its file, 400 queries -- even ones a row plus 1 % noise, odd ones
    fresh -- the oracle's distance of every query to every internal id, and every query's slack."""
    if dim in _W:
        return _W[dim]
    n, mb = _geometry()
    rng = np.random.default_rng(7000 + dim)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((NQ, dim)).astype(np.float32)
    Q[0::2] = X[rng.choice(n, NQ // 2, replace=False)] + 0.01 * Q[0::2]
    ix, p = _build(cph, monkeypatch, tmp_path_factory, X, dim, mb)
    oi = oracle.load(p)
    dist = _all_distances(oi, Q, _allowed(None, n))
    eps = slack_of(Q, ix.get_vectors(), DIMS[dim])
    _W[dim] = dict(ix=ix, oi=oi, Q=Q, dist=dist, eps=eps, n=n, mb=mb, dim=dim)
    return _W[dim]


def _whole_parts(n, k, mb, one_more):
    """The largest list size <= n that is a whole number of multi-tile parts (one_more: and one candidate in a last part
    of its own, so that every other column of that part's only tile is clamped)."""
    for m in range(n, 0, -1):
        pl = _plan(m, NQ, k, mb)
        if _multi_tile(pl, m, False) and m == (pl["P"] - (1 if one_more else 0)) * pl["part"] + (1 if one_more else 0):
            return m
    raise AssertionError("no such list size")


def _mask(w, fname, k):
    n, mb = w["n"], w["mb"]
    rng = np.random.default_rng(900 + w["dim"])
    if fname == "none":
        return None
    if fname == "p0.5":
        return rng.random(n) < 0.5
    if fname == "p0.1":
        return rng.random(n) < 0.1
    mask = np.zeros(n, bool)
    if fname == "range":                                         # contiguous, most of the index, from the middle of a tile
        mask[200:n - 197] = True
    else:                                                        # scattered ids, an exact count
        mask[rng.choice(n, _whole_parts(n, k, mb, fname == "parts+1"), replace=False)] = True
    return mask


@pytest.mark.parametrize("fname", ("none", "p0.5", "p0.1", "range", "parts", "parts+1"))
@pytest.mark.parametrize("dim", list(DIMS))
def test_multi_tile_parts_prune_and_certify(cph, oracle, monkeypatch, tmp_path_factory, dim, fname):
    w = _world(cph, oracle, monkeypatch, tmp_path_factory, dim)
    ix, Q, n = w["ix"], w["Q"], w["n"]
    ix.exact_engine = "matrix"
    for k in KS:
        mask = _mask(w, fname, k)
        allowed = _allowed(mask, n)
        m = len(allowed)
        pl = _plan(m, NQ, k, w["mb"])
        last = m - (pl["P"] - 1) * pl["part"]
        if fname in ("none", "range"):
            assert _multi_tile(pl, m, True), (fname, k, pl)
        elif fname == "parts":
            assert _multi_tile(pl, m, False) and last == pl["part"], (fname, k, pl)
        elif fname == "parts+1":
            assert _multi_tile(pl, m, False) and last == 1, (fname, k, pl)
        dist = w["dist"][:, allowed]
        need = _need(dist, k, w["eps"], pl)
        may_flag = int((need + 64 > pl["C"]).sum())
        if k != 64:
            assert may_flag == 0, ("bad input: queries that may need the fallback", dim, fname, k, int(need.max()), pl["C"])
        want_ids, want_d = _model(dist, allowed, k)
        f = None if mask is None else ix.make_filter(mask)
        ids, d = ix.search_batch(Q, k, filter=f, exact=True)
        st = ix.last_search_stats()
        print(f"dim {dim} {fname} k {k} m {m} P {pl['P']} part {pl['part']} tile_q {pl['tile_q']} need<= {int(need.max())} "
              f"may_flag {may_flag} survivors/(k nq) {st['matrix_survivors'] / (k * NQ):.3f} redo {st['matrix_redo']}")
        assert np.array_equal(ids, want_ids) and _beq(d, want_d), (dim, fname, k)
        assert st["matrix_parts"] == pl["P"], (dim, fname, k, st, pl)
        assert st["matrix_redo"] <= may_flag, (dim, fname, k, st)
        assert st["matrix_survivors"] >= k * (NQ - st["matrix_redo"]), (dim, fname, k, st)


@pytest.mark.parametrize("dim", list(DIMS))
def test_flags_land_on_their_own_query(cph, oracle, monkeypatch, tmp_path_factory, dim):
    """Four launches (q_first = 0, 128, 256, 384); a NaN query in wave 1 of the first, in wave 1 of the third and in the
    last row of the ragged fourth.  Those three are the fallback's, every other row is certified."""
    w = _world(cph, oracle, monkeypatch, tmp_path_factory, dim)
    ix, n, k = w["ix"], w["n"], 10
    pl = _plan(n, NQ, k, w["mb"])
    assert pl["tile_q"] == 128 and _multi_tile(pl, n, True)
    assert int((_need(w["dist"], k, w["eps"], pl) + 64 > pl["C"]).sum()) == 0
    bad = [37, 300, 399]
    Q = w["Q"].copy()
    Q[bad, 3] = np.nan
    ix.exact_engine = "vector"
    try:
        vids, vd = ix.search_batch(Q, k, exact=True)
    finally:
        ix.exact_engine = "matrix"
    ids, d = ix.search_batch(Q, k, exact=True)
    st = ix.last_search_stats()
    assert st["matrix_redo"] == 3 and st["matrix_parts"] == pl["P"], st
    assert np.array_equal(ids[bad], vids[bad]) and _beq(d[bad], vd[bad])
    good = np.setdiff1d(np.arange(NQ), bad)
    allowed = _allowed(None, n)
    want_ids, want_d = _model(w["dist"][good], allowed, k)
    assert np.array_equal(ids[good], want_ids) and _beq(d[good], want_d)


def test_fallback_beyond_wave_0(cph, oracle, monkeypatch, tmp_path_factory):
    """The duplicates of test_fallback_on_massive_duplicates at the multi-tile geometry: half the rows are one vector, and
    the queries 40..51 (wave 1 of the workgroup) lie near it and overflow their pools.  The other 116 are ordinary queries,
    but on this index they are the fallback's as well: the builder numbers neighbours next to each other, so whole parts
    hold nothing but copies, and in such a part the k-th of a prefix is a copy for EVERY query (the recorded run flagged all
    128).  What this test covers is therefore the flagged path at the multi-tile geometry -- flags raised from every wave
    and every part, the vector scan behind them, and under result_ids = "input" the row translation of the flagged merge.
    That certified rows keep their bytes beside flagged neighbours of the same tile is test_flags_land_on_their_own_query's
    to show."""
    n, mb = _geometry()
    rng = np.random.default_rng(55)
    X = rng.standard_normal((n, 24)).astype(np.float32)
    X[rng.choice(np.arange(1, n), 1299, replace=False)] = X[0]
    Q = rng.standard_normal((128, 24)).astype(np.float32)
    near = np.arange(40, 52)
    Q[near] = X[0] + 0.01 * Q[near]
    ix, p = _build(cph, monkeypatch, tmp_path_factory, X, 24, mb)
    oi = oracle.load(p)
    allowed = _allowed(None, n)
    pl = _plan(n, 128, 10, mb)
    assert _multi_tile(pl, n, True)
    dist = _all_distances(oi, Q, allowed)
    want_ids, want_d = _model(dist, allowed, 10)
    # the reference's verdict first: the twelve overflow a pool.  (So may an ordinary query: the builder numbers neighbours
    # next to each other, a part can hold nothing but copies, and then the k-th of its prefix is a copy for every query.)
    eps = slack_of(Q, X, 32)
    others = np.setdiff1d(np.arange(128), near)
    need = _need(dist, 10, eps, pl)
    may_flag = need + 64 > pl["C"]
    assert (need[near] > 1000).all(), ("bad input", need[near].min())
    ids, d = ix.search_batch(Q, 10, exact=True)
    st = ix.last_search_stats()
    print("duplicates:", pl, {key: st[key] for key in ("matrix_parts", "matrix_survivors", "matrix_redo")})
    assert 12 <= st["matrix_redo"] <= int(may_flag.sum()) and st["matrix_parts"] == pl["P"], (st, int(may_flag.sum()))
    assert np.array_equal(ids, want_ids) and _beq(d, want_d)
    # the ordinary queries on their own, at other rows of the tile and in another launch shape: the same rows
    oids, od = ix.search_batch(Q[others], 10, exact=True)
    assert ix.last_search_stats()["matrix_redo"] <= int(may_flag[others].sum())
    assert np.array_equal(oids, want_ids[others]) and _beq(od, want_d[others])
    rm = ix.row_map()
    ix.result_ids = "input"
    rids, rd = ix.search_batch(Q, 10, exact=True)
    assert ix.last_search_stats()["matrix_redo"] == st["matrix_redo"]
    assert np.array_equal(rids, rm[want_ids]) and _beq(rd, want_d)
