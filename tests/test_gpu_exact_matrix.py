"""The matrix engine of the exact scan (index.exact_engine = "matrix") against the ORACLE, as tests/test_gpu_exact.py tests
the vector engine: a row is the oracle's exact_l2 over the allowed ids, ordered by np.lexsort((ids, dist)), cut at k and
padded.  Ids and distance BYTES must be equal: the matrix cores only prune, the vector arithmetic forms every distance."""
import zlib

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path
from test_gpu_exact import CASES, _all_distances, _allowed, _beq, _load, _model
from exact_matrix_model import DEFAULT_BUDGET_MB, may_flag, plan, slack_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _matrix(cph, name, bits):
    ix = _load(cph, name, bits)
    ix.exact_engine = "matrix"
    return ix


@pytest.mark.parametrize("name,bits", CASES)
def test_every_dimension_ragged_tiles(cph, oracle, gold, name, bits):
    ix = _matrix(cph, name, bits)
    oi = oracle.load(fixture_path(name, bits))
    Q, n = gold[f"Q/{name}"], ix.size
    rng = np.random.default_rng(zlib.crc32(f"m{name}{bits}".encode()))
    one = np.zeros(n, bool)
    one[7] = True
    eps = slack_of(Q, ix.get_vectors(), DATASETS[name]["D"])
    for fname, mask in (("none", None), ("p0.5", rng.random(n) < 0.5), ("p0.1", rng.random(n) < 0.1), ("single", one)):
        allowed = _allowed(mask, n)
        dist = _all_distances(oi, Q, allowed)
        f = None if mask is None else ix.make_filter(mask)
        for k in (1, 10, 100, 1024):
            want_ids, want_d = _model(dist, allowed, k)
            ids, d = ix.search_batch(Q, k, filter=f, exact=True)
            st = ix.last_search_stats()
            print(name, fname, k, {key: st[key] for key in ("matrix_parts", "matrix_survivors", "matrix_redo")})
            assert np.array_equal(ids, want_ids) and _beq(d, want_d), (name, fname, k)
            if name == "g128" and mask is None:
                assert st["matrix_parts"] > 1
            if DATASETS[name]["kind"] == "gauss":
                # certified by the prefilter, not answered by the fallback behind it -- on inputs of which the reference
                # distances say that no pool can overflow (tests/exact_matrix_model.py)
                pl = plan(len(allowed), len(Q), k, DEFAULT_BUDGET_MB)
                assert not may_flag(dist, k, eps, pl).any(), ("bad input", name, fname, k)
                assert st["matrix_redo"] == 0 and st["matrix_parts"] == pl["P"], (name, fname, k, st, pl)


@pytest.mark.parametrize("k", (1, 32))
def test_four_query_tiles_of_self_matches(cph, oracle, k):
    import torch
    ix = _matrix(cph, "g128", 4)
    oi = oracle.load(fixture_path("g128", 4))
    Q = np.ascontiguousarray(ix.get_vectors())                 # 400 rows: three whole tiles of 128 and a ragged one
    allowed = _allowed(None, ix.size)
    want_ids, want_d = _model(_all_distances(oi, Q, allowed), allowed, k)
    assert (want_d[:, 0] <= 1e-4).all()
    ids, d = ix.search_batch(Q, k, exact=True)
    assert np.array_equal(ids, want_ids) and _beq(d, want_d)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    Qd = torch.from_numpy(Q).to(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    did, dd = ix.search_batch_device(Qd, k, stream=side, exact=True)
    ix.synchronize()
    assert np.array_equal(did.cpu().numpy(), want_ids) and _beq(dd.cpu().numpy(), want_d)


def test_scratch_follows_the_plan_of_every_batch(cph, oracle, monkeypatch):
    """One batch set, a pool budget of 1 MiB (read when the handle is made): 400 queries at k = 1024 are cut to launches
    of 128 queries with pools of 2,048 keys, the same 400 queries at k = 1 afterwards run 256 to a launch with pools of
    128 -- more queries per launch over FEWER pool keys.  Every scratch buffer has to follow its own size."""
    monkeypatch.setenv("CPH_EXACT_SCRATCH_MB", "1")
    ix = _matrix(cph, "g128", 4)
    ix.set_batch_sets(1)
    oi = oracle.load(fixture_path("g128", 4))
    Q = np.ascontiguousarray(ix.get_vectors())
    allowed = _allowed(None, ix.size)
    dist = _all_distances(oi, Q, allowed)
    for k in (1024, 1, 100):
        want_ids, want_d = _model(dist, allowed, k)
        ids, d = ix.search_batch(Q, k, exact=True)
        assert np.array_equal(ids, want_ids) and _beq(d, want_d), k


@pytest.mark.parametrize("name", ("g128", "g16"))
def test_near_ties_decide_the_order(cph, oracle, name):
    """Query i is the float32 midpoint of row i and its nearest neighbour: two candidates a few ulp apart, which the
    approximate distance cannot order.  The slack has to keep both, the re-score orders them."""
    bits = dict(CASES)[name]
    ix = _matrix(cph, name, bits)
    oi = oracle.load(fixture_path(name, bits))
    X = np.ascontiguousarray(ix.get_vectors())
    allowed = _allowed(None, ix.size)
    dx = _all_distances(oi, X, allowed)
    np.fill_diagonal(dx, np.inf)
    Q = ((X.astype(np.float64) + X[dx.argmin(1)]) / 2).astype(np.float32)
    dist = _all_distances(oi, Q, allowed)
    for k in (1, 2):
        want_ids, want_d = _model(dist, allowed, k)
        ids, d = ix.search_batch(Q, k, exact=True)
        assert np.array_equal(ids, want_ids) and _beq(d, want_d), (name, k)
        if k == 1:
            assert ix.last_search_stats()["matrix_survivors"] >= 1.5 * len(Q)


def test_fallback_on_massive_duplicates(cph, oracle, tmp_path):
    """600 rows of dim 24, 300 of them one vector: near it more candidates survive than a pool of k = 10 holds, the
    queries are flagged and the vector scan behind the matrix launches answers them.  A NaN query is flagged as well."""
    rng = np.random.default_rng(5)
    X = rng.standard_normal((600, 24)).astype(np.float32)
    X[300:] = X[0]
    Q = (X[0] + 0.01 * rng.standard_normal((12, 24))).astype(np.float32)
    Q[11] = rng.standard_normal(24)                             # one ordinary query among them
    ix = cph.CPIndex(24, 4)
    ix.build(X)
    ix.finalize()
    p = str(tmp_path / "dup.idx")
    ix.save(p)
    oi = oracle.load(p)
    allowed = _allowed(None, 600)
    want_ids, want_d = _model(_all_distances(oi, Q, allowed), allowed, 10)
    vids, vd = ix.search_batch(Q, 10, exact=True)
    Qn = Q.copy()
    Qn[3, 5] = np.nan
    nids, nd = ix.search_batch(Qn, 10, exact=True)
    ix.exact_engine = "matrix"
    ids, d = ix.search_batch(Q, 10, exact=True)
    st = ix.last_search_stats()
    assert st["matrix_redo"] > 0, st
    assert np.array_equal(ids, want_ids) and _beq(d, want_d)
    assert np.array_equal(ids, vids) and _beq(d, vd)
    ids, d = ix.search_batch(Qn, 10, exact=True)
    assert np.array_equal(ids, nids) and _beq(d, nd)


def test_default_engine_untouched(cph, gold):
    ix = _load(cph, "g128", 4)
    assert ix.exact_engine == "vector"
    ix.search_batch(gold["Q/g128"], 10, exact=True)
    assert not [key for key in ix.last_search_stats() if key.startswith("matrix")]
    with pytest.raises(ValueError):
        ix.exact_engine = "tensor"
