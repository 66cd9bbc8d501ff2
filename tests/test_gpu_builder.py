"""GPU tests of index construction: build()/finalize() of the drop-in.

The reference's own build is not reproducible across thread counts, so parity here
is (i) format/semantic: an index written by our builder loads in the compiled reference and the
reference's CPU search on it equals our GPU search bit for bit, and (ii) statistical: graph
quality (recall of the same search protocol) is not worse than the reference-built index'.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def sift_like(rng, n, dim, ncl):
    cent = rng.gamma(2, 15, (ncl, dim))
    X = cent[rng.integers(0, ncl, n)] + rng.normal(0, 12, (n, dim))
    return np.clip(np.round(X), 0, 218).astype(np.float32), cent


def brute_topk(X, Q, k):
    d = (Q ** 2).sum(1)[:, None] + (X ** 2).sum(1)[None, :] - 2.0 * Q.astype(np.float64) @ X.T.astype(np.float64)
    return np.argsort(d, axis=1)[:, :k]


def dedup_recall(ids, raw_of_id, gt_rows, X, k=10):
    """recall@k of the first k unique returned ids (ids are internal, with dups)."""
    hits = 0
    for q in range(len(ids)):
        seen, uniq = set(), []
        for i in ids[q]:
            if i >= 0 and i not in seen:
                seen.add(i)
                uniq.append(i)
            if len(uniq) == k:
                break
        got = {raw_of_id[i] for i in uniq}
        hits += len(got & set(gt_rows[q][:k].tolist()))
    return hits / (len(ids) * k)


def index_rows(path, n, dim, D):
    """internal id -> input row, recovered from the raw vectors stored in the file."""
    off = 68 + 248 + 72 + dim * 4 + n * 4 + n * 4
    raw = np.fromfile(path, dtype=np.float32, count=n * D, offset=off).reshape(n, D)[:, :dim]
    return raw


ENC_SHAPES = ((10, 16), (50, 64), (96, 128), (128, 128), (300, 512), (960, 1024), (24, 32), (200, 256), (1536, 2048))


@pytest.mark.parametrize("dim,D", ENC_SHAPES)
@pytest.mark.parametrize("bits", [1, 2, 4])
def test_gpu_edge_encoder_matches_reference(oracle, dim, D, bits):
    """The kernel finalize() encodes every edge with (one lane per edge, sequential coordinate descent on
    LDS rows) against what the reference's encoder computed for the same parent / neighbours: code values,
    nop, ip_qo, ip_cp (float bits) and both popcounts -- including an exact-duplicate neighbour (nop = 0)."""
    import cphnsw_mi355x
    from golden_util import enc_golden
    P, N, V, A, S = enc_golden(dim, D, bits)
    for c in range(len(P)):
        p, nb = P[c], N[c]
        v, a, s = cphnsw_mi355x.encode_edges(p, nb, bits)
        assert np.array_equal(v, V[c]), (dim, bits, c, int((v != V[c]).sum()))
        assert a.tobytes() == A[c].tobytes(), (dim, bits, c)
        assert np.array_equal(s, S[c])
        # fewer than 32 edges, and the oracle on fresh inputs
        rng = np.random.default_rng(c + dim)
        m = int(rng.integers(1, 32))
        p2 = rng.standard_normal(dim).astype(np.float32)
        nb2 = (p2 + 0.5 * rng.standard_normal((m, dim))).astype(np.float32)
        v2, a2, s2 = cphnsw_mi355x.encode_edges(p2, nb2, bits)
        ov, oa, os_ = oracle.encode_edges(p2, nb2, D, bits)
        assert np.array_equal(v2, ov) and a2.tobytes() == oa.tobytes() and np.array_equal(s2, os_)


def test_knn_queries_against_base():
    import cphnsw_mi355x
    rng = np.random.default_rng(8)
    X = rng.standard_normal((5000, 96)).astype(np.float32)
    Q = rng.standard_normal((300, 96)).astype(np.float32)
    ids, d = cphnsw_mi355x.knn_bruteforce(X, queries=Q)
    D2 = ((Q[:, None, :].astype(np.float64) - X[None, :, :]) ** 2).sum(-1)
    want = np.sort(D2, axis=1)[:, :32]
    assert ids.shape == (300, 32) and np.allclose(d, want, rtol=1e-4, atol=1e-3)
    assert np.allclose(np.take_along_axis(D2, ids.astype(np.int64), axis=1), want, rtol=1e-4, atol=1e-3)
    # fewer base rows than neighbours asked for: padded
    ids, d = cphnsw_mi355x.knn_bruteforce(X[:20], queries=Q[:3])
    assert (ids[:, 20:] == 0xFFFFFFFF).all() and (ids[:, :20] < 20).all()


def test_knn_bruteforce_is_exact():
    import cphnsw_mi355x
    rng = np.random.default_rng(3)
    for n, dim in ((1000, 128), (777, 96), (300, 10)):
        X = rng.standard_normal((n, dim)).astype(np.float32)
        ids, d = cphnsw_mi355x.knn_bruteforce(X)
        D2 = ((X[:, None, :].astype(np.float64) - X[None, :, :]) ** 2).sum(-1)
        np.fill_diagonal(D2, np.inf)
        want = np.sort(D2, axis=1)[:, :32]
        assert np.allclose(d, want, rtol=1e-4, atol=1e-3), (n, dim)
        got = np.take_along_axis(D2, ids.astype(np.int64), axis=1)
        assert np.allclose(got, want, rtol=1e-4, atol=1e-3)
        assert (ids != np.arange(n)[:, None]).all()


@pytest.mark.parametrize("n,dim,kind", [(40_000, 96, "gauss"), (33_000, 128, "clustered"), (36_001, 200, "gauss"), (33_000, 64, "dups")])
def test_knn_symmetric_self_join_is_exact(n, dim, kind, tmp_path):
    """From 32,768 rows on the self-join computes every tile of the distance matrix once (device_knn_sym.h: thresholds
    from a 1/16 sample, both sides of a tile appended to per-row buffers, selection, exact fallback for the rows whose
    threshold was too tight).  Checked against float64 on a sample of rows -- distances, the distances of the returned
    ids, no self, ascending order -- and against the two-pass kernel (CPH_KNN_SYM=0 in a child process: the switch is
    read once per process): the same id lists wherever the 32nd and 33rd distances are not (nearly) tied."""
    import subprocess, sys, os
    import cphnsw_mi355x
    rng = np.random.default_rng(n + dim)
    if kind == "gauss":
        X = rng.standard_normal((n, dim)).astype(np.float32)
    elif kind == "dups":
        # 500 distinct vectors, 66 copies of each: thresholds of zero or of a whole cluster, tiles with thousands of passing
        # pairs (the LDS queue overflows into direct appends), per-row buffers that overflow (fallback for most rows)
        X = np.repeat(rng.standard_normal((500, dim)).astype(np.float32), 66, axis=0)[rng.permutation(n)]
    else:
        X, _ = sift_like(rng, n, dim, 300)
    ids, d = cphnsw_mi355x.knn_bruteforce(X)
    assert (ids != np.arange(n, dtype=np.uint32)[:, None]).all() and (ids < n).all()
    assert (np.diff(d, axis=1) >= 0).all()
    rows = rng.integers(0, n, 300)
    X64 = X.astype(np.float64)
    for r in rows:
        dd = ((X64 - X64[r]) ** 2).sum(1)
        dd[r] = np.inf
        want = np.sort(dd)[:32]
        assert np.allclose(d[r], want, rtol=1e-4, atol=1e-3), (r, d[r][:4], want[:4])
        assert np.allclose(dd[ids[r].astype(np.int64)], want, rtol=1e-4, atol=1e-3), r
        assert len(set(ids[r].tolist())) == 32
        if kind == "dups":
            assert (dd[ids[r].astype(np.int64)] < 1e-3).all()      # 65 copies of itself to choose from
    # the two-pass kernel on the same input
    np.save(tmp_path / "x.npy", X)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import cphnsw_mi355x; X = np.load(%r); "
            "i, d = cphnsw_mi355x.knn_bruteforce(X); np.save(%r, i); np.save(%r, d)"
            % (os.path.dirname(os.path.dirname(cphnsw_mi355x.__file__)), str(tmp_path / "x.npy"), str(tmp_path / "i.npy"), str(tmp_path / "d.npy")))
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, CPH_KNN_SYM="0"))
    ids0, d0 = np.load(tmp_path / "i.npy"), np.load(tmp_path / "d.npy")
    assert np.allclose(d, d0, rtol=1e-5, atol=1e-3)
    differ = (ids != ids0).any(axis=1)
    if kind == "gauss":
        assert differ.mean() < 1e-2, differ.mean()          # only where two distances round differently around rank 32
    for r in np.nonzero(differ)[0][:300]:                   # a different id must be a tie within float32 rounding, never a farther row
        dd = ((X64 - X64[r]) ** 2).sum(1)
        dd[r] = np.inf
        want = np.sort(dd)[:32]
        for got in (ids[r], ids0[r]):
            assert np.allclose(np.sort(dd[got.astype(np.int64)]), want, rtol=1e-5, atol=1e-4), (r, kind)


@pytest.mark.parametrize("bits,n,dim", [(1, 6000, 128), (2, 6000, 128), (4, 6000, 128), (4, 2500, 960),
                                        (2, 3000, 96), (4, 1200, 10),
                                        # the generic search instantiation: D = 32, 256, 512 and 2048, with dims
                                        # far below D and (500, 2000) within its last 128 padded dims
                                        (4, 1500, 24), (1, 1200, 200), (2, 1000, 300), (2, 600, 1536), (4, 600, 1536),
                                        (2, 800, 500), (1, 500, 2000)])
def test_built_index_is_valid_for_reference_and_search_matches(tmp_path, bits, n, dim):
    import cphnsw_mi355x
    from oracle_lib import Oracle, ref_available, ref_module
    rng = np.random.default_rng(11 + bits + dim)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((48, dim)).astype(np.float32)
    ix = cphnsw_mi355x.CPIndex(dim, bits)
    assert ix.size == 0 and not ix.is_finalized
    ix.build(X)
    assert ix.size == n and not ix.is_finalized
    ix.finalize()
    assert ix.is_finalized and ix.size == n
    p = str(tmp_path / f"mine_{bits}.idx")
    ix.save(p)
    for k in (10, 50):
        ids, d = ix.search_batch(Q, k)
        oi = Oracle().load(p)
        oids, od, _ = oi.search_batch(Q, k)
        assert np.array_equal(ids, oids) and d.tobytes() == od.tobytes()
        if ref_available():
            r = ref_module().CPIndex(dim, bits)
            r.load(p)                                   # the reference accepts our file
            rids, rd = r.search_batch(Q, k)
            assert np.array_equal(ids, rids) and d.tobytes() == rd.tobytes()
    # a saved index round-trips through our own loader
    ix2 = cphnsw_mi355x.CPIndex(dim, bits)
    ix2.load(p)
    ids2, d2 = ix2.search_batch(Q, 10)
    ids1, d1 = ix.search_batch(Q, 10)
    assert np.array_equal(ids1, ids2) and d1.tobytes() == d2.tobytes()


def quality_data_20k():
    """Clustered, integer-valued 20k x 128 with 200 queries near the cluster centres."""
    rng = np.random.default_rng(5)
    X, cent = sift_like(rng, 20000, 128, 20)
    Q = (cent[rng.integers(0, 20, 200)] + rng.normal(0, 12, (200, 128))).astype(np.float32)
    return X, Q


def quality_data_100k():
    """BASELINE.md 2.2's generator at 100k x 128 (1,000 clusters), 300 integer-valued queries."""
    rng = np.random.default_rng(11)
    n, dim, nq = 100_000, 128, 300
    X, cent = sift_like(rng, n, dim, 1000)
    Q = np.clip(np.round(cent[rng.integers(0, 1000, nq)] + rng.normal(0, 12, (nq, dim))), 0, 218).astype(np.float32)
    return X, Q


def input_rows(path, X):
    """internal id -> input row of every vertex of an index over X (duplicates map to any equal row: distances equal)."""
    n, dim = X.shape
    raw = index_rows(path, n, dim, 128)
    key = {X[i].tobytes(): i for i in range(n)}
    return [key[raw[i].tobytes()] for i in range(n)]


def reference_recall(name):
    """What the compiled reference's own build + search reached on the same seeded data (tests/golden/make_golden_quality.py)."""
    import json
    from golden_util import GOLDEN_DIR
    with open(os.path.join(GOLDEN_DIR, "ref_graph_quality.json")) as f:
        return json.load(f)[name]


def test_graph_quality_not_worse_than_reference(tmp_path):
    import cphnsw_mi355x
    X, Q = quality_data_20k()
    dim, bits = X.shape[1], 4
    gt = brute_topk(X, Q, 10)
    mine = cphnsw_mi355x.CPIndex(dim, bits)
    mine.build(X)
    mine.finalize()
    pm = str(tmp_path / "mine.idx")
    mine.save(pm)
    ids_m, _ = mine.search_batch(Q, 20)
    rec_m = dedup_recall(ids_m, input_rows(pm, X), gt, X)
    rec_r = reference_recall("q20k_b4")["k20"]
    print("recall@10 (dedup of k=20): ours", rec_m, "reference", rec_r)
    assert rec_m >= rec_r - 0.05


def test_graph_quality_at_benchmark_scale_tracks_the_reference(tmp_path):
    """The gate that would catch a graph-quality regression at a size that is benchmarked: clustered, integer-valued
    100k x 128 at 4 bits (BASELINE.md 2.2's generator: 1,000 clusters), built by this repo's GPU builder, against what
    the compiled reference's build reached on the same data (it can finalize up to ~230k vertices, finding F9; stored
    in tests/golden/ref_graph_quality.json); same search protocol on both; dedup recall@10 of k = 20 and of k = 100
    must be within 0.03 of the reference's."""
    import cphnsw_mi355x
    X, Q = quality_data_100k()
    dim, bits = X.shape[1], 4
    gt = brute_topk(X, Q, 10)
    mine = cphnsw_mi355x.CPIndex(dim, bits)
    mine.build(X)
    mine.finalize()
    pm = str(tmp_path / "mine.idx")
    mine.save(pm)
    rm = input_rows(pm, X)
    ref = reference_recall("q100k_b4")
    for k in (20, 100):
        ids_m, _ = mine.search_batch(Q, k)
        rec_m = dedup_recall(ids_m, rm, gt, X)
        rec_r = ref[f"k{k}"]
        print(f"100k clustered, 4-bit: dedup recall@10 of k={k}: ours {rec_m:.4f}, reference {rec_r:.4f}")
        assert rec_m >= rec_r - 0.03, (k, rec_m, rec_r)
    # an index of this size (n + 1 beyond the default per-slot capacity) is where the copy-free small-batch path runs:
    # a handful of queries go straight onto the full-capacity slots, read and written over PCIe by the kernels
    ids_b, d_b = mine.search_batch(Q, 20)
    ids5, d5 = mine.search_batch(Q[:5], 20)
    assert np.array_equal(ids5, ids_b[:5]) and d5.tobytes() == d_b[:5].tobytes()
    for qi in (7, 8, 299):
        i1, d1 = mine.search(Q[qi], 20)
        m = int((ids_b[qi] >= 0).sum())
        assert np.array_equal(i1, ids_b[qi, :m]) and d1.tobytes() == d_b[qi, :m].tobytes()
    ids32, d32 = mine.search_batch(Q[100:132], 100)
    ids_k100, d_k100 = mine.search_batch(Q, 100)
    assert np.array_equal(ids32, ids_k100[100:132]) and d32.tobytes() == d_k100[100:132].tobytes()


@pytest.mark.parametrize("bits", [1, 2, 4])
def test_small_batch_path_equals_the_batch_path(bits):
    """Batches of up to 32 queries on an index beyond the default slot capacity take the copy-free path: one launch on the
    full-capacity slots, queries read and results written by the kernels over PCIe (cphnsw_mi355x.hip, Launch::Direct).
    Ids and distance bits must equal what the same queries get inside a large batch (the path the oracle and the
    reference pin), for every code width and for `search`."""
    import cphnsw_mi355x
    rng = np.random.default_rng(40 + bits)
    n, dim, nq = 70_000, 128, 200
    X, cent = sift_like(rng, n, dim, 700)
    Q = np.clip(np.round(cent[rng.integers(0, 700, nq)] + rng.normal(0, 12, (nq, dim))), 0, 218).astype(np.float32)
    ix = cphnsw_mi355x.CPIndex(dim, bits)
    ix.build(X)
    ix.finalize()
    for k in (10, 100):
        ids_b, d_b = ix.search_batch(Q, k)
        for lo, hi in ((0, 1), (1, 8), (8, 40)):
            ids_s, d_s = ix.search_batch(Q[lo:hi], k)
            assert np.array_equal(ids_s, ids_b[lo:hi]) and d_s.tobytes() == d_b[lo:hi].tobytes(), (bits, k, lo, hi)
        for qi in (41, 42, 199):
            i1, d1 = ix.search(Q[qi], k)
            m = int((ids_b[qi] >= 0).sum())
            assert np.array_equal(i1, ids_b[qi, :m]) and d1.tobytes() == d_b[qi, :m].tobytes(), (bits, k, qi)


def test_build_errors():
    import cphnsw_mi355x
    ix = cphnsw_mi355x.CPIndex(128, 4)
    with pytest.raises(RuntimeError, match="Cannot finalize an empty index"):
        ix.finalize()
    with pytest.raises(ValueError, match=r"vectors must be a \(n, dim\) float32 array"):
        ix.build(np.zeros((10, 64), np.float32))
    with pytest.raises(ValueError, match="at least one vector"):
        ix.build(np.zeros((0, 128), np.float32))
    ix.build(np.random.default_rng(0).standard_normal((30, 128)).astype(np.float32))
    with pytest.raises(RuntimeError, match="at least 50 nodes"):
        ix.finalize()


@pytest.mark.parametrize("D,n_rev,R,seed", [(128, 0, 32, 1), (128, 40, 32, 2), (128, 96, 32, 3), (16, 96, 18, 4), (1024, 60, 32, 5),
                                            (64, 96, 24, 6), (128, 10, 8, 7)])
def test_select_kernel_matches_the_rule_on_fixed_candidates(cph, oracle, D, n_rev, R, seed):
    """select_kernel (device_build.h) on one vertex with a given candidate list against the oracle's restatement of
    select_neighbors_alpha_cng (graph/neighbor_selection.hpp:21-88): the selected id LIST must be identical -- order
    included -- for clustered data (occlusions happen), repeated candidates, the vertex itself among the candidates,
    empty forward slots, error margins, equal distances (integer-valued rows) and lists shorter than R."""
    rng = np.random.default_rng(seed)
    n = 400
    cent = rng.normal(0, 4, (6, D))
    x = (cent[rng.integers(0, 6, n)] + rng.normal(0, 1, (n, D))).astype(np.float32)
    if seed % 2 == 0:
        x = np.round(x)                                  # ties in the distances
    for trial in range(6):
        v = int(rng.integers(0, n))
        fwd = rng.choice(n, 32, replace=False).astype(np.uint32)
        fwd[rng.integers(0, 32, 3)] = 0xFFFFFFFF          # empty slots
        fwd[5] = v                                        # the vertex itself
        rev = rng.choice(n, n_rev, replace=False).astype(np.uint32) if n_rev else np.zeros(0, np.uint32)
        if n_rev >= 4:
            rev[:2] = fwd[fwd != 0xFFFFFFFF][:2]          # ids that appear twice
        err = None if trial % 2 == 0 else np.abs(rng.normal(0, 0.3, n)).astype(np.float32)
        alpha, tau, amax = (1.2, 0.5, 0.0) if trial < 3 else (1.05, 2.0, 1.6)
        got = cph.select_neighbors_debug(x, v, fwd, rev, R, alpha, tau, amax, err)
        want = oracle.select_neighbors(x, v, np.concatenate([fwd, rev]), R, alpha, tau, amax, err)
        assert np.array_equal(got, want), (D, n_rev, R, trial, got, want)
        assert len(got) <= R and v not in got and len(set(got.tolist())) == len(got)


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g128", 2), ("g128", 1), ("sift96", 4), ("g16", 2), ("g1024", 2)])
def test_calib_kernel_records_match_the_oracle(cph, gold, name, bits):
    """calib_kernel's per-sample record on reference-built fixtures -- greedy hop, raw FastScan estimator term,
    floored ip_qo, exact <q - p, o - p> / nop and |q - o|^2 per edge -- against the oracle's block functions, bit for bit."""
    from golden_util import DATASETS, fixture_path
    from oracle_lib import Oracle
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits))
    oi = Oracle().load(fixture_path(name, bits))
    Q = gold[f"Q/{name}"]
    rng = np.random.default_rng(7)
    start = rng.integers(0, DATASETS[name]["n"], len(Q)).astype(np.uint32)
    rec, cnt, dqp = ix.calib_samples_debug(Q, start)
    for i in range(len(Q)):
        orec, ocnt, odqp = oi.calib_record(Q[i], start[i])
        assert cnt[i] == ocnt and dqp[i].tobytes() == odqp.tobytes(), (i, cnt[i], ocnt, dqp[i], odqp)
        assert rec[i, :ocnt].tobytes() == orec[:ocnt].tobytes(), (i, np.argwhere(rec[i, :ocnt] != orec[:ocnt])[:4])
