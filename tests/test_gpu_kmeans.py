"""CPIndex.kmeans: the matrix-core assignment, the vector kernel behind it and the deterministic update against a float64
Lloyd step over the stored rows.  Shapes are the edges of the kernel: 127 / 129 rows and centroids around the 128-wide
tiles, 300 for a third tile with a masked end, dim 10 (D = 16: the zero-filled half K chunk), 32 (one chunk), 96 (four
chunks) and 256 (eight)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLT_MAX = np.float32(3.4028234663852886e38)
_IX = {}


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _index(cph, dim, n):
    """Once per shape: blobs around n well-separated centres (row i belongs to centre i), built and finalized; the
    centres and the stored rows."""
    if (dim, n) not in _IX:
        rng = np.random.default_rng(100 * dim + n)
        centres = (8.0 * rng.standard_normal((n, dim))).astype(np.float32)
        ix = cph.CPIndex(dim, 4)
        ix.build(centres + 0.05 * rng.standard_normal((n, dim)).astype(np.float32))
        ix.finalize()
        _IX[dim, n] = ix, centres, ix.get_vectors(stored=True).astype(np.float64)
    return _IX[dim, n]


def _lloyd64(X, C, D):
    """float64 squared distances [n, k], and per row the gap under which the fp32 vector arithmetic may pick another
    centroid than float64: 2 (D / 8 + 8) u (|x|^2 + max |c|^2), the bound in the header of device_exact_mfma.h."""
    C = C.astype(np.float64)
    d = ((X[:, None, :] - C[None, :, :]) ** 2).sum(-1)
    return d, 2 * (D / 8 + 8) * U * ((X ** 2).sum(1) + (C ** 2).sum(1).max())


def _check_assign(assign, d, gap):
    """assign == float64 argmin on every row whose two best float64 distances are further apart than the gap; at most 1 %
    of the rows may be closer than that (a property of the inputs, checked first).  Returns the rows' float64 gaps."""
    s = np.sort(d, axis=1)
    gap64 = np.full(len(d), np.inf) if d.shape[1] == 1 else s[:, 1] - s[:, 0]
    sure = gap64 > gap
    print(f"undecided rows: {(~sure).sum()} of {len(d)}")
    assert (~sure).mean() <= 0.01, "the inputs leave too many rows undecided"
    assert np.array_equal(assign[sure], d.argmin(1)[sure])
    return gap64


CASES = [(dim, n, k) for dim in (10, 32, 96, 256) for n in (127, 129, 300) for k in (1, 2, 127, 129, 300) if k <= n]


@pytest.mark.parametrize("dim,n,k", CASES)
def test_one_step_against_float64(cph, dim, n, k):
    ix, centres, X = _index(cph, dim, n)
    D = max(16, 1 << (dim - 1).bit_length())
    # centroid c starts near centre c; the rows of the centres behind k fall wherever they are nearest
    C0 = (centres[:k] + 0.5 * np.random.default_rng(k).standard_normal((k, dim))).astype(np.float32)
    _, a0, dist0, counts0, moved0 = ix.kmeans(k, iters=0, init=C0)
    d0, gap0 = _lloyd64(X, C0, D)
    gap64 = _check_assign(a0, d0, gap0)
    # the matrix kernel certifies a row once its two best d^ are 2 eps apart, eps = (4.125 D + 24) u (|x|^2 + max |c|^2)
    # >= |d^ - d| and >= the centroid norms' own rounding: a float64 gap above 8 eps leaves more than 2 eps between them
    eps = (4.125 * D + 24) * U * gap0 / (2 * (D / 8 + 8) * U)
    passes, uncertain = ix.kmeans_stats()
    print(f"rows left to the vector kernel: {uncertain}")
    assert passes == 1 and uncertain <= (gap64 <= 8 * eps).sum()
    assert moved0.shape == (0,) and np.array_equal(counts0, np.bincount(a0, minlength=k))

    C1, a1, dist1, counts1, moved1 = ix.kmeans(k, iters=1, init=C0)
    assert C1.dtype == np.float32 and C1.shape == (k, dim) and a1.dtype == np.int32 and counts1.dtype == np.int64
    for c in range(k):                                       # the update: means under the assignment BEFORE it
        members = X[a0 == c]
        if len(members) == 0:
            assert C1[c].tobytes() == C0[c].tobytes()        # an empty cluster keeps its centroid
            continue
        tol = (len(members) + 2) * U * np.abs(members).mean(0)
        assert (np.abs(C1[c] - members.mean(0)) <= tol).all(), (c, len(members))
    d1, gap1 = _lloyd64(X, C1, D)
    _check_assign(a1, d1, gap1)
    assert np.array_equal(counts1, np.bincount(a1, minlength=k)) and counts1.sum() == n
    assert moved1.tolist() == [n]
    for a, dist, d, gap in ((a0, dist0, d0, gap0), (a1, dist1, d1, gap1)):
        assert (np.abs(dist - d[np.arange(n), a]) <= gap / 2).all()


def test_ties_and_the_uncertain_path(cph):
    """Equal distances go to the lowest centroid, in the vector kernel: rows that EQUAL two identical centroids have gap 0 and
    cannot be certified.  70 copies of a = e0, 70 of b = e1, 60 rows near g = 3 e2; every distance involved is exact."""
    dim = 16
    a, b, g = np.eye(dim, dtype=np.float32)[0], np.eye(dim, dtype=np.float32)[1], 3 * np.eye(dim, dtype=np.float32)[2]
    G = g + np.float32(2.0 ** -6) * np.random.default_rng(5).integers(-4, 5, (60, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 4)
    ix.build(np.concatenate([np.tile(a, (70, 1)), np.tile(b, (70, 1)), G]))
    ix.finalize()
    X = ix.get_vectors(stored=True)
    is_a, is_b = (X == a).all(1), (X == b).all(1)
    assert is_a.sum() == 70 and is_b.sum() == 70
    C0 = np.stack([a, a, b, g])
    C, assign, dist, counts, moved = ix.kmeans(4, iters=1, init=C0)
    assert np.array_equal(assign, np.where(is_a, 0, np.where(is_b, 2, 3)))
    assert counts.tolist() == [70, 0, 70, 60] and moved.tolist() == [200]
    assert C[0].tobytes() == a.tobytes() and C[1].tobytes() == a.tobytes() and C[2].tobytes() == b.tobytes()
    assert (dist[is_a | is_b] == 0).all()
    passes, uncertain = ix.kmeans_stats()
    assert passes == 2 and uncertain >= 2 * 70               # both passes sent the tied rows to the vector kernel
    # all live rows identical, two of three centroids equal to them: centroid 1, the lowest of the two
    ix.remove(np.flatnonzero(~is_a), ids="internal")
    C, assign, dist, counts, moved = ix.kmeans(3, iters=2, init=np.stack([b, a, a]))
    assert np.array_equal(assign, np.where(is_a, 1, -1)) and counts.tolist() == [0, 70, 0] and moved.tolist() == [70, 0]
    assert C.tobytes() == np.stack([b, a, a]).tobytes()
    assert (dist[is_a] == 0).all() and (dist[~is_a] == FLT_MAX).all()


def test_removed_and_added_rows(cph):
    dim, n, k = 24, 600, 8
    rng = np.random.default_rng(24)
    ix = cph.CPIndex(dim, 4)
    ix.build(rng.standard_normal((n, dim)).astype(np.float32))
    ix.finalize()
    gone = rng.choice(n, 300, replace=False)
    ix.remove(gone, ids="internal")
    tail = ix.add(3.0 + rng.standard_normal((40, dim)).astype(np.float32))
    X = ix.get_vectors(stored=True).astype(np.float64)
    live = np.ones(n + 40, bool)
    live[gone] = False
    # init=None: k distinct LIVE ids, the same for the same seed; iters=0 returns their stored rows
    picked = np.random.default_rng(3).choice(np.flatnonzero(live), size=k, replace=False)
    C, assign, dist, counts, _ = ix.kmeans(k, iters=0, seed=3)
    assert C.tobytes() == X[picked].astype(np.float32).tobytes()
    assert (assign[~live] == -1).all() and (dist[~live] == FLT_MAX).all() and (assign[live] >= 0).all()
    assert np.array_equal(counts, np.bincount(assign[live], minlength=k)) and counts.sum() == live.sum()
    d, gap = _lloyd64(X[live], C, 32)
    _check_assign(assign[live], d, gap)                      # the tail rows (the last 40 live ones) among them
    assert (assign[tail] >= 0).all()
    outs = [ix.kmeans(k, iters=3, seed=3) for _ in range(2)]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*outs))
    assert outs[0][4][0] == live.sum() and (outs[0][1][~live] == -1).all()


def test_determinism_and_the_device_form(cph):
    import torch
    dim, n, k = 32, 300, 5
    rng = np.random.default_rng(4)
    centres = (8.0 * rng.standard_normal((k, dim))).astype(np.float32)       # five separated blobs of 60 rows
    ix = cph.CPIndex(dim, 4)
    ix.build(np.repeat(centres, n // k, axis=0) + 0.5 * rng.standard_normal((n, dim)).astype(np.float32))
    ix.finalize()
    C0 = centres + np.float32(0.5)
    first, second = ix.kmeans(k, iters=5, init=C0), ix.kmeans(k, iters=5, init=C0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second))
    moved = first[4]
    assert moved[0] <= n and (np.diff(moved) <= 0).all() and moved[-1] == 0
    side = torch.cuda.Stream()
    outs = ix.kmeans_device(k, iters=5, init=C0, stream=side)
    side.synchronize()
    assert all(t.is_cuda for t in outs)
    assert all(x.tobytes() == t.cpu().numpy().tobytes() for x, t in zip(first, outs))


@pytest.mark.parametrize("case", ["ip", "partitioned", "k = 0", "k = live + 1", "init shape", "init nan", "iters < 0", "unfinalized"])
def test_refusals(cph, case):
    ix, centres, _ = _index(cph, 32, 127)
    good = centres[:3]
    call = {"ip": lambda: cph.CPIndex(32, 4, metric="ip").kmeans(3),
            "partitioned": lambda: cph.CPIndex(32, 4, devices=[0, 0], partition=True).kmeans(3),
            "k = 0": lambda: ix.kmeans(0),
            "k = live + 1": lambda: ix.kmeans(128),
            "init shape": lambda: ix.kmeans(3, init=good[:, :31]),
            "init nan": lambda: ix.kmeans(3, init=np.where(np.arange(32) == 7, np.nan, good).astype(np.float32)),
            "iters < 0": lambda: ix.kmeans(3, iters=-1, init=good),
            "unfinalized": lambda: cph.CPIndex(32, 4).kmeans(3)}[case]
    match = {"ip": 'metric="ip"', "partitioned": r"part\(i\)\.kmeans"}.get(case)
    with pytest.raises(ValueError, match=match):
        call()
