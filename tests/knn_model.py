"""The float64 judge of the exact-kNN kernels and of their host statement, and the cases both tiers run.

Three parties: the kernels (device_knn.h, device_knn_sym.h), their host statement in float32 (csrc/host_knn.h behind
cph_host_knn, which the kernels must equal byte for byte), and this module, which shares no arithmetic with either: squared
distances in float64 from the float32 inputs and a bound on what float32 may have lost.

The bound.  u = 2^-24, dim = the row length, D = max(32, next power of two >= dim), gamma_m = m u / (1 - m u).  The two-pass
kernel returns fl(nq - 2 s) with
    nq = a chain of dim fmafs for |q|^2                 |nq - |q|^2|  <= gamma_dim |q|^2
    nb = the same for |b|^2                             |nb - |b|^2|  <= gamma_dim |b|^2
    s  = a chain of D fmafs from -nb / 2 (exact) over q_k b_k: D roundings, each relative to a partial sum of terms whose
         absolute values add up to at most nb / 2 + S, S = sum_k |q_k b_k|
                                                        |s - (q.b - nb / 2)|  <= gamma_D (nb / 2 + S)
so before the last rounding the value is off by at most
    gamma_dim |q|^2 + gamma_dim |b|^2 + 2 gamma_D ((1 + gamma_dim) |b|^2 / 2 + S)  <=  gamma_D' (|q|^2 + 2 |b|^2 + 2 S)
with D' a little over D, and the last rounding adds u times a value that is itself at most |q|^2 + 2 |b|^2 + 2 S (up to the
same factor).  With m u / (1 - m u) <= m u (1 + D u / (1 - D u)) the sum is below
    tol(q, b) = (D + 4) u (|q|^2 + 2 |b|^2 + 2 S)
for every D <= 2048: D + 1 roundings of weight u, and three more units of u for the slack terms D u / (1 - D u) <= 2^-13 and
the (1 + gamma) factors, which together stay below 3 u as long as (D + 1) * 2^-12 < 3.  The clamp max(0, .) moves a value
towards the true distance, which is never negative.  The join returns fl(-2 acc + fl(nr + nc)): the D-term chain from zero
(at most gamma_D S, doubled), the two norm chains, one rounding of the sum of the norms and one of the result -- fewer terms
of the same sum, under the same bound.  The float64 side uses |q|^2 + |b|^2 - 2 q.b by matrix products; its own error is
below (D + 3) 2^-53 of the same sum, 2^-29 of tol.

Per row (check_lists): ids distinct, below nb, never self and never a row that holds a NaN; exactly min(32, eligible) valid
entries, then padding; |dist - d64| <= tol; distances ascend; RANKING: max over listed of (d64 - tol) <= min over eligible
unlisted of (d64 + tol); for byte-identical base rows i < j, j listed implies i listed before it.
"""
import ctypes as C
import functools

import numpy as np

from golden_util import sift_like

PAD = 0xFFFFFFFF
FMAX = np.float32(3.402823466e+38)
U = 2.0 ** -24


def padded_dim(dim):
    D = 32
    while D < dim:
        D *= 2
    return D


def host_knn(X, Q=None, q_ids=None, path=0):
    """cph_host_knn: (ids u32[rows, 32], dist f32[rows, 32], fallback rows, candidates per row of the join or None)."""
    from cphnsw_mi355x import _lib
    X = np.ascontiguousarray(X, np.float32)
    n, dim = X.shape
    Q = None if Q is None else np.ascontiguousarray(Q, np.float32)
    qi = None if q_ids is None else np.ascontiguousarray(q_ids, np.uint32)
    rows = n if Q is None else len(Q)
    ids = np.full((rows, 32), 0xA5A5A5A5, np.uint32)
    dist = np.full((rows, 32), -7, np.float32)
    cand = np.zeros(n, np.uint32) if path == 1 else None
    redo = C.c_uint32(0)
    _lib.check(_lib.lib().cph_host_knn(X.ctypes.data, n, dim, None if Q is None else Q.ctypes.data, 0 if Q is None else len(Q),
                                       None if qi is None else qi.ctypes.data, 0 if qi is None else 1, path, ids.ctypes.data,
                                       dist.ctypes.data, C.byref(redo), None if cand is None else cand.ctypes.data))
    return ids, dist, int(redo.value), cand


def reference(X, Q=None):
    """(d64[rows, nb], tol[rows, nb]) in float64; Q = None: X against itself."""
    X64 = np.asarray(X, np.float64)
    Q64 = X64 if Q is None else np.asarray(Q, np.float64)
    D = padded_dim(X64.shape[1])
    with np.errstate(invalid="ignore"):
        bn, qn = (X64 ** 2).sum(1), (Q64 ** 2).sum(1)
        d64 = qn[:, None] + bn[None, :] - 2.0 * (Q64 @ X64.T)
        tol = (D + 4) * U * (qn[:, None] + 2.0 * bn[None, :] + 2.0 * (np.abs(Q64) @ np.abs(X64).T))
    return d64, tol


def check_lists(ids, dist, d64, tol, self_col=None, base=None):
    """The per-row assertions of the module docstring on EVERY row.  self_col[rows]: the column a row must not list."""
    nq, nb = d64.shape
    assert ids.shape == (nq, 32) and dist.shape == (nq, 32) and ids.dtype == np.uint32 and dist.dtype == np.float32
    rows = np.arange(nq)[:, None]
    elig = np.isfinite(d64)                                   # a row with a NaN is nobody's neighbour and has none
    if self_col is not None:
        elig[np.arange(nq), np.asarray(self_col, np.int64)] = False
    valid = ids != PAD
    assert (valid.sum(1) == np.minimum(32, elig.sum(1))).all(), "number of valid entries"
    assert (valid[:, :-1] >= valid[:, 1:]).all(), "padding only at the end"
    assert (dist[~valid] == FMAX).all(), "padded distances"
    assert (ids[valid] < nb).all(), "id out of range"
    safe = np.where(valid, ids, 0).astype(np.int64)
    assert elig[rows, safe][valid].all(), "self or a NaN row listed"
    s = np.sort(np.where(valid, safe, -1 - np.arange(32)[None, :]), axis=1)
    assert (np.diff(s, axis=1) != 0).all(), "an id listed twice"
    err = np.abs(dist.astype(np.float64) - d64[rows, safe])
    assert (err[valid] <= tol[rows, safe][valid]).all(), ("distance off", float((err / np.maximum(tol[rows, safe], 1e-300))[valid].max()))
    assert (np.diff(dist.astype(np.float64), axis=1) >= 0).all(), "distances do not ascend"
    listed = np.zeros((nq, nb), bool)
    listed[np.broadcast_to(rows, ids.shape)[valid], safe[valid]] = True
    lo = np.where(listed, d64 - tol, -np.inf).max(1)
    hi = np.where(elig & ~listed, d64 + tol, np.inf).min(1)
    assert (lo <= hi).all(), ("a nearer row was left out", np.nonzero(lo > hi)[0][:5])
    if base is not None:
        pos = np.full((nq, nb), 99, np.int64)
        pos[np.broadcast_to(rows, ids.shape)[valid], safe[valid]] = np.broadcast_to(np.arange(32)[None, :], ids.shape)[valid]
        b = np.ascontiguousarray(base, np.float32)
        _, inv, cnt = np.unique(b.view(np.uint8).reshape(len(b), -1), axis=0, return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        for g in np.nonzero(cnt > 1)[0]:
            m = np.nonzero(inv == g)[0]                                   # ascending ids of one group of identical rows
            P = np.where(pos[:, m] < 99, pos[:, m], 100 + np.arange(len(m))[None, :])
            P = np.where(elig[:, m], P, -1)
            prev = np.concatenate([np.full((nq, 1), -1), np.maximum.accumulate(P, axis=1)[:, :-1]], axis=1)
            assert (P > prev)[elig[:, m]].all(), ("identical rows out of id order", m[:4])


def same_bytes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the cases -----------------------------------------------------------------------------------------------------------------
def _gauss(seed, n, dim):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


class Case:
    def __init__(self, X, Q=None, q_ids=None, path=0, blocks=0, launches=None, **promise):
        self.X, self.Q, self.q_ids, self.path, self.blocks, self.launches, self.promise = X, Q, q_ids, path, blocks, launches, promise
        self.X.setflags(write=False)
        if Q is not None:
            self.Q.setflags(write=False)

    @property
    def self_col(self):
        if self.Q is None:
            return np.arange(len(self.X))
        return None if self.q_ids is None else np.asarray(self.q_ids, np.int64)


NB_EDGES = (1, 2, 20, 31, 32, 33, 64, 65, 127, 128, 129, 255, 256, 257, 385)
NQ_EDGES = (1, 127, 128, 129, 257)
DIMS = (1, 10, 32, 33, 96, 200)
JOIN_PLAIN = {  # name: (n, dim, kind): even and odd block counts, a middle block, a last block of 1 and of 127 rows; D = 64, 128, 256
    "join_1024_d64_gauss": (1024, 64, "gauss"), "join_1025_d128_gauss": (1025, 100, "gauss"), "join_1151_d256_gauss": (1151, 200, "gauss"),
    "join_1152_d64_ints": (1152, 48, "ints"), "join_1153_d128_ints": (1153, 128, "ints"), "join_1409_d256_ints": (1409, 160, "ints"),
    "join_1409_d64_gauss": (1409, 40, "gauss"), "join_1024_d2048_gauss": (1024, 1536, "gauss"),
}


def _descending(D, reverse=False):
    # column j = 0.37 (400 - j) e_0: every column nearer to a query on the negative e_0 axis than all before it; the
    # queries differ in where they sit on the axis and carry a part orthogonal to every column (a constant in every distance)
    nb, nq = 400, 40
    X = np.zeros((nb, D), np.float32)
    X[:, 0] = (np.float32(0.37) * (nb - np.arange(nb))).astype(np.float32)
    if reverse:
        X = X[::-1].copy()
    Q = (0.05 * _gauss(D + 7, nq, D)).astype(np.float32)
    Q[:, 0] = -np.float32(0.25) * np.arange(nq)
    return Case(X, Q, order="ascending" if reverse else "descending")


def _identical():
    X = np.repeat(_gauss(21, 1, 24), 200, axis=0)
    return X


def _scattered_copies():
    rng = np.random.default_rng(40)
    X = rng.standard_normal((500, 48)).astype(np.float32)
    at = np.sort(np.concatenate([rng.choice(116, 10, replace=False) + 128 * t for t in range(4)]))      # ten in each of four tiles
    v = rng.standard_normal(48).astype(np.float32)
    X[at] = v
    Q = (v[None, :] + 0.01 * rng.standard_normal((20, 48))).astype(np.float32)
    return Case(X, Q, copies=at)


def _three_copies():
    rng = np.random.default_rng(257)
    V = rng.standard_normal((64, 40)).astype(np.float32)
    X = np.concatenate([np.repeat(V, 4, axis=0)[rng.permutation(256)], V[:1]])       # row 256: alone in the last tile
    return Case(X, copies_each=3)


def _large_norms():
    rng = np.random.default_rng(128)
    X = sift_like(rng, 400, 128)
    src = rng.choice(400, 100, replace=False)
    for a, b in zip(src[:50], src[50:]):                                             # 50 rows one step from another row
        X[a] = X[b]
        j = int(rng.integers(0, 128))
        X[a, j] += 1.0 if X[a, j] < 218 else -1.0
    return Case(X, near=src[:50], near_of=src[50:])


def _q_ids():
    rng = np.random.default_rng(130)
    X = rng.standard_normal((300, 72)).astype(np.float32)
    sel = rng.permutation(300)[:130].astype(np.uint32)
    sel[77] = sel[3]                                                                  # a repeated id; a permutation is not monotone
    assert (np.diff(sel.astype(np.int64)) < 0).any() and len(set(sel.tolist())) == 129
    return Case(X, X[sel].copy(), q_ids=sel)


def _join_data(n, dim, kind):
    rng = np.random.default_rng(n * 7 + dim)
    if kind == "gauss":
        return rng.standard_normal((n, dim)).astype(np.float32)
    if kind == "ints":
        return sift_like(rng, n, dim, 12)
    if kind == "dups":          # 4 vectors, 300 copies of each: every threshold is zero, every row has 299 candidates at distance zero
        return np.repeat(rng.standard_normal((4, dim)).astype(np.float32), 300, axis=0)[rng.permutation(1200)]
    if kind == "outlier":
        # 1,200 clustered rows and 20 rows far from them and (less far) from each other, all 20 of them rows of the join's sample
        # (ids 0, 16, 32, ...): a far row's eight nearest sample rows are far rows, its threshold holds fewer than 32 rows; the
        # clustered rows are left with 57 sample rows for 1,200, and the thresholds of some hold more than 256
        X = sift_like(rng, 1220, dim, 12)
        far = 16 * rng.choice(77, 20, replace=False)
        X[far] = (20000.0 + 4000.0 * rng.standard_normal((20, dim))).astype(np.float32)
        return X
    raise KeyError(kind)


def _nan_case(join):
    if join:
        X = _gauss(1100, 1100, 64).copy()
        X[517, 5] = np.nan
        return Case(X, path=1, nan_row=517)
    X = _gauss(11, 300, 40).copy()
    X[133, 39] = np.nan
    return Case(X, _gauss(12, 70, 40), nan_row=133)


def _build_cases():
    c = {}
    for nb in NB_EDGES:
        c[f"self_nb{nb}"] = lambda nb=nb: Case(_gauss(nb, nb, 40))
        for nq in NQ_EDGES:
            c[f"q{nq}_nb{nb}"] = lambda nb=nb, nq=nq: Case(_gauss(nb, nb, 40), _gauss(1000 + nq, nq, 40))
    for dim in DIMS:
        c[f"dim{dim}"] = lambda dim=dim: Case(_gauss(dim, 301, dim))
    c["dim1536"] = lambda: Case(_gauss(1536, 260, 1536))
    for tiles, nb in ((1, 100), (2, 200), (4, 500)):
        c[f"one_chunk_{tiles}tiles"] = lambda nb=nb: Case(_gauss(nb, nb, 20), _gauss(nb + 1, 70, 20))
    c["descending_d32"] = lambda: _descending(32)
    c["descending_d128"] = lambda: _descending(128)
    c["ascending_d32"] = lambda: _descending(32, True)
    c["identical_queries"] = lambda: Case(_identical(), _gauss(22, 10, 24))
    c["identical_self"] = lambda: Case(_identical())
    c["scattered_copies"] = _scattered_copies
    c["three_copies"] = _three_copies
    c["large_norms"] = _large_norms
    c["sliced"] = lambda: Case(_gauss(300, 500, 64), _gauss(301, 300, 64), blocks=1, launches=3)
    c["q_ids"] = _q_ids
    for name, (n, dim, kind) in JOIN_PLAIN.items():
        c[name] = lambda n=n, dim=dim, kind=kind: Case(_join_data(n, dim, kind), path=1, plain=True)
    c["join_dups"] = lambda: Case(_join_data(1200, 64, "dups"), path=1, overflow=True)
    c["join_outlier"] = lambda: Case(_join_data(1220, 96, "outlier"), path=1, overflow=True)
    c["join_sliced"] = lambda: Case(_join_data(1153, 128, "ints"), path=1, blocks=1, launches=5, plain=True)
    c["nan_queries"] = lambda: _nan_case(False)
    c["nan_join"] = lambda: _nan_case(True)
    return c


_CASES = _build_cases()
CASE_NAMES = tuple(_CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return _CASES[name]()


@functools.lru_cache(maxsize=None)
def model(name):
    """The host statement's answer for a case: computed once, shared by every test that needs it, never written to."""
    c = case(name)
    out = host_knn(c.X, c.Q, c.q_ids, c.path)
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def check_case(name, ids, dist):
    """The float64 judgement of one answer (the model's or the kernels') for a case, and what the case itself promises."""
    c = case(name)
    d64, tol = reference(c.X, c.Q)
    check_lists(ids, dist, d64, tol, c.self_col, c.X)
    p = c.promise
    if "nan_row" in p:
        assert not (ids == p["nan_row"]).any()
        if c.Q is None:
            assert (ids[p["nan_row"]] == PAD).all() and (dist[p["nan_row"]] == FMAX).all()
    if name.startswith("identical"):
        want = np.arange(33)[None, :].repeat(len(ids), 0)
        if c.Q is None:
            want = np.array([[j for j in range(33) if j != i][:32] for i in range(len(ids))])
        assert np.array_equal(ids, want[:, :32])
    if "copies" in p:                       # the 32 lowest of the 40 copies, in id order
        assert np.array_equal(ids, np.broadcast_to(p["copies"][:32].astype(np.uint32), ids.shape))
    if "copies_each" in p:                  # the copies first (distance exactly zero is not promised: see large norms), never itself
        X = c.X
        for i in range(len(X)):
            twins = [j for j in range(len(X)) if j != i and X[j].tobytes() == X[i].tobytes()]
            assert len(twins) >= 3 and ids[i, :len(twins)].tolist() == twins, i
    if "near" in p:
        for a, b in zip(p["near"], p["near_of"]):
            assert ids[a, 0] == b or d64[a, ids[a, 0]] <= 1.0, (a, b)
