"""The statement of fused search (search_fused: several query vectors per query, the k best rows by the exact weighted sum of
their distances) in numpy, the pair distance it is computed with, and the synthetic batch the host twin (cph_host_fused_rows)
and the kernel hook (cph_fused_rows_hook) are compared with it on.

Per query: T candidate rows [C] of internal ids (what an ordinary search at k = C returned for its T vectors, -1 = padding; the
distances of that search are used for nothing), of which the first L are live, and weights w [T], float32.
  candidates  the DISTINCT ids x, 0 <= x < n_ids, in the live rows;  hits(x) = the live rows that hold x (repeats inside one row
              count once);
  score(x)    s = +0.0; for t = 0 .. L - 1: s = float32(s + float32(w[t] * d_t(x))), d_t(x) being given by a callable --
              dist(t, ids) -> float32 [len(ids)], the bytes of exact_l2 for vector t and every id -- for EVERY live t;
  a candidate whose s is NaN is dropped; the k best by (s, id) ascending are the answer: (ids int64 [k], score float32 [k],
  hits int32 [k]), ids through the row map if one is given, padded with -1 / FLT_MAX / 0.
s is never -0.0, so value order and the order of the sign-flipped bits agree."""
import ctypes as C

import numpy as np

FMAX = np.float32(3.4028234663852886e38)
BIG = np.float32(3e38)


def same_bytes(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _orderable(s):
    u = np.asarray(s, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, u ^ 0xFFFFFFFF, u ^ 0x80000000)


def fused_model(cand, L, w, dist, n_ids, k, rows=None):
    """One query: cand int64 [T, C], L live rows, w float32 [T], dist(t, ids) -> float32 [len(ids)]."""
    cand = np.asarray(cand, np.int64)
    w = np.asarray(w, np.float32)
    out_ids, out_score, out_hits = np.full(k, -1, np.int64), np.full(k, FMAX, np.float32), np.zeros(k, np.int32)
    live = cand[:L]
    union = np.unique(live[(live >= 0) & (live < n_ids)])              # ascending
    if union.size == 0:
        return out_ids, out_score, out_hits
    hits = np.zeros(union.size, np.int32)
    for t in range(L):
        hits += np.isin(union, live[t]).astype(np.int32)
    s = np.zeros(union.size, np.float32)                               # +0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(L):
            d = np.asarray(dist(t, union), np.float32)
            p = w[t] * d                                               # float32 * float32: one rounding
            assert p.dtype == np.float32
            s = s + p                                                  # one rounding
            assert s.dtype == np.float32
    assert not np.any((s == 0) & np.signbit(s))
    keep = ~np.isnan(s)
    union, s, hits = union[keep], s[keep], hits[keep]
    order = np.lexsort((union, _orderable(s)))[:k]
    f = len(order)
    out_ids[:f] = union[order] if rows is None else np.asarray(rows)[union[order]]
    out_score[:f] = s[order]
    out_hits[:f] = hits[order]
    return out_ids, out_score, out_hits


def fused_model_batch(cand, n_vectors, weights, dist, n_ids, k, rows=None):
    """cand int64 [n, T, C]; n_vectors [n] or None; weights float32 [n, T]; dist(q, t, ids) -> float32 [len(ids)]."""
    n, T, _ = cand.shape
    out = (np.empty((n, k), np.int64), np.empty((n, k), np.float32), np.empty((n, k), np.int32))
    for q in range(n):
        r = fused_model(cand[q], T if n_vectors is None else int(n_vectors[q]), weights[q], lambda t, ids, q=q: dist(q, t, ids), n_ids, k, rows)
        for o, v in zip(out, r):
            o[q] = v
    return out


# ---- the pair distance from the oracle's free-array dot ----------------------------------------------------------------------
class OracleQueryDists:
    """dist(q, t, ids) over raw [n_ids, D] (zero-padded rows), norm_sq [n_ids] and FREE query vectors [n, T, dim]: the oracle's
    eight-chain dot (orc_dot) for dot(q_t, id) and for qnorm = dot(q_t, q_t) over the zero-padded vector, then float32
    (qnorm + norm_sq[id]) - 2 * dot clamped at 0 -- diverse_model.OraclePairs with the stored row s replaced by a free vector.
    one(vec, ids) is the same for a single vector; test_fused_host ties it byte for byte to OracleIndex.exact_l2."""

    def __init__(self, raw, norm_sq, queries=None):
        from oracle_lib import Oracle
        self.raw = np.ascontiguousarray(raw, np.float32)
        self.norm_sq = np.ascontiguousarray(norm_sq, np.float32)
        self.D = self.raw.shape[1]
        self._orc = Oracle()
        self._dot = self._orc.lib["orc_dot"]      # (a function object of its own: oracle_lib sets other argtypes on its)
        self._dot.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._dot.restype = C.c_int
        self.q = None if queries is None else self.padded(queries)
        self._memo = {}

    def padded(self, queries):
        queries = np.asarray(queries, np.float32)
        out = np.zeros(queries.shape[:-1] + (self.D,), np.float32)
        out[..., :queries.shape[-1]] = queries
        return out

    def one(self, vec, ids):
        ids = np.asarray(ids, np.int64)
        pq = np.ascontiguousarray(self.padded(vec))
        qn, dots = np.empty(1, np.float32), np.empty(len(ids), np.float32)
        f, D, base, stride, o = self._dot, self.D, self.raw.ctypes.data, self.D * 4, dots.ctypes.data
        f(D, pq.ctypes.data, pq.ctypes.data, qn.ctypes.data)
        for i, j in enumerate(ids.tolist()):
            f(D, pq.ctypes.data, base + j * stride, o + 4 * i)
        with np.errstate(over="ignore", invalid="ignore"):
            v = (qn[0] + self.norm_sq[ids]) - np.float32(2) * dots
        assert v.dtype == np.float32
        return np.where(v < 0, np.float32(0), v)          # (v < 0 ? 0 : v: a NaN stays, as in exact_from_dot)

    def __call__(self, q, t, ids):
        ids = np.asarray(ids, np.int64)
        memo = self._memo.setdefault((q, t), {})
        todo = [int(i) for i in ids if int(i) not in memo]
        if todo:
            memo.update(zip(todo, self.one(self.q[q, t, :], todo)))
        return np.array([memo[int(i)] for i in ids], np.float32)


# ---- synthetic vectors and the batch -------------------------------------------------------------------------------------------
N_SYNTH = 180
TWIN_LO, TWIN_HI = 7, N_SYNTH - 1
U_SIZES = (0, 1, 63, 64, 65)
KINDS = ("all_padding", "few", "out_of_range", "repeats", "twins", "dead", "negative", "zero", "nan", "scaled_a", "scaled_b")


def synth_index(D, dim, seed=0):
    """-> (raw [N_SYNTH, D] zero-padded, norm_sq [N_SYNTH]); ids TWIN_LO and TWIN_HI hold one vector (and one norm)."""
    rng = np.random.default_rng(15485863 * D + dim + seed)
    raw = np.zeros((N_SYNTH, D), np.float32)
    raw[:, :dim] = rng.standard_normal((N_SYNTH, dim)).astype(np.float32)
    raw[TWIN_HI] = raw[TWIN_LO]
    norm = (raw.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)      # (one chain in the builder; here a float64 sum)
    return raw, norm


def _row(ids, C_):
    r = np.full(C_, -1, np.int64)
    ids = np.asarray(ids, np.int64)[:C_]
    r[:len(ids)] = ids
    return r


def synth_batch(raw, dim, T, C_, twins, seed=0, u_sizes=U_SIZES):
    """One query per row kind that (T, C) can hold, then one per union size U in u_sizes that fits ->
    dict(cand int64 [n, T, C], Q float32 [n, T, dim], n_vectors int32 [n], weights float32 [n, T], kinds [n], mark {kind: ids ...}).
    raw [n_ids, >= dim]: the stored vectors (queries are made around them); twins = (lo id, hi id) of one vector under two ids.
    Unless a kind says otherwise a query's rows are random distinct ids, its vectors rows of the index plus noise, every vector
    live and every weight in [0.5, 1.5]."""
    n_ids = raw.shape[0]
    rng = np.random.default_rng(1000003 * T + 101 * C_ + seed)
    cand, Q, nv, W, kinds, mark = [], [], [], [], [], {}

    def plain_rows(exclude=()):
        pool = np.setdiff1d(np.arange(n_ids), np.asarray(exclude, np.int64))
        return np.stack([_row(rng.permutation(pool), C_) for _ in range(T)])

    def plain_q():
        return (raw[rng.integers(0, n_ids, T), :dim] + np.float32(0.3) * rng.standard_normal((T, dim))).astype(np.float32)

    def plain_w():
        return rng.uniform(0.5, 1.5, T).astype(np.float32)

    def add(kind, rows, q=None, L=T, w=None):
        cand.append(rows)
        Q.append(plain_q() if q is None else q)
        nv.append(L)
        W.append(plain_w() if w is None else np.asarray(w, np.float32))
        kinds.append(kind)

    add("all_padding", np.full((T, C_), -1, np.int64))
    a, b, x, z = (int(v) for v in rng.choice(np.setdiff1d(np.arange(n_ids), twins), 4, replace=False))
    rows = np.full((T, C_), -1, np.int64)
    rows[0, 0] = a
    rows[T - 1, C_ - 1] = b
    add("few", rows)
    mark["few"] = (a, b)
    rows = plain_rows()
    rows[:, ::3] = np.array([n_ids, n_ids + 5, 2 ** 31 + 7, 2 ** 40])[rng.integers(0, 4, rows[:, ::3].shape)]
    add("out_of_range", rows)
    if C_ >= 3:
        rows = plain_rows(exclude=(a, b))
        rows[0, :3] = (a, a, b)                                  # a: twice in row 0, nowhere else; b: in every row
        rows[1:, 0] = b
        add("repeats", rows)
        mark["repeats"] = (a, b)
    if C_ >= 2:
        rows = plain_rows(exclude=twins)
        rows[0, :2] = twins[::-1]                                # (the higher id first: the order of the union decides nothing)
        add("twins", rows, w=np.ones(T, np.float32))
    if T >= 2:
        L = max(1, T // 2)
        rows = plain_rows(exclude=(z,))
        rows[L:, :] = z                                          # the dead rows hold an id the live ones do not
        q = plain_q()
        q[L:] = np.float32(1e30)
        w = plain_w()
        w[L:] = np.float32(-7.0)
        add("dead", rows, q=q, L=L, w=w)
        mark["dead"] = (z,)
    # x IS every vector of the query: nearest to vector 0; under w = (1, -2) (T = 1: (-2,)) every other row scores below it
    rows = plain_rows(exclude=(x,))
    rows[0, 0] = x
    q = np.repeat(raw[x:x + 1, :dim], T, axis=0).astype(np.float32)
    w = np.zeros(T, np.float32)
    w[:2] = (1.0, -2.0)[:T] if T > 1 else (-2.0,)
    add("negative", rows, q=q, w=w)
    mark["negative"] = (x,)
    w = plain_w()
    w[T - 1] = 0.0
    add("zero", plain_rows(), w=w)
    if T >= 2:
        rows = plain_rows(exclude=(x,))
        rows[0, 0] = x
        w = np.zeros(T, np.float32)
        w[:2] = (BIG, -BIG)                                      # every distance above 1.14 overflows: inf + -inf; x stays (d0 == d1, tiny)
        add("nan", rows, q=q, w=w)
        mark["nan"] = (x,)
    rows, q = plain_rows(), plain_q()
    w = np.resize(np.array([0.5, 0.25], np.float32), T)
    add("scaled_a", rows, q=q, w=w)
    add("scaled_b", rows.copy(), q=q.copy(), w=w * np.float32(2.0))
    for U in u_sizes:
        if U > min(T * C_, n_ids) or U == 0:
            continue
        ids = rng.choice(n_ids, U, replace=False)
        extra = rng.choice(ids, min(T * C_ - U, U))
        entries = rng.permutation(np.concatenate([ids, extra]))
        flat = np.full(T * C_, -1, np.int64)
        flat[rng.choice(T * C_, len(entries), replace=False)] = entries      # scattered: padding between entries, repeats in a row
        add(f"u{U}", flat.reshape(T, C_))
    return dict(cand=np.stack(cand), Q=np.stack(Q), n_vectors=np.array(nv, np.int32), weights=np.stack(W), kinds=kinds, mark=mark)


def union_sizes(batch, n_ids):
    out = []
    for rows, L in zip(batch["cand"], batch["n_vectors"]):
        live = rows[:L]
        out.append(len(np.unique(live[(live >= 0) & (live < n_ids)])))
    return out


def check_batch_promises(batch, dist, n_ids, twins):
    """Every kind really is what its name says, by the model at k = all entries."""
    cand, nv, W, kinds, mark = batch["cand"], batch["n_vectors"], batch["weights"], batch["kinds"], batch["mark"]
    n, T, C_ = cand.shape
    k = T * C_
    ids, score, hits = fused_model_batch(cand, nv, W, dist, n_ids, k)
    U = union_sizes(batch, n_ids)
    found = (ids >= 0).sum(axis=1)
    at = {kind: i for i, kind in enumerate(kinds)}
    assert (ids[np.arange(k)[None, :] >= found[:, None]] == -1).all() and (ids < n_ids).all()
    i = at["all_padding"]
    assert U[i] == 0 and found[i] == 0 and (score[i] == FMAX).all() and (hits[i] == 0).all()
    i = at["few"]
    assert U[i] == 2 and set(ids[i, :2].tolist()) == set(mark["few"]) and (hits[i, :2] == 1).all()
    i = at["out_of_range"]
    assert (cand[i] >= n_ids).any() and found[i] == U[i] and (U[i] > 0 or C_ == 1)
    if "repeats" in at:
        i = at["repeats"]
        a, b = mark["repeats"]
        got = dict(zip(ids[i, :found[i]].tolist(), hits[i, :found[i]].tolist()))
        assert (cand[i, 0] == a).sum() == 2 and got[a] == 1 and got[b] == nv[i]
    if "twins" in at:
        i = at["twins"]
        pos = ids[i].tolist().index(twins[0])
        assert ids[i, pos + 1] == twins[1] and score[i, pos].tobytes() == score[i, pos + 1].tobytes()
    if "dead" in at:
        i = at["dead"]
        assert nv[i] < T and mark["dead"][0] in cand[i, nv[i]:] and mark["dead"][0] not in ids[i] and np.isfinite(score[i, :found[i]]).all()
    i = at["negative"]
    x = mark["negative"][0]
    w0 = W[i].copy()
    w0[1:] = 0
    w0[0] = 1
    first = fused_model(cand[i], nv[i], w0, lambda t, js: dist(i, t, js), n_ids, k)[0]
    assert first[0] == x and ids[i, found[i] - 1] == x and found[i] == U[i] > 1 and (W[i] < 0).any()
    i = at["zero"]
    assert (W[i] == 0).any()
    if "nan" in at:
        i = at["nan"]
        assert 0 < found[i] < U[i] and mark["nan"][0] in ids[i, :found[i]]
    i, j = at["scaled_a"], at["scaled_b"]
    assert np.array_equal(W[j], W[i] * 2) and np.array_equal(ids[i], ids[j]) and found[i] > 1
    for size in U_SIZES[1:]:
        if f"u{size}" in at:
            assert U[at[f"u{size}"]] == size == found[at[f"u{size}"]]
    return ids, score, hits


# ---- the library's implementations (host twin, kernel hook) ----------------------------------------------------------------------
def _outs(n, k):
    return np.full((n, k), -7, np.int64), np.full((n, k), -7, np.float32), np.full((n, k), -7, np.int32)


def _ptr(a):
    return None if a is None else a.ctypes.data


def host_fused_rows(cand, n_vectors, weights, qpad, raw, norm_sq, k, rows=None):
    from cphnsw_mi355x import _lib
    n, T, C_ = cand.shape
    cand = np.ascontiguousarray(cand, np.int64)
    nv = None if n_vectors is None else np.ascontiguousarray(n_vectors, np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    qpad, raw, norm_sq = (np.ascontiguousarray(x, np.float32) for x in (qpad, raw, norm_sq))
    rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
    out = _outs(n, k)
    _lib.check(_lib.lib().cph_host_fused_rows(cand.ctypes.data, n, T, _ptr(nv), _ptr(w), C_, qpad.ctypes.data, raw.ctypes.data,
                                              norm_sq.ctypes.data, raw.shape[0], raw.shape[1], _ptr(rows), k, *[o.ctypes.data for o in out]))
    return out


def hook_fused_rows(ix, cand, Q, n_vectors, weights, k):
    """The pad, union, scan and select kernels on the given candidate rows against the vectors of the (single-device) index."""
    from cphnsw_mi355x import _lib
    n, T, C_ = cand.shape
    cand, Q = np.ascontiguousarray(cand, np.int64), np.ascontiguousarray(Q, np.float32)
    nv = None if n_vectors is None else np.ascontiguousarray(n_vectors, np.int32)
    w = None if weights is None else np.ascontiguousarray(weights, np.float32)
    out = _outs(n, k)
    _lib.check(_lib.lib().cph_fused_rows_hook(ix._h, cand.ctypes.data, Q.ctypes.data, n, T, _ptr(nv), _ptr(w), C_, k,
                                              *[o.ctypes.data for o in out]))
    return out
