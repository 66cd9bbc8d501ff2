"""The statement of two-stage search (make_rescore_vectors, search_rescored) in plain numpy, and the synthetic rows the host
twin (cph_host_rescore_rows, cph_host_rescore_rows_in) and the kernels (cph_rescore_rows_hook, cph_rescore_vectors_get) are
compared with it on.  csrc/host_rescore.h states the same in C++.

The object: one row of dim_full coordinates per internal id, stored as float16 (round to nearest even: numpy's astype) or
float32; the stored row is `stride` bytes, dim_full coordinates and zeros up to a multiple of 16 bytes; one float32 squared
norm per row, summed from the STORED values.  A row whose norm is not < inf is refused (a NaN, an Inf, a value that
overflows float16, an overflowing norm: each leaves an Inf or a NaN among the stored values).

The layout of a sum, a pure function of (dim_full, dtype):
    piece     16 stored bytes: E = 8 float16 or 4 float32 coordinates; a row is P = stride / 16 pieces
    G         the lanes that share a row: the power of two >= P, at most 64
    lane l    takes the pieces l, l + G, l + 2 G, ... and adds their E products each, in ascending coordinate order, to ONE
              float32 partial sum that starts as +0
    the fold  for d = G/2, G/4, ... 1: p[l] = p[l] + p[l ^ d], all lanes at once
dot(q, x), qn = dot(q, q), xn = dot(x, x) are sums of this shape over the zero-padded float32 query and the stored row
converted to float32; every product and every sum is rounded on its own.  No such sum is ever -0 (a partial sum starts
as +0, and x + y is -0 only if both are), so the zero padding of a short last pass below changes nothing.
    "l2": score = max(0, (qn + xn) - 2 * dot)        "ip": score = -dot

A candidate row: C internal ids and first-stage distances, -1 / FLT_MAX padding.  Padding, ids at or above n_ids and every
occurrence of an id after its first are dropped, each survivor is scored, NaN scores are dropped, the k best by (score,
internal id) ascending are returned: ids (through the row map if there is one), score, first = the distance bytes at the
id's first position; unused slots are -1 / FLT_MAX / FLT_MAX.  A query whose qn is not < inf gets a row of padding."""
import ctypes as C

import numpy as np

from diverse_model import FMAX, ID_X, ID_Y, ID_Z, N_DUP, N_IDS, N_RANDOM, ROW_KINDS, synth_row

CS = (1, 63, 64, 65, 130, 1024)
KS = (1, 3, 10, 64)                                  # and k = C
DIMS = (1, 7, 8, 24, 64, 72, 520, 1024, 8192)        # below one piece, not a multiple of it, every G, several passes of G = 64
DTYPES = ("float16", "float32")
METRICS = ("l2", "ip")
KINDS = ROW_KINDS + ("one_more_than_k",)


class Layout:
    def __init__(self, dim_full, dtype):
        assert dtype in DTYPES and 1 <= dim_full <= 8192
        self.dim, self.dtype = int(dim_full), dtype
        self.elem_bytes = 4 if dtype == "float32" else 2
        self.E = 16 // self.elem_bytes
        self.pieces = -(-self.dim // self.E)
        self.stride = self.pieces * 16
        self.padded = self.pieces * self.E
        self.G = 1
        while self.G < self.pieces and self.G < 64:
            self.G *= 2
        self.np_dtype = np.float32 if dtype == "float32" else np.float16


def model_sum(a, b, L):
    """a [m, padded] (or [padded]) times b (broadcast) summed in the shape of the layout -> float32 [m]."""
    with np.errstate(all="ignore"):
        prod = np.atleast_2d(np.asarray(a, np.float32) * np.asarray(b, np.float32))
        assert prod.dtype == np.float32 and prod.shape[1] == L.padded
        m = prod.shape[0]
        passes = -(-L.pieces // L.G)
        full = np.zeros((m, passes * L.G * L.E), np.float32)
        full[:, :L.padded] = prod
        full = full.reshape(m, passes, L.G, L.E)
        acc = np.zeros((m, L.G), np.float32)
        for p in range(passes):
            for e in range(L.E):
                acc = acc + full[:, p, :, e]
        lanes = np.arange(L.G)
        d = L.G // 2
        while d:
            acc = acc + acc[:, lanes ^ d]
            d //= 2
        assert acc.dtype == np.float32
        return acc[:, 0].copy()


def stored_values(stored, L):
    """stored uint8 [n, stride] -> the rows as float32 [n, padded] (exact)."""
    return np.ascontiguousarray(stored).view(L.np_dtype).reshape(stored.shape[0], L.padded).astype(np.float32)


def rows_in_model(rows, dtype, row_map=None):
    """rows float32 [n, dim_full] -> (stored uint8 [n, stride], norms float32 [n], bad: the refused rows in the caller's
    numbering, ascending).  row_map [n_map]: the rows arrive in input order, row row_map[i] goes to position i, rows at or
    above n_map stay where they are."""
    rows = np.ascontiguousarray(rows, np.float32)
    n, dim = rows.shape
    L = Layout(dim, dtype)
    vals = np.zeros((n, L.padded), L.np_dtype)
    with np.errstate(all="ignore"):
        vals[:, :dim] = rows.astype(L.np_dtype)
    x = vals.astype(np.float32)
    norms = model_sum(x, x, L)
    bad = np.flatnonzero(~(norms < np.inf))
    if row_map is not None:
        order = np.concatenate([np.asarray(row_map, np.int64), np.arange(len(row_map), n)])
        vals, norms = vals[order], norms[order]
    return np.ascontiguousarray(vals).view(np.uint8).reshape(n, L.stride), norms, bad


def model_scores(fq, x, norms, L, metric):
    """The scores of the full query fq [dim_full] against the stored rows x float32 [m, padded] -> (float32 [m], qn)."""
    qv = np.zeros(L.padded, np.float32)
    qv[:L.dim] = fq
    qn = model_sum(qv, qv, L)[0]
    dot = model_sum(x, qv, L)
    with np.errstate(all="ignore"):
        if metric == "ip":
            return -dot, qn
        v = (qn + np.asarray(norms, np.float32)) - np.float32(2) * dot
    assert v.dtype == np.float32
    return np.where(v < 0, np.float32(0), v), qn


def rescore_model(ids_row, dist_row, k, fq, X, norms, L, metric, n_ids, rows=None):
    """One candidate row -> (ids [k] int64, score [k] float32, first [k] float32).  X: stored_values of the object."""
    ids_row = np.asarray(ids_row, np.int64)
    dist_row = np.asarray(dist_row, np.float32)
    ids, score, first = np.full(k, -1, np.int64), np.full(k, FMAX, np.float32), np.full(k, FMAX, np.float32)
    seen, pos = set(), []
    for j, i in enumerate(ids_row.tolist()):
        if i < 0 or i >= n_ids or i in seen:
            continue
        seen.add(i)
        pos.append(j)
    if not pos:
        return ids, score, first
    pos = np.array(pos, np.int64)
    cid = ids_row[pos]
    s, qn = model_scores(fq, X[cid], norms[cid], L, metric)
    if not qn < np.inf:
        return ids, score, first
    keep = ~np.isnan(s)
    pos, cid, s = pos[keep], cid[keep], s[keep]
    order = np.lexsort((cid, s))[:k]                 # by score, then by internal id (+0 == -0; neither metric has both)
    m = order.shape[0]
    ids[:m] = cid[order] if rows is None else np.asarray(rows)[cid[order]]
    score[:m] = s[order]
    first[:m] = dist_row[pos[order]]                 # (a float32 copy: the bytes of the row, -0.0 included)
    return ids, score, first


def rescore_model_batch(ids, dist, k, fq, X, norms, L, metric, n_ids, rows=None):
    n = ids.shape[0]
    out = (np.empty((n, k), np.int64), np.empty((n, k), np.float32), np.empty((n, k), np.float32))
    for q in range(n):
        r = rescore_model(ids[q], dist[q], k, fq[q], X, norms, L, metric, n_ids, rows)
        for o, v in zip(out, r):
            o[q] = v
    return out


# ---- synthetic full rows, queries and candidate rows ------------------------------------------------------------------------
# The id space is diverse_model's: ids 0 .. N_RANDOM - 1 are Gaussian rows; behind them N_DUP ids that repeat the rows of ids
# 0 .. N_DUP - 1 (duplicate vectors under other ids: equal scores, decided by id); Z the zero row, X = 100 e1, Y = 100 e2 (e2
# = e1 where dim_full == 1).
_VEC = {}


def synth_full(dim):
    """-> float32 [N_IDS, dim].  Cached."""
    if dim not in _VEC:
        rng = np.random.default_rng(104729 * dim + 11)
        x = np.zeros((N_IDS, dim), np.float32)
        x[:N_RANDOM] = rng.standard_normal((N_RANDOM, dim)).astype(np.float32)
        x[N_RANDOM:N_RANDOM + N_DUP] = x[:N_DUP]
        x[ID_X, 0] = 100.0
        x[ID_Y, min(1, dim - 1)] = 100.0
        x.setflags(write=False)
        _VEC[dim] = x
    return _VEC[dim]


def synth_rows(C, k, seed=0, n=len(KINDS), first=0):
    """n candidate rows cycling through KINDS -> (ids [n, C], dist [n, C], kinds)."""
    rng = np.random.default_rng(1000003 * seed + 8191 * C + 131 * k + 5)
    kinds = [KINDS[(first + i) % len(KINDS)] for i in range(n)]
    out = []
    for kind in kinds:
        if kind == "one_more_than_k":
            ids, dist = synth_row("plain", C, k, rng)
            cut = min(C, k + 1)
            ids[cut:], dist[cut:] = -1, FMAX
        else:
            ids, dist = synth_row(kind, C, k, rng)
        out.append((ids, dist))
    return np.stack([r[0] for r in out]), np.stack([r[1] for r in out]), kinds


def synth_queries(n, dim, seed=0):
    rng = np.random.default_rng(7919 * dim + seed)
    return rng.standard_normal((n, dim)).astype(np.float32)


def cases():
    """(C, k, dim_full, dtype, metric) of the CPU tests: every (C, k) that fits, k = C included, the other three cycling so
    that every dim_full meets both dtypes and both metrics."""
    combos = [(d, t, m) for d in DIMS for t in DTYPES for m in METRICS]
    pairs = [(Cn, k) for Cn in CS for k in sorted(set(x for x in KS + (Cn,) if x <= Cn))]
    assert len(combos) >= len(pairs) and np.gcd(7, len(combos)) == 1
    return [pairs[j % len(pairs)] + combos[(7 * j) % len(combos)] for j in range(len(combos))]


# ---- the library's implementations ---------------------------------------------------------------------------------------------
def _codes(dtype, metric):
    return (1 if dtype == "float32" else 0), (1 if metric == "ip" else 0)


def _outs(n, k):
    return (np.full((n, k), -7, np.int64), np.full((n, k), -7, np.float32), np.full((n, k), -7, np.float32))


def host_rows_in(rows, dtype, row_map=None):
    """cph_host_rescore_rows_in -> (stored uint8 [n, stride], norms, bad count, first bad row or None)."""
    from cphnsw_mi355x import _lib
    rows = np.ascontiguousarray(rows, np.float32)
    n, dim = rows.shape
    L = Layout(dim, dtype)
    stored, norms = np.full((n, L.stride), 0xA5, np.uint8), np.full(n, -7, np.float32)
    rm = None if row_map is None else np.ascontiguousarray(row_map, np.uint32)
    bad, first = C.c_uint64(), C.c_uint64()
    _lib.check(_lib.lib().cph_host_rescore_rows_in(rows.ctypes.data, n, dim, _codes(dtype, "l2")[0], None if rm is None else rm.ctypes.data,
                                                   0 if rm is None else rm.shape[0], stored.ctypes.data, norms.ctypes.data,
                                                   C.byref(bad), C.byref(first)))
    return stored, norms, bad.value, (None if first.value == 2 ** 64 - 1 else first.value)


def host_rescore_rows(ids, dist, k, fq, stored, norms, dtype, metric, rows=None):
    from cphnsw_mi355x import _lib
    n, Cn = ids.shape
    ids, dist = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(dist, np.float32)
    fq, stored, norms = np.ascontiguousarray(fq, np.float32), np.ascontiguousarray(stored, np.uint8), np.ascontiguousarray(norms, np.float32)
    rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
    dt, mt = _codes(dtype, metric)
    out = _outs(n, k)
    _lib.check(_lib.lib().cph_host_rescore_rows(ids.ctypes.data, dist.ctypes.data, n, Cn, fq.ctypes.data, fq.shape[1], stored.ctypes.data,
                                                norms.ctypes.data, stored.shape[0], dt, mt, None if rows is None else rows.ctypes.data, k,
                                                *[o.ctypes.data for o in out]))
    return out


def hook_rescore_rows(ix, vectors, ids, dist, k, fq):
    """The kernel on the given rows against a RescoreVectors of the (single-device) index ix."""
    from cphnsw_mi355x import _lib
    n, Cn = ids.shape
    ids, dist = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(dist, np.float32)
    fq = np.ascontiguousarray(fq, np.float32)
    assert fq.shape == (n, vectors.dim)
    out = tuple(np.full(o.shape, -7, o.dtype) for o in _outs(n, k))
    _lib.check(_lib.lib().cph_rescore_rows_hook(ix._h, ids.ctypes.data, dist.ctypes.data, n, Cn, fq.ctypes.data, vectors._hs[0], k,
                                                *[o.ctypes.data for o in out]))
    return out


def same_bytes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
