"""The statement of diversified search (search_diverse) in plain numpy / Python, and the synthetic vectors and candidate rows
the host twin (cph_host_diverse_rows) and the kernel hook (cph_diverse_rows_hook) are compared with it on.

A query's candidate row is what the ordinary search returns at k = C: C entries ascending by (distance, id), padded with
-1 / FLT_MAX.  Walk the row front to back, skip padding (and ids at or above n_ids) and ids that occurred earlier in the
row: the survivors are the candidates, each with its position j and its relevance r_j = dist[j].  a = float32(lam),
b = float32(1) - a.  Pick 0 is the first candidate.  For pick t >= 1 every unpicked candidate has m_j = min over picked s
of d(s, j) and score_j = (a * r_j) - (b * m_j), three float32 operations; the smallest score is picked, equal scores go to
the lower position; k picks, or until the candidates run out.  Outputs in pick order: ids (-1 padded), dist = r of the
pick, gap = m of the pick when it was taken (FLT_MAX for pick 0 and for padding).

d(s, j) goes through a callable pair(s, js) -> float32 [len(js)]: this file knows nothing about its arithmetic."""
import ctypes as C
import gzip
import os

import numpy as np

FMAX = np.float32(3.4028234663852886e38)

CS = (1, 63, 64, 65, 130, 1024)
KS = (1, 3, 10, 64)                 # and k = C
DS = (16, 128, 256)                 # padded dimensions: the short loop, one 128-chunk, two chunks
LAMS = (0.0, 0.3, 0.5, 0.7, 1.0)


def diverse_model(ids_row, dist_row, k, lam, pair, n_ids, rows=None):
    """-> (ids [k] int64, dist [k] float32, gap [k] float32)."""
    ids_row = np.asarray(ids_row, np.int64)
    dist_row = np.asarray(dist_row, np.float32)
    a = np.float32(lam)
    b = np.float32(1) - a
    ids = np.full(k, -1, np.int64)
    dist = np.full(k, FMAX, np.float32)
    gap = np.full(k, FMAX, np.float32)
    seen, pos = set(), []
    for j in range(ids_row.shape[0]):
        i = int(ids_row[j])
        if i < 0 or i >= n_ids or i in seen:
            continue
        seen.add(i)
        pos.append(j)
    pos = np.array(pos, np.int64)                  # the unpicked candidates, ascending by position
    m = np.full(pos.shape[0], FMAX, np.float32)
    take = 0
    for t in range(k):
        if pos.size == 0:
            break
        s = int(ids_row[pos[take]])
        ids[t] = s if rows is None else int(rows[s])
        dist[t] = dist_row[pos[take]]              # (a float32 copy: the bytes of the row, -0.0 included)
        gap[t] = m[take]
        pos, m = np.delete(pos, take), np.delete(m, take)
        if t + 1 == k or pos.size == 0:
            break
        d = np.asarray(pair(s, ids_row[pos]), np.float32)
        m = np.where(d < m, d, m)
        score = a * dist_row[pos] - b * m           # float32 arrays: every operation is rounded on its own
        assert score.dtype == np.float32
        take = int(np.argmin(score))                # (the first of equal scores: the lower position; +0 == -0)
    return ids, dist, gap


def diverse_model_batch(ids, dist, k, lam, pair, n_ids, rows=None):
    n = ids.shape[0]
    out = (np.empty((n, k), np.int64), np.empty((n, k), np.float32), np.empty((n, k), np.float32))
    for q in range(n):
        r = diverse_model(ids[q], dist[q], k, lam, pair, n_ids, rows)
        for o, v in zip(out, r):
            o[q] = v
    return out


# ---- the pair distance from the oracle's free-array dot --------------------------------------------------------------------
class OraclePairs:
    """pair(s, js) over raw [n_ids, D] (zero-padded rows) and norm_sq [n_ids]: the oracle's eight-chain dot (orc_dot) for
    dot(s, j) and for qnorm = dot(s, s), then float32 (qnorm + norm_sq[j]) - 2 * dot clamped at 0."""

    def __init__(self, raw, norm_sq):
        from oracle_lib import Oracle
        self.raw = np.ascontiguousarray(raw, np.float32)
        self.norm_sq = np.ascontiguousarray(norm_sq, np.float32)
        self.D = self.raw.shape[1]
        self._orc = Oracle()
        self._dot = self._orc.lib["orc_dot"]      # (a function object of its own: oracle_lib sets other argtypes on its)
        self._dot.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._dot.restype = C.c_int

    def dots(self, s, js):
        js = np.asarray(js, np.int64)
        out = np.empty(js.shape[0], np.float32)
        base, stride, o, f, D = self.raw.ctypes.data, self.D * 4, out.ctypes.data, self._dot, self.D
        ps = base + int(s) * stride
        for i, j in enumerate(js.tolist()):
            f(D, ps, base + j * stride, o + 4 * i)
        return out

    def __call__(self, s, js):
        js = np.asarray(js, np.int64)
        qn = self.dots(s, [s])[0]
        v = (qn + self.norm_sq[js]) - np.float32(2) * self.dots(s, js)
        assert v.dtype == np.float32
        return np.where(v > 0, v, np.float32(0))


def read_v2_vectors(path, n, dim, D):
    """(raw [n, D], norm_sq [n]) as a v2 index file stores them (header 68, calibration 248, profile 72, centroid, levels,
    norms, rows); path may be gzipped."""
    op = gzip.open if path.endswith(".gz") else open
    with op(path, "rb") as f:
        data = f.read()
    off = 68 + 248 + 72 + dim * 4 + n * 4
    norm = np.frombuffer(data, np.float32, n, off).copy()
    raw = np.frombuffer(data, np.float32, n * D, off + n * 4).reshape(n, D).copy()
    return raw, norm


# ---- synthetic vectors and rows ---------------------------------------------------------------------------------------------
# Ids 0 .. N_RANDOM - 1 are Gaussian rows.  Behind them: N_DUP ids whose vector is that of id (i - N_RANDOM) (duplicate
# vectors under other ids, with the norm of their twin's chains so that d = 0 exactly); then Z (the zero row), X = 100 e1
# and Y = 100 e2 (d(Z, X) == d(Z, Y) bit for bit), stored so that id X > id Y.
N_RANDOM, N_DUP = 1300, 8
ID_Z, ID_Y, ID_X = N_RANDOM + N_DUP, N_RANDOM + N_DUP + 1, N_RANDOM + N_DUP + 2
N_IDS = ID_X + 1
ROW_KINDS = ("plain", "all_padding", "partly_padding", "repeated_ids", "dup_vectors", "equal_relevance", "score_tie")

_VEC = {}


def synth_vectors(D, dim=None):
    """-> (raw [N_IDS, D], norm_sq [N_IDS], OraclePairs); dim < D leaves zero padding.  Cached per (D, dim)."""
    dim = D if dim is None else dim
    if (D, dim) not in _VEC:
        rng = np.random.default_rng(7919 * D + dim)
        raw = np.zeros((N_IDS, D), np.float32)
        raw[:N_RANDOM, :dim] = rng.standard_normal((N_RANDOM, dim)).astype(np.float32)
        raw[N_RANDOM:N_RANDOM + N_DUP] = raw[:N_DUP]
        raw[ID_X, 0] = 100.0
        raw[ID_Y, 1] = 100.0
        # the builder's norms come from one chain; here: a float64 sum, which the eight chains do not reproduce either
        norm = (raw.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
        pairs = OraclePairs(raw, norm)
        for i in range(N_RANDOM, N_RANDOM + N_DUP):
            norm[i] = pairs.dots(i, [i])[0]
        pairs = OraclePairs(raw, norm)
        _VEC[(D, dim)] = (raw, norm, pairs)
    return _VEC[(D, dim)]


def _sorted_dist(rng, C):
    return np.sort(rng.random(C, dtype=np.float32) * np.float32(40.0))


def synth_row(kind, C, k, rng):
    """One candidate row (ids int64 [C], dist float32 [C]) of the named kind."""
    dist = _sorted_dist(rng, C)
    ids = rng.permutation(N_RANDOM)[:C].astype(np.int64)
    if kind == "all_padding":
        ids[:] = -1
        dist[:] = FMAX
    elif kind == "partly_padding":
        cut = max(1, min(k - 1, C * 2 // 3))             # fewer than k candidates where k > 1
        ids[cut:] = -1
        dist[cut:] = FMAX
        if C >= 3:
            ids[C - 1] = N_IDS + 5                        # an id beyond the vectors counts as padding too
    elif kind == "repeated_ids":
        if C >= 2:
            ids[C // 2] = ids[0]                           # twice
        if C >= 6:
            ids[3] = ids[1]                                # three times, one of them right behind ...
            ids[C - 1] = ids[1]                            # ... one far away
    elif kind == "dup_vectors":
        ids[0] = int(rng.integers(0, N_DUP))
        ids[1:] = N_DUP + rng.permutation(N_RANDOM - N_DUP)[:C - 1]       # (none of the ids that have a twin)
        if C >= 2:
            ids[1] = N_RANDOM + ids[0]                     # the same vector under another id, right behind its twin
        if C >= 8:
            ids[C - 2] = N_RANDOM + (ids[0] + 1) % N_DUP   # another such id, whose twin is not in the row
    elif kind == "equal_relevance":
        dist = np.sort(rng.integers(0, 3, C).astype(np.float32))
        zeros = np.flatnonzero(dist == 0)
        dist[zeros[rng.random(zeros.size) < 0.5]] = np.float32(-0.0)      # equal as floats, other bytes
    elif kind == "score_tie":
        # Z first; X and Y with the same relevance far apart in the row (other 8-lane groups, waves and threads of the
        # kernel); X, the HIGHER id, at the lower position
        if C >= 3:
            px, py = 1 + (C - 2) // 3, C - 1
            ids[0], ids[px], ids[py] = ID_Z, ID_X, ID_Y
            dist[px:py + 1] = dist[px]
    return ids, dist


def synth_batch(C, k, n=len(ROW_KINDS), seed=0, first=0):
    """n rows cycling through ROW_KINDS from kind `first` on -> (ids [n, C], dist [n, C], rows [N_IDS], kinds [n]).
    rows: a permutation of the id space (the row map of the 'with a row map' half of every case)."""
    rng = np.random.default_rng(1000003 * seed + 8191 * C + 131 * k)
    kinds = [ROW_KINDS[(first + i) % len(ROW_KINDS)] for i in range(n)]
    rows_ = [synth_row(kind, C, k, rng) for kind in kinds]
    return (np.stack([r[0] for r in rows_]), np.stack([r[1] for r in rows_]), rng.permutation(N_IDS).astype(np.uint32), kinds)


INDEX_ROW_KINDS = ("plain", "all_padding", "partly_padding", "repeated_ids", "equal_relevance")


def index_rows(n_ids, C, k, n, seed=0, first=0):
    """n candidate rows over the ids of a loaded index (C <= n_ids), cycling through INDEX_ROW_KINDS -> (ids [n, C],
    dist [n, C], kinds [n]).  The relevances are made up: the statement takes the row as it is."""
    rng = np.random.default_rng(1000003 * seed + 8191 * C + 131 * k + n_ids)
    kinds = [INDEX_ROW_KINDS[(first + i) % len(INDEX_ROW_KINDS)] for i in range(n)]
    ids, dist = np.empty((n, C), np.int64), np.empty((n, C), np.float32)
    for q, kind in enumerate(kinds):
        i, d = rng.permutation(n_ids)[:C].astype(np.int64), _sorted_dist(rng, C)
        if kind == "all_padding":
            i[:], d[:] = -1, FMAX
        elif kind == "partly_padding":
            cut = max(1, min(k - 1, C * 2 // 3))
            i[cut:], d[cut:] = -1, FMAX
        elif kind == "repeated_ids":
            if C >= 2:
                i[C // 2] = i[0]
            if C >= 6:
                i[3] = i[C - 1] = i[1]
        elif kind == "equal_relevance":
            d = np.sort(rng.integers(0, 3, C).astype(np.float32))
            zeros = np.flatnonzero(d == 0)
            d[zeros[rng.random(zeros.size) < 0.5]] = np.float32(-0.0)
        ids[q], dist[q] = i, d
    return ids, dist, kinds


def cases():
    """(C, k, D, dim, lam) of the CPU tests: every (C, k) that fits, k = C included, D and lam cycling so that every value
    meets every C; every lam and every D at (65, 10); dim < D once."""
    out, i = [], 0
    for Cn in CS:
        for k in sorted(set(x for x in KS + (Cn,) if x <= Cn)):
            D = DS[i % len(DS)]
            out.append((Cn, k, D, D, LAMS[(i // len(DS) + i) % len(LAMS)]))
            i += 1
    out += [(65, 10, D, D, lam) for D in DS for lam in LAMS if (65, 10, D, D, lam) not in out]
    out.append((130, 10, 128, 100, 0.5))
    return out


# ---- the library's two implementations (host twin, kernel hook) ----------------------------------------------------------------
def _outs(n, k):
    return (np.full((n, k), -7, np.int64), np.full((n, k), -7, np.float32), np.full((n, k), -7, np.float32))


def host_diverse_rows(ids, dist, raw, norm_sq, k, lam, rows=None):
    from cphnsw_mi355x import _lib
    n, Cn = ids.shape
    ids, dist = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(dist, np.float32)
    raw, norm_sq = np.ascontiguousarray(raw, np.float32), np.ascontiguousarray(norm_sq, np.float32)
    rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
    out = _outs(n, k)
    _lib.check(_lib.lib().cph_host_diverse_rows(ids.ctypes.data, dist.ctypes.data, n, Cn, raw.ctypes.data, norm_sq.ctypes.data,
                                                raw.shape[0], raw.shape[1], None if rows is None else rows.ctypes.data, k, float(lam),
                                                *[o.ctypes.data for o in out]))
    return out


def hook_diverse_rows(ix, ids, dist, k, lam):
    """The kernel on the given rows against the vectors of the (single-device) index ix."""
    from cphnsw_mi355x import _lib
    n, Cn = ids.shape
    ids, dist = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(dist, np.float32)
    out = _outs(n, k)
    _lib.check(_lib.lib().cph_diverse_rows_hook(ix._h, ids.ctypes.data, dist.ctypes.data, n, Cn, k, float(lam),
                                                *[o.ctypes.data for o in out]))
    return out


def same_bytes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
