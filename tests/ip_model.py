"""The inner-product metric's arithmetic in numpy (csrc/host_ip.h and csrc/device_ip.h state the same), float32 throughout.

    s(x)   the cosine metric's sum (cosine_model.py): 64 lane sums of x[j] * x[j], product and sum rounded apart, then a
           xor butterfly at distances 32, 16, 8, 4, 2, 1
    row    out[0..dim) = x (the bits), out[dim] = sqrt(M2 - s)            (np.sqrt is correctly rounded)
    query  out[0..dim) = q (the bits), out[dim] = +0, c = s + M2
    score  dist = 0.5 * (dist - c) wherever id >= 0; a padding entry (id < 0) keeps its bytes

A vector is bad when not (s < inf): NaN, Inf, or an overflowing s.  A row is over the bound when s > M2.  Both are
written as dim + 1 zeros (+0.0) and counted apart; the lowest row of either kind is reported (NO_ROW when there is none).
A bad query is the zero vector with c = M2.  A zero vector is good.  M2 is the caller's, or the largest s over the good
rows."""
import numpy as np

NO_ROW = 2 ** 64 - 1
DIMS = (8, 63, 64, 65, 127, 128, 130, 960)         # both sides of the 64-lane stride, and the multi-pass loop
NS = (1, 3, 130)                                   # 130 rows: more than one workgroup of four waves
BAD_KINDS = ("nan", "inf", "overflow")


def sq_norm_model(x):
    """s of every row of x [n, dim]: float32 [n] (NaN or inf for a bad row)."""
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    chunks = (dim + 63) // 64
    with np.errstate(all="ignore"):
        sq = np.zeros((n, chunks * 64), np.float32)     # (padding with +0 changes no bit: cosine_model.py)
        sq[:, :dim] = x * x
        p = np.zeros((n, 64), np.float32)
        for c in range(chunks):
            p = p + sq[:, c * 64:(c + 1) * 64]
        lanes = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            p = p + p[:, lanes ^ d]
    assert p.dtype == np.float32
    return p[:, 0].copy()


def max_model(x):
    """M2 from the data: the largest s over the good rows (+0 when there is none)."""
    s = sq_norm_model(x)
    with np.errstate(all="ignore"):
        good = s < np.inf
    return np.float32(s[good].max()) if good.any() else np.float32(0.0)


def _counters(bad, over):
    both = np.flatnonzero(bad | over)
    return int(bad.sum()), int(over.sum()), int(both[0]) if both.size else NO_ROW


def rows_model(x, m2=None):
    """x [n, dim] -> (out [n, dim + 1] float32, M2, (bad, over, first))."""
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    m2 = max_model(x) if m2 is None else np.float32(m2)
    s = sq_norm_model(x)
    with np.errstate(all="ignore"):
        bad = ~(s < np.inf)
        over = ~bad & (s > m2)
        good = ~bad & ~over
        out = np.zeros((n, dim + 1), np.float32)
        out[good, :dim] = x[good]
        out[good, dim] = np.sqrt(m2 - s[good])
    assert out.dtype == np.float32
    return out, m2, _counters(bad, over)


def model(x, m2=None):
    """The rows as an inner-product index stores them (no bad or over-bound row allowed)."""
    out, _, cnt = rows_model(x, m2)
    assert cnt[:2] == (0, 0)
    return out


def queries_model(q, m2):
    """q [n, dim] -> (out [n, dim + 1] float32, c [n] float32, (bad, 0, first))."""
    q = np.ascontiguousarray(q, np.float32)
    n, dim = q.shape
    m2 = np.float32(m2)
    s = sq_norm_model(q)
    with np.errstate(all="ignore"):
        bad = ~(s < np.inf)
        out = np.zeros((n, dim + 1), np.float32)
        out[~bad, :dim] = q[~bad]
        c = np.where(bad, m2, s + m2).astype(np.float32)
    return out, c, _counters(bad, np.zeros(n, bool))


def epilogue_model(ids, dist, c):
    """ids, dist [n, k], c [n] -> the scores, float32 [n, k]; entries with id < 0 keep their bytes."""
    ids = np.asarray(ids)
    dist = np.ascontiguousarray(dist, np.float32)
    with np.errstate(all="ignore"):
        score = np.float32(0.5) * (dist - np.asarray(c, np.float32)[:, None])
    assert score.dtype == np.float32
    return np.where(ids >= 0, score, dist)


def case_rows(n, dim, seed=0):
    """Gaussian rows times per-row scales 2^-10 .. 2^10 (both ends present when n >= 2)."""
    rng = np.random.default_rng(1000 * dim + n + seed)
    e = rng.integers(-10, 11, n)
    e[0] = 10
    e[-1] = -10 if n > 1 else e[-1]
    return (rng.standard_normal((n, dim)) * np.exp2(e)[:, None]).astype(np.float32)


def bad_row(kind, dim, rng):
    r = rng.standard_normal(dim).astype(np.float32)
    if kind == "nan":
        r[rng.integers(0, dim)] = np.nan
    elif kind == "inf":
        r[rng.integers(0, dim)] = -np.inf if dim % 2 else np.inf
    elif kind == "overflow":
        r[:] = 3e38
    else:
        raise ValueError(kind)
    return r


def bad_cases(dim, n=7, seed=0):
    """[(kind, position, x, m2)]: each kind of bad row, and an over-bound row ("over", under the bound m2 = the largest
    s of the other rows), at row 0, in the middle and last of n Gaussian rows.  m2 is None for the bad kinds: from the data."""
    out = []
    for ki, kind in enumerate(BAD_KINDS + ("over",)):
        for pos in (0, n // 2, n - 1):
            rng = np.random.default_rng(seed + 10 * ki + pos + 100 * dim)
            x = case_rows(n, dim, seed=ki + 1)
            if kind == "over":
                others = np.arange(n) != pos
                m2 = max_model(x[others])
                x[pos] = x[others][np.argmax(sq_norm_model(x[others]))] * np.float32(1.5)
                out.append((kind, pos, x, m2))
            else:
                x[pos] = bad_row(kind, dim, rng)
                out.append((kind, pos, x, None))
    return out


def epilogue_case(n, k, seed=0):
    """(ids, dist, c): sorted rows of distances >= c's share, the last entries of some rows padding (-1 / FLT_MAX)."""
    rng = np.random.default_rng(7000 + 10 * n + k + seed)
    c = (rng.random(n) * 50 + 1).astype(np.float32)
    dist = np.sort((rng.random((n, k)) * 100).astype(np.float32), axis=1)
    ids = rng.integers(0, 1 << 40, (n, k)).astype(np.int64)
    pad = rng.integers(0, k + 1, n)
    pad[0] = 0
    pad[-1] = k if n > 1 else pad[-1]
    for i in range(n):
        if pad[i]:
            ids[i, k - pad[i]:] = -1
            dist[i, k - pad[i]:] = np.finfo(np.float32).max
    return ids, dist, c


def cases():
    return [(n, dim) for dim in DIMS for n in NS]
