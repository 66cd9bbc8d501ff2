"""The statement of multi-vector (MaxSim) search (search_maxsim) in numpy, and the synthetic candidate rows the host twin
(cph_host_maxsim_rows) and the kernel hook (cph_maxsim_rows_hook) are compared with it on.

A query has T token rows of C candidates each, of which the first L are live; a candidate row is what the ordinary search
returns at k = C (ids, dist; padding -1 / FLT_MAX).  An entry is valid when 0 <= id < n_ids.  Per live token t:
  floor_t   = the distance of the last valid entry of the row, +0.0 when there is none;
  pos_t(κ)  = the lowest position whose entry has key κ; term_t(κ) = the distance there, else floor_t.
score(κ) = ((+0.0 + term_0) + term_1) + ... in float32, hits(κ) = the live tokens that have a pos_t(κ).  The answer: the
min(k, distinct keys) keys with the smallest (score, key), with rows[t] = the id at pos_t(κ) or -1.  Padding: key 0, score
FLT_MAX, hits 0, rows -1."""
import numpy as np

FMAX = np.float32(3.4028234663852886e38)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

# every power-of-two boundary of the kernel's sort: T * C = 1, 64, 126, 195, 511, 2048, 5000, 8192, 8192
TCS = ((1, 1), (1, 64), (2, 63), (3, 65), (7, 73), (32, 64), (5, 1000), (8, 1024), (64, 128))
KS = (1, 10, 1024)


def shapes():
    return [(T, C, k) for (T, C) in TCS for k in KS]


def maxsim_model(ids, dist, L, key_of, n_ids, k, rows=None):
    """One query: ids int64 [T, C], dist float32 [T, C] -> (keys [k] int32, score [k] float32, hits [k] int32,
    rows [k, T] int64, found)."""
    ids = np.asarray(ids, np.int64)
    dist = np.asarray(dist, np.float32)
    T, C = ids.shape
    out_keys, out_score = np.zeros(k, np.int32), np.full(k, FMAX, np.float32)
    out_hits, out_rows = np.zeros(k, np.int32), np.full((k, T), -1, np.int64)
    live_ids = ids[:L]
    valid = (live_ids >= 0) & (live_ids < n_ids)
    if not valid.any():
        return out_keys, out_score, out_hits, out_rows, 0
    keys = np.where(valid, key_of[np.where(valid, live_ids, 0)], 0).astype(np.int64)
    ukeys = np.unique(keys[valid])
    U = len(ukeys)
    score = np.zeros(U, np.float32)                     # +0.0
    hits = np.zeros(U, np.int32)
    at = np.full((U, T), -1, np.int64)                  # pos_t of every key
    for t in range(L):
        js = np.flatnonzero(valid[t])
        term = np.full(U, dist[t, js[-1]] if js.size else np.float32(0.0), np.float32)         # floor_t
        if js.size:
            u, first = np.unique(np.searchsorted(ukeys, keys[t, js]), return_index=True)      # first: the lowest position of each
            at[u, t] = js[first]
            term[u] = dist[t, js[first]]
            hits[u] += 1
        score = (score + term).astype(np.float32)       # float32 + float32, one rounding, in token order
    order = np.lexsort((ukeys, score))[:k]
    found = len(order)
    out_keys[:found] = ukeys[order]
    out_score[:found] = score[order]
    out_hits[:found] = hits[order]
    for o, u in enumerate(order):
        ts = np.flatnonzero(at[u] >= 0)
        got = ids[ts, at[u, ts]]
        out_rows[o, ts] = got if rows is None else rows[got]
    return out_keys, out_score, out_hits, out_rows, found


def maxsim_model_batch(ids, dist, n_tokens, key_of, n_ids, k, rows=None):
    n, T, _ = ids.shape
    out = (np.empty((n, k), np.int32), np.empty((n, k), np.float32), np.empty((n, k), np.int32), np.empty((n, k, T), np.int64),
           np.empty(n, np.int32))
    for q in range(n):
        r = maxsim_model(ids[q], dist[q], T if n_tokens is None else int(n_tokens[q]), key_of, n_ids, k, rows)
        for o, v in zip(out, r):
            o[q] = v
    return out


# ---- synthetic queries ---------------------------------------------------------------------------------------------------
# The id space is cut into regions whose keys are chosen so that a query drawn from one region has the property its name
# says.  N_IDS is odd on purpose.
REGION = 8400                                           # (a query holds up to 8,192 entries)
R_ONE, R_DISTINCT, R_SPECIAL, R_MANY, R_FEW, R_SOLO = (i * REGION for i in range(6))
N_IDS = 6 * REGION + 1
KINDS = ("one_key", "distinct_keys", "special_keys", "repeated_ids", "padding_token", "partly_padded", "all_padded",
         "equal_distances", "negative_distances", "tied_scores", "few_keys", "one_token_key", "many_keys")
SPECIAL = (I32_MIN, -1, 0, 1, I32_MAX)
TIE_HI, TIE_LO = 900001, -900001                        # the two keys of a "tied_scores" query


def synth_keys():
    key_of = np.zeros(N_IDS, np.int32)
    key_of[R_ONE:R_ONE + REGION] = 7
    key_of[R_DISTINCT:R_DISTINCT + REGION] = 100000 + np.arange(REGION)
    key_of[R_SPECIAL:R_SPECIAL + REGION] = np.array(SPECIAL, np.int64)[np.arange(REGION) % 5].astype(np.int32)
    key_of[R_MANY:R_MANY + REGION] = np.arange(REGION) % 37 - 5
    key_of[R_FEW:R_FEW + REGION] = np.arange(REGION) % 3
    key_of[R_SOLO:R_SOLO + REGION] = 500000 + np.arange(REGION)
    key_of[R_SOLO] = TIE_HI
    key_of[R_SOLO + 1] = TIE_LO
    key_of[-1] = -77
    return key_of


def _draw(rng, lo, T, C):
    return (lo + rng.permutation(REGION)[:T * C]).reshape(T, C).astype(np.int64)


def synth_query(kind, T, C, L, rng):
    """One query (ids int64 [T, C], dist float32 [T, C]) of the named kind; the rows of the tokens t >= L hold garbage."""
    dist = np.sort(rng.random((T, C), dtype=np.float32) * np.float32(4.0) + np.float32(0.5), axis=1)
    if kind == "one_key":
        ids = _draw(rng, R_ONE, T, C)
    elif kind == "distinct_keys":
        ids = _draw(rng, R_DISTINCT, T, C)
    elif kind == "special_keys":
        ids = _draw(rng, R_SPECIAL, T, C)
    elif kind == "few_keys":
        ids = _draw(rng, R_FEW, T, C)
    else:
        ids = _draw(rng, R_MANY, T, C)
    if kind == "repeated_ids" and C >= 2:
        ids[:, C // 2] = ids[:, 0]                       # twice in every row
        if C >= 6:
            ids[:, 3] = ids[:, 1]                        # three times, one of them far away
            ids[:, C - 1] = ids[:, 1]
    elif kind == "padding_token":
        t = min(1, L - 1)                                # (L = 1: the query is all padding)
        ids[t], dist[t] = -1, FMAX
    elif kind == "partly_padded":
        for t in range(T):
            cut = (C * (t + 1)) // (T + 1)               # row t keeps `cut` entries: from none (C < T + 1) to most
            ids[t, cut:], dist[t, cut:] = -1, FMAX
        if C >= 4:
            ids[0, 1], dist[0, 1] = -1, FMAX             # a hole in front of valid entries: the floor is by position
    elif kind == "all_padded":
        ids[:], dist[:] = -1, FMAX
    elif kind == "equal_distances":
        dist = np.sort(rng.integers(0, 3, (T, C)).astype(np.float32), axis=1)
        zeros = np.argwhere(dist == 0)
        pick = zeros[rng.random(len(zeros)) < 0.5]
        dist[pick[:, 0], pick[:, 1]] = np.float32(-0.0)
        if C >= 2:
            dist[0, 0], dist[0, 1] = np.float32(-0.0), np.float32(0.0)          # side by side, whatever was drawn
    elif kind == "negative_distances":
        m = min(C, 3)
        dist[:, :m] = np.sort(-rng.random((T, m), dtype=np.float32) * np.float32(1e-6), axis=1)
    elif kind == "tied_scores" and C >= 2:
        # in every row the first two entries are one id of each tie key at ONE distance, the larger key in front: the
        # sums are bit-equal and the key order, not the position, decides
        ids[:, 0], ids[:, 1] = R_SOLO, R_SOLO + 1
        dist[:, 1] = dist[:, 0]
    elif kind == "one_token_key":
        # a key of its own at the front of token 0 only, nearer than everything: its score is that distance plus the
        # floors of all the other tokens
        ids[0, 0] = R_SOLO + 2
        dist[0, 0] = np.float32(0.25)
    if L < T:
        ids[L:] = rng.integers(-2 ** 62, 2 ** 62, (T - L, C))
        ids[L:, ::3] = rng.integers(0, N_IDS, ids[L:, ::3].shape)              # (some of the garbage looks valid)
        dist[L:] = rng.integers(0, 2 ** 32, (T - L, C), dtype=np.uint64).astype(np.uint32).view(np.float32)
    return ids, dist


def synth_batch(T, C, n=3 * len(KINDS), seed=0, first=0):
    """n queries cycling through KINDS from kind `first` on, their n_tokens through (T, 1, T - 1) -> (ids [n, T, C],
    dist [n, T, C], n_tokens int32 [n], key_of [N_IDS], rows uint32 [N_IDS], kinds [n]).  13 kinds and 3 lengths: 39
    queries hold every pair.  rows: a permutation of the id space (the row map of the 'with a row map' half of a case)."""
    rng = np.random.default_rng(1000003 * seed + 8191 * T + C)
    kinds = [KINDS[(first + i) % len(KINDS)] for i in range(n)]
    n_tokens = np.array([max(1, (T, 1, T - 1)[i % 3]) for i in range(n)], np.int32)
    qs = [synth_query(kind, T, C, int(L), rng) for kind, L in zip(kinds, n_tokens)]
    ids = np.stack([q[0] for q in qs])
    dist = np.stack([q[1] for q in qs])
    return ids, dist, n_tokens, synth_keys(), rng.permutation(N_IDS).astype(np.uint32), kinds


# ---- the library's two implementations (host twin, kernel hook) ------------------------------------------------------------
def _call_rows(fn, lead, ids, dist, n_tokens, key_of, rows, k):
    from cphnsw_mi355x import _lib
    n, T, C = ids.shape
    ids, dist = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(dist, np.float32)
    key_of = np.ascontiguousarray(key_of, np.int32)
    n_tokens = None if n_tokens is None else np.ascontiguousarray(n_tokens, np.int32)
    rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
    out = (np.full((n, k), -7, np.int32), np.full((n, k), -7, np.float32), np.full((n, k), -7, np.int32),
           np.full((n, k, T), -7, np.int64), np.full(n, -7, np.int32))
    _lib.check(fn(*lead, ids.ctypes.data, dist.ctypes.data, n, T, None if n_tokens is None else n_tokens.ctypes.data, C,
                  key_of.ctypes.data, key_of.size, None if rows is None else rows.ctypes.data, k, *[o.ctypes.data for o in out]))
    return out


def host_maxsim_rows(ids, dist, n_tokens, key_of, k, rows=None):
    from cphnsw_mi355x import _lib
    return _call_rows(_lib.lib().cph_host_maxsim_rows, (), ids, dist, n_tokens, key_of, rows, k)


def hook_maxsim_rows(device, ids, dist, n_tokens, key_of, k, rows=None):
    from cphnsw_mi355x import _lib
    return _call_rows(_lib.lib().cph_maxsim_rows_hook, (int(device),), ids, dist, n_tokens, key_of, rows, k)


def same_bytes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
