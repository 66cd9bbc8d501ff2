"""The statement of the exact rescoring stage of multi-vector search (search_maxsim(..., rescore=R)) in numpy, the synthetic
vectors, keys and candidates the host twin (cph_host_maxsim_rescore) and the kernel hook (cph_maxsim_rescore_hook) are
compared with it on, and the inverted key column (cph_host_key_rows) as a stable argsort.

Per query: f <= R candidate keys with lower bounds lb_j in (lb, key) order (the lower-bound statement, maxsim_model.py, at
k = R), T token rows of which the first L are live, and an allowed set (None: every id).  For every candidate and live token
  best_t = min over the allowed ids of the key of (bits(d(q_t, id)), id),
d being given by a callable -- dist_rows(q, t) -> float32 [n_ids], the distance of token t of query q to EVERY id (exact_l2
on a handle, or OracleTokenDists over free arrays, as diverse_model.OraclePairs over orc_dot) -- and
  score = ((+0.0 + d_0) + d_1) + ... in float32 over t < L.
The answer: the min(k, f) candidates with the smallest (score bits, key), with hits = L and rows[t] = the id of best_t (-1 for
t >= L); padding key 0, score FLT_MAX, hits 0, rows -1; certified = the leading slots whose score is strictly below lb_{R-1},
or found when f < R."""
import ctypes as C

import numpy as np

from maxsim_model import FMAX, I32_MAX, I32_MIN, same_bytes  # noqa: F401  (re-exported)


def _allow_of(allow, q):
    if allow is None:
        return None
    allow = np.asarray(allow, bool)
    return allow if allow.ndim == 1 else allow[q]


def rescore_model(cand_keys, cand_lb, f, L, T, key_of, dist_row, allow, k, rows=None):
    """One query -> (keys [k] int32, score [k] float32, hits [k] int32, rows [k, T] int64, found, certified).
    dist_row(t) -> float32 [n_ids]; allow: bool [n_ids] or None."""
    cand_keys, cand_lb = np.asarray(cand_keys, np.int32), np.asarray(cand_lb, np.float32)
    R, f = len(cand_keys), int(f)
    key_of = np.asarray(key_of, np.int32)
    out_keys, out_score = np.zeros(k, np.int32), np.full(k, FMAX, np.float32)
    out_hits, out_rows = np.zeros(k, np.int32), np.full((k, T), -1, np.int64)
    drows = [np.asarray(dist_row(t), np.float32) for t in range(L)]
    score = np.zeros(f, np.float32)                      # +0.0
    arg = np.full((f, T), -1, np.int64)
    for j in range(f):
        members = np.flatnonzero(key_of == cand_keys[j])
        if allow is not None:
            members = members[allow[members]]
        assert members.size, "a candidate key has an allowed row"
        s = np.float32(0.0)
        for t in range(L):
            d = drows[t][members]
            assert not np.signbit(d).any()
            best = np.lexsort((members, d.view(np.uint32)))[0]
            arg[j, t] = members[best]
            s = np.float32(s + d[best])                  # float32 + float32, one rounding, in token order
        score[j] = s
    order = np.lexsort((np.arange(f), cand_keys[:f].astype(np.int64), score.view(np.uint32)))[:k]
    found = len(order)
    out_keys[:found] = cand_keys[order]
    out_score[:found] = score[order]
    out_hits[:found] = L
    for o, j in enumerate(order):
        out_rows[o, :L] = arg[j, :L] if rows is None else rows[arg[j, :L]]
    if f < R:
        certified = found
    else:
        below = out_score[:found] < cand_lb[R - 1]
        certified = found if below.all() else int(np.argmin(below))
    return out_keys, out_score, out_hits, out_rows, found, certified


def rescore_model_batch(cand_keys, cand_lb, cand_found, n_tokens, T, key_of, dist_rows, allow, k, rows=None):
    """cand_keys / cand_lb [n, R], cand_found [n]; dist_rows(q, t) -> float32 [n_ids]; allow: None, bool [n_ids] or
    bool [n, n_ids] -> the six outputs."""
    n = len(cand_found)
    out = (np.empty((n, k), np.int32), np.empty((n, k), np.float32), np.empty((n, k), np.int32), np.empty((n, k, T), np.int64),
           np.empty(n, np.int32), np.empty(n, np.int32))
    for q in range(n):
        r = rescore_model(cand_keys[q], cand_lb[q], cand_found[q], T if n_tokens is None else int(n_tokens[q]), T, key_of,
                          lambda t, q=q: dist_rows(q, t), _allow_of(allow, q), k, rows)
        for o, v in zip(out, r):
            o[q] = v
    return out


def key_rows_model(keys):
    """-> (ids uint32 [n] by (key, id), distinct keys int32 ascending, offsets uint32 [distinct + 1])."""
    keys = np.asarray(keys, np.int32)
    ids = np.argsort(keys, kind="stable").astype(np.uint32)
    ukeys = np.unique(keys)
    offs = np.concatenate([np.searchsorted(keys[ids], ukeys, side="left"), [len(keys)]]).astype(np.uint32)
    return ids, ukeys, offs


# ---- the pair distance from the oracle's free-array dot --------------------------------------------------------------------
class OracleTokenDists:
    """dist_rows(q, t) over raw [n_ids, D] (zero-padded rows), norm_sq [n_ids] and tokens [n, T, dim]: the oracle's
    eight-chain dot (orc_dot) for dot(q_t, id) and for qnorm = dot(q_t, q_t) over the zero-padded token, then float32
    (qnorm + norm_sq[id]) - 2 * dot clamped at 0: the bytes of exact_l2.  Every row is computed once."""

    def __init__(self, raw, norm_sq, tokens):
        from oracle_lib import Oracle
        self.raw = np.ascontiguousarray(raw, np.float32)
        self.norm_sq = np.ascontiguousarray(norm_sq, np.float32)
        n, T, dim = tokens.shape
        self.D = self.raw.shape[1]
        self.tok = np.zeros((n, T, self.D), np.float32)
        self.tok[:, :, :dim] = tokens
        self._orc = Oracle()
        self._dot = self._orc.lib["orc_dot"]      # (a function object of its own: oracle_lib sets other argtypes on its)
        self._dot.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self._dot.restype = C.c_int
        self._rows = {}

    def _dots(self, pq, count):
        out = np.empty(count, np.float32)
        base, stride, o, f, D = self.raw.ctypes.data, self.D * 4, out.ctypes.data, self._dot, self.D
        for j in range(count):
            f(D, pq, base + j * stride, o + 4 * j)
        return out

    def __call__(self, q, t):
        if (q, t) not in self._rows:
            pq = self.tok[q, t].ctypes.data
            qn = np.empty(1, np.float32)
            self._dot(self.D, pq, pq, qn.ctypes.data)
            v = (qn[0] + self.norm_sq) - np.float32(2) * self._dots(pq, self.raw.shape[0])
            assert v.dtype == np.float32
            self._rows[q, t] = np.where(v > 0, v, np.float32(0))
        return self._rows[q, t]


# ---- synthetic vectors, keys and candidates ----------------------------------------------------------------------------------
# Keys by segment length (the 64-candidate edges of the scan), the ends of int32, a duplicated vector under two ids of one
# key, and two keys with identical rows.  `big` >= 2,000 only where asked for (the orc_dot model walks every row).
SEG_KEYS = {1: 11, 63: 12, 64: 13, 65: 14, 200: 15}
KEY_BIG, KEY_DUP, KEY_SAME_A, KEY_SAME_B, KEY_HALF = 16, 17, -5, 900, 18
SPECIAL_KEYS = (I32_MIN, I32_MAX, -1)


def synth_index(D, dim, big=0, seed=0):
    """-> dict(raw [n_ids, D], norm_sq, key_of int32 [n_ids], dup=(lo id, hi id), same=(key a, key b)).  The ids of every
    key are scattered over the id space (a random permutation), so a segment is never a run of consecutive ids."""
    rng = np.random.default_rng(104729 * D + 31 * dim + big + seed)
    keys = []
    for length, key in SEG_KEYS.items():
        keys += [key] * length
    keys += [KEY_BIG] * big
    keys += [KEY_DUP] * 6 + [KEY_SAME_A] * 3 + [KEY_SAME_B] * 3
    keys += list(SPECIAL_KEYS) * 2
    keys += list(range(1000, 1040))                       # singletons
    keys += [KEY_HALF] * len(keys)                        # one key owns half the rows
    keys = np.array(keys, np.int64)
    n_ids = len(keys)
    perm = rng.permutation(n_ids)
    key_of = np.empty(n_ids, np.int32)
    key_of[perm] = keys.astype(np.int32)
    raw = np.zeros((n_ids, D), np.float32)
    raw[:, :dim] = rng.standard_normal((n_ids, dim)).astype(np.float32)
    dup = np.flatnonzero(key_of == KEY_DUP)
    raw[dup[3]] = raw[dup[1]]                             # one vector under two ids of one key: the lower id wins
    a, b = np.flatnonzero(key_of == KEY_SAME_A), np.flatnonzero(key_of == KEY_SAME_B)
    raw[b] = raw[a]                                       # two keys with identical rows: the key order decides
    norm = (raw.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    norm[dup[3]] = norm[dup[1]]
    norm[b] = norm[a]
    return dict(raw=raw, norm_sq=norm, key_of=key_of, dup=(int(dup[1]), int(dup[3])), same=(KEY_SAME_A, KEY_SAME_B), dim=dim)


def synth_tokens(ix, n_tokens, T, seed=0):
    """len(n_tokens) queries of T token rows around rows of the index; garbage (huge values) in the rows t >= n_tokens."""
    rng = np.random.default_rng(seed + 17 * T)
    raw, dim = ix["raw"], ix["dim"]
    n = len(n_tokens)
    base = raw[rng.integers(0, len(raw), (n, T)), :dim]
    tok = (base + np.float32(0.3) * rng.standard_normal(base.shape)).astype(np.float32)
    for q, L in enumerate(n_tokens):
        tok[q, L:] = np.float32(1e30)
    return tok


def synth_candidates(key_of, n, R, founds, seed=0, must=()):
    """cand_keys int32 [n, R], cand_lb float32 [n, R], cand_found int32 [n]: query q gets founds[q] <= R distinct keys of
    the column -- `must` first where they fit -- with made-up ascending lower bounds (the hook takes them as given); the
    slots behind found hold garbage."""
    rng = np.random.default_rng(seed + R)
    ukeys = np.unique(key_of)
    ck = rng.integers(-2 ** 31, 2 ** 31, (n, R)).astype(np.int32)
    lb = rng.random((n, R), dtype=np.float32)
    cf = np.array(founds, np.int32)
    for q in range(n):
        f = int(cf[q])
        assert f <= min(R, len(ukeys))
        rest = rng.permutation(np.setdiff1d(ukeys, np.array(must, np.int64)))
        chosen = np.concatenate([np.array(must, np.int64), rest])[:f]
        ck[q, :f] = rng.permutation(chosen).astype(np.int32)
        lb[q, :f] = np.sort(rng.random(f, dtype=np.float32) * np.float32(30.0))
    return ck, lb, cf


def bitmap_words(allow, n_ids):
    """bool [..., n_ids] -> uint32 words [..., (n_ids + 31) // 32], bit id & 31 of word id >> 5."""
    allow = np.asarray(allow, bool)
    nw = (n_ids + 31) // 32
    pad = np.zeros(allow.shape[:-1] + (nw * 32,), bool)
    pad[..., :n_ids] = allow
    return np.ascontiguousarray(np.packbits(pad, axis=-1, bitorder="little")).view(np.uint32)


# ---- the library's implementations (host twin, kernel hook, host key rows) -----------------------------------------------------
def _outs(n, k, T):
    return (np.full((n, k), -7, np.int32), np.full((n, k), -7, np.float32), np.full((n, k), -7, np.int32),
            np.full((n, k, T), -7, np.int64), np.full(n, -7, np.int32), np.full(n, -7, np.int32))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _allow_words(allow, n, n_ids):
    if allow is None:
        return None
    allow = np.asarray(allow, bool)
    if allow.ndim == 1:
        allow = np.broadcast_to(allow, (n, n_ids))
    return bitmap_words(allow, n_ids)


def host_maxsim_rescore(cand_keys, cand_lb, cand_found, tokens, n_tokens, raw, norm_sq, key_of, allow, k, rows=None):
    from cphnsw_mi355x import _lib
    n, R = cand_keys.shape
    _, T, dim = tokens.shape
    ck, lb, cf = (np.ascontiguousarray(cand_keys, np.int32), np.ascontiguousarray(cand_lb, np.float32),
                  np.ascontiguousarray(cand_found, np.int32))
    tok = np.ascontiguousarray(tokens, np.float32)
    nt = None if n_tokens is None else np.ascontiguousarray(n_tokens, np.int32)
    raw, norm_sq = np.ascontiguousarray(raw, np.float32), np.ascontiguousarray(norm_sq, np.float32)
    key_of = np.ascontiguousarray(key_of, np.int32)
    words = _allow_words(allow, n, raw.shape[0])
    rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
    out = _outs(n, k, T)
    _lib.check(_lib.lib().cph_host_maxsim_rescore(ck.ctypes.data, lb.ctypes.data, cf.ctypes.data, n, R, tok.ctypes.data, T, dim, _ptr(nt),
                                                  raw.ctypes.data, norm_sq.ctypes.data, raw.shape[0], raw.shape[1], key_of.ctypes.data,
                                                  _ptr(words), _ptr(rows), k, *[o.ctypes.data for o in out]))
    return out


def hook_maxsim_rescore(ix, cand_keys, cand_lb, cand_found, tokens, n_tokens, keys, allow, k):
    """The pad, scan and select kernels on the given candidates against the vectors of the (single-device) index ix;
    keys: a GroupKeys of ix, or None (its label column)."""
    from cphnsw_mi355x import _lib
    n, R = cand_keys.shape
    _, T, _ = tokens.shape
    ck, lb, cf = (np.ascontiguousarray(cand_keys, np.int32), np.ascontiguousarray(cand_lb, np.float32),
                  np.ascontiguousarray(cand_found, np.int32))
    tok = np.ascontiguousarray(tokens, np.float32)
    nt = None if n_tokens is None else np.ascontiguousarray(n_tokens, np.int32)
    words = _allow_words(allow, n, ix.size)
    out = _outs(n, k, T)
    _lib.check(_lib.lib().cph_maxsim_rescore_hook(ix._h, ck.ctypes.data, lb.ctypes.data, cf.ctypes.data, n, R, tok.ctypes.data, T, _ptr(nt),
                                                  None if keys is None else keys._hs[0], _ptr(words), k,
                                                  *[o.ctypes.data for o in out]))
    return out


def host_key_rows(keys):
    from cphnsw_mi355x import _lib
    keys = np.ascontiguousarray(keys, np.int32)
    n = keys.size
    ids, ukeys, offs = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, -7, np.int32), np.full(n + 1, 0xA5A5A5A5, np.uint32)
    nk = C.c_uint64(0)
    _lib.check(_lib.lib().cph_host_key_rows(_ptr(keys) if n else None, n, ids.ctypes.data, ukeys.ctypes.data, offs.ctypes.data, C.byref(nk)))
    return ids, ukeys[:nk.value], offs[:nk.value + 1]
