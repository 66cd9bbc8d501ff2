"""The statement of grouped search (search_grouped) in plain numpy / Python, and the synthetic candidate rows the host twin
(cph_host_group_rows) and the kernel hook (cph_group_rows_hook) are compared with it on.

A query's candidate row is what the ordinary search returns at k = C: C entries ascending by (distance, id), padded with
-1 / FLT_MAX.  key_of[id] is an int32 per internal id.  Walk the row front to back:
  - skip padding;
  - skip an id that already occurred earlier in the row;
  - if the entry's key has no group yet and fewer than k groups exist, open a group for it at the next group index;
  - if the key has a group with fewer than g members, append the entry to it;
  - otherwise drop the entry.
complete = (k groups exist and each has g members) or (the row holds fewer than C entries that are not padding)."""
import numpy as np

FMAX = np.float32(3.4028234663852886e38)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

CS = (1, 63, 64, 65, 70, 128, 1000, 1024)
KGS = ((1, 1), (3, 2), (10, 3), (64, 1), (1, 64), (32, 32))


def shapes():
    """(C, k, g) of the CPU and hook tests: every pair with k * g <= C."""
    return [(C, k, g) for C in CS for (k, g) in KGS if k * g <= C]


def group_model(ids_row, dist_row, key_of, k, g, rows=None):
    """-> (ids [k, g] int64, dist [k, g] float32, keys [k] int32, counts [k] int32, complete bool)."""
    ids_row = np.asarray(ids_row, np.int64)
    dist_row = np.asarray(dist_row, np.float32)
    C = ids_row.shape[0]
    ids = np.full((k, g), -1, np.int64)
    dist = np.full((k, g), FMAX, np.float32)
    keys = np.zeros(k, np.int32)
    counts = np.zeros(k, np.int32)
    group_of, seen, valid = {}, set(), 0
    for j in range(C):
        i = int(ids_row[j])
        if i < 0:
            continue
        valid += 1
        if i in seen:
            continue
        seen.add(i)
        key = int(key_of[i])
        if key not in group_of:
            if len(group_of) == k:
                continue
            group_of[key] = len(group_of)
            keys[group_of[key]] = key
        G = group_of[key]
        if counts[G] == g:
            continue
        ids[G, counts[G]] = i if rows is None else int(rows[i])
        dist[G, counts[G]] = dist_row[j]          # (a float32 copy: the bytes of the row, -0.0 included)
        counts[G] += 1
    complete = (len(group_of) == k and bool((counts == g).all())) or valid < C
    return ids, dist, keys, counts, complete


def group_model_batch(ids, dist, key_of, k, g, rows=None):
    n = ids.shape[0]
    out = (np.empty((n, k, g), np.int64), np.empty((n, k, g), np.float32), np.empty((n, k), np.int32), np.empty((n, k), np.int32),
           np.empty(n, np.uint8))
    for q in range(n):
        r = group_model(ids[q], dist[q], key_of, k, g, rows)
        for o, v in zip(out, r):
            o[q] = v
    return out


# ---- synthetic rows -------------------------------------------------------------------------------------------------------
# The id space is cut into regions whose keys are chosen so that a row drawn from one region has the property its name
# says.  N_IDS is odd on purpose.
REGION = 1100
R_ONE, R_DISTINCT, R_SPECIAL, R_MANY, R_FEW, R_FULL = (i * REGION for i in range(6))
N_FULL = 2048
N_IDS = R_FULL + N_FULL + 1
ROW_KINDS = ("one_key", "distinct_keys", "special_keys", "repeated_ids", "partly_padding", "all_padding", "equal_distances",
             "few_keys", "full_at_last", "full_before_last")


def synth_keys(k):
    key_of = np.zeros(N_IDS, np.int32)
    key_of[R_ONE:R_ONE + REGION] = 7
    key_of[R_DISTINCT:R_DISTINCT + REGION] = 1000 + np.arange(REGION)
    key_of[R_SPECIAL:R_SPECIAL + REGION] = np.array([I32_MIN, -1, 0, 1, I32_MAX], np.int64)[np.arange(REGION) % 5].astype(np.int32)
    key_of[R_MANY:R_MANY + REGION] = np.arange(REGION) % 37 - 5
    key_of[R_FEW:R_FEW + REGION] = np.arange(REGION) % 3
    key_of[R_FULL:R_FULL + N_FULL] = 200000 + np.arange(N_FULL) % k       # group j: the ids == j (mod k), at least g + 1 of them
    key_of[-1] = -77
    return key_of


def _sorted_dist(rng, C):
    return np.sort(rng.random(C, dtype=np.float32) * np.float32(4.0))


def _draw(rng, lo, size, C):
    return (lo + rng.permutation(size)[:C]).astype(np.int64)


def synth_row(kind, C, k, g, rng):
    """One candidate row (ids int64 [C], dist float32 [C]) of the named kind."""
    ids, dist = np.full(C, -1, np.int64), _sorted_dist(rng, C)
    if kind == "one_key":
        ids = _draw(rng, R_ONE, REGION, C)
    elif kind == "distinct_keys":
        ids = _draw(rng, R_DISTINCT, REGION, C)
    elif kind == "special_keys":
        ids = _draw(rng, R_SPECIAL, REGION, C)
    elif kind == "repeated_ids":
        ids = _draw(rng, R_MANY, REGION, C)
        if C >= 2:
            ids[C // 2] = ids[0]                       # twice
        if C >= 6:
            ids[3] = ids[1]                            # three times, one of them right behind ...
            ids[C - 1] = ids[1]                        # ... one far away (another chunk of the kernel when C > 64)
    elif kind == "partly_padding":
        ids = _draw(rng, R_MANY, REGION, C)
        cut = C * 2 // 3
        ids[cut:] = -1
        dist[cut:] = FMAX
    elif kind == "all_padding":
        dist[:] = FMAX
    elif kind == "equal_distances":
        ids = _draw(rng, R_MANY, REGION, C)
        dist = np.sort(rng.integers(0, 3, C).astype(np.float32))
        zeros = np.flatnonzero(dist == 0)
        dist[zeros[rng.random(zeros.size) < 0.5]] = np.float32(-0.0)      # equal as floats, other bytes: the order stays
    elif kind == "few_keys":
        ids = _draw(rng, R_FEW, REGION, C)
    else:
        # k groups of g members each; the entry that fills the last group sits at `at`, fillers (entries that are dropped)
        # lie between the first k * g - 1 members and it, and behind it
        at = C - 1 if kind == "full_at_last" else C - 2
        per_key = [list(R_FULL + j + k * rng.permutation(N_FULL // k)) for j in range(k)]
        members = [per_key[j].pop() for _ in range(g) for j in range(k)]          # round robin: group j opens at entry j
        head, last = members[:-1], members[-1]
        if at < len(head):                             # (C - 2 < k * g - 1: the row cannot hold a filler behind the last member)
            at = len(head)
        # a filler: a fresh id under the key of a group that is already full (groups 0 .. k - 2), else a repeated id, else
        # (k = g = 1: nothing but padding is dropped before the first entry) padding
        fresh = [i for j in range(k - 1) for i in per_key[j]]

        def filler():
            return fresh.pop() if fresh else (head[0] if head else -1)
        row = list(head) + [filler() for _ in range(at - len(head))] + [last]
        row += [filler() for _ in range(C - len(row))]
        ids = np.array(row[:C], np.int64)
        dist[ids < 0] = FMAX
    return ids, dist


def synth_batch(C, k, g, n=len(ROW_KINDS), seed=0, first=0):
    """n rows cycling through ROW_KINDS from kind `first` on -> (ids [n, C], dist [n, C], key_of [N_IDS], rows [N_IDS],
    kinds [n]).  rows: a permutation of the id space (the row map of the 'with a row map' half of every case)."""
    rng = np.random.default_rng(1000003 * seed + 8191 * C + 131 * k + g)
    kinds = [ROW_KINDS[(first + i) % len(ROW_KINDS)] for i in range(n)]
    rows_ = [synth_row(kind, C, k, g, rng) for kind in kinds]
    ids = np.stack([r[0] for r in rows_])
    dist = np.stack([r[1] for r in rows_])
    return ids, dist, synth_keys(k), rng.permutation(N_IDS).astype(np.uint32), kinds


# ---- the library's two implementations (host twin, kernel hook) ----------------------------------------------------------------
def _call_rows(fn, lead, ids, dist, key_of, rows, k, g):
    from cphnsw_mi355x import _lib
    n, C = ids.shape
    ids, dist = np.ascontiguousarray(ids, np.int64), np.ascontiguousarray(dist, np.float32)
    key_of = np.ascontiguousarray(key_of, np.int32)
    rows = None if rows is None else np.ascontiguousarray(rows, np.uint32)
    out = (np.full((n, k, g), -7, np.int64), np.full((n, k, g), -7, np.float32), np.full((n, k), -7, np.int32),
           np.full((n, k), -7, np.int32), np.full(n, 7, np.uint8))
    _lib.check(fn(*lead, ids.ctypes.data, dist.ctypes.data, n, C, key_of.ctypes.data, key_of.size,
                  None if rows is None else rows.ctypes.data, k, g, *[o.ctypes.data for o in out]))
    return out


def host_group_rows(ids, dist, key_of, k, g, rows=None):
    from cphnsw_mi355x import _lib
    return _call_rows(_lib.lib().cph_host_group_rows, (), ids, dist, key_of, rows, k, g)


def hook_group_rows(device, ids, dist, key_of, k, g, rows=None):
    from cphnsw_mi355x import _lib
    return _call_rows(_lib.lib().cph_group_rows_hook, (int(device),), ids, dist, key_of, rows, k, g)


def same_bytes(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))
