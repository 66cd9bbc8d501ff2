"""The model of the tail fold (cph_add: a graph-routed search on an index with added rows), shared by the CPU and the GPU
tests: inputs for cph_host_tail_fold / cph_tail_fold_hook and the numpy statement of what they must return.

Row i of the answer = the first k entries of the stable merge of the graph's row G_i and the exact top-k T_i of the tail:
    order = argsort(concatenate([G_i, T_i]), kind="stable")[:k]
compared as float values, so the graph's entry comes first where two are equal and padding (-1 / FLT_MAX) stays last."""
import numpy as np

FMAX = np.finfo(np.float32).max
FOLD_KS = (1, 10, 64, 65, 1000, 1024)
FOLD_PS = (1, 2, 5)
FOLD_N = 7
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def pool_capacity(k):
    kp = 64
    while kp < k:
        kp *= 2
    return 2 * kp


def keys_of(dist, ids):
    return (dist.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)


def fold_model(g_ids, g_dist, pools, counts, k):
    """numpy statement: g_* [n][k], pools [P][n][C] u64 keys, counts [P][n]."""
    P, n, _ = pools.shape
    out_i, out_d = np.empty((n, k), np.int64), np.empty((n, k), np.float32)
    for q in range(n):
        keys = np.sort(np.concatenate([pools[p, q, :counts[p, q]] for p in range(P)]))[:k]
        t_d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        t_i = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        order = np.argsort(np.concatenate([g_dist[q], t_d]), kind="stable")[:k]
        out_i[q] = np.concatenate([g_ids[q], t_i])[order]
        out_d[q] = np.concatenate([g_dist[q], t_d])[order]
    return out_i, out_d


def fold_case(k, P, seed):
    """One batch of FOLD_N queries whose rows cover, in order: a full graph row against one tail entry; a partly padded
    row against fewer than k; an all-padding row against exactly k; a row with duplicate ids against an empty tail; a row
    whose values also occur in the tail (the graph's entry first) against a tail with equal distance bits (ordered by
    id); every list full (the union holds more than k); a partly padded row against an empty tail."""
    rng = np.random.default_rng(seed)
    n, C = FOLD_N, pool_capacity(k)
    base = 100000                                   # tail ids lie behind every graph id
    g_ids = np.full((n, k), -1, np.int64)
    g_dist = np.full((n, k), FMAX, np.float32)
    tails = []
    for q in range(n):
        gn = (k, max(k // 2, 0), 0, k, k, k, k // 3)[q]
        d = np.sort(rng.random(gn).astype(np.float32) * np.float32(4.0))
        g_dist[q, :gn] = d
        g_ids[q, :gn] = rng.integers(0, base, gn)
        if q == 3 and gn >= 2:                      # duplicate ids (and their equal distances), as the graph search may return
            g_ids[q, 1] = g_ids[q, 0]
            g_dist[q, 1] = g_dist[q, 0]
        tn = (1, max(k - 1, 0) // 2, k, 0, k, P * k, 0)[q]
        td = rng.random(tn).astype(np.float32) * np.float32(4.0)
        if q == 4 and tn:
            td[: (tn + 1) // 2] = g_dist[q, rng.integers(0, gn, (tn + 1) // 2)]     # ties with graph entries ...
            td[tn // 2:] = td[tn // 2]                                                # ... and equal bits inside the tail
        ti = base + rng.permutation(4 * max(tn, 1))[:tn]
        tails.append(np.sort(keys_of(td, ti)))
    pools = np.full((P, n, C), NO_KEY, np.uint64)
    counts = np.zeros((P, n), np.uint32)
    for q, keys in enumerate(tails):
        # dealt out to the P lists (every list ascending, at most k keys each)
        owner = rng.integers(0, P, len(keys)) if len(keys) <= k else np.arange(len(keys)) % P
        for p in range(P):
            mine = keys[owner == p][:k]
            pools[p, q, :len(mine)] = mine
            counts[p, q] = len(mine)
    return g_ids, g_dist, pools, counts, C
