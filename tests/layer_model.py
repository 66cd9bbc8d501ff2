"""The statement of layer-0 selection (builder.h: select_layer) in plain numpy plus the oracle's restatement of the
selection rule, for the whole-layer and the hub tests.

A layer is a table knn[n][32] of forward candidates (kInvalidNode = none).  The reverse list of v holds every row u
with v in knn[u].  The candidates of v are its forward list followed by its reverse list -- unless the reverse list
has more than 96 entries (a hub): then select_kernel streams the reverse list through its upper 64 slots in chunks of
64, sorts and deduplicates after each chunk and keeps the lower 64 slots.  What that loop amounts to, and what this
model states, is the HUB CUT: of the unique valid ids of both lists other than v, the 64 nearest by (distance, id).
The cut is a deliberate property of the kernel (a hub's list is pruned from 64 candidates, C <= 64), not of the
reference's rule; it does not depend on the order of the reverse list."""
import numpy as np

INVALID = np.uint32(0xFFFFFFFF)
HUB_REV = 96        # more reverse edges than this: the hub path
HUB_KEEP = 64       # candidates a hub keeps


def reverse_lists(knn, n):
    """-> list of n uint32 arrays: for every v the sorted rows u with v in knn[u] (one entry per occurrence, as the CSR
    counts them; a table row without repeated ids gives each u once).  kInvalidNode entries are ignored."""
    knn = np.asarray(knn, np.uint32).reshape(n, -1)
    ok = knn != INVALID
    u = np.repeat(np.arange(n, dtype=np.uint32), knn.shape[1]).reshape(knn.shape)[ok]
    v = knn[ok]
    order = np.lexsort((u, v))
    u, v = u[order], v[order]
    cuts = np.cumsum(np.bincount(v, minlength=n))[:-1]
    return np.split(u, cuts)


def candidates(oracle, x, v, fwd, rev):
    """The candidate list select_kernel prunes for vertex v: fwd then rev, or the hub cut (see above).  The branch is
    taken on the raw length of rev, as the kernel takes it on the CSR segment's length."""
    fwd = np.asarray(fwd, np.uint32)
    rev = np.asarray(rev, np.uint32)
    if len(rev) <= HUB_REV:
        return np.concatenate([fwd, rev])
    ids = np.unique(np.concatenate([fwd, rev]))
    ids = ids[(ids != np.uint32(v)) & (ids != INVALID)]
    d = np.array([oracle.l2(x[v], x[c]) for c in ids], np.float32)
    return ids[np.lexsort((ids, d))][:HUB_KEEP]


def select_layer(oracle, x, knn, R, alpha, tau, amax, err, rows=None):
    """-> (ids uint32[n, 32] padded with kInvalidNode, counts uint32[n]) of every vertex (or of `rows` only; the
    other rows stay empty)."""
    n = x.shape[0]
    knn = np.asarray(knn, np.uint32)
    rev = reverse_lists(knn, n)
    ids = np.full((n, 32), INVALID, np.uint32)
    cnt = np.zeros(n, np.uint32)
    for v in (range(n) if rows is None else rows):
        got = oracle.select_neighbors(x, v, candidates(oracle, x, v, knn[v], rev[v]), R, alpha, tau, amax, err)
        ids[v, :len(got)] = got
        cnt[v] = len(got)
    return ids, cnt
