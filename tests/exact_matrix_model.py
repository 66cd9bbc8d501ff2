"""What the tests of the exact scan's matrix engine share: the planner's cut of a batch (cph_host_exact_matrix_plan), the
slack of a query (cph_host_exact_matrix_slack), and, from REFERENCE distances, how many candidates a pool of the prefilter
may have to hold -- so that `matrix_redo == 0` is asserted only on inputs of which the reference says no pool overflows.

A pool is compacted over the candidates of a prefix of its part (32 columns at a time), the certify kernel folds whole
parts, and a compaction keeps what lies within tau^ + 2 eps of the k-th approximate distance, which is within 4 eps of the
k-th exact one (|d^ - d| <= eps, twice on either side).  need() is the largest number of candidates any such prefix holds
within that band; a query is flagged only if need + 64 > C."""
import ctypes as C

import numpy as np

U = 2.0 ** -24
DEFAULT_BUDGET_MB = 1024                   # the pool budget of a handle made without CPH_EXACT_SCRATCH_MB


def gamma(n):
    return n * U / (1 - n * U)


def plan(m, nq, k, mb):
    """The cut of m candidates, nq queries at k under a pool budget of mb MiB on device 0."""
    import torch
    from cphnsw_mi355x import _lib
    out = (C.c_uint64 * 6)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.check(_lib.lib().cph_host_exact_matrix_plan(m, nq, k, cus, mb << 20, out))
    return dict(zip(("Kp", "C", "tile_q", "P", "part", "pool_keys"), (int(x) for x in out)))


def slack(qn, bn_max, D):
    from cphnsw_mi355x import _lib
    out = C.c_float()
    eps = np.empty(len(qn))
    for i, x in enumerate(qn):
        _lib.check(_lib.lib().cph_host_exact_matrix_slack(float(x), float(bn_max), D, C.byref(out)))
        eps[i] = out.value
    return eps


def slack_of(Q, X, D):
    """Every query's slack from float64 norms of the queries Q and the stored rows X, rounded up by what a stored float32
    norm may differ: a float32 reduction of at most D terms is within gamma(D + 3) (device_exact_mfma.h)."""
    up = 1 + 2 * gamma(D + 3)
    bn_max = float((np.asarray(X, np.float64) ** 2).sum(1).max()) * up
    return slack((np.asarray(Q, np.float64) ** 2).sum(1) * up, bn_max, D)


def need(dist, k, eps, pl):
    """Per query: the most candidates within 4 eps of the k-th smallest exact distance, over every prefix a compaction can
    see -- the first 32 j columns of a part, and for the fold of the certify kernel the first p parts."""
    m = dist.shape[1]
    out = np.zeros(len(dist), np.int64)
    band = 4.0 * eps * (1 + 1e-6)
    spans = [(lo, min(e, lo + pl["part"], m)) for lo in range(0, m, pl["part"]) for e in range(lo + 32, lo + pl["part"] + 32, 32)]
    spans += [(0, min(e, m)) for e in range(pl["part"], m + pl["part"], pl["part"])]
    for lo, hi in sorted(set(spans)):
        if hi - lo <= k or hi <= lo:
            continue                                             # (fewer than k + 1 candidates: nothing beside the k)
        sub = dist[:, lo:hi].astype(np.float64)
        kth = np.partition(sub, k - 1, axis=1)[:, k - 1]
        out = np.maximum(out, (sub <= (kth + band)[:, None]).sum(1))
    return out


def may_flag(dist, k, eps, pl):
    """Per query: the reference allows the prefilter to flag it."""
    return need(dist, k, eps, pl) + 64 > pl["C"]
