"""CPU tier of the per-query filters: cph_host_filter_groups, the grouping and routing of a batch whose queries carry
their own filters, against a numpy restatement; and cph_host_exact_group_plan, the work-item table of the grouped exact
scan: every (candidate, query) pair of every segment exactly once, at most 256 parts, pools within the budget."""
import ctypes as C

import numpy as np
import pytest

PAD, SCAN, GRAPH = 0, 1, 2


def _groups(filter_of, pop, k=10, exact=False, threshold=0):
    from cphnsw_mi355x import _lib
    fo = np.ascontiguousarray(filter_of, np.int32)
    pc = np.ascontiguousarray(pop, np.uint64)
    F, n = len(pc), len(fo)
    routes = np.full(F + 1, 99, np.uint8)
    perm = np.full(max(n, 1), 0xDEADBEEF, np.uint32)
    seg = np.full(F + 2, 0xDEADBEEF, np.uint32)
    _lib.check(_lib.lib().cph_host_filter_groups(fo.ctypes.data if n else None, n, pc.ctypes.data if F else None, F, k,
                                                 int(exact), threshold, routes.ctypes.data, perm.ctypes.data, seg.ctypes.data))
    return routes, perm[:n], seg


def _groups_np(filter_of, pop, k, exact, threshold):
    fo = np.asarray(filter_of, np.int64)
    F = len(pop)
    routes = [PAD if p == 0 else SCAN if (exact or (threshold > 0 and p <= threshold and k <= 1024)) else GRAPH for p in pop]
    routes.append(SCAN if exact else GRAPH)
    key = np.where(fo < 0, F, fo)
    perm = np.argsort(key, kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=F + 1))])
    return np.array(routes, np.uint8), perm.astype(np.uint32), seg.astype(np.uint32)


def _check_groups(fo, pop, k=10, exact=False, threshold=0):
    got = _groups(fo, pop, k, exact, threshold)
    want = _groups_np(fo, pop, k, exact, threshold)
    for g, w, what in zip(got, want, ("routes", "perm", "seg")):
        assert np.array_equal(g, w), (what, g, w)
    return got


def test_groups_are_stable_and_routed_like_the_single_filter_call():
    rng = np.random.default_rng(5)
    pop = [100000, 4000, 4001, 1, 0, 37]
    fo = rng.integers(-1, len(pop), 5000)
    for exact in (False, True):
        for thr in (0, 1, 4000, 10 ** 6):
            for k in (1, 10, 1024, 1025) if not exact else (1, 10, 1024):
                _check_groups(fo, pop, k, exact, thr)
    routes, perm, seg = _check_groups(fo, pop, 10, False, 4000)
    assert list(routes) == [GRAPH, SCAN, GRAPH, SCAN, PAD, SCAN, GRAPH]
    for f in range(len(pop) + 1):                      # inside a filter: query order
        part = perm[seg[f]:seg[f + 1]]
        assert (np.diff(part.astype(np.int64)) > 0).all()
        assert (fo[part] == (f if f < len(pop) else -1)).all()
    # k above the scan's limit: a small filter stays on the graph; exact routes -1 to the scan too
    assert list(_groups(fo, pop, 1025, False, 4000)[0]) == [GRAPH, GRAPH, GRAPH, GRAPH, PAD, GRAPH, GRAPH]
    assert list(_groups(fo, pop, 10, True, 0)[0]) == [SCAN, SCAN, SCAN, SCAN, PAD, SCAN, SCAN]


def test_groups_edge_shapes():
    _check_groups([0], [5])                            # n = 1
    _check_groups([-1], [5])
    _check_groups([-1], [])                            # no filter at all
    _check_groups([], [3, 0])                          # no query
    n = 300
    _check_groups(np.arange(n), np.arange(n), threshold=100)          # every query under its own filter (one empty)
    _check_groups(np.arange(n)[::-1].copy(), np.arange(n), exact=True)
    _check_groups(np.full(40, 2), [1, 2, 3])           # one filter for all
    _check_groups(np.full(40, -1), [1, 2, 3])          # only unfiltered queries
    r, _, seg = _check_groups([1, 1, -1], [0, 0], threshold=10)       # empty filters only
    assert list(r) == [PAD, PAD, GRAPH] and list(seg) == [0, 0, 2, 3]


@pytest.mark.parametrize("bad", [-2, 3, 2 ** 31 - 1, -2 ** 31])
def test_groups_refuse_values_outside_the_filter_list(bad):
    with pytest.raises(ValueError, match=r"outside \[-1, 3\)"):
        _groups([0, 1, bad, 2], [1, 2, 3])


def _plan(seg_m, seg_q, k, cus, budget):
    from cphnsw_mi355x import _lib
    m = np.ascontiguousarray(seg_m, np.uint64)
    q = np.ascontiguousarray(seg_q, np.uint64)
    out = (C.c_uint64 * 6)()
    _lib.check(_lib.lib().cph_host_exact_group_plan(m.ctypes.data, q.ctypes.data, len(m), k, cus, budget, None, 0, out))
    n_items = int(out[0])
    items = np.full((max(n_items, 1), 8), 0xDEADBEEF, np.uint32)
    out2 = (C.c_uint64 * 6)()
    _lib.check(_lib.lib().cph_host_exact_group_plan(m.ctypes.data, q.ctypes.data, len(m), k, cus, budget, items.ctypes.data,
                                                    n_items, out2))
    assert list(out) == list(out2)
    return items[:n_items].astype(np.int64), [int(x) for x in out]


def _check_plan(seg_m, seg_q, k, cus, budget):
    items, (n_items, launches, gq, cap, pool_bytes, _) = _plan(seg_m, seg_q, k, cus, budget)
    kp = 64
    while kp < k:
        kp *= 2
    assert cap == 2 * kp and gq % 8 == 0
    seg, part, c_lo, c_hi, q_lo, q_cnt, pool, launch = items.T
    assert (np.diff(launch) >= 0).all() and (launches == 0 or launch.max() == launches - 1)
    worst = 0
    for s, (m, nq) in enumerate(zip(seg_m, seg_q)):
        mine = items[seg == s]
        if m == 0 or nq == 0:
            assert len(mine) == 0
            continue
        # every (candidate, query) pair exactly once
        cover = np.zeros((m, nq), np.uint8) if m * nq <= 1 << 24 else None
        groups = sorted(set(zip(mine[:, 4], mine[:, 5])))
        assert [g[0] for g in groups] == list(range(0, nq, gq))             # the queries: cut into groups once
        assert sum(g[1] for g in groups) == nq and all(0 < g[1] <= gq for g in groups)
        for g_lo, g_cnt in groups:
            parts = mine[(mine[:, 4] == g_lo)]
            parts = parts[np.argsort(parts[:, 1])]
            assert list(parts[:, 1]) == list(range(len(parts))) and len(parts) <= 256
            assert parts[0, 2] == 0 and parts[-1, 3] == m                  # the candidates: contiguous parts, all of them
            assert (parts[1:, 2] == parts[:-1, 3]).all() and (parts[:, 3] > parts[:, 2]).all()
            assert (parts[:, 2] % 64 == 0).all()
            assert len(set(parts[:, 7])) == 1                              # a group's parts share a launch (one merge)
            # the pools of the unit: part p, query i at pool + i -- disjoint, stride = the group's size
            assert (parts[:, 6] == parts[0, 6] + np.arange(len(parts)) * g_cnt).all()
            if cover is not None:
                for p in parts:
                    cover[p[2]:p[3], g_lo:g_lo + g_cnt] += 1
        if cover is not None:
            assert (cover == 1).all(), s
    for l in range(launches):                          # pools of a launch: disjoint, within the budget
        mine = items[launch == l]
        spans = sorted((int(p), int(p + c)) for p, c in zip(mine[:, 6], mine[:, 5]))
        assert spans[0][0] == 0
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        worst = max(worst, spans[-1][1] * cap * 8)
    assert worst == pool_bytes
    return items, launches, pool_bytes


@pytest.mark.parametrize("k", [1, 10, 100, 1024])
def test_group_plan_covers_every_pair_once_within_budget(k):
    rng = np.random.default_rng(k)
    shapes = [
        ([3000], [1]), ([1], [1]), ([64], [128]), ([65], [129]),
        ([100000], [1000]),                                    # one segment: parts and groups
        ([977] * 64, [int(x) for x in rng.integers(1, 40, 64)]),   # many small tenants
        ([0, 500, 70000, 1], [10, 0, 300, 5]),                 # empty segments get no item
        ([int(x) for x in rng.integers(1, 20000, 30)], [int(x) for x in rng.integers(1, 400, 30)]),
    ]
    for seg_m, seg_q in shapes:
        for cus in (1, 256):
            budget = 1 << 30
            items, launches, pool_bytes = _check_plan(seg_m, seg_q, k, cus, budget)
            assert pool_bytes <= budget
            assert launches <= 1 or k == 1024


def test_group_plan_small_budget_cuts_launches_and_parts():
    k, cap = 10, 128
    seg_m, seg_q = [50000, 3000, 20000], [1000, 300, 129]
    one_group = 128 * cap * 8                                  # the pools of one part of one full query group
    for budget in (one_group, 3 * one_group, 40 * one_group):
        items, launches, pool_bytes = _check_plan(seg_m, seg_q, k, 256, budget)
        assert pool_bytes <= budget and launches > 1
    # the work allows it: about two waves per SIMD over all segments
    items, launches, _ = _check_plan([1000000], [128], 10, 256, 1 << 30)
    assert launches == 1 and 250 <= len(items) <= 256          # (capped by the parts a merge folds)
    items, launches, _ = _check_plan([100000] * 8, [128] * 8, 10, 256, 1 << 30)
    assert 1024 <= len(items) <= 2048 + 8


def test_group_plan_argument_checks():
    from cphnsw_mi355x import _lib
    out = (C.c_uint64 * 6)()
    one = np.ones(1, np.uint64)
    for k in (0, 1025):
        rc = _lib.lib().cph_host_exact_group_plan(one.ctypes.data, one.ctypes.data, 1, k, 256, 1 << 30, None, 0, out)
        assert rc == _lib.INVALID_ARGUMENT
    assert _lib.lib().cph_host_exact_group_plan(one.ctypes.data, one.ctypes.data, 1, 10, 256, 1 << 30, None, 0, None) == _lib.INVALID_ARGUMENT
