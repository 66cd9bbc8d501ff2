"""cph_host_exact_matrix_groups_plan (plan_exact_matrix_groups, device_exact_mfma_groups.h): every (segment, query tile,
candidate) belongs to exactly one item; parts are whole 128-candidate tiles, at most 256 per segment; every launch's scratch
is within the budget unless one unit of one part alone exceeds it; the pool indices of a launch are disjoint."""
import ctypes as C

import numpy as np
import pytest


def _plan(seg_m, seg_q, k, cus, budget):
    from cphnsw_mi355x import _lib
    m, q = np.ascontiguousarray(seg_m, np.uint64), np.ascontiguousarray(seg_q, np.uint64)
    out = (C.c_uint64 * 6)()
    _lib.check(_lib.lib().cph_host_exact_matrix_groups_plan(m.ctypes.data, q.ctypes.data, len(m), k, cus, budget, None, 0, out))
    items = np.full((int(out[0]), 8), 0xDEADBEEF, np.uint32)
    _lib.check(_lib.lib().cph_host_exact_matrix_groups_plan(m.ctypes.data, q.ctypes.data, len(m), k, cus, budget, items.ctypes.data,
                                                            len(items), out))
    return items.astype(np.int64), [int(x) for x in out]


ROWS = [
    # seg_m, seg_q, k, CUs, budget
    ([400, 267, 1], [128, 129, 300], 10, 256, 1 << 30),
    ([(1 << 32) - 128], [129], 10, 256, 1 << 30),           # the longest list the engine takes: 64-bit part arithmetic
    ([(1 << 32) - 128, 5], [1000, 128], 100, 8, 1 << 30),
    ([1], [129], 1, 256, 1 << 30),                          # a single candidate
    ([0, 100000, 977], [128, 0, 640], 10, 256, 1 << 30),    # segments the caller zeroed get no item
    ([100000] * 8, [1250] * 8, 10, 256, 1 << 30),
    ([50000, 3000, 20000], [1000, 300, 129], 10, 256, 1 << 20),   # several parts per segment AND several launches
    ([50000, 3000], [1000, 300], 1024, 256, 1 << 20),       # one part of one tile exceeds the budget: a launch per unit
]


@pytest.mark.parametrize("seg_m,seg_q,k,cus,budget", ROWS)
def test_matrix_groups_plan(seg_m, seg_q, k, cus, budget):
    items, (n_items, launches, tile, cap, max_bytes, max_parts) = _plan(seg_m, seg_q, k, cus, budget)
    kp = 64
    while kp < k:
        kp *= 2
    assert tile == 128 and cap == 2 * kp and n_items == len(items)
    seg, part, c_lo, c_hi, q_lo, q_cnt, pool, launch = items.T
    assert (np.diff(launch) >= 0).all() and launch.max() == launches - 1
    seen_parts = 0
    for s, (m, nq) in enumerate(zip(seg_m, seg_q)):
        mine = items[seg == s]
        if m == 0 or nq == 0:
            assert len(mine) == 0
            continue
        tiles = sorted(set(zip(mine[:, 4].tolist(), mine[:, 5].tolist())))
        assert [t[0] for t in tiles] == list(range(0, nq, 128))                 # the queries: cut into tiles once
        assert [t[1] for t in tiles] == [min(128, nq - t[0]) for t in tiles]
        for t_lo, t_cnt in tiles:
            parts = mine[mine[:, 4] == t_lo]
            assert parts[:, 1].tolist() == list(range(len(parts))) and len(parts) <= 256
            seen_parts = max(seen_parts, len(parts))
            # the candidates: contiguous parts of whole 128-candidate tiles, all of them, none empty
            assert parts[0, 2] == 0 and parts[-1, 3] == m and (parts[1:, 2] == parts[:-1, 3]).all()
            assert (parts[:, 3] > parts[:, 2]).all() and (parts[:, 2] % 128 == 0).all()
            assert len(set(parts[:, 7].tolist())) == 1                          # a unit's parts share a launch (one certify)
            assert (parts[:, 6] == parts[0, 6] + np.arange(len(parts)) * t_cnt).all()
    assert seen_parts == max_parts
    worst = 0
    for l in range(launches):                                                   # pools of a launch: disjoint, within the budget
        mine = items[launch == l]
        spans = sorted((int(p), int(p + c)) for p, c in zip(mine[:, 6], mine[:, 5]))
        assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
        rows = int(mine[mine[:, 1] == 0][:, 5].sum())
        scratch = (spans[-1][1] + rows) * (cap * 8 + 4)
        units = len(set(zip(mine[:, 0].tolist(), mine[:, 4].tolist())))
        assert scratch <= budget or (units == 1 and mine[:, 1].max() == 0), (l, scratch)
        worst = max(worst, scratch)
    assert worst == max_bytes
    if budget == 1 << 20 and k == 10:
        assert launches > 1 and max_parts > 1
    if budget == 1 << 30:
        assert launches == 1

