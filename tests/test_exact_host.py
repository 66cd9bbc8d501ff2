"""CPU tier of the exact search: cph_host_filter_ids, the host statement of the bitmap -> ascending id list compaction
the exact scan runs on a filter (filter_ids_kernel), against np.flatnonzero; and cph_host_exact_plan, the cut of an
exact batch into candidate parts, query groups and launches."""
import ctypes as C

import numpy as np
import pytest


def _ids(words, n_bits, room):
    from cphnsw_mi355x import _lib
    out = np.full(max(room, 1), 0xDEADBEEF, np.uint32)
    cnt = C.c_uint64(123)
    w = np.ascontiguousarray(words, np.uint32)
    _lib.check(_lib.lib().cph_host_filter_ids(w.ctypes.data if w.size else None, n_bits, out.ctypes.data, C.byref(cnt)))
    assert (out[cnt.value:] == 0xDEADBEEF).all()          # nothing written behind the list
    return out[:cnt.value]


def _pack(mask):
    from cphnsw_mi355x.index import pack_allowed_bits
    return pack_allowed_bits(mask)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 1000, 70001])
def test_filter_ids_equals_flatnonzero(n):
    rng = np.random.default_rng(n)
    single = np.zeros(n, bool)
    single[n // 2] = True
    last = np.zeros(n, bool)
    last[n - 1] = True
    masks = {"empty": np.zeros(n, bool), "full": np.ones(n, bool), "single": single, "last": last,
             "p0.5": rng.random(n) < 0.5, "p0.01": rng.random(n) < 0.01}
    for name, m in masks.items():
        got = _ids(_pack(m), n, int(m.sum()))
        assert np.array_equal(got, np.flatnonzero(m).astype(np.uint32)), (n, name)


@pytest.mark.parametrize("n", [1, 31, 33, 70001])
def test_stray_bits_behind_n_bits_are_ignored(n):
    rng = np.random.default_rng(1000 + n)
    m = rng.random(n) < 0.3
    w = _pack(m).copy()
    assert n % 32 != 0
    w[-1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)        # every bit behind the last id set
    assert np.array_equal(_ids(w, n, int(m.sum())), np.flatnonzero(m).astype(np.uint32))
    # ... and a bitmap that is all ones, stray bits included, lists exactly 0..n-1
    assert np.array_equal(_ids(np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32), n, n), np.arange(n, dtype=np.uint32))


def test_no_bits_at_all():
    assert len(_ids(np.zeros(0, np.uint32), 0, 0)) == 0


def _plan(m, nq, k, cus, budget):
    from cphnsw_mi355x import _lib
    out = (C.c_uint64 * 6)()
    _lib.check(_lib.lib().cph_host_exact_plan(m, nq, k, cus, budget, out))
    return [int(x) for x in out]


@pytest.mark.parametrize("budget", [1 << 20, 8 << 20, 1 << 30])
@pytest.mark.parametrize("k", [1, 10, 550, 1024])
@pytest.mark.parametrize("m,nq", [(1, 1), (63, 7), (700, 200), (7000, 200), (70000, 24), (100000, 10000), (1000000, 10000)])
def test_exact_plan_covers_the_batch_within_the_budget(m, nq, k, budget):
    P, part, gq, tile_q, C_, pool_bytes = _plan(m, nq, k, 256, budget)
    kp = 64
    while kp < k:
        kp *= 2
    assert C_ == 2 * kp and C_ >= k + 64                       # a pool takes 64 appends on top of k kept keys
    assert part % 64 == 0 and (P - 1) * part < m <= P * part    # the parts cover the candidates, none is empty
    assert 1 <= P <= 256 and gq % 8 == 0
    assert tile_q == nq or (tile_q < nq and tile_q % gq == 0)   # launches of whole groups
    assert pool_bytes == P * tile_q * C_ * 8
    # over the budget only at the floor: one part, one group of queries per launch
    assert pool_bytes <= budget or (P == 1 and tile_q <= gq)


def test_exact_plan_tiles_and_cuts_parts_under_a_small_budget():
    # 7,000 candidates, 200 queries, k = 550 (pools of 2,048 keys): 1 GiB holds one launch of 110 parts, 8 MiB holds 4 parts
    # of 128 queries
    assert _plan(7000, 200, 550, 256, 1 << 30)[:4] == [110, 64, 128, 200]
    assert _plan(7000, 200, 550, 256, 8 << 20)[:4] == [4, 1792, 128, 128]
    # many queries fill the GPU on their own: few parts
    assert _plan(100000, 10000, 10, 256, 1 << 30)[0] == 26
    with pytest.raises(ValueError):
        _plan(7000, 200, 1025, 256, 1 << 30)
