"""The host side of the exhaustive rescored search (csrc/host_rescore_all.h), no GPU: the plan through
cph_host_plan_rescore_all, and the new entries on null handles."""
import ctypes as C

import pytest

from cphnsw_mi355x import _lib

INVALID_ARGUMENT = 1


def plan(size, n, k, cus, budget):
    out = (C.c_uint64 * 5)()
    _lib.check(_lib.lib().cph_host_plan_rescore_all(size, n, k, cus, budget, out))
    return dict(zip(("P", "part", "tile_q", "C", "bytes"), out))


@pytest.mark.parametrize("size,n,k,cus,budget", ((1_000_000, 16, 10, 256, 1 << 30), (1_000_000, 1000, 10, 256, 1 << 30),
                                                 (400, 1, 1, 256, 1 << 30), (1100, 130, 1024, 256, 1 << 30),
                                                 (1_000_000, 5000, 1024, 256, 64 << 20), (100_000, 300, 100, 1, 1 << 30)))
def test_plan(size, n, k, cus, budget):
    p = plan(size, n, k, cus, budget)
    assert p["part"] % 128 == 0 and p["P"] * p["part"] >= size > (p["P"] - 1) * p["part"]
    assert p["C"] >= 256 and p["C"] - 128 >= k and p["C"] & (p["C"] - 1) == 0
    assert p["bytes"] == p["P"] * p["tile_q"] * p["C"] * 8 <= budget
    assert p["tile_q"] == n or (p["tile_q"] % 128 == 0 and p["tile_q"] < n)
    tiles = -(-p["tile_q"] // 128)
    assert p["P"] <= 256 and p["P"] * tiles <= max(cus, tiles) + tiles          # about one workgroup per CU
    if cus == 1:
        assert p["P"] == 1
    if budget == 64 << 20:
        assert p["tile_q"] < n                                                  # a small budget tiles the batch


def test_plan_refuses_k_out_of_range():
    out = (C.c_uint64 * 5)()
    assert _lib.lib().cph_host_plan_rescore_all(1000, 10, 1025, 256, 1 << 30, out) == INVALID_ARGUMENT
    assert _lib.lib().cph_host_plan_rescore_all(1000, 10, 0, 256, 1 << 30, out) == INVALID_ARGUMENT


def test_null_handles():
    L = _lib.lib()
    assert L.cph_version() >= 121
    us = C.c_double()
    assert L.cph_search_rescored_all(None, None, 1, None, 16, 10, None, None, 0, None, 0, None, None, None) == INVALID_ARGUMENT
    assert L.cph_search_rescored_all_device(None, None, 1, None, 16, 10, None, None, 0, None, 0, None, None, None, None) == INVALID_ARGUMENT
    assert L.cph_multi_search_rescored_all(None, None, 1, None, 16, 10, None, None, 0, None, 0, None, None, None) == INVALID_ARGUMENT
    assert L.cph_rescore_all_hook(None, None, 1, None, None, 10, 0, None, None, None) == INVALID_ARGUMENT
    assert L.cph_debug_time_rescored_all(None, 1) == INVALID_ARGUMENT
    assert L.cph_debug_last_rescored_all_us(None, C.byref(us)) == INVALID_ARGUMENT
