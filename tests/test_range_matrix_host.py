"""Host statements of the matrix range search (device_range_mfma.h): the limit a query's approximate distances are compared
with, in exact rationals, and the scratch budget rule at its edge."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

FLT_MAX = float(np.finfo(np.float32).max)
TINY = float(np.finfo(np.float32).tiny)


def _limit(radius, eps):
    from cphnsw_mi355x import _lib
    out = C.c_float()
    _lib.check(_lib.lib().cph_host_range_matrix_limit(float(radius), float(eps), C.byref(out)))
    return out.value


def _fits(survivors, any_long, budget):
    from cphnsw_mi355x import _lib
    out = C.c_int(-1)
    _lib.check(_lib.lib().cph_host_range_matrix_fits(survivors, int(any_long), budget, C.byref(out)))
    return bool(out.value)


def _pairs():
    rng = np.random.default_rng(4)
    r = np.exp(rng.uniform(np.log(TINY) - 10, np.log(FLT_MAX), 4000)).astype(np.float32)
    e = np.exp(rng.uniform(np.log(TINY), np.log(FLT_MAX), 4000)).astype(np.float32)
    special = [2.0 ** -149, TINY, np.nextafter(np.float32(TINY), np.float32(1)), 1.0, np.nextafter(np.float32(1), np.float32(2)),
               3.0, 2.0 ** 24 + 2, FLT_MAX / 2, FLT_MAX]
    return list(zip(r.tolist(), e.tolist())) + [(float(a), float(b)) for a in special for b in special + [0.0]]


def test_limit_is_at_least_radius_plus_eps():
    for radius, eps in _pairs():
        lim = _limit(radius, eps)
        if math.isinf(lim):
            assert lim > 0
            continue
        assert Fraction(lim) >= Fraction(radius) + Fraction(eps), (radius, eps, lim)


@pytest.mark.parametrize("eps", (0.0, 1.0, float("inf"), float("nan")))
def test_radii_that_admit_nothing(eps):
    for radius in (float("nan"), 0.0, -0.0, -1.0, float("-inf")):
        assert _limit(radius, eps) == -1.0, (radius, eps)


def test_slack_that_is_not_finite_and_infinite_radius():
    for radius in (1e-30, 1.0, FLT_MAX, float("inf")):
        for eps in (float("inf"), float("-inf"), float("nan")):
            assert math.isnan(_limit(radius, eps)), (radius, eps)
    for eps in (0.0, 1.0, FLT_MAX):
        assert _limit(float("inf"), eps) == float("inf")


@pytest.mark.parametrize("any_long,per", ((False, 12), (True, 20)))
def test_budget_rule_at_its_edge(any_long, per):
    for keys in (1, 1000, (1 << 30) // per):
        assert _fits(keys, any_long, keys * per) and _fits(keys - 1, any_long, keys * per)
        assert not _fits(keys + 1, any_long, keys * per) and not _fits(keys, any_long, keys * per - 1)
    assert _fits(0, any_long, 0)
