"""The exhaustive MaxSim pass on the host: the ABI carries its symbols, and the term of its bound (csrc/host_maxsim_all.h,
cph_host_maxsim_all_term) never exceeds the real difference.

A distance is >= +0, so the term is clamped there: the statement checked is term <= max(m - eps, 0) in exact rationals, which
is `term <= m - eps` wherever that difference is not negative."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from cphnsw_mi355x import _lib

NEW = ("cph_search_maxsim_all", "cph_search_maxsim_all_device", "cph_multi_search_maxsim_all", "cph_maxsim_all_hook",
       "cph_host_maxsim_all_term")
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "cphnsw_mi355x.h")
FLT_MIN, FLT_MAX = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
MS = (0.0, 1e-42, 1.0, 1.0 + 2.0 ** -23, 255.99998, FLT_MAX / 2)
EPS = (0.0, FLT_MIN, 1e-3, 0.25)


def test_abi_has_the_symbols():
    with open(HEADER) as f:
        text = f.read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text) and name in _lib.SYMBOLS and hasattr(_lib.lib(), name), name
    assert _lib.lib().cph_version() >= 120


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("m", MS)
def test_term_is_below_the_real_difference(m, eps):
    m, eps = float(np.float32(m)), float(np.float32(eps))
    out = C.c_float()
    _lib.check(_lib.lib().cph_host_maxsim_all_term(m, eps, C.byref(out)))
    term = out.value
    assert term == term and term >= 0.0 and not np.signbit(np.float32(term))
    assert Fraction(term) <= max(Fraction(m) - Fraction(eps), Fraction(0))
    if m - eps > 1e-30:                       # and not uselessly far below: two roundings and the factor 1 - 2^-22
        assert Fraction(term) >= (Fraction(m) - Fraction(eps)) * (1 - Fraction(6, 2 ** 24))
