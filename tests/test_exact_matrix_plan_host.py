"""cph_host_exact_matrix_plan: the cut of a batch under the matrix engine of the exact scan (plan_exact_matrix,
csrc/device_exact_mfma.h) -- launches of tile_q queries, each a grid of P parts of `part` candidates x tiles of 128 queries,
pools of C keys.  The properties every cut must have, over the sizes at which the planner takes another branch, and the
two geometries tests/test_gpu_exact_matrix_tiles.py is written for."""
import ctypes as C
import itertools

import pytest

NAMES = ("Kp", "C", "tile_q", "P", "part", "pool_keys")


def _plan(m, nq, k, cus, budget):
    from cphnsw_mi355x import _lib
    out = (C.c_uint64 * 6)()
    _lib.check(_lib.lib().cph_host_exact_matrix_plan(m, nq, k, cus, budget, out))
    return dict(zip(NAMES, (int(x) for x in out)))


@pytest.mark.parametrize("budget", [1 << 20, 1 << 30])
@pytest.mark.parametrize("cus", [1, 256])
def test_every_cut_covers_the_batch_within_the_budget(cus, budget):
    for m, nq, k in itertools.product((1, 127, 128, 129, 2597, 100000, 2 ** 32 - 1), (1, 24, 128, 129, 400, 10000),
                                      (1, 64, 65, 1024)):
        pl = _plan(m, nq, k, cus, budget)
        what = (m, nq, k, cus, budget, pl)
        kp = 64
        while kp < max(k, 64):
            kp *= 2
        assert pl["Kp"] == kp and pl["C"] == 2 * kp, what
        assert pl["part"] % 128 == 0 and pl["part"] > 0, what
        assert pl["P"] == -(-m // pl["part"]) and 1 <= pl["P"] <= 256, what      # the parts cover the candidates, none is empty
        assert pl["tile_q"] == nq or (pl["tile_q"] % 128 == 0 and 0 < pl["tile_q"] < nq), what
        assert pl["pool_keys"] == pl["P"] * pl["tile_q"] * pl["C"], what
        # over the budget only at the floor: one part, one tile of queries per launch
        assert pl["pool_keys"] * 8 <= budget or (pl["P"] == 1 and pl["tile_q"] <= 128), what


def test_the_geometries_of_the_tile_tests():
    """At 256 CUs and a budget of 1 MiB 2,597 candidates are cut into parts of three and of six candidate tiles, the last
    part ragged."""
    a = _plan(2597, 128, 10, 256, 1 << 20)
    assert (a["P"], a["part"], a["tile_q"], a["C"]) == (7, 384, 128, 128)
    b = _plan(2597, 400, 100, 256, 1 << 20)
    assert (b["P"], b["part"], b["tile_q"], b["C"]) == (4, 768, 128, 256)
    # the default budget: one candidate tile per part, what every fixture of 400 rows or fewer runs with
    c = _plan(400, 24, 10, 256, 1 << 30)
    assert (c["P"], c["part"], c["tile_q"]) == (4, 128, 24)


def test_argument_checks_are_those_of_the_vector_plan():
    from cphnsw_mi355x import _lib
    for m, nq, k in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1025), (2 ** 32, 1, 1), (1, 2 ** 32, 1)):
        with pytest.raises(ValueError):
            _plan(m, nq, k, 256, 1 << 30)
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().cph_host_exact_plan(m, nq, k, 256, 1 << 30, (C.c_uint64 * 6)()))
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().cph_host_exact_matrix_plan(1, 1, 1, 256, 1 << 30, None))
