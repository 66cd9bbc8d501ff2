"""GPU tier of the exact-kNN kernels: knn_mfma_kernel (device_knn.h) and the symmetric self-join (device_knn_sym.h).

Every case of tests/knn_model.py runs through the debug entry knn_debug and must (i) equal the host statement
(csrc/host_knn.h, judged on the CPU by tests/test_knn_host.py) byte for byte in ids, distances and the number of fallback
rows, and (ii) pass the float64 checks with the derived bound on EVERY row.  The cases: tile edges in rows and columns, every
padded D, one K chunk per tile, forced compactions, ties by id, norms that dwarf the distances, sliced launches, q_ids, the
join at even and odd block counts with last blocks of 1 and 127 rows, its cap and queue overflows, a NaN row."""
import os
import subprocess
import sys

import numpy as np
import pytest

import knn_model as km

pytestmark = pytest.mark.gpu


def run(name, blocks=None):
    import cphnsw_mi355x
    c = km.case(name)
    return cphnsw_mi355x.knn_debug(c.X, c.Q, c.q_ids, c.path, c.blocks if blocks is None else blocks)


def agree(name):
    """One case: the kernels' bytes are the model's, and the float64 judge accepts them."""
    c = km.case(name)
    ids, dist, redo, made = run(name)
    km.check_case(name, ids, dist)
    want_ids, want_dist, want_redo, _ = km.model(name)
    bad = np.nonzero((ids != want_ids).any(1) | (dist.view(np.uint32) != want_dist.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, ("bytes", name, len(bad), int(bad[0]), ids[bad[0]].tolist(), want_ids[bad[0]].tolist(),
                           dist[bad[0]].tolist(), want_dist[bad[0]].tolist())
    assert redo == want_redo, ("fallback rows", name, redo, want_redo)
    if c.launches is not None:                   # sliced: the same bytes as one launch
        assert made == c.launches, (name, made)
        one = run(name, 0)
        assert one[3] == 1 and km.same_bytes(one[:2], (ids, dist)) and one[2] == redo
    return ids, dist


def test_two_pass_self_join_tile_edges():
    for nb in km.NB_EDGES:
        agree(f"self_nb{nb}")


@pytest.mark.parametrize("nq", km.NQ_EDGES)
def test_two_pass_queries_tile_edges(nq):
    for nb in km.NB_EDGES:
        agree(f"q{nq}_nb{nb}")


@pytest.mark.parametrize("dim", km.DIMS + (1536,))
def test_two_pass_every_padded_dimension(dim):
    agree(f"dim{dim}")


@pytest.mark.parametrize("tiles", (1, 2, 4))
def test_two_pass_one_chunk_per_tile(tiles):
    agree(f"one_chunk_{tiles}tiles")


@pytest.mark.parametrize("name", ("descending_d32", "descending_d128", "ascending_d32", "identical_queries", "identical_self",
                                  "scattered_copies", "three_copies"))
def test_two_pass_ordering_and_ties(name):
    agree(name)


def test_two_pass_large_norms():
    agree("large_norms")


def test_two_pass_sliced_launches():
    agree("sliced")


def test_two_pass_q_ids():
    ids, _ = agree("q_ids")
    c = km.case("q_ids")
    assert (ids != c.q_ids[:, None]).all()
    # without q_ids the same queries find themselves first
    import cphnsw_mi355x
    plain, d, _, _ = cphnsw_mi355x.knn_debug(c.X, c.Q)
    assert (plain[:, 0] == c.q_ids).all()


def test_production_entry_is_the_two_pass_path():
    """knn_bruteforce below the size limit and the debug entry with every knob at its default: the same bytes."""
    import cphnsw_mi355x
    for name in ("dim96", "one_chunk_4tiles", "join_1153_d128_ints"):
        c = km.case(name)
        got = cphnsw_mi355x.knn_bruteforce(c.X, c.Q)
        dbg = cphnsw_mi355x.knn_debug(c.X, c.Q)
        assert km.same_bytes(got, dbg[:2]) and dbg[2:] == (0, 1), name


@pytest.mark.parametrize("name", tuple(km.JOIN_PLAIN) + ("join_dups", "join_outlier", "join_sliced"))
def test_join(name):
    agree(name)


def test_join_through_the_environment_switch(tmp_path):
    """CPH_KNN_SYM=<n> lowers the size limit of the public entry (read once per process: a child)."""
    import cphnsw_mi355x
    name = "join_1409_d64_gauss"
    c = km.case(name)
    np.save(tmp_path / "x.npy", c.X)
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import cphnsw_mi355x; X = np.load(%r); "
            "i, d = cphnsw_mi355x.knn_bruteforce(X); np.save(%r, i); np.save(%r, d)"
            % (os.path.dirname(os.path.dirname(cphnsw_mi355x.__file__)), str(tmp_path / "x.npy"), str(tmp_path / "i.npy"), str(tmp_path / "d.npy")))
    subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, CPH_KNN_SYM="1024"), timeout=300)
    want = km.model(name)
    assert want[2] > 0                                      # (the join's answer differs from the two-pass one where it matters:
    two_pass = km.host_knn(c.X)                             # the distances are formed differently)
    assert not km.same_bytes(want[:2], two_pass[:2])
    assert km.same_bytes((np.load(tmp_path / "i.npy"), np.load(tmp_path / "d.npy")), want[:2])


@pytest.mark.parametrize("name", ("nan_queries", "nan_join"))
def test_one_nan_row(name):
    """A row that holds a NaN is never listed; as a row of a self-join its own list is all padding; every other list is the
    model's (and, by the float64 checks, what it would be without that row)."""
    agree(name)
