"""CPU checks of the models the builder's GPU tests compare against (tests/layer_model.py, tests/block_layout.py): the
reverse lists against a double loop, the hub cut against the uncut list where the cut removes nothing, its independence
of the reverse list's order, and the vectorised block reader against the loop it replaces."""
import numpy as np
import pytest

import block_layout
import layer_model
from layer_model import INVALID


def _table(rng, n, width=32, holes=0.2):
    """[n][32]: per row up to `width` distinct ids (self allowed), some slots empty."""
    knn = np.full((n, 32), INVALID, np.uint32)
    for u in range(n):
        m = min(width, n)
        row = rng.choice(n, m, replace=False).astype(np.uint32)
        row[rng.random(m) < holes] = INVALID
        knn[u, :m] = row
    return knn


@pytest.mark.parametrize("n", [1, 2, 7, 33, 60])
def test_reverse_lists_against_a_double_loop(n):
    rng = np.random.default_rng(n)
    for knn in (_table(rng, n), _table(rng, n, holes=0.0), np.full((n, 32), INVALID, np.uint32)):
        got = layer_model.reverse_lists(knn, n)
        assert len(got) == n
        for v in range(n):
            want = [u for u in range(n) for j in range(32) if knn[u, j] == v]
            assert got[v].dtype == np.uint32 and got[v].tolist() == want, (n, v)


def _clustered(rng, n, D, rounded):
    cent = rng.normal(0, 4, (6, D))
    x = (cent[rng.integers(0, 6, n)] + rng.normal(0, 1, (n, D))).astype(np.float32)
    return np.round(x) if rounded else x


@pytest.mark.parametrize("uniq,seed", [(10, 1), (40, 2), (63, 3)])
def test_hub_cut_that_removes_nothing_selects_what_the_uncut_list_selects(oracle, uniq, seed):
    """97 reverse ids take the hub branch; with fewer than 64 unique valid candidates the cut keeps all of them, so
    the rule must select exactly what it selects from the plain concatenation."""
    rng = np.random.default_rng(seed)
    n, D, v = 300, 16, 17
    x = _clustered(rng, n, D, seed % 2 == 0)
    pool = rng.choice(np.setdiff1d(np.arange(n), [v]), uniq, replace=False).astype(np.uint32)
    fwd = np.full(32, INVALID, np.uint32)
    fwd[:min(8, uniq)] = pool[:min(8, uniq)]
    rev = pool[rng.integers(0, uniq, 97)]
    rev[:uniq] = pool                                   # every id of the pool at least once
    rev[96] = v                                         # the vertex itself: dropped by the cut and by the rule
    cut = layer_model.candidates(oracle, x, v, fwd, rev)
    assert len(cut) == uniq < layer_model.HUB_KEEP and v not in cut
    for R in (32, 8):
        a = oracle.select_neighbors(x, v, cut, R, 1.2, 0.5, 0.0, None)
        b = oracle.select_neighbors(x, v, np.concatenate([fwd, rev]), R, 1.2, 0.5, 0.0, None)
        assert np.array_equal(a, b)


def test_candidates_below_the_branch_are_the_concatenation(oracle):
    rng = np.random.default_rng(5)
    x = _clustered(rng, 200, 16, False)
    fwd = rng.choice(200, 32, replace=False).astype(np.uint32)
    for m in (0, 1, 96):
        rev = rng.choice(200, m, replace=False).astype(np.uint32)
        assert np.array_equal(layer_model.candidates(oracle, x, 3, fwd, rev), np.concatenate([fwd, rev]))


@pytest.mark.parametrize("n_rev,seed", [(97, 1), (200, 2), (500, 4)])
def test_hub_cut_is_invariant_under_permutations_of_rev(oracle, n_rev, seed):
    rng = np.random.default_rng(seed)
    n, D, v = 600, 16, 5
    x = _clustered(rng, n, D, seed % 2 == 0)            # even seeds: equal distances at the cut
    fwd = rng.choice(n, 32, replace=False).astype(np.uint32)
    fwd[[3, 9]] = INVALID
    rev = rng.choice(n, n_rev, replace=False).astype(np.uint32)
    rev[:4] = fwd[fwd != INVALID][:4]
    want = layer_model.candidates(oracle, x, v, fwd, rev)
    assert len(want) == layer_model.HUB_KEEP and len(set(want.tolist())) == 64 and v not in want
    d = np.array([oracle.l2(x[v], x[c]) for c in want])
    assert np.all((d[:-1] < d[1:]) | ((d[:-1] == d[1:]) & (want[:-1] < want[1:])))
    rest = np.setdiff1d(np.concatenate([fwd[fwd != INVALID], rev]), np.concatenate([want, [v]]))
    assert all((oracle.l2(x[v], x[c]), c) > (d[-1], want[-1]) for c in rest)      # nothing nearer was cut
    for p in range(4):
        assert np.array_equal(layer_model.candidates(oracle, x, v, fwd, rng.permutation(rev)), want)
    assert np.array_equal(layer_model.candidates(oracle, x, v, fwd, rev[::-1]), want)


def test_select_layer_is_the_rule_on_every_row(oracle):
    rng = np.random.default_rng(9)
    n, D = 150, 16
    x = _clustered(rng, n, D, True)
    knn = _table(rng, n, holes=0.1)
    knn[:120, 0] = 7                                     # vertex 7: a hub
    ids, cnt = layer_model.select_layer(oracle, x, knn, 18, 1.2, 0.5, 0.0, None)
    rev = layer_model.reverse_lists(knn, n)
    assert len(rev[7]) > layer_model.HUB_REV
    for v in range(n):
        want = oracle.select_neighbors(x, v, layer_model.candidates(oracle, x, v, knn[v], rev[v]), 18, 1.2, 0.5, 0.0, None)
        assert cnt[v] == len(want) and np.array_equal(ids[v, :cnt[v]], want) and (ids[v, cnt[v]:] == INVALID).all()


@pytest.mark.parametrize("D,bits", [(16, 2), (16, 4), (32, 1), (64, 4), (128, 1), (128, 4), (512, 1), (512, 4)])
def test_vectorised_block_reader_equals_the_loop(D, bits):
    rng = np.random.default_rng(D + bits)
    stride = block_layout._layout(D, bits)[5]
    dev = rng.integers(0, 256, stride, dtype=np.uint8)
    assert np.array_equal(block_layout.block_codes(dev, D, bits), block_layout._codes_from_planes(dev, D, bits))
    o = block_layout.codes_bytes(D, bits)
    aux, pops = block_layout.block_aux(dev, D, bits)
    raw = dev[o:o + 512].view(np.uint32).reshape(32, 4)
    assert aux.tobytes() == raw[:, :3].tobytes()
    assert np.array_equal(pops[:, 0] | (pops[:, 1] << np.uint32(16)), raw[:, 3])
    ids, count = block_layout.block_ids(dev, D, bits)
    assert ids.tobytes() == dev[o + 512:o + 640].tobytes() and count == int(dev[o + 640:o + 644].view(np.uint32)[0])
    assert o + 644 <= stride


def test_selection_hooks_validate_their_arguments():
    """Both construction hooks check their inputs before they touch a device: ids < n or kInvalidNode, D a power of two
    in 16..2048, R in 1..32, at most 65,536 reverse candidates."""
    import cphnsw_mi355x as cph
    x = np.zeros((40, 16), np.float32)
    knn = np.full((40, 32), INVALID, np.uint32)
    bad = knn.copy()
    bad[39, 31] = 40
    with pytest.raises(ValueError, match="out of range"):
        cph.select_layer_debug(x, bad, 32, 1.2, 0.5, device=0)
    with pytest.raises(ValueError, match="R must be"):
        cph.select_layer_debug(x, knn, 0, 1.2, 0.5, device=0)
    with pytest.raises(ValueError, match="R must be"):
        cph.select_layer_debug(x, knn, 33, 1.2, 0.5, device=0)
    with pytest.raises(ValueError, match="power of two"):
        cph.select_layer_debug(np.zeros((40, 24), np.float32), knn, 32, 1.2, 0.5, device=0)
    with pytest.raises(ValueError, match="knn must be"):
        cph.select_layer_debug(x, knn[:39], 32, 1.2, 0.5, device=0)
    fwd = np.full(32, INVALID, np.uint32)
    with pytest.raises(ValueError, match="n_rev <= 65536"):
        cph.select_neighbors_debug(x, 0, fwd, np.zeros(65537, np.uint32), 32, 1.2, 0.5, device=0)
    with pytest.raises(ValueError, match="out of range"):
        cph.select_neighbors_debug(x, 0, fwd, np.full(200, 40, np.uint32), 32, 1.2, 0.5, device=0)
