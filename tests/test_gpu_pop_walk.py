"""The path walk of `heap_pop_wave` (csrc/device_search.h) against libstdc++, operation by operation.

A pop of a beam of up to 255 entries walks the root-to-leaf path on two ballot masks: six unconditional scalar steps,
the depth from the level count of the heap (L or L + 1), and a seventh step from the second mask once the heap holds
more than 130 entries.  From 256 entries on the hybrid routine takes over.  `heap_ops_debug` runs an operation list on
one wave and returns the heap array at its end; `oracle.std_heap_ops` replays the list with std::push_heap /
std::pop_heap.  Each list is run once per prefix, so heap positions and ids are compared after EVERY operation.  Keys
come from eight distinct values: equal keys are everywhere, and only the exact element movement decides where they sit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# where the walk changes: one level / two; six steps exactly (63..65 internal-node boundary of a 127 / 128 / 131-entry
# heap); the second mask (131 / 132 up); the last LDS size and the first hybrid pop (255 / 256)
SIZES = [3, 4, 63, 64, 65, 127, 128, 131, 132, 255, 256]
N_MAX = 300
DISTINCT = 8


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


@pytest.fixture(scope="module")
def pushed():
    """One list of (key, id) shared by every test: the heap after n pushes is the same heap in all of them."""
    rng = np.random.default_rng(20261019)
    keys = rng.integers(0, DISTINCT, size=4 * N_MAX).astype(np.float32)
    ids = np.arange(len(keys), dtype=np.uint32)
    return keys, ids


def _same(cph, oracle, ops, pushed, what):
    keys, ids = pushed
    ops = np.asarray(ops, np.uint8)
    n_push = int((ops != 0).sum())
    gk, gi = cph.heap_ops_debug(ops, keys[:n_push], ids[:n_push])
    wk, wi = oracle.std_heap_ops(ops, keys[:n_push], ids[:n_push])
    assert len(gi) == len(wi), (what, len(gi), len(wi))
    assert np.array_equal(gi, wi), (what, np.flatnonzero(gi != wi)[:8].tolist())
    assert gk.tobytes() == wk.tobytes(), what


def test_fill_to_every_size_then_one_pop(cph, oracle, pushed):
    """n pushes for every n in 1..300 (the state after every push of the longest fill), and one pop of each of those
    heaps: a pop at every size at which either LDS walk or the first hybrid pops run."""
    for n in range(1, N_MAX + 1):
        fill = np.ones(n, np.uint8)
        _same(cph, oracle, fill, pushed, ("fill", n))
        _same(cph, oracle, np.concatenate([fill, np.zeros(1, np.uint8)]), pushed, ("fill+pop", n))


@pytest.mark.parametrize("n", SIZES + [N_MAX])
def test_pop_to_empty(cph, oracle, pushed, n):
    """n pushes, then n pops, compared after every pop (the last prefix leaves the empty heap)."""
    ops = np.concatenate([np.ones(n, np.uint8), np.zeros(n, np.uint8)])
    for p in range(n + 1, 2 * n + 1):
        _same(cph, oracle, ops[:p], pushed, ("drain", n, p - n))


@pytest.mark.parametrize("n", SIZES)
def test_pushes_and_pops_interleaved(cph, oracle, pushed, n):
    """From n entries on: 80 operations -- pop, push, and pop-then-push the way one expansion does it -- that keep the
    size around n, compared after every one of them."""
    rng = np.random.default_rng(n)
    mix = rng.choice(np.array([0, 0, 1, 1, 2, 2, 2], np.uint8), size=80)
    ops = np.concatenate([np.ones(n, np.uint8), mix])
    for p in range(n + 1, len(ops) + 1):
        _same(cph, oracle, ops[:p], pushed, ("mix", n, p - n))
