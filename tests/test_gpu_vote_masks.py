"""The search kernel's wave votes as mask algebra (csrc/device_search.h: ballot_and, lanes_below; the call sites in
csrc/device_search_expansion.inc under `kMaskVotes`) against the oracle: rows, distance bytes, per-query expansions
and the batch counters, on the small fixtures under tests/golden, each batch also once in reversed order.  The main
launch on explicit slots runs the two-loop instantiations that take the new forms (`<4,128,true>`, `<4,1024,true>`); the
default launch, the narrow codes and the filtered batches run the instantiations that keep the former text, through the
same source and its `if constexpr` arms.

The cases are chosen so that every rewritten vote is reached with some lanes off:
* `shortcount`: neighbour lists of 0, 5, 13, 29 and 31 entries (the instantiation without probe first; empty lists);
* k = 1, 2, 3, 10, 100: beams and result heaps crossing 1, 2, 3, 64 / 65 and 128 / 129 entries in LDS (the pop's second
  mask, the push's depth mask); the 2-bit fixtures: beams that spill (the append onto a spilled beam);
* k = 100 on 160 to 400 rows: result heaps that fill late or never (the warm-up arms);
* a filtered batch and a batch with per-query filters (the allowed-id votes), against the unfiltered rows they allow;
* D = 16 (generic), 128 and 1024 at 2 and 4 bits; the fixtures' first query is a stored row (distance below 1e-12);
* capacities small enough that both capacity tests fire (the re-run answers), and that the id log fills and the bitmap
  is wiped, then the same handle again.
"""
import numpy as np
import pytest

from golden_util import DATASETS, fixture_path, golden

pytestmark = pytest.mark.gpu

# (fixture, bits, variant)
CASES = [("g128", 4, "plain"), ("g128", 4, "shortcount"), ("g128", 2, "plain"), ("g128", 2, "shortcount"),
         ("g16", 4, "plain"), ("g16", 2, "shortcount"), ("g1024", 2, "plain"), ("g1024", 2, "shortcount"),
         ("sift96", 4, "gamma")]
KS = (1, 2, 3, 10, 100)


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


_WANT = {}


def want_for(oracle, path, Q, k):
    """The oracle's answer of one (index file, k): computed once, shared, never modified."""
    key = (path, k, len(Q))
    if key not in _WANT:
        _WANT[key] = oracle.load(path).search_batch(Q, k, nthreads=16, counters=True)
    return _WANT[key]


def _check(ix, Q, k, want, where, reruns=None):
    oids, od, _, ctr = want
    ids, d = ix.search_batch(Q, k)
    st = ix.last_search_stats()
    work = ix.last_query_expansions(len(Q)).astype(np.uint64)
    print(where, st)
    assert np.array_equal(ids, oids), (where, int((ids != oids).any(axis=1).sum()))
    assert _beq(d, od), where
    assert np.array_equal(work, ctr[:, 0]), (where, int((work != ctr[:, 0]).sum()))
    if reruns is True:
        assert st["rerun_queries"] > 0, (where, st)
    elif reruns is False:
        assert st["rerun_queries"] == st["stage2_reruns"], (where, st)
    if st["rerun_queries"] == 0:
        assert st["expansions"] == int(ctr[:, 0].sum()), (where, st)
        assert st["new_neighbours"] == int(ctr[:, 3].sum()), (where, st)
        assert st["beam_pushes"] == int(ctr[:, 4].sum()) - len(Q), (where, st)     # (the oracle counts the entry's push)
        assert st["exact_l2"] >= int(ctr[:, 1].sum()), (where, st)                 # speculative reranks: a superset
    return st


def _rev(want):
    return tuple(np.ascontiguousarray(x[::-1]) for x in want)


@pytest.mark.parametrize("name,bits,variant", CASES)
def test_fixture_batches_forward_and_reversed(cph, oracle, name, bits, variant):
    """Default launch (24 queries: the instantiation without probe first on full-capacity slots) and the main launch
    on 8 slots (probe first where the index allows it), every k, forward and reversed."""
    path = fixture_path(name, bits, variant)
    Q = golden()[f"Q/{name}"]
    Qr = np.ascontiguousarray(Q[::-1])
    for slots in (0, 8):
        ix = cph.CPIndex(DATASETS[name]["dim"], bits)
        ix.load(path)
        ix.set_search_params(slots=slots, beam_capacity=0)
        for k in KS:
            want = want_for(oracle, path, Q, k)
            _check(ix, Q, k, want, (name, bits, variant, slots, k))
            _check(ix, Qr, k, _rev(want), (name, bits, variant, slots, k, "reversed"))


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g128", 2)])
def test_both_capacity_tests_fire_and_the_rerun_answers(cph, oracle, name, bits):
    """A slot capacity of 64: beams outgrow it (the oracle's largest beam says so) and the attempt ends at the beam's
    capacity test; the re-run launch answers.  `rerun_queries > 0`."""
    path = fixture_path(name, bits)
    Q = golden()[f"Q/{name}"]
    want = want_for(oracle, path, Q, 10)
    assert (want[3][:, 5] > 64).any(), int(want[3][:, 5].max())
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(path)
    ix.set_search_params(slots=8, beam_capacity=64)
    _check(ix, Q, 10, want, (name, bits, "cap 64"), reruns=True)
    _check(ix, np.ascontiguousarray(Q[::-1]), 10, _rev(want), (name, bits, "cap 64, reversed"), reruns=True)


def test_id_log_fills_and_the_bitmap_is_wiped(cph, oracle):
    """A capacity no beam of the batch overflows by itself but that the id log of some query outgrows: that query stops
    logging and wipes its bitmap at the end; a bitmap left dirty would show in the batches behind it on the handle."""
    path = fixture_path("g128", 4)
    Q = golden()["Q/g128"]
    want = want_for(oracle, path, Q, 10)
    ctr = want[3]
    cap = int(ctr[:, 5].max()) + 32
    assert (ctr[:, 3] + 1 > cap).any(), (cap, int(ctr[:, 3].max()))
    ix = cph.CPIndex(128, 4)
    ix.load(path)
    ix.set_search_params(slots=8, beam_capacity=cap)
    st = _check(ix, Q, 10, want, ("g128", "log fills"), reruns=False)
    assert st["capacity"] == max(64, cap), st
    _check(ix, Q, 10, want, ("g128", "log fills, again"), reruns=False)
    _check(ix, np.ascontiguousarray(Q[::-1]), 10, _rev(want), ("g128", "log fills, reversed"), reruns=False)


@pytest.mark.parametrize("bits", [2, 4])
def test_filtered_and_per_query_filtered_batches(cph, oracle, bits):
    """The filtered instantiations expand exactly what the unfiltered search expands (only the result heap is gated), so
    with every id allowed rows, distances and expansions are the oracle's; with half the ids allowed the per-query
    form of the batch must equal the single-filter form, query by query, forward and reversed."""
    path = fixture_path("g128", bits, "shortcount")
    Q = golden()["Q/g128"]
    Qr = np.ascontiguousarray(Q[::-1])
    ix = cph.CPIndex(128, bits)
    ix.load(path)
    ix.set_search_params(slots=8, beam_capacity=0)
    everything = ix.make_filter(np.ones(ix.size, bool))
    half = ix.make_filter(np.arange(ix.size) % 2 == 0)
    for k in (1, 10, 100):
        oids, od, _, ctr = want_for(oracle, path, Q, k)
        ids, d = ix.search_batch(Q, k, filter=everything)
        assert np.array_equal(ids, oids) and _beq(d, od), (bits, k)
        assert np.array_equal(ix.last_query_expansions(len(Q)).astype(np.uint64), ctr[:, 0]), (bits, k)
        fo = np.arange(len(Q)) % 2
        got = ix.search_batch(Q, k, filter=[everything, half], filter_of=fo)
        a = ix.search_batch(Q, k, filter=everything)
        b = ix.search_batch(Q, k, filter=half)
        assert (b[0][b[0] >= 0] % 2 == 0).all(), (bits, k)
        for j in (0, 1):
            src = (a, b)[j]
            assert np.array_equal(got[0][fo == j], src[0][fo == j]), (bits, k, j)
            assert _beq(got[1][fo == j], src[1][fo == j]), (bits, k, j)
        rev = ix.search_batch(Qr, k, filter=[everything, half], filter_of=fo[::-1].copy())
        assert np.array_equal(rev[0], got[0][::-1]) and _beq(rev[1], np.ascontiguousarray(got[1][::-1])), (bits, k, "reversed")


def test_d1024_four_bits(cph, oracle, tmp_path):
    """`<4,1024,*>` has no fixture: 600 Gaussian rows through the project's builder, 32 queries of which 8 are stored
    rows (distance below 1e-12: the estimator's arm outside its usual range), on 8 slots and in the default launch."""
    rng = np.random.default_rng(41024)
    X = rng.standard_normal((600, 1024)).astype(np.float32)
    Q = rng.standard_normal((32, 1024)).astype(np.float32)
    Q[::4] = X[:8]
    ix = cph.CPIndex(1024, 4)
    ix.build(X)
    ix.finalize()
    p = str(tmp_path / "d1024_b4.idx")
    ix.save(p)
    for slots in (0, 8):
        ix = cph.CPIndex(1024, 4)
        ix.load(p)
        ix.set_search_params(slots=slots, beam_capacity=0)
        for k in (1, 10, 100):
            want = want_for(oracle, p, Q, k)
            _check(ix, Q, k, want, (1024, 4, slots, k))
            _check(ix, np.ascontiguousarray(Q[::-1]), k, _rev(want), (1024, 4, slots, k, "reversed"))
