"""The tail of the steady expansion loop (csrc/device_search_expansion.inc, from the candidate ballot to the back edge):
in the steady copy of `search_kernel<4,128,true>` the beam pushes of an expansion take one of several arms -- nothing to
push, a lane-parallel append in LDS, an append onto a spilled beam, a single push that skips it, serial pushes, the
serial replay with candidates -- and the rarely changed state (speculative reranks, the id log's `wipe`) is not
carried through the loop.  Every case compares rows, distance bytes, per-query expansions and the batch totals
(`new_neighbours`, `beam_pushes`) with the oracle, as tests/test_gpu_steady_loop.py does.

4-bit, dim 128.  3,000 clustered rows (30 clusters; batches "c_...") and 4,000 Gaussian rows ("g_...": beams beyond 255
entries, and beams small enough early on that an expansion has more pushes than the beam has entries); 96 queries per
batch on 16 explicit slots with an explicit capacity: the main, probe-first launch (`<4,128,true>`), six queries per
wave.

One case per arm.  The shipped kernel counts no arm, and the oracle's counters can name only some (the largest beam,
the reranks, the new neighbours against the capacity: asserted on the CPU before anything runs on the GPU).  Which
arms each batch takes INSIDE THE STEADY COPY was counted once with a diagnostic build (`-DCPH_TAIL_CENSUS`,
`scripts/tail_census.py` over `CENSUS_BATCHES` below; table in profiles/steady_tail.md section 8).  Steady expansions per
batch, the arm each case is about in brackets:

    batch        append  spilled  single push   a push beats  nothing   more pushes   replay with
                 in LDS  append   skips append  its parent    to push   than entries  candidates
    c_k10        [360]   0        0             289           442       0             33
    c_k2         235     0        0             [306]         432       0             4
    c_k5         305     0        0             292           [463]     0             16
    g_k10        2534    0        0             9383          9786      [11]          429
    g_k100       3849    [829]    [3096]        11927         19252     9             3792
    c_k30        430     0        0             214           446       0             [140]
    c_k10_cap64  335     0        0             268           405       0             31      (6 queries re-run)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIM, N, N_GAUSS, NQ, SLOTS = 128, 3000, 4000, 96, 16
K_BEAM_LDS = 255


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


class Built:
    """The index, its oracle twin and the oracle's answers per k (computed once, on first use, never modified)."""

    def __init__(self, cph, oracle, tmp, clustered=True):
        rng = np.random.default_rng(8128 if clustered else 8129)
        if clustered:
            centres = rng.standard_normal((30, DIM)).astype(np.float32)
            X = (centres[rng.integers(0, 30, N)] + 0.35 * rng.standard_normal((N, DIM))).astype(np.float32)
            self.Q = (centres[rng.integers(0, 30, NQ)] + 0.35 * rng.standard_normal((NQ, DIM))).astype(np.float32)
        else:
            X = rng.standard_normal((N_GAUSS, DIM)).astype(np.float32)
            self.Q = rng.standard_normal((NQ, DIM)).astype(np.float32)
        self.n = len(X)
        ix = cph.CPIndex(DIM, 4)
        ix.build(X)
        ix.finalize()
        self.path = str(tmp / ("steady_tail_%d.idx" % clustered))
        ix.save(self.path)
        self.oi = oracle.load(self.path)
        self._want = {}

    def queries(self, name):
        return self.Q

    def want(self, k):
        if k not in self._want:
            self._want[k] = self.oi.search_batch(self.Q, k, nthreads=16, counters=True)
        return self._want[k]


_BUILT = {}


def built_for(cph, oracle, tmp, name):
    """The index a census batch (or a test) runs on: "g..." batches use the Gaussian rows, the others the clustered ones."""
    clustered = not name.startswith("g")
    if clustered not in _BUILT:
        _BUILT[clustered] = Built(cph, oracle, tmp, clustered)
    return _BUILT[clustered]


@pytest.fixture(scope="module")
def built(cph, oracle, tmp_path_factory):
    return built_for(cph, oracle, tmp_path_factory.mktemp("steady_tail"), "c")


@pytest.fixture(scope="module")
def built_gauss(cph, oracle, tmp_path_factory):
    """4,000 Gaussian rows: nothing to tell apart at dim 128, so the beams grow far beyond what the clustered rows need."""
    return built_for(cph, oracle, tmp_path_factory.mktemp("steady_tail_g"), "g")


# (name, capacity or 0 = rows + 1, k): the batches scripts/tail_census.py counts the arms of
CENSUS_BATCHES = [("c_k10", 0, 10), ("c_k2", 0, 2), ("c_k5", 0, 5), ("g_k10", 0, 10), ("g_k100", 0, 100), ("c_k30", 0, 30),
                  ("c_k10_cap64", 64, 10), ("c_k10_cap99", 99, 10)]


def _index(cph, b, cap):
    ix = cph.CPIndex(DIM, 4)
    ix.load(b.path)
    ix.set_search_params(slots=SLOTS, beam_capacity=cap)
    return ix


def _check(ix, Q, k, want, where, reruns=False):
    oids, od, _, ctr = want
    ids, d = ix.search_batch(Q, k)
    st = ix.last_search_stats()
    work = ix.last_query_expansions(len(Q)).astype(np.uint64)
    print(where, st)
    assert np.array_equal(ids, oids), (where, int((ids != oids).any(axis=1).sum()))
    assert _beq(d, od), where
    assert np.array_equal(work, ctr[:, 0]), (where, int((work != ctr[:, 0]).sum()))
    assert st["slots"] == SLOTS, (where, st)
    if reruns:
        assert st["rerun_queries"] > 0, (where, st)
        assert st["expansions"] >= int(ctr[:, 0].sum()), (where, st)
        return st
    assert st["rerun_queries"] == 0, (where, st)
    assert st["expansions"] == int(ctr[:, 0].sum()), (where, st)
    assert st["new_neighbours"] == int(ctr[:, 3].sum()), (where, st)
    assert st["beam_pushes"] == int(ctr[:, 4].sum()) - len(Q), (where, st)      # (the oracle counts the entry's push)
    assert st["exact_l2"] >= int(ctr[:, 1].sum()), (where, st)                  # speculative reranks: a superset
    return st


def test_usual_batch_appends_in_lds(cph, built):
    """c_k10, full capacity: every beam stays in LDS (the oracle's largest beam), queries run long past the warm-up (the
    oracle's expansions).  Census: 360 steady expansions append in LDS."""
    want = built.want(10)
    ctr = want[3]
    assert int(ctr[:, 5].max()) <= K_BEAM_LDS, int(ctr[:, 5].max())
    assert int(ctr[:, 0].min()) >= 10, int(ctr[:, 0].min())
    _check(_index(cph, built, N + 1), built.Q, 10, want, "c_k10")


def test_push_beats_its_parent_serial_pushes(cph, built):
    """c_k2: clustered rows, later neighbours closer than earlier ones.  Census: in 306 steady expansions the parent check
    of the append fails and the pushes run serially on the mask the append left untouched."""
    _check(_index(cph, built, N + 1), built.Q, 2, built.want(2), "c_k2")


def test_new_neighbours_but_nothing_to_push(cph, built):
    """c_k5.  Census: 463 steady expansions have new neighbours of which none passes the push test (np == 0): they reach
    the serial loop's test with an empty mask through the single compare `np - 1u <= beam_size`."""
    _check(_index(cph, built, N + 1), built.Q, 5, built.want(5), "c_k5")


def test_more_pushes_than_the_beam_has_entries(cph, built_gauss):
    """g_k10: Gaussian rows, a small k, so the beam is short when the query has just changed loops.  Census: 11 steady
    expansions have np > beam_size + 1 (the append cannot check its parents in parallel; serial pushes); none on the
    clustered rows."""
    want = built_gauss.want(10)
    assert int(want[3][:, 5].max()) <= K_BEAM_LDS, int(want[3][:, 5].max())
    _check(_index(cph, built_gauss, N_GAUSS + 1), built_gauss.Q, 10, want, "g_k10")


def test_beam_crosses_the_lds_levels(cph, built_gauss):
    """g_k100: k = 100 on the Gaussian rows (the index has no slack knob; this is the data on which k = 100 crosses).
    Asserted on the CPU from the oracle's push and pop counters: some query's beam outgrows kBeamLds = 255 entries and
    every result heap fills, so the crossing happens past the warm-up.  Census: 829 steady expansions append onto a
    spilled beam (`in_lds` false), 3,096 are the single push that skips the append, 3,849 still append in LDS."""
    want = built_gauss.want(100)
    assert int(want[3][:, 5].max()) > K_BEAM_LDS, int(want[3][:, 5].max())
    assert (want[2] == 100).all()
    _check(_index(cph, built_gauss, N_GAUSS + 1), built_gauss.Q, 100, want, "g_k100")


def test_candidates_inside_the_steady_copy(cph, built):
    """c_k30.  Census: 140 steady expansions have candidates and take the serial replay (`nn_push_wave<true>`).  The
    speculative reranks are summed in LDS in the two-loop instantiations: `exact_l2` covers the oracle's count, and
    the oracle reranks (exact distances beyond the entry and one per expansion) in every query."""
    want = built.want(30)
    ctr = want[3]
    reranks = ctr[:, 1].astype(np.int64) - 1 - ctr[:, 0].astype(np.int64)
    assert (reranks > 0).all(), reranks
    st = _check(_index(cph, built, N + 1), built.Q, 30, want, "c_k30")
    assert st["exact_l2"] >= NQ + st["expansions"] + int(reranks.sum()), st


def test_small_capacity_overflows_and_reruns(cph, built):
    """c_k10_cap64: queries whose beam outgrows 64 entries (the oracle's largest beam) end their attempt in the middle of
    an expansion and are answered by the re-run launch; they are long queries (at least ten expansions, asserted: the
    result heap of k = 10 is full behind the first).  Six queries of this batch re-run."""
    want = built.want(10)
    over = want[3][:, 5] > 64              # the oracle's largest beam: these queries overflow a slot of 64
    assert over.any()
    assert (want[3][over, 0] >= 10).all(), want[3][over, 0].min()
    _check(_index(cph, built, 64), built.Q, 10, want, "c_k10_cap64", reruns=True)


def test_id_log_wipes(cph, built):
    """c_k10_cap99: a capacity that no beam can overflow (the oracle's largest beam + 32 new neighbours) but that the id
    log of some query outgrows (new neighbours + the entry > capacity): the query stops logging and wipes its bitmap
    at the end.  `wipe` is derived from the log's length in the two-loop instantiations; a bitmap left dirty shows in
    the batches behind it, so the batch runs twice on the handle."""
    want = built.want(10)
    ctr = want[3]
    cap = 99
    assert int(ctr[:, 5].max()) + 32 <= cap, int(ctr[:, 5].max())
    assert (ctr[:, 3] + 1 > cap).any(), (cap, int(ctr[:, 3].max()))
    ix = _index(cph, built, cap)
    st = _check(ix, built.Q, 10, want, "c_k10_cap99")
    assert st["capacity"] == cap, st
    _check(ix, built.Q, 10, want, "c_k10_cap99, again")


def test_same_batch_three_times_one_reversed(cph, built):
    """One handle, the batch three times, the second time in reversed order: nothing a query leaves behind (bitmap, LDS
    totals, beam pages) may reach the next one."""
    want = built.want(10)
    ix = _index(cph, built, N + 1)
    _check(ix, built.Q, 10, want, "first")
    rev = tuple(np.ascontiguousarray(x[::-1]) for x in want)
    _check(ix, np.ascontiguousarray(built.Q[::-1]), 10, rev, "reversed")
    _check(ix, built.Q, 10, want, "third")
