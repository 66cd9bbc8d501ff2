"""The search kernel's two expansion loops: a query starts in the general loop and moves, once and at a loop head, into
the steady loop -- the same body compiled with the warm-up, the slack schedule and the repeated-id screen as
compile-time facts (csrc/device_search.h).  Nothing observable may depend on where a query changes loops, or on whether
it ever does: every case compares rows, distance bytes, per-query expansions, new neighbours and beam pushes with the
oracle (the filtered case: with the model of the filtered search).

The main cases run 40 queries on eight resident slots (`set_search_params(slots=8, beam_capacity=0)`: the main,
probe-first launch), so every wave answers five queries in a row and a steady query is followed by a fresh one.  k = 1
is steady after the first expansions, k = 300 lies beyond the 256 entries of the wave-parallel result heap, and one k
is larger than anything a query can fill (read off the oracle's counts): such a query never leaves the general loop.
The golden fixtures of the `affine` variant carry three slack levels, so their queries change loops only when the
schedule has reached the last one; the same fixture with repeated neighbour ids stays in the general loop throughout.

Only the 4-bit probe-first instantiations have a steady loop: the 4-bit cases on the main launch (the built indexes and
the `g128` 4-bit `affine` fixture with its repeated-ids copy) are the ones that cross the transition.  The direct
launch, the narrow codes, the filtered case and the other fixtures run one loop; they are here because the loop's text
and `nn_push_wave` are shared, so an edit for the steady copy must leave them where they were.
"""
import gzip

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path, vertex_layout

pytestmark = pytest.mark.gpu

# (dim, rows): D = 128 is the instantiation the benchmark runs, D = 1024 shares the code
SHAPES = {128: 3000, 1024: 1000}
NQ = 40


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


class Built:
    """One index from the project's builder, its oracle twin and the oracle's answers per k (computed once, on first
    use, never modified)."""

    def __init__(self, cph, oracle, tmp, dim, bits):
        self.dim, self.bits, self.n = dim, bits, SHAPES[dim]
        rng = np.random.default_rng(7100 + dim + bits)
        X = rng.standard_normal((self.n, dim)).astype(np.float32)
        self.Q = rng.standard_normal((NQ, dim)).astype(np.float32)
        ix = cph.CPIndex(dim, bits)
        ix.build(X)
        ix.finalize()
        self.path = str(tmp / f"steady_{dim}_b{bits}.idx")
        ix.save(self.path)
        self.oi = oracle.load(self.path)
        self._want = {}

    def want(self, k):
        if k not in self._want:
            self._want[k] = self.oi.search_batch(self.Q, k, nthreads=16, counters=True)
        return self._want[k]

    def unfillable_k(self):
        """One more than the most results any of the queries returns to a k far beyond the index (a result list may repeat
        ids, so the row count is no bound): no result heap of that size ever fills."""
        probe = 4 * self.n
        _, _, cnt, _ = self.oi.search_batch(self.Q, probe, nthreads=16, counters=True)
        assert int(cnt.max()) < probe
        return int(cnt.max()) + 1


@pytest.fixture(scope="module")
def built_cache(cph, oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("steady")
    cache = {}

    def get(dim, bits):
        if (dim, bits) not in cache:
            cache[(dim, bits)] = Built(cph, oracle, tmp, dim, bits)
        return cache[(dim, bits)]
    return get


def _check(ix, Q, k, want, nq_entry_pushes, where, reruns=False):
    """Rows, distance bytes and the search path of one batch against (ids, dist, counts, counters [nq, 9])."""
    oids, od, _, ctr = want
    ids, d = ix.search_batch(Q, k)
    st = ix.last_search_stats()
    work = ix.last_query_expansions(len(Q)).astype(np.uint64)
    print(where, st)
    assert np.array_equal(ids, oids), (where, int((ids != oids).any(axis=1).sum()))
    assert _beq(d, od), where
    assert np.array_equal(work, ctr[:, 0]), (where, int((work != ctr[:, 0]).sum()))
    if reruns:
        assert st["rerun_queries"] > 0, (where, st)                  # the case the test is about
        assert st["expansions"] >= int(ctr[:, 0].sum()), (where, st)  # (+ the overflowed first passes)
        return st
    assert st["rerun_queries"] == 0, (where, st)
    assert st["expansions"] == int(ctr[:, 0].sum()), (where, st)
    assert st["new_neighbours"] == int(ctr[:, 3].sum()), (where, st)
    assert st["beam_pushes"] == int(ctr[:, 4].sum()) - nq_entry_pushes, (where, st)   # (the oracle counts the entry's push)
    assert st["exact_l2"] >= int(ctr[:, 1].sum()), (where, st)                         # speculative reranks: a superset
    return st


def _main_launch(cph, b, k, cap=0):
    ix = cph.CPIndex(b.dim, b.bits)
    ix.load(b.path)
    ix.set_search_params(slots=8, beam_capacity=cap)
    assert len(b.Q) > 32       # more queries than full-capacity slots: the main launch, not the direct one
    return ix


@pytest.mark.parametrize("k", [1, 2, 10, 300, "unfillable"])
@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_main_launch_matches_oracle(cph, built_cache, dim, k):
    b = built_cache(dim, 4)
    unfillable = k == "unfillable"
    if unfillable:
        k = b.unfillable_k()
        assert (b.want(k)[2] < k).all()
    ix = _main_launch(cph, b, k)
    st = _check(ix, b.Q, k, b.want(k), NQ, (dim, 4, k, "main"))
    assert st["slots"] == 8, st
    if unfillable:
        # A search that never leaves the warm-up reranks every new neighbour and nothing else: no speculation, so the
        # exact-L2 count -- derived in this instantiation from the expansion count and the reranks -- is the oracle's, and
        # it is one per query (the entry) + one per expansion + one per new neighbour.
        assert st["exact_l2"] == int(b.want(k)[3][:, 1].sum()), st
        assert st["exact_l2"] == NQ + st["expansions"] + st["new_neighbours"], st


@pytest.mark.parametrize("dim", sorted(SHAPES))
def test_direct_launch_matches_oracle(cph, built_cache, dim):
    """32 queries or fewer: the direct launch on full-capacity slots, the instantiation without probe first (one loop,
    counters carried per expansion)."""
    b = built_cache(dim, 4)
    ix = cph.CPIndex(dim, 4)
    ix.load(b.path)
    for k in (1, 10):
        oids, od, cnt, ctr = b.want(k)
        for nq in (32, 5):
            _check(ix, b.Q[:nq], k, (oids[:nq], od[:nq], cnt[:nq], ctr[:nq]), nq, (dim, 4, k, "direct", nq))


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("bits", [2, 1])
def test_narrow_codes_match_oracle(cph, built_cache, bits, k):
    """2-bit and 1-bit codes on the main launch: one loop (the shared text with ST = false)."""
    b = built_cache(128, bits)
    ix = _main_launch(cph, b, k)
    _check(ix, b.Q, k, b.want(k), NQ, (128, bits, k, "main"))


def test_filtered_half_allowed_matches_model(cph, built_cache):
    """Half of the ids allowed: the result heap fills slowly.  The filtered instantiations run without probe first and
    keep one loop; what is covered is the shared text's heap-fill tests and `nn_push_wave`'s default arm under a filter."""
    from filtered_model_lib import ModelIndex
    b = built_cache(128, 4)
    mask = np.random.default_rng(7300).random(b.n) < 0.5
    mi = ModelIndex(b.path)
    ix = _main_launch(cph, b, 10)
    f = ix.make_filter(mask)
    for k in (1, 10):
        mids, md, _, mctr = mi.search_batch(b.Q, k, mask, nthreads=16)
        ids, d = ix.search_batch(b.Q, k, filter=f)
        st = ix.last_search_stats()
        assert np.array_equal(ids, mids), k
        assert _beq(d, md), k
        assert np.array_equal(ix.last_query_expansions(NQ).astype(np.uint64), mctr[:, 0]), k
        assert st["rerun_queries"] == 0, st
        assert st["expansions"] == int(mctr[:, 0].sum()), st
        assert st["new_neighbours"] == int(mctr[:, 3].sum()), st
        assert st["beam_pushes"] == int(mctr[:, 4].sum()) - NQ, st


def test_small_capacity_reruns_match_oracle(cph, built_cache):
    """Slots of 64 entries: the attempt ends in the steady loop and the query is answered by the re-run launch.  The
    order is forced: the first expansion reranks its up to 32 new neighbours into the result heap, so a heap of k = 10
    is full behind it and the query changes loops at the next head at which the slack schedule is saturated; the beam
    holds at most 33 entries behind the first expansion and 64 behind the second, so it cannot outgrow 64 before the
    third.  The overflowing queries are long ones (asserted below on the oracle's counts)."""
    b = built_cache(128, 4)
    want = b.want(10)
    over = want[3][:, 5] > 64              # the oracle's largest beam: these queries overflow a slot of 64
    assert over.any()
    assert (want[3][over, 0] >= 10).all(), want[3][over, 0].min()
    ix = _main_launch(cph, b, 10, cap=64)
    _check(ix, b.Q, 10, want, NQ, (128, 4, 10, "capacity 64"), reruns=True)


def _with_repeated_ids(src, name, bits, dst):
    """The fixture with slots 5 and 7 of every third vertex's list repeating slots 2 and 0 (the loader flags it)."""
    dim, n, D = DATASETS[name]["dim"], DATASETS[name]["n"], DATASETS[name]["D"]
    data = bytearray(gzip.open(src, "rb").read() if src.endswith(".gz") else open(src, "rb").read())
    vb, nb_off, codes = vertex_layout(D, bits)
    base = 68 + 248 + 72 + dim * 4 + n * 4 + n * 4 + n * D * 4
    ids_off = nb_off + codes + 3 * 128 + 64 + (64 if bits > 1 else 0)
    patched = 0
    for v in range(0, n, 3):
        o = base + v * vb + ids_off
        if int.from_bytes(data[o + 128:o + 132], "little") >= 8:
            data[o + 5 * 4:o + 6 * 4] = data[o + 2 * 4:o + 3 * 4]
            data[o + 7 * 4:o + 8 * 4] = data[o + 0 * 4:o + 1 * 4]
            patched += 1
    assert patched > 50
    with open(dst, "wb") as f:
        f.write(bytes(data))
    return dst


GOLDEN_CASES = [(n, bits, rep) for n, s in DATASETS.items() if "affine" in s["variants"] for bits in s["bits"]
                for rep in ((False, True) if (n, bits) == ("g128", 4) else (False,))]


@pytest.mark.parametrize("name,bits,repeated", GOLDEN_CASES)
def test_three_slack_levels_match_oracle(cph, oracle, gold, tmp_path, name, bits, repeated):
    """The `affine` fixtures: three slack levels, so a query reaches the steady loop only behind its third expansion
    with neighbours -- and never on the copy whose lists repeat ids.  24 queries on eight slots and on the direct launch."""
    p = fixture_path(name, bits, "affine")
    if repeated:
        p = _with_repeated_ids(p, name, bits, str(tmp_path / "affine_dups.idx"))
    oi = oracle.load(p)
    Q = gold[f"Q/{name}"]
    for slots in (8, 0):
        ix = cph.CPIndex(DATASETS[name]["dim"], bits)
        ix.load(p)
        ix.set_search_params(slots=slots, beam_capacity=0)
        for k in (1, 10, 100):
            want = oi.search_batch(Q, k, nthreads=16, counters=True)
            _check(ix, Q, k, want, len(Q), (name, bits, "affine", repeated, slots, k))
