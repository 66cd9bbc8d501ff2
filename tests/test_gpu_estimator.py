"""The N-bit estimator of the search kernels' expansion (csrc/device_fastscan.h: sqrt_in_range, lower_bounds_split and
stage2_est_only in their static-D forms; csrc/device_search_expansion.inc: `estimate`), which the static-D search
kernels evaluate with fewer vector instructions than the separate functions the block hook runs.

1. A device self-test (cph_debug_estimator, csrc/device_estimator_test.h): on 64 real neighbour blocks of a small index,
   at 2 and 4 bits and D = 128 and 1024, the expansion's path and stage1_lower + stage2_est give the same bits -- two zeros
   of different sign or two NaNs count as equal -- for the blocks as they are and with their aux values forced to the
   edges (ip_qo under the floor, at and under 1e-10, nop = 0, numerators that drive the cosine past +1 and past -1, a
   bound that rounds below 0), each over dqp in {1e-12, the next float, 1e-6, 1, 3e4, 1e30, FLT_MAX, +inf} (and, beyond what
   the range test lets through, 0 and 5e-13).

2. Whole searches against the oracle -- rows, distance bytes, per-query expansions, the batch counters -- at the smallest
   shapes that reach the arms: the batches of tests/test_gpu_steady_tail.py (96 queries, 16 slots, 3,000 clustered and
   4,000 Gaussian rows, D = 128) at 4 and at 2 bits, and one D = 1024 index of 2,000 rows; each also with queries that are
   base rows themselves, so that dqp = 0 at the hit and the arm outside the range runs.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, SLOTS = 96, 16
FMAX = np.float32(3.402823466e+38)


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


class Built:
    """An index, its oracle twin and the oracle's answers per (queries, k): computed once, on first use, never modified."""

    def __init__(self, cph, oracle, tmp, dim, bits, n, clustered):
        rng = np.random.default_rng(8128 if clustered else 8129)        # (the rows of tests/test_gpu_steady_tail.py at dim 128)
        if clustered:
            centres = rng.standard_normal((30, dim)).astype(np.float32)
            self.X = (centres[rng.integers(0, 30, n)] + 0.35 * rng.standard_normal((n, dim))).astype(np.float32)
            self.Q = (centres[rng.integers(0, 30, NQ)] + 0.35 * rng.standard_normal((NQ, dim))).astype(np.float32)
        else:
            self.X = rng.standard_normal((n, dim)).astype(np.float32)
            self.Q = rng.standard_normal((NQ, dim)).astype(np.float32)
        self.dim, self.bits, self.n = dim, bits, n
        ix = cph.CPIndex(dim, bits)
        ix.build(self.X)
        ix.finalize()
        self.path = str(tmp / ("est_%d_%d_%d.idx" % (dim, bits, clustered)))
        ix.save(self.path)
        self.oi = oracle.load(self.path)
        # queries that are base rows themselves (the stored rows: the builder reorders them), between ordinary ones
        rows = ix.get_vectors(0, n)[:: max(1, n // 32)][:32]
        self.Q_rows = np.ascontiguousarray(np.concatenate([rows, self.Q[: NQ - len(rows)]]), np.float32)
        self._want = {}

    def want(self, which, k):
        if (which, k) not in self._want:
            Q = self.Q if which == "q" else self.Q_rows
            self._want[(which, k)] = self.oi.search_batch(Q, k, nthreads=16, counters=True)
        return self._want[(which, k)]

    def index(self, cph, cap=0):
        ix = cph.CPIndex(self.dim, self.bits)
        ix.load(self.path)
        ix.set_search_params(slots=SLOTS, beam_capacity=cap if cap else self.n + 1)
        return ix


_BUILT = {}


@pytest.fixture(scope="module")
def built_for(cph, oracle, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("estimator")

    def get(dim, bits, n, clustered=True):
        key = (dim, bits, n, clustered)
        if key not in _BUILT:
            _BUILT[key] = Built(cph, oracle, tmp, dim, bits, n, clustered)
        return _BUILT[key]
    return get


# ---- 1. the device self-test -----------------------------------------------------------------------------------------
DQP = np.array([1e-12, np.nextafter(np.float32(1e-12), np.float32(1)), 1e-6, 1.0, 3e4, 1e30, FMAX, np.inf, 0.0, 5e-13], np.float32)
NOP, IPQO, IPCP = 1, 2, 4
# (mask, nop, ip_qo, ip_cp): what replaces the aux values of every lane of a block
FORCED = [
    (0, 0, 0, 0),                                   # the blocks as they are
    (IPQO, 0, 0.05, 0),                             # ip_qo below the floor of the first parameter set
    (IPQO, 0, 1e-10, 0),                            # ip_qo at 1e-10 (with floor = 0: ipq > 1e-10 is false)
    (IPQO, 0, np.nextafter(np.float32(1e-10), np.float32(1)), 0),   # ... just above it
    (IPQO, 0, 5e-11, 0),                            # ... below it
    (IPQO, 0, 0.0, 0),                              # ... zero: the quotients are inf or NaN, and discarded
    (NOP, 0.0, 0, 0),                               # nop = 0
    (IPCP, 0, 0, -1e6),                             # numerator far above: cosine past +1
    (IPCP, 0, 0, 1e6),                              # numerator far below: cosine past -1
    (IPQO | IPCP, 0, 1e-10, -1e6),
    # cosine = +1 and nop next to sqrt(dqp): nop^2 + dqp - 2 nop sqrt(dqp) is 0 up to rounding, below it for some
    (NOP | IPCP, 1e-6, 0, -1e6), (NOP | IPCP, np.nextafter(np.float32(1e-6), np.float32(1)), 0, -1e6),
    (NOP | IPCP, 1e-3, 0, -1e6), (NOP | IPCP, 1.0000001, 0, -1e6), (NOP | IPCP, 0.9999999, 0, -1e6),
    (NOP | IPCP, 173.20508, 0, -1e6), (NOP | IPCP, 173.2051, 0, -1e6), (NOP | IPCP, 1e15, 0, -1e6),
]
# affine_a, affine_b, floor, slack
PARAMS = [(0.97, 0.01, 0.2, 0.07), (1.0, 0.0, 0.0, 0.0), (0.93, 0.02, 0.0, -0.05)]
BLOCKS = 64


def _estimator(cph, ix, lut, qp, first, count):
    from cphnsw_mi355x import _lib
    force = np.ascontiguousarray([[f[1], f[2], f[3]] for f in FORCED], np.float32)
    fmask = np.ascontiguousarray([f[0] for f in FORCED], np.uint32)
    lut = np.ascontiguousarray(lut, np.uint8)
    qp = np.ascontiguousarray(qp, np.float32)
    out = np.zeros((count, len(FORCED), len(DQP), 6, 32), np.uint32)
    _lib.check(_lib.lib().cph_debug_estimator(ix._h, lut.ctypes.data, qp.ctypes.data, first, count, DQP.ctypes.data, len(DQP),
                                              force.ctypes.data, fmask.ctypes.data, len(FORCED), out.ctypes.data))
    return out


@pytest.mark.parametrize("dim,bits,n", [(128, 4, 3000), (128, 2, 3000), (1024, 4, 2000), (1024, 2, 300)])
def test_expansion_path_gives_the_separate_functions_bits(cph, built_for, dim, bits, n):
    b = built_for(dim, bits, n)
    ix = b.index(cph)
    for qi, tail in enumerate(PARAMS):
        lut, co = ix.encode_query(b.Q[qi])
        qp = np.array([co[0], co[1], co[2], *tail], np.float32)
        out = _estimator(cph, ix, lut, qp, 17 * qi, BLOCKS)
        new, ref = out[:, :, :, 0:3, :], out[:, :, :, 3:6, :]
        fn, fr = new.view(np.float32), ref.view(np.float32)
        same = (new == ref) | ((fn == 0) & (fr == 0)) | (np.isnan(fn) & np.isnan(fr))
        bad = np.argwhere(~same)
        print(dim, bits, "params", tail, "values", same.size, "differ", len(bad),
              "NaN", int(np.isnan(fr).sum()), "zero", int((fr == 0).sum()), "positive bounds", int((fr[:, :, :, :2] > 0).sum()))
        for blk, s, j, f, lane in bad[:10]:
            print("  block", 17 * qi + blk, "forced", FORCED[s], "dqp", DQP[j], ("lo1", "lo2", "est")[f], "lane", lane,
                  "expansion %r (%08x)" % (fn[blk, s, j, f, lane], new[blk, s, j, f, lane]),
                  "separate %r (%08x)" % (fr[blk, s, j, f, lane], ref[blk, s, j, f, lane]))
        assert len(bad) == 0, (dim, bits, tail, len(bad))
        # the inputs do reach the edges: clamped cosines give bounds of exactly 0 and positive ones, +inf gives NaN
        assert np.isnan(fr[:, 0, 7, 0, :]).any() and (fr[:, 7:, :8, :2, :] == 0).any() and (fr[:, 0, 2:7, :2, :] > 0).any()


def test_hook_refuses_what_it_cannot_run(cph, built_for):
    from cphnsw_mi355x import _lib
    b = built_for(128, 4, 3000)
    ix = b.index(cph)
    lut, co = ix.encode_query(b.Q[0])
    qp = np.array([co[0], co[1], co[2], *PARAMS[0]], np.float32)
    with pytest.raises(ValueError, match="vertex out of range"):
        _estimator(cph, ix, lut, qp, b.n - 10, BLOCKS)
    out = np.zeros(6 * 32, np.uint32)
    one = np.zeros(3, np.float32)
    m = np.zeros(1, np.uint32)
    with pytest.raises(ValueError):
        _lib.check(_lib.lib().cph_debug_estimator(ix._h, lut.ctypes.data, qp.ctypes.data, 0, 0, one.ctypes.data, 1, one.ctypes.data,
                                                  m.ctypes.data, 1, out.ctypes.data))


# ---- 2. whole searches -----------------------------------------------------------------------------------------------
def _check(ix, Q, k, want, where):
    oids, od, _, ctr = want
    ids, d = ix.search_batch(Q, k)
    st = ix.last_search_stats()
    work = ix.last_query_expansions(len(Q)).astype(np.uint64)
    print(where, st)
    assert np.array_equal(ids, oids), (where, int((ids != oids).any(axis=1).sum()))
    assert _beq(d, od), where
    assert np.array_equal(work, ctr[:, 0]), (where, int((work != ctr[:, 0]).sum()))
    assert st["slots"] == SLOTS, (where, st)
    if st["rerun_queries"]:              # a re-run query's first attempt is counted too
        assert st["expansions"] >= int(ctr[:, 0].sum()), (where, st)
        return st
    assert st["expansions"] == int(ctr[:, 0].sum()), (where, st)
    assert st["new_neighbours"] == int(ctr[:, 3].sum()), (where, st)
    assert st["beam_pushes"] == int(ctr[:, 4].sum()) - len(Q), (where, st)      # (the oracle counts the entry's push)
    assert st["exact_l2"] >= int(ctr[:, 1].sum()), (where, st)                  # speculative reranks: a superset
    return st


# (name, capacity or 0 = rows + 1, k): CENSUS_BATCHES of tests/test_gpu_steady_tail.py
BATCHES = [("c_k10", 0, 10), ("c_k2", 0, 2), ("c_k5", 0, 5), ("g_k10", 0, 10), ("g_k100", 0, 100), ("c_k30", 0, 30),
           ("c_k10_cap64", 64, 10), ("c_k10_cap99", 99, 10)]


@pytest.mark.parametrize("bits", [4, 2])
@pytest.mark.parametrize("name,cap,k", BATCHES)
def test_steady_tail_batches(cph, built_for, bits, name, cap, k):
    clustered = not name.startswith("g")
    b = built_for(128, bits, 3000 if clustered else 4000, clustered)
    st = _check(b.index(cph, cap), b.Q, k, b.want("q", k), "%s b%d" % (name, bits))
    if name == "c_k10_cap64" and bits == 4:
        assert st["rerun_queries"] > 0, st


@pytest.mark.parametrize("dim,bits,n", [(128, 4, 3000), (128, 2, 3000), (1024, 4, 2000)])
def test_queries_that_are_base_rows(cph, built_for, dim, bits, n):
    """32 of the 96 queries are stored rows: the search pops the row itself at distance 0 (asserted from the oracle's answer),
    below 1e-12, and that expansion takes the arm outside the estimator's range."""
    b = built_for(dim, bits, n)
    want = b.want("r", 10)
    print("hits below 1e-12:", int((want[1][:32, 0] < 1e-12).sum()), "of 32")
    assert (want[1][:32, 0] < 1e-12).any(), want[1][:32, 0]
    _check(b.index(cph), b.Q_rows, 10, want, "rows d%d b%d" % (dim, bits))


def test_dim_1024(cph, built_for):
    b = built_for(1024, 4, 2000)
    _check(b.index(cph), b.Q, 10, b.want("q", 10), "d1024 b4")
