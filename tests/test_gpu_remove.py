"""Removed rows on the GPU (CPIndex.remove / live_count / removed_mask / compact).

The contract: with a set R of removed ids, every search entry point returns the bytes the same call returns on the same
index without R under the filter F & ~R.  So handle A gets remove(R); handle B is the same file, untouched, and is
given the explicit filter -- ids, distance bytes, the counters other than kernel_us and the per-query expansions must be
equal; one batch case is also pinned independently of the library against the model of the filtered search
(tests/filtered_model_lib.ModelIndex)."""
import zlib

import numpy as np
import pytest

from filtered_model_lib import ModelIndex
from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
FIXTURES = [("g128", 4), ("g16", 1), ("g1024", 2)]      # the probe-first instantiation; n = 300: a partial last word; n = 160
R_KINDS = ["p10", "p50", "fifth", "one", "all_but_3", "every"]


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _load(cph, name, bits, **kw):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits, **kw)
    ix.load(fixture_path(name, bits))
    return ix


def _removed(kind, n, seed):
    rng = np.random.default_rng(seed)
    r = np.zeros(n, bool)
    if kind == "p10":
        r = rng.random(n) < 0.1
    elif kind == "p50":
        r = rng.random(n) < 0.5
    elif kind == "fifth":
        r[n // 3:n // 3 + n // 5] = True
    elif kind == "one":
        r[n - 1] = True
    elif kind == "all_but_3":
        r[:] = True
        r[rng.choice(n, 3, replace=False)] = False
    elif kind == "every":
        r[:] = True
    return r


def _stats(ix, nq):
    st = ix.last_search_stats()
    st.pop("kernel_us")
    return st, ix.last_query_expansions(nq)


def _same(a_call, b_call, A, B, nq, R, where):
    """Runs the two calls; rows, counters and expansions must be equal, and no row of A may hold a removed id."""
    ai, ad = a_call()
    sa, wa = _stats(A, nq)
    bi, bd = b_call()
    sb, wb = _stats(B, nq)
    assert np.array_equal(ai, bi), where
    assert _beq(ad, bd), where
    assert sa == sb, (where, sa, sb)
    assert np.array_equal(wa, wb), where
    got = ai[ai >= 0]
    assert not R[got].any(), where
    assert ((ai >= 0) == (ad != FMAX)).all(), where
    return ai, ad, sa, wa


@pytest.mark.parametrize("kind", R_KINDS)
@pytest.mark.parametrize("name,bits", FIXTURES)
def test_remove_equals_explicit_filter(cph, gold, name, bits, kind):
    import torch
    A, B = _load(cph, name, bits), _load(cph, name, bits)
    n = A.size
    Q = gold[f"Q/{name}"]
    nq = len(Q)
    seed = zlib.crc32(f"{name}{bits}{kind}".encode())
    R = _removed(kind, n, seed)
    rng = np.random.default_rng(seed + 1)
    G1, G2 = rng.random(n) < 0.5, rng.random(n) < 0.2
    fo = rng.integers(-1, 2, nq).astype(np.int32)
    fo[:3] = (-1, 0, 1)
    fo_b = np.where(fo < 0, 2, fo).astype(np.int32)
    assert A.remove(np.flatnonzero(R)) == int(R.sum())
    assert A.size == n and A.live_count == n - int(R.sum())
    assert np.array_equal(A.removed_mask(), R)
    notR = B.make_filter(~R)
    g1a, g2a = A.make_filter(G1), A.make_filter(G2)
    g1b, g2b = B.make_filter(G1 & ~R), B.make_filter(G2 & ~R)
    Qd = torch.from_numpy(Q).to(f"cuda:{A.devices[0]}")
    for k in (1, 10, 100):
        w = (name, bits, kind, k)
        ids, d, st, work = _same(lambda: A.search_batch(Q, k), lambda: B.search_batch(Q, k, filter=notR), A, B, nq, R, w + ("batch",))
        if kind == "all_but_3":
            # three ids are left.  The graph search may report an id in more than one slot (as the unfiltered search and
            # the reference do; the row equals B's above), so the bound is on the DISTINCT ids; rows are shorter than k
            assert all(len(set(r[r >= 0])) <= 3 for r in ids), w
            if k > 3:
                assert ((ids >= 0).sum(axis=1) < k).all() and (ids[:, -1] == -1).all(), w
        if kind == "every":
            assert (ids == -1).all() and (d == FMAX).all() and st["expansions"] == 0 and (work == 0).all(), w
        ids, d, st, work = _same(lambda: A.search_batch(Q, k, exact=True), lambda: B.search_batch(Q, k, filter=notR, exact=True), A, B,
                                 nq, R, w + ("exact",))
        if kind == "every":
            assert (ids == -1).all() and st["expansions"] == 0 and (work == 0).all(), w
        else:
            assert ((ids >= 0).sum(axis=1) == min(k, n - int(R.sum()))).all(), w
        _same(lambda: A.search_batch(Q, k, filter=g1a), lambda: B.search_batch(Q, k, filter=g1b), A, B, nq, R, w + ("user filter",))
        _same(lambda: A.search_batch(Q, k, filter=g1a, exact=True), lambda: B.search_batch(Q, k, filter=g1b, exact=True), A, B, nq, R,
              w + ("user filter, exact",))
        _same(lambda: A.search_batch(Q, k, filter=[g1a, g2a], filter_of=fo),
              lambda: B.search_batch(Q, k, filter=[g1b, g2b, notR], filter_of=fo_b), A, B, nq, R, w + ("per query",))
        # the exact threshold is compared with the EFFECTIVE count: between the two, one filter is scanned, one walks
        c1, c2 = int((G1 & ~R).sum()), int((G2 & ~R).sum())
        A.exact_threshold = B.exact_threshold = (c1 + c2) // 2
        _same(lambda: A.search_batch(Q, k, filter=g1a), lambda: B.search_batch(Q, k, filter=g1b), A, B, nq, R, w + ("threshold g1",))
        _same(lambda: A.search_batch(Q, k, filter=g2a), lambda: B.search_batch(Q, k, filter=g2b), A, B, nq, R, w + ("threshold g2",))
        _same(lambda: A.search_batch(Q, k, filter=[g1a, g2a], filter_of=fo),
              lambda: B.search_batch(Q, k, filter=[g1b, g2b, notR], filter_of=fo_b), A, B, nq, R, w + ("threshold, per query",))
        if c1 != c2:
            lo, hi = (g1a, g2a) if c1 < c2 else (g2a, g1a)
            A.search_batch(Q, k, filter=lo)
            assert A.last_search_stats()["expansions"] == 0, w           # scanned
            A.search_batch(Q, k, filter=hi)
            assert A.last_search_stats()["expansions"] > 0, w            # walked the graph
        A.exact_threshold = B.exact_threshold = 0
        for i in (0, nq - 1):
            ai, ad = A.search(Q[i], k)
            bi, bd = B.search(Q[i], k, filter=notR)
            assert np.array_equal(ai, bi) and _beq(ad, bd), w + ("search", i)
            assert not R[ai].any(), w

        def dev(ix, **kw):
            i_, d_ = ix.search_batch_device(Qd, k, **kw)
            ix.synchronize()
            torch.cuda.synchronize()
            return i_.cpu().numpy(), d_.cpu().numpy()
        _same(lambda: dev(A), lambda: dev(B, filter=notR), A, B, nq, R, w + ("device",))
        _same(lambda: dev(A, filter=g2a), lambda: dev(B, filter=g2b), A, B, nq, R, w + ("device, user filter",))
    if (name, bits, kind) == ("g128", 4, "p10"):
        # independently of the library: the model of the filtered search under ~R
        mi = ModelIndex(fixture_path(name, bits))
        mids, md, _, mctr = mi.search_batch(Q, 10, ~R, nthreads=16)
        ids, d = A.search_batch(Q, 10)
        assert np.array_equal(ids, mids) and _beq(d, md)
        assert np.array_equal(A.last_query_expansions(nq).astype(np.uint64), mctr[:, 0])


def test_remove_state(cph, gold, tmp_path):
    name, bits = "g128", 4
    Q = gold[f"Q/{name}"]
    nq = len(Q)
    A, U, F = _load(cph, name, bits), _load(cph, name, bits), _load(cph, name, bits)
    n = A.size
    rng = np.random.default_rng(5)
    R1, R2 = rng.random(n) < 0.2, rng.random(n) < 0.2
    # remove([]) changes nothing: results, counters, the bytes of save_native
    assert A.remove([]) == 0 and A.live_count == n and not A.removed_mask().any()
    ia, da = A.search_batch(Q, 10)
    sa = _stats(A, nq)
    if_, df = F.search_batch(Q, 10)
    sf = _stats(F, nq)
    assert np.array_equal(ia, if_) and _beq(da, df) and sa[0] == sf[0] and np.array_equal(sa[1], sf[1])
    A.save_native(str(tmp_path / "a.cphn"))
    F.save_native(str(tmp_path / "f.cphn"))
    assert (tmp_path / "a.cphn").read_bytes() == (tmp_path / "f.cphn").read_bytes()
    # a filter made BEFORE the removes, used (graph and exact: the id list is cached) before them
    G = rng.random(n) < 0.6
    ga = A.make_filter(G)
    A.search_batch(Q, 10, filter=ga)
    A.search_batch(Q, 10, filter=ga, exact=True)
    # two removes = one remove of the union; again: 0; a duplicate inside one call counts once
    i1 = np.flatnonzero(R1)
    assert A.remove(np.concatenate([i1, i1[:5]])) == len(i1)
    assert A.remove(i1) == 0
    assert A.remove(np.flatnonzero(R2)) == int((R2 & ~R1).sum())
    assert U.remove(np.flatnonzero(R1 | R2)) == int((R1 | R2).sum())
    assert np.array_equal(A.removed_mask(), R1 | R2) and A.live_count == U.live_count == n - int((R1 | R2).sum())
    for kw in ({}, {"exact": True}):
        ia, da = A.search_batch(Q, 10, **kw)
        iu, du = U.search_batch(Q, 10, **kw)
        assert np.array_equal(ia, iu) and _beq(da, du), kw
    # an id of `size` (or below 0): ValueError, nothing changes
    before = A.removed_mask()
    free = np.flatnonzero(~before)[:4]
    for bad in (n, -1):
        with pytest.raises(ValueError):
            A.remove(np.concatenate([free, [bad]]))
    assert np.array_equal(A.removed_mask(), before)
    # the old filter observes the removes: graph search and exact (its cached id list is rebuilt)
    R = R1 | R2
    gf = F.make_filter(G & ~R)
    for kw in ({}, {"exact": True}):
        _same(lambda: A.search_batch(Q, 10, filter=ga, **kw), lambda: F.search_batch(Q, 10, filter=gf, **kw), A, F, nq, R, ("old filter", kw))
    # one filter, two handles with different R, in turns
    C2 = _load(cph, name, bits)
    Rc = rng.random(n) < 0.3
    C2.remove(np.flatnonzero(Rc))
    gc2 = F.make_filter(G & ~Rc)
    for turn in range(2):
        for kw in ({}, {"exact": True}):
            _same(lambda: A.search_batch(Q, 10, filter=ga, **kw), lambda: F.search_batch(Q, 10, filter=gf, **kw), A, F, nq, R, ("shared", turn, kw))
            _same(lambda: C2.search_batch(Q, 10, filter=ga, **kw), lambda: F.search_batch(Q, 10, filter=gc2, **kw), C2, F, nq, Rc, ("shared", turn, kw))


def test_remove_input_rows(cph, gold):
    name, bits = "g16", 1
    Q = gold[f"Q/{name}"]
    nq = len(Q)
    A, B = _load(cph, name, bits), _load(cph, name, bits)
    n = A.size
    rng = np.random.default_rng(9)
    perm = rng.permutation(n)
    for ix in (A, B):
        ix.set_row_map(perm)
        ix.result_ids = "input"
    mask = rng.random(n) < 0.3                         # over input rows
    assert A.remove(np.flatnonzero(mask)) == int(mask.sum())
    assert np.array_equal(A.removed_mask(ids="input"), mask)
    assert np.array_equal(A.removed_mask(), mask)      # (the default space is result_ids)
    assert np.array_equal(A.removed_mask(ids="internal"), mask[perm])
    f = B.make_filter(~mask, ids="input")
    for kw in ({}, {"exact": True}):
        _same(lambda: A.search_batch(Q, 10, **kw), lambda: B.search_batch(Q, 10, filter=f, **kw), A, B, nq, mask, kw)
    A.result_ids = "internal"                          # R is kept in internal ids whatever the handle speaks
    assert np.array_equal(A.removed_mask(), mask[perm])
    assert A.remove(np.flatnonzero(mask[perm])) == 0
    C = _load(cph, name, bits)
    with pytest.raises(ValueError):
        C.remove([1], ids="input")                     # no row map


def test_remove_more_than_one_block(cph, tmp_path):
    """8,230 ids: 258 bitmap words, two blocks of the 256-thread bitmap kernels, a partial last word."""
    rng = np.random.default_rng(77)
    n, dim = 8230, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((16, dim)).astype(np.float32)
    A = cph.CPIndex(dim, 1)
    A.build(X)
    A.finalize()
    p = str(tmp_path / "big.cphn")
    A.save_native(p)
    B = cph.CPIndex(dim, 1)
    B.load_native(p)
    R = rng.random(n) < 0.05
    R[[0, 31, 32, 8191, 8192, 8229]] = True
    assert A.remove(np.flatnonzero(R)) == int(R.sum())
    assert np.array_equal(A.removed_mask(), R) and A.live_count == n - int(R.sum())
    f = B.make_filter(~R)
    _same(lambda: A.search_batch(Q, 10, exact=True), lambda: B.search_batch(Q, 10, filter=f, exact=True), A, B, len(Q), R, "exact")
    _same(lambda: A.search_batch(Q, 10), lambda: B.search_batch(Q, 10, filter=f), A, B, len(Q), R, "graph")
    rows = rng.random(n) < 0.5                         # ... and the input-row form of the mark kernel on the same size
    A.result_ids = B.result_ids = "input"
    newly = A.remove(np.flatnonzero(rows))
    both = R | rows[A.row_map()]                       # internal ids
    assert newly == int(both.sum()) - int(R.sum())
    assert np.array_equal(A.removed_mask(ids="internal"), both)


def test_remove_files(cph, gold, tmp_path):
    name, bits = "g128", 4
    Q = gold[f"Q/{name}"]
    A = _load(cph, name, bits)
    n = A.size
    R = np.random.default_rng(3).random(n) < 0.25
    A.remove(np.flatnonzero(R))
    p = str(tmp_path / "r.cphn")
    A.save_native(p)
    C = cph.CPIndex(DATASETS[name]["dim"], bits)
    C.load_native(p)
    assert np.array_equal(C.removed_mask(), R) and C.live_count == n - int(R.sum()) and C.size == n
    for kw in ({}, {"exact": True}):
        ia, da = A.search_batch(Q, 10, **kw)
        ic, dc = C.search_batch(Q, 10, **kw)
        assert np.array_equal(ia, ic) and _beq(da, dc)
    with pytest.raises(RuntimeError, match="compact.*save_native"):
        A.save(str(tmp_path / "r.idx"))
    C.load(fixture_path(name, bits))                   # a v2 load ends R
    assert not C.removed_mask().any() and C.live_count == n
    A.compact()
    A.save(str(tmp_path / "c.idx"))                    # nothing is removed any more
    D = cph.CPIndex(DATASETS[name]["dim"], bits)
    D.load(str(tmp_path / "c.idx"))
    assert D.size == A.size == n - int(R.sum())


def test_remove_replicas(cph, gold):
    name, bits = "g128", 4
    Q = gold[f"Q/{name}"][:7]                          # a ragged shard
    S = _load(cph, name, bits)
    M = _load(cph, name, bits, devices=[0, 0])
    M.set_min_shard(1)
    n = S.size
    R = np.random.default_rng(8).random(n) < 0.3
    assert M.remove(np.flatnonzero(R)) == S.remove(np.flatnonzero(R)) == int(R.sum())
    assert np.array_equal(M.removed_mask(), R) and M.live_count == S.live_count
    G = np.random.default_rng(9).random(n) < 0.5
    gm, gs = M.make_filter(G), S.make_filter(G)
    for kw_m, kw_s in (({}, {}), ({"exact": True}, {"exact": True}), ({"filter": gm}, {"filter": gs})):
        im, dm = M.search_batch(Q, 10, **kw_m)
        is_, ds = S.search_batch(Q, 10, **kw_s)
        assert np.array_equal(im, is_) and _beq(dm, ds), kw_s
        assert not R[im[im >= 0]].any()
    for i in range(4):                                 # single queries: round robin over the replicas
        im, dm = M.search(Q[i], 10)
        is_, ds = S.search(Q[i], 10)
        assert np.array_equal(im, is_) and _beq(dm, ds)


def test_remove_parts(cph):
    rng = np.random.default_rng(21)
    n, dim = 640, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((9, dim)).astype(np.float32)
    P = cph.CPIndex(dim, 4, devices=[0, 0], partition=True)
    P.build(X)
    P.finalize()
    (lo0, hi0), (lo1, hi1) = P.parts
    R = np.zeros(n, bool)
    R[hi0 - 30:hi0 + 25] = True                        # straddles the part bound
    R[rng.choice(n, 40, replace=False)] = True
    f = P.make_filter(~R)
    want = [P.search_batch(Q, 10, filter=f, **kw) for kw in ({}, {"exact": True})]
    assert P.remove(np.flatnonzero(R)) == int(R.sum())
    assert np.array_equal(P.removed_mask(), R) and P.live_count == n - int(R.sum()) and P.size == n
    for (wi, wd), kw in zip(want, ({}, {"exact": True})):
        ids, d = P.search_batch(Q, 10, **kw)
        assert np.array_equal(ids, wi) and _beq(d, wd), kw
        assert not R[ids[ids >= 0]].any()
    with pytest.raises(ValueError):
        P.remove([n])
    P.remove(np.arange(lo1, hi1))                      # all of part 1: the rows come from part 0 only
    for kw in ({}, {"exact": True}):
        ids, d = P.search_batch(Q, 10, **kw)
        assert (ids >= 0).all() and (ids < hi0).all(), kw
    old_live = ~P.removed_mask()
    m = P.compact()
    assert P.size == P.live_count == int(old_live.sum()) and not P.removed_mask().any()
    assert (m[~old_live] == -1).all() and np.array_equal(m[old_live], np.arange(P.size))
    ids, d = P.search_batch(Q, 10, exact=True)
    got = np.flatnonzero(old_live)[ids]                # new rows -> old rows
    # fp32 squared distances of 16 unit-variance coordinates (about 32): whatever the order of the sums, two evaluations
    # differ by a few ulps of the norms involved, 2^-23 * 64 * a few < 1e-4
    d2 = ((X[got].astype(np.float64) - Q[:, None, :]) ** 2).sum(-1)
    assert np.allclose(d, d2, rtol=1e-5, atol=1e-4)


def test_compact(cph, tmp_path):
    """1,500 distinct Gaussian rows, 4-bit, 30 % removed.  The builder is reproducible: with the library of the parent
    commit, on an MI355X, six build + finalize + save_native of one 1,050 x 24 array at 4 bits gave six byte-equal
    files, and three of one 8,230 x 16 array at 1 bit three byte-equal files (profiles/remove.md).  So the compacted
    index' file is also compared with the file of a fresh build of the live rows."""
    rng = np.random.default_rng(1234)
    n, dim, k = 1500, 24, 10
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((20, dim)).astype(np.float32)
    A = cph.CPIndex(dim, 4)
    A.build(X)
    A.finalize()
    A.result_ids = "input"
    R = np.zeros(n, bool)
    R[rng.choice(n, 450, replace=False)] = True
    assert A.remove(np.flatnonzero(R)) == 450
    E, Ed = A.search_batch(Q, k, exact=True)
    assert (E >= 0).all()
    m = A.compact()
    assert A.size == A.live_count == 1050 and not A.removed_mask().any()
    assert A.result_ids == "input" and A.has_row_map
    assert m.shape == (n,) and (m[R] == -1).all() and np.array_equal(m[~R], np.arange(1050))
    live = X[~R]
    assert A.get_vectors().tobytes() == live[A.row_map()].tobytes()
    ids, d = A.search_batch(Q, k, exact=True)
    assert np.array_equal(ids, m[E]) and _beq(d, Ed)
    fresh = cph.CPIndex(dim, 4)
    fresh.build(live)
    fresh.finalize()
    A.save_native(str(tmp_path / "compacted.cphn"))
    fresh.save_native(str(tmp_path / "fresh.cphn"))
    assert (tmp_path / "compacted.cphn").read_bytes() == (tmp_path / "fresh.cphn").read_bytes()
    ids, d = A.search_batch(Q, k)                      # the rebuilt graph answers, in new input rows
    assert ((ids >= 0) & (ids < 1050)).all()
    assert A.compact().tolist() == list(range(1050))   # nothing removed: it still rebuilds
    A.save(str(tmp_path / "c.idx"))
    # fewer live rows than the builder takes: its own error, the handle as it was
    A.remove(np.arange(1010))
    with pytest.raises(RuntimeError, match="at least 50 nodes"):
        A.compact()
    assert A.size == 1050 and A.live_count == 40
    ids, d = A.search_batch(Q, k, exact=True)
    assert ((ids >= 1010)).all()
