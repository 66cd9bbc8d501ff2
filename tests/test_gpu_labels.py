"""The label column on the GPU (CPIndex.set_labels / label_filter / label_filters / `label=`).

The yardstick is the path that existed before: the expected bitmap is numpy (pack_allowed_bits of the mask), the
expected rows are what make_filter(mask) plus the existing call return -- ids and distance bytes."""
import numpy as np
import pytest

from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

FMAX = np.finfo(np.float32).max
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
NOBODY = 123456789
# (lo, hi): equality, a range, lo > hi (empty), the full range (all ones, tail bits clear), a value nobody has, two
# overlapping ranges, equality at both ends of int32
BOUNDS = [(5, 5), (-1, 1), (5, -1), (I32_MIN, I32_MAX), (NOBODY, NOBODY), (0, 5), (1, I32_MAX), (I32_MIN, I32_MIN), (I32_MAX, I32_MAX)]


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


def _labels(n, seed):
    rng = np.random.default_rng(seed)
    special = np.array([I32_MIN, -1, 0, 1, 5, I32_MAX], np.int64)
    return np.where(rng.random(n) < 0.7, special[rng.integers(0, 6, n)], rng.integers(-50, 50, n))


def _mask(L, lo, hi):
    return (L >= lo) & (L <= hi)


def _check_filters(cph, ix, L_internal, bounds, fs):
    """fs[j] against numpy and against make_filter on the same mask: every word, the count."""
    for (lo, hi), f in zip(bounds, fs):
        mask = _mask(L_internal, lo, hi)
        want = cph.index.pack_allowed_bits(mask)
        got = f.words()
        assert got.dtype == np.uint32 and np.array_equal(got, want), (lo, hi)
        assert f.count == int(mask.sum()) and f.size == ix.size, (lo, hi)
        g = ix.make_filter(mask, ids="internal")
        assert np.array_equal(g.words(), got) and g.count == f.count, (lo, hi)
        g.close()


@pytest.mark.parametrize("name,bits", [("g16", 1), ("g1024", 2), ("g2048", 1)])
def test_label_bitmaps_small(cph, name, bits):
    """n = 300, 160, 88: fewer ids than one tile of the kernel (2,048), a partial last word."""
    ix = _load(cph, name, bits)
    n = ix.size
    assert n == {"g16": 300, "g1024": 160, "g2048": 88}[name]
    L = _labels(n, n)
    ix.set_labels(L)
    assert ix.has_labels and np.array_equal(ix.labels(), L)
    lo = [b[0] for b in BOUNDS]
    hi = [b[1] for b in BOUNDS]
    fs = ix.label_filters(lo, hi)
    assert len(fs) == len(BOUNDS)
    _check_filters(cph, ix, L, BOUNDS, fs)
    assert fs[2].count == 0 and fs[4].count == 0 and fs[3].count == n
    for f in fs:
        f.close()
    singles = [ix.label_filter(lo, hi) for lo, hi in BOUNDS]
    _check_filters(cph, ix, L, BOUNDS, singles)
    eq = ix.label_filter(5)                                # one argument: equality
    _check_filters(cph, ix, L, [(5, 5)], [eq])
    vals = ix.label_filters([5, -1, NOBODY])               # one array: equality per value
    _check_filters(cph, ix, L, [(5, 5), (-1, -1), (NOBODY, NOBODY)], vals)
    assert ix.label_filters([]) == []


def test_label_bitmaps_tiles_and_filter_chunks(cph):
    """8,230 x 16 at 1 bit: 258 bitmap words, five tiles of 2,048 ids with a partial last one and a partial last word.
    The ids on every word and tile border carry a label of their own, so single-bit filters sit there.  One call makes
    146 filters: more than two of the kernel's filter chunks (kLabelFilterChunk = 64 filters per blockIdx.y), with a
    partial third.  Labels are given in input rows; every word and count must equal numpy on labels[row_map()]."""
    rng = np.random.default_rng(77)
    n, dim = 8230, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    rows = ix.row_map()
    border = [0, 31, 32, 63, 64, 2047, 2048, 4095, 4096, 8191, 8192, 8229]
    L_internal = rng.integers(0, 130, n)
    L_internal[border] = 1000 + np.arange(len(border))
    L_rows = np.empty(n, np.int64)
    L_rows[rows] = L_internal
    ix.set_labels(L_rows, ids="input")
    assert np.array_equal(ix.labels(ids="input"), L_rows) and np.array_equal(ix.labels(ids="internal"), L_internal)
    bounds = [(1000 + i, 1000 + i) for i in range(len(border))] + [(v, v) for v in range(130)]
    bounds += [(0, 64), (60, 1005), (7, 3), (I32_MIN, I32_MAX)]
    assert len(bounds) == 146 > 2 * 64
    fs = ix.label_filters([b[0] for b in bounds], [b[1] for b in bounds])
    for i, b in enumerate(border):
        w = fs[i].words()
        assert fs[i].count == 1 and w[b >> 5] == np.uint32(1 << (b & 31)) and np.count_nonzero(w) == 1, b
    _check_filters(cph, ix, L_internal, bounds, fs)
    assert sum(f.count for f in fs[len(border):len(border) + 130]) == n - len(border)      # the values partition the rest


def _dev(ix, Qd, k, **kw):
    import torch
    i_, d_ = ix.search_batch_device(Qd, k, **kw)
    ix.synchronize()
    torch.cuda.synchronize()
    return i_.cpu().numpy(), d_.cpu().numpy()


def test_label_search_parity(cph, gold):
    import torch
    name, bits, k = "g128", 4, 10
    ix = _load(cph, name, bits)
    n = ix.size
    Q = gold[f"Q/{name}"]
    nq = len(Q)
    rng = np.random.default_rng(11)
    L = rng.choice([0, 1, 2, 3], n, p=[0.6, 0.3, 0.08, 0.02])
    ix.set_labels(L)

    def same(got, want, where):
        assert np.array_equal(got[0], want[0]) and _beq(got[1], want[1]), where

    for v in (0, 3, 99):
        f = ix.make_filter(L == v)
        same(ix.search_batch(Q, k, label=v), ix.search_batch(Q, k, filter=f), ("batch", v))
        same(ix.search_batch(Q, k, label=v, exact=True), ix.search_batch(Q, k, filter=f, exact=True), ("exact", v))
        same(ix.search(Q[0], k, label=v), ix.search(Q[0], k, filter=f), ("search", v))
        Qd = torch.from_numpy(Q).to(f"cuda:{ix.devices[0]}")
        same(_dev(ix, Qd, k, label=v), _dev(ix, Qd, k, filter=f), ("device", v))
        for kw in ({"exact": True}, {"exact": False, "max_results": 20}):
            a = ix.range_search(Q, 40.0, label=v, **kw)
            b = ix.range_search(Q, 40.0, filter=f, **kw)
            assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and _beq(a[2], b[2]), ("range", v, kw)
            a = ix.range_search_device(Qd, 40.0, label=v, **kw)
            assert np.array_equal(a[0].numpy(), b[0]) and np.array_equal(a[1].cpu().numpy(), b[1]), ("range device", v, kw)
            assert _beq(a[2].cpu().numpy(), b[2]), ("range device", v, kw)
        if v == 99:
            ids, d = ix.search_batch(Q, k, label=v)
            assert (ids == -1).all() and (d == FMAX).all()
        f.close()
    # one label per query, a label without rows among them: the filter_of path
    lq = rng.choice([0, 1, 2, 3, 99], nq)
    lq[:5] = (0, 1, 2, 3, 99)
    uniq, inv = np.unique(lq, return_inverse=True)
    fl = [ix.make_filter(L == u) for u in uniq]
    counts = [f.count for f in fl]
    for thr in (0, (int((L == 2).sum()) + int((L == 1).sum())) // 2):
        ix.exact_threshold = thr
        got = ix.search_batch(Q, k, label=lq)
        same(got, ix.search_batch(Q, k, filter=fl, filter_of=inv), ("per query", thr))
        assert (got[0][lq == 99] == -1).all()
        same(ix.search_batch(Q, k, label=lq.astype(np.int16), exact=True), ix.search_batch(Q, k, filter=fl, filter_of=inv, exact=True),
             ("per query exact", thr))
        same(_dev(ix, Qd, k, label=lq), _dev(ix, Qd, k, filter=fl, filter_of=inv), ("per query device", thr))
        if thr:                                             # one call mixes scanned and graph-searched queries
            assert any(0 < c <= thr for c in counts) and any(c > thr for c in counts)
            ix.search_batch(Q, k, label=lq)
            st = ix.last_search_stats()
            work = ix.last_query_expansions(nq)
            assert st["expansions"] > 0 and (work[np.isin(lq, [2, 3])] == 0).all() and (work[np.isin(lq, [0, 1])] > 0).all()
    ix.exact_threshold = 0
    # input rows: labels, filters and results all speak rows
    perm = rng.permutation(n)
    ix.set_row_map(perm)
    ix.result_ids = "input"
    assert np.array_equal(ix.labels(), L[np.argsort(perm)])           # the column stayed with the internal ids
    L_in = rng.integers(0, 3, n)
    ix.set_labels(L_in)                                               # default space: result_ids
    assert np.array_equal(ix.labels(), L_in) and np.array_equal(ix.labels(ids="internal"), L_in[perm])
    for v in (0, 2):
        f = ix.make_filter(L_in == v)
        got = ix.search_batch(Q, k, label=v)
        same(got, ix.search_batch(Q, k, filter=f), ("input rows", v))
        assert (L_in[got[0][got[0] >= 0]] == v).all()
    lq = rng.integers(0, 3, nq)
    same(ix.search_batch(Q, k, label=lq), ix.search_batch(Q, k, filter=[ix.make_filter(L_in == u) for u in range(3)], filter_of=lq),
         "input rows, per query")


def test_labels_removed_rows_and_compact(cph, tmp_path):
    """The 1,500 x 24 shape of test_compact."""
    rng = np.random.default_rng(1234)
    n, dim, k = 1500, 24, 10
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((20, dim)).astype(np.float32)
    A = cph.CPIndex(dim, 4)
    A.build(X)
    A.finalize()
    A.result_ids = "input"
    p = str(tmp_path / "a.cphn")
    A.save_native(p)
    B = cph.CPIndex(dim, 4)                                 # the same index, never told about labels or removals
    B.load_native(p)
    B.result_ids = "input"
    L = rng.integers(0, 4, n)
    A.set_labels(L)
    R = np.zeros(n, bool)
    R[rng.choice(n, 450, replace=False)] = True
    assert A.remove(np.flatnonzero(R)) == 450
    assert A.has_labels and np.array_equal(A.labels(), L)   # a remove leaves the column
    lq = rng.integers(0, 4, len(Q))
    for v in (0, 3):
        f = B.make_filter((L == v) & ~R)
        for kw in ({}, {"exact": True}):
            a, b = A.search_batch(Q, k, label=v, **kw), B.search_batch(Q, k, filter=f, **kw)
            assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]), (v, kw)
    a = A.search_batch(Q, k, label=lq)
    b = B.search_batch(Q, k, filter=[B.make_filter((L == u) & ~R) for u in range(4)], filter_of=lq)
    assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1])
    fa = A.label_filter(1)
    assert fa.count == int((L == 1).sum())                 # the filter is the label's; the removed rows go at search time
    A.compact()
    assert A.size == 1050 and A.has_labels
    newL = L[~R]
    assert np.array_equal(A.labels(ids="input"), newL)
    assert np.array_equal(A.labels(ids="internal"), newL[A.row_map()])
    for v in range(4):
        for kw in ({}, {"exact": True}):
            ids, d = A.search_batch(Q, k, label=v, **kw)
            assert (ids >= 0).any() and (newL[ids[ids >= 0]] == v).all(), (v, kw)
        ids, d = A.search_batch(Q, k, label=v, exact=True)
        assert ((ids >= 0).sum(axis=1) == min(k, int((newL == v).sum()))).all()


def test_labels_replicas(cph, gold):
    name, bits, k = "g128", 4, 10
    Q = gold[f"Q/{name}"][:7]                               # a ragged shard
    S = _load(cph, name, bits)
    M = _load(cph, name, bits, devices=[0, 0])
    M.set_min_shard(1)
    n = S.size
    rng = np.random.default_rng(8)
    L = rng.integers(0, 5, n)
    assert not M.has_labels
    S.set_labels(L)
    M.set_labels(L)
    assert M.has_labels and np.array_equal(M.labels(), L)
    lq = rng.integers(0, 6, len(Q))                         # 5: nobody
    lq[0] = 5
    for kw in ({"label": 2}, {"label": 2, "exact": True}, {"label": lq}, {"label": lq, "exact": True}):
        im, dm = M.search_batch(Q, k, **kw)
        is_, ds = S.search_batch(Q, k, **kw)
        assert np.array_equal(im, is_) and _beq(dm, ds), kw
    fm, fs = M.label_filter(1, 3), S.label_filter(1, 3)
    assert len(fm._hs) == 2 and fm.count == fs.count == int(((L >= 1) & (L <= 3)).sum())
    assert np.array_equal(fm.words(), fs.words())
    im, dm = M.search_batch(Q, k, filter=fm)
    is_, ds = S.search_batch(Q, k, filter=S.make_filter((L >= 1) & (L <= 3)))
    assert np.array_equal(im, is_) and _beq(dm, ds)
    im, dm = M.search(Q[0], k, label=4)
    is_, ds = S.search(Q[0], k, filter=S.make_filter(L == 4))
    assert np.array_equal(im, is_) and _beq(dm, ds)
    M.load(fixture_path(name, bits))                       # a load drops the column on every replica
    assert not M.has_labels
    with pytest.raises(ValueError):
        M.search_batch(Q, k, label=1)


def test_labels_parts(cph):
    rng = np.random.default_rng(21)
    n, dim, k = 640, 16, 10
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((9, dim)).astype(np.float32)
    P = cph.CPIndex(dim, 4, devices=[0, 0], partition=True)
    P.build(X)
    P.finalize()
    assert not P.has_labels
    (lo0, hi0), (lo1, hi1) = P.parts
    L = rng.integers(3, 6, n)
    L[hi0 - 30:hi0 + 25] = 1                                # straddles the part bound
    L[lo1 + 50:lo1 + 90] = 2                                # lives in part 1 only
    P.set_labels(L)
    assert P.has_labels and np.array_equal(P.labels(), L)
    lq = rng.choice([1, 2, 4, 99], len(Q))
    lq[:4] = (1, 2, 4, 99)
    uniq, inv = np.unique(lq, return_inverse=True)
    for kw in ({}, {"exact": True}):
        for v in (1, 2):
            a = P.search_batch(Q, k, label=v, **kw)
            b = P.search_batch(Q, k, filter=P.make_filter(L == v), **kw)
            assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]), (v, kw)
            assert (L[a[0][a[0] >= 0]] == v).all()
        a = P.search_batch(Q, k, label=lq, **kw)
        b = P.search_batch(Q, k, filter=[P.make_filter(L == u) for u in uniq], filter_of=inv, **kw)
        assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]), kw
    ids, d = P.search_batch(Q, k, label=2, exact=True)
    assert (ids >= lo1).all()
    a, b = P.search(Q[0], k, label=1), P.search(Q[0], k, filter=P.make_filter(L == 1))
    assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1])
    f = P.label_filter(1, 2)
    assert f.count == int(((L >= 1) & (L <= 2)).sum()) and f.size == n
    with pytest.raises(ValueError):
        f.words()
    with pytest.raises(ValueError):
        P.set_labels(L[:-1])
    R = np.zeros(n, bool)
    R[rng.choice(n, 60, replace=False)] = True
    R[hi0 - 5:hi0 + 5] = True
    P.remove(np.flatnonzero(R))
    a = P.search_batch(Q, k, label=1)
    b = P.search_batch(Q, k, filter=P.make_filter(L == 1))  # (the removed rows go from both)
    assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]) and not R[a[0][a[0] >= 0]].any()
    P.compact()
    newL = L[~R]
    assert P.size == len(newL) and P.has_labels and np.array_equal(P.labels(), newL)      # cut again at the new bounds
    for v in (1, 2):
        ids, d = P.search_batch(Q, k, label=v, exact=True)
        assert (ids >= 0).any() and (newL[ids[ids >= 0]] == v).all()
    P.build(X)
    P.finalize()
    assert not P.has_labels


def test_labels_lifecycle_and_errors(cph, gold, tmp_path):
    name, bits, k = "g16", 1, 5
    Q = gold[f"Q/{name}"]
    ix = _load(cph, name, bits)
    n = ix.size
    assert not ix.has_labels
    with pytest.raises(ValueError):
        ix.search_batch(Q, k, label=1)                      # no column
    with pytest.raises(ValueError):
        ix.label_filter(1)
    with pytest.raises(ValueError):
        ix.labels()
    plain = tmp_path / "plain.cphn"
    ix.save_native(str(plain))
    L = np.arange(n) % 7
    ix.set_labels(L.astype(np.uint8))                       # any integer width
    assert ix.has_labels and ix.labels().dtype == np.int32 and np.array_equal(ix.labels(), L)
    with_col = tmp_path / "labels.cphn"
    ix.save_native(str(with_col))
    assert with_col.read_bytes() == plain.read_bytes()      # no file carries the column
    # a filter made before a second set_labels keeps its bits
    f = ix.label_filter(3)
    before = f.words()
    assert np.array_equal(before, cph.index.pack_allowed_bits(L == 3))
    ix.set_labels((L + 1).astype(np.int64))
    assert np.array_equal(f.words(), before) and f.count == int((L == 3).sum())
    assert np.array_equal(ix.label_filter(4).words(), before)
    # the ValueErrors
    with pytest.raises(ValueError):
        ix.search_batch(Q, k, label=1, filter=f)
    with pytest.raises(ValueError):
        ix.search_batch(Q, k, label=1, filter=[f], filter_of=np.zeros(len(Q), np.int32))
    with pytest.raises(ValueError):
        ix.search_batch(Q, k, label=np.zeros(len(Q) + 1, np.int32))
    with pytest.raises(ValueError):
        ix.search(Q[0], k, label=np.zeros(1, np.int32))     # a label array on a one-query search
    with pytest.raises(ValueError):
        ix.range_search(Q, 1.0, label=np.zeros(len(Q), np.int32))
    with pytest.raises(ValueError):
        ix.search_batch(Q, k, label=2 ** 31)                # does not fit int32
    with pytest.raises(ValueError):
        ix.search_batch(Q, k, label=1.5)
    with pytest.raises(ValueError):
        ix.set_labels(np.full(n, 2 ** 31, np.int64))
    with pytest.raises(ValueError):
        ix.set_labels(np.zeros(n, np.float32))
    with pytest.raises(ValueError):
        ix.set_labels(L[:-1])
    with pytest.raises(ValueError):
        ix.set_labels(L, ids="input")                       # no row map
    with pytest.raises(ValueError):
        ix.label_filters([1, 2], [3])
    assert np.array_equal(ix.labels(), L + 1)               # none of them changed the column
    ix.set_labels(None)
    assert not ix.has_labels
    ix.set_labels(L)
    ix.load_native(str(with_col))
    assert not ix.has_labels
    ix.set_labels(L)
    ix.load(fixture_path(name, bits))
    assert not ix.has_labels
    ix.set_labels(L)
    X = np.random.default_rng(4).standard_normal((200, DATASETS[name]["dim"])).astype(np.float32)
    ix.build(X)
    assert not ix.has_labels
    with pytest.raises(ValueError):
        ix.set_labels(np.zeros(200, np.int32))              # not finalized
    ix.finalize()
    assert not ix.has_labels
    ix.set_labels(np.zeros(200, np.int32), ids="input")     # a built index has a row map
    assert ix.has_labels
