"""Tag columns on the GPU (CPIndex.set_tags / tags / tag_filter / tag_filters / where on a tag column).

The yardstick is the numpy model (tests/tags_model.py: canonicalise, count with np.isin and np.add.reduceat, compare by
mode, pack_allowed_bits) and the path that existed before: make_filter(mask) plus the existing call -- ids and distance
bytes."""
import numpy as np
import pytest

import tags_model as tm
from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

TILE = 256                            # csrc/device_tags.h: kTagTile, rows per wave
LDS_TAGS = 3072                       # kTagLdsTags: a tile with more tags than this is read from global memory
CHUNK = 64                            # kTagFilterChunk
VOCAB = np.array([tm.I32_MIN, -1, 0, tm.I32_MAX] + list(range(3, 15)), np.int64)      # 12 plus the four special tags


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


def _rows(n, seed, max_len=9, messy=True):
    """Rows as a caller gives them: lengths 0..max_len from VOCAB, and (messy) duplicates in any order on top."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        r = rng.choice(VOCAB, rng.integers(0, max_len + 1), replace=False)
        rows.append(np.concatenate([r, r[:rng.integers(0, 3)]]) if messy else r)
    return rows


def _all_kinds():
    ts = [tm.test_kinds(VOCAB, j) for j in range(24)]
    return [t for t, _ in ts], [m for _, m in ts]


def _check(cph, ix, lims, tags, tests, modes, fs, mk=True):
    """fs[j] against the model on the canonical column (internal ids) and against make_filter on the same mask."""
    assert len(fs) == len(tests)
    words, counts = tm.expect(lims, tags, tests, modes)
    for j, f in enumerate(fs):
        got = f.words()
        assert got.dtype == np.uint32 and np.array_equal(got, words[j]), (j, tests[j], modes[j])
        assert f.count == int(counts[j]) and f.size == ix.size, (j, tests[j], modes[j])
        if mk:
            g = ix.make_filter(tm.allowed(lims, tags, tests[j], modes[j]), ids="internal")
            assert np.array_equal(g.words(), got) and g.count == f.count, (j, tests[j], modes[j])
            g.close()


def _same_csr(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name,bits", [("g16", 1), ("g1024", 2), ("g2048", 1)])
def test_tag_bitmaps_small(cph, name, bits):
    """n = 300, 160, 88: fewer rows than one block's tiles, a partial last word.  Every test kind in every mode, in
    one call and as single calls; tags() in both id spaces."""
    ix = _load(cph, name, bits)
    n = ix.size
    assert n == {"g16": 300, "g1024": 160, "g2048": 88}[name]
    rows = _rows(n, n)
    assert ix.tag_columns == []
    ix.set_tags("t", rows)
    assert ix.tag_columns == ["t"]
    lims, tags = tm.canonical(*tm.to_csr(rows))
    got = ix.tags("t")
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and _same_csr(got, (lims, tags))
    tests, modes = _all_kinds()
    fs = ix.tag_filters("t", tests, modes)
    _check(cph, ix, lims, tags, tests, modes, fs)
    for t, m in zip(tests, modes):
        _check(cph, ix, lims, tags, [t], [m], [ix.tag_filter("t", t, m)])
    _check(cph, ix, lims, tags, [[5], [5, 7]], ["any", "any"], ix.tag_filters("t", [5, [7, 5, 5]]))      # an int: has this tag
    _check(cph, ix, lims, tags, [[5, 7]] * 2, ["all", "none"], ix.tag_filters("t", [[5, 7]] * 2, ["all", "none"]))
    assert ix.tag_filters("t", []) == []
    with pytest.raises(ValueError):
        ix.tag_filters("t", [list(range(65))])
    with pytest.raises(ValueError):
        ix.tag_filters("t", [1], "some")
    with pytest.raises(ValueError):
        ix.tag_filters("nope", [1])
    # the flat form, and both id spaces: input row perm[i] holds what internal id i holds
    flat_l, flat_t = tm.to_csr(rows)
    ix.set_tags("t", flat_t, lims=flat_l)
    assert _same_csr(ix.tags("t"), (lims, tags))
    perm = np.random.default_rng(n + 1).permutation(n)
    ix.set_row_map(perm)
    by_row = tm.canonical(flat_l, flat_t, np.argsort(perm))
    assert _same_csr(ix.tags("t", ids="input"), by_row) and _same_csr(ix.tags("t", ids="internal"), (lims, tags))
    ix.set_tags("t", [rows[i] for i in np.argsort(perm)], ids="input")
    assert _same_csr(ix.tags("t", ids="internal"), (lims, tags))


def test_tag_bitmaps_tiles_chunks_and_long_rows(cph):
    """8,230 x 16 at 1 bit: 258 bitmap words, 33 tiles of 256 rows with a partial last one and a partial last word.  The
    ids on every word and tile border carry a tag of their own, so single-bit filters sit there.  Rows of exactly 1,024
    tags -- two adjacent ones, and the last row with the two before it, so that the partial last tile is one of them --
    push their tiles past the LDS budget onto the global path; 200 empty rows in a run.  One call makes 146 filters: two
    filter chunks and a partial third, all modes.  Tags are given in input rows; every word and count must equal the
    model on the tags gathered through row_map()."""
    rng = np.random.default_rng(78)
    n, dim = 8230, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    rmap = ix.row_map()
    border = sorted(set([0, 31, 32, 63, 64, 2047, 2048, 4095, 4096, 8191, 8192, 8229] + list(range(0, n, TILE))))
    assert len(border) == 41
    internal = _rows(n, 5, max_len=11, messy=False)
    for i, b in enumerate(border):
        internal[b] = np.append(internal[b], 1000 + i)
    long_rows = (1000, 1001, n - 3, n - 2, n - 1)
    for r in long_rows:                                                       # exactly 1,024 distinct tags each
        keep = internal[r][internal[r] >= 1000]
        internal[r] = np.concatenate([keep, 20000 + r + np.arange(1024 - len(keep))])
    for r in range(3073, 3273):
        internal[r] = np.zeros(0, np.int64)
    assert not set(range(3073, 3273)) & set(border)
    by_row = [None] * n
    for i in range(n):
        by_row[rmap[i]] = rng.permutation(internal[i])                        # unsorted on the way in
    ix.set_tags("t", by_row, ids="input")
    lims, tags = tm.canonical(*tm.to_csr(internal))
    lens = np.diff(lims)
    assert lens.max() == 1024 and (lens == 1024).sum() == 5 and lens[:1000].max() <= 12
    spans = [lims[min(t + TILE, n)] - lims[t] for t in range(0, n, TILE)]
    assert sum(s > LDS_TAGS + 4 for s in spans) == 2 and spans[-1] > LDS_TAGS + 4                          # the global path, twice
    assert sum(0 < s <= LDS_TAGS for s in spans) == len(spans) - 2                                           # the staged path
    assert _same_csr(ix.tags("t", ids="internal"), (lims, tags))
    tests = [[1000 + i] for i in range(len(border))]
    modes = ["any"] * len(border)
    for j in range(146 - len(border)):
        t, m = tm.test_kinds(VOCAB, j)
        tests.append(t)
        modes.append(m)
    tests[-1], modes[-1] = [20000 + 1000 + 5, 20000 + 1001 + 5], "all"         # only the two adjacent long rows hold both
    assert len(tests) == 146 > 2 * CHUNK and len(tests) % CHUNK
    fs = ix.tag_filters("t", tests, modes)
    for i, b in enumerate(border):
        w = fs[i].words()
        assert fs[i].count == 1 and w[b >> 5] == np.uint32(1 << (b & 31)) and np.count_nonzero(w) == 1, b
    _check(cph, ix, lims, tags, tests, modes, fs, mk=False)
    assert fs[-1].count == 2


def test_tag_degenerate_columns(cph):
    ix = _load(cph, "g16", 1)
    n = ix.size
    assert n % 32
    ix.set_tags("t", [[]] * n)
    lims, tags = tm.to_csr([[]] * n)
    assert _same_csr(ix.tags("t"), (lims, tags))
    fs = ix.tag_filters("t", [[5], [5], [5], []], ["any", "none", "all", "all"])
    _check(cph, ix, lims, tags, [[5], [5], [5], []], ["any", "none", "all", "all"], fs)
    assert [f.count for f in fs] == [0, n, 0, n]
    assert fs[1].words()[-1] == np.uint32((1 << (n & 31)) - 1)               # clean tail bits
    ix.set_tags("t", np.full(n, 7), lims=np.arange(n + 1))                    # one tag shared by every row
    lims, tags = tm.to_csr([[7]] * n)
    fs = ix.tag_filters("t", [7, 7, [7, 8], [7, 8], 8], ["any", "none", "all", "any", "none"])
    _check(cph, ix, lims, tags, [[7], [7], [7, 8], [7, 8], [8]], ["any", "none", "all", "any", "none"], fs)
    assert [f.count for f in fs] == [n, 0, 0, n, n]


def _dev(ix, Qd, k, **kw):
    import torch
    i_, d_ = ix.search_batch_device(Qd, k, **kw)
    ix.synchronize()
    torch.cuda.synchronize()
    return i_.cpu().numpy(), d_.cpu().numpy()


def test_tag_search_parity(cph, gold):
    import torch
    name, bits, k = "g128", 4, 10
    ix = _load(cph, name, bits)
    n = ix.size
    Q = gold[f"Q/{name}"]
    nq = len(Q)
    rows = _rows(n, 12, max_len=4)
    ix.set_tags("acl", rows)
    lims, tags = tm.canonical(*tm.to_csr(rows))
    Qd = torch.from_numpy(Q).to(f"cuda:{ix.devices[0]}")

    def same(got, want, where):
        assert np.array_equal(got[0], want[0]) and _beq(got[1], want[1]), where

    def compare(where):
        for t, m in (([5], "any"), ([5, 7, 9], "all"), ([3, 4, -1], "none")):
            mask = tm.allowed(lims, tags, t, m)
            f, g = ix.tag_filter("acl", t, m), ix.make_filter(mask, ids="internal")
            same(ix.search_batch(Q, k, filter=f), ix.search_batch(Q, k, filter=g), (where, "batch", t, m))
            same(ix.search_batch(Q, k, filter=f, exact=True), ix.search_batch(Q, k, filter=g, exact=True), (where, "exact", t, m))
            same(_dev(ix, Qd, k, filter=f), _dev(ix, Qd, k, filter=g), (where, "device", t, m))
            a, b = ix.range_search(Q, 40.0, filter=f, exact=True), ix.range_search(Q, 40.0, filter=g, exact=True)
            assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and _beq(a[2], b[2]), (where, "range", t, m)
        # per-query permissions: five users' group sets, one filter each, filter_of says whose query it is
        groups = [[5], [7, 9], [tm.I32_MIN, tm.I32_MAX], [tm.NOBODY], [3, 4, 5, 6]]
        which = np.random.default_rng(3).integers(0, 5, nq)
        which[:5] = np.arange(5)
        fs = ix.tag_filters("acl", groups)
        gs = [ix.make_filter(tm.allowed(lims, tags, g, "any"), ids="internal") for g in groups]
        got = ix.search_batch(Q, k, filter=fs, filter_of=which)
        same(got, ix.search_batch(Q, k, filter=gs, filter_of=which), (where, "per query"))
        assert (got[0][which == 3] == -1).all()
        return fs, gs, which

    compare("whole")
    fs, gs, which = compare("again")
    gone = np.random.default_rng(4).choice(n, n // 5, replace=False)
    assert ix.remove(gone) == len(gone)
    got = ix.search_batch(Q, k, filter=fs, filter_of=which)                  # filters made before the remove observe it
    same(got, ix.search_batch(Q, k, filter=gs, filter_of=which), "removed, per query")
    assert not np.isin(got[0][got[0] >= 0], gone).any() and (got[0] >= 0).any()
    assert fs[0].count == gs[0].count                                         # the filter is the tag's; the rows go at search time
    compare("removed")


def test_tag_where(cph):
    ix = _load(cph, "g128", 4)
    n = ix.size
    rng = np.random.default_rng(9)
    rows = _rows(n, 13, max_len=5)
    year, label = rng.integers(1990, 2025, n), rng.integers(0, 5, n)
    ix.set_tags("acl", rows)
    ix.set_column("year", year)
    ix.set_labels(label)
    lims, tags = tm.canonical(*tm.to_csr(rows))
    f = ix.where(acl={"any": [5, 7, 9]}, year=(1995, 2015), label=3)
    mask = tm.allowed(lims, tags, [5, 7, 9], "any") & (year >= 1995) & (year <= 2015) & (label == 3)
    assert np.array_equal(f.words(), cph.index.pack_allowed_bits(mask)) and f.count == int(mask.sum()) and 0 < f.count < n
    for t, want in ((7, ([7], "any")), ({"all": [5, 7]}, ([5, 7], "all")), ({"none": (5, 7)}, ([5, 7], "none")), ({"any": []}, ([], "any"))):
        g = ix.where(acl=t)
        m2 = tm.allowed(lims, tags, *want)
        assert np.array_equal(g.words(), cph.index.pack_allowed_bits(m2)) and g.count == int(m2.sum()), t
    for bad in ((5, 7), [5, 7], {"any": [5], "all": [7]}, {"some": [5]}, {}):
        with pytest.raises(ValueError):
            ix.where(acl=bad)


def test_tag_lifecycle(cph, tmp_path):
    rng = np.random.default_rng(31)
    n, dim = 600, DATASETS["g16"]["dim"]
    X = rng.standard_normal((n, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    ix.result_ids = "input"
    rows = _rows(n, 14)
    rows[7] = np.arange(1024) - 500                                           # a long row travels too
    ix.set_tags("acl", rows)                                                  # (default space: result_ids = input rows)
    old = tm.rows_of(*tm.canonical(*tm.to_csr(rows)))
    assert _same_csr(ix.tags("acl"), tm.to_csr(old))
    # one namespace with the attribute columns
    with pytest.raises(ValueError):
        ix.set_column("acl", np.zeros(n, np.int32))
    ix.set_column("year", np.zeros(n, np.int32))
    with pytest.raises(ValueError):
        ix.set_tags("year", rows)
    with pytest.raises(ValueError):
        ix.set_tags("label", rows)
    ix.set_column("year", None)
    # slots: four columns, a fifth raises, a dropped one frees its slot
    for name in ("b", "c", "d"):
        ix.set_tags(name, [[1]] * n)
    assert sorted(ix.tag_columns) == ["acl", "b", "c", "d"]
    with pytest.raises(ValueError):
        ix.set_tags("e", [[1]] * n)
    ix.set_tags("c", None)
    ix.set_tags("e", [[2]] * n)
    assert sorted(ix.tag_columns) == ["acl", "b", "d", "e"] and ix.tag_filter("e", 2).count == n
    with pytest.raises(ValueError):
        ix.tags("c")
    for name in ("b", "d", "e"):
        ix.set_tags(name, None)
    # refusals leave the column as it is
    with pytest.raises(ValueError):
        ix.set_tags("acl", rows[:-1])
    with pytest.raises(ValueError):
        ix.set_tags("acl", [list(range(1025))] + rows[1:])
    with pytest.raises(ValueError):
        ix.set_tags("acl", [[2 ** 31]] + rows[1:])
    with pytest.raises(ValueError):
        ix.set_tags("acl", [1, 2], lims=[0, 2, 1] + [2] * (n - 2))
    assert _same_csr(ix.tags("acl"), tm.to_csr(old))
    with pytest.raises(ValueError):
        ix.add(X[:3])                                                         # the new rows would have no tags
    # compact carries the column
    gone = rng.choice(n, n // 3, replace=False)
    gone = gone[gone != 7]
    ix.remove(gone)
    assert _same_csr(ix.tags("acl"), tm.to_csr(old))                          # a remove leaves the column
    old_to_new = ix.compact()
    live = np.flatnonzero(old_to_new >= 0)
    assert ix.size == len(live) == n - len(gone) and ix.tag_columns == ["acl"]
    new = [None] * len(live)
    for r in live:
        new[old_to_new[r]] = old[r]
    assert _same_csr(ix.tags("acl", ids="input"), tm.to_csr(new))
    lims, tags = ix.tags("acl", ids="internal")
    assert _same_csr((lims, tags), tm.canonical(*tm.to_csr(new), ix.row_map()))
    tests, modes = _all_kinds()
    _check(cph, ix, lims, tags, tests, modes, ix.tag_filters("acl", tests, modes))
    # a load drops the column and its name
    p = str(tmp_path / "a.cphn")
    ix.save_native(p)
    ix.load_native(p)
    assert ix.tag_columns == []
    with pytest.raises(ValueError):
        ix.tag_filter("acl", 5)
    ix.set_tags("acl", new, ids="input")
    ix.load(fixture_path("g16", 1))
    assert ix.tag_columns == [] and ix.size == 300
    ix.set_tags("acl", [[1]] * 300)
    ix.build(X)
    assert ix.tag_columns == []


def test_tags_replicas(cph, gold):
    name, bits, k = "g128", 4, 10
    Q = gold[f"Q/{name}"][:7]
    S = _load(cph, name, bits)
    M = _load(cph, name, bits, devices=[0, 0])
    M.set_min_shard(1)
    n = S.size
    rows = _rows(n, 15, max_len=4)
    S.set_tags("acl", rows)
    M.set_tags("acl", rows)
    assert M.tag_columns == ["acl"] and _same_csr(M.tags("acl"), S.tags("acl"))
    tests, modes = _all_kinds()
    fm, fs = M.tag_filters("acl", tests, modes), S.tag_filters("acl", tests, modes)
    for a, b in zip(fm, fs):
        assert len(a._hs) == 2 and a.count == b.count and np.array_equal(a.words(), b.words())
    which = np.arange(len(Q)) % 3
    for kw in ({}, {"exact": True}):
        a, b = M.search_batch(Q, k, filter=fm[0], **kw), S.search_batch(Q, k, filter=fs[0], **kw)
        assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]), kw
        a, b = M.search_batch(Q, k, filter=fm[:3], filter_of=which, **kw), S.search_batch(Q, k, filter=fs[:3], filter_of=which, **kw)
        assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]), kw
    M.load(fixture_path(name, bits))                                          # a load drops the column on every replica
    assert M.tag_columns == []


def test_tags_parts(cph):
    rng = np.random.default_rng(22)
    n, dim, k = 640, 16, 10
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((9, dim)).astype(np.float32)
    P = cph.CPIndex(dim, 4, devices=[0, 0], partition=True)
    P.build(X)
    P.finalize()
    S = cph.CPIndex(dim, 4)
    S.build(X)
    S.finalize()
    S.result_ids = "input"
    (lo0, hi0), (lo1, hi1) = P.parts
    rows = _rows(n, 16, max_len=4)
    for r in range(hi0 - 30, hi0 + 25):
        rows[r] = np.array([100, 5])                                          # straddles the part bound
    for r in range(lo1 + 50, lo1 + 90):
        rows[r] = np.array([200])                                             # lives in part 1 only
    P.set_tags("acl", rows)                                                   # global input rows
    lims, tags = tm.canonical(*tm.to_csr(rows))
    assert P.tag_columns == ["acl"] and _same_csr(P.tags("acl"), (lims, tags))
    tests = [[100], [200], [100, 5], [100, 200], [100, 200], [tm.NOBODY], []]
    modes = ["any", "any", "all", "none", "any", "any", "all"]
    fs = P.tag_filters("acl", tests, modes)
    for t, m, f in zip(tests, modes, fs):
        mask = tm.allowed(lims, tags, t, m)
        assert f.count == int(mask.sum()) and f.size == n, (t, m)
        for kw in ({}, {"exact": True}):
            a = P.search_batch(Q, k, filter=f, **kw)
            b = P.search_batch(Q, k, filter=P.make_filter(mask), **kw)
            assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]), (t, m, kw)
        a = P.search_batch(Q, k, filter=f, exact=True)                        # the exact scan: the single index says the same
        b = S.search_batch(Q, k, filter=S.make_filter(mask), exact=True)
        assert np.array_equal(a[0], b[0]), (t, m)
    with pytest.raises(ValueError):
        P.set_tags("acl", rows[:-1])
    gone = rng.choice(n, 60, replace=False)
    P.remove(gone)
    old_to_new = P.compact()
    live = np.flatnonzero(old_to_new >= 0)
    canon = tm.rows_of(lims, tags)
    new = [None] * len(live)
    for r in live:
        new[old_to_new[r]] = canon[r]
    assert P.size == len(live) and P.tag_columns == ["acl"] and _same_csr(P.tags("acl"), tm.to_csr(new))      # cut again at the new bounds
    nl, nt = tm.to_csr(new)
    f = P.tag_filter("acl", [100, 200])
    assert f.count == int(tm.allowed(nl, nt, [100, 200], "any").sum())
    P.build(X)
    P.finalize()
    assert P.tag_columns == []
