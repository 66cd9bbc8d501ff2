"""Facet counts on the GPU (CPIndex.facet / prepare_facets; cph_facet_*; csrc/device_facets.h).

The yardstick is the numpy model (tests/facet_model.py) on the column in internal-id order, and, where it applies, the
path that existed before: (filter & label_filter(v)).count.  Everything is integers: every comparison is exact equality."""
import ctypes as C

import numpy as np
import pytest

import facet_model as fm
from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = fm.I32_MIN, fm.I32_MAX
A5 = 0xA5A5A5A5A5A5A5A5
PATH_AUTO, PATH_ONCHIP, PATH_GLOBAL = 0, 1, 2


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


@pytest.fixture(scope="module")
def lib():
    from cphnsw_mi355x import _lib
    return _lib


def _load(cph, name, bits, **kw):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits, **kw)
    ix.load(fixture_path(name, bits))
    return ix


def _labels(n, seed):
    rng = np.random.default_rng(seed)
    special = np.array([I32_MIN, -1, 0, 1, 5, I32_MAX], np.int64)
    return np.where(rng.random(n) < 0.7, special[rng.integers(0, 6, n)], rng.integers(-50, 50, n))


def _tag_rows(n, seed, vocab=12):
    rng = np.random.default_rng(seed)
    rows = [rng.choice(vocab, rng.integers(0, 5), replace=False) - 3 for _ in range(n)]
    if n:
        rows[0] = np.array([I32_MIN, I32_MAX, 4])
        rows[n // 2] = np.zeros(0, np.int64)
    return rows


def _csr(rows):
    lims = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=lims[1:])
    flat = np.concatenate([np.sort(np.asarray(r, np.int64)) for r in rows]) if rows else np.zeros(0, np.int64)
    return lims, flat


def _masks(n, m, seed):
    """m masks in rotation: None, all ones, empty, single bits on word borders, random."""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(m):
        kind = (j + seed) % 5
        if kind == 0:
            out.append(None)
            continue
        mk = np.zeros(n, bool)
        if kind == 1:
            mk[:] = True
        elif kind == 3:
            bits = [b for b in (0, 31, 32, 63, 64, n - 1) if b < n]
            mk[bits[j % len(bits)]] = True
        elif kind == 4:
            mk = rng.random(n) < rng.choice([0.05, 0.5, 0.9])
        out.append(mk)
    return out


def _filters(ix, masks):
    return [None if mk is None else ix.make_filter(mk, ids="internal") for mk in masks]


def _close(fs):
    for f in fs:
        if f is not None:
            f.close()


@pytest.mark.parametrize("name,bits", [("g16", 1), ("g1024", 2), ("g2048", 1)])
def test_facets_small(cph, name, bits):
    """n = 300, 160, 88: fewer rows than one workgroup's run (8,192 ids), a partial last word.  The label column, a named
    column and a tag column; filters None / all ones / empty / single bit / random; m = 1, 3 and 70."""
    ix = _load(cph, name, bits)
    n = ix.size
    assert n == {"g16": 300, "g1024": 160, "g2048": 88}[name]
    L = _labels(n, n)
    Y = np.random.default_rng(n).integers(1990, 2000, n)
    rows = _tag_rows(n, n)
    ix.set_labels(L)
    ix.set_column("year", Y)
    ix.set_tags("acl", rows)
    lims, flat = _csr(rows)
    cols = {"label": (L, None), "year": (Y, None), "acl": (flat, lims)}
    for col, (data, cl) in cols.items():
        values, counts = ix.facet(col)                                       # all live rows, no bitmap
        ev, ec = fm.counts(data, [None], None, cl)
        assert values.dtype == np.int32 and counts.dtype == np.int64 and counts.shape == (len(ev),)
        assert np.array_equal(values, ev) and np.array_equal(counts, ec[0]), col
        v0, c0 = ix.facet(col, filter=[])
        assert np.array_equal(v0, ev) and c0.shape == (0, len(ev))
        for m in (1, 3, 70):
            masks = _masks(n, m, n + m)
            fs = _filters(ix, masks)
            values, counts = ix.facet(col, filter=fs)
            ev, ec = fm.counts(data, masks, None, cl)
            assert counts.shape == (m, len(ev)) and np.array_equal(values, ev) and np.array_equal(counts, ec), (col, m)
            if cl is None:                                                   # single-valued: the counts partition the filter
                want = [n if f is None else f.count for f in fs]
                assert counts.sum(axis=1).tolist() == want, (col, m)
            if col == "label":                                               # against the path that existed before
                for v in np.random.default_rng(m).choice(ev, 6):
                    lf = ix.label_filter(int(v))
                    u = int(np.searchsorted(ev, v))
                    for j, f in enumerate(fs):
                        g = lf if f is None else f & lf
                        assert counts[j][u] == g.count, (v, j)
                        if g is not lf:
                            g.close()
                    lf.close()
            one = ix.facet(col, filter=fs[0])                                # a single filter: 1-D
            assert np.array_equal(one[1], ec[0])
            _close(fs)
        mk = np.random.default_rng(5).random(n) < 0.5                        # anything make_filter accepts, made and freed per call
        assert np.array_equal(ix.facet(col, filter=mk)[1], fm.counts(data, [mk], None, cl)[1][0])


@pytest.fixture(scope="module")
def built(cph):
    """The 8,230 x 16, 1-bit index of test_gpu_labels: 258 bitmap words, two tiles of 8,192 ids with a partial last word."""
    rng = np.random.default_rng(77)
    n, dim = 8230, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    border = [0, 31, 32, 63, 64, 2047, 2048, 4095, 4096, 8191, 8192, 8229]
    L = rng.integers(0, 130, n)
    L[border] = 1000 + np.arange(len(border))
    ix.set_labels(L, ids="internal")
    ix.set_column("one", np.full(n, 42), ids="internal")
    uniq = rng.permutation(n).astype(np.int64) * 7 - 20000
    ix.set_column("uniq", uniq, ids="internal")
    return ix, L, uniq, border


def test_facets_word_borders_filter_chunks_and_both_paths(built):
    """Ids on every word and run border carry a value of their own; 146 filters in one call (more than nine chunks of 16);
    U = 1 under the all-ones filter is the most contended bin; the all-distinct column has U = 8,230 values, above the
    on-chip limit, so the product itself takes the global path."""
    ix, L, uniq, border = built
    n = ix.size
    bounds = [(1000 + i, 1000 + i) for i in range(len(border))] + [(v, v) for v in range(130)]
    bounds += [(0, 64), (60, 1005), (7, 3), (I32_MIN, I32_MAX)]
    assert len(bounds) == 146
    fs = ix.label_filters([b[0] for b in bounds], [b[1] for b in bounds])
    masks = [(L >= lo) & (L <= hi) for lo, hi in bounds]
    values, counts = ix.facet("label", filter=fs)
    ev, ec = fm.counts(L, masks)
    assert np.array_equal(values, ev) and np.array_equal(counts, ec)
    for i in range(len(border)):                                             # one row, one value, one count
        assert counts[i].sum() == 1 and counts[i][np.searchsorted(ev, 1000 + i)] == 1
    v1, c1 = ix.facet("one", filter=fs)
    assert v1.tolist() == [42] and c1[:, 0].tolist() == [f.count for f in fs] and c1[145, 0] == n
    assert ix.facet("one")[1].tolist() == [n]
    vu, cu = ix.facet("uniq", filter=fs[130:])
    eu, ecu = fm.counts(uniq, masks[130:])
    assert len(vu) == n and np.array_equal(vu, eu) and np.array_equal(cu, ecu) and cu.max() == 1
    assert np.array_equal(ix.facet("uniq")[1], np.ones(n, np.int64))
    _close(fs)


def _hook(lib, codes, n, U, words, m, path, lims=None):
    """cph_facet_hook -> (counts int [m, U], guard words): the 0xA5 pre-fill gone from every counter, untouched behind."""
    L = lib.lib()
    G = 64                                                                   # CPH_FACET_HOOK_GUARD
    codes = np.ascontiguousarray(codes, np.uint32)
    out = np.zeros(m * U + G, np.uint64)
    w = None if words is None else np.ascontiguousarray(words, np.uint32)
    l32 = None if lims is None else np.ascontiguousarray(lims, np.uint32)
    us = C.c_double(-1.0)
    lib.check(L.cph_facet_hook(0, codes.ctypes.data if codes.size else None, codes.size, None if l32 is None else l32.ctypes.data, n, U,
                               None if w is None or not w.size else w.ctypes.data, m, path, out.ctypes.data, C.byref(us)))
    assert us.value >= 0
    assert (out[m * U:] == A5).all(), "the launcher wrote behind its output"
    assert not (out[:m * U] == A5).any(), "a counter kept its pre-fill"
    return out[:m * U].reshape(m, U).astype(np.int64)


def test_hook_both_paths_and_their_crossover(lib):
    """U one below, at and one above the on-chip bin limit (read from the library), n the smallest that holds that many
    values plus 33; the launcher's own choice and the forced opposite path give the same counters.  Above the limit the
    opposite path is the on-chip one, which cannot hold the bins: it is refused and leaves the output untouched."""
    LIM = lib.lib().cph_facet_onchip_limit()
    assert LIM >= 64
    for U in (LIM - 1, LIM, LIM + 1):
        n = U + 33
        rng = np.random.default_rng(U)
        codes = np.concatenate([rng.permutation(U), rng.integers(0, U, 33)])
        nw = (n + 31) // 32
        dirty = np.ones(nw * 32, bool)                                       # all ones, the bits behind n too
        rnd = np.zeros(nw * 32, bool)
        rnd[:n] = rng.random(n) < 0.5
        masks = [dirty[:n], rnd[:n], np.zeros(n, bool)]
        words = np.stack([fm.pack(dirty), fm.pack(rnd), np.zeros(nw, np.uint32)])
        want = np.stack([np.bincount(codes[mk], minlength=U) for mk in masks])
        auto = _hook(lib, codes, n, U, words, 3, PATH_AUTO)
        assert np.array_equal(auto, want), U
        assert np.array_equal(_hook(lib, codes, n, U, words, 3, PATH_GLOBAL), want), U
        if U <= LIM:
            assert np.array_equal(_hook(lib, codes, n, U, words, 3, PATH_ONCHIP), want), U
        else:
            out = np.full(3 * U + 64, 7, np.uint64)
            c32, w32 = codes.astype(np.uint32), np.ascontiguousarray(words, np.uint32)
            with pytest.raises(ValueError):
                lib.check(lib.lib().cph_facet_hook(0, c32.ctypes.data, n, None, n, U, w32.ctypes.data, 3, PATH_ONCHIP, out.ctypes.data, None))
            assert (out == 7).all()
        none = _hook(lib, codes, n, U, None, 2, PATH_AUTO)                   # no bitmap at all
        assert np.array_equal(none, np.stack([np.bincount(codes, minlength=U)] * 2)), U


def test_hook_small_shapes_tags_and_filter_passes(lib):
    """Both paths at small U: one value (every add meets in one bin), 17 filters (a partial second chunk), U = 600 (more
    than one on-chip pass per chunk: 13 filters per pass), several tiles, and a tag column with two rows of 1,024 tags."""
    rng = np.random.default_rng(3)
    # (20000, 3000, 1400): three tiles in 88 chunks, so the launcher gives a workgroup a run of two tiles, with bitmaps
    for n, U, m in ((1, 1, 1), (8230, 1, 17), (8230, 600, 17), (20000, 8, 33), (33, 5, 1), (20000, 3000, 1400)):
        codes = rng.integers(0, U, n)
        nw = (n + 31) // 32
        masks = [rng.random(n) < p for p in rng.choice([0.0, 0.3, 1.0], m)]
        words = np.stack([fm.pack(mk) for mk in masks])
        want = np.stack([np.bincount(codes[mk], minlength=U) for mk in masks])
        for path in (PATH_AUTO, PATH_ONCHIP, PATH_GLOBAL):
            assert np.array_equal(_hook(lib, codes, n, U, words, m, path), want), (n, U, m, path)
    # a run of two tiles per workgroup: the launcher lengthens the run only where the grid stays large, so 4,096 filters
    # (no bitmap: every one counts every row) over 17 tiles, the last run a single partial tile
    n, U, m = 16 * 8192 + 17, 1100, 4096
    codes = rng.integers(0, U, n)
    got = _hook(lib, codes, n, U, None, m, PATH_AUTO)
    assert (got == np.bincount(codes, minlength=U)[None, :]).all()
    n = 300
    rows = _tag_rows(n, 9)
    rows[7] = np.arange(1024) + 100
    rows[n - 1] = np.arange(1024) + 101
    lims, flat = _csr(rows)
    values, codes = fm.dictionary(flat)
    masks = [np.ones(n, bool), rng.random(n) < 0.5, np.zeros(n, bool)]
    masks[1][[7, n - 1]] = True
    want = fm.counts(flat, masks, None, lims)[1]
    words = np.stack([fm.pack(mk) for mk in masks])
    for path in (PATH_AUTO, PATH_GLOBAL):
        assert np.array_equal(_hook(lib, codes, n, len(values), words, 3, path, lims=lims), want), path


def test_counter_slab_groups(built, lib):
    """A call whose m x U exceeds the slab bound walks its filters in groups: with the bound lowered to 300 counters, 23
    filters x 142 values are twelve groups of two; the outputs equal those of one group, for counts and for top."""
    ix, L, _, _ = built
    n = ix.size
    masks = _masks(n, 23, 11)
    fs = _filters(ix, masks)
    whole = ix.facet("label", filter=fs)
    whole_top = ix.facet("label", filter=fs, top=10)
    assert len(whole[0]) == 142
    lib.check(lib.lib().cph_debug_facet_slab(ix._h, 300))
    try:
        grouped = ix.facet("label", filter=fs)
        grouped_top = ix.facet("label", filter=fs, top=10)
        lib.check(lib.lib().cph_debug_facet_slab(ix._h, 1))                  # below U: one filter per group still gets its U counters
        single = ix.facet("label", filter=fs)
    finally:
        lib.check(lib.lib().cph_debug_facet_slab(ix._h, 0))
    ev, ec = fm.counts(L, masks)
    assert np.array_equal(whole[1], ec)
    for a, b in zip(whole + whole_top, grouped + grouped_top):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(single[1], ec)
    _close(fs)


def test_top(built):
    """K = 1, 10 and 1,024; K above the number of non-zero values; many values tied in count, so the order among them is
    by value; found and the zero padding.  The all-distinct column scans 8,230 counters in several blocks, all tied at 1."""
    ix, L, uniq, _ = built
    n = ix.size
    ties = (np.arange(n) % 41) * 3 - 60                                      # 41 values: 30 with 201 rows, 11 with 200
    ties[:50] = 999                                                          # ... and one lighter, one new
    ix.set_column("ties", ties, ids="internal")
    masks = [None, np.arange(n) < 4000, np.zeros(n, bool), np.arange(n) % 41 < 3]
    fs = _filters(ix, masks)
    for col, data in (("ties", ties), ("label", L), ("uniq", uniq)):
        ev, ec = fm.counts(data, masks)
        for K in (1, 10, 1024):
            tv, tc, found = ix.facet(col, filter=fs, top=K)
            etv, etc, efound = fm.top(ev, ec, K)
            assert tv.dtype == np.int32 and tc.dtype == np.int64 and found.dtype == np.int32
            assert tv.shape == (4, K) and np.array_equal(tv, etv) and np.array_equal(tc, etc) and np.array_equal(found, efound), (col, K)
            assert found[2] == 0 and not tv[2].any() and not tc[2].any()
        one = ix.facet(col, filter=fs[1], top=10)                            # a single filter: [K], [K] and an int
        w = fm.top(ev, ec[1:2], 10)
        assert np.array_equal(one[0], w[0][0]) and np.array_equal(one[1], w[1][0]) and one[2] == int(w[2][0])
    tv, tc, found = ix.facet("ties", top=1024)                               # K above the number of values
    assert found == 42 and (tc[:42] > 0).all() and not tc[42:].any() and not tv[42:].any()
    assert (np.diff(tc[:42]) <= 0).all() and all(tv[i] < tv[i + 1] for i in range(41) if tc[i] == tc[i + 1])
    _close(fs)
    ix.set_column("ties", None)


def test_lifecycle(cph, tmp_path):
    rng = np.random.default_rng(5)
    n, dim = 700, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    L = rng.integers(0, 9, n)
    Y = rng.integers(2000, 2005, n)
    ix.set_labels(L, ids="internal")
    ix.set_column("year", Y, ids="internal")
    ix.prepare_facets("year")                                                # prepared, then asked: the same bytes as asked alone
    a = ix.facet("year")
    ix.set_column("year", Y, ids="internal")                                 # (drops the dictionary)
    b = ix.facet("year")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    mk = rng.random(n) < 0.5
    f = ix.make_filter(mk, ids="internal")
    before = ix.facet("label", filter=[None, f])
    R = np.zeros(n, bool)
    R[rng.choice(n, 150, replace=False)] = True
    R[L == 8] = True                                                         # a value loses every row: it stays, at count 0
    ix.remove(np.flatnonzero(R), ids="internal")
    after = ix.facet("label", filter=[None, f])                              # ... also through the filter made earlier
    ev, ec = fm.counts(L, [None, mk], R)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[0], ev) and np.array_equal(after[1], ec)
    assert np.array_equal(before[1] - after[1], fm.counts(L, [R, R & mk])[1]) and after[1][0][8] == 0
    tv, tc, found = ix.facet("label", top=1024)
    assert found == 8 and 8 not in tv[:8].tolist()
    f.close()
    ix.set_column("year", Y + 100, ids="internal")                           # other values: the dictionary is rebuilt
    ev, ec = fm.counts(Y + 100, [None], R)
    got = ix.facet("year")
    assert np.array_equal(got[0], ev) and np.array_equal(got[1], ec[0])
    new_map = ix.compact()                                                   # carries the columns; the facets follow the new rows
    assert ix.size == int((~R).sum()) and (new_map >= 0).sum() == ix.size
    for col, data in (("label", L), ("year", Y + 100)):
        ev, ec = fm.counts(data[~R], [None])
        got = ix.facet(col)
        assert np.array_equal(got[0], ev) and np.array_equal(got[1], ec[0]) and got[1].sum() == ix.size, col
    ix.set_column("year", None)                                              # add() refuses an index with named columns
    with pytest.raises(ValueError):
        ix.facet("year")
    Lc = ix.labels(ids="internal").astype(np.int64)
    new = np.array([100, 3, I32_MIN, 100, I32_MAX])
    ix.add(rng.standard_normal((5, dim)).astype(np.float32), labels=new)     # the label column grows, and so do its values
    ev, ec = fm.counts(np.concatenate([Lc, new]), [None])
    got = ix.facet("label")
    assert np.array_equal(got[0], ev) and np.array_equal(got[1], ec[0]) and got[0][0] == I32_MIN and got[0][-1] == I32_MAX
    p = str(tmp_path / "a.cphn")
    ix.compact()
    ix.save_native(p)
    ix.load_native(p)                                                        # a load drops the columns
    with pytest.raises(ValueError):
        ix.facet("label")


def test_dictionary_follows_set_labels_and_set_tags(cph):
    """Every column kind with a dictionary already built: replacing the label column, one named column or one tag column
    rebuilds exactly that dictionary, and the others keep theirs."""
    ix = _load(cph, "g16", 1)
    n = ix.size
    rng = np.random.default_rng(12)
    data = {"label": rng.integers(0, 6, n), "year": rng.integers(2000, 2004, n), "era": rng.integers(-3, 0, n)}
    rows = {"acl": _tag_rows(n, 1), "topic": _tag_rows(n, 2, vocab=30)}
    ix.set_labels(data["label"])
    ix.set_column("year", data["year"])
    ix.set_column("era", data["era"])
    for name, r in rows.items():
        ix.set_tags(name, r)

    def check():
        for name, col in data.items():
            ev, ec = fm.counts(col, [None])
            got = ix.facet(name)
            assert np.array_equal(got[0], ev) and np.array_equal(got[1], ec[0]), name
        for name, r in rows.items():
            lims, flat = _csr(r)
            ev, ec = fm.counts(flat, [None], None, lims)
            got = ix.facet(name)
            assert np.array_equal(got[0], ev) and np.array_equal(got[1], ec[0]), name

    check()                                                                  # (builds all five dictionaries)
    data["label"] = rng.integers(100, 103, n)
    ix.set_labels(data["label"])
    check()
    data["era"] = rng.integers(7, 30, n)
    ix.set_column("era", data["era"])
    check()
    rows["topic"] = _tag_rows(n, 3, vocab=9)
    ix.set_tags("topic", rows["topic"])
    check()
    rows["acl"] = [np.zeros(0, np.int64)] * n                                # a tag column without a tag: U = 0
    ix.set_tags("acl", rows["acl"])
    values, counts = ix.facet("acl", filter=[None, None])
    assert values.shape == (0,) and counts.shape == (2, 0)
    tv, tc, found = ix.facet("acl", top=3)
    assert not tv.any() and not tc.any() and found == 0
    ix.set_labels(None)
    with pytest.raises(ValueError):
        ix.facet("label")
    ix.set_tags("topic", None)
    with pytest.raises(ValueError):
        ix.facet("topic")


def test_part_views_know_column_names(cph):
    """part(i) reads the part's slice of the named and tag columns of its index, whether they were set before or after the
    view was made; a name the index does not hold is still refused."""
    rng = np.random.default_rng(31)
    n, dim = 640, 16
    P = cph.CPIndex(dim, 4, devices=[0, 0], partition=True)
    P.build(rng.standard_normal((n, dim)).astype(np.float32))
    P.finalize()
    Y = rng.integers(2000, 2006, n)
    P.set_column("year", Y)
    view = P.part(1)
    lo, hi = P.parts[1]
    assert view.columns == ["year"] and np.array_equal(view.column("year"), Y[lo:hi])
    f = view.where(year=(2001, 2003))
    assert f.count == int(((Y[lo:hi] >= 2001) & (Y[lo:hi] <= 2003)).sum())
    f.close()
    rows = _tag_rows(n, 6)
    P.set_tags("acl", rows)                                                  # after the view was made
    assert view.tag_columns == ["acl"]
    lims, flat = _csr(rows[lo:hi])
    ev, ec = fm.counts(flat, [None], None, lims)
    got = view.facet("acl")
    assert np.array_equal(got[0], ev) and np.array_equal(got[1], ec[0])
    with pytest.raises(ValueError):
        view.column_filter("price", 3)
    P.set_column("year", None)
    with pytest.raises(ValueError):
        view.facet("year")


def test_replicas_and_parts(cph):
    name, bits = "g128", 4
    S = _load(cph, name, bits)
    M = _load(cph, name, bits, devices=[0, 0])
    n = S.size
    rng = np.random.default_rng(8)
    L = rng.integers(0, 5, n)
    rows = _tag_rows(n, 4)
    masks = _masks(n, 7, 2)
    for ix in (S, M):
        ix.set_labels(L)
        ix.set_tags("acl", rows)
    fs_s, fs_m = _filters(S, masks), _filters(M, masks)
    assert len(fs_m[1]._hs) == 2
    for col in ("label", "acl"):
        for kw in ({}, {"top": 3}):
            a, b = S.facet(col, filter=fs_s, **kw), M.facet(col, filter=fs_m, **kw)
            assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b)), (col, kw)
    lims, flat = _csr(rows)
    assert np.array_equal(M.facet("acl", filter=fs_m)[1], fm.counts(flat, masks, None, lims)[1])
    with pytest.raises(ValueError):                                          # a filter with another replica count
        M.facet("label", filter=fs_s[1])
    _close(fs_s + fs_m)

    n, dim = 640, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    P = cph.CPIndex(dim, 4, devices=[0, 0], partition=True)
    P.build(X)
    P.finalize()
    L = rng.integers(3, 9, n)
    P.set_labels(L)
    P.set_column("year", L + 2000)
    with pytest.raises(ValueError, match=r"part\(i\)\.facet"):
        P.facet("label")
    with pytest.raises(ValueError, match=r"part\(i\)\.facet"):
        P.prepare_facets("label")
    (lo0, hi0), _ = P.parts
    part = P.part(0)
    mk = rng.random(hi0 - lo0) < 0.5
    for col, shift in (("label", 0), ("year", 2000)):
        ev, ec = fm.counts(L[lo0:hi0] + shift, [None, mk])                  # (column and mask both by input row)
        f = part.make_filter(mk, ids="input")
        got = part.facet(col, filter=[None, f])
        assert np.array_equal(got[0], ev) and np.array_equal(got[1], ec), col
        f.close()


def test_refusals(cph, lib, built):
    ix, L, _, _ = built
    n = ix.size
    f = ix.make_filter(np.ones(n, bool), ids="internal")
    for bad in (0, 1025, -1, True, 2.5):
        with pytest.raises(ValueError, match="top"):
            ix.facet("label", top=bad)
    for name in ("nope", "", 7):
        with pytest.raises(ValueError):
            ix.facet(name)
        with pytest.raises(ValueError):
            ix.prepare_facets(name)
    small = _load(cph, "g16", 1)
    with pytest.raises(ValueError, match="label"):                           # "label" without a label column
        small.facet("label")
    small.set_labels(np.zeros(small.size, np.int64))
    other = small.make_filter(np.ones(small.size, bool))
    with pytest.raises(ValueError):                                          # a filter of another size
        ix.facet("label", filter=other)
    with pytest.raises(ValueError):
        ix.facet("label", filter=[f, other])
    other.close()
    with pytest.raises(ValueError, match="closed"):
        ix.facet("label", filter=other)
    fresh = cph.CPIndex(16, 1)
    with pytest.raises(ValueError):                                          # not finalized
        fresh.facet("label")
    # the C entries: every refusal leaves preallocated outputs untouched
    Lb = lib.lib()
    counts = np.full(4 * 200, 77, np.uint64)
    tv, tc, found = np.full(8, 77, np.int32), np.full(8, 77, np.uint64), np.full(2, 77, np.uint32)
    U = C.c_uint64(77)
    two = (C.c_void_p * 2)(f._hs[0].value, f._hs[0].value)
    short = small.make_filter(np.ones(small.size, bool))                     # (held: the table below borrows its handle)
    mixed = (C.c_void_p * 2)(f._hs[0].value, short._hs[0].value)
    calls = [
        lambda: Lb.cph_facet_counts(ix._h, 7, 0, two, 2, counts.ctypes.data),                      # an unknown kind
        lambda: Lb.cph_facet_counts(ix._h, 1, 99, two, 2, counts.ctypes.data),                     # a slot out of range
        lambda: Lb.cph_facet_counts(ix._h, 1, 7, two, 2, counts.ctypes.data),                      # a slot without a column
        lambda: Lb.cph_facet_counts(ix._h, 2, 0, two, 2, counts.ctypes.data),                      # no tag column
        lambda: Lb.cph_facet_counts(ix._h, 0, 0, None, 2, counts.ctypes.data),                     # NULL filters stand for one
        lambda: Lb.cph_facet_counts(ix._h, 0, 0, mixed, 2, counts.ctypes.data),                    # a filter of another size
        lambda: Lb.cph_facet_counts(fresh._h, 0, 0, None, 1, counts.ctypes.data),                  # not finalized
        lambda: Lb.cph_facet_top(ix._h, 0, 0, two, 2, 0, tv.ctypes.data, tc.ctypes.data, found.ctypes.data),
        lambda: Lb.cph_facet_top(ix._h, 0, 0, two, 2, 1025, tv.ctypes.data, tc.ctypes.data, found.ctypes.data),
        lambda: Lb.cph_facet_top(ix._h, 0, 0, mixed, 2, 4, tv.ctypes.data, tc.ctypes.data, found.ctypes.data),
        lambda: Lb.cph_facet_values(ix._h, 1, 7, C.byref(U), None),
        lambda: Lb.cph_facet_prepare(fresh._h, 0, 0),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            lib.check(call())
        assert (counts == 77).all() and (tv == 77).all() and (tc == 77).all() and (found == 77).all() and U.value == 77, i
    lib.check(Lb.cph_facet_counts(ix._h, 0, 0, None, 1, counts.ctypes.data))                       # NULL with m == 1: all live rows
    assert np.array_equal(counts[:142].astype(np.int64), fm.counts(L, [None])[1][0]) and (counts[142:] == 77).all()
    us = C.c_double(0)
    with pytest.raises(ValueError):                                          # the timer is off by default: nothing was timed
        lib.check(Lb.cph_debug_last_facets_us(ix._h, C.byref(us)))
    ix.time_facets(True)
    ix.facet("label", filter=f)
    assert ix.last_facets_us() > 0
    ix.time_facets(False)
    f.close()
    short.close()
