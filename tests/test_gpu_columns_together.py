"""Every kind of row attribute on one index at once -- the label column, an int32 column, a tag column of empty rows (no
value buffer on the device) and a tag column with a row of CPH_MAX_TAGS_PER_ROW tags -- through the walks that treat them
alike: the replica fan-out, the copy to the replicas after a compact, the facet dictionary of a replica without host
arrays, the drop of one column among the others, a load, and the cut at the part bounds.

The yardsticks: numpy for the dense columns, tests/tags_model.py for the tag columns, a single-device index with the same
columns for the facets."""
import ctypes as C

import numpy as np
import pytest

import tags_model as tm
from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

DIM = DATASETS["g16"]["dim"]                      # the rows of the g16 fixture (padded to D = 16), so that it loads into the same index
LONG = np.arange(1024) - 500                       # CPH_MAX_TAGS_PER_ROW distinct tags
MODES = ("any", "all", "none")


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _same_csr(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _columns(n, seed, long_row):
    """The four columns by input row: labels, years, the canonical rows of `empty` and of `acl`."""
    rng = np.random.default_rng(seed)
    acl = [np.unique(rng.choice(np.arange(3, 15), rng.integers(0, 5), replace=False)) for _ in range(n)]
    acl[long_row] = LONG
    return dict(label=rng.integers(0, 7, n).astype(np.int32), year=rng.integers(1990, 2011, n).astype(np.int32),
                empty=[np.zeros(0, np.int64)] * n, acl=acl)


def _set_all(ix, cols):
    ix.set_labels(cols["label"])
    ix.set_column("year", cols["year"])
    ix.set_tags("empty", cols["empty"])
    ix.set_tags("acl", [np.concatenate([r[::-1], r[:2]]) for r in cols["acl"]])      # any order, duplicates: stored canonical


def _permuted(cols, old_to_new):
    """The columns of the compacted index: new input row old_to_new[r] holds what row r held."""
    live = np.flatnonzero(old_to_new >= 0)
    out = {}
    for name, c in cols.items():
        new = [None] * len(live)
        for r in live:
            new[old_to_new[r]] = c[r]
        out[name] = np.array(new, np.int32) if name in ("label", "year") else new
    return out


def _check_handle(ix, h, n, cols, names=("label", "year", "empty", "acl")):
    """What handle h (a replica, a part) holds of the named columns, by input row, against the model."""
    if "label" in names:
        assert np.array_equal(ix._labels_of(h, n, True), cols["label"])
    if "year" in names:
        assert np.array_equal(ix._labels_of(h, n, True, ix._slot("year")), cols["year"])
    for name in ("empty", "acl"):
        if name in names:
            assert _same_csr(ix._tags_of(h, n, True, ix._tag_slot(name)), tm.to_csr(cols[name])), name


def _holds(lib, h):
    """Which of the 1 + 8 + 4 columns handle h holds."""
    def flag(entry, *slot):
        f = C.c_int(0)
        assert entry(h, *slot, C.byref(f)) == 0
        return bool(f.value)
    return ([flag(lib.cph_has_labels)] + [flag(lib.cph_has_column, s) for s in range(8)] + [flag(lib.cph_has_tags, s) for s in range(4)])


def _filters(ix):
    """(what, filter, its mask by input row given the columns): every pass, every tag mode, and an & of two."""
    made = [("label", ix.label_filter(3), lambda c: c["label"] == 3),
            ("year", ix.column_filter("year", 2001, 2005), lambda c: (c["year"] >= 2001) & (c["year"] <= 2005))]
    for mode in MODES:
        for name, test in (("acl", [5, 9]), ("acl", [-500, 523]), ("empty", [5])):
            made.append((f"{name} {mode} {test}", ix.tag_filter(name, test, mode),
                         lambda c, name=name, test=test, mode=mode: tm.allowed(*tm.to_csr(c[name]), test, mode)))
    made.append(("label & acl", made[0][1] & made[2][1], lambda c: made[0][2](c) & made[2][2](c)))
    return made


def _export(lib, h, n):
    w, c = np.empty((n + 31) // 32, np.uint32), C.c_uint64(0)
    assert lib.cph_filter_export(h, w.ctypes.data, C.byref(c)) == 0
    return w, c.value


def _check_replica_filters(cph, lib, M, cols):
    """Every replica made the same bitmap, and it is the model's mask moved to internal ids."""
    n, rows = M.size, M.row_map()
    for what, f, mask in _filters(M):
        want = mask(cols)[rows]
        per_rep = [_export(lib, h, n) for h in f._hs]
        assert len(per_rep) == 2, what
        for w, c in per_rep:
            assert np.array_equal(w, cph.index.pack_allowed_bits(want)) and c == int(want.sum()) == f.count, what
        f.close()


def _facet_of(lib, h, kind, slot):
    """(values, counts over all live rows) as handle h answers cph_facet_values / cph_facet_counts."""
    U = C.c_uint64(0)
    assert lib.cph_facet_values(h, kind, slot, C.byref(U), None) == 0
    values, counts = np.empty(U.value, np.int32), np.zeros(U.value, np.uint64)
    assert lib.cph_facet_values(h, kind, slot, C.byref(U), values.ctypes.data if U.value else None) == 0
    assert lib.cph_facet_counts(h, kind, slot, None, 1, counts.ctypes.data if U.value else None) == 0
    return values, counts.view(np.int64)


def _check_facets(lib, M, S):
    """facet() of the replicated index, and of each replica on its own (the second one has no host arrays: its dictionary
    comes from the device copy), against the single index."""
    for name in ("acl", "label", "empty"):
        want = S.facet(name)
        assert _same_csr(M.facet(name), want), name
        kind, slot = M._facet_column(name)
        for h in M._replicas():
            assert _same_csr(_facet_of(lib, h, kind, slot), want), name
    assert len(S.facet("empty")[0]) == 0 and len(S.facet("acl")[0]) >= 1024


def test_columns_together_replicas(cph):
    lib = cph._lib.lib()
    rng = np.random.default_rng(41)
    n = 600                                              # 18 full bitmap words and one of 24 bits
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    cols = _columns(n, 42, 7)
    S, M = cph.CPIndex(DIM, 1), cph.CPIndex(DIM, 1, devices=[0, 0])
    for ix in (S, M):
        ix.build(X)
        ix.finalize()
        ix.result_ids = "input"
        _set_all(ix, cols)
    assert M.has_labels and M.columns == ["year"] and sorted(M.tag_columns) == ["acl", "empty"]
    for h in M._replicas():
        _check_handle(M, h, n, cols)
    _check_replica_filters(cph, lib, M, cols)
    _check_facets(lib, M, S)
    # compact: replica 0 sets the gathered columns again, the others receive its device copies
    gone = rng.choice(n, 200, replace=False)
    gone = gone[gone != 7]
    for ix in (S, M):
        ix.remove(gone)
    old_to_new = M.compact()
    assert np.array_equal(S.compact(), old_to_new)
    cols, n = _permuted(cols, old_to_new), n - len(gone)
    assert M.size == n and M.has_labels and M.columns == ["year"] and sorted(M.tag_columns) == ["acl", "empty"]
    assert len(cols["acl"][old_to_new[7]]) == 1024
    for h in M._replicas():
        _check_handle(M, h, n, cols)
    _check_replica_filters(cph, lib, M, cols)
    _check_facets(lib, M, S)
    # each column goes alone
    left = ["label", "year", "empty", "acl"]
    for name, drop in (("empty", lambda: M.set_tags("empty", None)), ("label", lambda: M.set_labels(None)),
                       ("acl", lambda: M.set_tags("acl", None)), ("year", lambda: M.set_column("year", None))):
        drop()
        left.remove(name)
        for h in M._replicas():
            _check_handle(M, h, n, cols, left)
            assert sum(_holds(lib, h)) == len(left), name
    # a load drops all of them on every replica
    _set_all(M, cols)
    for h in M._replicas():
        assert sum(_holds(lib, h)) == 4
    M.load(fixture_path("g16", 1))
    assert M.size == 300 and not M.has_labels and M.columns == [] and M.tag_columns == []
    for h in M._replicas():
        assert not any(_holds(lib, h))


def test_columns_together_parts(cph):
    lib = cph._lib.lib()
    rng = np.random.default_rng(43)
    n, k = 640, 10
    X = rng.standard_normal((n, DIM)).astype(np.float32)
    Q = rng.standard_normal((5, DIM)).astype(np.float32)
    P = cph.CPIndex(DIM, 1, devices=[0, 0], partition=True)
    P.build(X)
    P.finalize()
    (lo0, hi0), (lo1, hi1) = P.parts
    long_row = lo1 + 3                                   # the longest row lives in part 1
    cols = _columns(n, 44, long_row)
    for r in range(hi0 - 20, hi0 + 20):
        cols["acl"][r] = np.array([5, 100])              # rows with tags on both sides of the bound
    _set_all(P, cols)                                    # global input rows, cut at the bound

    def check_all(cols, names=("label", "year", "empty", "acl")):
        for h, (lo, hi) in zip(P._replicas(), P.parts):
            cut = {name: c[lo:hi] for name, c in cols.items()}
            _check_handle(P, h, hi - lo, cut, names)
        if "acl" in names:
            assert _same_csr(P.tags("acl"), tm.to_csr(cols["acl"]))
        assert np.array_equal(P.labels(), cols["label"]) and np.array_equal(P.column("year"), cols["year"])

    def check_filters(cols):
        for what, f, mask in _filters(P):
            want = mask(cols)
            assert f.count == int(want.sum()) and f.size == P.size, what
            g = P.make_filter(want)
            a, b = P.search_batch(Q, k, filter=f, exact=True), P.search_batch(Q, k, filter=g, exact=True)
            assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), what
            f.close()
            g.close()

    check_all(cols)
    check_filters(cols)
    # a refused call leaves every column on both parts
    with pytest.raises(ValueError):
        P.set_tags("acl", cols["acl"][:-1])
    check_all(cols)
    gone = rng.choice(n, 60, replace=False)
    gone = gone[gone != long_row]
    P.remove(gone)
    old_to_new = P.compact()
    cols = _permuted(cols, old_to_new)
    assert P.size == n - len(gone) and P.has_labels and P.columns == ["year"] and sorted(P.tag_columns) == ["acl", "empty"]
    check_all(cols)                                      # cut again at the new bounds
    check_filters(cols)
    # a row the second part refuses, after the first part took its slice: the column goes from both, the others stay
    (lo0, hi0), (lo1, hi1) = P.parts
    bad = list(cols["acl"])
    bad[lo1 + 1] = np.arange(1025)
    with pytest.raises(ValueError):
        P.set_tags("acl", bad)
    assert P.tag_columns == ["empty"]
    for h in P._replicas():
        assert sum(_holds(lib, h)) == 3
    check_all(cols, ("label", "year", "empty"))
