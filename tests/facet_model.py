"""numpy model of the facet counts (cph_facet_values, cph_facet_counts, cph_facet_top; csrc/device_facets.h).

A dense column is one int per row; a tag column is a canonical CSR (lims [n + 1], tags ascending and distinct inside a
row: tags_model.canonical).  Everything is integers: every comparison against this model is exact equality."""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def dictionary(column):
    """(values int32 [U] ascending, codes [len(column)]): the distinct values of the WHOLE column (removed rows too)."""
    values, codes = np.unique(np.asarray(column, np.int64), return_inverse=True)
    return values.astype(np.int32), codes.reshape(-1).astype(np.int64)


def unpack(words, n):
    """bool [n] of a bitmap (uint32 words, bit i & 31 of word i >> 5); what lies behind n is not looked at."""
    w = np.ascontiguousarray(words, np.uint32)
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:n].astype(bool)


def pack(mask):
    m = np.asarray(mask, bool)
    pad = np.zeros((len(m) + 31) // 32 * 32, np.uint8)
    pad[:len(m)] = m
    return np.packbits(pad, bitorder="little").view(np.uint32).copy()


def counts(column, masks, removed=None, lims=None):
    """(values, counts int64 [m, U]).  masks: m bool arrays [n], None = every row; removed: bool [n] or None; lims: the
    CSR limits of a tag column (column = its tags), None for a dense one."""
    values, codes = dictionary(column)
    n = len(column) if lims is None else len(lims) - 1
    live = np.ones(n, bool) if removed is None else ~np.asarray(removed, bool)
    out = np.zeros((len(masks), len(values)), np.int64)
    for j, mk in enumerate(masks):
        ok = live if mk is None else (np.asarray(mk, bool) & live)
        if lims is not None:
            ok = np.repeat(ok, np.diff(np.asarray(lims, np.int64)))          # a row counts once per tag it holds
        out[j] = np.bincount(codes[ok], minlength=len(values))
    return values, out


def top(values, cnt, K):
    """(values int32 [m, K], counts int64 [m, K], found int32 [m]) of counts [m, U]: the K largest non-zero counts, count
    descending, ties by value ascending; zero behind found."""
    cnt = np.atleast_2d(cnt)
    m = cnt.shape[0]
    tv, tc, found = np.zeros((m, K), np.int32), np.zeros((m, K), np.int64), np.zeros(m, np.int32)
    for j in range(m):
        nz = np.flatnonzero(cnt[j])
        order = nz[np.lexsort((values[nz].astype(np.int64), -cnt[j][nz]))][:K]
        found[j] = len(order)
        tv[j, :len(order)] = values[order]
        tc[j, :len(order)] = cnt[j][order]
    return tv, tc, found


def check_by_hand():
    """Five rows, one removed, one filter: small enough to read (run by tests/test_facet_host.py)."""
    col = [7, I32_MAX, I32_MIN, 7, 7]
    removed = np.array([0, 0, 0, 1, 0], bool)
    f = np.array([1, 1, 0, 1, 1], bool)
    values, c = counts(col, [None, f], removed)
    assert list(values) == [I32_MIN, 7, I32_MAX]                # the removed row's value stays in the list
    assert c.tolist() == [[1, 2, 1], [0, 2, 1]]
    tv, tc, found = top(values, c, 2)
    assert tv.tolist() == [[7, I32_MIN], [7, I32_MAX]] and tc.tolist() == [[2, 1], [2, 1]] and found.tolist() == [2, 2]
    tv, tc, found = top(values, c, 4)
    assert tv[1].tolist() == [7, I32_MAX, 0, 0] and tc[1].tolist() == [2, 1, 0, 0] and found.tolist() == [3, 2]
    # a tag column: rows {}, {1, 2}, {2}: row 1 counts once for each of its tags
    values, c = counts([1, 2, 2], [None, np.array([0, 0, 1], bool)], lims=[0, 0, 2, 3])
    assert list(values) == [1, 2] and c.tolist() == [[1, 2], [0, 1]]
    assert np.array_equal(unpack(pack(f), 5), f)
