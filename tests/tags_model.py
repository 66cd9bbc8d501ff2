"""The numpy statement of the tag columns (cph_set_tags / cph_filters_from_tags): both test tiers compare against it.

A column is a CSR (lims[n + 1], tags); canonical = every row ascending and distinct.  A test is a value set V (made
ascending and distinct) and a mode; with c(row) = number of the row's tags that are in V the row is allowed when c > 0
("any"), c == |V| ("all") or c == 0 ("none")."""
import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
MODES = {"any": 0, "all": 1, "none": 2}
NOBODY = 123456789                    # a value no generated row holds


def to_csr(rows):
    """A sequence of per-row integer sequences -> (lims int64[n + 1], tags int64)."""
    lims = np.zeros(len(rows) + 1, np.int64)
    if len(rows):
        np.cumsum([len(r) for r in rows], out=lims[1:])
    flat = [np.asarray(r, np.int64) for r in rows if len(r)]
    return lims, (np.concatenate(flat) if flat else np.zeros(0, np.int64))


def rows_of(lims, tags):
    return [np.asarray(tags[lims[i]:lims[i + 1]]) for i in range(len(lims) - 1)]


def canonical(lims, tags, order=None):
    """The canonical column; order (optional): canonical row i is the given row order[i]."""
    rows = rows_of(np.asarray(lims, np.int64), np.asarray(tags))
    if order is not None:
        rows = [rows[int(r)] for r in order]
    return to_csr([np.unique(r) for r in rows])


def counts_in(lims, tags, values):
    """c(row) for every row of a canonical column: np.isin and np.add.reduceat, guarded for empty rows."""
    n = len(lims) - 1
    c = np.zeros(n, np.int64)
    if n == 0 or len(tags) == 0:
        return c
    hit = np.isin(tags, values).astype(np.int64)
    lens = np.diff(lims)
    full = lens > 0
    c[full] = np.add.reduceat(hit, lims[:-1][full])      # (consecutive non-empty starts: every segment is one row)
    return c


def allowed(lims, tags, values, mode):
    """bool[n]: the rows test (values, mode) allows, on a canonical column."""
    v = np.unique(np.asarray(values, np.int64).ravel())
    c = counts_in(lims, tags, v)
    if mode == "any":
        return c > 0
    if mode == "all":
        return c == len(v)
    assert mode == "none", mode
    return c == 0


def pack(mask):
    from cphnsw_mi355x.index import pack_allowed_bits
    return pack_allowed_bits(mask)


def expect(lims, tags, tests, modes):
    """(words uint32[m][(n + 31) / 32], counts uint64[m]) of the tests on a canonical column."""
    n = len(lims) - 1
    words = np.zeros((len(tests), (n + 31) // 32), np.uint32)
    counts = np.zeros(len(tests), np.uint64)
    for j, (t, mode) in enumerate(zip(tests, modes)):
        mask = allowed(lims, tags, t, mode)
        words[j] = pack(mask)
        counts[j] = mask.sum()
    return words, counts


def test_kinds(present, j):
    """The test kinds of both tiers, cycling with j over 8 kinds x 3 modes -> (values, mode).  present: tags some row may
    hold (at least 2).  A single value; 2 values; exactly 64 distinct values; the empty set; a value nobody has;
    duplicated and unsorted input; INT32_MIN and INT32_MAX; a mix of held and unheld values."""
    p = [int(x) for x in present]
    kind, mode = j % 8, ("any", "all", "none")[(j // 8) % 3]
    pick = p[(j // 24) % len(p)]
    if kind == 0:
        v = [pick]
    elif kind == 1:
        v = [pick, p[(j // 24 + 1) % len(p)]]
    elif kind == 2:
        v = (p + [1000000 + i for i in range(64)])[:64]
    elif kind == 3:
        v = []
    elif kind == 4:
        v = [NOBODY]
    elif kind == 5:
        v = [p[1], pick, p[0], pick, p[1], p[1]]
    elif kind == 6:
        v = [I32_MAX, I32_MIN]
    else:
        v = [pick, NOBODY]
    return v, mode


test_kinds.__test__ = False
