"""Filter algebra and attribute columns on the GPU (IdFilter operators, combine_filters, set_column / column_filter /
where, cph_filter_combine_hook).

The expected values never come from the code under test: bitmaps and counts are numpy on the words
(tests/filter_ops_model.py, pack_allowed_bits of the numpy mask), rows are what make_filter(numpy-combined mask) plus the
existing search call return -- ids and distance bytes."""
import numpy as np
import pytest

from filter_ops_model import OPS, cases, expect, nwords, operands
from golden_util import DATASETS, fixture_path
from test_gpu_labels import BOUNDS, I32_MAX, I32_MIN

pytestmark = pytest.mark.gpu


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


def _pack(cph, mask):
    return cph.index.pack_allowed_bits(mask)


def _is(cph, f, mask, n):
    """f holds exactly `mask`: every word, the count, the size."""
    assert np.array_equal(f.words(), _pack(cph, mask)) and f.count == int(mask.sum()) and f.size == n


# ---- 1. the kernel through its hook ---------------------------------------------------------------------------------
def _hook(op, a, b, bc, n_bits):
    from cphnsw_mi355x import _lib
    m = a.shape[0]
    words = np.full((m, nwords(n_bits)), 0xDEADBEEF, np.uint32)
    counts = np.full(m, 12345, np.uint64)
    bb = None if op == "not" else np.ascontiguousarray(b)
    _lib.check(_lib.lib().cph_filter_combine_hook(0, OPS[op], a.ctypes.data, None if bb is None else bb.ctypes.data, int(bc), n_bits, m,
                                                  words.ctypes.data, counts.ctypes.data, None))
    return words, counts


@pytest.mark.parametrize("n_bits", [1, 33, 129, 32768, 32769, 100003])
def test_combine_kernel_words_and_counts(n_bits):
    """One word; a partial last word; nw % 4 in {1, 2, 0}; exactly one 256-thread block of quads (32,768 bits = 1,024
    words); one word into the second block; several blocks with a ragged end (100,003 bits: 3,126 words, nw % 4 = 2).
    Random words with dirty tails, the all-zero and the all-ones operand; the hook pre-fills the outputs with garbage."""
    nw = nwords(n_bits)
    for m in (1, 3, 70):
        a, b = operands(n_bits, m, 7 * n_bits + m)
        for op, bc in cases():
            bb = None if op == "not" else b[:1] if bc else b
            words, counts = _hook(op, a, bb, bc, n_bits)
            ew, ec = expect(op, a, bb, n_bits)
            assert np.array_equal(words, ew), (op, bc, m)
            assert np.array_equal(counts, ec), (op, bc, m)
    a, _ = operands(n_bits, 3, n_bits)
    for fill in (0, 0xFFFFFFFF):                           # the broadcast operand all zeros, all ones
        b = np.full((1, nw), fill, np.uint32)
        for op in ("and", "or", "andnot", "xor"):
            words, counts = _hook(op, a, b, True, n_bits)
            ew, ec = expect(op, a, b, n_bits)
            assert np.array_equal(words, ew) and np.array_equal(counts, ec), (op, fill)


# ---- 2. filters end to end -------------------------------------------------------------------------------------------
NP_OPS = {"and": lambda x, y: x & y, "or": lambda x, y: x | y, "andnot": lambda x, y: x & ~y, "xor": lambda x, y: x ^ y}


@pytest.mark.parametrize("name,bits", [("g16", 1), ("g1024", 2), ("g2048", 1)])
def test_filter_operators_end_to_end(cph, name, bits):
    ix = _load(cph, name, bits)
    n = ix.size
    assert n == {"g16": 300, "g1024": 160, "g2048": 88}[name]
    rng = np.random.default_rng(n)
    if name == "g16":                                      # a v2 fixture carries no row map: give one of them a map
        ix.set_row_map(rng.permutation(n))
    m1, m2 = rng.random(n) < 0.5, rng.random(n) < 0.3
    L = rng.integers(0, 4, n)
    ix.set_labels(L, ids="internal")
    lab = ix.label_filters([0, 1])                         # two views of one slab
    ops = [(ix.make_filter(m1, ids="internal"), m1), (ix.make_filter(np.flatnonzero(m2), ids="internal"), m2),
           (lab[0], L == 0), (lab[1], L == 1),
           (ix.make_filter(np.zeros(n, bool), ids="internal"), np.zeros(n, bool)),
           (ix.make_filter(np.ones(n, bool), ids="internal"), np.ones(n, bool))]
    if ix.has_row_map:
        m3 = rng.random(n) < 0.4
        ops.append((ix.make_filter(m3, ids="input"), m3[ix.row_map()]))
    first = ops[0][0] | ops[2][0]                          # the result of an earlier combine is an operand like any other
    ops.append((first, m1 | (L == 0)))
    before = [(f.words(), f.count) for f, _ in ops]
    for f, mf in ops:
        _is(cph, f, mf, n)
        inv = ~f
        _is(cph, inv, ~mf, n)
        back = ~inv
        _is(cph, back, mf, n)                              # ~~f == f
        g = ix.make_filter(~mf, ids="internal")            # ... and a make_filter of the numpy mask agrees
        assert np.array_equal(g.words(), inv.words()) and g.count == inv.count
        for x in (inv, back, g):
            x.close()
        for g, mg in ops:
            for h, want in ((f & g, mf & mg), (f | g, mf | mg), (f - g, mf & ~mg), (f ^ g, mf ^ mg)):
                _is(cph, h, want, n)
                h.close()
    fs, masks = [f for f, _ in ops], [mf for _, mf in ops]
    for op, fn in NP_OPS.items():
        one = ix.combine_filters(op, fs, ops[1][0])        # a list against a broadcast operand
        pair = ix.combine_filters(op, fs, fs[::-1])        # ... and against a list
        for j in range(len(fs)):
            _is(cph, one[j], fn(masks[j], m2), n)
            _is(cph, pair[j], fn(masks[j], masks[-1 - j]), n)
        for x in one + pair:
            x.close()
    for x, mf in zip(ix.combine_filters("not", fs), masks):
        _is(cph, x, ~mf, n)
    assert ix.combine_filters("and", [], ops[0][0]) == []
    chain = (ops[0][0] & ops[1][0]) | ~ops[2][0]           # the temporaries of a chain free themselves
    _is(cph, chain, (m1 & m2) | ~(L == 0), n)
    for (f, _), (w, c) in zip(ops, before):                # the inputs are unchanged
        assert np.array_equal(f.words(), w) and f.count == c


# ---- 3. search parity ---------------------------------------------------------------------------------------------------
def _dev(ix, Qd, k, **kw):
    import torch
    i_, d_ = ix.search_batch_device(Qd, k, **kw)
    ix.synchronize()
    torch.cuda.synchronize()
    return i_.cpu().numpy(), d_.cpu().numpy()


def _same(got, want, where):
    assert np.array_equal(got[0], want[0]) and _beq(got[1], want[1]), where


def _stats(ix):
    st = ix.last_search_stats()
    st.pop("kernel_us")
    return st


class _Parity:
    """g128 at 4 bits, k = 10, the queries of tests/test_gpu_labels.py: tenants in the label column, an "in stock" and a
    "blocked" mask, the combined filters next to the numpy masks they must equal."""

    def __init__(self, cph, gold):
        import torch
        self.k = 10
        self.ix = ix = _load(cph, "g128", 4)
        self.n = n = ix.size
        self.Q = gold["Q/g128"]
        self.Qd = torch.from_numpy(self.Q).to(f"cuda:{ix.devices[0]}")
        self.rng = rng = np.random.default_rng(11)
        self.L = L = rng.choice([0, 1, 2, 3], n, p=[0.6, 0.3, 0.08, 0.02])
        self.stock = stock = rng.random(n) < 0.5
        self.blocked = blocked = rng.random(n) < 0.1
        ix.set_labels(L)
        self.in_stock, self.f_blocked = in_stock, f_blocked = ix.make_filter(stock), ix.make_filter(blocked)
        t = ix.label_filters([0, 1, 2, 3])
        self.combos = [(t[0] & in_stock, (L == 0) & stock, "tenant AND stock"), (t[1] | t[2], (L == 1) | (L == 2), "category OR"),
                       (~f_blocked, ~blocked, "NOT blocked"), (in_stock - f_blocked, stock & ~blocked, "ANDNOT"),
                       (t[3] ^ in_stock, (L == 3) ^ stock, "XOR"),
                       ((t[2] | t[3]) & in_stock - f_blocked, ((L == 2) | (L == 3)) & stock & ~blocked, "chain")]
        # the per-tenant recipe: many tenant bitmaps AND one common mask, one filter per query
        lq = rng.choice([0, 1, 2, 3, 99], len(self.Q))
        lq[:5] = (0, 1, 2, 3, 99)
        vals, self.inv = np.unique(lq, return_inverse=True)
        self.gs = ix.combine_filters("and", ix.label_filters(vals), in_stock)
        self.host = [ix.make_filter((L == v) & stock) for v in vals]

    def every_call(self, h, mask, tag, ranges=True):
        ix, Q, Qd, k = self.ix, self.Q, self.Qd, self.k
        g = ix.make_filter(mask)
        assert h.count == g.count == int(mask.sum()), tag
        _same(ix.search_batch(Q, k, filter=h), ix.search_batch(Q, k, filter=g), (tag, "batch"))
        _same(ix.search(Q[0], k, filter=h), ix.search(Q[0], k, filter=g), (tag, "search"))
        _same(_dev(ix, Qd, k, filter=h), _dev(ix, Qd, k, filter=g), (tag, "device"))
        _same(ix.search_batch(Q, k, filter=h, exact=True), ix.search_batch(Q, k, filter=g, exact=True), (tag, "exact"))
        for kw in ({"exact": True}, {"exact": False, "max_results": 20}) if ranges else ():
            a, b = ix.range_search(Q, 40.0, filter=h, **kw), ix.range_search(Q, 40.0, filter=g, **kw)
            assert all(np.array_equal(x, y) for x, y in zip(a[:2], b[:2])) and _beq(a[2], b[2]), (tag, "range", kw)
        g.close()

    def per_tenant(self, tag):
        ix, Q, k = self.ix, self.Q, self.k
        for kw in ({}, {"exact": True}):
            _same(ix.search_batch(Q, k, filter=self.gs, filter_of=self.inv, **kw),
                  ix.search_batch(Q, k, filter=self.host, filter_of=self.inv, **kw), (tag, kw))
        _same(_dev(ix, self.Qd, k, filter=self.gs, filter_of=self.inv), _dev(ix, self.Qd, k, filter=self.host, filter_of=self.inv), (tag, "device"))


def test_combined_filter_search_parity(cph, gold):
    """search_batch, search, search_batch_device, exact=True and range_search under a combined filter equal the same
    call under make_filter(numpy-combined mask): ids and distance bytes."""
    p = _Parity(cph, gold)
    for h, mask, tag in p.combos:
        p.every_call(h, mask, tag)


def test_per_tenant_recipe_and_routing(cph, gold):
    """combine_filters("and", label_filters(vals), in_stock) with filter_of= equals filter=[make_filter(...)...] row for
    row; with exact_threshold set, a combined filter routes like the host-made one: equal last_search_stats."""
    p = _Parity(cph, gold)
    ix, Q, k = p.ix, p.Q, p.k
    assert [g.count for g in p.gs] == [f.count for f in p.host]
    p.per_tenant("per tenant")
    counts = sorted(g.count for g in p.gs if g.count)
    thr = (counts[0] + counts[-1]) // 2
    assert counts[0] <= thr < counts[-1]                   # one call mixes scanned and graph-searched queries
    ix.exact_threshold = thr
    p.per_tenant("per tenant, routed")
    stats = []
    for fl in (p.gs, p.host):
        ix.search_batch(Q, k, filter=fl, filter_of=p.inv)
        stats.append(_stats(ix))
    assert stats[0] == stats[1] and stats[0]["expansions"] > 0
    sides = set()
    for h, mask, tag in (p.combos[4], p.combos[5], p.combos[1]):
        g = ix.make_filter(mask)
        sides.add(h.count <= thr)
        _same(ix.search_batch(Q, k, filter=h), ix.search_batch(Q, k, filter=g), (tag, "routed"))
        ix.search_batch(Q, k, filter=h)
        sh = _stats(ix)
        ix.search_batch(Q, k, filter=g)
        assert sh == _stats(ix), tag
    assert sides == {True, False}                          # a scanned filter and a graph-searched one


def test_combined_filters_with_removed_rows(cph, gold):
    """Removed rows are not special: the same filters after a remove() of allowed rows; ~f sets their bits and the
    search drops them all the same."""
    p = _Parity(cph, gold)
    ix, Q, k = p.ix, p.Q, p.k
    gone = np.flatnonzero((p.L == 0) & p.stock & ~p.blocked)[:7]
    assert ix.remove(gone) == 7
    for h, mask, tag in p.combos[:4]:
        p.every_call(h, mask, tag + ", removed", ranges=tag == "NOT blocked")
        ids, _ = ix.search_batch(Q, k, filter=h, exact=True)
        assert not np.isin(ids, gone).any()
    f = p.combos[0][0]
    inv_f = ~f
    assert inv_f.count == p.n - f.count                    # ~f sets the removed rows' bits too ...
    ids, _ = ix.search_batch(Q, k, filter=inv_f | f, exact=True)
    assert (ids >= 0).all() and not np.isin(ids, gone).any()      # ... and the search drops them all the same
    p.per_tenant("per tenant, removed")


# ---- 4. replicas and parts ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built(cph):
    """640 x 16 at 4 bits, the shape of test_labels_parts: single device, two replicas, two parts; masks in input rows."""
    rng = np.random.default_rng(21)
    n, dim = 640, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((9, dim)).astype(np.float32)
    out = {}
    for key, kw in (("S", {}), ("M", {"devices": [0, 0]}), ("P", {"devices": [0, 0], "partition": True})):
        ix = cph.CPIndex(dim, 4, **kw)
        ix.build(X)
        ix.finalize()
        ix.result_ids = "input"
        out[key] = ix
    out["M"].set_min_shard(1)
    m1, m2 = rng.random(n) < 0.5, rng.random(n) < 0.3
    (lo0, hi0), _ = out["P"].parts
    m2[hi0 - 20:hi0 + 20] = True                           # straddles the part bound
    return out, X, Q, m1, m2


def test_filter_operators_replicas_and_parts(cph, built):
    ixs, X, Q, m1, m2 = built
    S, M, P = ixs["S"], ixs["M"], ixs["P"]
    n, k = S.size, 10
    for ix in (M, P):
        f, g = ix.make_filter(m1), ix.make_filter(m2)
        res = [(f & g, m1 & m2), (f | g, m1 | m2), (f - g, m1 & ~m2), (f ^ g, m1 ^ m2), (~f, ~m1)]
        res += list(zip(ix.combine_filters("and", [f, g, ~g], g), [m1 & m2, m2, np.zeros(n, bool)]))
        res += list(zip(ix.combine_filters("xor", [f, g], [g, f]), [m1 ^ m2, m1 ^ m2]))
        for h, mask in res:
            assert h.count == int(mask.sum()) and h.size == n
            own = ix.make_filter(mask)
            if ix is M:
                assert len(h._hs) == 2 and np.array_equal(h.words(), own.words())
            for kw in ({}, {"exact": True}):               # the same index under the host-made filter: every path
                _same(ix.search_batch(Q, k, filter=h, **kw), ix.search_batch(Q, k, filter=own, **kw), (ix is M, kw))
            # ... and the rows of the single-device index (the exact scan does not depend on the graph)
            _same(ix.search_batch(Q, k, filter=h, exact=True), S.search_batch(Q, k, filter=S.make_filter(mask), exact=True), (ix is M, "single"))
        fo = np.arange(len(Q)) % 2
        hs = ix.combine_filters("or", [f, g], ~f)
        _same(ix.search_batch(Q, k, filter=hs, filter_of=fo, exact=True),
              S.search_batch(Q, k, filter=[S.make_filter(m1 | ~m1), S.make_filter(m2 | ~m1)], filter_of=fo, exact=True), "filter_of")
    # mismatched replica and part counts, and a partitioned filter with a plain one
    fs, fm, fp = S.make_filter(m1), M.make_filter(m1), P.make_filter(m1)
    P3 = cph.CPIndex(16, 4, devices=[0, 0, 0], partition=True)
    P3.build(X)
    P3.finalize()
    fp3 = P3.make_filter(m1)
    for a, b in ((fs, fm), (fm, fs), (fp, fp3), (fs, fp), (fp, fm)):
        with pytest.raises(ValueError):
            a & b
        with pytest.raises(ValueError):
            cph.combine_filters("or", [a], [b])


# ---- 5. columns ---------------------------------------------------------------------------------------------------------
def _check_column_filters(cph, ix, V_internal, bounds, fs):
    for (lo, hi), f in zip(bounds, fs):
        mask = (V_internal >= lo) & (V_internal <= hi)
        _is(cph, f, mask, ix.size)
        g = ix.make_filter(mask, ids="internal")
        assert np.array_equal(g.words(), f.words()) and g.count == f.count, (lo, hi)
        g.close()


def _values(n, seed):
    rng = np.random.default_rng(seed)
    special = np.array([I32_MIN, -1, 0, 1, 5, I32_MAX], np.int64)
    return np.where(rng.random(n) < 0.7, special[rng.integers(0, 6, n)], rng.integers(-50, 50, n))


def test_columns_on_a_fixture(cph):
    ix = _load(cph, "g16", 1)
    n = ix.size
    assert ix.columns == []
    with pytest.raises(ValueError):
        ix.column("year")
    with pytest.raises(ValueError):
        ix.column_filter("year", 1)
    V, W, L = _values(n, 1), _values(n, 2), _values(n, 3)
    ix.set_column("year", V)
    ix.set_column("price", W.astype(np.int64))
    ix.set_labels(L)
    assert ix.columns == ["year", "price"]
    assert ix.column("year").dtype == np.int32 and np.array_equal(ix.column("year"), V) and np.array_equal(ix.column("price"), W)
    assert np.array_equal(ix.column("label"), L) and np.array_equal(ix.labels(), L)      # the label column stays what it is
    lo, hi = [b[0] for b in BOUNDS], [b[1] for b in BOUNDS]
    _check_column_filters(cph, ix, V, BOUNDS, ix.column_filters("year", lo, hi))
    _check_column_filters(cph, ix, W, BOUNDS, [ix.column_filter("price", a, b) for a, b in BOUNDS])
    _check_column_filters(cph, ix, V, [(5, 5)], [ix.column_filter("year", 5)])
    _check_column_filters(cph, ix, L, BOUNDS, ix.column_filters("label", lo, hi))
    assert ix.column_filters("year", []) == []
    # where: two columns plus the label column in one call
    _is(cph, ix.where(year=5, price=(-1, 5), label=(0, I32_MAX)), (V == 5) & (W >= -1) & (W <= 5) & (L >= 0), n)
    _is(cph, ix.where(year=(-1, 1)), (V >= -1) & (V <= 1), n)
    _is(cph, ix.where(label=1), L == 1, n)
    with pytest.raises(ValueError):
        ix.where()
    with pytest.raises(ValueError):
        ix.where(nobody=1)
    with pytest.raises(ValueError):
        ix.where(year=(1, 2, 3))
    # errors: none of them changes a column
    for bad in (V[:-1], np.zeros(n, np.float32), np.full(n, 2 ** 31, np.int64), np.zeros((n, 1), np.int32)):
        with pytest.raises(ValueError):
            ix.set_column("year", bad)
    with pytest.raises(ValueError):
        ix.set_column("label", V)
    with pytest.raises(ValueError):
        ix.set_column("", V)
    with pytest.raises(ValueError):
        ix.set_column("fresh", V, ids="input")             # no row map
    assert ix.columns == ["year", "price"] and np.array_equal(ix.column("year"), V)
    # a ninth name raises; dropping a column frees its name and its slot
    for i in range(6):
        ix.set_column(f"c{i}", V % 1000 + i)
    assert len(ix.columns) == 8
    with pytest.raises(ValueError):
        ix.set_column("ninth", V)
    ix.set_column("year", W)                               # (an existing name is replaced, not counted again)
    assert np.array_equal(ix.column("year"), W)
    ix.set_column("c3", None)
    assert "c3" not in ix.columns and len(ix.columns) == 7
    with pytest.raises(ValueError):
        ix.column("c3")
    ix.set_column("ninth", V)
    assert np.array_equal(ix.column("ninth"), V) and np.array_equal(ix.column("c4"), V % 1000 + 4)
    ix.set_column("absent", None)                          # dropping what is not there: nothing to do
    # add() with columns raises and says what to do; set_column after add() works at the new size
    X = np.random.default_rng(5).standard_normal((3, DATASETS["g16"]["dim"])).astype(np.float32)
    with pytest.raises(ValueError, match="drop the columns"):
        ix.add(X, labels=[1, 2, 3])
    assert ix.size == n
    for name in ix.columns:
        ix.set_column(name, None)
    assert ix.columns == []
    ix.add(X, labels=[1, 2, 3])
    assert ix.size == n + 3
    V2 = np.concatenate([V, [5, 6, 5]])
    ix.set_column("year", V2)
    assert np.array_equal(ix.column("year"), V2)
    _is(cph, ix.where(year=5, label=(1, 3)), (V2 == 5) & (np.concatenate([L, [1, 2, 3]]) >= 1) & (np.concatenate([L, [1, 2, 3]]) <= 3), n + 3)
    # load drops the columns and clears the names
    ix.load(fixture_path("g16", 1))
    assert ix.columns == [] and not ix.has_labels
    with pytest.raises(ValueError):
        ix.column_filter("year", 5)
    ix.set_column("other", V)                              # the slot is free again
    assert ix.columns == ["other"] and np.array_equal(ix.column("other"), V)


def test_columns_built_index_input_rows_and_compact(cph):
    """The 8,230 x 16 index of test_label_bitmaps_tiles_and_filter_chunks: values given in input rows, every word and
    count against numpy on values[row_map()]; then a remove and compact(), which carries the columns."""
    rng = np.random.default_rng(77)
    n, dim = 8230, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    rows = ix.row_map()
    V_rows, W_rows, L_rows = _values(n, 4), rng.integers(2015, 2026, n), rng.integers(0, 9, n)
    ix.set_column("v", V_rows, ids="input")
    ix.set_column("year", W_rows, ids="input")
    ix.set_labels(L_rows, ids="input")
    assert np.array_equal(ix.column("v", ids="input"), V_rows) and np.array_equal(ix.column("v", ids="internal"), V_rows[rows])
    _check_column_filters(cph, ix, V_rows[rows], BOUNDS, ix.column_filters("v", [b[0] for b in BOUNDS], [b[1] for b in BOUNDS]))
    f = ix.where(label=7, year=(2020, 2024), v=(-1, 5))
    _is(cph, f, ((L_rows == 7) & (W_rows >= 2020) & (W_rows <= 2024) & (V_rows >= -1) & (V_rows <= 5))[rows], n)
    ix.result_ids = "input"
    R = np.zeros(n, bool)
    R[rng.choice(n, 900, replace=False)] = True
    ix.remove(np.flatnonzero(R))
    assert ix.columns == ["v", "year"]                     # a remove leaves them
    ix.compact()
    assert ix.size == n - 900 and ix.columns == ["v", "year"] and ix.has_labels
    assert np.array_equal(ix.column("v"), V_rows[~R]) and np.array_equal(ix.column("year"), W_rows[~R])
    assert np.array_equal(ix.column("year", ids="internal"), W_rows[~R][ix.row_map()])
    g = ix.where(label=7, year=(2020, 2024))
    assert g.count == int(((L_rows == 7) & (W_rows >= 2020) & (W_rows <= 2024))[~R].sum())


def test_columns_replicas_and_parts(cph, built):
    ixs, X, Q, m1, m2 = built
    S, M, P = ixs["S"], ixs["M"], ixs["P"]
    n, k = S.size, 10
    rng = np.random.default_rng(5)
    V, L = rng.integers(2015, 2026, n), rng.integers(0, 4, n)
    (lo0, hi0), (lo1, hi1) = P.parts
    V[lo1 + 50:lo1 + 90] = 1999                            # lives in part 1 only
    mask = (L == 2) & (V >= 2018) & (V <= 2022)
    for ix in (S, M, P):
        ix.set_column("year", V)
        ix.set_labels(L)
        assert ix.columns == ["year"] and np.array_equal(ix.column("year"), V)
    for ix in (M, P):
        f = ix.where(label=2, year=(2018, 2022))
        assert f.count == int(mask.sum())
        for kw in ({}, {"exact": True}):
            _same(ix.search_batch(Q, k, filter=f, **kw), ix.search_batch(Q, k, filter=ix.make_filter(mask), **kw), kw)
        _same(ix.search_batch(Q, k, filter=f, exact=True), S.search_batch(Q, k, filter=S.make_filter(mask), exact=True), "single")
        only1 = ix.column_filter("year", 1999)
        assert only1.count == 40
        ids, _ = ix.search_batch(Q, k, filter=only1, exact=True)
        assert (V[ids[ids >= 0]] == 1999).all() and (ids >= 0).any()
        with pytest.raises(ValueError):
            ix.set_column("year", V[:-1])
    R = np.zeros(n, bool)
    R[rng.choice(n, 60, replace=False)] = True
    R[hi0 - 5:hi0 + 5] = True
    for ix in (M, P):
        ix.remove(np.flatnonzero(R))
        ix.compact()                                       # replicas copy the columns, parts cut them again at the new bounds
        assert ix.size == n - int(R.sum()) and ix.columns == ["year"]
        assert np.array_equal(ix.column("year"), V[~R]) and np.array_equal(ix.labels(), L[~R])
        assert ix.where(label=2, year=(2018, 2022)).count == int(mask[~R].sum())
        ix.build(X)                                        # a build drops them
        ix.finalize()
        assert ix.columns == [] and not ix.has_labels


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_filter_algebra_errors(cph):
    a, b = _load(cph, "g16", 1), _load(cph, "g2048", 1)
    rng = np.random.default_rng(3)
    f, g = a.make_filter(rng.random(a.size) < 0.5), a.make_filter(rng.random(a.size) < 0.5)
    other = b.make_filter(np.ones(b.size, bool))
    with pytest.raises(ValueError):
        f & other                                          # different sizes
    with pytest.raises(ValueError):
        a.combine_filters("or", [f, g], [other, f])
    with pytest.raises(ValueError):
        a.combine_filters("and", [f, g], [f])              # a second operand of the wrong length
    with pytest.raises(ValueError):
        a.combine_filters("and", [f, g], [f, g, f])
    with pytest.raises(ValueError):
        a.combine_filters("and", [f, g])                   # a binary op without a second operand
    with pytest.raises(ValueError):
        a.combine_filters("not", [f], g)                   # "not" with a second operand
    with pytest.raises(ValueError):
        a.combine_filters("nand", [f], g)
    with pytest.raises(ValueError):
        a.combine_filters("and", [f], np.ones(a.size, bool))
    with pytest.raises(TypeError):
        f & np.ones(a.size, bool)
    closed = a.make_filter(np.ones(a.size, bool))
    closed.close()
    for bad in (lambda: f & closed, lambda: closed | f, lambda: ~closed, lambda: a.combine_filters("xor", [f, closed], g)):
        with pytest.raises(ValueError, match="closed"):
            bad()
    h = f & g                                              # the operands are still good after all that
    assert np.array_equal(h.words(), f.words() & g.words())
    # a label= search still refuses filter=, whatever made the filter
    a.set_labels(np.zeros(a.size, np.int32))
    with pytest.raises(ValueError):
        a.search_batch(np.zeros((1, DATASETS["g16"]["dim"]), np.float32), 5, label=0, filter=h)
