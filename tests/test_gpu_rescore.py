"""Two-stage search on the GPU (CPIndex.make_rescore_vectors, search_rescored / search_rescored_device, cph_rescore_rows_hook).

The yardstick is tests/rescore_model.py.  Rows in: the stored bytes of an object (cph_rescore_vectors_get) against the host
statement and the model.  The kernel hook: against the host twin and the model on synthetic candidate rows over loaded golden
indexes.  End to end: a call against the model applied to the rows search_batch(q, C, ...) returns in internal ids on the same
handle, under every option the underlying search takes."""
import ctypes as C

import numpy as np
import pytest

from diverse_model import FMAX, INDEX_ROW_KINDS, index_rows
from golden_util import DATASETS, fixture_path
from rescore_model import (CS, DTYPES, KS, METRICS, Layout, hook_rescore_rows, host_rescore_rows, host_rows_in, rescore_model_batch,
                           rows_in_model, same_bytes, stored_values)

pytestmark = pytest.mark.gpu

FIXTURES = [("g16", 1), ("g128", 4), ("g1024", 2)]
IN_DIMS = (1, 7, 8, 72, 520, 1032)
HOOK_DIMS = (7, 64, 520, 1032)
N_TWINS = 8


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _full_rows(n, dim, seed=0):
    """float32 [n, dim]; the last N_TWINS rows repeat the first ones (equal scores under other ids)."""
    x = np.random.default_rng(1009 * dim + n + seed).standard_normal((n, dim)).astype(np.float32)
    x[n - N_TWINS:] = x[:N_TWINS]
    return x


def _built(cph, dim, bits, rows, **kw):
    ix = cph.CPIndex(dim, bits, **kw)
    ix.build(rows)
    ix.finalize()
    return ix


class Objects:
    """The RescoreVectors of one index, made on first use, with the model's view of each: (rv, L, stored, norms, X)."""

    def __init__(self, ix):
        self.ix, self.made = ix, {}

    def __call__(self, dim, dtype, metric):
        key = (dim, dtype, metric)
        if key not in self.made:
            full = _full_rows(self.ix.size, dim)
            rv = self.ix.make_rescore_vectors(full, ids="internal", dtype=dtype, metric=metric)
            stored, norms, bad = rows_in_model(full, dtype)
            L = Layout(dim, dtype)
            assert bad.size == 0 and rv.row_bytes == L.stride and (rv.dim, rv.dtype, rv.metric) == key
            assert rv.nbytes == self.ix.size * (L.stride + 4)
            self.made[key] = (rv, L, stored, norms, stored_values(stored, L))
        return self.made[key]


@pytest.fixture(scope="module")
def loaded(cph):
    out = {}
    for name, bits in FIXTURES:
        ix = cph.CPIndex(DATASETS[name]["dim"], bits)
        ix.load(fixture_path(name, bits))
        assert ix.size == DATASETS[name]["n"]
        out[name] = (ix, Objects(ix))
    return out


# ---- rows in -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", IN_DIMS)
def test_rows_in_has_the_bytes_of_the_host_statement(cph, dim, dtype):
    """float32 and float16 input, internal ids and input ids under a row map."""
    ix = cph.CPIndex(DATASETS["g16"]["dim"], 1)
    ix.load(fixture_path("g16", 1))
    n = ix.size
    full = _full_rows(n, dim)
    full[3, 0] = np.float32(65504.0) if dim > 1 else full[3, 0]
    rm = np.random.default_rng(dim).permutation(n)
    ix.set_row_map(rm)
    assert np.array_equal(ix.row_map(), rm)
    for rows in (full, full.astype(np.float16)):
        as32 = rows.astype(np.float32)
        for space, row_map in (("internal", None), ("input", rm.astype(np.uint32))):
            rv = ix.make_rescore_vectors(rows, ids=space, dtype=dtype)
            stored, norms = rv.stored()
            w_stored, w_norms, w_bad = rows_in_model(as32, dtype, row_map)
            h_stored, h_norms, h_bad, _ = host_rows_in(as32, dtype, row_map)
            assert w_bad.size == 0 and h_bad == 0
            assert stored.tobytes() == h_stored.tobytes() == w_stored.tobytes(), (rows.dtype, space)
            assert norms.tobytes() == h_norms.tobytes() == w_norms.tobytes(), (rows.dtype, space)
            part = rv.stored(5, 7)
            assert part[0].tobytes() == stored[5:12].tobytes() and part[1].tobytes() == norms[5:12].tobytes()
            rv.close()
    ix.result_ids = "input"                                # ids=None follows result_ids, as make_group_keys does
    rv = ix.make_rescore_vectors(full, dtype=dtype)
    assert rv.stored()[0].tobytes() == rows_in_model(full, dtype, rm)[0].tobytes()
    rv.close()


def test_bad_rows_are_refused_and_no_object_is_made(cph):
    from cphnsw_mi355x import _lib
    ix = cph.CPIndex(DATASETS["g16"]["dim"], 1)
    ix.load(fixture_path("g16", 1))
    n = ix.size
    full = _full_rows(n, 24)
    full[211, 5] = np.nan
    full[17, 23] = np.float32(70000.0)
    with pytest.raises(ValueError, match=r"row 17 .*\(2 such rows"):
        ix.make_rescore_vectors(full, ids="internal", dtype="float16")
    with pytest.raises(ValueError, match=r"row 211 .*\(1 such row "):
        ix.make_rescore_vectors(full, ids="internal", dtype="float32")
    out = C.c_void_p(12345)
    rc = _lib.lib().cph_rescore_vectors_create(ix._h, full.ctypes.data, n, 24, _lib.IDS_INTERNAL, _lib.RESCORE_FLOAT16, _lib.RESCORE_L2, C.byref(out))
    assert rc == _lib.INVALID_ARGUMENT and not out.value
    full[211, 5], full[17, 23] = 1.0, np.float32(65504.0)
    ix.make_rescore_vectors(full, ids="internal", dtype="float16").close()
    for bad in (dict(rows=full[:-1]), dict(rows=full.astype(np.float64)), dict(rows=np.zeros((n, 8193), np.float32)), dict(dtype="bfloat16"),
                dict(metric="cosine"), dict(ids="input")):                       # (no row map: the input form needs one)
        kw = dict(rows=full, ids="internal")
        kw.update(bad)
        with pytest.raises(ValueError):
            ix.make_rescore_vectors(kw.pop("rows"), **kw)


# ---- the kernel against the host twin and the model ------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", CS)
@pytest.mark.parametrize("name,bits", FIXTURES)
def test_kernel_hook_matches_host_twin_and_model(loaded, name, bits, Cn):
    """n = 1, 3 and 130 rows (more than one workgroup) at every k that fits; C capped by the index; dim_full, dtype and metric
    cycle: every dim_full meets both dtypes on every index (13 of the 16 combinations each; all 16 run in the next test)."""
    ix, objects = loaded[name]
    n_ids = ix.size
    Cn = min(Cn, n_ids)
    combos = [(d, t, m) for d in HOOK_DIMS for t in DTYPES for m in METRICS]
    for i, k in enumerate(sorted(set(x for x in KS + (Cn,) if x <= Cn))):
        dim, dtype, metric = combos[(5 * (CS.index(Cn) if Cn in CS else len(CS)) + 3 * i + len(name)) % len(combos)]
        rv, L, stored, norms, X = objects(dim, dtype, metric)
        for n, first in ((1, 3), (3, 1), (130, 0)):
            if n == 130 and k > 64:
                continue                                   # (the model's time; k = C has n = 1 and 3)
            ids, dist, kinds = index_rows(n_ids, Cn, k, n, seed=n, first=first)
            assert ids.shape == (n, Cn) and (n < len(INDEX_ROW_KINDS) or set(kinds) == set(INDEX_ROW_KINDS))
            if Cn >= 2 and kinds[0] == "plain":
                ids[0, 0], ids[0, 1] = n_ids - N_TWINS, 0  # twins: equal scores, the lower id first
            if Cn >= 3:
                ids[n - 1, Cn // 2] = n_ids + 3            # an id beyond the index counts as padding
            fq = np.random.default_rng(n + k).standard_normal((n, dim)).astype(np.float32)
            want = rescore_model_batch(ids, dist, k, fq, X, norms, L, metric, n_ids)
            assert same_bytes(host_rescore_rows(ids, dist, k, fq, stored, norms, dtype, metric), want), (name, Cn, k, dim, dtype, metric, n)
            got = hook_rescore_rows(ix, rv, ids, dist, k, fq)
            # no slot was left alone: the hook's outputs start as 0xA5 bytes
            assert not (got[0] == np.int64(-0x5A5A5A5A5A5A5A5B)).any()
            assert not (got[1].view(np.uint32) == 0xA5A5A5A5).any() and not (got[2].view(np.uint32) == 0xA5A5A5A5).any()
            assert same_bytes(got, want), (name, Cn, k, dim, dtype, metric, n)


def test_kernel_hook_every_layout_the_row_map_and_bad_queries(loaded):
    ix, objects = loaded["g128"]
    n_ids = ix.size
    ids, dist, _ = index_rows(n_ids, 65, 10, 20, seed=9)
    for dim in HOOK_DIMS:
        for dtype in DTYPES:
            for metric in METRICS:
                rv, L, stored, norms, X = objects(dim, dtype, metric)
                fq = np.random.default_rng(dim).standard_normal((20, dim)).astype(np.float32)
                fq[0, dim // 2], fq[1, 0], fq[2, :] = np.nan, np.inf, np.float32(3e19)       # no finite norm: padding
                want = rescore_model_batch(ids, dist, 10, fq, X, norms, L, metric, n_ids)
                assert (want[0][:3] == -1).all() and (want[1][:3] == FMAX).all()
                assert same_bytes(hook_rescore_rows(ix, rv, ids, dist, 10, fq), want), (dim, dtype, metric)
    rows = np.random.default_rng(5).permutation(n_ids)
    rv, L, stored, norms, X = objects(64, "float16", "l2")
    fq = np.random.default_rng(1).standard_normal((20, 64)).astype(np.float32)
    ix.set_row_map(rows)
    ix.result_ids = "input"
    try:
        want = rescore_model_batch(ids, dist, 10, fq, X, norms, L, "l2", n_ids, rows)
        assert same_bytes(hook_rescore_rows(ix, rv, ids, dist, 10, fq), want)
        assert same_bytes(host_rescore_rows(ids, dist, 10, fq, stored, norms, "float16", "l2", rows.astype(np.uint32)), want)
    finally:
        ix.result_ids = "internal"
        ix.set_row_map(None)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _rows_internal(ix, Q, C_, **kw):
    """The candidate rows of the statement: search_batch at k = C in internal ids on the same handle."""
    was = ix.result_ids
    ix.result_ids = "internal"
    try:
        return ix.search_batch(Q, C_, **kw)
    finally:
        ix.result_ids = was


def _expect(ix, obj, Q, FQ, k, C_, **kw):
    rv, L, stored, norms, X = obj
    ids, dist = _rows_internal(ix, Q, C_, **kw)
    rows = ix.row_map() if ix.result_ids == "input" else None
    return rescore_model_batch(ids, dist, k, FQ, X, norms, L, rv.metric, ix.size, rows)


def _object_over(ix, full, dtype, metric):
    rv = ix.make_rescore_vectors(full, ids="internal", dtype=dtype, metric=metric)
    stored, norms, _ = rows_in_model(full, dtype)
    L = Layout(full.shape[1], dtype)
    return (rv, L, stored, norms, stored_values(stored, L))


def _prefix_data(ix, dim_full, nq, seed):
    """Full rows whose first ix.dim coordinates are the index' own rows, and full queries near some of them."""
    rng = np.random.default_rng(seed)
    full = rng.standard_normal((ix.size, dim_full)).astype(np.float32) * np.float32(0.5)
    full[:, :ix.dim] = ix.get_vectors()
    FQ = full[rng.integers(0, ix.size, nq)] + np.float32(0.3) * rng.standard_normal((nq, dim_full)).astype(np.float32)
    return full, np.ascontiguousarray(FQ)


@pytest.mark.parametrize("state", ("plain", "input", "removed"))
def test_end_to_end_options(cph, state):
    import torch
    name, bits = "g128", 4
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits))
    n, dim = ix.size, ix.dim
    rng = np.random.default_rng(len(state))
    full, FQ = _prefix_data(ix, 200, 12, 7)
    Q = np.ascontiguousarray(FQ[:, :dim])
    key_of = rng.integers(0, 5, n)
    ix.set_labels(key_of, ids="internal")
    if state == "input":
        ix.set_row_map(rng.permutation(n))
        ix.result_ids = "input"
    if state == "removed":
        gone = rng.choice(n, n // 5, replace=False)
        assert ix.remove(gone, ids="internal") == len(gone)
    objs = {(t, m): _object_over(ix, full, t, m) for t, m in (("float16", "l2"), ("float32", "ip"))}
    f = ix.make_filter(rng.random(n) < 0.4, ids="internal")
    f2 = ix.make_filter(rng.random(n) < 0.08, ids="internal")
    empty = ix.make_filter(np.zeros(n, bool), ids="internal")
    fo = rng.integers(-1, 2, len(Q))
    lab = key_of[rng.integers(0, n, len(Q))]
    variants = [dict(), dict(exact=True), dict(filter=f), dict(filter=f, exact=True), dict(filter=empty), dict(label=0), dict(label=lab),
                dict(label=lab, exact=True), dict(filter=[f, f2], filter_of=fo), dict(filter=[f, f2], filter_of=fo, exact=True)]
    FQd = torch.from_numpy(FQ).cuda()
    Qd = torch.from_numpy(Q).cuda()
    reordered = False
    for j, (k, C_) in enumerate(((1, 1), (3, 17), (10, 70), (10, 64), (8, 130))):
        obj = objs[("float16", "l2") if j % 2 == 0 else ("float32", "ip")]
        for kw in variants:
            got = ix.search_rescored(Q, k, obj[0], full_queries=FQ, candidates=C_, **kw)
            assert got[0].shape == got[1].shape == got[2].shape == (len(Q), k)
            want = _expect(ix, obj, Q, FQ, k, C_, **kw)
            assert same_bytes(got, want), (state, k, C_, sorted(kw))
            # the prefix form and the device form give the same bytes
            assert same_bytes(ix.search_rescored(FQ, k, obj[0], candidates=C_, **kw), want), (state, k, C_, sorted(kw), "prefix")
            dev = ix.search_rescored_device(Qd, k, obj[0], full_queries=FQd, candidates=C_, **kw)
            torch.cuda.synchronize()
            assert same_bytes([t.cpu().numpy() for t in dev], want), (state, k, C_, sorted(kw), "device")
            if not kw and C_ == 70:
                first = _rows_internal(ix, Q, C_)[1][:, :k]
                reordered |= bool((got[2] != first).any())
    assert reordered, "no query shows a reordering by the full rows"
    dev = ix.search_rescored_device(FQd, 5, objs[("float16", "l2")][0], candidates=40)       # the prefix is made on the device
    torch.cuda.synchronize()
    assert same_bytes([t.cpu().numpy() for t in dev], ix.search_rescored(Q, 5, objs[("float16", "l2")][0], full_queries=FQ, candidates=40))
    # candidates=None: one pass at C = min(1024, max(64, 4 k))
    obj = objs[("float16", "l2")]
    assert same_bytes(ix.search_rescored(Q, 10, obj[0], full_queries=FQ), ix.search_rescored(Q, 10, obj[0], full_queries=FQ, candidates=64))
    assert same_bytes(ix.search_rescored(Q, 20, obj[0], full_queries=FQ), ix.search_rescored(Q, 20, obj[0], full_queries=FQ, candidates=80))
    # exact=True with C >= the live rows: the model over all live ids
    live = np.flatnonzero(~ix.removed_mask(ids="internal"))
    all_ids = np.tile(live, (len(Q), 1))
    rows = ix.row_map() if state == "input" else None
    for obj in objs.values():
        rv, L, stored, norms, X = obj
        got = ix.search_rescored(Q, 10, rv, full_queries=FQ, candidates=n, exact=True)
        want = rescore_model_batch(all_ids, np.zeros(all_ids.shape, np.float32), 10, FQ, X, norms, L, rv.metric, n, rows)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (state, rv.dtype, rv.metric)
    for x in (f, f2, empty):
        x.close()


def test_device_variant_streams_out_and_timer(cph):
    import torch
    ix = cph.CPIndex(DATASETS["g16"]["dim"], 1)
    ix.load(fixture_path("g16", 1))
    full, FQ = _prefix_data(ix, 72, 12, 3)
    Q = np.ascontiguousarray(FQ[:, :ix.dim])
    rv = ix.make_rescore_vectors(full, ids="internal")
    dev = torch.device("cuda", 0)
    Qd, FQd = torch.from_numpy(Q).to(dev), torch.from_numpy(FQ).to(dev)
    k, C_ = 5, 40
    st1, st2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for st in (st1, st2):
        st.wait_stream(torch.cuda.current_stream(dev))
    want = ix.search_rescored(Q, k, rv, full_queries=FQ, candidates=C_)
    out = (torch.full((len(Q), k), -9, dtype=torch.int64, device=dev), torch.full((len(Q), k), -9.0, device=dev),
           torch.full((len(Q), k), -9.0, device=dev))
    st1.wait_stream(torch.cuda.current_stream(dev))
    res = ix.search_rescored_device(Qd, k, rv, full_queries=FQd, candidates=C_, out=out, stream=st1)
    with torch.cuda.stream(st1):
        copies = [t.clone() for t in res]
    st1.synchronize()
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
    assert same_bytes([t.cpu().numpy() for t in copies], want)
    # two batches on two streams, one of them in the prefix form
    want_b = ix.search_rescored(Q[::-1].copy(), 7, rv, full_queries=FQ[::-1].copy(), candidates=90, exact=True)
    FQr = torch.from_numpy(FQ[::-1].copy()).to(dev)
    torch.cuda.synchronize()
    for _ in range(3):
        a = ix.search_rescored_device(Qd, k, rv, full_queries=FQd, candidates=C_, stream=st1)
        b = ix.search_rescored_device(FQr, 7, rv, candidates=90, exact=True, stream=st2)
        with torch.cuda.stream(st1):
            ca = [t.clone() for t in a]
        with torch.cuda.stream(st2):
            cb = [t.clone() for t in b]
        st1.synchronize()
        st2.synchronize()
        assert same_bytes([t.cpu().numpy() for t in ca], want) and same_bytes([t.cpu().numpy() for t in cb], want_b)
    ix.synchronize()
    with pytest.raises(ValueError):
        ix.last_rescored_us()
    ix.time_rescored(True)
    ix.search_rescored(Q, k, rv, full_queries=FQ, candidates=C_)
    assert ix.last_rescored_us() > 0
    ix.time_rescored(False)
    rv.close()
    with pytest.raises(ValueError, match="closed"):
        ix.search_rescored(Q, k, rv, full_queries=FQ)


def test_cosine_index(cph):
    rng = np.random.default_rng(31)
    n, dim, dim_full = 1500, 24, 96
    full = rng.standard_normal((n, dim_full)).astype(np.float32)
    ix = _built(cph, dim, 4, np.ascontiguousarray(full[:, :dim]), metric="cosine")
    assert ix.metric == "cosine"
    # cosine at full width: unit rows and unit queries under "ip"
    unit = full / np.linalg.norm(full, axis=1, keepdims=True)
    by_input = ix.make_rescore_vectors(unit, ids="input", dtype="float32", metric="ip")
    FQ = unit[rng.integers(0, n, 10)] + np.float32(0.1) * rng.standard_normal((10, dim_full)).astype(np.float32)
    FQ = np.ascontiguousarray(FQ / np.linalg.norm(FQ, axis=1, keepdims=True), np.float32)
    Q = np.ascontiguousarray(FQ[:, :dim])
    assert by_input.stored()[0].tobytes() == rows_in_model(unit, "float32", ix.row_map())[0].tobytes()
    obj = _object_over(ix, np.ascontiguousarray(unit[ix.row_map()]), "float32", "ip")
    assert obj[0].stored()[0].tobytes() == by_input.stored()[0].tobytes()
    for kw in (dict(), dict(exact=True)):
        for space in ("internal", "input"):
            ix.result_ids = space
            got = ix.search_rescored(Q, 10, by_input, full_queries=FQ, candidates=64, **kw)
            assert same_bytes(got, _expect(ix, obj, Q, FQ, 10, 64, **kw)), (space, sorted(kw))
            assert same_bytes(ix.search_rescored(FQ, 10, obj[0], candidates=64, **kw), got)
    ix.result_ids = "input"
    got = ix.search_rescored(Q, 1, by_input, full_queries=FQ, candidates=1024, exact=True)
    cos = (unit.astype(np.float64) @ FQ.astype(np.float64).T).T
    assert (np.abs(-got[1][:, 0] - cos[np.arange(10), got[0][:, 0]]) < 1e-5).all()


# ---- replicas, siblings and refusals ---------------------------------------------------------------------------------------
def test_replicas_equal_one_device(cph):
    name, bits = "g16", 1
    one = cph.CPIndex(DATASETS[name]["dim"], bits)
    one.load(fixture_path(name, bits))
    rows = np.random.default_rng(5).permutation(one.size)
    one.set_row_map(rows)
    m = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0])
    m.set_min_shard(1)
    m.load(fixture_path(name, bits))
    m.set_row_map(rows)
    n = one.size
    full, FQ = _prefix_data(one, 72, 9, 11)
    Q = np.ascontiguousarray(FQ[:, :one.dim])
    mask = np.arange(n) % 4 != 1
    fo = np.arange(len(Q)) % 3 - 1
    for ix in (one, m):
        ix.set_labels(np.arange(n) % 3, ids="internal")
    for ids in ("internal", "input"):
        one.result_ids = m.result_ids = ids
        src = full if ids == "internal" else np.ascontiguousarray(full[np.argsort(rows)])      # the same object either way
        r1, rm = one.make_rescore_vectors(src), m.make_rescore_vectors(src)
        assert len(rm._hs) == 2 and rm.nbytes == 2 * r1.nbytes
        assert rm.stored(replica=1)[0].tobytes() == r1.stored()[0].tobytes() == rows_in_model(full, "float16")[0].tobytes()
        f1, fm = one.make_filter(mask, ids="internal"), m.make_filter(mask, ids="internal")
        e1, em = one.make_filter(~mask, ids="internal"), m.make_filter(~mask, ids="internal")
        for kw1, kwm in ((dict(), dict()), (dict(exact=True), dict(exact=True)), (dict(filter=f1), dict(filter=fm)),
                         (dict(filter=[f1, e1], filter_of=fo), dict(filter=[fm, em], filter_of=fo)), (dict(label=0), dict(label=0))):
            for cand in (40, None):
                assert same_bytes(m.search_rescored(Q, 6, rm, full_queries=FQ, candidates=cand, **kwm),
                                  one.search_rescored(Q, 6, r1, full_queries=FQ, candidates=cand, **kw1)), (ids, sorted(kw1), cand)
        with pytest.raises(ValueError, match="replicas"):
            m.search_rescored(Q, 6, r1, full_queries=FQ)
        for x in (f1, fm, e1, em, r1, rm):
            x.close()


def test_siblings_keep_their_bytes(cph, gold):
    ix = cph.CPIndex(DATASETS["g16"]["dim"], 1)
    ix.load(fixture_path("g16", 1))
    n = ix.size
    ix.set_labels(np.arange(n) % 7, ids="internal")
    Q = gold["Q/g16"][:12]
    T = np.ascontiguousarray(Q.reshape(4, 3, -1))

    def siblings():
        return (ix.search_grouped(Q, 5, 2, candidates=40) + ix.search_diverse(Q, 5, 0.5, candidates=40) +
                ix.search_maxsim(T, 4, candidates=30) + ix.search_batch(Q, 10))
    before = siblings()
    full, FQ = _prefix_data(ix, 72, 12, 2)
    rv = ix.make_rescore_vectors(full, ids="internal")
    for C_ in (40, 200):
        ix.search_rescored(np.ascontiguousarray(FQ[:, :ix.dim]), 5, rv, full_queries=FQ, candidates=C_)
        ix.search_rescored(FQ, 5, rv, candidates=C_, exact=True)
    assert same_bytes(siblings(), before)
    rv.close()
    assert same_bytes(siblings(), before)


def test_refusals_write_nothing(cph):
    import torch
    from cphnsw_mi355x import _lib
    name, bits = "g16", 1
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits))
    full, FQ = _prefix_data(ix, 72, 9, 5)
    Q = np.ascontiguousarray(FQ[:, :ix.dim])
    rv = ix.make_rescore_vectors(full, ids="internal")
    for bad in (dict(k=0), dict(k=65, candidates=64), dict(candidates=1025), dict(k=1025), dict(vectors=None), dict(vectors=full),
                dict(full_queries=FQ[:, :70]), dict(full_queries=FQ[:5]), dict(filter=[ix.make_filter(np.ones(ix.size, bool))] * 2)):
        kw = dict(k=3, vectors=rv, full_queries=FQ, candidates=20)
        kw.update(bad)
        with pytest.raises(ValueError):
            ix.search_rescored(Q, **kw)
    with pytest.raises(ValueError):
        ix.search_rescored(Q[:, :5], 3, rv)              # the prefix form needs at least dim coordinates
    with pytest.raises(ValueError, match="coordinates"):
        ix.search_rescored(Q, 3, rv)                     # ... and dim_full of them
    p = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0], partition=True)
    with pytest.raises(ValueError, match=r"partitioned.*part\(i\)\.search_rescored"):
        p.search_rescored(Q, 6, rv, full_queries=FQ)
    with pytest.raises(ValueError, match="partitioned"):
        p.search_rescored_device(torch.from_numpy(Q).cuda(), 6, rv, full_queries=torch.from_numpy(FQ).cuda())
    with pytest.raises(ValueError, match="partitioned"):
        p.make_rescore_vectors(full)
    # an inner-product index
    rng = np.random.default_rng(3)
    X = rng.standard_normal((600, ix.dim)).astype(np.float32)
    ipx = _built(cph, ix.dim, 4, X, metric="ip")
    rv_ip = ipx.make_rescore_vectors(rng.standard_normal((600, 72)).astype(np.float32), ids="internal")
    # another index; the same index after add() (the size message) and after compact() (another index)
    other = cph.CPIndex(DATASETS[name]["dim"], bits)
    other.load(fixture_path(name, bits))
    grown = cph.CPIndex(DATASETS[name]["dim"], bits)
    grown.load(fixture_path(name, bits))
    rv_grown = grown.make_rescore_vectors(full, ids="internal")
    grown.add(grown.get_vectors(0, 1))
    packed = cph.CPIndex(DATASETS[name]["dim"], bits)
    packed.load(fixture_path(name, bits))
    rv_packed = packed.make_rescore_vectors(full, ids="internal")
    packed.compact()
    assert packed.size == ix.size
    L, N, k = _lib.lib(), len(Q), 3
    refused = [(ipx._h, rv_ip, k, 20, 72, b"inner-product"), (other._h, rv, k, 20, 72, b"another index"), (grown._h, rv_grown, k, 20, 72, b"cover 300 ids"),
               (packed._h, rv_packed, k, 20, 72, b"another index"), (ix._h, rv, 21, 20, 72, b"k <= candidates"), (ix._h, rv, k, 1025, 72, b"1024"),
               (ix._h, rv, k, 20, 70, b"70 coordinates"), (ix._h, rv, 0, 20, 72, b"k >= 1")]
    q = torch.from_numpy(Q).cuda()
    fq = torch.from_numpy(FQ).cuda()
    for (h, obj, kk, C_, width, why) in refused:
        ids, score, first = np.full((N, k), -7, np.int64), np.full((N, k), -7.0, np.float32), np.full((N, k), -7.0, np.float32)
        rc = L.cph_search_rescored(h, Q.ctypes.data, N, FQ.ctypes.data, width, kk, C_, obj._hs[0], None, 0, None, 0, ids.ctypes.data,
                                   score.ctypes.data, first.ctypes.data)
        assert rc == _lib.INVALID_ARGUMENT and why in L.cph_last_error(), (why, L.cph_last_error())
        assert (ids == -7).all() and (score == -7.0).all() and (first == -7.0).all()
        d_ids = torch.full((N, k), -7, dtype=torch.int64, device="cuda")
        d_score = torch.full((N, k), -7.0, device="cuda")
        d_first = torch.full((N, k), -7.0, device="cuda")
        torch.cuda.synchronize()
        rc = L.cph_search_rescored_device(h, q.data_ptr(), N, fq.data_ptr(), width, kk, C_, obj._hs[0], None, 0, None, 0, d_ids.data_ptr(),
                                          d_score.data_ptr(), d_first.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == _lib.INVALID_ARGUMENT and why in L.cph_last_error(), why
        torch.cuda.synchronize()
        assert (d_ids == -7).all() and (d_score == -7.0).all() and (d_first == -7.0).all()
    for (obj, owner) in ((rv_grown, grown), (rv_packed, packed), (rv, other)):
        with pytest.raises(ValueError):
            owner.search_rescored(Q, 3, obj, full_queries=FQ)
    # the hook refuses a foreign object too
    with pytest.raises(ValueError, match="another index"):
        hook_rescore_rows(other, rv, np.zeros((1, 4), np.int64), np.zeros((1, 4), np.float32), 2, FQ[:1])
    for x in (rv, rv_ip, rv_grown, rv_packed):
        x.close()
