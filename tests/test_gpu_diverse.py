"""Diversified search on the GPU (CPIndex.search_diverse / search_diverse_device, cph_diverse_rows_hook).

The yardstick is tests/diverse_model.py with the pair distance ix.exact_l2(ix.get_vectors(s, 1)[0], ids): the kernel hook
is compared with it and with the host twin on synthetic rows over loaded golden indexes; an end-to-end call is compared
with the model applied to the rows search_batch(q, C, ...) returns in internal ids on the same handle, under every option
the underlying search takes."""
import ctypes as C

import numpy as np
import pytest

from diverse_model import (CS, FMAX, INDEX_ROW_KINDS, KS, LAMS, diverse_model_batch, hook_diverse_rows, host_diverse_rows,
                           index_rows, read_v2_vectors, same_bytes)
from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

FIXTURES = [("g16", 1), ("g128", 4), ("g1024", 2)]        # D = 16 (the short loop), 128 (one chunk), 1024 (eight chunks)
STATES = ("plain", "input", "removed", "added")


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


class IndexPairs:
    """pair(s, js) = ix.exact_l2(ix.get_vectors(s, 1)[0], js): asked once per s for every id, then served from the table.
    Made anew after the index changed size."""

    def __init__(self, ix):
        self.ix, self.all, self.rows = ix, np.arange(ix.size), {}

    def __call__(self, s, js):
        if s not in self.rows:
            self.rows[s] = self.ix.exact_l2(self.ix.get_vectors(s, 1)[0], self.all)
        return self.rows[s][np.asarray(js, np.int64)]


# ---- the kernel against the host twin and the model -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def loaded(cph):
    """Every golden index of FIXTURES, loaded once, with its vectors and norms as the file holds them and its pair table."""
    out = {}
    for name, bits in FIXTURES:
        spec = DATASETS[name]
        ix = cph.CPIndex(spec["dim"], bits)
        ix.load(fixture_path(name, bits))
        raw, norm = read_v2_vectors(fixture_path(name, bits), spec["n"], spec["dim"], spec["D"])
        assert ix.size == spec["n"] and np.array_equal(ix.get_vectors(), raw[:, :spec["dim"]])
        out[name] = (ix, raw, norm, IndexPairs(ix))
    return out


@pytest.mark.parametrize("Cn", CS)
@pytest.mark.parametrize("name,bits", FIXTURES)
def test_kernel_hook_matches_host_twin_and_model(loaded, name, bits, Cn):
    """n = 1, 3 and 130 rows (more than one workgroup; every row kind 26 times) at every k that fits; C capped by the index."""
    ix, raw, norm, pairs = loaded[name]
    n_ids = ix.size
    Cn = min(Cn, n_ids)
    for i, k in enumerate(sorted(set(x for x in KS + (Cn,) if x <= Cn))):
        lam = LAMS[(i + Cn) % len(LAMS)]
        for n, first in ((1, 3), (3, 1), (130, 0)):
            if n == 130 and k > 64:
                continue                                   # (the model's time; k = C has n = 1 and 3)
            ids, dist, kinds = index_rows(n_ids, Cn, k, n, seed=n, first=first)
            assert ids.shape == (n, Cn) and (n < len(INDEX_ROW_KINDS) or set(kinds) == set(INDEX_ROW_KINDS))
            want = diverse_model_batch(ids, dist, k, lam, pairs, n_ids)
            assert same_bytes(host_diverse_rows(ids, dist, raw, norm, k, lam), want), (name, Cn, k, lam, n, "host twin")
            got = hook_diverse_rows(ix, ids, dist, k, lam)
            # no slot was left alone: the hook's outputs start as 0xA5 bytes
            assert not (got[0] == np.int64(-0x5A5A5A5A5A5A5A5B)).any()
            assert not (got[1].view(np.uint32) == 0xA5A5A5A5).any() and not (got[2].view(np.uint32) == 0xA5A5A5A5).any()
            assert same_bytes(got, want), (name, Cn, k, lam, n)


def test_kernel_hook_every_lam_and_the_row_map(loaded):
    ix, raw, norm, pairs = loaded["g128"]
    n_ids = ix.size
    ids, dist, _ = index_rows(n_ids, 65, 10, 20, seed=9)
    ids[0, 7] = n_ids + 3                                  # an id beyond the index counts as padding
    picks = []
    for lam in LAMS:
        want = diverse_model_batch(ids, dist, 10, lam, pairs, n_ids)
        assert same_bytes(hook_diverse_rows(ix, ids, dist, 10, lam), want), lam
        picks.append(want[0])
    assert not np.array_equal(picks[0], picks[2]) and not np.array_equal(picks[2], picks[4])      # lam matters
    assert (picks[2][:, 1] != ids[:, 1]).any(), "no row shows a reordering at lam = 0.5"
    rows = np.random.default_rng(5).permutation(n_ids)
    ix.set_row_map(rows)
    ix.result_ids = "input"
    try:
        want = diverse_model_batch(ids, dist, 10, 0.5, pairs, n_ids, rows)
        assert same_bytes(hook_diverse_rows(ix, ids, dist, 10, 0.5), want)
        assert same_bytes(host_diverse_rows(ids, dist, raw, norm, 10, 0.5, rows.astype(np.uint32)), want)
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


def _expect(ix, pairs, Q, k, lam, C_, **kw):
    ids, dist = _rows_internal(ix, Q, C_, **kw)
    rows = ix.row_map() if ix.result_ids == "input" else None
    return diverse_model_batch(ids, dist, k, lam, pairs, ix.size, rows)


@pytest.fixture(scope="module")
def built(cph, tmp_path_factory):
    """8,230 x 16 at 1 bit, as tests/test_gpu_grouped.py builds it, saved once; every test loads its own copy.  The first
    2,000 input rows are one tight cluster: a candidate row of a query in it is full of near copies."""
    rng = np.random.default_rng(77)
    n, dim = 8230, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[:2000] = np.float32(6.0) + np.float32(0.05) * X[:2000]
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    path = str(tmp_path_factory.mktemp("diverse") / "built.cphn")
    ix.save_native(path)
    Q = rng.standard_normal((12, dim)).astype(np.float32)
    Q[:4] = np.float32(6.0) + np.float32(0.05) * Q[:4]
    return dict(path=path, X=X, Q=Q, dim=dim)


@pytest.mark.parametrize("state", STATES)
def test_end_to_end_options(cph, built, state):
    ix = cph.CPIndex(built["dim"], 1)
    ix.load_native(built["path"])
    Q = built["Q"].copy()
    n0 = ix.size
    rng = np.random.default_rng(n0 + len(state))
    key_of = rng.integers(0, 5, n0)
    ix.set_labels(key_of, ids="internal")
    if state == "input":
        ix.result_ids = "input"
    if state in ("removed", "added"):
        gone = rng.choice(n0, n0 // 5, replace=False)
        assert ix.remove(gone, ids="internal") == len(gone)
    if state == "added":
        # a twin of base row 5 (m = 0 against it), a near copy, and fresh rows; query 5 IS one of the fresh rows
        twin = ix.get_vectors(5, 1)
        extra = np.concatenate([twin, twin + np.float32(0.25), rng.standard_normal((6, ix.dim)).astype(np.float32)])
        extra_keys = rng.integers(0, 5, len(extra))
        ix.add(extra, labels=extra_keys)
        key_of = np.concatenate([key_of, extra_keys])
        Q[5] = extra[4]
        Q[6] = twin[0]
    n = ix.size
    pairs = IndexPairs(ix)
    mask = rng.random(n) < 0.4
    small = rng.random(n) < 0.08
    f = ix.make_filter(mask, ids="internal")
    f2 = ix.make_filter(small, ids="internal")
    empty = ix.make_filter(np.zeros(n, bool), ids="internal")
    fo = rng.integers(-1, 2, len(Q))
    assert set(fo.tolist()) == {-1, 0, 1}
    lab = key_of[rng.integers(0, n, len(Q))]
    variants = [dict(), dict(exact=True), dict(filter=f), dict(filter=f, exact=True), dict(filter=empty), dict(label=0),
                dict(label=lab, exact=True), dict(filter=[f, f2], filter_of=fo, exact=True)]
    if state == "added":
        # inherited: per-query filters (a label per query is that) would walk the graph of an index with a tail
        with pytest.raises(NotImplementedError):
            ix.search_diverse(Q, 3, candidates=17, filter=[f, f2], filter_of=np.zeros(len(Q), np.int64))
    else:
        variants += [dict(label=lab), dict(filter=[f, f2], filter_of=fo)]
    tail_picked = reordered = False
    for (k, lam, C_) in ((1, 0.5, 1), (3, 0.3, 17), (10, 0.5, 70), (10, 0.0, 64), (8, 1.0, 130)):
        for kw in variants:
            got = ix.search_diverse(Q, k, lam, candidates=C_, **kw)
            assert got[0].shape == got[1].shape == got[2].shape == (len(Q), k)
            assert same_bytes(got, _expect(ix, pairs, Q, k, lam, C_, **kw)), (state, k, lam, C_, sorted(kw))
            if not kw and state == "added":
                tail_picked |= bool((got[0] >= n0).any())
            if not kw and C_ == 70:
                rows = _rows_internal(ix, Q, C_)[0]
                shown = got[0] if state != "input" else np.argsort(ix.row_map())[got[0]]
                reordered |= bool((shown[:, 1] != rows[:, 1]).any())
    assert reordered, "no query shows a reordering at lam = 0.5"
    # candidates=None: one pass at C = min(1024, max(64, 4 k))
    assert same_bytes(ix.search_diverse(Q, 10, 0.5), ix.search_diverse(Q, 10, 0.5, candidates=64))
    assert same_bytes(ix.search_diverse(Q, 20, 0.7, exact=True), ix.search_diverse(Q, 20, 0.7, candidates=80, exact=True))
    if state == "added":
        assert tail_picked, "no tail row among the picks"
        got = ix.search_diverse(Q[6:7], 4, 1.0, candidates=16, exact=True)
        if not ix.removed_mask(ids="internal")[5]:
            assert set(got[0][0, :2].tolist()) == {5, n0}       # row 5 and its twin in the tail, both at the query
    for x in (f, f2, empty):
        x.close()


def test_lam_one_is_the_plain_search_and_stats_are_the_search_s(cph, built):
    ix = cph.CPIndex(built["dim"], 1)
    ix.load_native(built["path"])
    Q, k, C_ = built["Q"], 10, 64
    for space in ("internal", "input"):
        ix.result_ids = space
        rows = _rows_internal(ix, Q, C_, exact=True)[0]
        assert (rows >= 0).all() and all(len(set(r.tolist())) == C_ for r in rows)      # C candidates, no repeats
        ids, dist = ix.search_batch(Q, k, exact=True)
        got = ix.search_diverse(Q, k, 1.0, candidates=C_, exact=True)
        assert got[0].tobytes() == ids.tobytes() and got[1].tobytes() == dist.tobytes()
        assert (got[2][:, 0] == FMAX).all() and (got[2][:, 1:] < FMAX).all()
        assert ix.result_ids == space
    ix.result_ids = "internal"
    # last_search_stats: the underlying search only
    import torch
    Qd = torch.from_numpy(Q).cuda()
    for kw in (dict(), dict(exact=True)):
        ix.search_batch_device(Qd, C_, **kw)         # (the batch a diverse call enqueues is a device-form one)
        ix.synchronize()
        plain = ix.last_search_stats()
        ix.search_diverse(Q, k, 0.5, candidates=C_, **kw)
        after = ix.last_search_stats()
        timed = {x for x in plain if x.endswith("_us")}
        assert {x: v for x, v in plain.items() if x not in timed} == {x: v for x, v in after.items() if x not in timed}
    before = ix.search_batch(Q, 10)
    ix.search_diverse(Q, 4, 0.5)
    assert same_bytes(before, ix.search_batch(Q, 10))


# ---- the device variant ------------------------------------------------------------------------------------------------------
def test_device_variant(cph, gold):
    import torch
    ix = cph.CPIndex(DATASETS["g16"]["dim"], 1)
    ix.load(fixture_path("g16", 1))
    Q = gold["Q/g16"][:12]
    n = ix.size
    ix.set_labels(np.arange(n) % 4, ids="internal")
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    f = ix.make_filter(np.arange(n) % 3 != 0, ids="internal")
    fo = np.arange(len(Q)) % 2 - 1
    k, lam, C_ = 5, 0.5, 40
    cases = [dict(), dict(exact=True), dict(filter=f), dict(filter=[f], filter_of=fo), dict(label=0)]
    st1, st2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for st in (st1, st2):
        st.wait_stream(torch.cuda.current_stream(dev))
    for kw in cases:
        want = ix.search_diverse(Q, k, lam, candidates=C_, **kw)
        got = ix.search_diverse_device(Qd, k, lam, candidates=C_, **kw)
        torch.cuda.synchronize()
        assert same_bytes([t.cpu().numpy() for t in got], want), sorted(kw)
        # out= and a side stream; the results are used in stream order, with no host wait in between
        out = (torch.full((len(Q), k), -9, dtype=torch.int64, device=dev), torch.full((len(Q), k), -9.0, device=dev),
               torch.full((len(Q), k), -9.0, device=dev))
        st1.wait_stream(torch.cuda.current_stream(dev))
        res = ix.search_diverse_device(Qd, k, lam, candidates=C_, out=out, stream=st1, **kw)
        with torch.cuda.stream(st1):
            copies = [t.clone() for t in res]
        st1.synchronize()
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
        assert same_bytes([t.cpu().numpy() for t in copies], want), sorted(kw)
    # default candidates
    got = ix.search_diverse_device(Qd, k, lam)
    torch.cuda.synchronize()
    assert same_bytes([t.cpu().numpy() for t in got], ix.search_diverse(Q, k, lam, candidates=64))
    # two batches on two streams
    want_a = ix.search_diverse(Q, k, lam, candidates=C_)
    want_b = ix.search_diverse(Q[::-1].copy(), 7, 0.3, candidates=90, exact=True)
    Qr = torch.from_numpy(Q[::-1].copy()).to(dev)
    torch.cuda.synchronize()
    for _ in range(3):
        a = ix.search_diverse_device(Qd, k, lam, candidates=C_, stream=st1)
        b = ix.search_diverse_device(Qr, 7, 0.3, candidates=90, exact=True, stream=st2)
        with torch.cuda.stream(st1):
            ca = [t.clone() for t in a]
        with torch.cuda.stream(st2):
            cb = [t.clone() for t in b]
        st1.synchronize()
        st2.synchronize()
        assert same_bytes([t.cpu().numpy() for t in ca], want_a) and same_bytes([t.cpu().numpy() for t in cb], want_b)
    ix.synchronize()
    # the debug timer
    ix.time_diverse(True)
    ix.search_diverse(Q, k, lam, candidates=C_)
    assert ix.last_diverse_rows_us() > 0
    ix.time_diverse(False)
    f.close()


# ---- replicas, parts and refusals ----------------------------------------------------------------------------------------------
def test_replicas_equal_one_device(cph, gold):
    name, bits = "g16", 1
    one = cph.CPIndex(DATASETS[name]["dim"], bits)
    one.load(fixture_path(name, bits))
    rows = np.random.default_rng(5).permutation(one.size)
    one.set_row_map(rows)
    Q = gold[f"Q/{name}"][:9]
    m = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0])
    m.set_min_shard(1)
    m.load(fixture_path(name, bits))
    m.set_row_map(rows)
    n = one.size
    mask = np.arange(n) % 4 != 1
    fo = np.arange(len(Q)) % 3 - 1
    for ix in (one, m):
        ix.set_labels(np.arange(n) % 3, ids="internal")
    for ids in ("internal", "input"):
        one.result_ids = m.result_ids = ids
        f1, fm = one.make_filter(mask, ids="internal"), m.make_filter(mask, ids="internal")
        e1, em = one.make_filter(~mask, ids="internal"), m.make_filter(~mask, ids="internal")
        for kw1, kwm in ((dict(), dict()), (dict(exact=True), dict(exact=True)), (dict(filter=f1), dict(filter=fm)),
                         (dict(filter=[f1, e1], filter_of=fo), dict(filter=[fm, em], filter_of=fo)), (dict(label=0), dict(label=0))):
            for cand in (40, None):
                assert same_bytes(m.search_diverse(Q, 6, 0.5, candidates=cand, **kwm),
                                  one.search_diverse(Q, 6, 0.5, candidates=cand, **kw1)), (ids, sorted(kw1), cand)
        for x in (f1, fm, e1, em):
            x.close()


def test_refusals_write_nothing(cph, gold):
    import torch
    from cphnsw_mi355x import _lib
    name, bits = "g16", 1
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits))
    Q = gold[f"Q/{name}"][:9]
    for bad in (dict(k=0), dict(k=65, candidates=64), dict(candidates=1025), dict(k=1025), dict(lam=-0.1), dict(lam=1.5),
                dict(lam=float("nan")), dict(filter=[ix.make_filter(np.ones(ix.size, bool))] * 2)):
        kw = dict(k=3, lam=0.5, candidates=20)
        kw.update(bad)
        with pytest.raises(ValueError):
            ix.search_diverse(Q, **kw)
    with pytest.raises(ValueError):
        ix.search_diverse(Q[:, :5], 3)
    p = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0], partition=True)
    with pytest.raises(ValueError, match=r"partitioned.*part\(i\)\.search_diverse"):
        p.search_diverse(Q, 6)
    with pytest.raises(ValueError, match="partitioned"):
        p.search_diverse_device(torch.from_numpy(Q).cuda(), 6)
    # through the C entries: rows of sentinels stay untouched
    L, N, k = _lib.lib(), len(Q), 3
    other = cph.CPIndex(DATASETS[name]["dim"], bits)
    other.load(fixture_path(name, bits))
    short = other.make_filter(np.ones(other.size, bool))
    other.add(other.get_vectors(0, 1))                       # `short` no longer covers the index it was made for
    fh = (C.c_void_p * 1)(short._hs[0].value)
    nan = float("nan")
    refused = [(ix._h, 0, 0.5, 20, None, 0), (ix._h, 21, 0.5, 20, None, 0), (ix._h, k, 0.5, 1025, None, 0), (ix._h, k, -0.5, 20, None, 0),
               (ix._h, k, 1.0001, 20, None, 0), (ix._h, k, nan, 20, None, 0), (other._h, k, 0.5, 20, fh, 1), (ix._h, k, 0.5, 20, None, 2)]
    for (h, kk, lam, C_, filters, nf) in refused:
        ids, dist, gap = np.full((N, k), -7, np.int64), np.full((N, k), -7.0, np.float32), np.full((N, k), -7.0, np.float32)
        rc = L.cph_search_diverse(h, Q.ctypes.data, N, kk, lam, C_, filters, nf, None, 0, ids.ctypes.data, dist.ctypes.data,
                                  gap.ctypes.data)
        assert rc == _lib.INVALID_ARGUMENT, (kk, lam, C_, nf)
        assert (ids == -7).all() and (dist == -7.0).all() and (gap == -7.0).all()
        q = torch.from_numpy(Q).cuda()
        d_ids = torch.full((N, k), -7, dtype=torch.int64, device="cuda")
        d_dist = torch.full((N, k), -7.0, device="cuda")
        d_gap = torch.full((N, k), -7.0, device="cuda")
        torch.cuda.synchronize()
        rc = L.cph_search_diverse_device(h, q.data_ptr(), N, kk, lam, C_, filters, nf, None, 0, d_ids.data_ptr(), d_dist.data_ptr(),
                                         d_gap.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == _lib.INVALID_ARGUMENT, (kk, lam, C_, nf)
        torch.cuda.synchronize()
        assert (d_ids == -7).all() and (d_dist == -7.0).all() and (d_gap == -7.0).all()
    short.close()
