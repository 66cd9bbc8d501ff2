"""One index split across devices (CPIndex(devices=[...], partition=True), cph_parts_*): P single-device indexes over
contiguous slices of the input rows, every query searched by all of them, the rows merged on the first device by
merge_parts_kernel.  On a one-GPU box the parts share device 0 (ordinals may repeat), which exercises everything but
the copy between two GPUs.

The reference of every search test is the same: search each index.part(i) on its own (slice-local input rows), add the
part's first row, stable-argsort the concatenation on the CPU.  Ids must match exactly, distances as bytes."""
import os
import shutil

import numpy as np
import pytest

from golden_util import fixture_path

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(3.4028234663852886e38)


def _beq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _merge(rows_ids, rows_d, los, k):
    """Stable merge of the parts' rows: [n, k] ids (first rows added) and distances."""
    ids = np.concatenate([np.where(i >= 0, i + lo, i) for i, lo in zip(rows_ids, los)], axis=1)
    d = np.concatenate(rows_d, axis=1)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(ids, order, 1), np.take_along_axis(d, order, 1)


def _by_parts(ix, call, k):
    """call(part, i, lo, hi) -> (ids, dist) of part i; the merged rows."""
    got = [call(ix.part(i), i, lo, hi) for i, (lo, hi) in enumerate(ix.parts)]
    return _merge([g[0] for g in got], [g[1] for g in got], [lo for lo, _ in ix.parts], k)


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


class Built:
    def __init__(self, cph, n, dim, bits, devices, seed):
        rng = np.random.default_rng(seed)
        self.X = rng.standard_normal((n, dim)).astype(np.float32)
        self.Q = rng.standard_normal((200, dim)).astype(np.float32)
        self.ix = cph.CPIndex(dim, bits, devices=devices, partition=True)
        self.ix.build(self.X)
        self.ix.finalize()


@pytest.fixture(scope="module")
def ragged3(cph):
    """6,001 x 128, 4-bit, three parts of 2001 / 2000 / 2000 rows."""
    return Built(cph, 6001, 128, 4, [0, 0, 0], 11)


@pytest.fixture(scope="module")
def two40(cph):
    """4,000 x 40, 1-bit, two parts."""
    return Built(cph, 4000, 40, 1, [0, 0], 12)


# ---- 1. the merge kernel alone ------------------------------------------------------------------------------------
def _merge_case(P, k, seed):
    """n = 5 rows of P part rows: distances from 4 distinct values (ties across and inside parts), rows partly padding,
    row 3: part 0 entirely smaller than part 1, row 4: all padding."""
    rng = np.random.default_rng(seed)
    n = 5
    values = np.array([0.25, 1.0, 1.5, 7.0], np.float32)
    ids = np.full((P, n, k), -1, np.int64)
    d = np.full((P, n, k), FLT_MAX, np.float32)
    for p in range(P):
        for r in range(n):
            m = k if r == 0 else int(rng.integers(0, k + 1))       # row 0: every part full
            pool = values
            if r == 3:
                m = max(m, 1)
                pool = values[:1] if p == 0 else values[2:] if p == 1 else values
            if r == 4:
                m = 0
            d[p, r, :m] = np.sort(rng.choice(pool, m))
            ids[p, r, :m] = rng.integers(0, 1 << 20, m)
    lo = np.arange(P, dtype=np.int64) * 1000003
    return ids, d, lo


@pytest.mark.parametrize("k", [1, 10, 64, 65, 1000])
@pytest.mark.parametrize("P", [1, 2, 3, 16])
def test_merge_kernel_equals_stable_argsort(cph, P, k):
    from cphnsw_mi355x import _lib
    ids, d, lo = _merge_case(P, k, 100 * P + k)
    n = ids.shape[1]
    if P >= 2:
        assert d[0, 3][d[0, 3] < FLT_MAX].max() < d[1, 3].min()
    out_ids = np.full((n, k), -7, np.int64)                        # sentinels: every slot has to be written
    out_d = np.full((n, k), -1.0, np.float32)
    _lib.check(_lib.lib().cph_merge_rows_hook(0, ids.ctypes.data, d.ctypes.data, P, n, k, lo.ctypes.data,
                                              out_ids.ctypes.data, out_d.ctypes.data))
    want_ids, want_d = _merge(list(ids), list(d), list(lo), k)
    assert not (out_ids == -7).any() and not (out_d == -1.0).any()
    assert np.array_equal(out_ids, want_ids), (P, k)
    assert _beq(out_d, want_d), (P, k)
    assert (out_ids[4] == -1).all() and (out_d[4] == FLT_MAX).all()
    assert ((out_ids >= 0) == (out_d < FLT_MAX)).all()             # padding stays padding, and last


def test_merge_hook_refuses_bad_shapes(cph):
    from cphnsw_mi355x import _lib
    a = np.zeros(17 * 4, np.int64)
    f = np.zeros(17 * 4, np.float32)
    for P, n, k in ((0, 1, 1), (17, 1, 1), (1, 0, 1), (1, 1, 0)):
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().cph_merge_rows_hook(0, a.ctypes.data, f.ctypes.data, P, n, k, a.ctypes.data,
                                                      a.ctypes.data, f.ctypes.data))


# ---- 2. built indexes, ragged parts ---------------------------------------------------------------------------------
def _check_search(b, nq, k):
    import torch
    ix, Q = b.ix, b.Q[:nq]
    ids, d = ix.search_batch(Q, k)
    exp = ix.last_query_expansions(nq)
    # (read before the parts are searched on their own: each part's last batch is still its share of that call)
    part_exp = [ix.part(i).last_query_expansions(nq) for i in range(len(ix.parts))]

    def one(part, i, lo, hi):
        assert part.result_ids == "input" and part.size == hi - lo
        return part.search_batch(Q, k)

    want_ids, want_d = _by_parts(ix, one, k)
    assert ids.shape == (nq, k) and ids.dtype == np.int64 and d.dtype == np.float32
    assert np.array_equal(ids, want_ids), (nq, k)
    assert _beq(d, want_d), (nq, k)
    assert ((ids >= 0) == (d < FLT_MAX)).all()
    assert ids.max() < ix.size
    assert np.array_equal(exp, np.sum(part_exp, axis=0, dtype=np.uint64).astype(np.uint32))
    # search(): row 0, unpadded
    si, sd = ix.search(Q[0], k)
    m = int((ids[0] >= 0).sum())
    assert np.array_equal(si, ids[0, :m]) and _beq(sd, d[0, :m])
    # the device form: the same bytes
    qt = torch.from_numpy(Q).cuda(0)
    ti, td = ix.search_batch_device(qt, k)
    torch.cuda.synchronize()
    assert np.array_equal(ti.cpu().numpy(), ids) and _beq(td.cpu().numpy(), d), (nq, k)
    return ids, d


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("nq", [1, 7, 33, 200])
def test_ragged_three_parts_equal_merged_parts(ragged3, nq, k):
    assert ragged3.ix.parts == [(0, 2001), (2001, 4001), (4001, 6001)]
    assert ragged3.ix.size == 6001 and ragged3.ix.is_finalized and ragged3.ix.result_ids == "input"
    ids, _ = _check_search(ragged3, nq, k)
    assert (ids >= 0).all()


@pytest.mark.parametrize("k", [1, 10, 100, 3000])
@pytest.mark.parametrize("nq", [1, 7, 33, 200])
def test_two_parts_one_bit_equal_merged_parts(two40, nq, k):
    assert two40.ix.parts == [(0, 2000), (2000, 4000)]
    ids, d = _check_search(two40, nq, k)
    if k == 3000:       # more than a part holds: each part pads, the padding merges behind everything found
        found = (ids >= 0).sum(axis=1)
        assert (found >= 1).all() and (found <= 3000).all()
        for r in range(nq):
            assert (ids[r, found[r]:] == -1).all() and (d[r, found[r]:] == FLT_MAX).all()


def test_stats_are_summed_over_parts(ragged3):
    ix, Q = ragged3.ix, ragged3.Q[:64]
    ix.search_batch(Q, 10)
    st = ix.last_search_stats()
    per = [ix.part(i).last_search_stats() for i in range(3)]      # each part's last batch: its share of that call
    for key in ("expansions", "exact_l2", "new_neighbours", "beam_pushes", "stage2_skipped", "rerun_queries"):
        assert st[key] == sum(p[key] for p in per), key
    assert st["kernel_us"] == max(p["kernel_us"] for p in per)
    assert st["expansions"] > 0 and "merge_us" in st
    with pytest.raises(ValueError):
        ix.last_query_expansions(63)


# ---- 3. exact --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 10, 100])
def test_exact_is_the_global_top_k(ragged3, k):
    ix, Q, X = ragged3.ix, ragged3.Q[:33], ragged3.X
    ids, d = ix.search_batch(Q, k, exact=True)
    want_ids, want_d = _by_parts(ix, lambda part, i, lo, hi: part.search_batch(Q, k, exact=True), k)
    assert np.array_equal(ids, want_ids) and _beq(d, want_d)
    assert (ids >= 0).all() and (np.diff(d, axis=1) >= 0).all()
    for r in range(len(Q)):
        assert len(set(ids[r].tolist())) == k
    # float64 brute force over the whole input array: the largest returned true distance is the k-th true distance, up
    # to the fp32 rounding of a 128-term sum (128 * 2^-24 ~ 8e-6 relative)
    true = ((Q.astype(np.float64)[:, None, :] - X.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    kth = np.sort(true, axis=1)[:, k - 1]
    worst = np.take_along_axis(true, ids, 1).max(axis=1)
    assert (worst <= kth * (1 + 1e-5)).all(), float((worst / kth).max())


# ---- 4. filters ------------------------------------------------------------------------------------------------------
def _mask(b, per_part):
    """Global mask with per_part[i] allowed rows in part i."""
    rng = np.random.default_rng(5)
    mask = np.zeros(b.ix.size, bool)
    for (lo, hi), cnt in zip(b.ix.parts, per_part):
        mask[lo + rng.choice(hi - lo, cnt, replace=False)] = True
    return mask


def _filtered_by_parts(ix, Q, k, mask, **kw):
    return _by_parts(ix, lambda part, i, lo, hi: part.search_batch(Q, k, filter=part.make_filter(mask[lo:hi]), **kw), k)


def test_filter_cut_at_part_bounds(ragged3):
    ix, Q = ragged3.ix, ragged3.Q[:33]
    mask = _mask(ragged3, [0, 20, 20])                          # the whole first part disallowed, 1 % of the rest
    f = ix.make_filter(mask)
    assert f.count == 40 and f.size == 6001
    for k in (1, 10, 100):
        ids, d = ix.search_batch(Q, k, filter=f)
        assert mask[ids[ids >= 0]].all()
        assert (ids[ids >= 0] >= 2001).all()
        want_ids, want_d = _filtered_by_parts(ix, Q, k, mask)
        assert np.array_equal(ids, want_ids) and _beq(d, want_d), k
    # ids instead of a mask, and a filter made on the fly
    ids2, d2 = ix.search_batch(Q, 10, filter=np.flatnonzero(mask))
    ids1, d1 = ix.search_batch(Q, 10, filter=f)
    assert np.array_equal(ids1, ids2) and _beq(d1, d2)
    si, sd = ix.search(Q[0], 10, filter=f)
    m = int((ids1[0] >= 0).sum())
    assert np.array_equal(si, ids1[0, :m]) and _beq(sd, d1[0, :m])
    # exact under the filter: all 40 allowed rows, in order
    ei, ed = ix.search_batch(Q, 100, filter=f, exact=True)
    wi, wd = _filtered_by_parts(ix, Q, 100, mask, exact=True)
    assert np.array_equal(ei, wi) and _beq(ed, wd)
    assert ((ei >= 0).sum(axis=1) == 40).all()
    assert all(set(r[:40].tolist()) == set(np.flatnonzero(mask).tolist()) for r in ei)


def test_all_ones_filter_equals_unfiltered(ragged3):
    ix, Q = ragged3.ix, ragged3.Q[:33]
    ones = ix.make_filter(np.ones(ix.size, bool))
    for k in (1, 10, 100):
        a = ix.search_batch(Q, k, filter=ones)
        b = ix.search_batch(Q, k)
        assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1]), k


def test_exact_threshold_is_compared_per_part(ragged3):
    ix, Q = ragged3.ix, ragged3.Q[:33]
    mask = _mask(ragged3, [0, 10, 40])
    try:
        ix.exact_threshold = 25                                 # part 1 (10 allowed) is scanned, part 2 (40) walks its graph
        assert ix.exact_threshold == 25
        ids, d = ix.search_batch(Q, 10, filter=mask)
        want_ids, want_d = _filtered_by_parts(ix, Q, 10, mask)
        assert np.array_equal(ids, want_ids) and _beq(d, want_d)
        assert mask[ids[ids >= 0]].all()
        # part 1 alone, scanned exactly: its 10 allowed rows all come back
        p1 = ix.part(1)
        i1, _ = p1.search_batch(Q, 10, filter=p1.make_filter(mask[2001:4001]))
        e1, _ = p1.search_batch(Q, 10, filter=p1.make_filter(mask[2001:4001]), exact=True)
        assert np.array_equal(i1, e1)
    finally:
        ix.exact_threshold = 0


def test_per_query_filters(ragged3):
    import torch
    ix, Q = ragged3.ix, ragged3.Q[:40]
    fa = ix.make_filter(_mask(ragged3, [0, 20, 20]))
    fb = ix.make_filter(_mask(ragged3, [300, 5, 0]))
    fo = np.array([0, 1, -1, 1, 0, -1, 0, 0, 1, -1] * 4, np.int32)
    for exact in (False, True):
        ids, d = ix.search_batch(Q, 10, filter=[fa, fb], filter_of=fo, exact=exact)
        for v, f in ((0, fa), (1, fb), (-1, None)):
            rows = np.flatnonzero(fo == v)
            wi, wd = ix.search_batch(Q[rows], 10, filter=f, exact=exact)
            assert np.array_equal(ids[rows], wi) and _beq(d[rows], wd), (v, exact)
        ti, td = ix.search_batch_device(torch.from_numpy(Q).cuda(0), 10, filter=[fa, fb], filter_of=fo, exact=exact)
        torch.cuda.synchronize()
        assert np.array_equal(ti.cpu().numpy(), ids) and _beq(td.cpu().numpy(), d)
    with pytest.raises(ValueError):
        ix.search_batch(Q, 10, filter=[fa, fb], filter_of=np.full(40, 2))


# ---- 5. files and refusals -------------------------------------------------------------------------------------------
def test_native_round_trip_and_load_refusals(cph, ragged3, tmp_path):
    ix, Q = ragged3.ix, ragged3.Q[:33]
    path = str(tmp_path / "parts.cphn")
    ix.save_native(path)
    assert sorted(os.listdir(tmp_path)) == [f"parts.cphn.p{i}of3" for i in range(3)]
    want = ix.search_batch(Q, 10)
    fresh = cph.CPIndex(128, 4, devices=[0, 0, 0], partition=True)
    assert not fresh.is_finalized and fresh.size == 0
    fresh.load_native(path)
    assert fresh.is_finalized and fresh.size == 6001 and fresh.parts == ix.parts and fresh.result_ids == "input"
    got = fresh.search_batch(Q, 10)
    assert np.array_equal(got[0], want[0]) and _beq(got[1], want[1])
    # every part file is an ordinary native file of one part
    single = cph.CPIndex(128, 4, device=0)
    single.load_native(path + ".p1of3")
    single.result_ids = "input"
    a, b = single.search_batch(Q, 10), ix.part(1).search_batch(Q, 10)
    assert np.array_equal(a[0], b[0]) and _beq(a[1], b[1])
    # another number of devices, another dim, another bits: ValueError
    with pytest.raises(ValueError):
        cph.CPIndex(128, 4, devices=[0, 0], partition=True).load_native(path)
    for dim, bits in ((64, 4), (128, 2)):
        other = cph.CPIndex(dim, bits, devices=[0, 0, 0], partition=True)
        for i in range(3):
            shutil.copyfile(path + f".p{i}of3", str(tmp_path / f"x{dim}_{bits}.p{i}of3"))
        with pytest.raises(ValueError):
            other.load_native(str(tmp_path / f"x{dim}_{bits}"))
    # a part file missing: ValueError, and the handle keeps the index it had
    os.remove(path + ".p2of3")
    with pytest.raises(ValueError, match="p2of3"):
        fresh.load_native(path)
    assert fresh.is_finalized and fresh.parts == ix.parts
    got = fresh.search_batch(Q, 10)
    assert np.array_equal(got[0], want[0]) and _beq(got[1], want[1])
    # a part without a row map (a format-1 file): ValueError
    single.set_row_map(None)
    single.save_native(str(tmp_path / "nomap.p0of1"))
    with pytest.raises(ValueError, match="row map"):
        cph.CPIndex(128, 4, devices=[0], partition=True).load_native(str(tmp_path / "nomap"))
    # the reference's v2 format holds one graph and no row map
    with pytest.raises(RuntimeError):
        ix.save(str(tmp_path / "v2.idx"))
    with pytest.raises(RuntimeError):
        fresh.load(fixture_path("g128", 4))
    assert fresh.is_finalized


def test_refusals(cph, ragged3):
    ix = ragged3.ix
    with pytest.raises(ValueError):
        ix.result_ids = "internal"
    assert ix.result_ids == "input"
    with pytest.raises(ValueError):
        ix.make_filter(np.ones(ix.size, bool), ids="internal")
    with pytest.raises(ValueError):
        ix.make_filter(np.ones(ix.size - 1, bool))
    with pytest.raises(ValueError):
        ix.make_filter([ix.size])
    with pytest.raises(ValueError):
        cph.CPIndex(128, 4, device=0, partition=True)
    with pytest.raises(ValueError):
        cph.CPIndex(128, 4, partition=True)
    with pytest.raises(ValueError):
        cph.CPIndex(128, 4, devices=[0] * 17, partition=True)
    small = cph.CPIndex(128, 4, devices=[0, 0], partition=True)
    with pytest.raises(ValueError, match="64"):
        small.build(ragged3.X[:127])
    small.build(ragged3.X[:128])
    assert small.size == 128 and small.parts == [(0, 64), (64, 128)] and not small.is_finalized
    q = ragged3.Q[0]
    for call in (lambda: ix.row_map(), lambda: ix.get_vectors(0, 1), lambda: ix.exact_l2(q, [0]),
                 lambda: ix.fastscan_block(np.zeros((32, 16), np.uint8), np.zeros(7, np.float32), 0, 0.0),
                 lambda: ix.entry_point(q), lambda: ix.encode_query(q)):
        with pytest.raises(ValueError, match=r"part\(i\)"):
            call()
    # the parts answer those themselves, in their own spaces
    p1 = ix.part(1)
    rm = p1.row_map()
    assert sorted(rm.tolist()) == list(range(2000))
    assert _beq(p1.get_vectors(0, 3), ragged3.X[2001 + rm[:3]])
    with pytest.raises(ValueError):
        p1.build(ragged3.X[:100])
    with pytest.raises(ValueError):
        ix.part(3)
    # a filter of another index shape is refused
    with pytest.raises(ValueError):
        ix.search_batch(ragged3.Q[:2], 10, filter=p1.make_filter(np.ones(2000, bool)))


def test_plain_devices_list_is_still_a_replica_set(cph, gold):
    ix = cph.CPIndex(128, 4, devices=[0, 0])
    ix.load(fixture_path("g128", 4))
    assert not ix.partitioned and ix.result_ids == "internal"
    ids, _ = ix.search_batch(gold["Q/g128"], 10)
    assert np.array_equal(ids, gold["S/g128/b4/plain/k10/ids"])


def test_two_gpus_equal_merged_parts(cph):
    """Parts on two real devices: the rows of part 1 cross to device 0 by peer copy (or through pinned memory)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    b = Built(cph, 4001, 128, 4, [0, 1], 13)
    for nq, k in ((7, 10), (200, 100)):
        _check_search(b, nq, k)
