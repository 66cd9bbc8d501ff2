"""Grouped search on the GPU (CPIndex.search_grouped / search_grouped_device, cph_group_rows_hook).

The yardstick is tests/group_model.py: the kernel hook is compared with it and with the host twin on synthetic rows; an
end-to-end call is compared with the model applied to the rows search_batch(q, C, ...) returns in internal ids on the same
handle, under every option the underlying search takes."""
import numpy as np
import pytest

from golden_util import DATASETS, fixture_path
from group_model import (CS, I32_MAX, I32_MIN, KGS, ROW_KINDS, group_model_batch, hook_group_rows, host_group_rows, same_bytes,
                         synth_batch)

pytestmark = pytest.mark.gpu

FIXTURES = [("g16", 1), ("g1024", 2), ("g2048", 1)]
STATES = ("plain", "input", "removed", "added")
CAP = 1024


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


# ---- the kernel against the host twin and the model -----------------------------------------------------------------------
@pytest.mark.parametrize("Cn", CS)
def test_kernel_hook_matches_host_twin_and_model(Cn):
    """n = 1, 3 and 130 rows (more than one workgroup; every row kind at least 13 times) at every (k, g) that fits."""
    for (k, g) in KGS:
        if k * g > Cn:
            continue
        for n, first in ((1, 3), (3, 7), (130, 0)):
            ids, dist, key_of, rows, kinds = synth_batch(Cn, k, g, n=n, seed=n, first=first)
            assert ids.shape == (n, Cn) and (n < len(ROW_KINDS) or set(kinds) == set(ROW_KINDS))
            want = group_model_batch(ids, dist, key_of, k, g)
            assert same_bytes(host_group_rows(ids, dist, key_of, k, g), want), (Cn, k, g, n)
            assert same_bytes(hook_group_rows(0, ids, dist, key_of, k, g), want), (Cn, k, g, n)
            twin = host_group_rows(ids, dist, key_of, k, g, rows)
            m = want[0] >= 0                                  # (the row map only renames members: checked on the CPU tier)
            assert np.array_equal(twin[0][m], rows[want[0][m]]) and same_bytes(twin[1:], want[1:])
            assert same_bytes(hook_group_rows(0, ids, dist, key_of, k, g, rows), twin), (Cn, k, g, n, "rows")


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _keys_for(n, seed):
    """Some keys own hundreds of rows (or, on the small fixtures, most of them), some one row; the ends of int32 occur."""
    rng = np.random.default_rng(seed)
    a = rng.random(n)
    keys = np.where(a < 0.5, 0, np.where(a < 0.8, rng.integers(1, 4, n), 1000 + np.arange(n)))
    keys[rng.integers(0, n, 3)] = [I32_MIN, I32_MAX, -1]
    return keys.astype(np.int64)


def _rows_internal(ix, Q, C_, **kw):
    """The candidate rows of the statement: search_batch at k = C in internal ids on the same handle."""
    was = ix.result_ids
    ix.result_ids = "internal"
    try:
        return ix.search_batch(Q, C_, **kw)
    finally:
        ix.result_ids = was


def _expect(ix, Q, k, g, C_, key_of, **kw):
    ids, dist = _rows_internal(ix, Q, C_, **kw)
    rows = ix.row_map() if ix.result_ids == "input" else None
    return group_model_batch(ids, dist, key_of, k, g, rows)


def _same(got, want):
    assert got[4].dtype == bool
    return same_bytes(tuple(got[:4]) + (got[4].astype(np.uint8),), want)


@pytest.fixture(scope="module")
def built(cph, tmp_path_factory):
    """8,230 x 16 at 1 bit, as tests/test_gpu_labels.py builds it, saved once; every test loads its own copy.  The first
    2,000 input rows are one tight cluster (the 'near rows' of the candidates=None test)."""
    rng = np.random.default_rng(77)
    n, dim = 8230, 16
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[:2000] = np.float32(6.0) + np.float32(0.05) * X[:2000]
    ix = cph.CPIndex(dim, 1)
    ix.build(X)
    ix.finalize()
    path = str(tmp_path_factory.mktemp("grouped") / "built.cphn")
    ix.save_native(path)
    Q = rng.standard_normal((12, dim)).astype(np.float32)
    Q[:4] = np.float32(6.0) + np.float32(0.05) * Q[:4]
    return dict(path=path, X=X, Q=Q, dim=dim)


def _open(cph, gold, built, name, bits):
    if name == "built":
        ix = cph.CPIndex(built["dim"], bits)
        ix.load_native(built["path"])
        return ix, built["Q"]
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits))
    ix.set_row_map(np.random.default_rng(5).permutation(ix.size))      # (a v2 file carries none)
    return ix, gold[f"Q/{name}"][:12]


def _brute_force(ix, Q, allowed, key_of, k, g):
    """The exact grouped top-k by numpy over ALL allowed ids: distances from exact_l2 (the bytes every search reports),
    ordered by (distance, internal id)."""
    ids = np.flatnonzero(allowed)
    rows = np.full((len(Q), len(ids) + 1), -1, np.int64)
    dist = np.full((len(Q), len(ids) + 1), np.finfo(np.float32).max, np.float32)
    for i, q in enumerate(Q):
        d = ix.exact_l2(q, ids)
        o = np.lexsort((ids, d))
        rows[i, :len(ids)], dist[i, :len(ids)] = ids[o], d[o]
    return group_model_batch(rows, dist, key_of, k, g, ix.row_map() if ix.result_ids == "input" else None)


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name,bits", FIXTURES + [("built", 1)])
def test_end_to_end_options(cph, gold, built, name, bits, state):
    ix, Q = _open(cph, gold, built, name, bits)
    n0 = ix.size
    rng = np.random.default_rng(n0 + len(state))
    key_of = _keys_for(n0, n0)
    ix.set_labels(key_of, ids="internal")
    counts = np.unique(key_of, return_counts=True)[1]
    assert counts.max() >= min(100, n0 // 3) and (counts == 1).sum() >= 10
    if state == "input":
        ix.result_ids = "input"
    if state in ("removed", "added"):
        gone = rng.choice(n0, n0 // 5, replace=False)
        assert ix.remove(gone, ids="internal") == len(gone)
    if state == "added":
        # a twin of base row 5 under another key, and a few fresh rows
        twin = ix.get_vectors(5, 1)
        extra = np.concatenate([twin, twin + np.float32(0.25), rng.standard_normal((6, ix.dim)).astype(np.float32)])
        extra_keys = np.array([777777, int(key_of[5]), 0, 0, 1, 424242, I32_MIN, -1], np.int64)
        assert extra_keys[0] != key_of[5]
        ix.add(extra, labels=extra_keys)
        key_of = np.concatenate([key_of, extra_keys])
    n = ix.size
    removed = ix.removed_mask(ids="internal")
    mask = rng.random(n) < 0.4
    small = rng.random(n) < 0.08
    f = ix.make_filter(mask, ids="internal")
    f2 = ix.make_filter(small, ids="internal")
    empty = ix.make_filter(np.zeros(n, bool), ids="internal")
    fo = rng.integers(-1, 3, len(Q))
    lab = key_of[rng.integers(0, n, len(Q))]
    variants = [dict(), dict(exact=True), dict(filter=f), dict(filter=f, exact=True), dict(filter=empty), dict(label=0),
                dict(label=lab, exact=True), dict(filter=[f, f2, empty], filter_of=fo, exact=True)]
    if state == "added":
        # inherited: per-query filters (a label per query is that) would walk the graph of an index with a tail
        with pytest.raises(NotImplementedError):
            ix.search_grouped(Q, 3, 2, candidates=17, filter=[f, f2, empty], filter_of=np.zeros(len(Q), np.int64))
        with pytest.raises(NotImplementedError):
            ix.search_grouped(Q, 3, 2, candidates=17, label=lab)
    else:
        variants += [dict(label=lab), dict(filter=[f, f2, empty], filter_of=fo)]
    other = (key_of * 7 + 3) % 11                         # a second column: other groups
    gk_same = ix.make_group_keys(key_of, ids="internal")
    gk_other = ix.make_group_keys(other, ids="internal")
    for (k, g, C_) in ((1, 1, 1), (3, 2, 17), (10, 3, 70), (8, 4, 130)):
        for kw in variants:
            got = ix.search_grouped(Q, k, g, candidates=C_, **kw)
            assert got[0].shape == (len(Q), k, g) and got[2].shape == (len(Q), k) and got[4].shape == (len(Q),)
            assert _same(got, _expect(ix, Q, k, g, C_, key_of, **kw)), (name, state, k, g, C_, sorted(kw))
        # a keys object: the label column's values give the label column's bytes, other values other groups
        got = ix.search_grouped(Q, k, g, candidates=C_, exact=True)
        assert same_bytes(ix.search_grouped(Q, k, g, candidates=C_, keys=gk_same, exact=True), got)
        got_o = ix.search_grouped(Q, k, g, candidates=C_, keys=gk_other, filter=f)
        assert _same(got_o, _expect(ix, Q, k, g, C_, other, filter=f))
        if C_ >= 17:
            assert not np.array_equal(got_o[2], ix.search_grouped(Q, k, g, candidates=C_, filter=f)[2])
    # keys given in input rows land where the label column's do
    if ix.has_row_map:
        by_row = np.empty(n, np.int64)
        by_row[ix.row_map()] = key_of
        gk_rows = ix.make_group_keys(by_row, ids="input")
        assert same_bytes(ix.search_grouped(Q, 3, 2, candidates=17, keys=gk_rows), ix.search_grouped(Q, 3, 2, candidates=17))
        gk_rows.close()
    # exactness: exact=True with C above the number of allowed ids is complete everywhere and equals brute force
    allowed = (small if n > CAP - 1 else np.ones(n, bool)) & ~removed
    assert allowed.sum() < CAP
    kw = dict(filter=f2) if n > CAP - 1 else {}          # (f2: `small` as a filter in internal ids)
    C_ = int(allowed.sum()) + 1
    if C_ >= 10 * 3:
        got = ix.search_grouped(Q, 10, 3, candidates=C_, exact=True, **kw)
        assert got[4].all()
        assert _same(got, _brute_force(ix, Q, allowed, key_of, 10, 3)), (name, state)
    if state == "added":
        # the twin and its base row are equally near and sit in different groups
        got = ix.search_grouped(ix.get_vectors(5, 1), 4, 1, candidates=32, exact=True)
        if not removed[5]:
            assert {int(key_of[5]), 777777} <= set(got[2][0].tolist())
        # a keys object made before an add no longer fits
        old = ix.make_group_keys(key_of, ids="internal")
        ix.add(ix.get_vectors(0, 1), labels=[5])
        with pytest.raises(ValueError, match=f"cover {n} ids, the index holds {n + 1}"):
            ix.search_grouped(Q, 3, 2, candidates=17, keys=old)
        with pytest.raises(ValueError, match=f"covers {n} ids, the index holds {n + 1}"):
            ix.search_batch(Q, 3, filter=f)               # (the size error a filter gets)
        old.close()
    for x in (f, f2, empty, gk_same, gk_other):
        x.close()


def test_keys_object_lifetime_and_refusals(cph, gold):
    ix, Q = _open(cph, gold, None, "g16", 1)
    n = ix.size
    with pytest.raises(ValueError, match="set_labels"):
        ix.search_grouped(Q, 3, 2)                         # no label column, no keys
    gk = ix.make_group_keys(np.arange(n) % 7)
    assert gk.size == n
    got = ix.search_grouped(Q, 3, 2, candidates=20, keys=gk)
    assert _same(got, _expect(ix, Q, 3, 2, 20, np.arange(n) % 7))
    for bad in (dict(k=0), dict(group_size=0), dict(k=33, group_size=32), dict(k=5, group_size=5, candidates=24),
                dict(candidates=1025), dict(keys=np.arange(n))):
        kw = dict(k=3, group_size=2, candidates=20, keys=gk)
        kw.update(bad)
        with pytest.raises(ValueError):
            ix.search_grouped(Q, **kw)
    with pytest.raises(ValueError):
        ix.make_group_keys(np.arange(n + 1))
    with pytest.raises(ValueError):
        ix.make_group_keys(np.arange(n, dtype=np.int64) << 31)
    other, _ = _open(cph, gold, None, "g16", 1)
    with pytest.raises(ValueError, match="another index"):
        other.search_grouped(Q, 3, 2, candidates=20, keys=gk)
    ix.set_labels(np.arange(n) % 7, ids="internal")
    ix.remove(np.arange(0, n, 9), ids="internal")
    ix.compact()
    with pytest.raises(ValueError, match="cover|another index"):      # compact() invalidates it
        ix.search_grouped(Q, 3, 2, candidates=20, keys=gk)
    assert ix.search_grouped(Q, 3, 2, candidates=20)[0].shape == (len(Q), 3, 2)      # (the label column was carried over)
    gk.close()
    with pytest.raises(ValueError, match="closed"):
        ix.search_grouped(Q, 3, 2, candidates=20, keys=gk)


# ---- candidates=None ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", (True, False))
def test_default_candidates_policy(cph, built, exact):
    """The documented loop, repeated here with search_batch and the model: C0 = min(1024, max(64, 4 k g)), the incomplete
    queries again at min(4 C, 1024) until complete or C = 1024, a query's answer that of its last pass."""
    ix = cph.CPIndex(built["dim"], 1)
    ix.load_native(built["path"])
    Q, k, g = built["Q"], 10, 3
    n = ix.size
    rows = ix.row_map()
    # the cluster is one key; sixty keys share the rest: a row of 120 candidates holds about two of each, too few for ten
    # groups of three, a row of 480 about eight
    by_row = np.where(np.arange(n) < 2000, 0, 1 + np.arange(n) % 60)
    key_of = by_row[rows]
    ix.set_labels(key_of, ids="internal")
    # the inputs: the first four queries sit in the cluster, whose 2,000 rows carry one key
    near = _rows_internal(ix, Q[:4], CAP, exact=True)[0]
    assert (key_of[near] == 0).all()
    got = ix.search_grouped(Q, k, g, exact=exact)
    C_ = min(CAP, max(64, 4 * k * g))
    assert C_ == 120
    want = list(_expect(ix, Q, k, g, C_, key_of, exact=exact))
    first_pass = want[4].copy()
    todo = np.flatnonzero(want[4] == 0)
    passes = 1
    while todo.size and C_ < CAP:
        C_ = min(4 * C_, CAP)
        sub = _expect(ix, Q[todo], k, g, C_, key_of, exact=exact)
        for w, s_ in zip(want, sub):
            w[todo] = s_
        todo = todo[sub[4] == 0]
        passes += 1
    assert _same(got, tuple(want))
    assert passes >= 2 and ((first_pass == 0) & (want[4] == 1)).any(), "no query needed a second pass and got complete"
    if exact:       # (the graph route may return fewer than 1,024 ids, which is the other reason to be complete)
        assert C_ == CAP and (want[4][:4] == 0).all(), "the cluster's queries must stay incomplete at C = 1024"
        assert (want[3][:4, 0] == g).all() and (want[3][:4, 1:] == 0).all()     # one full group, nothing else


# ---- the device variant ------------------------------------------------------------------------------------------------------
def test_device_variant(cph, gold):
    import torch
    ix, Q = _open(cph, gold, None, "g16", 1)
    n = ix.size
    key_of = _keys_for(n, 3)
    ix.set_labels(key_of, ids="internal")
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    f = ix.make_filter(np.arange(n) % 3 != 0, ids="internal")
    fo = np.arange(len(Q)) % 2 - 1
    k, g, C_ = 5, 2, 40
    cases = [dict(), dict(exact=True), dict(filter=f), dict(filter=[f], filter_of=fo), dict(label=0)]
    st1, st2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    for st in (st1, st2):
        st.wait_stream(torch.cuda.current_stream(dev))
    for kw in cases:
        want = ix.search_grouped(Q, k, g, candidates=C_, **kw)
        got = ix.search_grouped_device(Qd, k, g, candidates=C_, **kw)
        torch.cuda.synchronize()
        assert got[4].dtype == torch.bool and same_bytes([t.cpu().numpy() for t in got], want), sorted(kw)
        # out= and a side stream; the results are used in stream order, with no host wait in between
        out = (torch.full((len(Q), k, g), -9, dtype=torch.int64, device=dev), torch.full((len(Q), k, g), -9.0, device=dev),
               torch.full((len(Q), k), -9, dtype=torch.int32, device=dev), torch.full((len(Q), k), -9, dtype=torch.int32, device=dev),
               torch.full((len(Q),), 9, dtype=torch.uint8, device=dev))
        st1.wait_stream(torch.cuda.current_stream(dev))
        res = ix.search_grouped_device(Qd, k, g, candidates=C_, out=out, stream=st1, **kw)
        with torch.cuda.stream(st1):
            copies = [t.clone() for t in res]
        st1.synchronize()
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
        assert same_bytes([t.cpu().numpy() for t in copies], want), sorted(kw)
    # default candidates: the single pass at C0
    got = ix.search_grouped_device(Qd, k, g)
    torch.cuda.synchronize()
    assert same_bytes([t.cpu().numpy() for t in got], ix.search_grouped(Q, k, g, candidates=64))
    # two batches on two streams
    want_a = ix.search_grouped(Q, k, g, candidates=C_)
    want_b = ix.search_grouped(Q[::-1].copy(), 3, 4, candidates=90, exact=True)
    Qr = torch.from_numpy(Q[::-1].copy()).to(dev)
    torch.cuda.synchronize()
    for _ in range(3):
        a = ix.search_grouped_device(Qd, k, g, candidates=C_, stream=st1)
        b = ix.search_grouped_device(Qr, 3, 4, candidates=90, exact=True, stream=st2)
        with torch.cuda.stream(st1):
            ca = [t.clone() for t in a]
        with torch.cuda.stream(st2):
            cb = [t.clone() for t in b]
        st1.synchronize()
        st2.synchronize()
        assert same_bytes([t.cpu().numpy() for t in ca], want_a) and same_bytes([t.cpu().numpy() for t in cb], want_b)
    ix.synchronize()
    f.close()


# ---- replicas and parts ------------------------------------------------------------------------------------------------------
def test_replicas_equal_one_device_and_parts_are_refused(cph, gold):
    name, bits = "g16", 1
    one, Q = _open(cph, gold, None, name, bits)
    Q = gold[f"Q/{name}"]
    m = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0])
    m.set_min_shard(1)
    m.load(fixture_path(name, bits))
    m.set_row_map(one.row_map())
    n = one.size
    key_of = _keys_for(n, 9)
    other = (key_of * 5 + 1) % 13
    mask = np.arange(n) % 4 != 1
    fo = np.arange(len(Q)) % 3 - 1
    for ix in (one, m):
        ix.set_labels(key_of, ids="internal")
    for ids in ("internal", "input"):
        one.result_ids = m.result_ids = ids
        gk1, gkm = one.make_group_keys(other, ids="internal"), m.make_group_keys(other, ids="internal")
        f1, fm = one.make_filter(mask, ids="internal"), m.make_filter(mask, ids="internal")
        e1, em = one.make_filter(~mask, ids="internal"), m.make_filter(~mask, ids="internal")
        for kw1, kwm in ((dict(), dict()), (dict(exact=True), dict(exact=True)), (dict(filter=f1), dict(filter=fm)),
                         (dict(keys=gk1, filter=f1, exact=True), dict(keys=gkm, filter=fm, exact=True)),
                         (dict(filter=[f1, e1], filter_of=fo), dict(filter=[fm, em], filter_of=fo)), (dict(label=0), dict(label=0))):
            for cand in (40, None):
                assert same_bytes(m.search_grouped(Q, 6, 3, candidates=cand, **kwm),
                                  one.search_grouped(Q, 6, 3, candidates=cand, **kw1)), (ids, sorted(kw1), cand)
        for x in (gk1, gkm, f1, fm, e1, em):
            x.close()
    p = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0], partition=True)
    with pytest.raises(ValueError, match="partitioned"):
        p.search_grouped(Q, 6, 3)
    with pytest.raises(ValueError, match="partitioned"):
        p.make_group_keys(np.zeros(4, np.int64))


# ---- nothing else moved ------------------------------------------------------------------------------------------------------
def test_ungrouped_search_is_untouched(cph, gold):
    ix, Q = _open(cph, gold, None, "g16", 1)
    ix.set_labels(_keys_for(ix.size, 1), ids="internal")
    for space in ("internal", "input"):
        ix.result_ids = space
        before = ix.search_batch(Q, 10)
        stats_before = ix.last_search_stats()
        ix.search_grouped(Q, 4, 2, candidates=50)
        ix.search_grouped(Q, 4, 2, candidates=50, exact=True)
        assert ix.result_ids == space
        after = ix.search_batch(Q, 10)
        stats_after = ix.last_search_stats()
        assert same_bytes(before, after)
        timed = {k for k in stats_before if k.endswith("_us")}
        assert {k: v for k, v in stats_before.items() if k not in timed} == {k: v for k, v in stats_after.items() if k not in timed}
    ix.result_ids = "internal"
    assert np.array_equal(ix.search_batch(Q, 10)[0], gold["S/g16/b1/plain/k10/ids"][:len(Q)])       # (Q: the first 12 queries)
