"""The inner-product metric on the GPU (CPIndex(..., metric="ip"); cph_set_metric_ip; csrc/device_ip.h).

An inner-product index stores [x, sqrt(M2 - |x|^2)] and searches [q, 0], so the squared-L2 kernels rank by inner product;
an epilogue turns every distance into -(q.x) = 0.5 * (d - (|q|^2 + M2)).  tests/ip_model.py states all of it in numpy, bit
for bit.  The main test is the L2 twin: index A is built with metric="ip" from X, index B is a plain index of dim + 1 built
from model(X); A is asked with Q, B with the model's [Q, 0].  The builder is reproducible, so every call must return B's
ids and the model's epilogue of B's distance BYTES -- no tolerance anywhere except where a test compares against float64
truth, with the bound the arithmetic allows."""
import ctypes as C
import gzip
import os
import threading

import numpy as np
import pytest

from ip_model import (DIMS, NO_ROW, NS, bad_cases, case_rows, cases, epilogue_case, epilogue_model, max_model, model,
                      queries_model, rows_model, sq_norm_model)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N, NQ, K = 1500, 64, 10
CONFIGS = ((24, 4), (31, 1), (32, 2))            # stored 25, 32, 33: D = 32 (padding), 32 (none), 64 (the doubling case)
A5 = np.frombuffer(b"\xa5" * 4, np.float32)[0]
FLT_MAX = np.finfo(np.float32).max


def _beq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _dev(cph):
    return cph.index._default_device()


def _data(dim, seed=0):
    """The recipe of tests/test_gpu_cosine.py: X: N distinct Gaussian rows times per-row scales in [0.25, 4]; Q: NQ such
    queries; Y: 100 more rows."""
    rng = np.random.default_rng(7000 + dim + seed)

    def rows(n):
        return (rng.standard_normal((n, dim)) * rng.uniform(0.25, 4.0, n)[:, None]).astype(np.float32)
    X, Q, Y = rows(N), rows(NQ), rows(100)
    assert len(np.unique(X, axis=0)) == N
    return X, Q, Y


def _built(cph, dim, bits, rows, **kw):
    ix = cph.CPIndex(dim, bits, **kw)
    ix.build(rows)
    ix.finalize()
    return ix


def _truth(Q, X):
    return -(Q.astype(np.float64) @ X.astype(np.float64).T)


def _bound(dim, m2, Q):
    """Per query: the worst case of a (dim + 1)-term fp32 sum of squares of magnitude at most 2 (M2 + |q|^2), halved, plus
    the norm, root and epilogue roundings."""
    return (dim + 8) * 2.0 ** -24 * (float(m2) + (Q.astype(np.float64) ** 2).sum(axis=1))


def dev_augment(cph, x, mode, m2=0.0):
    from cphnsw_mi355x import _lib
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    out = np.full((n, dim + 1), 7.0, np.float32)
    c = np.full(n, 7.0, np.float32)
    used = C.c_float(-1.0)
    cnt = (C.c_uint64 * 3)(77, 77, 77)
    _lib.check(_lib.lib().cph_ip_augment_hook(_dev(cph), x.ctypes.data, n, dim, mode, float(m2), out.ctypes.data, c.ctypes.data,
                                              C.byref(used), cnt))
    return out, c, np.float32(used.value), (int(cnt[0]), int(cnt[1]), int(cnt[2]))


def dev_epilogue(cph, ids, dist, c, pinned):
    from cphnsw_mi355x import _lib
    ids = np.ascontiguousarray(ids, np.int64)
    d = np.ascontiguousarray(dist, np.float32).copy()
    c = np.ascontiguousarray(c, np.float32)
    _lib.check(_lib.lib().cph_ip_epilogue_hook(_dev(cph), ids.ctypes.data, d.ctypes.data, ids.shape[0], ids.shape[1], c.ctypes.data,
                                               int(pinned)))
    return d


# ---- 1. the kernels against the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_kernels_have_the_model_s_bytes(cph, dim):
    a5 = np.float32(A5).view(np.uint32)
    for n in NS:                                   # (130 rows: more than one workgroup)
        x = case_rows(n, dim)
        want, m2, cnt = rows_model(x)
        got, c, used, gcnt = dev_augment(cph, x, 1)
        assert _beq(used, m2) and gcnt == cnt == (0, 0, NO_ROW) and _beq(got, want), (n, dim)
        # the hook's device outputs start as 0xA5 bytes: rows write every slot of out and leave c alone
        assert not (got.view(np.uint32) == a5).any() and (c.view(np.uint32) == a5).all()
        below = np.nextafter(m2, np.float32(0.0))
        want, _, cnt = rows_model(x, below)
        got, _, _, gcnt = dev_augment(cph, x, 0, below)
        assert cnt[1] >= 1 and gcnt == cnt and _beq(got, want), (n, dim)
        q = case_rows(n, dim, seed=3)
        q[n // 2, 0] = np.nan if dim % 2 else q[n // 2, 0]
        want, wc, cnt = queries_model(q, m2)
        got, c, _, gcnt = dev_augment(cph, q, 2, m2)
        assert gcnt == cnt and _beq(got, want) and _beq(c, wc), (n, dim)
        assert not (got.view(np.uint32) == a5).any() and not (c.view(np.uint32) == a5).any()
    assert (130, dim) in cases()


@pytest.mark.parametrize("dim", (8, 64, 65, 130))
def test_kernel_bad_and_over_bound_rows(cph, dim):
    for kind, pos, x, m2 in bad_cases(dim):
        want, wm2, wcnt = rows_model(x, m2)
        got, _, used, cnt = dev_augment(cph, x, 1 if m2 is None else 0, 0.0 if m2 is None else m2)
        assert cnt == wcnt == ((0, 1, pos) if kind == "over" else (1, 0, pos)) and _beq(used, wm2), (kind, pos)
        assert _beq(got, want) and _beq(got[pos], np.zeros(dim + 1, np.float32)), (kind, pos)
    x = case_rows(130, dim)                        # several, in several workgroups: all counted, kinds apart, the lowest kept
    keep = np.setdiff1d(np.arange(130), [5, 64, 129])
    m2 = max_model(x[keep])
    x[64] = x[keep][int(np.argmax(sq_norm_model(x[keep])))] * np.float32(2)
    x[5] = np.nan
    x[129, 0] = np.inf
    got, _, _, cnt = dev_augment(cph, x, 0, m2)
    assert cnt == (2, 1, 5) == rows_model(x, m2)[2] and _beq(got, rows_model(x, m2)[0])


@pytest.mark.parametrize("pinned", (0, 1), ids=("device", "pinned"))
def test_epilogue_kernel_has_the_model_s_bytes(cph, pinned):
    for n, k in [(1, 1), (3, 10), (130, 7), (64, 100), (16, 10)]:
        ids, dist, c = epilogue_case(n, k)
        got = dev_epilogue(cph, ids, dist, c, pinned)
        assert _beq(got, epilogue_model(ids, dist, c)), (n, k)
        pad = ids < 0
        assert _beq(got[pad], dist[pad])                                   # padding keeps its bytes


# ---- 2. the L2 twin ------------------------------------------------------------------------------------------------------
def _labels(n, seed):
    return np.random.default_rng(seed).integers(0, 7, n).astype(np.int32)


def _calls(ix, Q, size, tail=False):
    """Every search an inner-product index serves, by name -> (ids, dist, the query of every row)."""
    import torch
    rng = np.random.default_rng(5)
    m1, m2 = rng.random(size) < 0.5, rng.random(size) < 0.2
    m3 = np.zeros(size, bool)
    m3[rng.choice(size, 4, replace=False)] = True  # fewer allowed ids than k: every row ends in padding
    fo = rng.integers(-1, 2, len(Q)).astype(np.int32)
    every = np.arange(len(Q))
    out = {}
    i, d = ix.search(Q[0], K)
    out["search"] = (i[None, :], d[None, :], every[:1])
    for n in (1, 16, 64):                          # 16: the pinned route
        out[f"batch{n}"] = ix.search_batch(Q[:n], K) + (every[:n],)
    dq = torch.from_numpy(Q).to(f"cuda:{ix.devices[0]}")
    ids, d = ix.search_batch_device(dq, K)
    torch.cuda.synchronize()
    out["device"] = (ids.cpu().numpy(), d.cpu().numpy(), every)
    out["filtered"] = ix.search_batch(Q, K, filter=m1) + (every,)
    out["exact"] = ix.search_batch(Q, K, exact=True) + (every,)
    out["exact_filtered"] = ix.search_batch(Q, K, filter=m2, exact=True) + (every,)
    # (an index with added rows serves per-query filters on the scan only)
    out["filter_of"] = ix.search_batch(Q, K, filter=[m1, m2], filter_of=fo, exact=tail) + (every,)
    out["label"] = ix.search_batch(Q, K, label=3) + (every,)
    out["few"] = ix.search_batch(Q, K, filter=m3) + (every,)
    out["few_exact"] = ix.search_batch(Q, K, filter=m3, exact=True) + (every,)
    ix.result_ids = "input"
    out["input"] = ix.search_batch(Q, K) + (every,)
    ix.result_ids = "internal"
    return out


def _same(a, b, c, what):
    """a: the inner-product index's calls, b: the twin's, c [NQ]: the model's c of every query."""
    assert a.keys() == b.keys()
    padded = 0
    for key in a:
        (ai, ad, aq), (bi, bd, _) = a[key], b[key]
        assert _beq(ai, bi), (what, key)                                        # B's ids, byte for byte
        assert _beq(ad, epilogue_model(bi, bd, c[aq])), (what, key)             # the model's scores of B's distances
        pad = bi < 0
        padded += int(pad.sum())
        assert _beq(ad[pad], bd[pad]) and (ad[pad] == FLT_MAX).all(), (what, key)          # padding untouched
        live = np.where(pad, np.inf, ad.astype(np.float64))
        with np.errstate(invalid="ignore"):
            assert not (np.diff(live, axis=1) < 0).any(), (what, key)            # rows ascend
    return padded


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"dim{c[0]}b{c[1]}")
def twin(cph, request):
    dim, bits = request.param
    X, Q, Y = _data(dim)
    Y = Y * np.float32(0.5)                        # (added rows must stay under the bound of the rows of build())
    m2 = max_model(X)
    assert sq_norm_model(Y).max() <= m2
    mX, mY = model(X), model(Y, m2)
    mQ, c, _ = queries_model(Q, m2)
    A = _built(cph, dim, bits, X, metric="ip")
    B = _built(cph, dim + 1, bits, mX)
    lab = _labels(N, dim)
    A.set_labels(lab, ids="input")
    B.set_labels(lab, ids="input")
    return dict(dim=dim, bits=bits, X=X, Q=Q, Y=Y, mX=mX, mQ=mQ, mY=mY, c=c, m2=m2, A=A, B=B)


def test_l2_twin_every_search_has_the_same_ids_and_the_model_s_scores(twin):
    A, B, Q, mQ, dim = twin["A"], twin["B"], twin["Q"], twin["mQ"], twin["dim"]
    assert A.metric == "ip" and B.metric == "l2" and A.size == B.size == N and A.dim == dim and B.dim == dim + 1
    assert _beq(np.float32(A.ip_bound), twin["m2"])
    assert np.array_equal(A.row_map(), B.row_map())
    assert _beq(A.get_vectors(stored=True), twin["mX"][A.row_map()])      # what the index stores: model(X), in its own order
    assert _beq(A.get_vectors(stored=True), B.get_vectors())
    assert _beq(A.get_vectors(), twin["X"][A.row_map()])                  # ... whose first dim columns are the caller's rows
    padded = _same(_calls(A, Q, N), _calls(B, mQ, N), twin["c"], "built")
    assert padded >= NQ * (K - 4)                                         # (the four-id filter leaves padded rows)


def test_l2_twin_after_remove_add_and_compact(twin):
    A, B, Q, mQ, c = twin["A"], twin["B"], twin["Q"], twin["mQ"], twin["c"]
    gone = np.random.default_rng(3).choice(N, (N * 3) // 10, replace=False)
    assert A.remove(gone, ids="input") == B.remove(gone, ids="input") == len(gone)
    _same(_calls(A, Q, N), _calls(B, mQ, N), c, "removed")
    labY = _labels(100, 99)
    assert np.array_equal(A.add(twin["Y"], labels=labY), B.add(twin["mY"], labels=labY))
    assert A.tail_size == B.tail_size == 100
    assert _beq(A.get_vectors(N, 100, stored=True), twin["mY"]) and _beq(A.get_vectors(stored=True), B.get_vectors())
    _same(_calls(A, Q, N + 100, tail=True), _calls(B, mQ, N + 100, tail=True), c, "added")
    # compact passes the live rows through as they are: it does not augment again, and M2 stays
    ma, mb = A.compact(), B.compact()
    assert np.array_equal(ma, mb) and A.size == B.size == N - len(gone) + 100 and A.tail_size == 0
    assert _beq(np.float32(A.ip_bound), twin["m2"])
    assert np.array_equal(A.row_map(), B.row_map()) and _beq(A.get_vectors(stored=True), B.get_vectors())
    live = np.concatenate([np.delete(twin["mX"], gone, axis=0), twin["mY"]])
    assert _beq(A.get_vectors(stored=True), live[A.row_map()])
    _same(_calls(A, Q, A.size), _calls(B, mQ, B.size), c, "compacted")
    assert A.metric_stats()[0] > 0 and B.metric_stats() == (0, 0)


# ---- 3. truth ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(cph):
    dim, bits = 24, 4
    X, Q, Y = _data(dim)
    A = _built(cph, dim, bits, X, metric="ip")
    A.result_ids = "input"
    return dict(dim=dim, bits=bits, X=X, Q=Q, Y=Y, A=A, m2=max_model(X))


def _check_truth(ids, d, Q, X, dim, m2):
    bound = _bound(dim, m2, Q)
    t = _truth(Q, X)
    err = np.abs(d.astype(np.float64) - np.take_along_axis(t, ids, axis=1))
    print("max |score + q.x| / bound =", (err / bound[:, None]).max())
    assert (ids >= 0).all() and (err <= bound[:, None]).all()
    st = np.sort(t, axis=1)
    clear = st[:, K] - st[:, K - 1] > 2 * bound
    print("queries skipped by the gap rule:", int((~clear).sum()), "of", len(Q))
    assert (~clear).mean() <= 0.05
    top = np.argsort(t, axis=1)[:, :K]
    for i in np.flatnonzero(clear):
        assert set(ids[i]) == set(top[i]), i
    assert (np.diff(d, axis=1) >= 0).all()
    return top


def test_exact_scores_against_float64(small):
    """Every exact=True score within (dim + 8) * 2^-24 * (M2 + |q|^2) of the float64 -(q.x); the id set is the float64
    top-10 wherever the 10th and 11th float64 scores differ by more than twice that bound (the float64 reference skips 0 of
    64 queries on this data; at most 5 % may be)."""
    A, X, Q = small["A"], small["X"], small["Q"]
    ids, d = A.search_batch(Q, K, exact=True)
    _check_truth(ids, d, Q, X, small["dim"], small["m2"])


# ---- 4. the test that fails without the feature -------------------------------------------------------------------------------
def test_inner_product_ranks_differently_from_l2_and_cosine(cph, small):
    A, X, Q, dim, bits = small["A"], small["X"], small["Q"], small["dim"], small["bits"]
    ids, d = A.search_batch(Q, K, exact=True)
    _check_truth(ids, d, Q, X, dim, small["m2"])                          # the float64 inner-product top-10
    for metric in ("l2", "cosine"):
        O = _built(cph, dim, bits, X, metric=metric)
        O.result_ids = "input"
        oi, _ = O.search_batch(Q, K, exact=True)
        differ = np.mean([set(ids[i]) != set(oi[i]) for i in range(NQ)])
        print(f"queries whose ip top-10 differs from the {metric} top-10:", differ)
        assert differ > 0.5, metric


# ---- 5. bound and add ---------------------------------------------------------------------------------------------------------
def test_bound_and_add(cph, small):
    X, Q, dim, bits, m2 = small["X"], small["Q"], small["dim"], small["bits"], small["m2"]
    s = sq_norm_model(X)
    half = 0.5 * float(np.sqrt(m2))
    low = np.float32(half) * np.float32(half)      # (max_norm is squared in float32)
    over = np.flatnonzero(s > low)
    assert 1 < len(over) < N
    ix = cph.CPIndex(dim, bits, metric="ip", max_norm=half)
    assert _beq(np.float32(ix.ip_bound), low)
    with pytest.raises(ValueError, match=rf"row {over[0]} .*\({len(over)} such row"):
        ix.build(X)
    assert ix.size == 0 and not ix.is_finalized
    ix.build(X * np.float32(0.25))                 # the handle is empty and reusable
    ix.finalize()
    assert ix.size == N and ix.is_finalized
    # add() checks against the M2 of the index
    A = small["A"]
    long_row = X[int(np.argmax(s))] * np.float32(1.5)
    before = A.search_batch(Q, K)
    with pytest.raises(ValueError, match=r"row 1 .*rebuil"):
        A.add(np.stack([X[0] * np.float32(0.5), long_row]))
    after = A.search_batch(Q, K)
    assert A.tail_size == 0 and A.size == N and _beq(before[0], after[0]) and _beq(before[1], after[1])
    bad = np.stack([X[0], X[1]])
    bad[0, 3] = np.nan
    with pytest.raises(ValueError, match=r"row 0 "):
        A.add(bad)
    assert A.tail_size == 0
    W = _built(cph, dim, bits, X, metric="ip", max_norm=2.0 * float(np.sqrt(m2)))     # M2 = 4 max |x|^2
    W.result_ids = "input"
    twice = 2.0 * float(np.sqrt(m2))
    assert np.array_equal(W.add(long_row[None, :]), [N])
    assert W.tail_size == 1 and _beq(np.float32(W.ip_bound), np.float32(twice) * np.float32(twice))
    for kw in (dict(), dict(exact=True)):
        ids, d = W.search_batch(long_row[None, :], K, **kw)
        assert ids[0, 0] == N, kw                  # (a query parallel to the longest row finds it first)
        want = -float(long_row.astype(np.float64) @ long_row.astype(np.float64))
        assert abs(d[0, 0] - want) <= _bound(dim, W.ip_bound, long_row[None, :])[0]


# ---- 6. threads -----------------------------------------------------------------------------------------------------------------
def test_eight_threads_search_concurrently(small):
    A, Q = small["A"], small["Q"]
    want = A.search_batch(Q, K)
    got, errs = [None] * 8, []

    def work(t):
        try:
            got[t] = [A.search(Q[i], K) for i in range(t, NQ, 8)]
        except Exception as e:       # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for t in range(8):
        for j, i in enumerate(range(t, NQ, 8)):
            assert _beq(got[t][j][0], want[0][i]) and _beq(got[t][j][1], want[1][i]), i


# ---- 7. replicas ----------------------------------------------------------------------------------------------------------------
def test_replicas_have_the_single_device_bytes(cph, small):
    dim, bits, X, Q = small["dim"], small["bits"], small["X"], small["Q"]
    d = _dev(cph)
    A = _built(cph, dim, bits, X, metric="ip")
    M = _built(cph, dim, bits, X, devices=[d, d], metric="ip")
    assert M.metric == "ip" and M.dim == dim and _beq(M.get_vectors(stored=True), A.get_vectors(stored=True))
    assert _beq(np.float32(M.ip_bound), np.float32(A.ip_bound))
    mask = np.random.default_rng(5).random(N) < 0.5
    for kw in (dict(), dict(exact=True), dict(filter=mask)):
        a, m = A.search_batch(Q, K, **kw), M.search_batch(Q, K, **kw)
        assert _beq(a[0], m[0]) and _beq(a[1], m[1]), kw
    a, m = A.search(Q[3], K), M.search(Q[3], K)
    assert _beq(a[0], m[0]) and _beq(a[1], m[1])


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_what_is_not_served_yet_refuses_before_it_writes(cph, small, tmp_path):
    from cphnsw_mi355x import _lib
    L = _lib.lib()
    A, Q, dim = small["A"], small["Q"], small["dim"]
    A.set_labels(_labels(N, 1), ids="input")
    n, k = 4, 5
    q = np.ascontiguousarray(Q[:n])
    ids = np.full((n, k, 2), -77, np.int64)
    dist = np.full((n, k, 2), 77.0, np.float32)
    i32 = [np.full((n, k * 2), -77, np.int32) for _ in range(4)]
    u8 = np.full((n, k), 77, np.uint8)

    def refused(rc):
        assert rc == _lib.INVALID_ARGUMENT and b"inner-product" in L.cph_last_error()
        assert (ids == -77).all() and (dist == 77.0).all() and (u8 == 77).all() and all((a == -77).all() for a in i32)
    refused(L.cph_search_grouped(A._h, q.ctypes.data, n, k, 2, 64, None, None, 0, None, 0, ids.ctypes.data, dist.ctypes.data,
                                 i32[0].ctypes.data, i32[1].ctypes.data, u8.ctypes.data))
    refused(L.cph_search_diverse(A._h, q.ctypes.data, n, k, C.c_float(0.5), 64, None, 0, None, 0, ids.ctypes.data, dist.ctypes.data,
                                 dist.ctypes.data))
    refused(L.cph_search_maxsim(A._h, q.ctypes.data, n, 1, None, k, 64, None, None, 0, None, 0, i32[0].ctypes.data, dist.ctypes.data,
                                i32[1].ctypes.data, ids.ctypes.data, i32[2].ctypes.data))
    rad = np.ones(n, np.float32)
    r, total = C.c_void_p(), C.c_uint64(77)
    refused(L.cph_range_search_begin(A._h, q.ctypes.data, 0, n, rad.ctypes.data, None, 1, 0, None, C.byref(r), C.byref(total)))
    assert not r.value and total.value == 0
    # ... and through Python, with the C layer's message
    for call in (lambda: A.range_search(Q, 1.0), lambda: A.range_search(Q, 1.0, exact=False, max_results=8),
                 lambda: A.search_grouped(Q, 5, 2), lambda: A.search_diverse(Q, K), lambda: A.search_maxsim(Q[:, None, :], 3),
                 lambda: A.save(str(tmp_path / "a.idx")), lambda: cph.CPIndex(dim, 4, metric="ip").load(str(tmp_path / "none.idx"))):
        with pytest.raises(ValueError, match="inner-product"):
            call()
    assert not (tmp_path / "a.idx").exists()
    with pytest.raises(ValueError, match="partition"):
        cph.CPIndex(dim, 4, devices=[_dev(cph)] * 2, partition=True, metric="ip")
    # the entry that sets L2 and cosine keeps refusing every other value; a partitioned handle names the metric
    fresh = cph.CPIndex(dim, 4)
    assert L.cph_set_metric(fresh._h, 2) == _lib.INVALID_ARGUMENT and b"cph_set_metric_ip" in L.cph_last_error()
    P = cph.CPIndex(dim, 4, devices=[_dev(cph)] * 2, partition=True)
    assert L.cph_parts_set_metric(P._p, 2) == _lib.INVALID_ARGUMENT and b"inner-product" in L.cph_last_error()
    # the metric and the bound are fixed once the handle holds rows; widths past 2048 are refused
    assert L.cph_set_metric_ip(A._h) == _lib.INVALID_ARGUMENT and b"empty handle" in L.cph_last_error()
    assert L.cph_set_ip_bound(A._h, 1.0) == _lib.INVALID_ARGUMENT and b"empty handle" in L.cph_last_error()
    assert L.cph_set_ip_bound(fresh._h, 1.0) == _lib.INVALID_ARGUMENT and b"l2" in L.cph_last_error()
    with pytest.raises(ValueError, match="2048"):
        cph.CPIndex(2048, 4, metric="ip")
    assert cph.CPIndex(2047, 4, metric="ip").dim == 2047
    after = A.search_batch(Q, K)
    assert (after[0] >= 0).all()


# ---- 9. files -------------------------------------------------------------------------------------------------------------------
def test_native_files_carry_the_metric_and_the_bound(cph, small, tmp_path):
    A, Q, dim, bits = small["A"], small["Q"], small["dim"], small["bits"]
    pa = str(tmp_path / "a.cphn")
    A.save_native(pa)
    E = cph.CPIndex(dim, bits, metric="ip")
    E.load_native(pa)
    E.result_ids = "input"
    assert E.metric == "ip" and E.size == N and _beq(np.float32(E.ip_bound), np.float32(A.ip_bound))
    for kw in (dict(), dict(exact=True)):
        a, e = A.search_batch(Q, K, **kw), E.search_batch(Q, K, **kw)
        assert _beq(a[0], e[0]) and _beq(a[1], e[1]), kw
    E.save_native(str(tmp_path / "again.cphn"))
    assert (tmp_path / "again.cphn").read_bytes() == (tmp_path / "a.cphn").read_bytes()
    # an L2 or a cosine handle of the stored width refuses the file by its metric, one of the caller's width by its width
    for metric in ("l2", "cosine"):
        with pytest.raises(ValueError, match=f"ip rows.*{metric}"):
            cph.CPIndex(dim + 1, bits, metric=metric).load_native(pa)
        with pytest.raises((ValueError, RuntimeError)):
            cph.CPIndex(dim, bits, metric=metric).load_native(pa)
    B = _built(cph, dim + 1, bits, model(small["X"]))
    pb = str(tmp_path / "b.cphn")
    B.save_native(pb)
    with pytest.raises(ValueError, match="l2 rows.*ip"):
        E.load_native(pb)
    a, e = A.search_batch(Q, K), E.search_batch(Q, K)                   # the refused load left E as it was
    assert _beq(a[0], e[0]) and _beq(a[1], e[1])


def _golden_cosine_rows():
    rng = np.random.default_rng(20261020)
    return (rng.standard_normal((200, 16)) * rng.uniform(0.25, 4.0, 200)[:, None]).astype(np.float32)


def test_l2_and_cosine_native_files_have_the_bytes_of_the_older_library(cph, tmp_path):
    """tests/golden/ip_parent_cosine_native_f4.cphn.gz was written by the library of the commit before the inner product
    existed (200 rows of _golden_cosine_rows, dim 16, 1 bit, metric="cosine"; the builder is reproducible): a cosine index
    must still be written as exactly those bytes.  The L2 golden is the one tests/test_gpu_cosine.py reads."""
    from golden_util import DATASETS, fixture_path
    ix = _built(cph, 16, 1, _golden_cosine_rows(), metric="cosine")
    ix.save_native(str(tmp_path / "cos.cphn"))
    with gzip.open(os.path.join(HERE, "golden", "ip_parent_cosine_native_f4.cphn.gz"), "rb") as f:
        assert (tmp_path / "cos.cphn").read_bytes() == f.read()
    l2 = cph.CPIndex(DATASETS["g16"]["dim"], 1)
    l2.load(fixture_path("g16", 1))
    n = l2.size
    l2.set_row_map((7 * np.arange(n) + 3) % n)
    l2.save_native(str(tmp_path / "l2.cphn"))
    with gzip.open(os.path.join(HERE, "golden", "remove_g16_b1_parent_native_f2.cphn.gz"), "rb") as f:
        assert (tmp_path / "l2.cphn").read_bytes() == f.read()


# ---- 10. the other metrics untouched --------------------------------------------------------------------------------------------
def test_the_other_metrics_launch_what_they_launched(cph, small):
    import torch
    X, Q, Y = small["X"], small["Q"], small["Y"] * np.float32(0.5)
    counts = {}
    for metric in ("l2", "cosine", "ip"):
        ix = _built(cph, 24, 4, X, metric=metric)
        built = ix.metric_stats()
        ix.search(Q[0], K)
        ix.search_batch(Q[:16], K)
        ix.search_batch(Q, K)
        ix.search_batch(Q, K, exact=True)
        ix.search_batch(Q, K, filter=[np.arange(N) % 2 == 0, np.arange(N) % 3 == 0], filter_of=np.arange(NQ) % 2)
        dq = torch.from_numpy(Q).to(f"cuda:{ix.devices[0]}")
        ix.search_batch_device(dq, K)
        torch.cuda.synchronize()
        ix.add(Y)
        ix.search_batch(Q, K)
        searched = ix.metric_stats()
        ix.compact()
        counts[metric] = (built, searched, ix.metric_stats())
    assert counts["l2"] == ((0, 0), (0, 0), (0, 0))
    # cosine: one launch for the build, one per batch (7 above), one for add(), none for compact() -- as before
    built, searched, compacted = counts["cosine"]
    assert built == (1, 0) and searched[0] == 1 + 7 + 1 and searched[1] > 0 and compacted[0] == searched[0]
    # ip: the max pass and the row pass for the build, two per batch, one for add(), none for compact()
    built, searched, compacted = counts["ip"]
    assert built == (2, 0) and searched[0] == 2 + 2 * 7 + 1 and searched[1] > 0 and compacted[0] == searched[0]


# ---- 11. a non-finite query -----------------------------------------------------------------------------------------------------
def test_a_non_finite_query_searches_as_the_zero_vector(small):
    A, Q, dim, m2 = small["A"], small["Q"], small["dim"], small["m2"]
    q = Q[:4].copy()
    q[0, 5] = np.nan
    q[1, 0] = np.inf
    q[2] = 3e38                                     # (a squared norm that overflows)
    bound = _bound(dim, m2, np.zeros((1, dim), np.float32))[0]
    for kw in (dict(), dict(exact=True)):
        ids, d = A.search_batch(q, K, **kw)
        assert (ids >= 0).all() and np.isfinite(d).all()
        assert np.abs(d[:3]).max() <= bound, kw                          # -(0 . x) = 0
        good = A.search_batch(Q[3:4], K, **kw)
        assert _beq(ids[3], good[0][0]) and _beq(d[3], good[1][0])
    ids, d = A.search(q[0], K)
    assert len(ids) == K and np.abs(d).max() <= bound
