"""The cosine metric on the GPU (CPIndex(..., metric="cosine"); cph_set_metric; csrc/device_normalize.h).

A cosine index stores x / sqrt(2 |x|^2) and normalises its queries the same way, so the squared-L2 kernels report
1 - cos.  tests/cosine_model.py states the normalisation in numpy, bit for bit.  The main test is the L2 twin: index A is
built with metric="cosine" from X, index B is a plain index built from model(X); A is asked with Q, B with model(Q).  The
builder is reproducible, so every call must return the same ids and the same distance BYTES on both -- no tolerance
anywhere except where a test compares against float64 truth, with the bound the arithmetic allows."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from cosine_model import DIMS, NO_BAD_ROW, NS, bad_cases, case_rows, cases, model, normalize_model
from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
N, NQ, K = 1500, 64, 10
CONFIGS = ((24, 4), (128, 1), (130, 2))          # D = 32, 256, 256
A5 = np.frombuffer(b"\xa5" * 4, np.float32)[0]


def _beq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _dev(cph):
    return cph.index._default_device()


def _data(dim, seed=0):
    """X: N distinct Gaussian rows times per-row scales in [0.25, 4]; Q: NQ such queries; Y: 100 more rows."""
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


def _cos_dist64(Q, X):
    q = Q.astype(np.float64)
    x = X.astype(np.float64)
    q /= np.linalg.norm(q, axis=1)[:, None]
    x /= np.linalg.norm(x, axis=1)[:, None]
    return 1.0 - q @ x.T


def hook(cph, x, in_place=False):
    from cphnsw_mi355x import _lib
    x = np.ascontiguousarray(x, np.float32)
    out = x.copy() if in_place else np.full(x.shape, 7.0, np.float32)
    src = out if in_place else x
    bad, first = C.c_uint64(77), C.c_uint64(77)
    _lib.check(_lib.lib().cph_normalize_rows_hook(_dev(cph), src.ctypes.data, x.shape[0], x.shape[1], out.ctypes.data, C.byref(bad),
                                                  C.byref(first)))
    return out, int(bad.value), int(first.value)


# ---- 1. the kernel against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_kernel_has_the_model_s_bytes(cph, dim):
    for n in NS:                                   # (130 rows: more than one workgroup)
        x = case_rows(n, dim)
        want, wbad, wfirst = normalize_model(x)
        got, bad, first = hook(cph, x)
        # the hook's device output starts as 0xA5 bytes: a slot the kernel left alone would come back as that
        assert not (got.view(np.uint32) == np.float32(A5).view(np.uint32)).any()
        assert _beq(got, want) and (bad, first) == (wbad, wfirst) == (0, NO_BAD_ROW), (n, dim)
        got, bad, first = hook(cph, x, in_place=True)
        assert _beq(got, want) and (bad, first) == (0, NO_BAD_ROW), (n, dim)
    assert (130, dim) in cases()


@pytest.mark.parametrize("dim", (1, 3, 64, 65, 130))
def test_kernel_bad_rows(cph, dim):
    for kind, pos, x in bad_cases(dim):
        want, wbad, wfirst = normalize_model(x)
        for in_place in (False, True):
            got, bad, first = hook(cph, x, in_place=in_place)
            assert (bad, first) == (wbad, wfirst) == (1, pos), (kind, pos)
            assert _beq(got, want) and got[pos].tobytes() == np.zeros(dim, np.float32).tobytes(), (kind, pos)
    x = case_rows(130, dim)
    x[[5, 64, 129]] = 0.0                          # several bad rows, in several workgroups: all counted, the lowest kept
    got, bad, first = hook(cph, x)
    assert (bad, first) == (3, 5) and _beq(got, normalize_model(x)[0])


# ---- 2. the L2 twin ------------------------------------------------------------------------------------------------------
def _labels(n, seed):
    return np.random.default_rng(seed).integers(0, 7, n).astype(np.int32)


def _calls(ix, Q, radius, size, tail=False):
    """Every search of the index, by name -> arrays.  `size`: the ids a filter may name."""
    import torch
    rng = np.random.default_rng(5)
    m1, m2 = rng.random(size) < 0.5, rng.random(size) < 0.2
    fo = rng.integers(-1, 2, len(Q)).astype(np.int32)
    out = {}
    out["search"] = ix.search(Q[0], K)
    for n in (1, 16, 64):                          # 16: the pinned route
        out[f"batch{n}"] = ix.search_batch(Q[:n], K)
    dq = torch.from_numpy(Q).to(f"cuda:{ix.devices[0]}")
    ids, d = ix.search_batch_device(dq, K)
    torch.cuda.synchronize()
    out["device"] = (ids.cpu().numpy(), d.cpu().numpy())
    out["filtered"] = ix.search_batch(Q, K, filter=m1)
    out["exact"] = ix.search_batch(Q, K, exact=True)
    out["exact_filtered"] = ix.search_batch(Q, K, filter=m2, exact=True)
    # (an index with added rows serves per-query filters on the scan only)
    out["filter_of"] = ix.search_batch(Q, K, filter=[m1, m2], filter_of=fo, exact=tail)
    out["label"] = ix.search_batch(Q, K, label=3)
    out["range_exact"] = ix.range_search(Q, radius)
    out["range_graph"] = ix.range_search(Q, radius, exact=False, max_results=32)
    out["grouped"] = ix.search_grouped(Q, 5, 2, candidates=64)
    out["diverse"] = ix.search_diverse(Q, K, lam=0.5, candidates=64)
    ix.result_ids = "input"
    out["input"] = ix.search_batch(Q, K)
    ix.result_ids = "internal"
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert len(a[key]) == len(b[key])
        for x, y in zip(a[key], b[key]):
            assert _beq(np.asarray(x), np.asarray(y)), (what, key)


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: f"dim{c[0]}b{c[1]}")
def twin(cph, request):
    dim, bits = request.param
    X, Q, Y = _data(dim)
    mX, mQ, mY = model(X), model(Q), model(Y)
    A = _built(cph, dim, bits, X, metric="cosine")
    B = _built(cph, dim, bits, mX)
    lab = _labels(N, dim)
    A.set_labels(lab, ids="input")
    B.set_labels(lab, ids="input")
    # a radius (in 1 - cos, the same number on both) that returns between 1 and 200 ids for most queries
    d64 = np.sort(_cos_dist64(Q, X), axis=1)
    radius = float(np.float32(np.median(d64[:, 20])))
    hits = (d64 < radius).sum(axis=1)
    assert ((hits >= 1) & (hits <= 200)).mean() > 0.9
    return dict(dim=dim, bits=bits, X=X, Q=Q, Y=Y, mX=mX, mQ=mQ, mY=mY, A=A, B=B, radius=radius, lab=lab)


def test_l2_twin_every_search_has_the_same_bytes(twin):
    A, B, Q, mQ, r = twin["A"], twin["B"], twin["Q"], twin["mQ"], twin["radius"]
    assert A.metric == "cosine" and B.metric == "l2" and A.size == B.size == N
    assert np.array_equal(A.row_map(), B.row_map())
    assert _beq(A.get_vectors(), twin["mX"][A.row_map()])            # what the index stores: model(X), in its own order
    assert _beq(A.get_vectors(), B.get_vectors())
    a = _calls(A, Q, r, N)
    _same(a, _calls(B, mQ, r, N), "built")
    lims = a["range_exact"][0]
    per = np.diff(lims)
    assert ((per >= 1) & (per <= 200)).mean() > 0.8 and lims[-1] > 0


def test_l2_twin_after_remove_add_and_compact(twin):
    A, B, Q, mQ, r = twin["A"], twin["B"], twin["Q"], twin["mQ"], twin["radius"]
    gone = np.random.default_rng(3).choice(N, (N * 3) // 10, replace=False)
    assert A.remove(gone, ids="input") == B.remove(gone, ids="input") == len(gone)
    _same(_calls(A, Q, r, N), _calls(B, mQ, r, N), "removed")
    labY = _labels(100, 99)
    assert np.array_equal(A.add(twin["Y"], labels=labY), B.add(twin["mY"], labels=labY))
    assert A.tail_size == B.tail_size == 100
    assert _beq(A.get_vectors(N, 100), twin["mY"]) and _beq(A.get_vectors(), B.get_vectors())
    _same(_calls(A, Q, r, N + 100, tail=True), _calls(B, mQ, r, N + 100, tail=True), "added")
    # compact passes the live rows through as they are: a second normalisation would change bits here
    ma, mb = A.compact(), B.compact()
    assert np.array_equal(ma, mb) and A.size == B.size == N - len(gone) + 100 and A.tail_size == 0
    assert np.array_equal(A.row_map(), B.row_map()) and _beq(A.get_vectors(), B.get_vectors())
    live = np.concatenate([np.delete(twin["mX"], gone, axis=0), twin["mY"]])
    assert _beq(A.get_vectors(), live[A.row_map()])
    _same(_calls(A, Q, r, A.size), _calls(B, mQ, r, B.size), "compacted")
    assert A.metric_stats()[0] > 0 and B.metric_stats() == (0, 0)


# ---- 3. scale invariance end to end: the test that fails without the feature ---------------------------------------------------
def test_scaling_rows_and_queries_by_powers_of_two_changes_no_byte(cph):
    dim, bits = 24, 4
    X, Q, _ = _data(dim)
    rng = np.random.default_rng(11)
    sx = np.exp2(rng.integers(-8, 9, N)).astype(np.float32)[:, None]
    sq = np.exp2(rng.integers(-8, 9, NQ)).astype(np.float32)[:, None]
    A = _built(cph, dim, bits, X, metric="cosine")
    S = _built(cph, dim, bits, X * sx, metric="cosine")
    assert np.array_equal(A.row_map(), S.row_map()) and _beq(A.get_vectors(), S.get_vectors())
    for kw in (dict(), dict(exact=True)):
        a, s = A.search_batch(Q, K, **kw), S.search_batch(Q * sq, K, **kw)
        assert np.array_equal(a[0], s[0]) and _beq(a[1], s[1]), kw
    # a plain L2 index is not invariant: the same two calls differ
    La, Ls = _built(cph, dim, bits, X), _built(cph, dim, bits, X * sx)
    a, s = La.search_batch(Q, K, exact=True), Ls.search_batch(Q * sq, K, exact=True)
    La.result_ids = Ls.result_ids = "input"
    ai, si = La.search_batch(Q, K, exact=True), Ls.search_batch(Q * sq, K, exact=True)
    assert not _beq(a[1], s[1]) and not np.array_equal(ai[0], si[0])


# ---- 4. truth ---------------------------------------------------------------------------------------------------------------
def test_exact_cosine_distances_against_float64(cph):
    """Every distance within (D + 16) * 2^-24 of the float64 1 - cos: the worst case of a D-term fp32 dot of two vectors of
    squared norm 1/2, plus the norm terms.  The id set is the float64 top-10 wherever the 10th and 11th float64 distances
    differ by more than twice that bound (on this data the rule skips no query; at most 5 % may be)."""
    dim, bits, D = 24, 4, 32
    X, Q, _ = _data(dim)
    A = _built(cph, dim, bits, X, metric="cosine")
    A.result_ids = "input"
    ids, d = A.search_batch(Q, K, exact=True)
    bound = (D + 16) * 2.0 ** -24
    t = _cos_dist64(Q, X)
    err = np.abs(d.astype(np.float64) - np.take_along_axis(t, ids, axis=1))
    print("max |dist - (1 - cos)| =", err.max(), "bound", bound)
    assert (ids >= 0).all() and err.max() <= bound
    st = np.sort(t, axis=1)
    clear = st[:, K] - st[:, K - 1] > 2 * bound
    print("queries skipped by the gap rule:", int((~clear).sum()), "of", NQ)
    assert (~clear).mean() <= 0.05 and (~clear).sum() == 0          # (0 of 64 when the float64 reference was run on a CPU)
    top = np.argsort(t, axis=1)[:, :K]
    for i in np.flatnonzero(clear):
        assert set(ids[i]) == set(top[i]), i
    assert (np.diff(d, axis=1) >= 0).all()


# ---- 5. replicas and parts -----------------------------------------------------------------------------------------------------
def test_replicas_have_the_single_device_bytes(cph):
    dim, bits = 24, 4
    X, Q, _ = _data(dim)
    d = _dev(cph)
    A = _built(cph, dim, bits, X, metric="cosine")
    M = _built(cph, dim, bits, X, devices=[d, d], metric="cosine")
    assert M.metric == "cosine" and _beq(M.get_vectors(), A.get_vectors())
    mask = np.random.default_rng(5).random(N) < 0.5
    for kw in (dict(), dict(exact=True), dict(filter=mask)):
        a, m = A.search_batch(Q, K, **kw), M.search_batch(Q, K, **kw)
        assert np.array_equal(a[0], m[0]) and _beq(a[1], m[1]), kw
    a, m = A.search(Q[3], K), M.search(Q[3], K)
    assert np.array_equal(a[0], m[0]) and _beq(a[1], m[1])
    r = float(np.float32(np.median(np.sort(_cos_dist64(Q, X), axis=1)[:, 20])))
    for x, y in zip(A.range_search(Q, r), M.range_search(Q, r)):
        assert _beq(x, y)


def test_partitioned_equals_the_partitioned_l2_twin(cph):
    dim, bits = 24, 4
    X, Q, _ = _data(dim)
    d = _dev(cph)
    P = _built(cph, dim, bits, X, devices=[d, d], partition=True, metric="cosine")
    T = _built(cph, dim, bits, model(X), devices=[d, d], partition=True)
    assert P.metric == "cosine" and P.part(1).metric == "cosine" and T.part(0).metric == "l2"
    assert _beq(P.part(1).get_vectors(), T.part(1).get_vectors())
    mask = np.random.default_rng(5).random(N) < 0.3
    for kw in (dict(), dict(filter=mask, exact=True)):
        p, t = P.search_batch(Q, K, **kw), T.search_batch(model(Q), K, **kw)
        assert np.array_equal(p[0], t[0]) and _beq(p[1], t[1]), kw
    # a refused row is reported by its global number, and the index is as it was
    before = P.search_batch(Q, K)
    bad = X.copy()
    bad[1200] = 0.0                                # (in part 1)
    bad[1333, 2] = np.nan
    with pytest.raises(ValueError, match=r"row 1200 .*2 such rows"):
        P.build(bad)
    after = P.search_batch(Q, K)
    assert P.is_finalized and P.size == N and np.array_equal(before[0], after[0]) and _beq(before[1], after[1])
    # compact() cuts the live rows again without normalising them twice
    gone = np.arange(0, N, 3)
    assert P.remove(gone) == T.remove(gone) == len(gone)
    assert np.array_equal(P.compact(), T.compact())
    p, t = P.search_batch(Q, K), T.search_batch(model(Q), K)
    assert np.array_equal(p[0], t[0]) and _beq(p[1], t[1])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(cph):
    dim, bits = 24, 4
    X, Q, Y = _data(dim)
    return dict(dim=dim, bits=bits, X=X, Q=Q, Y=Y, A=_built(cph, dim, bits, X, metric="cosine"), B=_built(cph, dim, bits, model(X)))


def test_build_and_add_refuse_rows_without_a_direction(cph, small):
    from cphnsw_mi355x import _lib
    A, X, Q, Y = small["A"], small["X"], small["Q"], small["Y"]
    before = A.search_batch(Q, K)

    def unchanged():
        after = A.search_batch(Q, K)
        return A.is_finalized and A.size == N and A.tail_size == 0 and np.array_equal(before[0], after[0]) and _beq(before[1], after[1])
    for kind, value in (("zero", 0.0), ("nan", np.nan)):
        bad = X.copy()
        bad[700] = value
        with pytest.raises(ValueError, match=r"row 700 "):
            A.build(bad)
        assert unchanged(), kind
        bad = Y.copy()
        bad[[41, 77]] = value
        with pytest.raises(ValueError, match=r"row 41 .*2 such rows"):
            A.add(bad)
        assert unchanged(), kind
    # the metric is fixed once the handle holds rows
    assert _lib.lib().cph_set_metric(A._h, _lib.METRIC_L2) == _lib.INVALID_ARGUMENT
    assert b"empty handle" in _lib.lib().cph_last_error()
    m = C.c_int(-1)
    _lib.check(_lib.lib().cph_get_metric(A._h, C.byref(m)))
    assert m.value == _lib.METRIC_COSINE and unchanged()
    fresh = cph.CPIndex(24, 4)
    fresh.build(model(X))                           # pending rows count too
    assert _lib.lib().cph_set_metric(fresh._h, _lib.METRIC_COSINE) == _lib.INVALID_ARGUMENT
    assert _lib.lib().cph_set_metric(cph.CPIndex(24, 4)._h, 2) == _lib.INVALID_ARGUMENT
    with pytest.raises(ValueError, match="metric"):
        cph.CPIndex(24, 4, metric="dot")


def test_files_carry_the_metric_or_refuse(cph, small, tmp_path):
    A, B, Q = small["A"], small["B"], small["Q"]
    with pytest.raises(ValueError, match="cannot carry the cosine metric"):
        A.save(str(tmp_path / "a.idx"))
    assert not (tmp_path / "a.idx").exists()
    B.save(str(tmp_path / "b.idx"))
    E = cph.CPIndex(24, 4, metric="cosine")
    with pytest.raises(ValueError, match="cannot carry the cosine metric"):
        E.load(str(tmp_path / "b.idx"))
    pa, pb = str(tmp_path / "a.cphn"), str(tmp_path / "b.cphn")
    A.save_native(pa)
    B.save_native(pb)
    # the files differ by the 16-byte record alone: sections may move by whole pages, so compare through a load
    E.load_native(pa)
    assert E.metric == "cosine" and E.size == N
    for kw in (dict(), dict(exact=True)):
        a, e = A.search_batch(Q, K, **kw), E.search_batch(Q, K, **kw)
        assert np.array_equal(a[0], e[0]) and _beq(a[1], e[1]), kw
    E.save_native(str(tmp_path / "again.cphn"))
    assert (tmp_path / "again.cphn").read_bytes() == (tmp_path / "a.cphn").read_bytes()
    with pytest.raises(ValueError, match="cosine.*l2"):
        cph.CPIndex(24, 4).load_native(pa)
    with pytest.raises(ValueError, match="l2.*cosine"):
        E.load_native(pb)
    a, e = A.search_batch(Q, K), E.search_batch(Q, K)                   # the refused load left E as it was
    assert np.array_equal(a[0], e[0]) and _beq(a[1], e[1])
    # partitioned: every part's file carries the record
    d = _dev(cph)
    P = _built(cph, 24, 4, small["X"], devices=[d, d], partition=True, metric="cosine")
    P.save_native(str(tmp_path / "parts.cphn"))
    P2 = cph.CPIndex(24, 4, devices=[d, d], partition=True, metric="cosine")
    P2.load_native(str(tmp_path / "parts.cphn"))
    p, p2 = P.search_batch(Q, K), P2.search_batch(Q, K)
    assert np.array_equal(p[0], p2[0]) and _beq(p[1], p2[1])
    with pytest.raises(ValueError, match="cosine.*l2"):
        cph.CPIndex(24, 4, devices=[d, d], partition=True).load_native(str(tmp_path / "parts.cphn"))


def test_l2_native_file_has_the_bytes_of_the_older_library(cph, tmp_path):
    """tests/golden/remove_g16_b1_parent_native_f2.cphn.gz was written by write_native of a commit before the metric existed
    (g16 1-bit fixture, row map (7 i + 3) mod n): an L2 index must still be written as exactly those bytes."""
    ix = cph.CPIndex(DATASETS["g16"]["dim"], 1)
    ix.load(fixture_path("g16", 1))
    n = ix.size
    ix.set_row_map((7 * np.arange(n) + 3) % n)
    ix.save_native(str(tmp_path / "l2.cphn"))
    with gzip.open(os.path.join(HERE, "golden", "remove_g16_b1_parent_native_f2.cphn.gz"), "rb") as f:
        assert (tmp_path / "l2.cphn").read_bytes() == f.read()
    assert ix.metric == "l2" and ix.metric_stats() == (0, 0)


def test_a_query_without_a_direction_searches_as_the_zero_vector(small):
    A, B, Q = small["A"], small["B"], small["Q"]
    q = Q[:4].copy()
    q[0] = 0.0
    q[1, 5] = np.nan
    q[2, 0] = np.inf
    zero = np.zeros_like(q[0])
    for kw in (dict(), dict(exact=True)):
        ids, d = A.search_batch(q, K, **kw)
        assert (ids >= 0).all() and np.isfinite(d).all()
        for i in range(3):
            # each distance is that id's stored norm: what the L2 twin computes for the zero vector, about 1/2
            assert _beq(d[i], B.exact_l2(zero, ids[i])), (kw, i)
            stored = (A.get_vectors()[ids[i]].astype(np.float64) ** 2).sum(axis=1)
            assert np.abs(d[i] - stored).max() <= 24 * 2.0 ** -24 and np.abs(d[i] - 0.5).max() < 1e-5
        good = A.search_batch(Q[3:4], K, **kw)
        assert np.array_equal(ids[3], good[0][0]) and _beq(d[3], good[1][0])
    ids, d = A.search(zero, K)
    assert len(ids) == K and _beq(d, B.exact_l2(zero, ids))


# ---- 7. L2 untouched -----------------------------------------------------------------------------------------------------------
def test_an_l2_index_launches_and_allocates_nothing_for_the_metric(cph, small):
    from cphnsw_mi355x import _lib
    import torch
    X, Q, Y = small["X"], small["Q"], small["Y"]
    for metric in ("l2", "cosine"):
        ix = _built(cph, 24, 4, X, metric=metric)
        m = C.c_int(-1)
        _lib.check(_lib.lib().cph_get_metric(ix._h, C.byref(m)))
        assert m.value == (_lib.METRIC_COSINE if metric == "cosine" else _lib.METRIC_L2)
        built = ix.metric_stats()
        ix.search(Q[0], K)
        ix.search_batch(Q[:16], K)
        ix.search_batch(Q, K)
        ix.search_batch(Q, K, exact=True)
        ix.search_batch(Q, K, filter=[np.arange(N) % 2 == 0, np.arange(N) % 3 == 0], filter_of=np.arange(NQ) % 2)
        dq = torch.from_numpy(Q).to(f"cuda:{ix.devices[0]}")
        ix.search_batch_device(dq, K)
        torch.cuda.synchronize()
        ix.range_search(Q, 0.5)
        ix.range_search(Q, 0.5, exact=False, max_results=16)
        ix.search_diverse(Q, K)
        ix.add(Y)
        ix.search_batch(Q, K)
        searched = ix.metric_stats()
        ix.compact()
        if metric == "l2":
            assert built == searched == ix.metric_stats() == (0, 0)
        else:
            # one launch for the build, one per batch (10 above: the coalesced single query, the two range searches and
            # the diverse search included), one for add(), none for compact(); the buffers exist while the index does
            assert built == (1, 0) and searched[0] == 1 + 10 + 1 and searched[1] > 0
            assert ix.metric_stats()[0] == searched[0]
