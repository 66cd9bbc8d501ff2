"""Exhaustive int8 rescoring on the GPU: search_rescored(..., candidates="all") and cph_rescore_all_hook
(csrc/device_rescore_i8_all.h) against the statement of DESIGN.md section 4, "int8 rows", in plain numpy.

Integer sums are exact and every float operation is stated, so ids and scores are compared as bytes; `first` is FLT_MAX."""
import numpy as np
import pytest

from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

F32 = np.float32
FMAX = np.finfo(F32).max


# ---- the statement -----------------------------------------------------------------------------------------------------------
def reference(fq, codes, s, xn, metric, k, allow=None, rows=None):
    """-> (ids, score, first).  codes int8 [size, dim], s / xn float32 [size] as stored; allow: bool [n, size] or None."""
    n, size = fq.shape[0], codes.shape[0]
    out = (np.full((n, k), -1, np.int64), np.full((n, k), FMAX, F32), np.full((n, k), FMAX, F32))
    c64 = codes.astype(np.int64)
    for i, q in enumerate(fq):
        qmax = np.abs(q).max()
        if not qmax < np.inf:
            continue
        sq = qmax / F32(16256)
        with np.errstate(all="ignore"):
            r = np.rint(q / sq)
        t = np.where(np.isnan(r) | (qmax == 0), F32(0), np.clip(r, -16256, 16256)).astype(np.int64)
        h = (t + 64) >> 7
        l = t - 128 * h
        H = c64 @ h
        L = c64 @ l
        I = 128 * H + L
        If = I.astype(np.float64).astype(F32)
        T2f = np.float64((t * t).sum()).astype(F32)
        with np.errstate(all="ignore"):
            qn = (sq * sq) * T2f
            ssq = s * sq
            dot = ssq * If
            if metric == "ip":
                score = F32(0) - dot
            else:
                sum_ = qn + xn
                two = F32(2) * dot
                v = sum_ - two
                score = np.where(v < 0, F32(0), v)
        ids = np.flatnonzero(~np.isnan(score) & (np.ones(size, bool) if allow is None else allow[i]))
        order = ids[np.lexsort((ids, score[ids]))][:k]
        out[0][i, :len(order)] = order if rows is None else np.asarray(rows)[order]
        out[1][i, :len(order)] = score[order]
    return out


def stored(rv, dim):
    rows, xn = rv.stored()
    return rows.view(np.int8)[:, :dim], rv.scales(), xn


def same(got, want):
    return (got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            and got[2].tobytes() == want[2].tobytes() and (got[2] == FMAX).all())


def hook(ix, rv, fq, k, allow=None, parts=0):
    from cphnsw_mi355x import _lib
    n = fq.shape[0]
    out = (np.empty((n, k), np.int64), np.empty((n, k), F32), np.empty((n, k), F32))
    words = None
    if allow is not None:
        bits = np.zeros((n, -(-ix.size // 32) * 32), bool)
        bits[:, :ix.size] = allow
        words = np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint32))
    fq = np.ascontiguousarray(fq, F32)
    _lib.check(_lib.lib().cph_rescore_all_hook(ix._h, fq.ctypes.data, n, rv._hs[0], None if words is None else words.ctypes.data, k, parts,
                                               *[o.ctypes.data for o in out]))
    assert not (out[1].view(np.uint32) == 0xA5A5A5A5).any() and not (out[2].view(np.uint32) == 0xA5A5A5A5).any()
    return out


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


@pytest.fixture(scope="module")
def g128(cph):
    ix = cph.CPIndex(DATASETS["g128"]["dim"], 4)
    ix.load(fixture_path("g128", 4))
    return ix


@pytest.fixture(scope="module")
def big(cph):
    """1,100 rows: nine 128-row steps, the last one partial."""
    ix = cph.CPIndex(16, 1)
    ix.build(np.random.default_rng(11).standard_normal((1100, 16)).astype(F32))
    ix.finalize()
    return ix


def full_rows(n, dim, seed):
    """The last 8 rows repeat the first 8 (equal scores under other ids); row 5 is zero."""
    x = np.random.default_rng(seed).standard_normal((n, dim)).astype(F32)
    x[5] = 0
    x[n - 8:] = x[:8]
    return x


def queries(n, dim, seed):
    fq = np.random.default_rng(seed).standard_normal((n, dim)).astype(F32)
    if n > 2:
        fq[1] = 0
        fq[2, dim // 2] = np.nan
    return fq


# ---- the kernels against the statement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,metric,n,k,filt", (
    (16, "l2", 1, 1, None), (16, "ip", 130, 10, "one"), (40, "l2", 130, 1024, None), (40, "ip", 5, 10, "each"),
    (64, "l2", 5, 10, "one"), (64, "ip", 1, 1024, None), (272, "l2", 5, 10, None), (300, "ip", 130, 10, "each")))
def test_hook_matches_the_statement(g128, dim, metric, n, k, filt):
    size = g128.size
    rv = g128.make_rescore_vectors(full_rows(size, dim, dim), ids="internal", dtype="int8", metric=metric)
    fq = queries(n, dim, dim + n)
    rng = np.random.default_rng(k)
    allow = None if filt is None else (np.tile(rng.random(size) < 0.05, (n, 1)) if filt == "one" else rng.random((n, size)) < 0.3)
    want = reference(fq, *stored(rv, dim), metric, k, allow)
    if n > 2:
        assert (want[0][2] == -1).all()                               # the NaN query: a row of padding
    assert same(hook(g128, rv, fq, k, allow), want)
    rv.close()


@pytest.mark.parametrize("metric", ("l2", "ip"))
@pytest.mark.parametrize("parts", (0, 3))
def test_parts_fold(big, metric, parts):
    rv = big.make_rescore_vectors(full_rows(big.size, 40, 7), ids="internal", dtype="int8", metric=metric)
    fq = queries(130, 40, 9)
    allow = np.random.default_rng(3).random((130, big.size)) < 0.5
    for k in (10, 1024):
        assert same(hook(big, rv, fq, k, allow, parts), reference(fq, *stored(rv, 40), metric, k, allow))
    rv.close()


@pytest.mark.parametrize("metric", ("l2", "ip"))
def test_past_32_bits(g128, metric):
    """dim_full = 1100, rows of all +127 and all -128 against constant-sign queries: |I| = 128 H + L passes 2^31."""
    size, dim = g128.size, 1100
    codes = np.random.default_rng(1100).integers(-128, 128, (size, dim)).astype(np.int8)
    codes[0], codes[1] = 127, -128
    scales = (np.random.default_rng(1).random(size, dtype=F32) + F32(0.5)) * F32(0.01)
    rv = g128.make_rescore_vectors(codes, ids="internal", dtype="int8", metric=metric, scales=scales)
    fq = np.stack([np.full(dim, 0.75), np.full(dim, -3.0)]).astype(F32)
    c, s, xn = stored(rv, dim)
    assert abs(int(c[1].astype(np.int64).sum()) * 16256) > 2 ** 31
    assert same(hook(g128, rv, fq, 10), reference(fq, c, s, xn, metric, 10))
    rv.close()


# ---- the public call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ("plain", "filter", "filter_of", "input", "device"))
def test_end_to_end(cph, state):
    ix = cph.CPIndex(DATASETS["g128"]["dim"], 4)
    ix.load(fixture_path("g128", 4))
    size, dim, rng = ix.size, 200, np.random.default_rng(5)
    rv = ix.make_rescore_vectors(full_rows(size, dim, 200), ids="internal", dtype="int8")
    fq = queries(12, dim, 13)
    c, s, xn = stored(rv, dim)
    allow, rows, kw = None, None, {}
    if state == "filter":
        m = rng.random(size) < 0.05
        allow, kw = np.tile(m, (12, 1)), dict(filter=ix.make_filter(m, ids="internal"))
    elif state == "filter_of":
        ms = rng.random((3, size)) < 0.3
        fo = rng.integers(-1, 3, 12)
        fo[0] = -1
        best = reference(fq, c, s, xn, "l2", 4, ms[fo])[0]
        gone = np.unique(best[best >= 0])[::2]                               # some true neighbours
        ix.remove(gone, ids="internal")
        live = np.ones(size, bool)
        live[gone] = False
        allow = np.where((fo >= 0)[:, None], ms[fo], True) & live
        kw = dict(filter=[ix.make_filter(m, ids="internal") for m in ms], filter_of=fo)
    elif state == "input":
        rows = rng.permutation(size)
        ix.set_row_map(rows)
        ix.result_ids = "input"
    want = reference(fq, c, s, xn, "l2", 10, allow, rows)
    if state == "device":
        import torch
        got = tuple(t.cpu().numpy() for t in ix.search_rescored_device(torch.from_numpy(fq).cuda(), 10, rv, candidates="all"))
    else:
        got = ix.search_rescored(fq, 10, rv, candidates="all", **kw)
    assert same(got, want)
    if state == "plain":                                                     # the two-stage call over every row agrees
        two = ix.search_rescored(fq, 10, rv, candidates=size, exact=True)
        assert two[0].tobytes() == got[0].tobytes() and two[1].tobytes() == got[1].tobytes()
    rv.close()


@pytest.mark.parametrize("case", ("float16", "everything", "partitioned"))
def test_refusals(cph, g128, case):
    fq = queries(3, 24, 1)
    if case == "partitioned":
        ix = cph.CPIndex(128, 4, devices=[0, 0], partition=True)
        with pytest.raises(ValueError, match="partitioned"):
            ix.search_rescored(np.zeros((3, 128), F32), 10, None, full_queries=fq, candidates="all")
        return
    rv = g128.make_rescore_vectors(full_rows(g128.size, 24, 2), ids="internal", dtype="float16" if case == "float16" else "int8")
    with pytest.raises(ValueError, match="int8" if case == "float16" else '"all"'):
        g128.search_rescored(np.zeros((3, 128), F32), 10, rv, full_queries=fq, candidates="all" if case == "float16" else "everything")
    rv.close()
