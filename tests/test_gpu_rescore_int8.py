"""Two-stage search over int8 rows on the GPU (make_rescore_vectors(dtype="int8"), csrc/device_rescore_i8.h).

The yardstick is the numpy model below: the statement of DESIGN.md section 4, "int8 rows", with int64 sums.  Rows in: the
stored bytes, scales and norms of an object.  The kernel hook: all three outputs, byte for byte, on candidate rows with
padding, repeats, ids out of range and twin rows.  End to end: a call against the model applied to the rows search_batch
returns on the same handle.  Before the hook runs, the model itself is held against float64 on the same data."""
import numpy as np
import pytest

from diverse_model import FMAX
from golden_util import DATASETS, fixture_path
from rescore_model import hook_rescore_rows, same_bytes

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32 = np.float32
N_TWINS = 8


# ---- the model ---------------------------------------------------------------------------------------------------------------
def _codes(v, scale, lim):
    """clamp(rint(v / scale), -lim, lim) in float32, ties to even; a NaN quotient (0 / 0) gives 0 -> int64."""
    with np.errstate(all="ignore"):
        r = np.rint(np.asarray(v, F32) / F32(scale))
    return np.where(np.isnan(r), F32(0), np.clip(r, -lim, lim)).astype(np.int64)


def norms_model(c, s):
    S2 = (c.astype(np.int64) ** 2).sum(axis=1)
    with np.errstate(over="ignore"):
        return (s * s) * S2.astype(F32)


def rows_model(x):
    """float32 [n, d] -> (codes int8 [n, d], scales float32 [n], norms float32 [n])."""
    x = np.asarray(x, F32)
    m = np.abs(x).max(axis=1)
    s = m / F32(127)
    c = np.stack([_codes(x[i], s[i], 127) if m[i] != 0 else np.zeros(x.shape[1], np.int64) for i in range(len(x))]).astype(np.int8)
    return c, s, norms_model(c, s)


def stored_model(c, row_map=None):
    """The stored bytes: 16-byte pieces, zeros behind dim_full; under a row map position i holds input row row_map[i]."""
    out = np.zeros((c.shape[0], -(-c.shape[1] // 16) * 16), np.int8)
    out[:, :c.shape[1]] = c
    return (out if row_map is None else out[row_map]).view(np.uint8)


def query_model(q):
    """-> (t int64 [d], sq, qn), or None for a query whose maximum is not finite."""
    qmax = np.abs(q).max()
    if not qmax < np.inf:
        return None
    sq = qmax / F32(16256)
    t = _codes(q, sq, 16256) if qmax != 0 else np.zeros(q.shape[0], np.int64)
    h = (t + 64) >> 7
    l = t - 128 * h
    assert np.abs(h).max() <= 127 and l.min() >= -64 and l.max() <= 63          # the two planes are int8
    with np.errstate(over="ignore"):
        return t, sq, (sq * sq) * np.int64((t * t).sum()).astype(F32)


def scores_model(qm, c, s, xn, metric):
    t, sq, qn = qm
    I = c.astype(np.int64) @ t                                                   # = 128 H + L
    with np.errstate(all="ignore"):
        dot = (s * sq) * I.astype(F32)
        if metric == "ip":
            return F32(0) - dot
        v = (qn + xn) - F32(2) * dot
    return np.where(v < 0, F32(0), v)


def rescore_model(ids, dist, k, fq, c, s, xn, metric, rows=None):
    n = ids.shape[0]
    out = (np.full((n, k), -1, np.int64), np.full((n, k), FMAX, F32), np.full((n, k), FMAX, F32))
    for q in range(n):
        qm = query_model(fq[q])
        row = ids[q].tolist()
        pos = np.array([j for j, i in enumerate(row) if 0 <= i < len(c) and i not in row[:j]], np.int64)
        if qm is None or pos.size == 0:
            continue
        cid = ids[q, pos]
        sc = scores_model(qm, c[cid], s[cid], xn[cid], metric)
        keep = ~np.isnan(sc)
        pos, cid, sc = pos[keep], cid[keep], sc[keep]
        order = np.lexsort((cid, sc))[:k]
        m = order.shape[0]
        out[0][q, :m] = cid[order] if rows is None else np.asarray(rows)[cid[order]]
        out[1][q, :m] = sc[order]
        out[2][q, :m] = dist[q, pos[order]]
    return out


def check_model_against_float64(x, fq, c, s, xn, metric):
    """Every model score lies within 8 u (|q^|^2 + |x^|^2 + |q^ . x^|) of the float64 score of the dequantised pair, and the
    dequantised dot within (s / 2 + u m) |q|_1 + (sq / 2 + u qmax) |x^|_1 of the dot of the float rows."""
    xh = s.astype(np.float64)[:, None] * c
    for q in fq:
        qm = query_model(q)
        if qm is None:
            continue
        t, sq, _ = qm
        qh = np.float64(sq) * t
        dot = xh @ qh
        q2, x2 = qh @ qh, (xh * xh).sum(axis=1)
        want = -dot if metric == "ip" else np.maximum(0.0, q2 + x2 - 2 * dot)
        got = scores_model(qm, c, s, xn, metric).astype(np.float64)
        assert (np.abs(got - want) <= 8 * U * (q2 + x2 + np.abs(dot))).all()
        m, qmax = np.abs(x).max(axis=1).astype(np.float64), np.float64(np.abs(q).max())
        bound = (s / 2.0 + U * m) * np.abs(q, dtype=np.float64).sum() + (sq / 2.0 + U * qmax) * np.abs(xh).sum(axis=1)
        assert (np.abs(dot - x.astype(np.float64) @ q.astype(np.float64)) <= bound).all()


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _load(cph, name, bits, **kw):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits, **kw)
    ix.load(fixture_path(name, bits))
    return ix


@pytest.fixture(scope="module")
def g16(cph):
    return _load(cph, "g16", 1)


@pytest.fixture(scope="module")
def g128(cph):
    return _load(cph, "g128", 4)


def _full_rows(n, dim):
    """float32 [n, dim]; the last N_TWINS rows repeat the first ones (equal scores under other ids); row 5 is zero."""
    x = np.random.default_rng(1009 * dim + n).standard_normal((n, dim)).astype(F32)
    x[5] = 0
    x[n - N_TWINS:] = x[:N_TWINS]
    return x


def _candidates(n_ids, n, Cn, seed):
    """Rows with padding (-1), ids beyond the object, repeats and, in row 0, a twin pair."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(-1, n_ids + 2, (n, Cn))
    dist = np.sort(rng.random((n, Cn), dtype=F32), axis=1)
    if Cn >= 2:
        ids[0, 0], ids[0, 1] = n_ids - N_TWINS, 0
        ids[1, Cn - 1] = ids[1, 0]
    return ids, dist


# ---- rows in ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (1, 15, 16, 17, 72, 1024, 1040))
def test_rows_in_has_the_bytes_of_the_model(g16, dim):
    ix, n = g16, g16.size
    full = _full_rows(n, dim)
    rm = np.random.default_rng(dim).permutation(n)
    ix.set_row_map(rm)
    try:
        for rows in (full, full.astype(np.float16)):
            c, s, xn = rows_model(rows.astype(F32))
            assert not c[5].any() and s[5] == 0 and xn[5] == 0
            for space, row_map in (("internal", None), ("input", rm)):
                rv = ix.make_rescore_vectors(rows, ids=space, dtype="int8")
                pick = slice(None) if row_map is None else row_map
                assert rv.dtype == "int8" and rv.row_bytes == -(-dim // 16) * 16 and rv.nbytes == n * (rv.row_bytes + 8)
                stored, norms = rv.stored()
                assert stored.tobytes() == stored_model(c, row_map).tobytes(), (rows.dtype, space)
                assert rv.scales().tobytes() == s[pick].tobytes() and norms.tobytes() == xn[pick].tobytes(), (rows.dtype, space)
                assert rv.scales(5, 7).tobytes() == s[pick][5:12].tobytes()
                rv.close()
        # codes the caller holds: stored as given, -128 included
        codes = np.random.default_rng(dim + 1).integers(-128, 128, (n, dim)).astype(np.int8)
        codes[3] = -128
        scales = np.random.default_rng(dim + 2).random(n, dtype=F32)
        scales[7] = 0
        for sc, space, row_map in ((None, "internal", None), (scales, "internal", None), (scales, "input", rm)):
            rv = ix.make_rescore_vectors(codes, ids=space, dtype="int8", scales=sc)
            s = np.ones(n, F32) if sc is None else sc
            pick = slice(None) if row_map is None else row_map
            stored, norms = rv.stored()
            assert stored.tobytes() == stored_model(codes, row_map).tobytes()
            assert rv.scales().tobytes() == s[pick].tobytes() and norms.tobytes() == norms_model(codes, s)[pick].tobytes()
            rv.close()
    finally:
        ix.set_row_map(None)


def test_bad_rows_and_scales_are_refused(g16):
    ix, n = g16, g16.size
    full = _full_rows(n, 24)
    codes = np.ones((n, 24), np.int8)
    scales = np.ones(n, F32)
    for row, col, bad in ((211, 5, np.nan), (17, 23, np.inf)):
        x = full.copy()
        x[row, col] = bad
        x[250, 0] = bad
        with pytest.raises(ValueError, match=rf"row {row} .*\(2 such rows"):
            ix.make_rescore_vectors(x, ids="internal", dtype="int8")
    for bad in (-1.0, np.nan, np.inf):
        sc = scales.copy()
        sc[[40, 200]] = bad
        with pytest.raises(ValueError, match=r"row 40 .*\(2 such rows"):
            ix.make_rescore_vectors(codes, ids="internal", dtype="int8", scales=sc)
    for kw in (dict(rows=codes, dtype="float16"), dict(rows=full, dtype="int8", scales=scales), dict(rows=codes, dtype="int8", scales=scales[:-1])):
        with pytest.raises(ValueError):
            ix.make_rescore_vectors(kw.pop("rows"), ids="internal", **kw)
    rv = ix.make_rescore_vectors(full, ids="internal")
    with pytest.raises(ValueError, match="INT8"):
        rv.scales()
    rv.close()


# ---- the kernel against the model -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def objects(g128):
    """(dim, metric) -> (rv, x, c, s, xn, fq) on g128, made on first use; the model is held against float64 first."""
    made = {}

    def get(dim, metric):
        if (dim, metric) not in made:
            x = _full_rows(g128.size, dim)
            c, s, xn = rows_model(x)
            fq = np.random.default_rng(dim).standard_normal((6, dim)).astype(F32)
            fq[2], fq[3, dim // 2] = 0, np.inf
            check_model_against_float64(x, fq, c, s, xn, metric)
            made[(dim, metric)] = (g128.make_rescore_vectors(x, ids="internal", dtype="int8", metric=metric), x, c, s, xn, fq)
        return made[(dim, metric)]
    return get


@pytest.mark.parametrize("Cn,k", ((1, 1), (64, 10), (100, 100), (1024, 10)))
@pytest.mark.parametrize("metric", ("l2", "ip"))
@pytest.mark.parametrize("dim", (7, 16, 72, 1024, 1040))
def test_kernel_hook_matches_the_model(g128, objects, dim, metric, Cn, k):
    rv, x, c, s, xn, fq = objects(dim, metric)
    ids, dist = _candidates(g128.size, len(fq), Cn, 131 * Cn + k)
    want = rescore_model(ids, dist, k, fq, c, s, xn, metric)
    assert (want[0][3] == -1).all() and (want[1][3] == FMAX).all()             # the Inf query: a row of padding
    got = hook_rescore_rows(g128, rv, ids, dist, k, fq)
    assert not (got[1].view(np.uint32) == 0xA5A5A5A5).any()                    # every slot was written
    assert same_bytes(got, want)


@pytest.mark.parametrize("metric", ("l2", "ip"))
def test_kernel_hook_past_32_bits(g16, metric):
    """dim_full = 8192, rows of all +127, all -128 and alternating signs against queries whose every t_i is +/-16256: |I|
    reaches 1.7e10 and T2 2.2e12."""
    n, dim = g16.size, 8192
    rng = np.random.default_rng(8192)
    codes = rng.integers(-128, 128, (n, dim)).astype(np.int8)
    alt = np.where(np.arange(dim) % 2 == 0, 1, -1)
    codes[0], codes[1], codes[2] = 127, -128, 127 * alt
    scales = (rng.random(n, dtype=F32) + F32(0.5)) * F32(0.01)
    fq = np.stack([np.full(dim, 0.75), -0.75 * alt, np.full(dim, -3.0)]).astype(F32)
    xn = norms_model(codes, scales)
    assert abs(int(codes[1].astype(np.int64) @ query_model(fq[2])[0])) > 2 ** 32 and int((query_model(fq[0])[0] ** 2).sum()) > 2 ** 40
    rv = g16.make_rescore_vectors(codes, ids="internal", dtype="int8", metric=metric, scales=scales)
    ids = np.tile(np.arange(64), (3, 1))
    dist = np.zeros((3, 64), F32)
    want = rescore_model(ids, dist, 10, fq, codes, scales, xn, metric)
    assert same_bytes(hook_rescore_rows(g16, rv, ids, dist, 10, fq), want)
    rv.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state", ("plain", "filter", "input", "replicas"))
def test_end_to_end(cph, state):
    ix = _load(cph, "g128", 4, **(dict(devices=[0, 0]) if state == "replicas" else {}))
    if state == "replicas":
        ix.set_min_shard(1)
    n, rng = ix.size, np.random.default_rng(7)
    full = rng.standard_normal((n, 200)).astype(F32) * F32(0.5)
    full[:, :ix.dim] = ix.get_vectors()
    FQ = np.ascontiguousarray(full[rng.integers(0, n, 12)] + F32(0.3) * rng.standard_normal((12, 200)).astype(F32))
    Q = np.ascontiguousarray(FQ[:, :ix.dim])
    c, s, xn = rows_model(full)
    rv = ix.make_rescore_vectors(full, ids="internal", dtype="int8")
    kw = dict(filter=ix.make_filter(rng.random(n) < 0.4, ids="internal")) if state == "filter" else {}
    ids, dist = ix.search_batch(Q, 64, **kw)                                   # (internal ids: result_ids is still the default)
    rows = None
    if state == "input":
        rows = rng.permutation(n)
        ix.set_row_map(rows)
        ix.result_ids = "input"
    got = ix.search_rescored(Q, 10, rv, full_queries=FQ, candidates=64, **kw)
    assert same_bytes(got, rescore_model(ids, dist, 10, FQ, c, s, xn, "l2", rows))
    rv.close()
