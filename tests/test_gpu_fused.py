"""Fused search on the GPU (CPIndex.search_fused, search_fused_device, cph_fused_rows_hook): several query vectors per query,
the k best rows by the exact weighted sum of their distances.

The yardstick is tests/fused_model.py.  The kernel hook is compared with it and with the host twin on the synthetic batch of
that file against golden indexes of D = 16, 128 and 2048 (the last one takes the chunked path of the candidate loop) that got
three added rows, two of them one vector.  An end-to-end call is compared with the model applied to (search_batch over the
n * T vectors at k = C on the same handle, exact_l2 bytes) under every option the underlying search takes.  Every comparison
is a byte comparison."""
import numpy as np
import pytest

from fused_model import (FMAX, U_SIZES, OracleQueryDists, check_batch_promises, fused_model_batch, hook_fused_rows, host_fused_rows,
                         same_bytes, synth_batch, union_sizes)
from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _stored(ix, D):
    """(raw [size, D] zero-padded, norm_sq [size]) of the handle for the host twin: exact_l2 of the zero vector is
    (+0 + norm) - 2 * 0 = the stored norm, bit for bit."""
    raw = np.zeros((ix.size, D), np.float32)
    raw[:, :ix.dim] = ix.get_vectors(0, ix.size)
    return raw, ix.exact_l2(np.zeros(ix.dim, np.float32), np.arange(ix.size, dtype=np.uint32))


# ---- the kernels against the host twin and the model -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,bits", (("g16", 1), ("g128", 4), ("g2048", 1)))
def test_hook_matches_host_twin_and_model(cph, name, bits):
    spec = DATASETS[name]
    ix = cph.CPIndex(spec["dim"], bits)
    ix.load(fixture_path(name, bits))
    n0 = ix.size
    ix.set_row_map(np.random.default_rng(5).permutation(n0))
    v = np.random.default_rng(n0).standard_normal((2, spec["dim"])).astype(np.float32)
    ix.add(np.stack([v[0], v[1], v[0]]))                       # ids n0 and n0 + 2: one vector under two ids
    twins = (n0, n0 + 2)
    raw, norm = _stored(ix, spec["D"])
    n_ids = ix.size
    assert n_ids == n0 + 3 and raw[twins[0]].tobytes() == raw[twins[1]].tobytes() and norm[twins[0]].tobytes() == norm[twins[1]].tobytes()
    seen_u = set()
    for T, C_, ks, whole in ((5, 14, (1, 10, 67), True), (64, 128, (20,), False)):
        batch = synth_batch(raw, spec["dim"], T, C_, twins, seed=bits)
        if not whole:                                         # ONE query of 8,192 entries: the full sort
            at = batch["kinds"].index("zero")
            batch = dict(cand=batch["cand"][at:at + 1], Q=batch["Q"][at:at + 1], n_vectors=batch["n_vectors"][at:at + 1],
                         weights=batch["weights"][at:at + 1], kinds=["zero"], mark={})
            assert batch["cand"].size == 8192 and batch["n_vectors"][0] == 64
        dist = OracleQueryDists(raw, norm, batch["Q"])
        if whole:
            check_batch_promises(batch, dist, n_ids, twins)
            seen_u |= set(union_sizes(batch, n_ids))
        cand, nv, w = batch["cand"], batch["n_vectors"], batch["weights"]
        for space in ("internal", "input"):
            ix.result_ids = space
            rows = ix.row_map().astype(np.uint32) if space == "input" else None
            for k in ks:
                want = fused_model_batch(cand, nv, w, dist, n_ids, k, rows)
                assert same_bytes(host_fused_rows(cand, nv, w, dist.q, raw, norm, k, rows), want), (name, T, k, space, "host twin")
                assert same_bytes(hook_fused_rows(ix, cand, batch["Q"], nv, w, k), want), (name, T, k, space, "kernels")
        ix.result_ids = "internal"
        if not whole:
            k = ks[0]
            want = fused_model_batch(cand, None, np.ones_like(w), dist, n_ids, k)
            assert same_bytes(hook_fused_rows(ix, cand, batch["Q"], None, None, k), want), (name, "no n_vectors, no weights")
    assert seen_u >= set(U_SIZES)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
class Dists:
    """dist(q, t, ids) of the model from the handle: exact_l2 of the vector (cosine: normalised as the search does) against
    every id, computed once per vector."""

    def __init__(self, ix, Q, cosine=False):
        from cosine_model import model
        self.ix, self.rows = ix, {}
        self.Q = model(Q.reshape(-1, Q.shape[2])).reshape(Q.shape) if cosine else Q
        self.all = np.arange(ix.size, dtype=np.uint32)

    def __call__(self, q, t, ids):
        if (q, t) not in self.rows:
            self.rows[q, t] = self.ix.exact_l2(self.Q[q, t], self.all)
        return self.rows[q, t][np.asarray(ids, np.int64)]


def _rows_internal(ix, Q, C_, **kw):
    """The candidate rows of the statement: search_batch over the n * T vectors at k = C, in internal ids, on the same handle;
    a per-query argument serves the T vectors of its query."""
    n, T, dim = Q.shape
    for name in ("filter_of", "label"):
        if name in kw and np.ndim(kw[name]) == 1:
            kw[name] = np.repeat(np.asarray(kw[name]), T)
    was = ix.result_ids
    ix.result_ids = "internal"
    try:
        ids, _ = ix.search_batch(Q.reshape(n * T, dim), C_, **kw)
    finally:
        ix.result_ids = was
    return ids.reshape(n, T, C_)


def _expect(ix, Q, k, C_, weights, n_vectors, cosine=False, **kw):
    cand = _rows_internal(ix, Q, C_, **kw)
    rows = ix.row_map() if ix.result_ids == "input" else None
    n, T, _ = Q.shape
    w = np.ascontiguousarray(np.broadcast_to(np.ones(T, np.float32) if weights is None else np.asarray(weights, np.float32), (n, T)))
    return fused_model_batch(cand, n_vectors, w, Dists(ix, Q, cosine), ix.size, k, rows), cand


def _queries(Q, n, T, seed):
    """n queries of T vectors around rows of Q: rewrites of one question."""
    rng = np.random.default_rng(seed)
    base = Q[rng.integers(0, len(Q), n)][:, None, :]
    return (base + np.float32(0.2) * np.abs(base).mean() * rng.standard_normal((n, T, Q.shape[1]))).astype(np.float32)


N, T, C0, K = 5, 3, 32, 10
WEIGHTS = np.array([[1.0, 0.5, 0.25], [1.0, -0.5, 2.0], [0.0, 1.0, 1.0], [3.0, 3.0, 3.0], [1.0, 1.0, -1.0]], np.float32)
NV = np.array([3, 2, 3, 1, 3], np.int32)


def _open(cph, gold, name="g16", bits=1):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits))
    ix.set_row_map(np.random.default_rng(5).permutation(ix.size))      # (a v2 file carries none)
    return ix, gold[f"Q/{name}"][:12]


@pytest.mark.parametrize("state", ("plain", "input", "removed", "added"))
def test_end_to_end_options(cph, gold, state):
    ix, Q0 = _open(cph, gold)
    n0 = ix.size
    rng = np.random.default_rng(n0 + len(state))
    labels = rng.integers(0, 4, n0).astype(np.int64)
    ix.set_labels(labels, ids="internal")
    live = np.ones(n0, bool)
    if state == "input":
        ix.result_ids = "input"
    if state in ("removed", "added"):
        gone = rng.choice(n0, n0 // 5, replace=False)
        assert ix.remove(gone, ids="internal") == len(gone)
        live[gone] = False
    if state == "added":
        twin = ix.get_vectors(5, 1)
        extra = np.concatenate([twin, twin + np.float32(0.25), rng.standard_normal((6, ix.dim)).astype(np.float32)])
        extra_labels = np.array([0, 1, 2, 3, 0, 1, 2, 3], np.int64)
        ix.add(extra, labels=extra_labels)
        labels = np.concatenate([labels, extra_labels])
        live = np.concatenate([live, np.ones(len(extra_labels), bool)])
    n = ix.size
    mask = rng.random(n) < 0.4
    small = rng.random(n) < 0.08
    f = ix.make_filter(mask, ids="internal")
    f2 = ix.make_filter(small, ids="internal")
    empty = ix.make_filter(np.zeros(n, bool), ids="internal")
    fo = np.array([-1, 0, 1, 2, 0])
    lab = np.array([0, 1, 2, 3, 1])
    variants = [dict(), dict(exact=True), dict(filter=f), dict(filter=f, exact=True), dict(filter=empty), dict(label=lab, exact=True),
                dict(filter=[f, f2, empty], filter_of=fo, exact=True)]
    if state != "added":        # (inherited: per-query filters would walk the graph of an index with a tail)
        variants += [dict(label=lab), dict(filter=[f, f2, empty], filter_of=fo)]
    Q = _queries(Q0, N, T, n0)
    Q[3, 1:] = np.float32(1e3)                                # garbage in the dead vectors of query 3
    for kw in variants:
        for weights, nv in ((WEIGHTS, NV), (None, None), (WEIGHTS[1], None)):
            got = ix.search_fused(Q, K, weights=weights, n_vectors=nv, candidates=C0, **kw)
            assert [g.shape for g in got] == [(N, K), (N, K), (N, K)] and [g.dtype for g in got] == [np.int64, np.float32, np.int32]
            want, cand = _expect(ix, Q, K, C0, weights, nv, **kw)
            assert same_bytes(got, want), (state, sorted(kw), weights is None)
            if "filter" in kw and kw["filter"] is empty:
                assert (got[0] == -1).all() and (got[1] == FMAX).all() and (got[2] == 0).all()
        if not kw:
            internal = got[0] if state != "input" else None
            if internal is not None:
                assert live[internal[internal >= 0]].all()
    assert same_bytes(ix.search_fused(Q, K), ix.search_fused(Q, K, candidates=40))          # candidates=None: max(32, 4 k)
    for x in (f, f2, empty):
        x.close()


def test_cosine_metric(cph):
    rng = np.random.default_rng(11)
    n, dim = 2500, 24
    X = (rng.standard_normal((n, dim)) * rng.uniform(0.2, 5.0, (n, 1))).astype(np.float32)
    ix = cph.CPIndex(dim, 4, metric="cosine")
    ix.build(X)
    ix.finalize()
    Q = _queries(rng.standard_normal((8, dim)).astype(np.float32), N, T, 9)
    Q[:-1] *= np.float32(3.0)                                 # (the length of a query vector does not matter)
    for kw in (dict(), dict(exact=True)):
        got = ix.search_fused(Q, K, weights=WEIGHTS, n_vectors=NV, candidates=C0, **kw)
        want, _ = _expect(ix, Q, K, C0, WEIGHTS, NV, cosine=True, **kw)
        assert same_bytes(got, want), sorted(kw)
        assert (got[0] >= 0).all()


@pytest.mark.parametrize("exact", (True, False))
def test_one_vector_weight_one_is_the_deduplicated_search(cph, gold, exact):
    ix, Q0 = _open(cph, gold)
    q = Q0[:6]
    C_, k = 40, 12
    was, ix.result_ids = ix.result_ids, "internal"
    ids, dist = ix.search_batch(q, C_, exact=exact)
    ix.result_ids = was
    got = ix.search_fused(q[:, None, :], k, candidates=C_, exact=exact)
    for i in range(len(q)):
        valid = ids[i][(ids[i] >= 0) & (ids[i] < ix.size)]
        _, first = np.unique(valid, return_index=True)
        head = np.sort(first)[:k]
        assert len(head) == k and np.array_equal(got[0][i], valid[head]) and got[1][i].tobytes() == dist[i][(ids[i] >= 0)][head].tobytes()
        assert (got[2][i] == 1).all()
    real = ids[0] >= 0                                        # the graph rows carry exact_l2's bytes
    assert ix.exact_l2(q[0], ids[0][real].astype(np.uint32)).tobytes() == dist[0][real].tobytes()


def test_weights_scaled_by_two_give_the_same_ids(cph, gold):
    ix, Q0 = _open(cph, gold)
    Q = _queries(Q0, N, T, 4)
    a = ix.search_fused(Q, K, weights=WEIGHTS, n_vectors=NV, candidates=C0)
    for scale in (2.0, 0.25):
        b = ix.search_fused(Q, K, weights=WEIGHTS * np.float32(scale), n_vectors=NV, candidates=C0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
        real = a[0] >= 0
        assert (b[1][real] == a[1][real] * np.float32(scale)).all()


# ---- the device variant, replicas -------------------------------------------------------------------------------------------------
def test_device_variant(cph, gold):
    import torch
    ix, Q0 = _open(cph, gold)
    n = ix.size
    dev = torch.device("cuda", 0)
    Q = _queries(Q0, N, T, 9)
    Qd = torch.from_numpy(Q).to(dev)
    ix.set_labels(np.arange(n) % 3, ids="internal")
    f = ix.make_filter(np.arange(n) % 3 != 0, ids="internal")
    fo = np.arange(N) % 2 - 1
    st1 = torch.cuda.Stream(dev)
    for kw in (dict(), dict(weights=WEIGHTS, n_vectors=NV), dict(weights=WEIGHTS, exact=True), dict(weights=WEIGHTS[0], filter=f),
               dict(n_vectors=NV, filter=[f], filter_of=fo), dict(weights=WEIGHTS, label=0)):
        want = ix.search_fused(Q, K, candidates=C0, **kw)
        got = ix.search_fused_device(Qd, K, candidates=C0, **kw)
        torch.cuda.synchronize()
        assert len(got) == 3 and same_bytes([t.cpu().numpy() for t in got], want), sorted(kw)
        # into given tensors that are longer than the batch: the rows past n stay as they were
        big = [torch.full((N + 3,) + w.shape[1:], -9, dtype=getattr(torch, w.dtype.name), device=dev) for w in want]
        out = [b[:N] for b in big]
        st1.wait_stream(torch.cuda.current_stream(dev))
        res = ix.search_fused_device(Qd, K, candidates=C0, out=out, stream=st1, **kw)
        st1.synchronize()
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, out))
        assert same_bytes([t.cpu().numpy() for t in res], want), sorted(kw)
        assert all((b[N:] == -9).all().item() for b in big)
    with pytest.raises(ValueError, match="three tensors"):
        ix.search_fused_device(Qd, K, candidates=C0, out=out[:2])
    # more calls than the handle has scratch sets, at growing shapes, host calls in between
    for C2 in (8, 64, 200, 16, 1024):
        want = ix.search_fused(Q, 8, weights=WEIGHTS, n_vectors=NV, candidates=C2)
        got = ix.search_fused_device(Qd, 8, weights=WEIGHTS, n_vectors=NV, candidates=C2)
        torch.cuda.synchronize()
        assert same_bytes([t.cpu().numpy() for t in got], want), C2
    ix.time_fused(True)
    ix.search_fused(Q, K, candidates=C0)
    assert ix.last_fused_us() > 0
    ix.time_fused(False)
    ix.synchronize()
    f.close()


def test_device_variant_returns_without_waiting(cph, gold):
    """The stream is kept busy by a spin kernel of about 0.15 s (calibrated on a short one); the call enqueues behind it and
    returns while it still runs."""
    import torch
    ix, Q0 = _open(cph, gold)
    dev = torch.device("cuda", 0)
    Q = _queries(Q0, N, T, 2)
    Qd = torch.from_numpy(Q).to(dev)
    want = ix.search_fused(Q, K, weights=WEIGHTS, n_vectors=NV, candidates=C0)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    for _ in range(4):                                        # every scratch set of the handle has served this shape once
        ix.search_fused_device(Qd, K, weights=WEIGHTS, n_vectors=NV, candidates=C0, stream=st)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record()
        torch.cuda._sleep(1_000_000)
        e1.record()
    e1.synchronize()
    cycles = int(1_000_000 * 150.0 / max(e0.elapsed_time(e1), 1e-3))
    with torch.cuda.stream(st):
        torch.cuda._sleep(cycles)
    got = ix.search_fused_device(Qd, K, weights=WEIGHTS, n_vectors=NV, candidates=C0, stream=st)
    pending = not st.query()
    st.synchronize()
    assert pending, "search_fused_device returned only after the stream had drained"
    assert same_bytes([t.cpu().numpy() for t in got], want)


def test_replicas_equal_one_device(cph, gold):
    name, bits = "g16", 1
    one, Q0 = _open(cph, gold, name, bits)
    m = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0])
    m.set_min_shard(1)
    m.load(fixture_path(name, bits))
    m.set_row_map(one.row_map())
    n = one.size
    mask = np.arange(n) % 4 != 1
    n_q = 9                                                   # nine queries over two replicas: shards of five and four
    Q = _queries(Q0, n_q, T, 2)
    rng = np.random.default_rng(3)
    W = rng.uniform(-1.0, 2.0, (n_q, T)).astype(np.float32)
    nv = rng.integers(1, T + 1, n_q).astype(np.int32)
    fo = np.arange(n_q) % 3 - 1
    for ix in (one, m):
        ix.set_labels(np.arange(n) % 5, ids="internal")
    for ids in ("internal", "input"):
        one.result_ids = m.result_ids = ids
        f1, fm = one.make_filter(mask, ids="internal"), m.make_filter(mask, ids="internal")
        e1, em = one.make_filter(~mask, ids="internal"), m.make_filter(~mask, ids="internal")
        for kw1, kwm in ((dict(), dict()), (dict(exact=True), dict(exact=True)), (dict(filter=f1), dict(filter=fm)),
                         (dict(filter=[f1, e1], filter_of=fo), dict(filter=[fm, em], filter_of=fo)), (dict(label=0), dict(label=0))):
            assert same_bytes(m.search_fused(Q, 6, weights=W, n_vectors=nv, candidates=40, **kwm),
                              one.search_fused(Q, 6, weights=W, n_vectors=nv, candidates=40, **kw1)), (ids, sorted(kw1))
        for x in (f1, fm, e1, em):
            x.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(cph, gold):
    import torch
    from cphnsw_mi355x import _lib
    ix, Q0 = _open(cph, gold)
    Q = _queries(Q0, N, T, 1)
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    out = [torch.full((N, K), -9, dtype=dt, device=dev) for dt in (torch.int64, torch.float32, torch.int32)]
    bad_w, bad_nv = WEIGHTS.copy(), NV.copy()
    bad_w[2, 1] = np.inf
    bad_nv[4] = T + 1
    for kw, what in ((dict(k=0), "1 <= k <= 1024"), (dict(k=1025, candidates=1024), "1 <= k <= 1024"), (dict(k=T * 3 + 1, candidates=3), "k <= vectors"),
                     (dict(candidates=0), r"candidates in \[1, 1024\]"), (dict(candidates=1025), r"candidates in \[1, 1024\]"),
                     (dict(weights=bad_w), "finite weights"), (dict(weights=WEIGHTS[:, :2]), r"weights of shape \(3,\) or \(5, 3\)"),
                     (dict(n_vectors=bad_nv), r"n_vectors in \[1, 3\]"), (dict(n_vectors=NV[:3]), "n_vectors as a 1D integer array of length 5")):
        for call in (lambda **a: ix.search_fused(Q, **a), lambda **a: ix.search_fused_device(Qd, out=out, **a)):
            with pytest.raises(ValueError, match="search_fused needs " + what):
                call(**dict(dict(k=K), **kw))
    big = np.zeros((2, 65, ix.dim), np.float32)
    with pytest.raises(ValueError, match="search_fused needs 1 <= vectors <= 64"):
        ix.search_fused(big, 3)
    with pytest.raises(ValueError, match=r"search_fused needs vectors \* candidates <= 8192"):
        ix.search_fused(big[:, :9], 3, candidates=1024)
    with pytest.raises(ValueError, match=r"\(n, vectors, dim\)"):
        ix.search_fused(Q[:, 0], 3)
    torch.cuda.synchronize()
    assert all((o == -9).all().item() for o in out)
    # the library's own refusals name the entry's limits too (the Python checks are in front of them), before any output
    L = _lib.lib()
    o = (np.full((N, K), -7, np.int64), np.full((N, K), -7, np.float32), np.full((N, K), -7, np.int32))
    po = [x.ctypes.data for x in o]
    w, nv = np.ascontiguousarray(WEIGHTS), NV

    def raw_call(T_=T, k_=K, C__=C0, w_=w, nv_=nv, n_=N):
        return L.cph_search_fused(ix._h, Q.ctypes.data, n_, T_, nv_.ctypes.data, w_.ctypes.data, k_, C__, None, 0, None, 0, *po)
    for bad, what in ((dict(T_=65), b"fused search supports 1 <= vectors <= 64"), (dict(C__=1025), b"fused search supports 1 <= candidates <= 1024"),
                      (dict(T_=9, C__=1024), b"fused search needs vectors * candidates <= 8192"), (dict(k_=0), b"fused search supports 1 <= k"),
                      (dict(k_=T * C0 + 1), b"fused search supports 1 <= k"), (dict(n_=2 ** 31), b"fused search needs n * vectors"),
                      (dict(w_=bad_w), b"weights[2][1] is not finite"), (dict(nv_=bad_nv), b"n_vectors[4] = 4 is outside [1, 3]")):
        assert raw_call(**bad) == _lib.INVALID_ARGUMENT, bad
        assert what in L.cph_last_error(), (bad, L.cph_last_error())
        assert all((x == -7).all() for x in o), bad
    assert raw_call() == _lib.OK and (o[0] >= 0).all()
    assert [g.shape for g in ix.search_fused(np.zeros((0, T, ix.dim), np.float32), 3)] == [(0, 3)] * 3       # an empty batch is no error
    with pytest.raises(ValueError, match="no timed fused search"):
        ix.last_fused_us()
    # the inner-product metric, through refuse_ip; a partitioned index
    ip = cph.CPIndex(ix.dim, 1, metric="ip")
    ip.build(np.random.default_rng(1).standard_normal((300, ix.dim)).astype(np.float32))
    ip.finalize()
    with pytest.raises(ValueError, match=r"fused search is not available under the inner-product \(ip\) metric"):
        ip.search_fused(Q, 3)
    with pytest.raises(ValueError, match=r"fused search is not available under the inner-product \(ip\) metric"):
        ip.search_fused_device(Qd, K, out=out)
    for x in o:
        x[:] = -7
    assert L.cph_search_fused(ip._h, Q.ctypes.data, N, T, nv.ctypes.data, w.ctypes.data, K, C0, None, 0, None, 0, *po) == _lib.INVALID_ARGUMENT
    assert b"fused search is not available" in L.cph_last_error() and all((x == -7).all() for x in o)
    p = cph.CPIndex(DATASETS["g16"]["dim"], 1, devices=[0, 0], partition=True)
    with pytest.raises(ValueError, match=r"partitioned index.*part\(i\)\.search_fused"):
        p.search_fused(Q, 3)
    with pytest.raises(ValueError, match=r"partitioned index.*part\(i\)\.search_fused"):
        p.search_fused_device(Qd, K, out=out)
    torch.cuda.synchronize()
    assert all((t == -9).all().item() for t in out)
