"""Filtered search on the GPU: the HIP kernels' filtered instantiations against the reference's goldens (all-ones filter)
and against the model of the filtered search (tests/filtered_model/filtered_search.cpp: the oracle's search with the
result-heap push gated), ids, distance bytes and per-query expansions, on every path a batch can take: the small-batch
launch, the general path with a queue, and the capacity-overflow re-run."""
import gc
import zlib

import numpy as np
import pytest

from filtered_model_lib import ModelIndex
from golden_util import DATASETS, KS, fixture_path

pytestmark = pytest.mark.gpu

CASES = [(n, b, v) for n, s in DATASETS.items() for b in s["bits"] for v in s["variants"]]
FMAX = np.finfo(np.float32).max
# search parameters of the three paths: default (24 queries: one launch on full-capacity slots), a queue on 8 slots,
# and 8 slots of capacity 64 (queries overflow and are answered by the re-run launch)
PATHS = {"default": (0, 0), "queue": (8, 0), "overflow": (8, 64)}


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _load(cph, name, bits, variant="plain"):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits)
    ix.load(fixture_path(name, bits, variant))
    return ix


def _filters(n, seed):
    rng = np.random.default_rng(seed)
    out = {"p0.5": rng.random(n) < 0.5, "p0.1": rng.random(n) < 0.1}
    out["even"] = np.arange(n) % 2 == 0
    r = np.zeros(n, bool)
    r[n // 4:n // 4 + max(1, n // 5)] = True
    out["range"] = r
    one = np.zeros(n, bool)
    one[7] = True
    out["single"] = one
    out["empty"] = np.zeros(n, bool)
    return out


@pytest.mark.parametrize("name,bits,variant", CASES)
def test_all_ones_filter_equals_goldens(cph, gold, name, bits, variant):
    """Every id allowed: the filtered instantiations return exactly the unfiltered search -- the reference's goldens."""
    ix = _load(cph, name, bits, variant)
    Q = gold[f"Q/{name}"]
    f = ix.make_filter(np.ones(ix.size, bool))
    for k in KS:
        ids, d = ix.search_batch(Q, k, filter=f)
        assert np.array_equal(ids, gold[f"S/{name}/b{bits}/{variant}/k{k}/ids"]), (name, bits, variant, k)
        assert _beq(d, gold[f"S/{name}/b{bits}/{variant}/k{k}/d"]), (name, bits, variant, k)
    ix.set_search_params(slots=8, beam_capacity=0)
    for k in (10, 100):
        ids, d = ix.search_batch(Q, k, filter=f)
        assert np.array_equal(ids, gold[f"S/{name}/b{bits}/{variant}/k{k}/ids"]), (name, bits, variant, k, "general path")
        assert _beq(d, gold[f"S/{name}/b{bits}/{variant}/k{k}/d"]), (name, bits, variant, k, "general path")
        assert ix.last_search_stats()["slots"] == 8


@pytest.mark.parametrize("name,bits,variant", CASES)
def test_filtered_search_matches_model(cph, gold, name, bits, variant):
    ix = _load(cph, name, bits, variant)
    mi = ModelIndex(fixture_path(name, bits, variant))
    Q = gold[f"Q/{name}"]
    nq = len(Q)
    for fname, mask in _filters(ix.size, zlib.crc32(f"{name}{bits}{variant}".encode())).items():
        f = ix.make_filter(mask)
        for k in (1, 10, 100):
            mids, md, mcnt, mctr = mi.search_batch(Q, k, mask, nthreads=16)
            for path, (slots, cap) in PATHS.items():
                ix.set_search_params(slots=slots, beam_capacity=cap)
                ids, d = ix.search_batch(Q, k, filter=f)
                where = (name, bits, variant, fname, k, path)
                assert np.array_equal(ids, mids), where
                assert _beq(d, md), where
                st = ix.last_search_stats()
                work = ix.last_query_expansions(nq).astype(np.uint64)
                if fname == "empty":
                    # nothing can enter a result heap: no launch, no expansion (the model walks the whole component)
                    assert (ids == -1).all() and (d == FMAX).all() and (mcnt == 0).all(), where
                    assert st["expansions"] == 0 and (work == 0).all(), where
                    continue
                assert np.array_equal(work, mctr[:, 0]), where
                if path == "overflow":
                    # a beam the model grew past 64 entries has overflowed a slot of capacity 64
                    assert (st["rerun_queries"] > 0) or not (mctr[:, 5] > 64).any(), where
                    assert st["expansions"] >= int(mctr[:, 0].sum()), where      # (+ the overflowed first passes)
                else:
                    assert st["rerun_queries"] == 0, where
                    assert st["expansions"] == int(mctr[:, 0].sum()), where
                    assert st["new_neighbours"] == int(mctr[:, 3].sum()), where
                    assert st["beam_pushes"] == int(mctr[:, 4].sum()) - nq, where   # (the model counts the entry's push)


def test_filtered_search_at_scale(cph, tmp_path):
    """A GPU-built 70,000-vertex 4-bit index (above the default per-slot capacity of 65,536, so that the batch path keeps
    its re-run launch and small batches take the full-capacity slots directly) with a 1 % filter: 200 queries on the
    general path, on small slots that overflow, and a batch small enough for the full-capacity slots -- ids, distance
    bytes and per-query expansions equal the model's."""
    rng = np.random.default_rng(4242)
    n, dim, k = 70000, 128, 10
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((200, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 4)
    ix.build(X)
    ix.finalize()
    p = str(tmp_path / "flt.idx")
    ix.save(p)
    mask = rng.random(n) < 0.01
    mi = ModelIndex(p)
    mids, md, _, mctr = mi.search_batch(Q, k, mask, nthreads=16)
    f = ix.make_filter(mask)

    ids, d = ix.search_batch(Q, k, filter=f)
    st = ix.last_search_stats()
    assert np.array_equal(ids, mids) and _beq(d, md)
    assert np.array_equal(ix.last_query_expansions(len(Q)).astype(np.uint64), mctr[:, 0])
    print("1 % filter, general path:", st)

    ix.set_search_params(slots=64, beam_capacity=1024)
    ids, d = ix.search_batch(Q, k, filter=f)
    st = ix.last_search_stats()
    assert st["rerun_queries"] > 0, st
    assert np.array_equal(ids, mids) and _beq(d, md)
    assert np.array_equal(ix.last_query_expansions(len(Q)).astype(np.uint64), mctr[:, 0])
    print("1 % filter, overflow:", st)

    ix.set_search_params(slots=0, beam_capacity=0)
    ids, d = ix.search_batch(Q[:16], k, filter=f)
    st = ix.last_search_stats()
    assert st["slots"] == 16 and st["capacity"] == n + 1, st          # the small-batch launch
    assert np.array_equal(ids, mids[:16]) and _beq(d, md[:16])
    assert np.array_equal(ix.last_query_expansions(16).astype(np.uint64), mctr[:16, 0])


def test_single_query_and_device_batch_with_filter(cph, gold):
    import torch
    ix = _load(cph, "g128", 4)
    Q = gold["Q/g128"]
    rng = np.random.default_rng(5)
    mask = rng.random(ix.size) < 0.2
    f = ix.make_filter(mask)
    for k in (0, 1, 10):
        ids, d = ix.search_batch(Q, max(k, 1), filter=f)
        for i in range(len(Q)):
            si, sd = ix.search(Q[i], k, filter=f)
            m = int((ids[i] >= 0).sum())
            assert np.array_equal(si, ids[i, :m]) and _beq(sd, d[i, :m]), (k, i)
    # ids or a mask are accepted where a filter is
    ids10, d10 = ix.search_batch(Q, 10, filter=f)
    for alt in (mask, np.flatnonzero(mask), np.flatnonzero(mask).tolist()):
        a_ids, a_d = ix.search_batch(Q, 10, filter=alt)
        assert np.array_equal(a_ids, ids10) and _beq(a_d, d10)
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    for k in (10, 100):
        ids, d = ix.search_batch(Q, k, filter=f)
        did, dd = ix.search_batch_device(Qd, k, filter=f)
        torch.cuda.synchronize()
        assert np.array_equal(did.cpu().numpy(), ids) and _beq(dd.cpu().numpy(), d), k
    # the empty filter on the device path: padding written by copy commands
    did, dd = ix.search_batch_device(Qd, 10, filter=np.zeros(ix.size, bool))
    torch.cuda.synchronize()
    assert (did.cpu().numpy() == -1).all() and (dd.cpu().numpy() == FMAX).all()
    # without a filter nothing changed
    ids, d = ix.search_batch(Q, 10)
    assert np.array_equal(ids, gold["S/g128/b4/plain/k10/ids"]) and _beq(d, gold["S/g128/b4/plain/k10/d"])


def test_filter_errors_and_lifetime(cph, gold, tmp_path):
    import torch
    ix = _load(cph, "g128", 4)
    other = _load(cph, "g16", 2)
    Q = gold["Q/g128"]
    n = ix.size
    with pytest.raises(ValueError):
        ix.search_batch(Q, 10, filter=other.make_filter(np.ones(other.size, bool)))    # another index size
    with pytest.raises(ValueError):
        ix.make_filter(np.ones(n + 1, bool))
    with pytest.raises(ValueError):
        ix.make_filter(np.ones(n - 1, bool))
    with pytest.raises(ValueError):
        ix.make_filter([0, 5, n])
    with pytest.raises(ValueError):
        ix.make_filter([-1])
    with pytest.raises(ValueError):
        ix.search_batch(Q, 10, filter=np.ones(n - 3, bool))
    f = ix.make_filter(np.arange(0, n, 3))
    f.close()
    with pytest.raises(ValueError):
        ix.search_batch(Q, 10, filter=f)
    # a filter made for one index serves another of the same size; one loaded with another file is refused
    twin = _load(cph, "g128", 4, "gamma")
    g = twin.make_filter(np.arange(0, n, 3))
    want_ids, want_d = ix.search_batch(Q, 100, filter=g)
    small = cph.CPIndex(128, 4)
    small.build(np.random.default_rng(3).standard_normal((300, 128)).astype(np.float32))
    small.finalize()
    small.save(str(tmp_path / "small.idx"))
    twin.load(str(tmp_path / "small.idx"))
    assert twin.size == 300
    with pytest.raises(ValueError):
        twin.search_batch(Q, 10, filter=g)
    # destroyed or collected while a device batch that reads it is in flight: the batch still completes correctly
    dev = torch.device("cuda", 0)
    Qd = torch.from_numpy(Q).to(dev)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    h = ix.make_filter(np.arange(0, n, 3))
    ids1, d1 = ix.search_batch_device(Qd, 100, stream=st, filter=h)
    h.close()
    h2 = ix.make_filter(np.arange(0, n, 3))
    ids2, d2 = ix.search_batch_device(Qd, 100, stream=st, filter=h2)
    del h2
    gc.collect()
    ix.synchronize()
    for ids, d in ((ids1, d1), (ids2, d2)):
        assert np.array_equal(ids.cpu().numpy(), want_ids) and _beq(d.cpu().numpy(), want_d)
