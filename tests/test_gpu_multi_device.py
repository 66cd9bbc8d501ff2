"""One index on several devices in one process (CPIndex(devices=[...]), cph_multi_*): the index replicated on every
listed device, queries split into contiguous shards, each shard answered by the single-device search on its replica.
On a one-GPU box the replicas share device 0 (duplicates are allowed), which exercises everything but the peer copy
between two GPUs: every split result must equal the reference's goldens, or a single-device index, byte for byte."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from golden_util import DATASETS, KS, fixture_path

pytestmark = pytest.mark.gpu

CASES = [(n, b, v) for n, s in DATASETS.items() for b in s["bits"] for v in s["variants"]]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _multi(cph, name, bits, variant="plain", devices=(0, 0)):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits, devices=list(devices))
    ix.set_min_shard(1)
    ix.load(fixture_path(name, bits, variant))
    return ix


def _single(cph, name, bits, variant="plain"):
    ix = cph.CPIndex(DATASETS[name]["dim"], bits, device=0)
    ix.load(fixture_path(name, bits, variant))
    return ix


@pytest.mark.parametrize("replicas", [2, 3])
@pytest.mark.parametrize("name,bits,variant", CASES)
def test_split_batches_equal_goldens(cph, gold, name, bits, variant, replicas):
    """nq = 1, 7, 24 and Q tiled 5x (120 queries: the general path on every shard), every k, then again with 8 slots of
    capacity 64 (the overflow re-run on every replica)."""
    ix = _multi(cph, name, bits, variant, devices=[0] * replicas)
    assert ix.devices == [0] * replicas
    Q = gold[f"Q/{name}"]
    for params in ((0, 0), (8, 64)):
        ix.set_search_params(slots=params[0], beam_capacity=params[1])
        for k in KS:
            gi, gd = gold[f"S/{name}/b{bits}/{variant}/k{k}/ids"], gold[f"S/{name}/b{bits}/{variant}/k{k}/d"]
            for nq in (1, 7, 24):
                ids, d = ix.search_batch(Q[:nq], k)
                assert np.array_equal(ids, gi[:nq]), (name, bits, variant, k, nq, params)
                assert _beq(d, gd[:nq]), (name, bits, variant, k, nq, params)
            ids, d = ix.search_batch(np.tile(Q, (5, 1)), k)
            assert np.array_equal(ids, np.tile(gi, (5, 1))), (name, bits, variant, k, "tiled", params)
            assert _beq(d, np.tile(gd, (5, 1))), (name, bits, variant, k, "tiled", params)


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g128", 1), ("g1024", 2), ("g16", 2)])
def test_expansions_and_stats_equal_single_device(cph, gold, name, bits):
    Q = np.tile(gold[f"Q/{name}"], (5, 1))
    m, s = _multi(cph, name, bits), _single(cph, name, bits)
    mi, md = m.search_batch(Q, 10)
    si, sd = s.search_batch(Q, 10)
    assert np.array_equal(mi, si) and _beq(md, sd)
    me, se = m.last_query_expansions(len(Q)), s.last_query_expansions(len(Q))
    assert np.array_equal(me, se)
    ms, ss = m.last_search_stats(), s.last_search_stats()
    assert ms["expansions"] == ss["expansions"] == int(se.sum())
    assert ms["exact_l2"] == ss["exact_l2"]
    with pytest.raises(ValueError):
        m.last_query_expansions(len(Q) - 1)


@pytest.mark.parametrize("name,bits,variant", [(n, b, v) for (n, b, v) in CASES if v in ("plain", "shortcount")])
def test_filtered_split_batches(cph, gold, name, bits, variant):
    m, s = _multi(cph, name, bits, variant), _single(cph, name, bits, variant)
    Q = gold[f"Q/{name}"]
    ones = m.make_filter(np.ones(m.size, bool))
    for k in (1, 10, 100):
        ids, d = m.search_batch(Q, k, filter=ones)
        assert np.array_equal(ids, gold[f"S/{name}/b{bits}/{variant}/k{k}/ids"]), (name, bits, variant, k)
        assert _beq(d, gold[f"S/{name}/b{bits}/{variant}/k{k}/d"]), (name, bits, variant, k)
    mask = np.random.default_rng(bits * 31 + len(name)).random(m.size) < 0.1
    mf, sf = m.make_filter(mask), s.make_filter(mask)
    Qt = np.tile(Q, (3, 1))
    for k in (1, 10, 100):
        mi, md = m.search_batch(Qt, k, filter=mf)
        si, sd = s.search_batch(Qt, k, filter=sf)
        assert np.array_equal(mi, si) and _beq(md, sd), (name, bits, variant, k)
        assert np.array_equal(m.last_query_expansions(len(Qt)), s.last_query_expansions(len(Qt)))
    mi, md = m.search(Q[3], 10, filter=mask)
    si, sd = s.search(Q[3], 10, filter=mask)
    assert np.array_equal(mi, si) and _beq(md, sd)
    with pytest.raises(ValueError):
        m.make_filter(np.ones(m.size + 1, bool))
    with pytest.raises(ValueError):
        m.search_batch(Q, 10, filter=sf)            # one bitmap, two replicas


def _build_case(cph, tmp_path, n, dim, bits, nq, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = rng.standard_normal((nq, dim)).astype(np.float32)
    m = cph.CPIndex(dim, bits, devices=[0, 0])
    m.set_min_shard(1)
    m.build(X)
    assert not m.is_finalized and m.size == n
    with pytest.raises(RuntimeError, match="invalid entry point"):
        m.search_batch(Q[:4], 10)
    m.finalize()
    assert m.is_finalized and m.size == n
    p = str(tmp_path / f"built_{dim}_{bits}.idx")
    m.save(p)
    s = cph.CPIndex(dim, bits, device=0)
    s.load(p)
    return m, s, Q


@pytest.mark.parametrize("n,dim,bits", [(20000, 128, 4), (4000, 1000, 2)])
def test_built_index_replicated(cph, tmp_path, n, dim, bits):
    """finalize() builds on replica 0 and copies to replica 1: both halves of a split batch equal a single-device index
    that loads the multi handle's save file (4-bit at D = 128: the resident nibble layout)."""
    m, s, Q = _build_case(cph, tmp_path, n, dim, bits, 2000, n + dim)
    for k in (10, 100):
        mi, md = m.search_batch(Q, k)
        si, sd = s.search_batch(Q, k)
        assert np.array_equal(mi, si) and _beq(md, sd), k
        assert np.array_equal(m.last_query_expansions(len(Q)), s.last_query_expansions(len(Q)))
    # a device-resident batch on either replica
    import torch
    tq = torch.from_numpy(Q[:300]).to("cuda:0")
    si, sd = s.search_batch(Q[:300], 10)
    for _ in range(2):
        ti, td = m.search_batch_device(tq, 10)
        torch.cuda.synchronize()
        assert np.array_equal(ti.cpu().numpy(), si) and _beq(td.cpu().numpy(), sd)
    # the vectors come from replica 0's host arrays
    assert np.array_equal(m.get_vectors(0, 50), s.get_vectors(0, 50))


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g1024", 2), ("g16", 1), ("sift96", 4)])
def test_save_and_native_round_trip(cph, gold, tmp_path, name, bits):
    m, s = _multi(cph, name, bits), _single(cph, name, bits)
    pm, ps = tmp_path / "multi.idx", tmp_path / "single.idx"
    m.save(pm)
    s.save(ps)
    assert pm.read_bytes() == ps.read_bytes()
    nm, ns = tmp_path / "multi.cphn", tmp_path / "single.cphn"
    m.save_native(nm)
    s.save_native(ns)
    assert nm.read_bytes() == ns.read_bytes()
    Q = np.tile(gold[f"Q/{name}"], (4, 1))
    ref_i, ref_d = m.search_batch(Q, 20)
    m2 = cph.CPIndex(DATASETS[name]["dim"], bits, devices=[0, 0, 0])
    m2.set_min_shard(1)
    m2.load_native(str(nm))
    i2, d2 = m2.search_batch(Q, 20)
    assert np.array_equal(i2, ref_i) and _beq(d2, ref_d)


def test_concurrent_single_queries(cph, gold):
    """16 threads x 50 search() calls on two replicas: each answer equals the single-device search of the same query."""
    m, s = _multi(cph, "g128", 4), _single(cph, "g128", 4)
    Q = gold["Q/g128"]
    want = [s.search(q, 10) for q in Q]
    errors = []

    def worker(t):
        try:
            for i in range(50):
                j = (t * 7 + i) % len(Q)
                ids, d = m.search(Q[j], 10)
                if not (np.array_equal(ids, want[j][0]) and _beq(d, want[j][1])):
                    errors.append((t, i, j))
        except Exception as e:                      # noqa: BLE001
            errors.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors[:5]


def test_concurrent_batches(cph, gold):
    """Batches from several threads at once share the replicas' workers."""
    m = _multi(cph, "g128", 2)
    Q = np.tile(gold["Q/g128"], (5, 1))
    gi = np.tile(gold["S/g128/b2/plain/k10/ids"], (5, 1))
    errors = []

    def worker():
        for _ in range(10):
            ids, _ = m.search_batch(Q, 10)
            if not np.array_equal(ids, gi):
                errors.append(1)

    th = [threading.Thread(target=worker) for _ in range(6)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors


def test_search_batch_device_equals_search_batch(cph, gold):
    import torch
    m = _multi(cph, "g128", 4)
    Q = np.tile(gold["Q/g128"], (5, 1))
    want_i, want_d = m.search_batch(Q, 10)
    tq = torch.from_numpy(Q).to("cuda:0")
    for _ in range(3):                                      # alternates between the two replicas on device 0
        ids, d = m.search_batch_device(tq, 10)
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy(), want_i) and _beq(d.cpu().numpy(), want_d)
    f = m.make_filter(np.ones(m.size, bool))
    ids, d = m.search_batch_device(tq, 10, filter=f)
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy(), want_i) and _beq(d.cpu().numpy(), want_d)
    with pytest.raises(ValueError):
        m.search_batch_device(torch.from_numpy(Q), 10)      # host tensor: no replica there


def test_errors_and_refusals(cph, gold):
    import torch
    from cphnsw_mi355x import _lib
    with pytest.raises(ValueError):
        cph.CPIndex(128, 4, devices=[])
    with pytest.raises(ValueError):
        cph.CPIndex(128, 4, devices=[0, torch.cuda.device_count()])
    with pytest.raises(ValueError):
        cph.CPIndex(128, 4, device=0, devices=[0])
    with pytest.raises(ValueError):
        cph.CPIndex(128, 4, devices=[0] * 17)
    m = cph.CPIndex(128, 4, devices=[0, 0])
    assert not m.is_finalized
    with pytest.raises(RuntimeError, match="Search failed: invalid entry point after finalize."):
        m.search_batch(gold["Q/g128"], 10)
    with pytest.raises(RuntimeError, match="Search failed: invalid entry point after finalize."):
        m.search(gold["Q/g128"][0], 10)
    m.set_min_shard(1)
    with pytest.raises(ValueError):
        m.set_min_shard(0)
    m.load(fixture_path("g128", 4))
    L = _lib.lib()
    n = C.c_uint32(0)
    assert L.cph_multi_num_replicas(m._m, C.byref(n)) == _lib.OK and n.value == 2
    # borrowed replicas refuse the lifecycle calls; replica 1 keeps no host arrays
    for r in m._reps:
        assert L.cph_load(r, fixture_path("g128", 4).encode()) == _lib.INVALID_ARGUMENT
        assert b"replica" in L.cph_last_error()
        assert L.cph_load_native(r, b"x") == _lib.INVALID_ARGUMENT
        assert L.cph_finalize(r) == _lib.INVALID_ARGUMENT
        assert L.cph_destroy(r) == _lib.INVALID_ARGUMENT
    out = np.empty(128, np.float32)
    assert L.cph_get_vectors(m._reps[1], 0, 1, out.ctypes.data) == _lib.INVALID_ARGUMENT
    assert L.cph_get_vectors(m._reps[0], 0, 1, out.ctypes.data) == _lib.OK
    bad = C.c_void_p()
    assert L.cph_multi_replica(m._m, 2, C.byref(bad)) == _lib.INVALID_ARGUMENT
    # a file that fails to parse leaves every replica with the previous index
    with pytest.raises(RuntimeError):
        m.load("/nonexistent/index.idx")
    ids, _ = m.search_batch(gold["Q/g128"], 10)
    assert np.array_equal(ids, gold["S/g128/b4/plain/k10/ids"])
    # a borrowed replica's own batch still works (hooks, device batches)
    ep = m.entry_point(gold["Q/g128"][0])
    assert ep == _single(cph, "g128", 4).entry_point(gold["Q/g128"][0])


@pytest.mark.skipif("not __import__('torch').cuda.device_count() >= 2", reason="needs two or more GPUs")
def test_several_gpus_equal_single_device(cph, tmp_path):
    """C2 shape (1M x 128, 4-bit, k = 10, 10k queries) on up to 8 GPUs: byte-identical to one device."""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.CONFIGS["c2"]
    n, nq = cfg["n"], 10000
    X = bench.make_base(cfg, n)
    Q = bench.make_queries(cfg, n, nq)
    s = cph.CPIndex(128, 4, device=0)
    s.build(X)
    s.finalize()
    p = str(tmp_path / "c2.idx")
    s.save(p)
    m = cph.CPIndex(128, 4, devices=list(range(min(torch.cuda.device_count(), 8))))
    m.load(p)
    mi, md = m.search_batch(Q, 10)
    si, sd = s.search_batch(Q, 10)
    assert np.array_equal(mi, si) and _beq(md, sd)
