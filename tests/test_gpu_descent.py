"""GPU tests of the upper-layer descent of the query encoder (csrc/device_encode.h) against the oracle.

Each index is built here with this repository's builder and saved; the oracle loads the saved file.  Per index, 256
queries: `CPIndex.entry_point(q)` equals `Oracle().load(path).entry_point(q)` (the layer-0 entry the descent ends at),
and `search_batch(Q, 10)` equals the oracle's ids and distance bytes, which pins the entry distance as well: it is the
launch-order key and the first expansion's distance.

What the cases reach in the kernel (asserted from the saved file, `upper_layers`):
  * dups128b4   D = 128, every row four times: equal distances inside one neighbour list, so "first stored position
                on a tie" decides.  Two layers have more than 16 nodes (vertex -> row map, the paired one-pass hop with
                the next hop's row taken from nbr_info), the top layer has at most 16 (binary search over its nodes).
  * d96b2       dim 96 padded to D = 128, 2-bit codes: the paired hop on a padded query.
  * d960b4      D = 1024: the paired hop's loop over 64-element parts with carried accumulators.
  * d48b4       D = 64: not a multiple of 128, so mapped layers take the eight-lanes-per-neighbour loop.
The builder's upper layers never hold more than 32 neighbours per vertex (asserted below for every case).  The hop for
33..62 neighbours of a mapped layer, the unmapped fallback and the other dimensions are reached on hand-made layers:
tests/test_gpu_descent_shapes.py.
"""
import ctypes as C
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ = 256

# name: (dim, bits, n, kind)
CASES = {
    "dups128b4": (128, 4, 20_000, "dups"),
    "d96b2": (96, 2, 20_000, "gauss"),
    "d960b4": (960, 4, 4_000, "gauss"),
    "d48b4": (48, 4, 20_000, "gauss"),
}


def make_data(dim, n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "dups":
        X = np.repeat(rng.standard_normal((n // 4, dim)).astype(np.float32), 4, axis=0)[rng.permutation(n)]
    else:
        X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = (X[rng.integers(0, n, NQ)] + 0.3 * rng.standard_normal((NQ, dim))).astype(np.float32)
    return np.ascontiguousarray(X), Q


def upper_layers(path, vertex_bytes):
    """[(nodes, max degree)] per upper layer of a saved index (the layout HostIndex::save writes)."""
    with open(path, "rb") as f:
        hdr = f.read(68)
        D, dim = struct.unpack_from("<I", hdr, 12)[0], struct.unpack_from("<I", hdr, 24)[0]
        n = struct.unpack_from("<Q", hdr, 28)[0]
        f.seek(68 + 248 + 72 + dim * 4 + n * 4 + n * 4 + n * D * 4 + n * vertex_bytes)
        (nl,) = struct.unpack("<I", f.read(4))
        out = []
        for _ in range(nl):
            (sz,) = struct.unpack("<I", f.read(4))
            deg = 0
            for _ in range(sz):
                _, cnt = struct.unpack("<II", f.read(8))
                f.seek(cnt * 4, os.SEEK_CUR)
                deg = max(deg, cnt)
            out.append((sz, deg))
    return out


_BUILT = {}


def _case(name, tmp_path_factory, oracle):
    """(name, index, path, oracle index, queries, oracle entry points, oracle search): built once per session."""
    import cphnsw_mi355x
    if name not in _BUILT:
        dim, bits, n, kind = CASES[name]
        X, Q = make_data(dim, n, kind, 7000 + dim)
        ix = cphnsw_mi355x.CPIndex(dim, bits, device=0)
        ix.build(X)
        ix.finalize()
        path = str(tmp_path_factory.mktemp("descent") / f"{name}.idx")
        ix.save(path)
        oi = oracle.load(path)
        want_ep = np.array([oi.entry_point(q) for q in Q], np.int64)
        want_ids, want_d, _ = oi.search_batch(Q, 10)
        _BUILT[name] = (name, ix, path, oi, Q, want_ep, want_ids, want_d)
    return _BUILT[name]


@pytest.fixture(params=list(CASES))
def built(request, tmp_path_factory, oracle):
    return _case(request.param, tmp_path_factory, oracle)


def test_layers_are_the_ones_the_cases_are_for(built):
    name, _, path, oi, *_ = built
    layers = upper_layers(path, oi.vertex_bytes)[:oi.max_level]
    print(name, "upper layers (nodes, max degree):", layers)
    assert layers and all(deg <= 32 for _, deg in layers), layers
    mapped = [sz for sz, _ in layers if sz > 16]
    assert mapped, layers                                   # a layer with a vertex -> row map
    if name == "dups128b4":
        assert len(mapped) >= 2 and layers[-1][0] <= 16, layers
        assert layers[0][0] >= 200, layers


def test_entry_points_equal_the_oracles(built):
    name, ix, _, _, Q, want_ep, _, _ = built
    got = np.array([ix.entry_point(q) for q in Q], np.int64)
    assert np.array_equal(got, want_ep), (name, np.flatnonzero(got != want_ep)[:8])


def test_search_equals_the_oracles(built):
    name, ix, _, _, Q, _, want_ids, want_d = built
    ids, d = ix.search_batch(Q, 10)
    assert np.array_equal(ids, want_ids), name
    assert d.tobytes() == want_d.tobytes(), name


def test_replica_descends_like_the_first(oracle, tmp_path_factory):
    """CPIndex(devices=[0, 0]) loaded from the duplicated-rows file: replica 1 has its own copies of the upper layers, the
    row maps and nbr_info behind rebased pointers.  Its entry points (asked of the replica itself) and a batch split
    over both replicas equal the oracle's."""
    import cphnsw_mi355x
    from cphnsw_mi355x import _lib
    name, _, path, _, Q, want_ep, want_ids, want_d = _case("dups128b4", tmp_path_factory, oracle)
    dim, bits, _, _ = CASES[name]
    m = cphnsw_mi355x.CPIndex(dim, bits, devices=[0, 0])
    m.set_min_shard(1)
    m.load(path)
    got = np.array([m.entry_point(q) for q in Q], np.int64)
    assert np.array_equal(got, want_ep)
    rep1 = m._reps[1]
    ep = C.c_uint32(0)
    got1 = np.empty(NQ, np.int64)
    for i, q in enumerate(Q):
        q = np.ascontiguousarray(q, np.float32)
        _lib.check(_lib.lib().cph_entry_point(rep1, q.ctypes.data, C.byref(ep)))
        got1[i] = ep.value
    assert np.array_equal(got1, want_ep)
    ids, d = m.search_batch(Q, 10)
    assert np.array_equal(ids, want_ids) and d.tobytes() == want_d.tobytes()
