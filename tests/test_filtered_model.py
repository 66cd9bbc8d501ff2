"""The model of the filtered search (tests/filtered_model/filtered_search.cpp) on the CPU, and the filter's C-ABI and bit
packing.  The model is what tests/test_gpu_filtered.py holds the GPU to, so it is pinned here first: with every id
allowed it IS the oracle's search, byte for byte and counter for counter; with a filter it returns allowed ids only."""
import os
import re
import zlib

import numpy as np
import pytest

from filtered_model_lib import ModelIndex, compiler, pack_words
from golden_util import DATASETS, KS, fixture_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, b, v) for n, s in DATASETS.items() for b in s["bits"] for v in s["variants"]]
NEW_SYMBOLS = ("cph_filter_create", "cph_filter_destroy", "cph_search_batch_filtered", "cph_search_batch_device_filtered")

needs_gxx = pytest.mark.skipif(compiler() is None, reason="g++ not available")


def _beq(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@needs_gxx
@pytest.mark.parametrize("name,bits,variant", CASES)
def test_all_ones_filter_is_the_oracle(oracle, gold, name, bits, variant):
    p = fixture_path(name, bits, variant)
    mi = ModelIndex(p)
    oi = oracle.load(p)
    Q = gold[f"Q/{name}"]
    ones = np.ones(mi.n, bool)
    for k in KS:
        oids, od, ocnt, octr = oi.search_batch(Q, k, counters=True)
        ids, d, cnt, ctr = mi.search_batch(Q, k, ones)
        assert np.array_equal(ids, oids) and _beq(d, od), (name, bits, variant, k)
        assert np.array_equal(cnt, ocnt) and np.array_equal(ctr, octr), (name, bits, variant, k)
        # and the goldens of the reference itself
        assert np.array_equal(ids, gold[f"S/{name}/b{bits}/{variant}/k{k}/ids"]), (name, bits, variant, k)


@needs_gxx
@pytest.mark.parametrize("name,bits,variant", CASES)
def test_random_filters_return_allowed_ids_only(gold, name, bits, variant):
    p = fixture_path(name, bits, variant)
    mi = ModelIndex(p)
    Q = gold[f"Q/{name}"]
    rng = np.random.default_rng(zlib.crc32(f"{name}{bits}{variant}".encode()))
    for prob in (0.5, 0.1):
        mask = rng.random(mi.n) < prob
        for k in (1, 10, 100):
            ids, d, cnt, ctr = mi.search_batch(Q, k, mask)
            for i in range(len(Q)):
                row = ids[i, :cnt[i]]
                assert (row >= 0).all() and mask[row].all(), (name, bits, variant, prob, k, i)
                assert (ids[i, cnt[i]:] == -1).all() and (d[i, cnt[i]:] == np.finfo(np.float32).max).all()
                assert np.all(np.diff(d[i, :cnt[i]]) >= 0)
                # (an id can be in the result heap twice -- reranked as a neighbour, pushed again when it is popped --
                # as in the reference)
                assert cnt[i] <= k and len(np.unique(row)) <= int(mask.sum())


@needs_gxx
@pytest.mark.parametrize("name,bits", [("g128", 4), ("g16", 2), ("g1024", 2)])
def test_empty_filter_gives_an_empty_result(gold, name, bits):
    mi = ModelIndex(fixture_path(name, bits))
    Q = gold[f"Q/{name}"]
    ids, d, cnt, _ = mi.search_batch(Q, 10, np.zeros(mi.n, bool))
    assert (cnt == 0).all() and (ids == -1).all() and (d == np.finfo(np.float32).max).all()


@needs_gxx
def test_single_allowed_id(gold):
    """With one allowed id the warm-up never ends: every query walks its whole connected component and returns that id
    -- once or twice (reranked as a neighbour, pushed again when popped, as the reference does) -- if the component holds
    it, nothing otherwise (g128's vertex 399 is not reachable from the entry)."""
    mi = ModelIndex(fixture_path("g128", 4))
    Q = gold["Q/g128"]
    for vid, found in ((0, True), (7, True), (399, False)):
        mask = np.zeros(mi.n, bool)
        mask[vid] = True
        ids, _, cnt, ctr = mi.search_batch(Q, 10, mask)
        assert ((cnt >= 1) if found else (cnt == 0)).all(), vid
        assert all(set(ids[i, :cnt[i]].tolist()) <= {vid} for i in range(len(Q)))
        assert len(set(ctr[:, 0].tolist())) == 1          # the same component, expanded whole, by every query


def _declared_symbols():
    txt = open(os.path.join(ROOT, "include", "cphnsw_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(cph_[a-z0-9_]+)\s*\(", txt))


def test_filter_symbols_are_declared_and_exported():
    from cphnsw_mi355x import _lib
    declared = _declared_symbols()
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} not declared in include/cphnsw_mi355x.h"
        assert s in _lib.SYMBOLS, f"{s} missing from the ctypes table"
        assert hasattr(L, s), f"{s} not exported by the library"


@pytest.mark.parametrize("n", [1, 5, 31, 32, 33, 63, 64, 65, 400, 1001])
def test_bit_packing_matches_numpy_little_endian(n):
    from cphnsw_mi355x.index import pack_allowed_bits
    rng = np.random.default_rng(n)
    for prob in (0.0, 0.3, 1.0):
        mask = rng.random(n) < prob
        w = pack_allowed_bits(mask)
        assert w.dtype == np.uint32 and w.shape == ((n + 31) // 32,)
        assert np.array_equal(w, pack_words(mask))
        b = np.packbits(mask, bitorder="little")
        assert w.view(np.uint8)[:len(b)].tobytes() == b.tobytes() if np.little_endian else True
        # bit i of word i >> 5 is mask[i]
        ids = np.arange(n)
        assert np.array_equal(((w[ids >> 5] >> (ids & 31).astype(np.uint32)) & 1).astype(bool), mask)
