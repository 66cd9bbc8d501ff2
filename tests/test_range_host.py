"""CPU tier of the range search: the host statements of what the device does behind the distances -- the rank rule of one
merge pass (cph_host_range_merge_pass), the cut of a batch into scratch tiles (cph_host_range_tiles) and into candidate
parts (cph_host_range_plan) -- and the argument checks of the new entry points."""
import ctypes as C

import numpy as np
import pytest

INVALID_ARGUMENT = 1


def _L():
    from cphnsw_mi355x import _lib
    return _lib, _lib.lib()


def _merge_pass(keys, width):
    _lib, L = _L()
    a = np.ascontiguousarray(keys, np.uint64)
    out = np.full(max(len(a), 1), 0xDEADBEEFDEADBEEF, np.uint64)
    _lib.check(L.cph_host_range_merge_pass(a.ctypes.data, out.ctypes.data, len(a), width))
    return out[:len(a)]


@pytest.mark.parametrize("w", [4, 64])
def test_merge_passes_sort_runs_of_any_length(w):
    rng = np.random.default_rng(w)
    for n in (1, w, w + 1, 2 * w, 2 * w + 1, 3 * w - 1, 5 * w + 7):
        # unique keys shaped like the device's: distance bits << 32 | id, with many equal distances
        keys = (rng.integers(0, 5, n).astype(np.uint64) << np.uint64(32)) | rng.permutation(n).astype(np.uint64)
        assert len(set(keys.tolist())) == n
        cur = keys.copy()
        for lo in range(0, n, w):                       # the runs the LDS sort leaves
            cur[lo:lo + w] = np.sort(cur[lo:lo + w])
        width = w
        while width < n:
            nxt = _merge_pass(cur, width)
            assert sorted(nxt.tolist()) == sorted(keys.tolist()), (n, width)      # a permutation: nothing lost, nothing twice
            for lo in range(0, n, 2 * width):
                assert (np.diff(nxt[lo:lo + 2 * width].astype(np.int64)) > 0).all(), (n, width, lo)
            cur = nxt
            width *= 2
        assert np.array_equal(cur, np.sort(keys)), n
    # a single run is its own merge: copied
    one = np.sort(rng.permutation(w - 1).astype(np.uint64))
    assert np.array_equal(_merge_pass(one, w), one)


def _tiles(lims, budget):
    _lib, L = _L()
    lims = np.ascontiguousarray(lims, np.int64)
    n = len(lims) - 1
    starts = np.full(n + 2, -1, np.int64)
    nt = C.c_uint64(99)
    _lib.check(L.cph_host_range_tiles(lims.ctypes.data, n, budget, starts.ctypes.data, C.byref(nt)))
    t = nt.value
    if t == 0:
        assert (starts == -1).all()
        return []
    assert (starts[t + 1:] == -1).all()
    return [int(x) for x in starts[:t + 1]]


def _run():
    return _plan(100000, 100, 256)[3]


def _rows_read(lo, hi, gq):
    """One past the last padded query row a fill launch over the queries [lo, hi) reads: its groups of gq start at lo, and
    every group reads whole tiles of 8 rows (exact_fma_chunk), also behind its last query."""
    end = 0
    for g0 in range(lo, hi, gq):
        cnt = min(gq, hi - g0)
        end = max(end, g0 + (cnt + 7) // 8 * 8)
    return end


@pytest.mark.parametrize("budget", [1, 4096, 1 << 16, 1 << 20, 1 << 30])
def test_tiles_are_consecutive_cover_all_queries_and_fit(budget):
    rng = np.random.default_rng(budget % 1000)
    run = _run()
    for counts in (rng.integers(0, 50, 200), rng.integers(0, 3 * run, 40), np.array([0, 0, 5 * run, 0, 1, run, run + 1, 0]),
                   np.array([7])):
        lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        n = len(counts)
        gq, rows = _plan(100000, n, 256)[2], _plan(100000, n, 256)[4]
        starts = _tiles(lims, budget)
        assert starts[0] == 0 and starts[-1] == n and all(b > a for a, b in zip(starts, starts[1:]))
        for lo, hi in zip(starts, starts[1:]):
            keys = int(lims[hi] - lims[lo])
            twice = 2 if (counts[lo:hi] > run).any() else 1          # merge passes need the second buffer
            assert keys * 8 * twice <= budget or hi - lo == 1, (budget, lo, hi)
            assert _rows_read(lo, hi, gq) <= rows, (lo, hi, rows)     # the padded query array holds every row the fill reads
            if hi < n:                                               # maximal: the next query would not have fitted
                twice2 = 2 if (counts[lo:hi + 1] > run).any() else 1
                assert int(lims[hi + 1] - lims[lo]) * 8 * twice2 > budget, (budget, lo, hi)


def test_tiles_of_an_empty_answer():
    assert _tiles(np.zeros(11, np.int64), 1 << 20) in ([], [0, 10])
    assert _tiles(np.zeros(1, np.int64), 1 << 20) == []              # n = 0
    _lib, L = _L()
    bad = np.array([0, 5, 3], np.int64)
    out = np.zeros(4, np.uint64)
    nt = C.c_uint64(0)
    assert L.cph_host_range_tiles(bad.ctypes.data, 2, 1 << 20, out.ctypes.data, C.byref(nt)) == INVALID_ARGUMENT


def _plan(m, nq, cus):
    _lib, L = _L()
    out = (C.c_uint64 * 5)()
    _lib.check(L.cph_host_range_plan(m, nq, cus, out))
    return [int(x) for x in out]


@pytest.mark.parametrize("cus", [1, 64, 256])
@pytest.mark.parametrize("m,nq", [(1, 1), (63, 7), (700, 200), (7000, 200), (70000, 24), (100000, 10000), (1000000, 10000)])
def test_range_plan_covers_the_candidates(m, nq, cus):
    P, part, gq, run, rows = _plan(m, nq, cus)
    assert rows % 8 == 0 and rows >= nq + 7
    assert part % 64 == 0 and (P - 1) * part < m <= P * part         # the parts cover the candidates, none is empty
    assert 1 <= P <= 256 and gq % 8 == 0
    assert run >= 64 and run & (run - 1) == 0 and run * 8 <= 64 * 1024


def test_range_plan_follows_the_exact_plan_and_refuses_nonsense():
    # few queries: as many parts as fill the GPU; many queries fill it on their own
    assert _plan(70000, 24, 256)[0] > 1
    assert _plan(9001, 24, 256)[0] > 1
    assert _plan(100000, 10000, 256)[0] == 26
    # the padded query array: whole tiles of 8 rows plus one tile, for a fill launch that starts between two tiles
    assert [_plan(1000, nq, 256)[4] for nq in (1, 8, 9, 24)] == [16, 16, 24, 32]
    assert _rows_read(14, 24, 128) == 30 <= _plan(9001, 24, 256)[4]           # the tile [14, 24) of 24 queries
    _lib, L = _L()
    out = (C.c_uint64 * 5)()
    assert L.cph_host_range_plan(0, 10, 256, out) == INVALID_ARGUMENT
    assert L.cph_host_range_plan(10, 0, 256, out) == INVALID_ARGUMENT
    assert L.cph_host_range_plan(10, 10, 256, None) == INVALID_ARGUMENT


def test_null_arguments_are_invalid():
    _lib, L = _L()
    obj, total = C.c_void_p(), C.c_uint64(7)
    q = np.zeros((2, 8), np.float32)
    r = np.ones(2, np.float32)
    assert L.cph_range_search_begin(None, q.ctypes.data, 0, 2, r.ctypes.data, None, 1, 0, None, C.byref(obj), C.byref(total)) == INVALID_ARGUMENT
    assert "null" in L.cph_last_error().decode()
    assert L.cph_multi_range_search_begin(None, q.ctypes.data, 2, r.ctypes.data, None, 1, 0, C.byref(obj), C.byref(total)) == INVALID_ARGUMENT
    lims = np.zeros(3, np.int64)
    assert L.cph_range_search_finish(None, lims.ctypes.data, None, None, 0) == INVALID_ARGUMENT
    assert L.cph_multi_range_search_finish(None, lims.ctypes.data, None, None) == INVALID_ARGUMENT
    assert L.cph_range_destroy(None) == 0 and L.cph_multi_range_destroy(None) == 0          # no-ops, like cph_filter_destroy
    k = np.arange(4, dtype=np.uint64)
    assert L.cph_host_range_merge_pass(None, k.ctypes.data, 4, 2) == INVALID_ARGUMENT
    assert L.cph_host_range_merge_pass(k.ctypes.data, None, 4, 2) == INVALID_ARGUMENT
    assert L.cph_host_range_merge_pass(k.ctypes.data, k.ctypes.data, 4, 0) == INVALID_ARGUMENT
    nt = C.c_uint64(0)
    assert L.cph_host_range_tiles(None, 2, 1 << 20, k.ctypes.data, C.byref(nt)) == INVALID_ARGUMENT
    assert L.cph_host_range_tiles(lims.ctypes.data, 2, 1 << 20, k.ctypes.data, None) == INVALID_ARGUMENT


def test_range_search_fails_loudly_without_gpu():
    """No handle can be made without a HIP device, so there is nothing a range search could run on: the methods exist,
    and the way to them raises instead of answering from the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import cphnsw_mi355x
    assert callable(cphnsw_mi355x.CPIndex.range_search) and callable(cphnsw_mi355x.CPIndex.range_search_device)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cphnsw_mi355x.CPIndex(128, 4).range_search(np.zeros((1, 128), np.float32), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cphnsw_mi355x.CPIndex(128, 4, devices=[0, 0]).range_search(np.zeros((1, 128), np.float32), 1.0)
