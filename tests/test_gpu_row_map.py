"""GPU tests of the row map: results and filters in input rows (rows of the array given to build()).

Indexes are built here, one per kernel shape (D = 128, 960 -> 1024, the generic instantiation at 200 -> 256, and
96 -> 128 once more with 2-bit codes), two of them on data in which every row occurs several times: there exact row
matching (internal_to_input_rows) cannot tell the copies apart and only the builder's own map is right.  Everything
is an identity, not a tolerance: the map is a permutation, get_vectors()[i] is base[row_map()[i]] bit for bit,
result_ids = "input" returns row_map()[internal ids] with the same distance bytes on every search path, and a filter
given in input rows equals the internal filter made from mask[row_map()].
"""
import struct
import threading

import numpy as np
import pytest

from golden_util import fixture_path

pytestmark = pytest.mark.gpu

FMAX = np.float32(3.402823466e+38)

# (dim, bits, n, kind): n neither a multiple of 32 nor of 64 except where the copies dictate it
CASES = {
    "d128b4": (128, 4, 20_001, "gauss"),
    "d960b2": (960, 2, 6_007, "gauss"),
    "d200b1dups": (200, 1, 8_000, "dups"),      # 1,000 distinct rows x 8 copies; generic kernel (D = 256)
    "d96b2dups": (96, 2, 10_010, "dups"),       # 770 distinct rows x 13 copies
}


def make_data(dim, n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "dups":
        copies = 8 if n % 8 == 0 else 13
        X = np.repeat(rng.standard_normal((n // copies, dim)).astype(np.float32), copies, axis=0)[rng.permutation(n)]
    else:
        X = rng.standard_normal((n, dim)).astype(np.float32)
    Q = (X[rng.integers(0, n, 3000)] + 0.3 * rng.standard_normal((3000, dim))).astype(np.float32)
    return np.ascontiguousarray(X), Q


_BUILT = {}


@pytest.fixture(params=list(CASES))
def built(request):
    """(index, base, queries, row_map) of one case; built once per session, handed out in internal mode."""
    import cphnsw_mi355x
    name = request.param
    if name not in _BUILT:
        dim, bits, n, kind = CASES[name]
        X, Q = make_data(dim, n, kind, 1000 + n)
        ix = cphnsw_mi355x.CPIndex(dim, bits, device=0)
        ix.build(X)
        ix.finalize()
        assert ix.has_row_map and ix.result_ids == "internal"
        _BUILT[name] = (ix, X, Q, ix.row_map())
    ix = _BUILT[name][0]
    ix.result_ids = "internal"
    ix.set_search_params(0, 0)
    yield _BUILT[name]
    ix.result_ids = "internal"
    ix.set_search_params(0, 0)


def mapped(ids, rm):
    return np.where(ids >= 0, rm[np.maximum(ids, 0)], -1)


def in_both_modes(ix, fn):
    """fn() under result_ids "internal", then "input"."""
    ix.result_ids = "internal"
    a = fn()
    ix.result_ids = "input"
    try:
        b = fn()
    finally:
        ix.result_ids = "internal"
    return a, b


def assert_translated(internal, inp, rm, what):
    (ii, di), (ir, dr) = internal, inp
    assert ii.shape == ir.shape and ir.dtype == np.int64, what
    assert np.array_equal(ir, mapped(ii, rm)), what
    assert di.tobytes() == dr.tobytes(), what


def test_row_map_is_the_builders_permutation(built):
    ix, X, _, rm = built
    n = X.shape[0]
    assert rm.dtype == np.int64 and rm.shape == (n,)
    assert np.array_equal(np.sort(rm), np.arange(n))
    assert ix.get_vectors().tobytes() == X[rm].tobytes()          # exact also where rows repeat


def test_batch_paths_return_mapped_ids(built):
    ix, X, Q, rm = built
    for nq, k in ((5, 10), (32, 1), (3000, 10), (700, 100)):
        a, b = in_both_modes(ix, lambda: ix.search_batch(Q[:nq], k))
        assert (a[0] >= 0).any()
        assert_translated(a, b, rm, (nq, k))
    # the ids really are input rows: the base row they name is the stored vector the internal id names
    ids_int, _ = a
    ids_row, _ = b
    ok = ids_int >= 0
    assert ix.get_vectors()[ids_int[ok][:500]].tobytes() == X[ids_row[ok][:500]].tobytes()


def test_forced_rerun_launch_returns_mapped_ids(built):
    ix, X, Q, rm = built
    ix.set_search_params(slots=8, beam_capacity=64)
    reruns = []

    def run():
        out = ix.search_batch(Q[:300], 10)
        reruns.append(ix.last_search_stats()["rerun_queries"])
        return out
    a, b = in_both_modes(ix, run)
    assert reruns[0] > 0 and reruns[1] == reruns[0]               # the re-run launch did answer queries, in both modes
    assert_translated(a, b, rm, "rerun")
    ix.set_search_params(0, 0)
    c = ix.search_batch(Q[:300], 10)
    assert np.array_equal(c[0], a[0]) and c[1].tobytes() == a[1].tobytes()


def test_device_batch_on_a_side_stream_returns_mapped_ids(built):
    import torch
    ix, X, Q, rm = built
    dq = torch.from_numpy(Q[:1500]).to("cuda:0")
    side = torch.cuda.Stream(device="cuda:0")

    def run():
        torch.cuda.synchronize()
        ids, dist = ix.search_batch_device(dq, 10, stream=side)
        side.synchronize()
        return ids.cpu().numpy(), dist.cpu().numpy()
    a, b = in_both_modes(ix, run)
    assert_translated(a, b, rm, "device batch")
    host = ix.search_batch(Q[:1500], 10)
    assert np.array_equal(host[0], a[0])


def test_concurrent_single_queries_return_mapped_ids(built):
    """search() from 16 threads: the callers are gathered into shared launches whose kernel raises each caller's done
    flag itself, so the ids must be translated before that flag."""
    ix, X, Q, rm = built
    T, per = 16, 12

    def run():
        out = [None] * (T * per)
        errs = []

        def worker(t):
            try:
                for j in range(per):
                    out[t * per + j] = ix.search(Q[t * per + j], 10)
            except Exception as e:       # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=worker, args=(t,)) for t in range(T)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        return out
    a, b = in_both_modes(ix, run)
    for q in range(T * per):
        (ii, di), (ir, dr) = a[q], b[q]
        assert len(ii) > 0 and np.array_equal(ir, rm[ii]) and di.tobytes() == dr.tobytes(), q
    ref = ix.search_batch(Q[:T * per], 10)
    for q in range(T * per):
        m = len(a[q][0])
        assert np.array_equal(a[q][0], ref[0][q, :m])


def test_filtered_batches_and_padding_return_mapped_ids(built):
    ix, X, Q, rm = built
    n = X.shape[0]
    rng = np.random.default_rng(5)
    half = ix.make_filter(rng.random(n) < 0.5, ids="internal")
    # four ids the queries do reach (their unfiltered nearest neighbours)
    few_ids = np.array(list(dict.fromkeys(ix.search_batch(Q[:400], 1)[0][:, 0].tolist()))[:4])
    assert few_ids.size == 4 and (few_ids >= 0).all()
    few = ix.make_filter(few_ids, ids="internal")                 # fewer than k ids allowed: rows end in padding
    for f, nq in ((half, 8), (half, 1200), (few, 8), (few, 400)):
        a, b = in_both_modes(ix, lambda: ix.search_batch(Q[:nq], 10, filter=f))
        assert_translated(a, b, rm, ("filtered", nq))
    ids_int, dist = a
    ids_row = b[0]
    # (an id may fill more than one slot of a row, SURVEY F2: count the padding, do not place it)
    pad = ids_int == -1
    assert pad.any(axis=1).all() and (ids_row[pad] == -1).all() and (dist[pad] == FMAX).all() and (ids_row[~pad] >= 0).all()
    assert (ids_int >= 0).any()
    assert set(ids_row[ids_row >= 0].tolist()) <= set(rm[few_ids].tolist())
    # a single filtered query (unpadded rows)
    a, b = in_both_modes(ix, lambda: ix.search(Q[0], 10, filter=few))
    assert len(a[0]) < 10 and set(a[0].tolist()) <= set(few_ids.tolist()) and np.array_equal(b[0], rm[a[0]]) and a[1].tobytes() == b[1].tobytes()


def test_filter_in_input_rows_equals_the_mapped_internal_filter(built):
    ix, X, Q, rm = built
    n = X.shape[0]
    rng = np.random.default_rng(9)
    contiguous = np.zeros(n, bool)
    contiguous[n // 5: n // 5 + n // 3] = True                    # "only rows a..b of my table"
    masks = {"half": rng.random(n) < 0.5, "one percent": rng.random(n) < 0.01, "range": contiguous}
    ix.result_ids = "input"
    for name, m in masks.items():
        f_rows = ix.make_filter(m)                                # default id space: the index' result_ids
        f_int = ix.make_filter(m[rm], ids="internal")
        assert f_rows.count == f_int.count == int(m.sum())
        for nq in (6, 900):
            a = ix.search_batch(Q[:nq], 10, filter=f_rows)
            b = ix.search_batch(Q[:nq], 10, filter=f_int)
            assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), (name, nq)
            got = a[0][a[0] >= 0]
            assert got.size and m[got].all(), (name, nq)
        # made on the fly from the mask, and from the list of allowed rows
        c = ix.search_batch(Q[:900], 10, filter=m)
        d = ix.search_batch(Q[:900], 10, filter=np.flatnonzero(m))
        assert np.array_equal(c[0], a[0]) and np.array_equal(d[0], a[0]) and d[1].tobytes() == a[1].tobytes()
        # the same filter object under internal result ids: the same rows, named by their internal ids
        ix.result_ids = "internal"
        e = ix.search_batch(Q[:900], 10, filter=f_rows)
        ix.result_ids = "input"
        assert np.array_equal(mapped(e[0], rm), a[0])
        f_rows.close()
        f_int.close()
    none = ix.make_filter(np.zeros(n, bool), ids="input")
    assert none.count == 0
    ids, dist = ix.search_batch(Q[:50], 10, filter=none)
    assert (ids == -1).all() and (dist == FMAX).all()
    with pytest.raises(ValueError):
        ix.make_filter(np.zeros(n + 1, bool), ids="input")
    with pytest.raises(ValueError):
        ix.make_filter(m, ids="rows")


def test_replicas_on_one_device_return_mapped_ids(built, tmp_path):
    """CPIndex(devices=[0, 0]) loaded from the native file of the built index: replica 1 receives the resident map."""
    import cphnsw_mi355x
    ix, X, Q, rm = built
    dim, bits = X.shape[1], ix._bits
    path = str(tmp_path / "ix.cphn")
    ix.save_native(path)
    multi = cphnsw_mi355x.CPIndex(dim, bits, devices=[0, 0])
    multi.load_native(path)
    multi.set_min_shard(64)
    assert multi.has_row_map and np.array_equal(multi.row_map(), rm)
    want = ix.search_batch(Q[:1000], 10)
    a, b = in_both_modes(multi, lambda: multi.search_batch(Q[:1000], 10))
    assert np.array_equal(a[0], want[0]) and a[1].tobytes() == want[1].tobytes()
    assert_translated(a, b, rm, "two replicas")
    multi.result_ids = "input"
    m = np.random.default_rng(2).random(X.shape[0]) < 0.3
    got = multi.search_batch(Q[:1000], 10, filter=m)             # one row-space filter per replica
    f_int = ix.make_filter(m[rm], ids="internal")
    ref = ix.search_batch(Q[:1000], 10, filter=f_int)
    assert np.array_equal(got[0], mapped(ref[0], rm)) and got[1].tobytes() == ref[1].tobytes()
    for q in range(6):                                            # single queries alternate between the replicas
        ids, dist = multi.search(Q[q], 10)
        assert np.array_equal(ids, rm[want[0][q, :len(ids)]])
    # a map handed to the multi-device handle reaches every replica; without one the mode falls back
    multi.set_row_map(None)
    assert not multi.has_row_map and multi.result_ids == "internal"
    with pytest.raises(ValueError):
        multi.result_ids = "input"
    multi.set_row_map(rm)
    multi.result_ids = "input"
    again = multi.search_batch(Q[:1000], 10)
    assert np.array_equal(again[0], b[0]) and again[1].tobytes() == b[1].tobytes()


def native_version(path):
    """Format of a native file: 2 when its small section ends in the row-map record, else 1.  The header's own version
    field is 1 in both, so that a library that knows format 1 only still loads the file."""
    with open(path, "rb") as f:
        head = f.read(120)
        version, = struct.unpack_from("<I", head, 8)
        small_bytes, = struct.unpack_from("<Q", head, 80)
        assert version == 1
        f.seek(120 + small_bytes - 24)
        magic, fmt = struct.unpack("<QI", f.read(12))
    return fmt if magic == int.from_bytes(b"CPHIROWS", "little") else 1


def test_persistence_and_handles_without_a_map(tmp_path):
    import cphnsw_mi355x
    dim, bits, n = 128, 4, 9_001
    X, Q = make_data(dim, n, "gauss", 77)
    ix = cphnsw_mi355x.CPIndex(dim, bits, device=0)
    ix.build(X)
    ix.finalize()
    rm = ix.row_map()
    ix.result_ids = "input"
    want = ix.search_batch(Q[:500], 10)
    native, v2 = str(tmp_path / "a.cphn"), str(tmp_path / "a.idx")
    ix.save_native(native)
    ix.save(v2)
    assert native_version(native) == 2

    # the native file keeps the map, and the mode works after loading
    a = cphnsw_mi355x.CPIndex(dim, bits, device=0)
    a.load_native(native)
    assert a.has_row_map and a.result_ids == "internal" and np.array_equal(a.row_map(), rm)
    a.result_ids = "input"
    got = a.search_batch(Q[:500], 10)
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
    a.save_native(str(tmp_path / "b.cphn"))
    assert open(native, "rb").read() == open(str(tmp_path / "b.cphn"), "rb").read()

    # the reference's format cannot carry it
    b = cphnsw_mi355x.CPIndex(dim, bits, device=0)
    b.load(v2)
    assert not b.has_row_map
    with pytest.raises(ValueError):
        b.result_ids = "input"
    assert b.result_ids == "internal"
    with pytest.raises(ValueError):
        b.row_map()
    with pytest.raises(ValueError):
        b.make_filter(np.ones(n, bool), ids="input")
    internal = b.search_batch(Q[:500], 10)
    assert np.array_equal(mapped(internal[0], rm), want[0])
    b.save_native(str(tmp_path / "nomap.cphn"))
    assert native_version(str(tmp_path / "nomap.cphn")) == 1
    # ... its owner can hand the map back
    for bad in (np.r_[rm[:-1], rm[0]], rm[:-1], np.r_[rm[:-1], n], np.r_[rm[:-1], -1], rm.astype(np.float64)):
        with pytest.raises(ValueError):
            b.set_row_map(bad)
    assert not b.has_row_map
    b.set_row_map(rm)
    assert b.has_row_map and np.array_equal(b.row_map(), rm)
    b.result_ids = "input"
    got = b.search_batch(Q[:500], 10)
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
    b.save_native(str(tmp_path / "c.cphn"))
    assert native_version(str(tmp_path / "c.cphn")) == 2
    # losing the map puts the handle back to internal ids: set_row_map(None), a v2 load, build()
    b.set_row_map(None)
    assert not b.has_row_map and b.result_ids == "internal"
    got = b.search_batch(Q[:500], 10)
    assert np.array_equal(got[0], internal[0])
    a.load(v2)
    assert not a.has_row_map and a.result_ids == "internal"
    assert np.array_equal(a.search_batch(Q[:500], 10)[0], internal[0])
    ix.build(X[:3000])
    assert ix.result_ids == "internal"
    ix.finalize()
    assert ix.has_row_map and ix.row_map().shape == (3000,)
    assert (ix.search_batch(Q[:20], 10)[0] < 3000).all()


def test_native_file_of_a_reference_built_index_stays_version_1(tmp_path):
    import cphnsw_mi355x
    ix = cphnsw_mi355x.CPIndex(128, 4, device=0)
    ix.load(fixture_path("g128", 4))
    assert not ix.has_row_map
    p = str(tmp_path / "g128.cphn")
    ix.save_native(p)
    assert native_version(p) == 1
    again = cphnsw_mi355x.CPIndex(128, 4, device=0)
    again.load_native(p)
    assert not again.has_row_map
    with pytest.raises(ValueError):
        again.result_ids = "input"
