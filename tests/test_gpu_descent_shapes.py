"""GPU tests of the upper-layer descent (csrc/device_encode.h) on hand-made layers: every hop routine, every D.

tests/test_gpu_descent.py reaches the descent through indexes built here, whose layers never hold more than 32
neighbours per vertex.  These tests take a golden fixture's bytes, replace the upper-layer section by layers written by
hand (tests/descent_files.py) and let the library, the oracle and -- where it was compiled -- the reference load the
same file.  Per (fixture, shape), with the fixtures' last bit width, so D = 16, 32, 64, 128, 128 padded from 96, 256,
512, 1024 and 2048:

  wide          layer 1 = every vertex, degrees 0, 1, 2, 7, 8, 9, 31, 32, 33, 40, 61, 62: the paired hop and the
                eight-lane hop of a mapped layer in one walk (one query makes three moves in layer 1 by construction);
                layer 2 has 17 nodes (mapped), layer 3 has 16 (binary search), layer 4 the entry alone
  fallback      wide with layer-1 lists of 63, 64 and min(n - 1, 100): the whole layer loses its map and is searched
                by lower_bound, lists in chunks of eight with a partial last chunk
  stray         neighbour ids that are no nodes of their layer (kInvalidNode in nbr_info / row_of): the walk moves
                there and stops; stray_entry: the entry is no node of the top layer either
  ties          equal raw rows at list positions (0,1), (1,2), (3,4), (7,8), (15,16) in a list of 32 and in a list of
                62, and (31,32), (32,33), (47,48), (60,61) in a list of 62, each with a query that copies the row, so
                that the first stored position decides the id at every level of both reductions; one list holds a copy
                of its own node's row (d == best: no move)
  extra         four layers stored, max_level = 2; extra_level0: max_level = 0: the entry stays where it is
  deep24        24 layers, the most the encoder carries: load_layer's run-time index over all descriptors
  deep25        25 usable layers: refused at load / load_native (the encoder would start layer 24 at the file's entry
                vertex, where the reference starts layer 25 there)

`census` (float64, counts only) asserts before any GPU call that the queries reach what the shape is for.  Then
`entry_point(q)` equals the oracle's for every query, and `search_batch(Q, 10)` equals the oracle's ids and distance
bytes, and the compiled reference's where present; no tolerance anywhere.  The search pins the entry distance (the
launch-order key and the first expansion's distance); it pins the oracle's own descent only as far as the entry point
changes a result -- tests/test_descent_files_host.py compares the oracle with the reference on the same files.
"""
import ctypes as C
import struct

import numpy as np
import pytest

import descent_files as df
from golden_util import DATASETS
from oracle_lib import ref_available, ref_module

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name, bits, shape, gold, oracle, tmp_path_factory):
    """(made, path, loaded index, oracle entry points, oracle ids, oracle distances): once per session."""
    import cphnsw_mi355x
    key = (name, bits, shape)
    if key not in _CASES:
        made = df.make_shape(name, bits, shape, gold[f"Q/{name}"])
        c = df.check_reach(name, shape, made)             # reach, before any GPU call
        print(name, shape, "hops", dict(c["hops"]), "absent", dict(c["absent"]), "max moves", c["max_moves"],
              "ties", dict(c["ties"]), "equal best", c["equal_best"])
        path = str(tmp_path_factory.mktemp("shapes") / f"{name}_b{bits}_{shape}.idx")
        with open(path, "wb") as f:
            f.write(made["data"])
        oi = oracle.load(path)
        want_ep = np.array([oi.entry_point(q) for q in made["Q"]], np.int64)
        want_ids, want_d, _ = oi.search_batch(made["Q"], 10)
        ix = cphnsw_mi355x.CPIndex(DATASETS[name]["dim"], bits, device=0)
        ix.load(path)
        _CASES[key] = (made, path, ix, want_ep, want_ids, want_d)
    return _CASES[key]


PER_SHAPE = [(name, bits, shape) for name, bits in df.FIXTURES for shape in df.SHAPES]


@pytest.mark.parametrize("name,bits,shape", PER_SHAPE)
def test_entry_points_equal_the_oracles(name, bits, shape, gold, oracle, tmp_path_factory):
    made, _, ix, want_ep, _, _ = _case(name, bits, shape, gold, oracle, tmp_path_factory)
    got = np.array([ix.entry_point(q) for q in made["Q"]], np.int64)
    assert np.array_equal(got, want_ep), (name, shape, np.flatnonzero(got != want_ep)[:8])


@pytest.mark.parametrize("name,bits,shape", PER_SHAPE)
def test_search_equals_the_oracles_and_the_references(name, bits, shape, gold, oracle, tmp_path_factory):
    made, path, ix, _, want_ids, want_d = _case(name, bits, shape, gold, oracle, tmp_path_factory)
    ids, d = ix.search_batch(made["Q"], 10)
    assert np.array_equal(ids, want_ids), (name, shape, np.flatnonzero((ids != want_ids).any(1))[:8])
    assert d.tobytes() == want_d.tobytes(), (name, shape)
    if ref_available():
        r = ref_module().CPIndex(DATASETS[name]["dim"], bits)
        r.load(path)
        rids, rd = r.search_batch(made["Q"], 10)
        assert np.array_equal(ids, rids) and d.tobytes() == rd.tobytes(), (name, shape)


@pytest.mark.parametrize("name,shape", [("g16", "wide"), ("g128", "wide"), ("g64", "fallback")])
def test_a_wave_descends_several_queries(name, shape, gold, oracle, tmp_path_factory):
    """3 * grid + 1 queries in one batch (grid = CUs * 32 encoder waves): every wave descends three or four queries, each
    with the registers of the one before behind it.  The shape's queries are cycled with small seeded noise, so that
    consecutive queries of a wave (grid apart) take different hop classes.  Row for row the oracle's."""
    import torch
    bits = DATASETS[name]["bits"][-1]
    made, _, ix, *_ = _case(name, bits, shape, gold, oracle, tmp_path_factory)
    grid = torch.cuda.get_device_properties(0).multi_processor_count * 32
    nq, base = 3 * grid + 1, made["Q"]
    rng = np.random.default_rng(len(base) + grid)
    pick = (np.arange(nq) + 5 * (np.arange(nq) // grid)) % len(base)
    assert (pick[grid:] != pick[:-grid]).all()            # a wave's next query is another one of the shape's
    Q = base[pick] +(1e-3 * float(base.std()) * rng.standard_normal((nq, base.shape[1]))).astype(np.float32)
    Q = np.ascontiguousarray(Q, np.float32)
    oi = oracle.load(_case(name, bits, shape, gold, oracle, tmp_path_factory)[1])
    want_ids, want_d, _ = oi.search_batch(Q, 10)
    ids, d = ix.search_batch(Q, 10)
    bad = np.flatnonzero((ids != want_ids).any(1))
    assert len(bad) == 0, (name, shape, len(bad), bad[:8], bad[:8] // grid)
    assert d.tobytes() == want_d.tobytes()


def test_replica_descends_a_wide_layer_like_the_first(gold, oracle, tmp_path_factory):
    """CPIndex(devices=[0, 0]) on g128 `wide`: replica 1 has its own copies of the layers, row maps and nbr_info."""
    import cphnsw_mi355x
    from cphnsw_mi355x import _lib
    made, path, _, want_ep, want_ids, want_d = _case("g128", 4, "wide", gold, oracle, tmp_path_factory)
    m = cphnsw_mi355x.CPIndex(128, 4, devices=[0, 0])
    m.set_min_shard(1)
    m.load(path)
    ep = C.c_uint32(0)
    got1 = np.empty(len(made["Q"]), np.int64)
    for i, q in enumerate(made["Q"]):
        q = np.ascontiguousarray(q, np.float32)
        _lib.check(_lib.lib().cph_entry_point(m._reps[1], q.ctypes.data, C.byref(ep)))
        got1[i] = ep.value
    assert np.array_equal(got1, want_ep)
    ids, d = m.search_batch(made["Q"], 10)
    assert np.array_equal(ids, want_ids) and d.tobytes() == want_d.tobytes()


@pytest.mark.parametrize("name", ["g16", "g1024"])
@pytest.mark.parametrize("shape", ["wide", "fallback"])
def test_files_round_trip(name, shape, gold, oracle, tmp_path_factory, tmp_path):
    """save() of a loaded hand-made file is that file; save_native / load_native keeps the entry points."""
    import cphnsw_mi355x
    bits = DATASETS[name]["bits"][-1]
    made, _, ix, want_ep, want_ids, want_d = _case(name, bits, shape, gold, oracle, tmp_path_factory)
    ix.save(str(tmp_path / "again.idx"))
    assert (tmp_path / "again.idx").read_bytes() == made["data"]
    ix.save_native(str(tmp_path / "native.bin"))
    nat = cphnsw_mi355x.CPIndex(DATASETS[name]["dim"], bits, device=0)
    nat.load_native(str(tmp_path / "native.bin"))
    got = np.array([nat.entry_point(q) for q in made["Q"]], np.int64)
    assert np.array_equal(got, want_ep)
    ids, d = nat.search_batch(made["Q"], 10)
    assert np.array_equal(ids, want_ids) and d.tobytes() == want_d.tobytes()


@pytest.mark.parametrize("name,bits", [("g128", 4), ("g64", 4)])
def test_more_layers_than_the_encoder_carries_are_refused(name, bits, gold, oracle, tmp_path_factory, tmp_path):
    """25 usable layers: load refuses, names the limit, and leaves the handle as it was and usable.  The same 25 stored
    layers with max_level = 24 load and descend like the oracle; their native file with max_level patched back to 25
    (NativeHeader::max_level, byte 40) is refused by load_native in the same way."""
    import cphnsw_mi355x
    spec = DATASETS[name]
    made = df.make_shape(name, bits, "deep25", gold[f"Q/{name}"])
    assert len(made["layers"]) == 25 and len(made["layers"][24]) >= 2 and made["max_level"] == 25
    _, good, _, want_ep, want_ids, want_d = _case(name, bits, "wide", gold, oracle, tmp_path_factory)
    Q = df.make_shape(name, bits, "wide", gold[f"Q/{name}"])["Q"]
    deep = tmp_path / "deep25.idx"
    deep.write_bytes(made["data"])
    ix = cphnsw_mi355x.CPIndex(spec["dim"], bits, device=0)
    for _ in range(2):                                    # on an empty handle, then on one that holds an index
        with pytest.raises(RuntimeError, match=r"25 upper layers.*at most 24"):
            ix.load(str(deep))
        ix.load(good)
        assert np.array_equal(np.array([ix.entry_point(q) for q in Q], np.int64), want_ep)
    # 25 stored, 24 used: fine, and exact
    cut = bytearray(made["data"])
    struct.pack_into("<i", cut, df.MAX_LEVEL_OFF, 24)
    (tmp_path / "cut.idx").write_bytes(bytes(cut))
    oi = oracle.load(str(tmp_path / "cut.idx"))
    ix.load(str(tmp_path / "cut.idx"))
    cut_ep = np.array([oi.entry_point(q) for q in made["Q"]], np.int64)
    assert np.array_equal(np.array([ix.entry_point(q) for q in made["Q"]], np.int64), cut_ep)
    ix.save_native(str(tmp_path / "cut.bin"))
    nat = bytearray((tmp_path / "cut.bin").read_bytes())
    assert struct.unpack_from("<i", nat, 40)[0] == 24 and struct.unpack_from("<I", nat, 44)[0] == made["entry"]
    struct.pack_into("<i", nat, 40, 25)
    (tmp_path / "deep25.bin").write_bytes(bytes(nat))
    with pytest.raises(RuntimeError, match=r"25 upper layers.*at most 24"):
        ix.load_native(str(tmp_path / "deep25.bin"))
    assert np.array_equal(np.array([ix.entry_point(q) for q in made["Q"]], np.int64), cut_ep)     # still the cut file's
    ix.load_native(str(tmp_path / "cut.bin"))
    assert np.array_equal(np.array([ix.entry_point(q) for q in made["Q"]], np.int64), cut_ep)
    ix.load(good)
    ids, d = ix.search_batch(Q, 10)
    assert np.array_equal(ids, want_ids) and d.tobytes() == want_d.tobytes()
