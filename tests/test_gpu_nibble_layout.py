"""GPU: the device re-layout of 4-bit codes (plane-major storage layout <-> resident neighbour-major nibbles).  The
device's conversion in both directions against the host restatement, and byte-identical files after a load."""

import numpy as np
import pytest

from golden_util import DATASETS, fixture_path

pytestmark = pytest.mark.gpu

FOUR_BIT = [n for n, s in DATASETS.items() if 4 in s["bits"]]


@pytest.fixture(scope="module")
def cph():
    import cphnsw_mi355x
    return cphnsw_mi355x


def _stride(D, bits):
    return (32 * bits * max(1, D // 32) * 4 + 512 + 128 + 4 + 63) // 64 * 64


def _export(ix, D, resident):
    """All device blocks of a 4-bit index: as resident, or converted back to the storage layout by the device."""
    from cphnsw_mi355x import _lib
    n = ix.size
    out = np.zeros(n * _stride(D, 4), np.uint8)
    _lib.check(_lib.lib().cph_export_blocks(ix._h, 0, n, int(resident), out.ctypes.data))
    return out.reshape(n, -1)


def _load(cph, name):
    ix = cph.CPIndex(DATASETS[name]["dim"], 4)
    ix.load(fixture_path(name, 4))
    return ix


def _host_resident(D, bits, storage):
    from cphnsw_mi355x import _lib
    res = np.zeros_like(storage)
    for v in range(storage.shape[0]):
        _lib.check(_lib.lib().cph_host_relayout_block(D, bits, storage[v].ctypes.data, res[v].ctypes.data, None))
    return res


@pytest.mark.parametrize("name", FOUR_BIT)
def test_device_relayout_matches_host(cph, name):
    ix = _load(cph, name)
    D = DATASETS[name]["D"]
    storage = _export(ix, D, False)    # device nib -> plane (staging copy)
    resident = _export(ix, D, True)    # as searched
    want = _host_resident(D, 4, storage)
    assert resident.tobytes() == want.tobytes()
    if D >= 128:
        assert resident.tobytes() != storage.tobytes()
    else:
        assert resident.tobytes() == storage.tobytes()
    # the export leaves the resident copy as it was
    assert _export(ix, D, True).tobytes() == resident.tobytes()


@pytest.mark.parametrize("name", FOUR_BIT)
def test_save_after_load_is_byte_identical(cph, name, tmp_path):
    ix = _load(cph, name)
    D = DATASETS[name]["D"]
    a, n1, b = tmp_path / "a.idx", tmp_path / "a.native", tmp_path / "b.idx"
    ix.save(a)
    ix.save_native(n1)
    ix2 = cph.CPIndex(DATASETS[name]["dim"], 4)
    ix2.load_native(n1)
    ix2.save(b)
    assert a.read_bytes() == b.read_bytes()
    n2 = tmp_path / "b.native"
    ix2.save_native(n2)
    assert n1.read_bytes() == n2.read_bytes()
    assert _export(ix2, D, True).tobytes() == _export(ix, D, True).tobytes()
    # and a v2 file loaded again gives the same native file
    ix3 = cph.CPIndex(DATASETS[name]["dim"], 4)
    ix3.load(a)
    n3 = tmp_path / "c.native"
    ix3.save_native(n3)
    assert n1.read_bytes() == n3.read_bytes()


@pytest.mark.parametrize("dim", [1000, 200])
def test_built_index_round_trip(cph, dim, tmp_path):
    """A built index (codes written by the edge encoder, then re-laid out): export both ways, save / load, search."""
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((400, dim)).astype(np.float32)
    Q = rng.standard_normal((16, dim)).astype(np.float32)
    ix = cph.CPIndex(dim, 4)
    ix.build(X)
    ix.finalize()
    D = 1024 if dim == 1000 else 256
    storage, resident = _export(ix, D, False), _export(ix, D, True)
    assert resident.tobytes() == _host_resident(D, 4, storage).tobytes()
    ids, d = ix.search_batch(Q, 10)
    p = tmp_path / "x.idx"
    ix.save(p)
    ix2 = cph.CPIndex(dim, 4)
    ix2.load(p)
    assert _export(ix2, D, True).tobytes() == resident.tobytes()
    ids2, d2 = ix2.search_batch(Q, 10)
    assert np.array_equal(ids, ids2) and d.tobytes() == d2.tobytes()
