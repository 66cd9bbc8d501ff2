"""The resident layout of 4-bit codes at D >= 128 (neighbour-major nibbles, cph_core.h `nib`) on the host: the
library's host restatement of the device re-layout against the layout's definition, and the v_dot8 sums of the
FastScan estimator against the plane sums they replace."""
import ctypes as C

import numpy as np
import pytest

from block_layout import _codes_from_planes, _layout, _plane_dword_offset  # noqa: F401


@pytest.fixture(scope="module")
def L():
    from cphnsw_mi355x import _lib
    return _lib


def _relayout(L, D, bits, dev):
    res = np.zeros_like(dev)
    back = np.zeros_like(dev)
    L.check(L.lib().cph_host_relayout_block(D, bits, dev.ctypes.data, res.ctypes.data, back.ctypes.data))
    return res, back


def _random_block(D, bits, seed, count=32):
    stride = _layout(D, bits)[5]
    rng = np.random.default_rng(seed)
    dev = rng.integers(0, 256, stride, dtype=np.uint8)
    codes = 32 * bits * max(1, D // 32) * 4
    dev[codes + 512 + 128:codes + 512 + 132] = np.array([count], np.uint32).view(np.uint8)
    return dev, codes


@pytest.mark.parametrize("D", [128, 256, 1024, 2048])
@pytest.mark.parametrize("count", [32, 29, 5])
def test_nibble_round_trip_and_byte_positions(L, D, count):
    dev, codes = _random_block(D, 4, D * 100 + count, count)
    res, back = _relayout(L, D, 4, dev)
    assert back.tobytes() == dev.tobytes()
    assert res[codes:].tobytes() == dev[codes:].tobytes()    # aux, ids, count, padding unchanged
    c = _codes_from_planes(dev, D, 4)
    words = res[:codes].view(np.uint32).reshape(32, D // 8)   # neighbour i's D/2 bytes at i * D/2
    for j in range(8):                                        # dim 8w + j in bits 4j..4j+3 of word w
        assert np.array_equal((words >> np.uint32(4 * j)) & np.uint32(15), c[:, j::8].astype(np.uint32))


@pytest.mark.parametrize("D,bits", [(128, 1), (128, 2), (1024, 2), (16, 4), (32, 4), (64, 4)])
def test_other_formats_are_resident_as_stored(L, D, bits):
    dev, _ = _random_block(D, bits, D + bits)
    res, back = _relayout(L, D, bits, dev)
    assert res.tobytes() == dev.tobytes() and back.tobytes() == dev.tobytes()


def _dot8(a, b):
    """v_dot8_u32_u4 without clamp: sum over the eight nibble pairs of two words (arrays of uint32)."""
    s = np.zeros(np.broadcast(a, b).shape, np.int64)
    for j in range(8):
        s += ((a.astype(np.int64) >> (4 * j)) & 15) * ((b.astype(np.int64) >> (4 * j)) & 15)
    return s


def _qmask_nib(qu):
    """The query's bit-sliced masks {Q0..Q3} per 32 dims, turned into nibble words as the kernels' LDS fill does."""
    D = len(qu)
    masks = np.zeros((D // 32, 4), np.uint64)
    for d in range(D):
        for j in range(4):
            if (qu[d] >> j) & 1:
                masks[d // 32, j] |= np.uint64(1 << (d % 32))
    out = np.zeros(D // 8, np.int64)
    for g in range(D // 32):
        for s in range(4):
            v = 0
            for j in range(4):
                byte = (int(masks[g, j]) >> (8 * s)) & 0xFF
                for t in range(8):
                    v |= ((byte >> t) & 1) << (4 * t + j)
            out[4 * g + s] = v
    return out


@pytest.mark.parametrize("D", [128, 256, 1024])
def test_dot8_sums_equal_plane_sums(L, D):
    rng = np.random.default_rng(D)
    dev, codes = _random_block(D, 4, D + 7)
    res, _ = _relayout(L, D, 4, dev)
    c = _codes_from_planes(dev, D, 4)
    for trial in range(3):
        qu = rng.integers(0, 16, D)
        if trial == 1:
            qu[:] = 15
        # the plane sums of the estimator: S_b = sum_d q_u[d] bit_b[d]
        bit = [(c >> (3 - b)) & 1 for b in range(4)]
        S = [(bit[b] * qu[None, :]).sum(1) for b in range(4)]
        nbit = 8 * S[0] + 4 * S[1] + 2 * S[2] + S[3]
        msb, msb2 = S[0], 2 * S[0] + S[1]
        # the kernels: lane half h sums words h, h + 2, .. of 16-B chunks (4 words each), then the halves are added
        words = res[:codes].view(np.uint32).reshape(32, D // 8).astype(np.int64)
        qn = _qmask_nib(qu)
        s = _dot8(words, qn[None, :]).sum(1)
        s8 = _dot8(words & 0x88888888, qn[None, :]).sum(1)
        s12 = _dot8(words & 0xCCCCCCCC, qn[None, :]).sum(1)
        assert np.array_equal(s, nbit)
        assert np.array_equal(s8, 8 * msb) and np.array_equal(s12 >> 2, msb2) and np.all(s12 % 4 == 0)
        if D <= 256:   # the packed merge of s and s8 (nib_merge): both totals fit 16 bits
            assert s.max() < 65536 and s8.max() < 65536


def test_relayout_rejects_bad_arguments(L):
    dev = np.zeros(4096, np.uint8)
    with pytest.raises(ValueError):
        L.check(L.lib().cph_host_relayout_block(100, 4, dev.ctypes.data, dev.ctypes.data, None))
    with pytest.raises(ValueError):
        L.check(L.lib().cph_host_relayout_block(128, 3, dev.ctypes.data, dev.ctypes.data, None))
