"""The storage (plane-major) layout of a device neighbour block (cph_core.h: make_dev_layout, plane_dword_offset), read
with numpy: 32 x bits x PW code dwords, then 32 aux uint4 {nop, ip_qo, ip_cp, msb popcount | weighted popcount << 16},
32 neighbour ids, the count, padding to 64 bytes."""
import numpy as np


def _layout(D, bits):
    PW = max(1, D // 32)
    T = bits * PW
    wide = D >= 128
    NH = 2 if (wide and T // 4 >= 2) else 1
    CPL = (T // 4 // NH) if wide else 0
    stride = (32 * T * 4 + 512 + 128 + 4 + 63) // 64 * 64
    return PW, T, wide, NH, CPL, stride


def _plane_dword_offset(D, bits, b, w, i):
    PW, T, wide, NH, CPL, _ = _layout(D, bits)
    t = b * PW + w
    if wide:
        ck, e = t // 4, t % 4
        h = ck // CPL if NH == 2 else 0
        k = ck % CPL if NH == 2 else ck
        return (k * NH * 32 + h * 32 + i) * 16 + e * 4
    return (t * 32 + i) * 4


def _codes_from_planes(dev, D, bits):
    """c[i, d] = sum_b 2^(bits-1-b) bit_b[d] of neighbour i, read from a plane-major block."""
    PW = max(1, D // 32)
    c = np.zeros((32, D), np.int64)
    for b in range(bits):
        for w in range(PW):
            for i in range(32):
                o = _plane_dword_offset(D, bits, b, w, i)
                v = int(dev[o:o + 4].view(np.uint32)[0])
                for t in range(min(32, D)):
                    c[i, 32 * w + t] += ((v >> t) & 1) << (bits - 1 - b)
    return c


def codes_bytes(D, bits):
    return 32 * _layout(D, bits)[1] * 4


def block_codes(dev, D, bits):
    """_codes_from_planes without the Python loops over neighbours and bits: uint8[32, D]."""
    PW = max(1, D // 32)
    words = np.ascontiguousarray(dev[:codes_bytes(D, bits)]).view(np.uint32)
    i = np.arange(32)
    t = np.arange(min(32, D), dtype=np.uint32)
    c = np.zeros((32, D), np.uint8)
    for b in range(bits):
        for w in range(PW):
            v = words[_plane_dword_offset(D, bits, b, w, i) // 4]                       # [32] dwords, one per neighbour
            bit = ((v[:, None] >> t[None, :]) & np.uint32(1)).astype(np.uint8)
            c[:, 32 * w:32 * w + len(t)] += bit << np.uint8(bits - 1 - b)
    return c


def block_aux(dev, D, bits):
    """-> (aux float32[32, 3] = nop, ip_qo, ip_cp; pops uint32[32, 2] = msb popcount, weighted popcount)."""
    o = codes_bytes(D, bits)
    a = np.ascontiguousarray(dev[o:o + 512]).view(np.uint32).reshape(32, 4)
    aux = np.ascontiguousarray(a[:, :3]).view(np.float32)
    pops = np.stack([a[:, 3] & np.uint32(0xFFFF), a[:, 3] >> np.uint32(16)], axis=1)
    return aux, pops


def block_ids(dev, D, bits):
    """-> (ids uint32[32], count)."""
    o = codes_bytes(D, bits) + 512
    ids = np.ascontiguousarray(dev[o:o + 128]).view(np.uint32).copy()
    count = int(np.ascontiguousarray(dev[o + 128:o + 132]).view(np.uint32)[0])
    return ids, count
