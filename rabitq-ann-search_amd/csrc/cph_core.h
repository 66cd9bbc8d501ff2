// cph_core.h — shared host/device definitions of the MI355X-native CP-HNSW hot path.
//
// Data layout in HBM.  The reference stores, per vertex, a
// VertexSearchData<D,32,BW> (graph/rabitq_graph.hpp:19-29): the vertex' own code (never
// read at query time) followed by the neighbour block (bit-plane FastScan code blocks +
// nop/ip_qo/ip_cp/popcounts/ids, distance/fastscan_layout.hpp:51-155).  The device copy
// keeps only what the query path reads and re-lays it out for a 64-lane wavefront:
//
//   device block (one per vertex, `stride` bytes, 64-B aligned)
//     codes   32 neighbours x BW planes x PW dwords, bit t of dword w of plane b of
//             neighbour i = code bit of dimension 32w+t.  "wide" (D >= 128): 16-B chunks
//             ordered [k][half][neighbour] so that one wave instruction reads 1 KiB
//             contiguous; lane (half h, neighbour i) owns chunks h*CPL .. h*CPL+CPL-1 of
//             its neighbour's BW*PW dwords (plane-major).  "small" (D < 128): dwords
//             ordered [plane*PW+w][neighbour].
//     aux     32 x {nop, ip_qo, ip_cp, popcount | weighted_popcount << 16}   (16 B each)
//     ids     32 x u32
//     count   u32
//
// 4-bit codes at D >= 128 are RESIDENT on the device in a second code layout (`nib`): neighbour i's D/2 bytes are
// contiguous at byte i*D/2, and 32-bit word w of a neighbour holds dimensions 8w..8w+7, dimension 8w+j in bits
// 4j..4j+3 as the 4-bit value c = sum_b 2^(3-b) bit_b (the operand order of v_dot8_u32_u4).  Two neighbours share
// a 128-B line instead of eight, and one dot instruction sums eight dimensions of all four planes.  The plane-major
// layout above stays the STORAGE layout (native file, repack_*): the device converts after every upload and back
// before every download (relayout_kernel, device_relayout.h).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define CPH_HD __host__ __device__
#else
#define CPH_HD
#endif

namespace cph {

constexpr uint32_t kInvalidNode = 0xFFFFFFFFu;
constexpr int kR = 32;                 // graph degree, src/bindings.cpp:42
constexpr float kEpsTiny = 1e-20f;     // core/constants.hpp:12
constexpr float kEpsSmall = 1e-12f;    // :13
constexpr float kEpsMedium = 1e-10f;   // :14
constexpr int kMaxSlack = 32;          // :29

struct DevLayout {
    uint32_t D;        // padded dimension (power of two, 16..2048)
    uint32_t BW;       // bits per dimension (1, 2, 4)
    uint32_t PW;       // dwords per plane per neighbour = max(1, D/32)
    uint32_t wide;     // D >= 128
    uint32_t NH;       // lane halves that carry codes (wide: 2 if BW*PW >= 8 else 1)
    uint32_t CPL;      // 16-B chunks per lane (wide)
    uint32_t codes_bytes;
    uint32_t aux_off;  // byte offsets inside a block
    uint32_t ids_off;
    uint32_t count_off;
    uint32_t stride;   // block bytes (multiple of 64)
    uint32_t nib;      // BW == 4 and wide: the resident codes are neighbour-major nibbles (see the top of this file)
};

#ifndef CPH_BLOCK_ALIGN
#define CPH_BLOCK_ALIGN 64u   // (128 -- a block never straddles one more 128-byte line than it needs -- measured: see DESIGN.md section 6)
#endif
// The byte offsets of make_dev_layout as compile-time constants, for the kernels with a compile-time D: a block's
// address arithmetic then needs neither scalar registers for the layout nor (what the compiler did when it ran out of
// them) a reload of it from the kernarg segment inside the expansion loop.
template <int BW, int SD>
struct StaticLayout {
    static constexpr uint32_t kCodesBytes = 32u * (uint32_t)BW * (SD >= 32 ? (uint32_t)SD / 32u : 1u) * 4u;
    static constexpr uint32_t kAuxOff = kCodesBytes;
    static constexpr uint32_t kIdsOff = kAuxOff + 32u * 16u;
    static constexpr uint32_t kCountOff = kIdsOff + 32u * 4u;
    static constexpr uint32_t kStride = (kCountOff + 4u + CPH_BLOCK_ALIGN - 1u) / CPH_BLOCK_ALIGN * CPH_BLOCK_ALIGN;
};

inline DevLayout make_dev_layout(uint32_t D, uint32_t BW) {
    DevLayout L{};
    L.D = D;
    L.BW = BW;
    L.PW = D >= 32 ? D / 32 : 1;
    L.wide = D >= 128 ? 1 : 0;
    uint32_t T = BW * L.PW;  // dwords per neighbour
    if (L.wide) {
        L.NH = (T / 4 >= 2) ? 2 : 1;
        L.CPL = T / 4 / L.NH;
    } else {
        L.NH = 1;
        L.CPL = 0;
    }
    L.codes_bytes = 32 * T * 4;
    L.aux_off = L.codes_bytes;           // multiple of 128
    L.ids_off = L.aux_off + 32 * 16;
    L.count_off = L.ids_off + 32 * 4;
    L.stride = (L.count_off + 4 + CPH_BLOCK_ALIGN - 1) / CPH_BLOCK_ALIGN * CPH_BLOCK_ALIGN;
    L.nib = (BW == 4 && L.wide) ? 1 : 0;
    return L;
}

// Byte offset of plane-major code dword (plane, w) of neighbour i (the storage layout).
CPH_HD inline uint32_t plane_dword_offset(const DevLayout& L, uint32_t plane, uint32_t w, uint32_t i) {
    const uint32_t t = plane * L.PW + w;
    if (L.wide) {
        const uint32_t ck = t / 4, e = t % 4;
        const uint32_t h = (L.NH == 2) ? ck / L.CPL : 0;
        const uint32_t k = (L.NH == 2) ? ck % L.CPL : ck;
        return (k * L.NH * 32 + h * 32 + i) * 16 + e * 4;
    }
    return (t * 32 + i) * 4;
}

// bit j of the low byte -> bit 4j, and back
CPH_HD inline uint32_t nib_spread8(uint32_t x) {
    x &= 0xFFu;
    x = (x | (x << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    return (x | (x << 3)) & 0x11111111u;
}
CPH_HD inline uint32_t nib_compact8(uint32_t x) {
    x &= 0x11111111u;
    x = (x | (x >> 3)) & 0x03030303u;
    x = (x | (x >> 6)) & 0x000F000Fu;
    return (x | (x >> 12)) & 0xFFu;
}
// Nibble word w (dims 8w..8w+7) of one neighbour from its four plane dwords of 32-dim word w/4 (plane 0 = MSB).
CPH_HD inline uint32_t nib_word_from_planes(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t w) {
    const uint32_t sh = 8u * (w & 3u);
    return (nib_spread8(p0 >> sh) << 3) | (nib_spread8(p1 >> sh) << 2) | (nib_spread8(p2 >> sh) << 1) |
           nib_spread8(p3 >> sh);
}
// Plane dword (plane b, 32-dim word pw) of one neighbour from its nibble words 4pw..4pw+3.
CPH_HD inline uint32_t plane_dword_from_nibs(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t b) {
    const uint32_t sh = 3u - b;
    return nib_compact8(n0 >> sh) | (nib_compact8(n1 >> sh) << 8) | (nib_compact8(n2 >> sh) << 16) |
           (nib_compact8(n3 >> sh) << 24);
}
// The query's 4-bit scalars of 32 dims, bit-sliced {Q0,Q1,Q2,Q3} (bit t of Q_j = bit j of q_u[32g+t]), as the four
// nibble words of those dims (dims 32g+8s.. in word s).
CPH_HD inline uint32_t qmask_nib_word(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, uint32_t s) {
    const uint32_t sh = 8u * s;
    return nib_spread8(q0 >> sh) | (nib_spread8(q1 >> sh) << 1) | (nib_spread8(q2 >> sh) << 2) | (nib_spread8(q3 >> sh) << 3);
}

// Reference (file) layout of VertexSearchData<D,32,BW>; SURVEY.md §5.4.
struct RefLayout {
    size_t vertex_bytes, nb_off;
    size_t codes, nop, ip_qo, ip_cp, pop, wpop, ids, count;  // inside the neighbour block
    size_t plane_bytes, nb_bytes;
};

inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

inline RefLayout make_ref_layout(size_t D, size_t bw) {
    RefLayout L{};
    size_t words = (D + 63) / 64;
    size_t code = round_up(round_up(bw * words * 8, 64) + 8, 64);
    L.plane_bytes = (((D + 3) / 4 + 1) / 2) * 32;
    size_t o = 0;
    L.codes = o; o += bw * round_up(L.plane_bytes, 64);
    L.nop = o;   o += 128;
    L.ip_qo = o; o += 128;
    L.ip_cp = o; o += 128;
    L.pop = o;   o += 64;
    if (bw > 1) { L.wpop = o; o += 64; } else { L.wpop = (size_t)-1; }
    L.ids = o;   o += 128;
    L.count = o; o += 4;
    L.nb_bytes = round_up(o, 64);
    L.nb_off = code;
    L.vertex_bytes = code + L.nb_bytes;
    return L;
}

// Per-query record handed to the search kernel (host- or device-encoded).
// qparams mirror RaBitQQuery's scalars (core/codes.hpp:79-93).
struct QueryHeader {
    float A, B, C;        // coeff_fastscan, coeff_popcount, coeff_constant
    uint32_t entry;       // layer-0 entry point after the upper-layer descent
};

// Search-wide constants (CalibrationSnapshot, api/hnsw_index.hpp:33-58).
struct SearchConsts {
    float affine_a, affine_b, ip_qo_floor;
    float gamma, gamma_max, gamma_beta;
    uint64_t gamma_warmup;
    int32_t num_slack;
    float slack[kMaxSlack];
};

enum QueryStatus : uint32_t { kStatusOk = 0, kStatusOverflow = 1 };

}  // namespace cph
