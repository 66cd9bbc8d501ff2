// host_rescore.h — the host statement of two-stage search (cph_rescore_vectors_create, cph_search_rescored;
// device_rescore.h holds the kernels): no HIP call, so the CPU tests build this file with plain g++ under sanitizers.
// Build it with -ffp-contract=off: every product, sum and difference below is rounded on its own.
// tests/rescore_model.py is the same statement in numpy.
//
// The object: one row of dim_full coordinates per internal id, stored as float16 or float32, the row stride padded with
// zeros to a multiple of 16 bytes, and one float32 squared norm per row, summed from the STORED values.
//
// The layout of a sum (rescore_layout), a pure function of (dim_full, dtype):
//     piece      16 stored bytes: E = 8 float16 or 4 float32 coordinates; a row is P = stride / 16 pieces
//     G          the lanes that share a row: the power of two >= P, at most 64
//     lane l     takes the pieces l, l + G, l + 2 G, ... and adds their E products each, in ascending coordinate order, to
//                ONE partial sum that starts as +0
//     the fold   a xor butterfly over the G partial sums: for d = G/2, G/4, ... 1: p[l] = p[l] + p[l ^ d] (all lanes at
//                once); every lane ends with the same value
// dot(q, x), qn = dot(q, q) and xn = dot(x, x) are all sums of this shape; q is the float32 query padded with zeros to the
// row's P * E coordinates, x the stored row converted to float32 (exact).  A partial sum starts as +0 and x + y is -0
// only if both are: no sum of this shape is ever -0.
//     "l2": score = max(0, (qn + xn) - 2 * dot), the shape of the library's exact distance; never -0
//     "ip": score = -dot; never +0
// so that ordering scores as floats and ordering their sign-folded bits agree.
//
// A candidate row is C entries of internal ids and first-stage distances, padded with -1 / FLT_MAX.  Padding, ids at or
// above n_ids and every occurrence of an id after its first are dropped; each survivor is scored; a NaN score is dropped;
// the k best by (score, internal id) ascending are returned with `first` = the distance bytes at the id's first position;
// unused slots are -1 / FLT_MAX / FLT_MAX.  A query whose qn is not < inf gets a row of padding.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <unordered_set>
#include <vector>

namespace cph {

constexpr uint32_t kRescoreMaxCandidates = 1024;    // C <= this (the longest row a search returns)
constexpr uint32_t kRescoreMaxDim = 8192;           // dim_full <= this (the query is held on chip as float32: 32 KiB)
constexpr unsigned long long kRescoreNoRow = ~0ull;

struct RescoreLayout {
    uint32_t elem_bytes;     // 2 or 4
    uint32_t E;              // coordinates per 16-byte piece
    uint32_t stride;         // stored bytes per row, a multiple of 16
    uint32_t pieces;         // stride / 16
    uint32_t padded;         // pieces * E: coordinates per stored row, zeros behind dim_full
    uint32_t G, log2G;       // lanes per row
};

inline RescoreLayout rescore_layout(uint32_t dim_full, bool f32) {
    RescoreLayout L{};
    L.elem_bytes = f32 ? 4u : 2u;
    L.E = 16u / L.elem_bytes;
    L.pieces = (dim_full + L.E - 1) / L.E;
    L.stride = L.pieces * 16u;
    L.padded = L.pieces * L.E;
    L.G = 1;
    L.log2G = 0;
    while (L.G < L.pieces && L.G < 64u) {
        L.G *= 2;
        ++L.log2G;
    }
    return L;
}

// float32 -> float16, round to nearest even; a value that rounds past 65,504 becomes an infinity.
inline uint16_t rescore_f32_to_f16(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7FFFFFFFu;
    if (x > 0x7F800000u) return (uint16_t)(sign | 0x7E00u);                  // NaN
    if (x >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);                 // >= 65,520, Inf
    if (x >= 0x38800000u) {                                                  // a normal float16
        x += 0xFFFu + ((x >> 13) & 1u);
        x -= 0x38000000u;
        return (uint16_t)(sign | (x >> 13));
    }
    const uint32_t e = x >> 23;
    if (e < 102u) return sign;                                               // below 2^-25: zero
    const uint32_t m = (x & 0x7FFFFFu) | 0x800000u, shift = 126u - e;        // value = m * 2^(e - 150) = (m >> shift) * 2^-24
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
    if (rem > half || (rem == half && (h & 1u))) ++h;
    return (uint16_t)(sign | h);
}

// float16 -> float32, exact.
inline float rescore_f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1Fu, m = h & 0x3FFu;
    uint32_t x;
    if (e == 0) {
        const float v = (float)m * 5.9604644775390625e-8f;                   // m * 2^-24
        std::memcpy(&x, &v, 4);
        x |= sign;
    } else if (e == 31) {
        x = sign | 0x7F800000u | (m << 13);
    } else {
        x = sign | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    std::memcpy(&f, &x, 4);
    return f;
}

// The sum of a[i] * b[i] over L.padded coordinates in the shape above.
inline float rescore_sum(const float* a, const float* b, const RescoreLayout& L) {
    float p[64], t[64];
    for (uint32_t l = 0; l < L.G; ++l) {
        float s = 0.0f;
        for (uint32_t piece = l; piece < L.pieces; piece += L.G)
            for (uint32_t e = 0; e < L.E; ++e) {
                const float prod = a[piece * L.E + e] * b[piece * L.E + e];
                s = s + prod;
            }
        p[l] = s;
    }
    for (uint32_t d = L.G >> 1; d; d >>= 1) {
        for (uint32_t l = 0; l < L.G; ++l) t[l] = p[l] + p[l ^ d];
        for (uint32_t l = 0; l < L.G; ++l) p[l] = t[l];
    }
    return p[0];
}

// A stored row as L.padded float32 values.
inline void rescore_load_row(const uint8_t* stored, const RescoreLayout& L, float* out) {
    if (L.elem_bytes == 4) {
        std::memcpy(out, stored, (size_t)L.padded * 4);
        return;
    }
    for (uint32_t i = 0; i < L.padded; ++i) {
        uint16_t h;
        std::memcpy(&h, stored + (size_t)i * 2, 2);
        out[i] = rescore_f16_to_f32(h);
    }
}

inline float rescore_score(float qn, float xn, float dot, bool ip) {
    if (ip) return -dot;
    const float two_dot = 2.0f * dot;
    const float sum = qn + xn;
    const float v = sum - two_dot;
    return (v < 0.0f) ? 0.0f : v;
}

// inv[input row] = internal id, from the row map rows[internal id] = input row over the nb rows of the graph; a row
// behind them (the tail) is its own input row.
inline std::vector<uint32_t> rescore_inverse_rows(const uint32_t* rows, uint64_t nb, uint64_t size) {
    std::vector<uint32_t> inv(size, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < nb; ++i) {
        if (rows[i] >= nb || inv[rows[i]] != 0xFFFFFFFFu) throw std::invalid_argument("the row map is not a permutation");
        inv[rows[i]] = (uint32_t)i;
    }
    for (uint64_t i = nb; i < size; ++i) inv[i] = (uint32_t)i;
    return inv;
}

// Rows in: row r of in [n][dim_full] is converted, written at position dst = inv ? inv[r] : r of stored [n][L.stride] with
// the stride padding zeroed, and norms[dst] = the sum of the squares of the stored values.  A row whose norm is not < inf
// is bad -- it holds a NaN or an Inf, a value that overflows float16, or its norm overflows; the stored values of an Inf,
// a NaN or an overflow are infinities or NaNs, so the one test covers all of them.  -> the number of bad rows; *first_bad:
// the lowest one (kRescoreNoRow: none).
inline uint64_t rescore_rows_in_host(const float* in, uint64_t n, uint32_t dim_full, bool f32, const uint32_t* inv, uint8_t* stored,
                                     float* norms, unsigned long long* first_bad) {
    const RescoreLayout L = rescore_layout(dim_full, f32);
    std::vector<float> x(L.padded);
    uint64_t bad = 0;
    *first_bad = kRescoreNoRow;
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t dst = inv ? inv[r] : r;
        uint8_t* o = stored + dst * L.stride;
        std::memset(o, 0, L.stride);
        if (f32) {
            std::memcpy(o, in + r * dim_full, (size_t)dim_full * 4);
        } else {
            for (uint32_t i = 0; i < dim_full; ++i) {
                const uint16_t h = rescore_f32_to_f16(in[r * dim_full + i]);
                std::memcpy(o + (size_t)i * 2, &h, 2);
            }
        }
        rescore_load_row(o, L, x.data());
        const float xn = rescore_sum(x.data(), x.data(), L);
        norms[dst] = xn;
        if (!(xn < INFINITY)) {
            ++bad;
            if (*first_bad == kRescoreNoRow) *first_bad = r;
        }
    }
    return bad;
}

// n candidate rows of C entries -> per row out_ids / out_score / out_first [k].  fq [n][dim_full]; stored [n_ids][stride]
// and norms [n_ids] as rows-in made them; rows (may be null): ids are written as rows[id].
inline void rescore_rows_host(const int64_t* ids, const float* dist, uint64_t n, uint32_t C, const float* fq, uint32_t dim_full,
                              const uint8_t* stored, const float* norms, uint64_t n_ids, bool f32, bool ip, const uint32_t* rows,
                              uint32_t k, int64_t* out_ids, float* out_score, float* out_first) {
    const RescoreLayout L = rescore_layout(dim_full, f32);
    const float fmax = FLT_MAX;
    struct Cand {
        float score;
        uint64_t id;
        uint32_t pos;
    };
    std::vector<float> qv(L.padded), x(L.padded);
    std::vector<Cand> cand;
    std::unordered_set<int64_t> seen;
    for (uint64_t q = 0; q < n; ++q) {
        const int64_t* ri = ids + q * C;
        const float* rd = dist + q * C;
        std::fill(qv.begin(), qv.end(), 0.0f);
        std::memcpy(qv.data(), fq + q * dim_full, (size_t)dim_full * 4);
        const float qn = rescore_sum(qv.data(), qv.data(), L);
        cand.clear();
        seen.clear();
        for (uint32_t j = 0; j < C && qn < INFINITY; ++j) {
            const int64_t id = ri[j];
            if (id < 0 || (uint64_t)id >= n_ids) continue;
            if (!seen.insert(id).second) continue;
            rescore_load_row(stored + (uint64_t)id * L.stride, L, x.data());
            const float score = rescore_score(qn, norms[id], rescore_sum(qv.data(), x.data(), L), ip);
            if (score != score) continue;
            cand.push_back({score, (uint64_t)id, j});
        }
        std::sort(cand.begin(), cand.end(), [](const Cand& a, const Cand& b) { return a.score < b.score || (a.score == b.score && a.id < b.id); });
        for (uint32_t t = 0; t < k; ++t) {
            if (t < cand.size()) {
                out_ids[q * k + t] = rows ? (int64_t)rows[cand[t].id] : (int64_t)cand[t].id;
                out_score[q * k + t] = cand[t].score;
                std::memcpy(out_first + q * k + t, rd + cand[t].pos, 4);
            } else {
                out_ids[q * k + t] = -1;
                std::memcpy(out_score + q * k + t, &fmax, 4);
                std::memcpy(out_first + q * k + t, &fmax, 4);
            }
        }
    }
}

}  // namespace cph
