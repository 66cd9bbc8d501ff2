// device_rescore_i8.h — two-stage search over int8 rows (CPH_RESCORE_INT8): the kernels that bring rows into a resident
// object as 16-byte pieces of signed bytes with one scale and one norm per row, and the kernel that rescores a candidate
// row against them with exact integer dot products (v_dot4_i32_i8).
//
// The statement ("int8 rows"; tests/test_gpu_rescore_int8.py states it in numpy).  Every float
// operation is rounded on its own; a quotient that is NaN (0 / 0, where a scale underflowed to zero) gives code 0.
//     row     m = max |x_i|, s = m / 127, c_i = m == 0 ? 0 : clamp(rint(x_i / s), -127, 127), S2 = sum c_i^2 (int32),
//             xn = (s * s) * float(S2).  int8 input: the codes as given, s the caller's scale.
//     query   qmax = max |q_i|, sq = qmax / 16256, t_i = qmax == 0 ? 0 : clamp(rint(q_i / sq), -16256, 16256), held as two
//             int8 planes h_i = (t_i + 64) >> 7 and l_i = t_i - 128 h_i; T2 = sum t_i^2 (64 bits), qn = (sq * sq) * float(T2).
//     score   H = sum h_i c_i, L = sum l_i c_i (int32 each), I = 128 H + L (64 bits), dot = (s * sq) * float(I);
//             "l2": max(0, (qn + xn) - 2 dot), "ip": 0 - dot.  Neither is ever -0.
// An integer sum is exact in any order: unlike device_rescore.h nothing here prescribes a sum shape, and the split below
// is chosen for the hardware alone.  A maximum is taken on the bit patterns of |x| as unsigned integers, which order as
// the values do and put Inf and every NaN above all finite values: one v_max_u32 finds the scale and the bad row at once.
//
// rescore_i8_kernel runs ONE 256-thread workgroup per query, like rescore_rows_kernel, and shares its candidate table,
// its sort and its epilogue (device_wg_primitives.h).  LDS:
//     w[P2]                 the sort words: (sign-folded score << 32) | id
//     hq[padded], lq[padded] the two query planes as packed bytes, padded = 16 P, zeros behind dim_full: 2 bytes per
//                           coordinate (16 KiB at 8,192 against the 32 KiB of the float kernels)
//     c_id[C], tab_id[H], tab_pos[H]   as in rescore_rows_kernel
//     red[16]               the cross-wave cells of the qmax and T2 reductions
// The prologue reads the float query twice (the maximum, then the codes: the second read hits the cache).  Thread t makes
// the codes of coordinates 4 t .. 4 t + 3 and writes one dword per plane.  Main loop: G lanes per row, G = the power of
// two >= P, at most 64; lane l takes the pieces l, l + G, ...; per piece one 16-byte global load per candidate in flight,
// two 16-byte LDS reads shared by all of them, and eight dot instructions per candidate.  kRescoreI8Unroll candidates per
// group are in flight with independent accumulators.  H and L fold across the G lanes as two int32 butterflies (each
// total fits: |H| <= 127 x 128 x 8,192 < 2^27.1); lane 0 of the group widens to 64 bits, forms the score, writes the word.
//
// rescore_i8_in_kernel (float rows in) and rescore_i8_copy_in_kernel (int8 rows in) stream one G-lane group per row,
// grid-stride, as rescore_rows_in_kernel does.  The float kernel reads its row twice (group maximum, then the codes).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_rescore.h"

namespace cph {

constexpr uint32_t kRescoreI8Unroll = 4;
constexpr float kRescoreI8RowMax = 127.0f;
constexpr float kRescoreI8QueryMax = 16256.0f;        // 127 x 128: the two planes hold [-16256, 16256]

struct RescoreI8Args {
    RescoreArgs a;                        // a.s: rows of int8 pieces, norms, the int8 layout (E = 16)
    const float* scales;                  // [n_ids]
};

inline size_t rescore_i8_lds_bytes(uint32_t C, uint32_t padded) {
    return (size_t)wg_sort_len(C) * 8 + (size_t)padded * 2 + ((size_t)C + 2 * (size_t)diverse_table_slots(C)) * 4 + 16 * 8;   // at most 45 KiB
}

__device__ __forceinline__ uint32_t rescore_i8_abs_bits(float v) { return __float_as_uint(v) & 0x7FFFFFFFu; }

// clamp(rint(v / s), -lim, lim) as an integer; a NaN quotient gives 0.
__device__ __forceinline__ int rescore_i8_code(float v, float s, float lim) {
    const float r = rintf(__fdiv_rn(v, s));
    if (r != r) return 0;
    return (int)fminf(fmaxf(r, -lim), lim);
}

__device__ __forceinline__ int rescore_i8_fold(int p, uint32_t G) {
    for (uint32_t d = G >> 1; d; d >>= 1) p += __shfl_xor(p, (int)d, 64);
    return p;
}

__device__ __forceinline__ uint32_t rescore_i8_fold_max(uint32_t p, uint32_t G) {
    for (uint32_t d = G >> 1; d; d >>= 1) p = max(p, (uint32_t)__shfl_xor((int)p, (int)d, 64));
    return p;
}

__device__ __forceinline__ int rescore_i8_dot16(const uint4& x, const uint4& y, int acc) {
    acc = __builtin_amdgcn_sdot4((int)x.x, (int)y.x, acc, false);
    acc = __builtin_amdgcn_sdot4((int)x.y, (int)y.y, acc, false);
    acc = __builtin_amdgcn_sdot4((int)x.z, (int)y.z, acc, false);
    acc = __builtin_amdgcn_sdot4((int)x.w, (int)y.w, acc, false);
    return acc;
}

// An integer below 2^53 in magnitude as the nearest float: exact in double, then one rounding.
__device__ __forceinline__ float rescore_i8_to_float(long long v) { return __double2float_rn(__ll2double_rn(v)); }

// ---- the query side of the statement, shared with the exhaustive scan's pack kernel (device_rescore_i8_all.h) ----
// The largest |q_i| by bit pattern over this wave's share of the query: thread tid of T takes i = tid, tid + T, ...
__device__ __forceinline__ uint32_t rescore_i8_query_max(const float* __restrict__ fq, uint32_t dim, uint32_t tid) {
    uint32_t qbits = 0;
    for (uint32_t i = tid; i < dim; i += kRescoreThreads) qbits = max(qbits, rescore_i8_abs_bits(fq[i]));
    return rescore_i8_fold_max(qbits, 64);
}

// The codes t of coordinates 4 i .. 4 i + 3 (0 behind dim, or where the query is not live: qmax zero, NaN or Inf) as one
// dword per plane; t2 += their squares.
__device__ __forceinline__ void rescore_i8_plane_words(const float* __restrict__ fq, uint32_t i, uint32_t dim, bool live, float sq,
                                                       uint32_t& hw, uint32_t& lw, unsigned long long& t2) {
    hw = 0;
    lw = 0;
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
        const uint32_t c = 4 * i + e;
        const int t = (live && c < dim) ? rescore_i8_code(fq[c], sq, kRescoreI8QueryMax) : 0;
        const int h = (t + 64) >> 7, l = t - 128 * h;
        hw |= ((uint32_t)h & 0xFFu) << (8 * e);
        lw |= ((uint32_t)l & 0xFFu) << (8 * e);
        t2 += (unsigned long long)(uint32_t)(t * t);
    }
}

__device__ __forceinline__ float rescore_i8_query_norm(float sq, unsigned long long T2) {
    return __fmul_rn(__fmul_rn(sq, sq), rescore_i8_to_float((long long)T2));
}

// The score of one pair from its integer dot I = 128 H + L: every float operation rounded on its own.
__device__ __forceinline__ float rescore_i8_score(long long I, float scale, float sq, float qn, float xn, bool ip) {
    const float dot = __fmul_rn(__fmul_rn(scale, sq), rescore_i8_to_float(I));
    if (ip) return __fsub_rn(0.0f, dot);
    const float v = __fsub_rn(__fadd_rn(qn, xn), __fmul_rn(2.0f, dot));
    return (v < 0.0f) ? 0.0f : v;
}

// Grid n, kRescoreThreads threads; LDS: rescore_i8_lds_bytes(C, s.padded).
__global__ __launch_bounds__(kRescoreThreads) void rescore_i8_kernel(RescoreI8Args args) {
    extern __shared__ __align__(16) unsigned char smem[];
    const RescoreArgs& a = args.a;
    const uint32_t C = a.C, k = a.k, P2 = wg_sort_len(C), H = diverse_table_slots(C);
    const uint32_t G = a.s.G, pieces = a.s.pieces, padded = a.s.padded, dim = a.s.dim;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long* red = w + P2;
    uint32_t* hq = reinterpret_cast<uint32_t*>(red + 16);                     // (16-byte aligned: P2 * 8 + 128)
    uint32_t* lq = hq + padded / 4;
    uint32_t* c_id = lq + padded / 4;
    uint32_t* tab_id = c_id + C;
    uint32_t* tab_pos = tab_id + H;
    const uint32_t tid = threadIdx.x, sub = tid & (G - 1), grp = tid >> a.s.log2G, groups = kRescoreThreads >> a.s.log2G;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const size_t q = blockIdx.x;
    const int64_t* __restrict__ row_ids = a.ids + q * C;
    const uint32_t* __restrict__ row_dist = reinterpret_cast<const uint32_t*>(a.dist) + q * C;
    const float* __restrict__ fq = a.fq + q * dim;

    // qmax: the largest |q_i| by bit pattern
    uint32_t qbits = rescore_i8_query_max(fq, dim, tid);
    if (lane == 0) red[wave] = qbits;
    for (uint32_t s = tid; s < H; s += kRescoreThreads) id_table_clear(tab_id, tab_pos, s);
    for (uint32_t j = tid; j < P2; j += kRescoreThreads) w[j] = kSortNone;
    __syncthreads();
    qbits = max(max((uint32_t)red[0], (uint32_t)red[1]), max((uint32_t)red[2], (uint32_t)red[3]));
    const bool q_ok = qbits < 0x7F800000u;                                    // (the same in every thread)
    const float qmax = __uint_as_float(qbits);
    const float sq = __fdiv_rn(qmax, kRescoreI8QueryMax);

    // the two planes and T2; the candidates: an id's first position in the row
    unsigned long long t2 = 0;
    for (uint32_t i = tid; i < padded / 4; i += kRescoreThreads) {
        uint32_t hw, lw;
        rescore_i8_plane_words(fq, i, dim, q_ok && qbits != 0, sq, hw, lw, t2);
        hq[i] = hw;
        lq[i] = lw;
    }
    for (uint32_t d = 32; d; d >>= 1) t2 += __shfl_xor(t2, (int)d, 64);
    if (lane == 0) red[4 + wave] = t2;                                        // (cells of their own: red[0..3] may still be read)
    for (uint32_t j = tid; j < C; j += kRescoreThreads) {
        const int64_t id64 = row_ids[j];
        const bool valid = id64 >= 0 && (unsigned long long)id64 < a.s.n_ids;
        const uint32_t id = valid ? (uint32_t)id64 : kNoId;
        c_id[j] = id;
        if (valid) id_table_insert(tab_id, tab_pos, H, id, j);
    }
    __syncthreads();
    for (uint32_t j = tid; j < C; j += kRescoreThreads) {
        const uint32_t id = c_id[j];
        if (id == kNoId) continue;
        if (tab_pos[id_table_find(tab_id, H, id)] != j) c_id[j] = kNoId;      // a repeat
    }
    const unsigned long long T2 = red[4] + red[5] + red[6] + red[7];
    const float qn = rescore_i8_query_norm(sq, T2);
    __syncthreads();

    const uint4* __restrict__ hq4 = reinterpret_cast<const uint4*>(hq);
    const uint4* __restrict__ lq4 = reinterpret_cast<const uint4*>(lq);
    for (uint32_t base = 0; base < C; base += groups * kRescoreI8Unroll) {    // uniform: every thread takes every step
        uint32_t id[kRescoreI8Unroll];
        const uint4* xr[kRescoreI8Unroll];
        int ph[kRescoreI8Unroll], pl[kRescoreI8Unroll];
#pragma unroll
        for (uint32_t u = 0; u < kRescoreI8Unroll; ++u) {
            const uint32_t j = base + u * groups + grp;
            id[u] = (q_ok && j < C) ? c_id[j] : kNoId;
            xr[u] = reinterpret_cast<const uint4*>(a.s.rows + (size_t)(id[u] == kNoId ? 0u : id[u]) * a.s.stride);
            ph[u] = 0;
            pl[u] = 0;
        }
        for (uint32_t piece = sub; piece < pieces; piece += G) {
            uint4 x[kRescoreI8Unroll];
#pragma unroll
            for (uint32_t u = 0; u < kRescoreI8Unroll; ++u) x[u] = id[u] != kNoId ? xr[u][piece] : make_uint4(0u, 0u, 0u, 0u);
            const uint4 qh = hq4[piece], ql = lq4[piece];
#pragma unroll
            for (uint32_t u = 0; u < kRescoreI8Unroll; ++u) {
                ph[u] = rescore_i8_dot16(x[u], qh, ph[u]);
                pl[u] = rescore_i8_dot16(x[u], ql, pl[u]);
            }
        }
        // one butterfly level for all 2 x kRescoreI8Unroll sums at a time: the shuffles of a level are independent, so a
        // level costs one round trip, not one per sum
        for (uint32_t d = G >> 1; d; d >>= 1) {
            int th[kRescoreI8Unroll], tl[kRescoreI8Unroll];
#pragma unroll
            for (uint32_t u = 0; u < kRescoreI8Unroll; ++u) {
                th[u] = __shfl_xor(ph[u], (int)d, 64);
                tl[u] = __shfl_xor(pl[u], (int)d, 64);
            }
#pragma unroll
            for (uint32_t u = 0; u < kRescoreI8Unroll; ++u) {
                ph[u] += th[u];
                pl[u] += tl[u];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < kRescoreI8Unroll; ++u) {
            if (sub != 0 || id[u] == kNoId) continue;
            const long long I = 128ll * (long long)ph[u] + (long long)pl[u];
            const float score = rescore_i8_score(I, args.scales[id[u]], sq, qn, a.ip ? 0.0f : a.s.norms[id[u]], a.ip != 0);
            if (score == score) w[base + u * groups + grp] = ((unsigned long long)orderable(score) << 32) | id[u];
        }
    }
    __syncthreads();
    wg_sort(w, P2, tid);

    int64_t* __restrict__ out_ids = a.out_ids + q * k;
    uint32_t* __restrict__ out_score = reinterpret_cast<uint32_t*>(a.out_score) + q * k;
    uint32_t* __restrict__ out_first = reinterpret_cast<uint32_t*>(a.out_first) + q * k;
    for (uint32_t t = tid; t < k; t += kRescoreThreads) {
        const unsigned long long word = w[t];             // (k <= C <= P2)
        if (word == kSortNone) {
            out_ids[t] = -1;
            out_score[t] = 0x7F7FFFFFu;                   // FLT_MAX
            out_first[t] = 0x7F7FFFFFu;
            continue;
        }
        const uint32_t id = (uint32_t)word;
        const uint32_t s = id_table_find(tab_id, H, id);
        out_ids[t] = (int64_t)(a.rows ? a.rows[id] : id);
        out_score[t] = __float_as_uint(from_orderable((uint32_t)(word >> 32)));
        out_first[t] = row_dist[tab_pos[s]];
    }
}

// Enqueues the pass over n rows (n >= 1).
inline void rescore_i8_rows(const RescoreI8Args& a, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(rescore_i8_kernel, dim3(n), dim3(kRescoreThreads), rescore_i8_lds_bytes(a.a.C, a.a.s.padded), st, a);
    HIP_CHECK(hipGetLastError());
}

// Lane 0 of a row's group: the scale, the norm, and the count of a bad row.
__device__ __forceinline__ void rescore_i8_finish_row(uint64_t dst, uint64_t row, float s, int S2, bool bad, float* out_scales,
                                                      float* out_norms, unsigned long long* counters) {
    const float xn = __fmul_rn(__fmul_rn(s, s), (float)S2);
    out_scales[dst] = s;
    out_norms[dst] = xn;
    if (bad || !(xn < __builtin_inff())) {
        atomicAdd(counters, 1ull);
        atomicMin(counters + 1, (unsigned long long)row);
    }
}

// in [n][dim] float32 (rows row_base .. row_base + n of the caller's array) -> codes, scales and norms at dst = inv ?
// inv[row] : row; counters = {bad rows, the lowest bad row}.
__global__ __launch_bounds__(256) void rescore_i8_in_kernel(const float* in, uint64_t n, uint64_t row_base, const uint32_t* inv, RescoreStore s,
                                                            uint8_t* out_rows, float* out_scales, float* out_norms,
                                                            unsigned long long* counters) {
    const uint32_t G = s.G, sub = threadIdx.x & (G - 1), grp = threadIdx.x >> s.log2G, groups = 256u >> s.log2G;
    for (uint64_t r0 = (uint64_t)blockIdx.x * groups; r0 < n; r0 += (uint64_t)gridDim.x * groups) {      // uniform
        const uint64_t row = r0 + grp;
        const bool live = row < n;
        const uint64_t dst = !live ? 0 : (inv ? (uint64_t)inv[row_base + row] : row_base + row);
        const float* x = in + row * s.dim;
        uint32_t mbits = 0;
        if (live)
            for (uint32_t i = sub; i < s.dim; i += G) mbits = max(mbits, rescore_i8_abs_bits(x[i]));
        mbits = rescore_i8_fold_max(mbits, G);
        const float sc = __fdiv_rn(__uint_as_float(mbits), kRescoreI8RowMax);
        int S2 = 0;
        for (uint32_t piece = sub; piece < s.pieces; piece += G) {
            uint32_t o[4];
#pragma unroll
            for (uint32_t d = 0; d < 4; ++d) {
                o[d] = 0;
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e) {
                    const uint32_t c = piece * 16 + d * 4 + e;
                    const int code = (live && mbits != 0 && c < s.dim) ? rescore_i8_code(x[c], sc, kRescoreI8RowMax) : 0;
                    o[d] |= ((uint32_t)code & 0xFFu) << (8 * e);
                }
                S2 = __builtin_amdgcn_sdot4((int)o[d], (int)o[d], S2, false);
            }
            if (live) *reinterpret_cast<uint4*>(out_rows + dst * s.stride + (size_t)piece * 16) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        S2 = rescore_i8_fold(S2, G);
        if (live && sub == 0) rescore_i8_finish_row(dst, row_base + row, sc, S2, mbits >= 0x7F800000u, out_scales, out_norms, counters);
    }
}

// in [n][dim] int8 and scales [n] (null: 1.0), rows row_base .. row_base + n -> the same object; a row is bad unless its
// scale is finite and >= 0 and its norm is < inf.
__global__ __launch_bounds__(256) void rescore_i8_copy_in_kernel(const int8_t* in, const float* scales, uint64_t n, uint64_t row_base,
                                                                 const uint32_t* inv, RescoreStore s, uint8_t* out_rows, float* out_scales,
                                                                 float* out_norms, unsigned long long* counters) {
    const uint32_t G = s.G, sub = threadIdx.x & (G - 1), grp = threadIdx.x >> s.log2G, groups = 256u >> s.log2G;
    for (uint64_t r0 = (uint64_t)blockIdx.x * groups; r0 < n; r0 += (uint64_t)gridDim.x * groups) {      // uniform
        const uint64_t row = r0 + grp;
        const bool live = row < n;
        const uint64_t dst = !live ? 0 : (inv ? (uint64_t)inv[row_base + row] : row_base + row);
        const uint8_t* x = reinterpret_cast<const uint8_t*>(in) + row * s.dim;      // (a row need not be aligned: byte loads)
        int S2 = 0;
        for (uint32_t piece = sub; piece < s.pieces; piece += G) {
            uint32_t o[4];
#pragma unroll
            for (uint32_t d = 0; d < 4; ++d) {
                o[d] = 0;
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e) {
                    const uint32_t c = piece * 16 + d * 4 + e;
                    o[d] |= ((live && c < s.dim) ? (uint32_t)x[c] : 0u) << (8 * e);
                }
                S2 = __builtin_amdgcn_sdot4((int)o[d], (int)o[d], S2, false);
            }
            if (live) *reinterpret_cast<uint4*>(out_rows + dst * s.stride + (size_t)piece * 16) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        S2 = rescore_i8_fold(S2, G);
        if (!live || sub != 0) continue;
        const float sc = scales ? scales[row] : 1.0f;
        rescore_i8_finish_row(dst, row_base + row, sc, S2, !(sc >= 0.0f && sc < __builtin_inff()), out_scales, out_norms, counters);
    }
}

// Enqueues rows-in for one uploaded chunk: `in` is float32 rows, or int8 rows with their scales (may be null).
inline void rescore_i8_rows_in(const void* in, bool in_i8, const float* scales, uint64_t n, uint64_t row_base, const uint32_t* inv,
                               const RescoreStore& s, uint8_t* out_rows, float* out_scales, float* out_norms, unsigned long long* counters,
                               hipStream_t st) {
    if (n == 0) return;
    const uint64_t groups = 256u >> s.log2G;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + groups - 1) / groups, 256u * 32u);
    if (in_i8)
        hipLaunchKernelGGL(rescore_i8_copy_in_kernel, dim3(grid), dim3(256), 0, st, static_cast<const int8_t*>(in), scales, n, row_base, inv, s,
                           out_rows, out_scales, out_norms, counters);
    else
        hipLaunchKernelGGL(rescore_i8_in_kernel, dim3(grid), dim3(256), 0, st, static_cast<const float*>(in), n, row_base, inv, s, out_rows,
                           out_scales, out_norms, counters);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
