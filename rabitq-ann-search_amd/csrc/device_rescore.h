// device_rescore.h — two-stage search (cph_rescore_vectors_create, cph_search_rescored*): the kernel that brings full-size
// rows into a resident object and the kernel that rescores a candidate row against them.
//
// The statement, the layout of a row and the shape of every sum are host_rescore.h's (rescore_layout): a stored row is P
// pieces of 16 bytes, G lanes share it, lane l takes the pieces l, l + G, ..., a xor butterfly folds the G partial sums.
// Every product and sum is its own instruction (__fmul_rn / __fadd_rn): no FMA.
//
// rescore_rows_in_kernel streams: one G-lane group per row, 256 / G rows per workgroup and step, grid-stride.  A lane
// reads the E coordinates of its pieces (4-byte loads: an input row need not be 16-byte aligned), converts them, writes
// the piece with one 16-byte store at the row's internal position (zeros behind dim_full) and squares what it stored;
// lane 0 of the group writes the norm and counts a bad row with ordinary vector atomics.
//
// rescore_rows_kernel runs ONE 256-thread workgroup per query (not a scan kernel per (query, candidate) plus a select
// kernel: the selection is a sort of at most 1,024 words, which one workgroup does in LDS, and a separate scan would
// write and re-read n x C scores and re-read the query per candidate instead of once per workgroup).  LDS:
//     w[P2]                 the sort words, P2 = the power of two >= max(C, 64): (sign-folded score << 32) | id
//     qv[padded]            the full query as float32, zeros behind dim_full: read from global memory once
//     c_id[C]               per row position: the internal id, kNoId for padding, an id beyond the object, or a repeat
//     tab_id[H], tab_pos[H] the first-position id table (device_wg_primitives.h): an id's slot keeps its lowest position
// The 256 / G groups take candidates group, group + 256 / G, ...; a group works on kRescoreUnroll candidates at a time
// with one accumulator each, so a lane has that many independent 16-byte row loads in flight per step (G = 64 at 2 KiB
// rows: 4 x 1 KiB per wave-instruction, 16 KiB per workgroup).  A lane whose candidate is no candidate loads nothing and
// adds zeros: the butterflies run in uniform control flow.  Lane 0 of the group turns the dot into the score and writes
// the sort word; wg_sort (device_wg_primitives.h) sorts them; thread t < k writes output slot t -- every slot is written.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buf.h"
#include "device_diverse.h"
#include "device_wg_primitives.h"
#include "host_rescore.h"

namespace cph {

constexpr uint32_t kRescoreThreads = kWgSortThreads;
constexpr uint32_t kRescoreUnroll = 4;

struct RescoreStore {
    const uint8_t* rows;                  // [n_ids][stride]
    const float* norms;                   // [n_ids]
    uint32_t n_ids, dim;
    uint32_t stride, pieces, padded, G, log2G;
};

struct RescoreArgs {
    const int64_t* ids;                   // [n][C] candidate rows: internal ids, -1 = padding
    const float* dist;                    // [n][C]
    const float* fq;                      // [n][dim] full queries
    uint32_t C, k;                        // 1 <= k <= C <= kRescoreMaxCandidates
    RescoreStore s;
    int ip;                               // 0: "l2", 1: "ip"
    const uint32_t* rows;                 // [n_ids] row map, or null: ids are written as they are
    int64_t* out_ids;                     // [n][k]
    float* out_score;                     // [n][k]
    float* out_first;                     // [n][k]
};

inline size_t rescore_lds_bytes(uint32_t C, uint32_t padded) {
    return (size_t)wg_sort_len(C) * 8 + (size_t)padded * 4 + ((size_t)C + 2 * (size_t)diverse_table_slots(C)) * 4;   // at most 60 KiB
}

__device__ __forceinline__ float rescore_fold(float p, uint32_t G) {
    for (uint32_t d = G >> 1; d; d >>= 1) p = __fadd_rn(p, __shfl_xor(p, (int)d, 64));
    return p;
}

__device__ __forceinline__ float rescore_half_lo(uint32_t w) { return __half2float(__ushort_as_half((unsigned short)(w & 0xFFFFu))); }
__device__ __forceinline__ float rescore_half_hi(uint32_t w) { return __half2float(__ushort_as_half((unsigned short)(w >> 16))); }

// p + the E products of one 16-byte piece x with the query coordinates at q, in ascending coordinate order.
template <bool kF32>
__device__ __forceinline__ float rescore_piece(float p, const uint4& x, const float* q) {
    const float4 q0 = *reinterpret_cast<const float4*>(q);
    if (kF32) {
        p = __fadd_rn(p, __fmul_rn(q0.x, __uint_as_float(x.x)));
        p = __fadd_rn(p, __fmul_rn(q0.y, __uint_as_float(x.y)));
        p = __fadd_rn(p, __fmul_rn(q0.z, __uint_as_float(x.z)));
        p = __fadd_rn(p, __fmul_rn(q0.w, __uint_as_float(x.w)));
    } else {
        const float4 q1 = *reinterpret_cast<const float4*>(q + 4);
        p = __fadd_rn(p, __fmul_rn(q0.x, rescore_half_lo(x.x)));
        p = __fadd_rn(p, __fmul_rn(q0.y, rescore_half_hi(x.x)));
        p = __fadd_rn(p, __fmul_rn(q0.z, rescore_half_lo(x.y)));
        p = __fadd_rn(p, __fmul_rn(q0.w, rescore_half_hi(x.y)));
        p = __fadd_rn(p, __fmul_rn(q1.x, rescore_half_lo(x.z)));
        p = __fadd_rn(p, __fmul_rn(q1.y, rescore_half_hi(x.z)));
        p = __fadd_rn(p, __fmul_rn(q1.z, rescore_half_lo(x.w)));
        p = __fadd_rn(p, __fmul_rn(q1.w, rescore_half_hi(x.w)));
    }
    return p;
}

// Grid n, kRescoreThreads threads; LDS: rescore_lds_bytes(C, s.padded).
template <bool kF32>
__global__ __launch_bounds__(kRescoreThreads) void rescore_rows_kernel(RescoreArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr uint32_t E = kF32 ? 4u : 8u;
    const uint32_t C = a.C, k = a.k, P2 = wg_sort_len(C), H = diverse_table_slots(C);
    const uint32_t G = a.s.G, pieces = a.s.pieces, padded = a.s.padded;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(smem);
    float* qv = reinterpret_cast<float*>(w + P2);
    uint32_t* c_id = reinterpret_cast<uint32_t*>(qv + padded);
    uint32_t* tab_id = c_id + C;
    uint32_t* tab_pos = tab_id + H;
    const uint32_t tid = threadIdx.x, sub = tid & (G - 1), grp = tid >> a.s.log2G, groups = kRescoreThreads >> a.s.log2G;
    const size_t q = blockIdx.x;
    const int64_t* __restrict__ row_ids = a.ids + q * C;
    const uint32_t* __restrict__ row_dist = reinterpret_cast<const uint32_t*>(a.dist) + q * C;
    const float* __restrict__ fq = a.fq + q * a.s.dim;

    for (uint32_t i = tid; i < padded; i += kRescoreThreads) qv[i] = i < a.s.dim ? fq[i] : 0.0f;
    for (uint32_t s = tid; s < H; s += kRescoreThreads) id_table_clear(tab_id, tab_pos, s);
    for (uint32_t j = tid; j < P2; j += kRescoreThreads) w[j] = kSortNone;
    __syncthreads();
    // the candidates: an id's first position in the row
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
    __syncthreads();

    float qn = 0.0f;
    for (uint32_t piece = sub; piece < pieces; piece += G)
        for (uint32_t e = 0; e < E; ++e) {
            const float v = qv[piece * E + e];
            qn = __fadd_rn(qn, __fmul_rn(v, v));
        }
    qn = rescore_fold(qn, G);
    const bool q_ok = qn < __builtin_inff();              // (the same in every thread)

    for (uint32_t base = 0; base < C; base += groups * kRescoreUnroll) {      // uniform: every thread takes every step
        uint32_t id[kRescoreUnroll];
        const uint4* xr[kRescoreUnroll];
        float p[kRescoreUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kRescoreUnroll; ++u) {
            const uint32_t j = base + u * groups + grp;
            id[u] = (q_ok && j < C) ? c_id[j] : kNoId;
            xr[u] = reinterpret_cast<const uint4*>(a.s.rows + (size_t)(id[u] == kNoId ? 0u : id[u]) * a.s.stride);
            p[u] = 0.0f;
        }
        for (uint32_t piece = sub; piece < pieces; piece += G) {
            uint4 x[kRescoreUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kRescoreUnroll; ++u) x[u] = id[u] != kNoId ? xr[u][piece] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (uint32_t u = 0; u < kRescoreUnroll; ++u) p[u] = rescore_piece<kF32>(p[u], x[u], qv + piece * E);
        }
#pragma unroll
        for (uint32_t u = 0; u < kRescoreUnroll; ++u) p[u] = rescore_fold(p[u], G);
#pragma unroll
        for (uint32_t u = 0; u < kRescoreUnroll; ++u) {
            const float dot = p[u];
            if (sub != 0 || id[u] == kNoId) continue;
            float score;
            if (a.ip) {
                score = -dot;
            } else {
                const float v = __fsub_rn(__fadd_rn(qn, a.s.norms[id[u]]), __fmul_rn(2.0f, dot));
                score = (v < 0.0f) ? 0.0f : v;
            }
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
inline void rescore_rows(const RescoreArgs& a, bool f32, uint32_t n, hipStream_t st) {
    const size_t lds = rescore_lds_bytes(a.C, a.s.padded);
    if (f32) hipLaunchKernelGGL(rescore_rows_kernel<true>, dim3(n), dim3(kRescoreThreads), lds, st, a);
    else hipLaunchKernelGGL(rescore_rows_kernel<false>, dim3(n), dim3(kRescoreThreads), lds, st, a);
    HIP_CHECK(hipGetLastError());
}

// in [n][dim] (rows row_base .. row_base + n of the caller's array) -> the object's rows and norms at dst = inv ?
// inv[row] : row; counters = {bad rows, the lowest bad row}.
template <bool kF32>
__global__ __launch_bounds__(256) void rescore_rows_in_kernel(const float* in, uint64_t n, uint64_t row_base, const uint32_t* inv,
                                                              RescoreStore s, uint8_t* out_rows, float* out_norms,
                                                              unsigned long long* counters) {
    constexpr uint32_t E = kF32 ? 4u : 8u;
    const uint32_t G = s.G, sub = threadIdx.x & (G - 1), grp = threadIdx.x >> s.log2G, groups = 256u >> s.log2G;
    for (uint64_t r0 = (uint64_t)blockIdx.x * groups; r0 < n; r0 += (uint64_t)gridDim.x * groups) {      // uniform
        const uint64_t row = r0 + grp;
        const bool live = row < n;
        const uint64_t dst = !live ? 0 : (inv ? (uint64_t)inv[row_base + row] : row_base + row);
        const float* x = in + row * s.dim;
        float p = 0.0f;
        for (uint32_t piece = sub; piece < s.pieces; piece += G) {
            float v[E];
#pragma unroll
            for (uint32_t e = 0; e < E; ++e) v[e] = (live && piece * E + e < s.dim) ? x[piece * E + e] : 0.0f;
            uint4 o;
            if constexpr (kF32) {
                o = make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
            } else {
                uint32_t h[E];
#pragma unroll
                for (uint32_t e = 0; e < E; ++e) {
                    const __half hv = __float2half_rn(v[e]);
                    h[e] = __half_as_ushort(hv);
                    v[e] = __half2float(hv);                  // the norm is that of the stored values
                }
                o = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
            }
#pragma unroll
            for (uint32_t e = 0; e < E; ++e) p = __fadd_rn(p, __fmul_rn(v[e], v[e]));
            if (live) *reinterpret_cast<uint4*>(out_rows + dst * s.stride + (size_t)piece * 16) = o;
        }
        const float xn = rescore_fold(p, G);
        if (!live || sub != 0) continue;
        out_norms[dst] = xn;
        if (!(xn < __builtin_inff())) {
            atomicAdd(counters, 1ull);
            atomicMin(counters + 1, (unsigned long long)(row_base + row));
        }
    }
}

// Enqueues rows-in for one uploaded chunk.
inline void rescore_rows_in(const float* in, uint64_t n, uint64_t row_base, const uint32_t* inv, const RescoreStore& s, bool f32,
                            uint8_t* out_rows, float* out_norms, unsigned long long* counters, hipStream_t st) {
    if (n == 0) return;
    const uint64_t groups = 256u >> s.log2G;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + groups - 1) / groups, 256u * 32u);
    if (f32) hipLaunchKernelGGL(rescore_rows_in_kernel<true>, dim3(grid), dim3(256), 0, st, in, n, row_base, inv, s, out_rows, out_norms, counters);
    else hipLaunchKernelGGL(rescore_rows_in_kernel<false>, dim3(grid), dim3(256), 0, st, in, n, row_base, inv, s, out_rows, out_norms, counters);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
