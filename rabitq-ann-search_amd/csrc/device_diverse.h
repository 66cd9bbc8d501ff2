// device_diverse.h — diversified search (cph_search_diverse*): MMR re-ranking of a candidate row.
//
// The statement is host_diverse.h's.  diverse_rows_kernel runs one 256-thread workgroup per query:
//     c_id[C], c_r[C], c_m[C]   per row position: the internal id (kNoId: padding, a repeat, or picked already), the
//                               relevance bits, the smallest pair distance to a pick so far
//     tab_id[H], tab_pos[H]     the first-position id table (device_wg_primitives.h): an id's slot keeps the lowest
//                               position it occurs at, so the candidates are the entries that sit at their id's position
//     qv[D]                     the stored row of the last pick
// A pick loads its row into qv; every 8-lane group computes qnorm with the chains of the search kernel's query_norm_sq and
// then takes the positions group, group + 32, ...: lane c of the group runs chain c of group_dot8 against the candidate's
// row in HBM (32 candidates per step of the workgroup), lane 0 of the group folds the distance into c_m and keeps the best
// (score, position) it has seen.  The argmin is a wave reduction over (score, position) and one LDS step over the four
// waves.  The scores of all unpicked candidates are recomputed in every pass, no lazy evaluation.
// A pass reads every candidate's row from global memory: C x D x 4 bytes, k - 1 times, served by L2 after the first pass.
// Keeping the rows of a short candidate row in LDS instead (C = 64 at D = 128: 34 KiB with a conflict-free stride) was
// built and measured: the kernel took 467 us instead of 248 us for 10,000 rows (profiles/diverse_search.md), so it is not
// done.
// Every output slot is written here: picks as they are taken, the rest as padding at the end.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buf.h"
#include "device_fastscan.h"
#include "device_wg_primitives.h"
#include "host_diverse.h"

namespace cph {

struct DiverseArgs {
    const int64_t* ids;                   // [n][C] candidate rows: internal ids, -1 = padding
    const float* dist;                    // [n][C]
    uint32_t C, k;                        // 1 <= k <= C <= kDiverseMaxCandidates
    float a, b;                           // lam and 1 - lam, rounded once on the host
    const float* raw;                     // [n_ids][D] stored rows, zero-padded
    const float* norm_sq;                 // [n_ids]
    uint32_t n_ids, D;                    // ids at or above n_ids are treated as padding (no search returns one)
    const uint32_t* rows;                 // [n_ids] row map, or null: ids are written as they are
    int64_t* out_ids;                     // [n][k]
    float* out_dist;                      // [n][k]
    float* out_gap;                       // [n][k]
};

constexpr uint32_t kDiverseThreads = 256;
inline size_t diverse_lds_bytes(uint32_t C, uint32_t D) {
    return ((size_t)D + 3 * (size_t)C + 2 * (size_t)diverse_table_slots(C) + 2 * (kDiverseThreads / 64)) * 4;   // at most 37 KiB
}

// (score, position) order of the statement: the smaller score, then the lower position; position kNoId = nothing.
__device__ __forceinline__ bool diverse_better(float s1, uint32_t p1, float s2, uint32_t p2) {
    if (p1 == kNoId) return false;
    if (p2 == kNoId) return true;
    return s1 < s2 || (s1 == s2 && p1 < p2);
}

// Grid n, kDiverseThreads threads; LDS: diverse_lds_bytes(C, D).
__global__ __launch_bounds__(kDiverseThreads) void diverse_rows_kernel(DiverseArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t C = a.C, k = a.k, D = a.D, H = diverse_table_slots(C);
    float* qv = reinterpret_cast<float*>(smem);
    uint32_t* c_id = reinterpret_cast<uint32_t*>(qv + D);
    uint32_t* c_r = c_id + C;
    float* c_m = reinterpret_cast<float*>(c_r + C);
    uint32_t* tab_id = reinterpret_cast<uint32_t*>(c_m + C);
    uint32_t* tab_pos = tab_id + H;
    float* w_score = reinterpret_cast<float*>(tab_pos + H);
    uint32_t* w_pos = reinterpret_cast<uint32_t*>(w_score + kDiverseThreads / 64);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = tid >> 3, chain = tid & 7;
    const size_t q = blockIdx.x;
    const int64_t* __restrict__ row_ids = a.ids + q * C;
    const uint32_t* __restrict__ row_dist = reinterpret_cast<const uint32_t*>(a.dist) + q * C;
    int64_t* __restrict__ out_ids = a.out_ids + q * k;
    uint32_t* __restrict__ out_dist = reinterpret_cast<uint32_t*>(a.out_dist) + q * k;
    uint32_t* __restrict__ out_gap = reinterpret_cast<uint32_t*>(a.out_gap) + q * k;

    // the candidates: an id's first position in the row.  (device_wg_primitives.h's table, written out: with its functions
    // inlined here the compiler swaps two instructions of the pick loop, and this kernel's instruction stream is pinned.)
    for (uint32_t s = tid; s < H; s += kDiverseThreads) {
        tab_id[s] = kNoId;
        tab_pos[s] = kNoId;
    }
    __syncthreads();
    for (uint32_t j = tid; j < C; j += kDiverseThreads) {
        const int64_t id64 = row_ids[j];
        const bool valid = id64 >= 0 && (unsigned long long)id64 < a.n_ids;
        const uint32_t id = valid ? (uint32_t)id64 : kNoId;
        c_id[j] = id;
        c_r[j] = row_dist[j];
        c_m[j] = 3.402823466e+38f;
        if (valid) {
            uint32_t s = (id * 2654435761u) & (H - 1);
            for (;;) {                                    // (the table has at least C free slots: the probe ends)
                const uint32_t old = atomicCAS(&tab_id[s], kNoId, id);
                if (old == kNoId || old == id) break;
                s = (s + 1) & (H - 1);
            }
            atomicMin(&tab_pos[s], j);
        }
    }
    __syncthreads();
    for (uint32_t j = tid; j < C; j += kDiverseThreads) {
        const uint32_t id = c_id[j];
        if (id == kNoId) continue;
        uint32_t s = (id * 2654435761u) & (H - 1);
        while (tab_id[s] != id) s = (s + 1) & (H - 1);
        if (tab_pos[s] != j) c_id[j] = kNoId;             // a repeat
    }
    __syncthreads();

    uint32_t t = 0;
    for (; t < k; ++t) {
        // my best (score, position): pick 0 takes the first candidate, later picks the scores of the pass below
        float my_s = 0.0f;
        uint32_t my_p = kNoId;
        if (t == 0) {
            for (uint32_t j = tid; j < C; j += kDiverseThreads)
                if (c_id[j] != kNoId && my_p == kNoId) my_p = j;
        } else {
            float c = 0.0f;
            for (uint32_t i = chain; i < D; i += 8) c = __fmaf_rn(qv[i], qv[i], c);
            const float qnorm = group_reduce8(c);
            for (uint32_t base = 0; base < C; base += kDiverseThreads / 8) {
                const uint32_t j = base + grp;
                const uint32_t id = j < C ? c_id[j] : kNoId;
                if (id == kNoId) continue;                // (the eight lanes of a group leave together)
                const float dot = group_dot8(qv, a.raw + (size_t)id * D, D, (int)chain);
                const float d = exact_from_dot(qnorm, a.norm_sq[id], dot);
                if (chain == 0) {
                    float m = c_m[j];
                    if (d < m) {
                        m = d;
                        c_m[j] = d;
                    }
                    const float score = __fsub_rn(__fmul_rn(a.a, __uint_as_float(c_r[j])), __fmul_rn(a.b, m));
                    if (diverse_better(score, j, my_s, my_p)) {
                        my_s = score;
                        my_p = j;
                    }
                }
            }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(my_s, off);
            const uint32_t op = (uint32_t)__shfl_xor((int)my_p, off);
            if (diverse_better(os, op, my_s, my_p)) {
                my_s = os;
                my_p = op;
            }
        }
        if (lane == 0) {
            w_score[wave] = my_s;
            w_pos[wave] = my_p;
        }
        __syncthreads();                                  // (also: every c_m of the pass is written, qv is free)
        float best_s = w_score[0];
        uint32_t best_p = w_pos[0];
        for (uint32_t w = 1; w < kDiverseThreads / 64; ++w)
            if (diverse_better(w_score[w], w_pos[w], best_s, best_p)) {
                best_s = w_score[w];
                best_p = w_pos[w];
            }
        if (best_p == kNoId) break;                       // (uniform) the candidates ran out
        const uint32_t sid = c_id[best_p];
        if (t + 1 < k)
            for (uint32_t i = tid; i < D; i += kDiverseThreads) qv[i] = a.raw[(size_t)sid * D + i];
        __syncthreads();                                  // everyone has read c_id[best_p], w_score and w_pos
        if (tid == 0) {
            out_ids[t] = (int64_t)(a.rows ? a.rows[sid] : sid);
            out_dist[t] = c_r[best_p];
            out_gap[t] = __float_as_uint(c_m[best_p]);
            c_id[best_p] = kNoId;
        }
        __syncthreads();
    }
    for (uint32_t i = t + tid; i < k; i += kDiverseThreads) {
        out_ids[i] = -1;
        out_dist[i] = 0x7F7FFFFFu;                        // FLT_MAX
        out_gap[i] = 0x7F7FFFFFu;
    }
}

// Enqueues the pass over n rows (n >= 1).
inline void diverse_rows(const DiverseArgs& a, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(diverse_rows_kernel, dim3(n), dim3(kDiverseThreads), diverse_lds_bytes(a.C, a.D), st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
