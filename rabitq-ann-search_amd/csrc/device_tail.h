// device_tail.h — rows added to a finalized index (cph_add): the TAIL, a flat segment of fp32 rows behind the graph's.
//
// The graph, its blocks, the encoder and the search kernel never hear of it.  Tail row j lives at index n_b + j of the
// resident vector / norm / row-map / label arrays (n_b: the rows of the graph), so raw + id * D is valid for every id
// below the size and the exact paths (device_exact.h, device_range.h, the hooks) see the tail as more candidates.  A
// graph-routed batch is the unchanged graph launch over the base rows plus an exact scan of the tail, folded into the
// graph's rows.  Three kernels:
//
//   tail_append_kernel  the device pass of cph_add over m new rows: zero-pads each to D, writes its norm with the
//                       arithmetic of the builder's row_norms_kernel (ONE fmaf chain over the first dim elements, so a
//                       tail row has the norm bits the same floats would get from a build), extends the row map by the
//                       identity, the label column by the given labels and the removed bitmap by clear bits.
//   tail_scan_kernel    the scan of device_exact.h (its chains, its tree, exact_from_dot, query values through scalar
//                       loads, the pool / threshold / compaction selection) over the candidates n_b .. n_b + t - 1, with
//                       the allowed bit of the effective filter tested where `pass` is formed: no id list per filter is
//                       made and no count comes to the host.  A body of its own next to exact_scan_work, so that the
//                       exact instantiations keep the code they had; the helpers are shared.  Parts over t come from
//                       plan_exact.
//   tail_fold_kernel    one wave per query: folds the query's P sorted tail lists in LDS (exact_merge_query's bitonic
//                       merges), stages the graph's row, places every entry at its rank in the stable merge (graph
//                       entry first where the float values are equal -- merge_parts_kernel's rule) and writes the
//                       first k over the graph's row.  The whole row is in LDS before the first store, so it folds in
//                       place, also rows that live in pinned host memory (small batches).
//
// The host statements (tail_fold_host, tail_capacity) are in host_tail.h.
#pragma once
#include <hip/hip_runtime.h>

#include "device_buf.h"
#include "device_exact.h"
#include "device_merge.h"
#include "host_tail.h"

namespace cph {

// ---- cph_add ------------------------------------------------------------------------------------------------------------
struct TailAppendArgs {
    const float* src;             // [m][dim] the new rows
    const int32_t* src_labels;    // [m], or null: the handle has no label column
    uint64_t first, m;            // the new rows get ids first .. first + m - 1
    uint32_t dim, D;
    float* raw;                   // [>= first + m][D]
    float* norm_sq;               // [>= first + m]
    uint32_t* rows;               // row map, or null: the handle has none
    int32_t* labels;              // label column (with src_labels)
    uint32_t* removed;            // removed bitmap, or null: nothing is removed
};

__global__ __launch_bounds__(256) void tail_append_kernel(TailAppendArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t e = t0; e < a.m * a.D; e += stride) {
        const uint64_t r = e / a.D;
        const uint32_t d = (uint32_t)(e % a.D);
        a.raw[(a.first + r) * a.D + d] = d < a.dim ? a.src[r * a.dim + d] : 0.0f;
    }
    for (uint64_t r = t0; r < a.m; r += stride) {
        const float* v = a.src + r * a.dim;
        float s = 0.0f;
        for (uint32_t j = 0; j < a.dim; ++j) s = __fmaf_rn(v[j], v[j], s);
        const uint64_t id = a.first + r;
        a.norm_sq[id] = s;
        if (a.rows) a.rows[id] = (uint32_t)id;
        if (a.labels) a.labels[id] = a.src_labels[r];
        if (a.removed) atomicAnd(&a.removed[id >> 5], ~(1u << (id & 31)));
    }
}

inline void tail_append(const TailAppendArgs& a, hipStream_t st) {
    if (a.m == 0) return;
    const uint64_t blocks = (a.m * a.D + 255) / 256;
    hipLaunchKernelGGL(tail_append_kernel, dim3((uint32_t)std::min<uint64_t>(blocks, 1u << 16)), dim3(256), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

// ---- the scan -------------------------------------------------------------------------------------------------------------
struct TailScanArgs {
    const float* raw;             // [n_b + t][D]
    const float* norm_sq;         // [n_b + t]
    const uint32_t* allow;        // the effective filter's bitmap over all ids, or null: every id
    uint32_t base, t;             // tail candidate c is id base + c
    uint32_t D;
    const float* qpad;            // [nq_pad][D]
    const float* qnorm;           // [nq_pad]
    uint32_t q_first, q_count;    // the queries of this launch
    uint32_t gq, part, k, C;      // as in ExactArgs
    unsigned long long* pools;    // [P][q_count][C]
    uint32_t* counts;             // [P][q_count]
};

// Grid (P, G), one wave per workgroup; LDS: C keys + 2 gq words -- the geometry of exact_scan_kernel.
template <int SD, int CH>
__global__ __launch_bounds__(64) void tail_scan_kernel(TailScanArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t D = SD ? (uint32_t)SD : a.D;
    const uint32_t p = blockIdx.x;
    const uint32_t c_lo = p * a.part, c_hi = min(a.t, c_lo + a.part);
    const uint32_t ql_lo = blockIdx.y * a.gq, ql_hi = min(a.q_count, ql_lo + a.gq);   // relative to q_first
    if (c_lo >= c_hi || ql_lo >= ql_hi) return;
    const uint32_t nqg = ql_hi - ql_lo, gq = a.gq, k = a.k, C = a.C;
    const size_t pool0 = (size_t)p * a.q_count + ql_lo;
    unsigned long long* const pools = a.pools + pool0 * C;
    uint32_t* const counts = a.counts + pool0;
    const exact_uniform_ptr qbase = (exact_uniform_ptr)(a.qpad + (size_t)(a.q_first + ql_lo) * D);
    const exact_uniform_ptr qnorms = (exact_uniform_ptr)(a.qnorm + a.q_first + ql_lo);

    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    uint32_t* s_thr = reinterpret_cast<uint32_t*>(sm + C);
    uint32_t* s_cnt = s_thr + gq;
    const int lane = threadIdx.x;
    for (uint32_t i = lane; i < gq; i += 64) { s_thr[i] = 0xFFFFFFFFu; s_cnt[i] = 0; }
    __syncthreads();

    for (uint32_t cb = c_lo; cb < c_hi; cb += 64) {
        const bool valid = cb + lane < c_hi;
        const uint32_t id = a.base + (valid ? cb + lane : c_hi - 1);
        const bool allowed = valid && (a.allow == nullptr || ((a.allow[id >> 5] >> (id & 31)) & 1u));
        const float* __restrict__ row = a.raw + (size_t)id * D;
        const float nrm = a.norm_sq[id];
        float v[CH];
        if constexpr (SD == CH) exact_load_chunk<CH>(row, v);
        for (uint32_t qt = 0; qt < nqg; qt += kExactQT) {
            float acc[kExactQT][8];
#pragma unroll
            for (int t = 0; t < kExactQT; ++t)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[t][j] = 0.0f;
            if constexpr (SD == CH) {
                exact_fma_chunk<CH>(v, qbase + (size_t)qt * D, D, acc);
            } else {
#pragma unroll 2
                for (uint32_t b = 0; b < D; b += CH) {
                    exact_load_chunk<CH>(row + b, v);
                    exact_fma_chunk<CH>(v, qbase + (size_t)qt * D + b, D, acc);
                }
            }
#pragma unroll
            for (int t = 0; t < kExactQT; ++t) {
                const uint32_t ql = qt + t;                        // index inside the group
                if (ql >= nqg) break;                              // (wave-uniform)
                const float dot = ((acc[t][0] + acc[t][4]) + (acc[t][1] + acc[t][5])) + ((acc[t][2] + acc[t][6]) + (acc[t][3] + acc[t][7]));
                const uint32_t dbits = __float_as_uint(exact_from_dot(qnorms[ql], nrm, dot));
                const bool pass = allowed && dbits <= s_thr[ql];
                const unsigned long long mask = __ballot(pass);
                if (mask == 0) continue;
                unsigned long long* pool = pools + (size_t)ql * C;
                uint32_t cnt = s_cnt[ql];
                const uint32_t add = (uint32_t)__popcll(mask);
                if (cnt + add > C) {                               // (afterwards cnt <= k <= C - 64)
                    uint32_t thr;
                    cnt = exact_compact(sm, pool, cnt, k, lane, thr);
                    if (lane == 0) s_thr[ql] = thr;
                }
                if (pass) pool[cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = ((unsigned long long)dbits << 32) | id;
                if (lane == 0) s_cnt[ql] = cnt + add;
            }
        }
    }
    // every pool: sorted, cut to k
    for (uint32_t ql = 0; ql < nqg; ++ql) {
        uint32_t cnt = s_cnt[ql], thr;
        if (cnt) cnt = exact_compact(sm, pools + (size_t)ql * C, cnt, k, lane, thr);
        if (lane == 0) counts[ql] = cnt;
    }
}

inline void launch_tail_scan(uint32_t D, dim3 grid, size_t lds, hipStream_t st, const TailScanArgs& a) {
    if (D == 128) hipLaunchKernelGGL((tail_scan_kernel<128, 128>), grid, dim3(64), lds, st, a);
    else if (D == 1024) hipLaunchKernelGGL((tail_scan_kernel<1024, 64>), grid, dim3(64), lds, st, a);
    else hipLaunchKernelGGL((tail_scan_kernel<0, 16>), grid, dim3(64), lds, st, a);
    HIP_CHECK(hipGetLastError());
}

// ---- the fold -------------------------------------------------------------------------------------------------------------
struct TailFoldArgs {
    const unsigned long long* pools;   // [P][q_count][C]
    const uint32_t* counts;            // [P][q_count], every count <= k
    uint32_t P, q_first, q_count, k, C;
    int64_t* ids;                      // [nq][k] the graph's rows, folded in place
    float* dist;
    uint32_t* out_count;               // [nq] entries that are not padding, or null
    uint32_t* done_flags;              // as SearchArgs::done_flags (the graph launch of such a batch raises none), or null
    uint32_t done_seq;
};

inline size_t tail_fold_lds(uint32_t k, uint32_t C) { return (size_t)C * 8 + (size_t)k * 12; }

// One wave per query of the launch.  LDS: C keys | k graph ids | k graph distances.
__global__ __launch_bounds__(64) void tail_fold_kernel(TailFoldArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    int64_t* g_id = reinterpret_cast<int64_t*>(sm + a.C);
    float* g_d = reinterpret_cast<float*>(g_id + a.k);
    const int lane = threadIdx.x;
    const uint32_t k = a.k, C = a.C, Kp = C / 2;
    const size_t qi = (size_t)a.q_first + blockIdx.x, o = qi * k;
    // the tail's top-k: sm[0 .. Kp) ascending, behind the keys kExactNoKey
    for (uint32_t i = lane; i < Kp; i += 64) sm[i] = kExactNoKey;
    uint32_t tn = 0;
    for (uint32_t p = 0; p < a.P; ++p) {
        const size_t pi = (size_t)p * a.q_count + blockIdx.x;
        const uint32_t cnt = a.counts[pi];                          // <= k <= Kp
        const unsigned long long* pool = a.pools + pi * C;
        for (uint32_t i = lane; i < Kp; i += 64) sm[C - 1 - i] = i < cnt ? pool[i] : kExactNoKey;
        __syncthreads();
        exact_merge_keys(sm, C, lane);
        tn += cnt;
    }
    tn = tn < k ? tn : k;
    // the graph's row, all of it, before anything is stored
    uint32_t gn = 0;
    for (uint32_t i = lane; i < k; i += 64) {
        const int64_t id = a.ids[o + i];
        g_id[i] = id;
        g_d[i] = a.dist[o + i];
        gn += id >= 0 ? 1u : 0u;
    }
    gn = wave_sum_u32(gn);
    __syncthreads();
    // graph entry j: behind the tail entries that are smaller; tail entry j: behind the graph entries that are not larger
    for (uint32_t j = lane; j < k; j += 64) {
        const float d = g_d[j];
        uint32_t lo = 0, hi = tn;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (__uint_as_float((uint32_t)(sm[mid] >> 32)) < d) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t pos = j + lo;
        if (pos < k) {
            a.ids[o + pos] = g_id[j];
            a.dist[o + pos] = d;
        }
    }
    for (uint32_t j = lane; j < tn; j += 64) {
        const unsigned long long key = sm[j];
        const float d = __uint_as_float((uint32_t)(key >> 32));
        const uint32_t pos = j + merge_count_below(g_d, k, d, true);
        if (pos < k) {
            a.ids[o + pos] = (int64_t)(uint32_t)key;
            a.dist[o + pos] = d;
        }
    }
    if (a.out_count && lane == 0) a.out_count[qi] = gn + tn < k ? gn + tn : k;
    if (a.done_flags) {
        __threadfence_system();          // every lane's stores, and lane 0's count, before the flag
        if (lane == 0) __hip_atomic_store(&a.done_flags[qi], a.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

inline void tail_fold(const TailFoldArgs& a, hipStream_t st) {
    if (a.q_count == 0) return;
    hipLaunchKernelGGL(tail_fold_kernel, dim3(a.q_count), dim3(64), tail_fold_lds(a.k, a.C), st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
