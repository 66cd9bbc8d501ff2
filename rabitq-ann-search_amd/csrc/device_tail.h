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
//   tail_scan_kernel    the scan of device_exact.h (exact_scan_candidates into the top-k pools of ExactPoolSink) over the
//                       candidates n_b .. n_b + t - 1.  Only the candidate source is the tail's own: it tests the allowed
//                       bit of the effective filter, once per 64 candidates, so no id list per filter is made and no
//                       count comes to the host.  Parts over t come from plan_exact.
//   tail_fold_kernel    one wave per query: folds the query's P sorted tail lists in LDS (exact_fold_parts, the fold of
//                       exact_merge_query), stages the graph's row, places every entry at its rank in the stable merge (graph
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
    ScanCommon s;                 // (raw, norm_sq: [n_b + t] rows)
    const uint32_t* allow;        // the effective filter's bitmap over all ids, or null: every id
    uint32_t base, t;             // tail candidate c is id base + c
    uint32_t k, C;                // as in ExactArgs
    unsigned long long* pools;    // [P][q_count][C]
    uint32_t* counts;             // [P][q_count]
};

// The tail's candidate source: candidate c is id base + c, allowed where the effective filter's bit is set.
struct TailSource {
    const uint32_t* allow;
    uint32_t base;
    __device__ __forceinline__ uint32_t id(uint32_t c) const { return base + c; }
    __device__ __forceinline__ bool allowed(uint32_t id) const { return allow == nullptr || ((allow[id >> 5] >> (id & 31)) & 1u); }
};

// Grid (P, G), one wave per workgroup; LDS: C keys + 2 gq words -- the geometry of exact_scan_kernel.
template <int SD, int CH>
__global__ __launch_bounds__(64) void tail_scan_kernel(TailScanArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    const ScanCut c = scan_cut(a.s, a.t, D);
    if (c.c_lo >= c.c_hi || c.ql_lo >= c.ql_hi) return;
    const size_t pool = (size_t)blockIdx.x * a.s.q_count + c.ql_lo;
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, TailSource{a.allow, a.base}, c.c_lo, c.c_hi, c.q_rows, c.q_norms,
                                  c.ql_hi - c.ql_lo, ExactPoolSink(smem, a.s.gq, a.pools + pool * a.C, a.counts + pool, a.k, a.C));
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
    const uint32_t k = a.k;
    const size_t qi = (size_t)a.q_first + blockIdx.x, o = qi * k;
    // the tail's top-k: sm[0 .. tn) ascending
    uint32_t tn = exact_fold_parts(sm, a.pools, a.counts, blockIdx.x, a.q_count, a.P, a.C, lane);
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
