// device_merge.h — the merge of a partitioned index (cph_parts_*): P result rows per query, one from every part, become
// the first k entries of their stable merge.
//
// Input: ids[P][n][k] (int64; -1 = padding) and dist[P][n][k] (f32; FLT_MAX = padding), every row ascending in distance,
// and lo[P], the first input row of every part.  Output row i = the first k entries of the stable merge of the P rows i
// in part order: ascending distance compared as float values, equal distances lower part first, inside a part the part's
// own order -- numpy: argsort(concatenate(rows), kind="stable")[:k].
//
// One wave per query row.  Candidate j of part p lands at
//     j + sum over p' != p of |{entries of part p' that are < d}|      (p' > p)
//                             |{entries of part p' that are <= d}|     (p' < p)
// which is one binary search per other part; the candidates of a row go over the lanes in passes of 64.  The rule is a
// permutation of 0..P*k-1 (it is the rank under the total order (distance, part, position)), so no two lanes write one slot
// and every slot below k is written exactly once.  A lane whose position is below k writes its id, with lo[p] added where
// the id is not padding, and its distance bytes.  Padding sorts last and stays padding.
//
// The binary searches read the distances of the row from LDS when the P rows fit the staging area (kMergeStageKeys
// floats), else straight from global memory: P * k is not limited by LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buf.h"

namespace cph {

constexpr uint32_t kMergeStageKeys = 4096;      // 16 KiB of LDS: P * k up to this many distances are staged

// Entries of the ascending row[0..k) that are < d (or_equal: <= d).
__device__ __forceinline__ uint32_t merge_count_below(const float* row, uint32_t k, float d, bool or_equal) {
    uint32_t lo = 0, hi = k;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const float v = row[mid];
        const bool below = or_equal ? (v <= d) : (v < d);
        if (below) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// part_stride = n * k: the distance between two parts' rows of one query.
template <bool kStaged>
__global__ __launch_bounds__(64) void merge_parts_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dist, uint32_t P,
                                                         uint32_t n, uint32_t k, const int64_t* __restrict__ lo,
                                                         int64_t* __restrict__ out_ids, float* __restrict__ out_dist) {
    extern __shared__ float merge_stage[];      // kStaged: [P][k]
    const uint32_t lane = threadIdx.x;
    const uint64_t part_stride = (uint64_t)n * k;
    const uint32_t total = P * k;               // P <= 16, k < 2^27 (checked by the launcher)
    for (uint32_t row = blockIdx.x; row < n; row += gridDim.x) {
        const float* g_row = dist + (uint64_t)row * k;              // part p's row: g_row + p * part_stride
        if (kStaged) {
            __syncthreads();                                        // the previous row's searches are done
            for (uint32_t c = lane; c < total; c += 64) merge_stage[c] = g_row[(uint64_t)(c / k) * part_stride + c % k];
            __syncthreads();
        }
        for (uint32_t c = lane; c < total; c += 64) {
            const uint32_t p = c / k, j = c % k;
            const float d = kStaged ? merge_stage[c] : g_row[(uint64_t)p * part_stride + j];
            uint32_t pos = j;
            for (uint32_t o = 0; o < P && pos < k; ++o) {
                if (o == p) continue;
                const float* other = kStaged ? merge_stage + o * k : g_row + (uint64_t)o * part_stride;
                pos += merge_count_below(other, k, d, o < p);
            }
            if (pos < k) {
                const int64_t id = ids[(uint64_t)p * part_stride + (uint64_t)row * k + j];
                out_ids[(uint64_t)row * k + pos] = id >= 0 ? id + lo[p] : id;
                out_dist[(uint64_t)row * k + pos] = d;
            }
        }
    }
}

// Enqueues the merge on `st`; every pointer lives on the current device.  1 <= P <= 16, n >= 1, 1 <= k, P * k < 2^31.
inline void merge_parts(const int64_t* d_ids, const float* d_dist, uint32_t P, uint32_t n, uint32_t k, const int64_t* d_lo,
                        int64_t* d_out_ids, float* d_out_dist, hipStream_t st) {
    const uint32_t grid = n < (1u << 20) ? n : (1u << 20);
    if ((uint64_t)P * k <= kMergeStageKeys)
        hipLaunchKernelGGL((merge_parts_kernel<true>), dim3(grid), dim3(64), (size_t)P * k * sizeof(float), st, d_ids, d_dist, P, n, k,
                           d_lo, d_out_ids, d_out_dist);
    else
        hipLaunchKernelGGL((merge_parts_kernel<false>), dim3(grid), dim3(64), 0, st, d_ids, d_dist, P, n, k, d_lo, d_out_ids,
                           d_out_dist);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
