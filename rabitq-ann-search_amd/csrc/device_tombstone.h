// device_tombstone.h — the bitmap kernels of cph_remove: a removed row is a tombstone, a bit in the handle's bitmap R
// of removed internal ids.  The search kernels never see R: every search of a handle with tombstones runs under the
// effective filter F & ~R (F: the caller's filter, or every id) through the filtered, exact and per-query paths as they
// are.  Three small kernels, all bandwidth-trivial (one bit per vertex: 128 KiB per million rows):
//
//   mark_ids_kernel     id list -> bitmap, one atomicOr per id (ids validated on the host: every id < n).  For ids in
//                       input rows the list marks a ROW bitmap, which rows_filter_kernel (device_rows.h) converts.
//   fold_removed_kernel R |= new, and counts the bits that were not set before.
//   live_filter_kernel  out = F & ~R (F null: ~R) and its popcount; the bits of the last word behind n stay clear,
//                       whatever the inputs hold there.
//
// The two counting kernels reduce inside the wave (__shfl_xor over 64 lanes), then inside the block through LDS, and
// issue ONE atomicAdd per block.  Thread t handles word t: coalesced, no loop.  The host statement of the third kernel
// is live_filter_host (cph_host_live_filter).
#pragma once
#include <hip/hip_runtime.h>

#include "device_buf.h"

namespace cph {

constexpr uint32_t kTombBlock = 256;          // threads per block: 256 words = 8,192 ids

__device__ __forceinline__ uint32_t tomb_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// Every thread of the block calls it (no early return before): adds the block's sum of v to *total with one atomic.
__device__ __forceinline__ void tomb_block_add(uint32_t v, unsigned long long* total) {
    __shared__ uint32_t part[kTombBlock / 64];
    v = tomb_wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < kTombBlock / 64; ++w) s += part[w];
        if (s) atomicAdd(total, (unsigned long long)s);
    }
}

// bitmap: (n + 31) / 32 words, zeroed by the caller; ids[m], every one < n.
__global__ __launch_bounds__(kTombBlock) void mark_ids_kernel(const uint32_t* __restrict__ ids, uint64_t m, uint64_t n,
                                                              uint32_t* __restrict__ bitmap) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t id = ids[i];
    if (id < n) atomicOr(&bitmap[id >> 5], 1u << (id & 31));      // (the host has checked: the guard keeps a bad list inside the bitmap)
}

// removed[w] |= fresh[w] for the nw words; *newly += bits of fresh that removed did not hold.
__global__ __launch_bounds__(kTombBlock) void fold_removed_kernel(uint32_t* __restrict__ removed, const uint32_t* __restrict__ fresh,
                                                                  uint64_t nw, unsigned long long* newly) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    if (w < nw) {
        const uint32_t old = removed[w], add = fresh[w] & ~old;
        if (add) removed[w] = old | add;
        c = (uint32_t)__popc(add);
    }
    tomb_block_add(c, newly);
}

// out[w] = (allow ? allow[w] : ~0) & ~removed[w], tail bits of the last word clear; *count += popcount(out).
__global__ __launch_bounds__(kTombBlock) void live_filter_kernel(const uint32_t* __restrict__ allow, const uint32_t* __restrict__ removed,
                                                                 uint64_t n, uint64_t nw, uint32_t* __restrict__ out,
                                                                 unsigned long long* count) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    if (w < nw) {
        uint32_t x = (allow ? allow[w] : 0xFFFFFFFFu) & ~removed[w];
        if (w == nw - 1 && (n & 31)) x &= (1u << (n & 31)) - 1u;
        out[w] = x;
        c = (uint32_t)__popc(x);
    }
    tomb_block_add(c, count);
}

inline uint32_t tomb_grid(uint64_t items) { return (uint32_t)((items + kTombBlock - 1) / kTombBlock); }

// All three enqueue on `st`; every pointer lives on the current device.  The counters are zeroed here.
inline void mark_ids(const uint32_t* d_ids, uint64_t m, uint64_t n, uint32_t* d_bitmap, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(d_bitmap, 0, ((n + 31) / 32) * 4, st));
    if (m == 0) return;
    hipLaunchKernelGGL(mark_ids_kernel, dim3(tomb_grid(m)), dim3(kTombBlock), 0, st, d_ids, m, n, d_bitmap);
    HIP_CHECK(hipGetLastError());
}

inline void fold_removed(uint32_t* d_removed, const uint32_t* d_fresh, uint64_t n, unsigned long long* d_newly, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(d_newly, 0, 8, st));
    if (n == 0) return;
    const uint64_t nw = (n + 31) / 32;
    hipLaunchKernelGGL(fold_removed_kernel, dim3(tomb_grid(nw)), dim3(kTombBlock), 0, st, d_removed, d_fresh, nw, d_newly);
    HIP_CHECK(hipGetLastError());
}

inline void live_filter(const uint32_t* d_allow, const uint32_t* d_removed, uint64_t n, uint32_t* d_out, unsigned long long* d_count,
                        hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(d_count, 0, 8, st));
    if (n == 0) return;
    const uint64_t nw = (n + 31) / 32;
    hipLaunchKernelGGL(live_filter_kernel, dim3(tomb_grid(nw)), dim3(kTombBlock), 0, st, d_allow, d_removed, n, nw, d_out, d_count);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
