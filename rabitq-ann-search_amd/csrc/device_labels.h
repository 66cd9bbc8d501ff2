// device_labels.h — label filters (cph_filters_from_labels): m allowed-id bitmaps from the handle's label column in one
// pass.  Filter j allows the ids whose label x satisfies lo[j] <= x <= hi[j] (signed, inclusive; lo > hi: nothing).
//
// One wave owns a tile of kLabelTile = 2,048 consecutive ids = 64 bitmap words per filter, and lane l owns word l of
// the tile: the 32 consecutive ids 32 l .. 32 l + 31.  It loads their labels ONCE, as eight 16 B loads of its own 128 B
// line (a wave's eight load instructions together read the tile's 8 KiB, every byte used; a load touches 64 lines, the
// other seven hit them in L1 -- paid once per tile and chunk, not per filter), then walks the filters of its chunk
// (blockIdx.y: kLabelFilterChunk filters, so a small index with many filters still fills the device).  lo[j] and hi[j]
// are wave-uniform loads; a lane builds its word in registers with one unsigned range test per id, (x - lo) <= (hi - lo),
// and the 64 words leave as one coalesced 256 B store to words[j][tile * 64 + lane].  No ballot and no cross-lane step:
// a ballot's result is a scalar, and the compiler offers no way to drop 32 scalars into 64 lanes that does not cost
// more than the range tests themselves.  Every word below (n + 31) / 32 is written, zeros included, and a lane clears
// the bits of its word at ids >= n: the result does not depend on what the bitmaps held before.  The wave sums its
// popcounts (__shfl_xor) and adds them to counts[j] with one atomicAdd (counts zeroed by the launcher).
// The host statement is host_index.h: label_filters_host.
#pragma once
#include <hip/hip_runtime.h>

#include "device_buf.h"

namespace cph {

constexpr uint32_t kLabelTile = 2048;         // ids per wave: 32 per lane, one bitmap word per lane and filter
constexpr uint32_t kLabelFilterChunk = 64;    // filters per blockIdx.y: the label column is read once per chunk
constexpr uint32_t kLabelBlock = 256;         // threads per block: 4 waves, 4 tiles
constexpr uint32_t kLabelMaxFilters = 65535u * kLabelFilterChunk;   // filters per call: one launch, grid.y <= 65,535

// labels: [n], 16 B aligned; lo / hi: [m]; words: m bitmaps, filter j at words + j * stride (stride >= (n + 31) / 32
// words); counts: [m].
__global__ __launch_bounds__(kLabelBlock) void label_filters_kernel(const int32_t* __restrict__ labels, uint64_t n,
                                                                    const int32_t* __restrict__ lo, const int32_t* __restrict__ hi,
                                                                    uint32_t m, uint32_t* __restrict__ words,
                                                                    uint64_t stride, unsigned long long* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = (uint64_t)blockIdx.x * (kLabelBlock / 64) + (threadIdx.x >> 6);
    if (tile * kLabelTile >= n) return;                    // (wave-uniform; the kernel has no barrier)
    const uint64_t nw = (n + 31) / 32, w = tile * 64 + lane, id0 = w * 32;
    int32_t lab[32];
    uint32_t keep;                                         // the bits of this lane's word that are ids below n
    if (id0 + 32 <= n) {
        keep = 0xFFFFFFFFu;
        const int4* src = reinterpret_cast<const int4*>(labels + id0);
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            const int4 v = src[q];
            lab[4 * q] = v.x; lab[4 * q + 1] = v.y; lab[4 * q + 2] = v.z; lab[4 * q + 3] = v.w;
        }
    } else {                                               // the last word of the index, and the lanes behind it
        keep = id0 < n ? (1u << (uint32_t)(n - id0)) - 1u : 0u;
#pragma unroll
        for (uint32_t t = 0; t < 32; ++t) lab[t] = id0 + t < n ? labels[id0 + t] : 0;
    }
    const uint64_t j0 = (uint64_t)blockIdx.y * kLabelFilterChunk;
    const uint64_t j1 = j0 + kLabelFilterChunk < m ? j0 + kLabelFilterChunk : m;
    for (uint64_t j = j0; j < j1; ++j) {
        const int32_t a = lo[j], b = hi[j];
        const uint32_t span = (uint32_t)b - (uint32_t)a;   // a <= x <= b  <=>  (x - a) mod 2^32 <= span, for a <= b
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t t = 0; t < 32; ++t) mine |= ((uint32_t)lab[t] - (uint32_t)a <= span ? 1u : 0u) << t;
        mine = a <= b ? mine & keep : 0u;
        if (w < nw) words[j * stride + w] = mine;
        uint32_t c = (uint32_t)__popc(mine);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
        if (lane == 0 && c) atomicAdd(&counts[j], (unsigned long long)c);
    }
}

// Enqueues the pass on `st` (counts zeroed first); every pointer lives on the current device.  1 <= m <= kLabelMaxFilters.
inline void label_filters(const int32_t* d_labels, uint64_t n, const int32_t* d_lo, const int32_t* d_hi, uint32_t m,
                          uint32_t* d_words, uint64_t stride, unsigned long long* d_counts, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)m * 8, st));
    if (n == 0) return;
    const uint64_t tiles = (n + kLabelTile - 1) / kLabelTile, per_block = kLabelBlock / 64;
    const uint32_t gx = (uint32_t)((tiles + per_block - 1) / per_block);
    const uint32_t gy = (m + kLabelFilterChunk - 1) / kLabelFilterChunk;
    hipLaunchKernelGGL(label_filters_kernel, dim3(gx, gy), dim3(kLabelBlock), 0, st, d_labels, n, d_lo, d_hi, m, d_words, stride,
                       d_counts);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
