// device_wg_primitives.h — what the re-rank kernels share inside one 256-thread workgroup: the bitonic sort of 64-bit words
// in LDS (maxsim, rescored maxsim, rescored and fused search) and the first-position id table (diverse and rescored search).
//
// Bank conflicts of the sort (cdna_hip_programming.md, LDS): a compare-exchange at distance j >= 64 reads and writes 64-bit
// words at consecutive addresses across each half wave (32 x 8 B = the 256-B bank row), conflict-free.  At j < 64 the same
// mapping would put the lanes l and l + 16 of a half wave on one bank (2-way), so those steps never touch LDS: every lane
// holds one element of a 64-element tile and exchanges it with lane ^ j by shuffle.  All lengths up to 64 are one such
// pass, and every longer length ends in one; a wave works on four tiles at a time, four independent shuffle chains.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cph {

constexpr uint32_t kWgSortThreads = 256;
constexpr unsigned long long kSortNone = ~0ull;           // the word that sorts behind every entry

__host__ __device__ inline uint32_t wg_sort_len(uint32_t entries) {
    uint32_t p = 64;
    while (p < entries) p *= 2;
    return p;
}

// float32 <-> the uint32 that orders the same way: the usual sign flip (a distance can be slightly negative).
__device__ __forceinline__ uint32_t orderable(float s) {
    const uint32_t u = __float_as_uint(s);
    return u ^ ((u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float from_orderable(uint32_t v) {
    return __uint_as_float((v & 0x80000000u) ? (v ^ 0x80000000u) : ~v);
}

// One compare-exchange step at distance j < 64 of the element at index i, held by this lane (lane = i & 63).
__device__ __forceinline__ unsigned long long wg_sort_lane_step(unsigned long long a, uint32_t i, uint32_t j, uint32_t len) {
    const unsigned long long b = __shfl_xor(a, (int)j);
    const bool keep_min = ((i & j) == 0) == ((i & len) == 0);
    return keep_min ? (a < b ? a : b) : (a < b ? b : a);
}

// The steps at distances first_j, first_j / 2, ... 1 of the merges of length len_lo, 2 len_lo, ... len_hi (each merge starts
// at min(first_j, its length / 2)) on every 64-element tile of w[0, P).  A wave holds four tiles at a time, one element per
// lane each: the four shuffle chains are independent, which hides the latency of one behind the others.
__device__ __forceinline__ void wg_sort_lane_pass(unsigned long long* w, uint32_t P, uint32_t tid, uint32_t len_lo, uint32_t len_hi,
                                                  uint32_t first_j) {
    constexpr uint32_t kTiles = 4;
    for (uint32_t base = tid; base < P; base += kTiles * kWgSortThreads) {      // (base & ~63 is the same in a whole wave)
        unsigned long long a[kTiles];
#pragma unroll
        for (uint32_t u = 0; u < kTiles; ++u) a[u] = base + u * kWgSortThreads < P ? w[base + u * kWgSortThreads] : kSortNone;
        for (uint32_t len = len_lo; len <= len_hi; len <<= 1)
            for (uint32_t j = (len >> 1) < first_j ? (len >> 1) : first_j; j; j >>= 1) {
#pragma unroll
                for (uint32_t u = 0; u < kTiles; ++u) a[u] = wg_sort_lane_step(a[u], base + u * kWgSortThreads, j, len);
            }
#pragma unroll
        for (uint32_t u = 0; u < kTiles; ++u)
            if (base + u * kWgSortThreads < P) w[base + u * kWgSortThreads] = a[u];
    }
}

// Ascending bitonic sort of w[0, P), P a power of two >= 64, by the whole workgroup of kWgSortThreads; ends with a barrier.
__device__ inline void wg_sort(unsigned long long* w, uint32_t P, uint32_t tid) {
    wg_sort_lane_pass(w, P, tid, 2, 64, 32);
    __syncthreads();
    for (uint32_t len = 128; len <= P; len <<= 1) {
        for (uint32_t j = len >> 1; j >= 64; j >>= 1) {
            for (uint32_t p = tid; p < P / 2; p += kWgSortThreads) {
                const uint32_t lo = 2 * p - (p & (j - 1)), hi = lo + j;
                const unsigned long long a = w[lo], b = w[hi];
                if ((a > b) == ((lo & len) == 0)) {
                    w[lo] = b;
                    w[hi] = a;
                }
            }
            __syncthreads();
        }
        wg_sort_lane_pass(w, P, tid, len, len, 32);
        __syncthreads();
    }
}

// The first-position id table over the C ids of a candidate row, in LDS: tab_id[H], tab_pos[H], H = diverse_table_slots(C)
// = the power of two >= 2 C.  An id's slot keeps the lowest position the id occurs at.  The caller puts a barrier between
// the clear, the inserts and the finds.
constexpr uint32_t kNoId = 0xFFFFFFFFu;   // (n_ids <= 0xFFFFFFFF: no id has this value)

__host__ __device__ inline uint32_t diverse_table_slots(uint32_t C) {
    uint32_t h = 2;
    while (h < 2 * C) h *= 2;
    return h;
}

// Clears slot s.
__device__ __forceinline__ void id_table_clear(uint32_t* tab_id, uint32_t* tab_pos, uint32_t s) {
    tab_id[s] = kNoId;
    tab_pos[s] = kNoId;
}

__device__ __forceinline__ void id_table_insert(uint32_t* tab_id, uint32_t* tab_pos, uint32_t H, uint32_t id, uint32_t j) {
    uint32_t s = (id * 2654435761u) & (H - 1);
    for (;;) {                                            // (the table has at least C free slots: the probe ends)
        const uint32_t old = atomicCAS(&tab_id[s], kNoId, id);
        if (old == kNoId || old == id) break;
        s = (s + 1) & (H - 1);
    }
    atomicMin(&tab_pos[s], j);
}

// -> the slot of an id that was inserted.
__device__ __forceinline__ uint32_t id_table_find(const uint32_t* tab_id, uint32_t H, uint32_t id) {
    uint32_t s = (id * 2654435761u) & (H - 1);
    while (tab_id[s] != id) s = (s + 1) & (H - 1);
    return s;
}

}  // namespace cph
