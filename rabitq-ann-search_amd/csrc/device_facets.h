// device_facets.h — facet counts (cph_facet_counts, cph_facet_top): for m allowed-id bitmaps at once, the number of allowed
// rows per distinct value of one column.  The column is given as dictionary codes: code[i] < U names the value of row i
// (host_index.h: facet_dictionary_host; codes ascend with values); a tag column is its CSR lims[n + 1] plus one code per
// CSR entry, and a row counts once for every tag it holds.  counts[j][u] = |{ i < n : bit i of filter j, code u in row i }|.
//
// facet_counts_kernel.  A workgroup of kFacetBlock = 256 threads owns a run of `run_tiles` consecutive tiles of
// kFacetTileIds = 8,192 ids (256 bitmap words, one word per thread) and the kFacetFilterChunk = 16 filters of its
// blockIdx.y.  A thread loads the 32 codes of its word ONCE per tile, as eight 16 B loads of its own 128 B line (the
// register tile of device_labels.h), and reuses them for every filter of the pass: per filter it reads its bitmap word
// (one coalesced 256 B load per wave; a null table entry means "every row" and reads nothing) and adds one count per set
// bit.  Bits at ids >= n are masked off, and no word at or behind (n + 31) / 32 is read.
//
// Where the counts go (template parameter kLds):
//   on-chip  U <= kFacetLdsBins = 8,192.  The block keeps `fpp` = min(16, 8,192 / U) histograms of U 32-bit bins in LDS --
//            32 KiB per block, so the four blocks a CU is meant to hold use 128 of its 160 KiB -- and walks its chunk in
//            passes of fpp filters: zero, count the whole run with LDS atomics, then flush every NON-ZERO bin with one
//            64-bit global atomic (once per workgroup, filter and value).  With U <= 512 all 16 filters share one pass and
//            the codes are loaded once per tile and chunk; above that they are loaded once per pass (from L2 after the
//            first).  A bin counts at most the ids of the run, which the launcher keeps below 2^32.
//   global   U above the limit: 64-bit global atomics straight into counts[j][code], no LDS.  With that many values a
//            filter's rows are spread over many counters unless the data is skewed.
// Contention.  The common case is every allowed row falling into ONE value (a tenant's filter faceted by tenant).  A
// thread therefore walks its 32 ids in order and merges a run of equal codes into one add: sorted or clustered columns,
// and U = 1, cost one atomic per thread and filter instead of 32; on the on-chip path those meet in LDS, and the global
// word sees one add per workgroup.  On the global path the merged adds of 256 threads still go to memory one by one;
// that path is for large U only.
// Run length.  Zeroing and flushing cost about 2 U / 256 LDS steps per thread and filter, counting 32 steps per tile; the
// launcher asks for run_tiles >= U / 1,024 (the overhead is then a quarter of the counting at most) and gives that up only
// where the grid would drop below kFacetMinBlocks = 128 workgroups.  That floor is measured (profiles/facets.md, "run
// length"; 1M rows, U = 8,000): at m = 256 a floor of 2,048 keeps every run at one tile and takes 1,369 us, floors of 128
// and 16 allow runs of 8 tiles and take 476 us; at m = 16 (123 tiles in all) floors of 2,048 and 128 both keep one tile per
// workgroup, 125 us, while a floor of 16 leaves 18 workgroups and takes 406 us.
// Counter width.  Global counters are 64-bit: no index size the handle accepts (below 2^32 rows, 2^32 CSR entries)
// overflows them, so nothing is refused for width.  The slab of one launch is bounded: kFacetSlabCounters = 2^22 counters
// (32 MiB) -- when m x U exceeds it the host walks the filters in groups of slab / U (one filter at least: a single
// filter always needs its U counters).
// On-chip limit.  8,192 bins is what four resident blocks leave room for; it is not a crossover: at 1M rows the on-chip
// path is 2.8x to 17x faster than the global one at U = 8,192 (123 against 346 us uniform, 121 against 2,118 us skewed,
// m = 16) and 10x to 196x at U = 8 and 1,000, so the limit is the largest the LDS allows (profiles/facets.md, "paths").
// The third variant -- per-value bit masks of a lane's 32 ids built once, then AND + popcount per value and filter, no
// atomics before the wave reduction -- is NOT built: it costs U x 16 mask words per lane, so it only fits U <= 4 or so,
// and the run merging above already removes the same-bin contention it was meant for.  Measured at U = 8 and 1M rows the
// on-chip path takes 13 us for one filter and 40 us for 16 (launch and chunk latency: 123 workgroups on 256 CUs) and
// 255 to 877 us for 1,024, 8 to 29 % of the byte floor; what a mask variant could save there is the LDS atomics of the
// 100 % selectivity rows, and nobody has shown that it would.
// Integer adds commute: every count is exact and the same on every run.  No float anywhere.
//
// facet_top_kernel.  One workgroup per filter scans its U counters in blocks and keeps the K <= kFacetTopMax = 1,024 best
// in LDS: buf[0, K) the best so far, buf[K, kFacetTopLen = 2,048) the block's candidates, keys (~count << 32) | code --
// ascending keys are count descending, then code (= value) ascending -- zero counts as kSortNone, so they never enter;
// wg_sort (device_wg_primitives.h) over the 16 KiB buffer, skipped for a block without a non-zero count.  It writes
// values[code], the count and found = min(K, non-zero counters); the slots behind `found` get 0.  count < 2^32 (n is).
// The host statements are host_index.h: facet_counts_host, facet_top_host.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "device_buf.h"
#include "device_wg_primitives.h"

namespace cph {

constexpr uint32_t kFacetBlock = 256;                     // threads per block: one bitmap word per thread and tile
constexpr uint32_t kFacetTileIds = 32 * kFacetBlock;      // ids per tile
constexpr uint32_t kFacetFilterChunk = 16;                // filters per blockIdx.y
constexpr uint32_t kFacetLdsBins = 8192;                  // the on-chip bin limit: 32 KiB of LDS per block, 4 blocks per CU
constexpr uint32_t kFacetBlocksPerCu = 4;                 // ... the residency that limit was chosen for
#ifndef CPH_FACET_MIN_BLOCKS
#define CPH_FACET_MIN_BLOCKS 128                          // (a diagnostic build may set another: profiles/facets.md, run length)
#endif
constexpr uint32_t kFacetMinBlocks = CPH_FACET_MIN_BLOCKS;   // the grid the run length is not allowed to starve
constexpr uint32_t kFacetMaxRunTiles = (1u << 19) - 1;    // run ids < 2^32: a 32-bit LDS bin cannot overflow
constexpr uint32_t kFacetMaxFilters = 65535u * kFacetFilterChunk;   // filters per launch: grid.y <= 65,535
constexpr uint64_t kFacetSlabCounters = 1ull << 22;       // counters of one launch's slab (x 8 B = 32 MiB)
constexpr uint32_t kFacetTopMax = 1024;                   // K of facet_top_kernel, at most
constexpr uint32_t kFacetTopLen = 2 * kFacetTopMax;       // its LDS buffer: K best + (kFacetTopLen - K) candidates
enum FacetPath { kFacetAuto = 0, kFacetOnChip = 1, kFacetGlobal = 2 };

struct FacetArgs {
    const uint32_t* codes;            // [n] (dense column), or [lims[n]] parallel to the tags (16 B aligned)
    const uint32_t* lims;             // tag column: [n + 1]; null for a dense column
    uint64_t n;
    uint32_t U;
    const uint32_t* const* filters;   // [m] bitmaps of (n + 31) / 32 words; a null entry: every row
    uint32_t m;
    unsigned long long* counts;       // [m][U], zeroed by the launcher
    uint32_t run_tiles;               // tiles per workgroup
    uint32_t fpp;                     // on-chip: filters per pass, fpp * U <= kFacetLdsBins
};

// One thread's word of one filter into `bins` (LDS or global): dense column, the codes in registers.  A run of equal
// codes among the set bits is one add.
template <class Bin>
__device__ __forceinline__ void facet_count_dense(const uint32_t (&code)[32], uint32_t word, Bin* bins) {
    uint32_t cur = 0, cnt = 0;
#pragma unroll
    for (uint32_t t = 0; t < 32; ++t) {
        if ((word >> t) & 1u) {
            if (code[t] != cur && cnt) {
                atomicAdd(&bins[cur], (Bin)cnt);
                cnt = 0;
            }
            cur = code[t];
            ++cnt;
        }
    }
    if (cnt) atomicAdd(&bins[cur], (Bin)cnt);
}

// ... tag column: the entries of every allowed row, read from global memory (rows of up to 1,024 tags: the long-row walk
// of device_tags.h).  Tags are distinct inside a row, so a row adds one to each of its bins.
template <class Bin>
__device__ __forceinline__ void facet_count_tags(const uint32_t* __restrict__ codes, const uint32_t* __restrict__ lims, uint64_t id0,
                                                 uint32_t word, Bin* bins) {
    while (word) {
        const uint32_t t = (uint32_t)__builtin_ctz(word);
        word &= word - 1u;
        const uint32_t b = lims[id0 + t], e = lims[id0 + t + 1];
        for (uint32_t x = b; x < e; ++x) atomicAdd(&bins[codes[x]], (Bin)1);
    }
}

template <bool kTags, bool kLds>
__global__ __launch_bounds__(kFacetBlock) void facet_counts_kernel(const FacetArgs a) {
    __shared__ uint32_t hist[kLds ? kFacetLdsBins : 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t nw = (a.n + 31) / 32, tiles = (a.n + kFacetTileIds - 1) / kFacetTileIds;
    const uint64_t t0 = (uint64_t)blockIdx.x * a.run_tiles;
    const uint64_t t1 = t0 + a.run_tiles < tiles ? t0 + a.run_tiles : tiles;
    const uint32_t j0 = blockIdx.y * kFacetFilterChunk;
    const uint32_t j1 = j0 + kFacetFilterChunk < a.m ? j0 + kFacetFilterChunk : a.m;
    const uint32_t step = kLds ? a.fpp : kFacetFilterChunk;
    for (uint32_t jp = j0; jp < j1; jp += step) {            // (every loop bound is block-uniform: the barriers are safe)
        const uint32_t jq = jp + step < j1 ? jp + step : j1;
        if (kLds) {
            for (uint32_t i = tid; i < (jq - jp) * a.U; i += kFacetBlock) hist[i] = 0u;
            __syncthreads();
        }
        for (uint64_t tile = t0; tile < t1; ++tile) {
            const uint64_t w = tile * kFacetBlock + tid, id0 = w * 32;
            const bool in = w < nw;
            const uint32_t keep = !in ? 0u : id0 + 32 <= a.n ? 0xFFFFFFFFu : (1u << (uint32_t)(a.n - id0)) - 1u;
            uint32_t code[32];
            if (!kTags) {
                if (id0 + 32 <= a.n) {
                    const uint4* src = reinterpret_cast<const uint4*>(a.codes + id0);
#pragma unroll
                    for (uint32_t q = 0; q < 8; ++q) {
                        const uint4 v = src[q];
                        code[4 * q] = v.x; code[4 * q + 1] = v.y; code[4 * q + 2] = v.z; code[4 * q + 3] = v.w;
                    }
                } else {                                     // the last word of the index, and the threads behind it
#pragma unroll
                    for (uint32_t t = 0; t < 32; ++t) code[t] = id0 + t < a.n ? a.codes[id0 + t] : 0u;
                }
            }
            for (uint32_t j = jp; j < jq; ++j) {
                const uint32_t* f = a.filters ? a.filters[j] : nullptr;       // (block-uniform)
                const uint32_t word = (in && f ? f[w] : 0xFFFFFFFFu) & keep;
                if (kLds) {
                    uint32_t* bins = hist + (j - jp) * a.U;
                    if (kTags) facet_count_tags(a.codes, a.lims, id0, word, bins);
                    else facet_count_dense(code, word, bins);
                } else {
                    unsigned long long* bins = a.counts + (uint64_t)j * a.U;
                    if (kTags) facet_count_tags(a.codes, a.lims, id0, word, bins);
                    else facet_count_dense(code, word, bins);
                }
            }
        }
        if (kLds) {
            __syncthreads();
            unsigned long long* out = a.counts + (uint64_t)jp * a.U;          // the pass's histograms are contiguous there too
            for (uint32_t i = tid; i < (jq - jp) * a.U; i += kFacetBlock) {
                const uint32_t c = hist[i];
                if (c) atomicAdd(&out[i], (unsigned long long)c);
            }
            __syncthreads();
        }
    }
}

// The launch shape of one pass: which path, how many tiles per workgroup, how many filters per on-chip pass.
struct FacetPlan {
    bool lds;
    uint32_t run_tiles, fpp, gx, gy;
};
inline FacetPlan facet_plan(uint64_t n, uint32_t U, uint32_t m, int path) {
    if (path != kFacetAuto && path != kFacetOnChip && path != kFacetGlobal) throw std::invalid_argument("unknown facet counting path");
    if (path == kFacetOnChip && U > kFacetLdsBins)
        throw std::invalid_argument("the on-chip facet path holds at most " + std::to_string(kFacetLdsBins) + " values");
    FacetPlan p{};
    p.lds = path == kFacetAuto ? U <= kFacetLdsBins : path == kFacetOnChip;
    const uint64_t tiles = (n + kFacetTileIds - 1) / kFacetTileIds;
    p.gy = (m + kFacetFilterChunk - 1) / kFacetFilterChunk;
    p.fpp = kFacetFilterChunk;
    uint64_t run = 1;
    if (p.lds) {
        p.fpp = std::max<uint32_t>(1, std::min<uint32_t>(kFacetFilterChunk, kFacetLdsBins / std::max<uint32_t>(U, 1)));
        const uint64_t want = std::max<uint64_t>(1, ((uint64_t)U + 1023) / 1024);
        const uint64_t cap = std::max<uint64_t>(1, tiles * p.gy / kFacetMinBlocks);
        run = std::min<uint64_t>(std::min(want, cap), kFacetMaxRunTiles);
    }
    p.run_tiles = (uint32_t)run;
    p.gx = (uint32_t)((tiles + run - 1) / run);
    return p;
}

// Enqueues the pass on `st` (the m * U counters zeroed first); every pointer lives on the current device.
// 1 <= m <= kFacetMaxFilters, U >= 1, n < 2^32; d_filters may be null when every filter is "every row".
inline void facet_counts(const uint32_t* d_codes, const uint32_t* d_lims, uint64_t n, uint32_t U, const uint32_t* const* d_filters,
                         uint32_t m, unsigned long long* d_counts, int path, hipStream_t st) {
    const FacetPlan p = facet_plan(n, U, m, path);
    HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)m * U * 8, st));
    if (n == 0) return;
    FacetArgs a{d_codes, d_lims, n, U, d_filters, m, d_counts, p.run_tiles, p.fpp};
    const dim3 grid(p.gx, p.gy), block(kFacetBlock);
    if (d_lims) {
        if (p.lds) hipLaunchKernelGGL((facet_counts_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((facet_counts_kernel<true, false>), grid, block, 0, st, a);
    } else {
        if (p.lds) hipLaunchKernelGGL((facet_counts_kernel<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((facet_counts_kernel<false, false>), grid, block, 0, st, a);
    }
    HIP_CHECK(hipGetLastError());
}

// counts: [m][U]; values: [U] (the dictionary); out_values / out_counts: [m][K]; found: [m].
__global__ __launch_bounds__(kWgSortThreads) void facet_top_kernel(const unsigned long long* __restrict__ counts, uint32_t U,
                                                                   const int32_t* __restrict__ values, uint32_t K,
                                                                   int32_t* __restrict__ out_values,
                                                                   unsigned long long* __restrict__ out_counts,
                                                                   uint32_t* __restrict__ found) {
    __shared__ unsigned long long buf[kFacetTopLen];
    const uint32_t tid = threadIdx.x, j = blockIdx.x;
    const unsigned long long* c = counts + (uint64_t)j * U;
    for (uint32_t i = tid; i < kFacetTopLen; i += kWgSortThreads) buf[i] = kSortNone;
    __syncthreads();
    const uint32_t block = kFacetTopLen - K;
    for (uint64_t base = 0; base < U; base += block) {
        int any = 0;
        for (uint32_t i = tid; i < block; i += kWgSortThreads) {
            const uint64_t u = base + i;
            const unsigned long long cnt = u < U ? c[u] : 0ull;
            buf[K + i] = cnt ? ((unsigned long long)(~(uint32_t)cnt) << 32) | u : kSortNone;
            any |= cnt != 0;
        }
        if (__syncthreads_or(any)) wg_sort(buf, kFacetTopLen, tid);      // (ends with a barrier; the vote is one, too)
    }
    uint32_t total = 0;
    for (uint32_t r = 0; r < (K + kWgSortThreads - 1) / kWgSortThreads; ++r) {
        const uint32_t i = r * kWgSortThreads + tid;
        const unsigned long long key = i < K ? buf[i] : kSortNone;
        const bool have = key != kSortNone;
        if (i < K) {
            out_values[(uint64_t)j * K + i] = have ? values[(uint32_t)key] : 0;
            out_counts[(uint64_t)j * K + i] = have ? (unsigned long long)(~(uint32_t)(key >> 32)) : 0ull;
        }
        total += (uint32_t)__syncthreads_count(have);
    }
    if (tid == 0) found[j] = total;
}

// Enqueues the selection behind a facet_counts pass on `st`.  1 <= K <= kFacetTopMax, m >= 1; U == 0 is fine (all empty).
inline void facet_top(const unsigned long long* d_counts, uint32_t U, const int32_t* d_values, uint32_t m, uint32_t K,
                      int32_t* d_out_values, unsigned long long* d_out_counts, uint32_t* d_found, hipStream_t st) {
    hipLaunchKernelGGL(facet_top_kernel, dim3(m), dim3(kWgSortThreads), 0, st, d_counts, U, d_values, K, d_out_values, d_out_counts,
                       d_found);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
