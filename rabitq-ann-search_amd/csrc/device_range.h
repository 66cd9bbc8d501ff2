// device_range.h — range search (cph_range_search_*): every allowed id closer than a per-query radius, in CSR form.
//
// The distance of a (query, id) pair is the one of device_exact.h, formed by the same function (exact_scan_candidates),
// so its bits are those the exact search and the graph search report.  What is new is everything behind the distance
// (RangeSink): the selection is a threshold, not a top-k, and the output has no fixed shape.
//
// Two passes over the candidates, one kernel body (range_scan_kernel<SD, CH, kFill>), the work split of exact_scan_kernel
// (P contiguous parts x G query groups, one wave per workgroup, a lane owns a candidate):
//   count   counts[q * P + p] = hits of query q in part p               (query-major: a query's parts are adjacent)
//   offsets an exclusive uint64 scan over the nq * P counters (three launches), lims[q] = offs[q * P]
//   fill    the same loop; a hit's key (distance bits << 32 | internal id) goes to its place behind offs[q * P + p]
// Parts are ascending id ranges and ballots keep lane order, so the fill is deterministic: a query's segment comes out
// ascending in id.  The segmented sort then orders every segment by key -- ascending (distance bits, internal id), the
// order of the exact search -- and range_emit_kernel writes ids (through the row map if asked to) and distances straight
// into the caller's arrays.
//
// Sort.  A segment of at most kRangeRun keys: one wave, bitonic in LDS (exact_sort_keys), padded with kExactNoKey.  A longer
// one: its kRangeRun-sized runs are sorted like that, then merge passes of width w = kRangeRun, 2 kRangeRun, ... go back and
// forth between the arena and a second buffer of the same size: an element of the left run of a pair lands at its own
// index plus the number of strictly smaller keys in the right run, one of the right run the other way round
// (range_merge_dest: one binary search per element and pass; keys carry the id and are unique, so this is a permutation);
// an unpaired last run is copied.
//
// The graph route (exact = false) cuts the [n][K] rows of an ordinary search at the radius: range_cut_count_kernel,
// the same offsets scan, range_cut_emit_kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_exact.h"

namespace cph {

constexpr uint32_t kRangeRun = 4096;          // keys of one LDS sort: 32 KiB
constexpr uint32_t kRangeScanSpan = 2048;     // counters per block of the offsets scan (256 threads x 8)

// ---- the scan: count and fill -------------------------------------------------------------------------------------------
struct RangeArgs {
    ScanCommon s;
    const uint32_t* ids;                  // [m] ascending internal ids, or null: candidate c is id c
    uint32_t m;                           // candidates
    uint32_t P;                           // parts
    const float* radius;                  // [nq]
    uint32_t* counts;                     // [nq][P]: written by the count pass
    const unsigned long long* offs;       // [nq * P + 1]: read by the fill pass
    unsigned long long tile_base;         // offs[q_first * P]: the arena starts there
    unsigned long long* arena;
};

// The sink of exact_scan_candidates for a part's hits of the queries q0 .. q0 + nqg - 1: counted (count pass) or written
// to the arena behind the part's offset (fill pass).  LDS: gq counters (count) or gq 64-bit write positions (fill), then
// gq radii.
template <bool kFill>
struct RangeSink {
    unsigned long long* s_pos;            // fill: next free arena index
    uint32_t* s_cnt;                      // count: hits so far
    float* s_rad;
    unsigned long long* arena;
    uint32_t* counts;                     // the counter of (query q0, this part); query q0 + i: counts[i * P]
    uint32_t P;

    __device__ __forceinline__ RangeSink(unsigned char* smem, const RangeArgs& a, uint32_t q0, uint32_t nqg)
        : s_pos(reinterpret_cast<unsigned long long*>(smem)), s_cnt(reinterpret_cast<uint32_t*>(smem)),
          s_rad(reinterpret_cast<float*>(smem + (size_t)a.s.gq * 8)), arena(a.arena), counts(a.counts + (size_t)q0 * a.P + blockIdx.x),
          P(a.P) {
        for (uint32_t i = threadIdx.x; i < nqg; i += 64) {
            s_rad[i] = a.radius[q0 + i];
            if constexpr (kFill) s_pos[i] = a.offs[(size_t)(q0 + i) * a.P + blockIdx.x] - a.tile_base;
            else s_cnt[i] = 0;
        }
        __syncthreads();
    }

    __device__ __forceinline__ void take(uint32_t ql, float d, uint32_t id, bool live, int lane) const {
        const bool hit = live && d < s_rad[ql];            // strict; a NaN radius selects nothing
        const unsigned long long mask = __ballot(hit);
        if (mask == 0) return;
        const uint32_t add = (uint32_t)__popcll(mask);
        if constexpr (kFill) {
            // (every lane reads the position lane 0 stored after the query's previous hits: no barrier in between, for
            //  ExactPoolSink's reason -- one wave, LDS in program order)
            const unsigned long long at = s_pos[ql];
            if (hit) arena[at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = ((unsigned long long)__float_as_uint(d) << 32) | id;
            if (lane == 0) s_pos[ql] = at + add;
        } else {
            if (lane == 0) s_cnt[ql] += add;
        }
    }

    __device__ __forceinline__ void finish(uint32_t nqg, int lane) const {
        if constexpr (!kFill) {
            __syncthreads();
            for (uint32_t i = lane; i < nqg; i += 64) counts[(size_t)i * P] = s_cnt[i];
        }
    }
};

// Grid (P, G), one wave per workgroup; LDS: 12 gq bytes (RangeSink).  A part behind the candidates still writes its zeros.
template <int SD, int CH, bool kFill>
__global__ __launch_bounds__(64) void range_scan_kernel(RangeArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    const ScanCut c = scan_cut(a.s, a.m, D);
    if (c.ql_lo >= c.ql_hi) return;
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, ExactListSource{a.ids}, c.c_lo, c.c_hi, c.q_rows, c.q_norms, c.ql_hi - c.ql_lo,
                                  RangeSink<kFill>(smem, a, a.s.q_first + c.ql_lo, c.ql_hi - c.ql_lo));
}

// ---- offsets: exclusive uint64 scan of counts[n_cnt] -------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_scan_u64(unsigned long long v, int lane) {   // inclusive
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_up(v, d);
        if (lane >= d) v += y;
    }
    return v;
}

// Inclusive scan of one value per thread over a block of 256; *total = the block's sum.  s4: 4 words of LDS.
__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v, unsigned long long* s4, unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long x = wave_scan_u64(v, lane);
    if (lane == 63) s4[wave] = x;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned long long s = s4[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return x + before;
}

// sums[b] = sum of counts [2048 b, 2048 b + 2048).
__global__ __launch_bounds__(256) void range_offs_sums_kernel(const uint32_t* __restrict__ counts, uint64_t n_cnt,
                                                              unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long s4[4];
    const uint64_t first = (uint64_t)blockIdx.x * kRangeScanSpan + (uint64_t)threadIdx.x * 8;
    unsigned long long t = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e)
        if (first + e < n_cnt) t += counts[first + e];
    unsigned long long total;
    (void)block_scan_u64(t, s4, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// In-place exclusive scan of sums[nb] (nb = n_cnt / 2048: a few thousand at most); sums[nb] = the total.  One wave.
__global__ __launch_bounds__(64) void range_offs_scan_kernel(unsigned long long* sums, uint32_t nb) {
    const int lane = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < nb; base += 64) {
        const uint32_t i = base + lane;
        const unsigned long long v = i < nb ? sums[i] : 0ull;
        const unsigned long long x = wave_scan_u64(v, lane);
        if (i < nb) sums[i] = carry + x - v;
        carry += __shfl(x, 63);
    }
    if (lane == 0) sums[nb] = carry;
}

// offs[i] = counts before i (offs[n_cnt] = the total); lims[q] = offs[q * P], lims[nq] = the total.
__global__ __launch_bounds__(256) void range_offs_apply_kernel(const uint32_t* __restrict__ counts, uint64_t n_cnt,
                                                               const unsigned long long* __restrict__ sums, uint32_t nb, uint32_t P,
                                                               unsigned long long* __restrict__ offs, unsigned long long* __restrict__ lims) {
    __shared__ unsigned long long s4[4];
    const uint64_t first = (uint64_t)blockIdx.x * kRangeScanSpan + (uint64_t)threadIdx.x * 8;
    uint32_t c[8];
    unsigned long long t = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        c[e] = first + e < n_cnt ? counts[first + e] : 0u;
        t += c[e];
    }
    unsigned long long total;
    unsigned long long at = sums[blockIdx.x] + block_scan_u64(t, s4, &total) - t;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint64_t i = first + e;
        if (i < n_cnt) {
            offs[i] = at;
            if (i % P == 0) lims[i / P] = at;
        }
        at += c[e];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        offs[n_cnt] = sums[nb];
        lims[n_cnt / P] = sums[nb];
    }
}

// Enqueues the three launches.  d_sums: n_cnt / 2048 + 2 words of scratch.
inline void range_offsets(const uint32_t* d_counts, uint64_t n_cnt, uint32_t P, unsigned long long* d_sums, unsigned long long* d_offs,
                          unsigned long long* d_lims, hipStream_t st) {
    const uint32_t nb = (uint32_t)((n_cnt + kRangeScanSpan - 1) / kRangeScanSpan);
    hipLaunchKernelGGL(range_offs_sums_kernel, dim3(nb), dim3(256), 0, st, d_counts, (uint64_t)n_cnt, d_sums);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(range_offs_scan_kernel, dim3(1), dim3(64), 0, st, d_sums, nb);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(range_offs_apply_kernel, dim3(nb), dim3(256), 0, st, d_counts, (uint64_t)n_cnt, (const unsigned long long*)d_sums, nb, P,
                       d_offs, d_lims);
    HIP_CHECK(hipGetLastError());
}

// ---- segmented sort ------------------------------------------------------------------------------------------------------
// One LDS sort: keys [start, start + len) of the arena, 2 <= len <= kRangeRun.
struct RangeRun {
    unsigned long long start;
    uint32_t len, reserved;
};

// One wave per run; LDS: the launch's longest run rounded up to a power of two (>= 64) keys.
__global__ __launch_bounds__(64) void range_sort_runs_kernel(const RangeRun* __restrict__ runs, unsigned long long* __restrict__ arena) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    const RangeRun r = runs[blockIdx.x];
    const int lane = threadIdx.x;
    uint32_t N = 64;
    while (N < r.len) N <<= 1;
    unsigned long long* keys = arena + r.start;
    for (uint32_t i = lane; i < N; i += 64) sm[i] = i < r.len ? keys[i] : kExactNoKey;
    __syncthreads();
    exact_sort_keys(sm, N, lane);
    for (uint32_t i = lane; i < r.len; i += 64) keys[i] = sm[i];
}

// Where element i of a segment of `len` keys, sorted in runs of `w`, goes in the merge pass of width w (the statement
// both the kernel and cph_host_range_merge_pass run).
__host__ __device__ inline uint64_t range_merge_dest(const unsigned long long* in, uint64_t len, uint64_t w, uint64_t i) {
    const uint64_t run = i / w, other = (run ^ 1) * w;
    if (other >= len) return i;                                   // the unpaired last run: copied
    const uint64_t olen = len - other < w ? len - other : w;
    const unsigned long long key = in[i];
    uint64_t lo = 0, hi = olen;                                   // keys of the other run that are smaller (none is equal)
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (in[other + mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return (run >> 1) * 2 * w + (i - run * w) + lo;
}

// A segment longer than kRangeRun: keys [start, start + len) of both buffers.
struct RangeLong {
    unsigned long long start, len;
};

// Grid (blocks of the longest segment, segments): one merge pass of every listed segment, src -> dst.
__global__ __launch_bounds__(256) void range_merge_pass_kernel(const RangeLong* __restrict__ segs, const unsigned long long* __restrict__ src,
                                                               unsigned long long* __restrict__ dst, unsigned long long w) {
    const RangeLong s = segs[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.len) return;
    const unsigned long long* in = src + s.start;
    dst[s.start + range_merge_dest(in, s.len, w, i)] = in[i];
}

// One block per query of the tile: its sorted keys -> ids (through `rows` if given) and distances at lims[q].  A segment
// longer than kRangeRun is read from `keys_long` (where its last merge pass left it), any other from `keys`.
__global__ __launch_bounds__(256) void range_emit_kernel(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ keys_long,
                                                         const unsigned long long* __restrict__ lims, uint32_t q_first,
                                                         unsigned long long tile_base, const uint32_t* __restrict__ rows,
                                                         int64_t* __restrict__ out_ids, float* __restrict__ out_dist) {
    const uint32_t q = q_first + blockIdx.x;
    const unsigned long long lo = lims[q], hi = lims[q + 1];
    const unsigned long long* src = hi - lo > kRangeRun ? keys_long : keys;
    for (unsigned long long i = lo + threadIdx.x; i < hi; i += 256) {
        const unsigned long long key = src[i - tile_base];
        const uint32_t id = (uint32_t)key;
        out_ids[i] = (int64_t)(rows ? rows[id] : id);
        out_dist[i] = __uint_as_float((uint32_t)(key >> 32));
    }
}

// ---- the graph route: rows of a search, cut at the radius -----------------------------------------------------------------
// One wave per row: counts[q] = entries of row q with id >= 0 and dist < radius[q].
__global__ __launch_bounds__(64) void range_cut_count_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dist, uint32_t K,
                                                             const float* __restrict__ radius, uint32_t* __restrict__ counts) {
    const uint32_t q = blockIdx.x;
    const float r = radius[q];
    uint32_t c = 0;
    for (uint32_t j = threadIdx.x; j < K; j += 64) c += (ids[(size_t)q * K + j] >= 0 && dist[(size_t)q * K + j] < r) ? 1u : 0u;
    c = wave_sum_u32(c);
    if (threadIdx.x == 0) counts[q] = c;
}

// One wave per row: the entries that pass, in row order, at lims[q].
__global__ __launch_bounds__(64) void range_cut_emit_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dist, uint32_t K,
                                                            const float* __restrict__ radius, const unsigned long long* __restrict__ lims,
                                                            int64_t* __restrict__ out_ids, float* __restrict__ out_dist) {
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x;
    const float r = radius[q];
    unsigned long long at = lims[q];
    for (uint32_t base = 0; base < K; base += 64) {
        const uint32_t j = base + lane;
        const int64_t id = j < K ? ids[(size_t)q * K + j] : -1;
        const float d = j < K ? dist[(size_t)q * K + j] : 0.0f;
        const bool hit = id >= 0 && d < r;
        const unsigned long long mask = __ballot(hit);
        if (hit) {
            const unsigned long long o = at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            out_ids[o] = id;
            out_dist[o] = d;
        }
        at += (uint32_t)__popcll(mask);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// How the scan of nq queries against m candidates is cut: one grid of P parts x G groups per pass.
struct RangePlan {
    uint32_t P, part;     // parts, candidates per part
    uint32_t gq;          // queries per group
    uint32_t run;         // keys of one LDS sort
};

// The rule of plan_exact for the parts: enough waves for two per SIMD, few parts when the queries alone fill the GPU, never
// more than kExactMaxParts (the counters are nq x P).  There is no pool, so nothing here depends on a budget.
inline RangePlan plan_range(uint64_t m, uint64_t nq, int num_cus) {
    RangePlan pl{};
    pl.gq = 128;
    pl.run = kRangeRun;
    const uint64_t waves = (uint64_t)std::max(1, num_cus) * 8, blocks = (m + 63) / 64;
    const uint64_t G = std::max<uint64_t>(1, (nq + pl.gq - 1) / pl.gq);
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>({(waves + G - 1) / G, blocks, (uint64_t)kExactMaxParts}));
    pl.part = (uint32_t)(std::max<uint64_t>(1, (blocks + want - 1) / want) * 64);
    pl.P = (uint32_t)std::max<uint64_t>(1, (m + pl.part - 1) / pl.part);
    return pl;
}

// Rows of the padded query array of a batch of nq queries: nq rounded up to whole query tiles plus one tile more, because
// a fill launch starts at any query and always reads whole tiles (the rows behind nq are zero and their results unused).
inline uint64_t range_query_rows(uint64_t nq) {
    return (nq + kExactQT - 1) / kExactQT * kExactQT + kExactQT;
}

// Scratch bytes of the queries [lo, hi): their keys, twice when one of the segments needs merge passes.
inline uint64_t range_tile_bytes(const int64_t* lims, uint64_t lo, uint64_t hi, bool any_long) {
    return (uint64_t)(lims[hi] - lims[lo]) * 8 * (any_long ? 2 : 1);
}

// Cuts n queries into maximal consecutive tiles whose scratch fits the budget; a tile of a single query may exceed it.
// Returns starts[tiles + 1]: tile t holds the queries [starts[t], starts[t + 1]) (n = 0: empty, no tile).
inline std::vector<uint64_t> range_tiles(const int64_t* lims, uint64_t n, uint64_t budget) {
    std::vector<uint64_t> starts;
    uint64_t lo = 0;
    while (lo < n) {
        starts.push_back(lo);
        uint64_t hi = lo + 1;
        bool any_long = (uint64_t)(lims[hi] - lims[lo]) > kRangeRun;
        while (hi < n) {
            const bool nl = any_long || (uint64_t)(lims[hi + 1] - lims[hi]) > kRangeRun;
            if (range_tile_bytes(lims, lo, hi + 1, nl) > budget) break;
            any_long = nl;
            ++hi;
        }
        lo = hi;
    }
    if (n) starts.push_back(n);
    return starts;
}

}  // namespace cph
