// device_exact.h — exact search over a candidate set (cph_search_batch_exact): every query against every allowed id,
// brute force on the fp32 VALU, top-k selected on the device.  No nq x m distance matrix is ever written.
//
// Arithmetic (fixed): the distance of (query q, id i) has the bits cph_exact_l2 returns for the pair, and so the bits the
// graph search returns for that id (core/memory.hpp:81-95, search/rabitq_search.hpp:90-93): eight FMA chains, chain j
// over elements j, j+8, ... of the padded rows from 0, reduced as ((c0+c4)+(c1+c5))+((c2+c6)+(c3+c7)); qnorm the same
// chains over q*q; exact_from_dot on top.  The graph search spreads the eight chains over eight lanes and reduces them
// with lane exchanges; here ONE lane owns a candidate and all eight chains of every (candidate, query) pair it works on,
// so the reduction is three in-lane additions and the inner loop has no cross-lane traffic at all.  MFMA is out: its
// accumulation order is another one.
//
// Work split.  The candidates (the filter's ascending id list, or 0..n-1) are cut into P contiguous PARTS, the queries of
// one launch into G GROUPS of `gq`; workgroup (p, g) is one wave.  It takes 64 candidates of its part at a time -- a lane
// holds its candidate's vector in VGPRs (D = 128: all of it, loaded once per 64 candidates; other D: CH dimensions at a
// time) -- and runs the group's queries past them in tiles of kExactQT: the tile's query values are wave-uniform and come
// through scalar loads (constant address space), so every FMA is  v_fma acc, s_query, v_candidate  -- one VALU
// instruction per pair-dimension, 2 D flop per pair, the bound is VALU fp32.
//
// Selection.  Per (part, query) the wave keeps a POOL of C = 2 Kp keys in HBM (Kp = max(64, k rounded up to a power of two);
// key = distance bits << 32 | internal id: distances are >= +0, so unsigned order is (distance, id) order) and, in LDS, the
// pool's fill count and a threshold -- the k-th smallest distance seen once the pool has been compacted to k keys.  Lanes
// whose distance is <= the threshold append by ballot; a pool that would overflow is first sorted in LDS (bitonic) and cut
// to its k smallest keys, which also lowers the threshold.  A dropped key is never among the k smallest of its part, so
// after the last candidate the pool, sorted and cut once more, is the part's exact top-k.  exact_merge_kernel (one wave
// per query) folds the P sorted lists into one, translates ids through the row map if asked to, and pads.
// Scratch: P x queries-per-launch x C keys; the host cuts a batch into several launches if that would not fit.
//
// Order: ascending distance, equal distance bits by ascending internal id; every id at most once (parts are disjoint).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <stdexcept>
#include <string>
#include <vector>

#include "device_buf.h"
#include "device_fastscan.h"
#include "device_search.h"

namespace cph {

constexpr uint32_t kExactMaxK = 1024;
constexpr int kExactQT = 8;                              // queries per tile: 8 x 8 chain accumulators per lane
constexpr unsigned long long kExactNoKey = ~0ull;        // sorts behind every real key (its distance bits are a NaN's)
constexpr uint32_t kExactMaxParts = 256;                 // lists the merge kernel folds per query, at most
constexpr uint32_t kFilterSpan = 2048;                   // ids per block of the compaction kernels (64 bitmap words)

// ---- allowed bitmap -> ascending id list ----------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// Allowed ids of bitmap word w: bits behind n_bits in the last word do not count, whoever made the bitmap.
__device__ __forceinline__ uint32_t filter_word_count(const uint32_t* __restrict__ words, uint64_t w, uint64_t nw, uint64_t n_bits) {
    if (w >= nw) return 0u;
    uint32_t x = words[w];
    if (w == nw - 1 && (n_bits & 31)) x &= (1u << (n_bits & 31)) - 1u;
    return (uint32_t)__popc(x);
}

// counts[b] = allowed ids among ids [2048 b, 2048 b + 2048); one wave per block.
__global__ __launch_bounds__(64) void filter_count_kernel(const uint32_t* __restrict__ words, uint64_t n_bits, uint64_t nw,
                                                          uint32_t* __restrict__ counts) {
    const uint64_t w = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    const uint32_t c = wave_sum_u32(filter_word_count(words, w, nw, n_bits));
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// In-place exclusive scan of counts[nb]; one wave.
__global__ __launch_bounds__(64) void filter_scan_kernel(uint32_t* counts, uint32_t nb) {
    const int lane = threadIdx.x;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += 64) {
        const uint32_t i = base + lane;
        const uint32_t v = i < nb ? counts[i] : 0u;
        uint32_t x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (i < nb) counts[i] = carry + x - v;
        carry += __shfl(x, 63);
    }
}

// Scatter: block b writes its ids at offs[b]; each of its four waves owns 512 consecutive ids (16 words), starts behind
// the waves before it and appends 64 ids at a time at ballot / popcount prefixes -- the list comes out ascending.
__global__ __launch_bounds__(256) void filter_ids_kernel(const uint32_t* __restrict__ words, uint64_t n_bits, uint64_t nw,
                                                         const uint32_t* __restrict__ offs, uint32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * 64 + lane;
    uint32_t base = offs[blockIdx.x] + wave_sum_u32(lane < wave * 16 ? filter_word_count(words, w, nw, n_bits) : 0u);
    const uint64_t first = (uint64_t)blockIdx.x * kFilterSpan + (uint64_t)wave * 512;
    for (int it = 0; it < 8; ++it) {
        const uint64_t id = first + (uint64_t)it * 64 + lane;
        const bool bit = id < n_bits && ((words[id >> 5] >> (id & 31)) & 1u);
        const unsigned long long mask = __ballot(bit);
        if (bit) out[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)id;
        base += (uint32_t)__popcll(mask);
    }
}

// Enqueues the three kernels on `st`: d_ids[popcount] = the set bits of d_words, ascending.  d_counts: (n_bits + 2047) /
// 2048 words of scratch that must live until the kernels have run.
inline void filter_ids(const uint32_t* d_words, uint64_t n_bits, uint32_t* d_counts, uint32_t* d_ids, hipStream_t st) {
    if (n_bits == 0) return;
    const uint64_t nw = (n_bits + 31) / 32;
    const uint32_t nb = (uint32_t)((n_bits + kFilterSpan - 1) / kFilterSpan);
    hipLaunchKernelGGL(filter_count_kernel, dim3(nb), dim3(64), 0, st, d_words, n_bits, nw, d_counts);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(filter_scan_kernel, dim3(1), dim3(64), 0, st, d_counts, nb);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(filter_ids_kernel, dim3(nb), dim3(256), 0, st, d_words, n_bits, nw, (const uint32_t*)d_counts, d_ids);
    HIP_CHECK(hipGetLastError());
}

// Host statement of the same compaction (cph_host_filter_ids).
inline uint64_t filter_ids_host(const uint32_t* words, uint64_t n_bits, uint32_t* out) {
    uint64_t c = 0;
    for (uint64_t w = 0, nw = (n_bits + 31) / 32; w < nw; ++w) {
        uint32_t x = words[w];
        if (w == nw - 1 && (n_bits & 31)) x &= (1u << (n_bits & 31)) - 1u;
        for (; x; x &= x - 1) out[c++] = (uint32_t)(w * 32 + (uint64_t)__builtin_ctz(x));
    }
    return c;
}

// ---- queries: zero-padded rows and their norms ------------------------------------------------------------------------
// qpad[nq_pad][D] (rows behind nq are zero: the last tile reads them), qnorm[nq_pad] = the search kernel's query_norm_sq
// (the same chains, the same tree).  Also leaves the batch's one statistic, the number of exact evaluations.
// perm (the grouped form): padded row j holds query perm[j] -- a batch with per-query filters lays the queries of one filter
// next to each other (cphnsw_mi355x.hip: enqueue_filters); null: row j holds query j.
__device__ __forceinline__ void exact_pad_rows(const float* __restrict__ q, const uint32_t* __restrict__ perm, uint32_t nq,
                                               uint32_t nq_pad, uint32_t dim, uint32_t D, float* __restrict__ qpad,
                                               float* __restrict__ qnorm, unsigned long long* stats, unsigned long long n_exact) {
    __shared__ float s_q[2048];
    const int lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) stats[kStatExact] = n_exact;
    for (uint32_t qi = blockIdx.x; qi < nq_pad; qi += gridDim.x) {
        const size_t src = (perm && qi < nq) ? perm[qi] : qi;
        for (uint32_t d = lane; d < D; d += 64) {
            const float x = (qi < nq && d < dim) ? q[src * dim + d] : 0.0f;
            s_q[d] = x;
            qpad[(size_t)qi * D + d] = x;
        }
        __syncthreads();
        float c = 0.0f;
        for (uint32_t i = lane & 7; i < D; i += 8) c = __fmaf_rn(s_q[i], s_q[i], c);
        c = group_reduce8(c);
        if (lane == 0) qnorm[qi] = c;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void exact_pad_kernel(const float* __restrict__ q, uint32_t nq, uint32_t nq_pad, uint32_t dim,
                                                       uint32_t D, float* __restrict__ qpad, float* __restrict__ qnorm,
                                                       unsigned long long* stats, unsigned long long n_exact) {
    exact_pad_rows(q, nullptr, nq, nq_pad, dim, D, qpad, qnorm, stats, n_exact);
}

__global__ __launch_bounds__(64) void exact_pad_groups_kernel(const float* __restrict__ q, const uint32_t* __restrict__ perm,
                                                              uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t D,
                                                              float* __restrict__ qpad, float* __restrict__ qnorm,
                                                              unsigned long long* stats, unsigned long long n_exact) {
    exact_pad_rows(q, perm, nq, nq_pad, dim, D, qpad, qnorm, stats, n_exact);
}

// ---- the scan ---------------------------------------------------------------------------------------------------------
// What every scan kernel is told about the rows, the padded queries and the cut of a launch (scan_common in
// cphnsw_mi355x.hip fills it); the kernels' own argument structs embed it.
struct ScanCommon {
    const float* raw;             // [n][D]
    const float* norm_sq;         // [n]
    const float* qpad;            // [nq_pad][D]
    const float* qnorm;           // [nq_pad]
    uint32_t D;
    uint32_t gq;                  // queries per group (a multiple of kExactQT)
    uint32_t q_first, q_count;    // the queries of this launch   (the grouped scan: unused, its items state the cut)
    uint32_t part;                // candidates per part (a multiple of 64)
};

struct ExactArgs {
    ScanCommon s;
    const uint32_t* ids;          // [m] ascending internal ids, or null: candidate c is id c
    uint32_t m;                   // candidates
    uint32_t k, C;                // pool capacity C = 2 Kp >= k + 64, a power of two
    unsigned long long* pools;    // [P][q_count][C]
    uint32_t* counts;             // [P][q_count]
};

// Ascending bitonic sort of sm[N] (N a power of two >= 2) by one wave; sm is complete and visible on entry (a barrier
// before), sorted and visible on return.
__device__ __forceinline__ void exact_sort_keys(unsigned long long* sm, uint32_t N, int lane) {
    for (uint32_t kk = 2; kk <= N; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < N / 2; i += 64) {
                const uint32_t lo = ((i & ~(j - 1u)) << 1) | (i & (j - 1u)), hi = lo | j;
                const bool up = (lo & kk) == 0;
                const unsigned long long x = sm[lo], y = sm[hi];
                if ((x > y) == up) { sm[lo] = y; sm[hi] = x; }
            }
            __syncthreads();
        }
}

// sm[N] holds an ascending half followed by a descending half (a bitonic sequence): the log N stages that leave it
// ascending.  Same entry and exit conditions as exact_sort_keys.
__device__ __forceinline__ void exact_merge_keys(unsigned long long* sm, uint32_t N, int lane) {
    for (uint32_t j = N >> 1; j > 0; j >>= 1) {
        for (uint32_t i = lane; i < N / 2; i += 64) {
            const uint32_t lo = ((i & ~(j - 1u)) << 1) | (i & (j - 1u)), hi = lo | j;
            const unsigned long long x = sm[lo], y = sm[hi];
            if (x > y) { sm[lo] = y; sm[hi] = x; }
        }
        __syncthreads();
    }
}

// pool[cnt] (cnt <= C) -> its min(cnt, k) smallest keys, ascending; returns that count and, through thr, the distance bits
// of the k-th (all ones while there are fewer than k).
__device__ __forceinline__ uint32_t exact_compact(unsigned long long* sm, unsigned long long* pool, uint32_t cnt, uint32_t k,
                                                  int lane, uint32_t& thr) {
    __threadfence();                              // the appended keys, written by single lanes, are visible to all
    uint32_t N = 64;
    while (N < cnt) N <<= 1;
    for (uint32_t i = lane; i < N; i += 64) sm[i] = i < cnt ? pool[i] : kExactNoKey;
    __syncthreads();
    exact_sort_keys(sm, N, lane);
    const uint32_t kept = cnt < k ? cnt : k;
    for (uint32_t i = lane; i < kept; i += 64) pool[i] = sm[i];
    thr = kept == k ? (uint32_t)(sm[k - 1] >> 32) : 0xFFFFFFFFu;
    __syncthreads();                              // sm is free again
    return kept;
}

typedef __attribute__((address_space(4))) const float* exact_uniform_ptr;

// acc[t][j] += the CH elements v[] of chain j against query t's; q = first query of the tile at the chunk's first dimension.
// The query values arrive in blocks of up to 32 scalar registers, two blocks in flight: block i + 1 is requested, then block
// i's FMAs run.  The empty asm statements pin that order (left alone, the compiler hoists all 8 x CH scalar loads of a tile
// to the front and spills most of them to VGPR lanes); they emit nothing.
template <int CH>
__device__ __forceinline__ void exact_fma_chunk(const float (&v)[CH], exact_uniform_ptr q, uint32_t D, float (&acc)[kExactQT][8]) {
    constexpr int SB = CH < 32 ? CH : 32, NB = CH / SB, TOT = kExactQT * NB;
    float qs[2][SB];
#pragma unroll
    for (int e = 0; e < SB; ++e) qs[0][e] = q[e];
#pragma unroll
    for (int i = 0; i < TOT; ++i) {
        const int t = i / NB, b = (i % NB) * SB;
#pragma unroll
        for (int e = 0; e < SB; ++e) asm volatile("" : "+s"(qs[i & 1][e]));       // block i has arrived
        if (i + 1 < TOT) {
            exact_uniform_ptr nx = q + (size_t)((i + 1) / NB) * D + ((i + 1) % NB) * SB;
            asm volatile("" : "+s"(nx));
#pragma unroll
            for (int e = 0; e < SB; ++e) qs[(i + 1) & 1][e] = nx[e];
        }
#pragma unroll
        for (int e = 0; e < SB; ++e) acc[t][(b + e) & 7] = __fmaf_rn(qs[i & 1][e], v[b + e], acc[t][(b + e) & 7]);
#pragma unroll
        for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(acc[t][j]));
    }
}

template <int CH>
__device__ __forceinline__ void exact_load_chunk(const float* __restrict__ row, float (&v)[CH]) {
#pragma unroll
    for (int e = 0; e < CH; e += 4) {
        const float4 x = *reinterpret_cast<const float4*>(row + e);
        v[e] = x.x; v[e + 1] = x.y; v[e + 2] = x.z; v[e + 3] = x.w;
    }
}

// The candidate source of the exact, grouped and range scans: candidate c is ids[c] (null: c), and every id may be
// selected -- the list is the filter.  (The tail's source, which tests a bitmap, is in device_tail.h.)
struct ExactListSource {
    const uint32_t* ids;
    __device__ __forceinline__ uint32_t id(uint32_t c) const { return ids ? ids[c] : c; }
    __device__ __forceinline__ bool allowed(uint32_t) const { return true; }
};

// THE candidate loop, the one place that forms a distance: every scan kernel (exact, grouped, tail, range) is this
// function with a source and a sink of its own.  Candidates [c_lo, c_hi) of `src` against the nqg queries whose padded
// rows start at qbase / qnorms; the workgroup is one wave.
//   Source  id(c): candidate c's internal id;  allowed(id): whether it may be selected -- asked once per 64 candidates,
//           before the query tiles.
//   Sink    take(ql, d, id, live, lane): called by the whole wave once per (query ql of the group, 64 candidates) with
//           each lane's distance; live is false in lanes behind c_hi or not allowed (their d and id are a neighbour's and
//           must not be selected).  finish(nqg, lane): after the last candidate.  A sink sets its LDS up, and lets a barrier
//           follow, where it is constructed.
// SD: compile-time padded dimension (0: D, any power of two 16..2048); CH: dimensions a lane holds at a time (CH == SD:
// the whole vector, loaded once per 64 candidates).
template <int SD, int CH, class Source, class Sink>
__device__ __forceinline__ void exact_scan_candidates(const float* __restrict__ raw, const float* __restrict__ norm_sq, uint32_t D,
                                                      const Source src, uint32_t c_lo, uint32_t c_hi, exact_uniform_ptr qbase,
                                                      exact_uniform_ptr qnorms, uint32_t nqg, const Sink sink) {
    const int lane = threadIdx.x;
    for (uint32_t cb = c_lo; cb < c_hi; cb += 64) {
        const bool valid = cb + lane < c_hi;
        const uint32_t id = src.id(valid ? cb + lane : c_hi - 1);
        const bool live = valid && src.allowed(id);
        const float* __restrict__ row = raw + (size_t)id * D;
        const float nrm = norm_sq[id];
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
                for (uint32_t base = 0; base < D; base += CH) {
                    exact_load_chunk<CH>(row + base, v);
                    exact_fma_chunk<CH>(v, qbase + (size_t)qt * D + base, D, acc);
                }
            }
#pragma unroll
            for (int t = 0; t < kExactQT; ++t) {
                const uint32_t ql = qt + t;                        // index inside the group
                if (ql >= nqg) break;                              // (wave-uniform: the rows behind the group in its last tile)
                const float dot = ((acc[t][0] + acc[t][4]) + (acc[t][1] + acc[t][5])) + ((acc[t][2] + acc[t][6]) + (acc[t][3] + acc[t][7]));
                sink.take(ql, exact_from_dot(qnorms[ql], nrm, dot), id, live, lane);
            }
        }
    }
    sink.finish(nqg, lane);
}

// The top-k sink of the exact, grouped and tail scans: the pools and fill counts of the work item's queries (query ql's at
// pools + ql * C, counts + ql).  LDS: C keys | gq thresholds | gq fill counts.  No barrier between lane 0's store of a
// count or threshold and the wave's next load of it: the workgroup is ONE wave, whose LDS operations complete in program
// order, and the store and the load are ordinary accesses of one address the compiler keeps in order.
struct ExactPoolSink {
    unsigned long long* sm;
    uint32_t* s_thr;
    uint32_t* s_cnt;
    unsigned long long* pools;
    uint32_t* counts;
    uint32_t k, C;

    __device__ __forceinline__ ExactPoolSink(unsigned char* smem, uint32_t gq, unsigned long long* pools_, uint32_t* counts_,
                                             uint32_t k_, uint32_t C_)
        : sm(reinterpret_cast<unsigned long long*>(smem)), s_thr(reinterpret_cast<uint32_t*>(sm + C_)), s_cnt(s_thr + gq),
          pools(pools_), counts(counts_), k(k_), C(C_) {
        for (uint32_t i = threadIdx.x; i < gq; i += 64) { s_thr[i] = 0xFFFFFFFFu; s_cnt[i] = 0; }
        __syncthreads();
    }

    __device__ __forceinline__ void take(uint32_t ql, float d, uint32_t id, bool live, int lane) const {
        const uint32_t dbits = __float_as_uint(d);
        const bool pass = live && dbits <= s_thr[ql];
        const unsigned long long mask = __ballot(pass);
        if (mask == 0) return;
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

    // every pool: sorted, cut to k
    __device__ __forceinline__ void finish(uint32_t nqg, int lane) const {
        for (uint32_t ql = 0; ql < nqg; ++ql) {
            uint32_t cnt = s_cnt[ql], thr;
            if (cnt) cnt = exact_compact(sm, pools + (size_t)ql * C, cnt, k, lane, thr);
            if (lane == 0) counts[ql] = cnt;
        }
    }
};

// The cut of a (parts, query groups) grid: workgroup (p, g) takes candidates [c_lo, c_hi) of m and the launch's queries
// [ql_lo, ql_hi) (relative to q_first); q_rows / q_norms: where the padded rows and the norms of those queries start.
struct ScanCut {
    uint32_t c_lo, c_hi, ql_lo, ql_hi;
    exact_uniform_ptr q_rows, q_norms;
};

__device__ __forceinline__ ScanCut scan_cut(const ScanCommon& s, uint32_t m, uint32_t D) {
    ScanCut c;
    c.c_lo = blockIdx.x * s.part;
    c.c_hi = min(m, c.c_lo + s.part);
    c.ql_lo = blockIdx.y * s.gq;
    c.ql_hi = min(s.q_count, c.ql_lo + s.gq);
    c.q_rows = (exact_uniform_ptr)(s.qpad + (size_t)(s.q_first + c.ql_lo) * D);
    c.q_norms = (exact_uniform_ptr)(s.qnorm + s.q_first + c.ql_lo);
    return c;
}

// Grid (P, G), one wave per workgroup; LDS: C keys + 2 gq words.
template <int SD, int CH>
__global__ __launch_bounds__(64) void exact_scan_kernel(ExactArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    const ScanCut c = scan_cut(a.s, a.m, D);
    if (c.c_lo >= c.c_hi || c.ql_lo >= c.ql_hi) return;
    const size_t pool = (size_t)blockIdx.x * a.s.q_count + c.ql_lo;
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, ExactListSource{a.ids}, c.c_lo, c.c_hi, c.q_rows, c.q_norms, c.ql_hi - c.ql_lo,
                                  ExactPoolSink(smem, a.s.gq, a.pools + pool * a.C, a.counts + pool, a.k, a.C));
}

// The grouped scan of a batch with per-query filters: ONE launch for every scanned (filter, query) pair.  A SEGMENT is a
// filter's id list (or the whole index) together with the queries that name it, contiguous in the padded query array
// (exact_pad_groups_kernel); the host planner (plan_exact_groups) cuts every segment into parts x query groups and
// writes one descriptor per work item; workgroup b, one wave, runs item b.  Pool geometry, LDS and the arithmetic are
// those of exact_scan_kernel -- the same source and sink.
struct ExactItem {                // 32 bytes
    const uint32_t* ids;          // the segment's ascending id list, or null: candidate c is id c
    uint32_t c_lo, c_hi;          // candidates of this part
    uint32_t q_lo, q_cnt;         // padded query rows of this group, q_cnt <= gq
    uint32_t pool;                // pool (and count) index of (this part, row q_lo); row q_lo + i: pool + i
    uint32_t reserved;
};

struct ExactGroupArgs {
    ScanCommon s;                 // (qpad: permuted)
    uint32_t k, C;
    unsigned long long* pools;    // [pools of the launch][C]
    uint32_t* counts;             // [pools of the launch]
    const ExactItem* items;       // [gridDim.x]
};

template <int SD, int CH>
__global__ __launch_bounds__(64) void exact_scan_groups_kernel(ExactGroupArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    typedef __attribute__((address_space(4))) const uint32_t* word_ptr;
    const word_ptr w = (word_ptr)reinterpret_cast<const uint32_t*>(a.items + blockIdx.x);   // wave-uniform: scalar loads
    ExactItem it;
    it.ids = reinterpret_cast<const uint32_t*>((uint64_t)w[0] | ((uint64_t)w[1] << 32));
    it.c_lo = w[2]; it.c_hi = w[3]; it.q_lo = w[4]; it.q_cnt = w[5]; it.pool = w[6];
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    if (it.c_lo >= it.c_hi || it.q_cnt == 0) return;
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, ExactListSource{it.ids}, it.c_lo, it.c_hi,
                                  (exact_uniform_ptr)(a.s.qpad + (size_t)it.q_lo * D), (exact_uniform_ptr)(a.s.qnorm + it.q_lo), it.q_cnt,
                                  ExactPoolSink(smem, a.s.gq, a.pools + (size_t)it.pool * a.C, a.counts + it.pool, a.k, a.C));
}

// One query's P sorted part lists (part p's pool is pool index first + p * stride) -> sm[0 .. Kp), Kp = C / 2, ascending,
// padded with kExactNoKey; returns the lists' total length.  sm: C keys: the lower half holds the Kp smallest keys so far,
// ascending; a part's list is laid behind it in descending order and one bitonic merge (log C stages, not a sort) leaves
// all C ascending again.  One wave.
__device__ __forceinline__ uint32_t exact_fold_parts(unsigned long long* sm, const unsigned long long* __restrict__ pools,
                                                     const uint32_t* __restrict__ counts, size_t first, uint32_t stride, uint32_t P,
                                                     uint32_t C, int lane) {
    const uint32_t Kp = C / 2;
    uint32_t total = 0;
    for (uint32_t i = lane; i < Kp; i += 64) sm[i] = kExactNoKey;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t cnt = counts[first + (size_t)p * stride];    // <= k <= Kp
        const unsigned long long* pool = pools + (first + (size_t)p * stride) * C;
        for (uint32_t i = lane; i < Kp; i += 64) sm[C - 1 - i] = i < cnt ? pool[i] : kExactNoKey;
        __syncthreads();
        exact_merge_keys(sm, C, lane);
        total += cnt;
    }
    return total;
}

// One wave per query of the launch: the P sorted part lists -> out rows [k], ascending, ids through `rows` if given,
// padded with -1 / FLT_MAX.  LDS: C keys.  exact_merge_query is one query's fold, shared by both merge kernels; the row
// goes to out row `out_row`.
__device__ __forceinline__ void exact_merge_query(const unsigned long long* __restrict__ pools, const uint32_t* __restrict__ counts,
                                                  size_t first, uint32_t stride, uint32_t P, uint32_t k, uint32_t C,
                                                  const uint32_t* __restrict__ rows, int64_t* __restrict__ out_ids,
                                                  float* __restrict__ out_dist, size_t out_row, unsigned char* smem) {
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    const int lane = threadIdx.x;
    (void)exact_fold_parts(sm, pools, counts, first, stride, P, C, lane);
    __syncthreads();
    const size_t o = out_row * k;
    for (uint32_t i = lane; i < k; i += 64) {
        const unsigned long long key = sm[i];
        const bool have = key != kExactNoKey;
        const uint32_t id = (uint32_t)key;
        out_ids[o + i] = have ? (int64_t)(rows ? rows[id] : id) : (int64_t)-1;
        out_dist[o + i] = have ? __uint_as_float((uint32_t)(key >> 32)) : FLT_MAX;
    }
}

__global__ __launch_bounds__(64) void exact_merge_kernel(const unsigned long long* __restrict__ pools, const uint32_t* __restrict__ counts,
                                                         uint32_t P, uint32_t q_first, uint32_t q_count, uint32_t k, uint32_t C,
                                                         const uint32_t* __restrict__ rows, int64_t* __restrict__ out_ids,
                                                         float* __restrict__ out_dist) {
    extern __shared__ __align__(16) unsigned char smem[];
    exact_merge_query(pools, counts, blockIdx.x, q_count, P, k, C, rows, out_ids, out_dist, (size_t)q_first + blockIdx.x, smem);
}

// The grouped merge: one wave per scanned query of the launch.  desc[q] = (pool index of its part 0, pool index stride
// between its parts, its segment's parts, its row in the batch): the query folds the parts of its OWN segment and writes
// to its original row.
__global__ __launch_bounds__(64) void exact_merge_groups_kernel(const unsigned long long* __restrict__ pools,
                                                                const uint32_t* __restrict__ counts, const uint4* __restrict__ desc,
                                                                uint32_t k, uint32_t C, const uint32_t* __restrict__ rows,
                                                                int64_t* __restrict__ out_ids, float* __restrict__ out_dist) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 d = desc[blockIdx.x];
    exact_merge_query(pools, counts, d.x, d.y, d.z, k, C, rows, out_ids, out_dist, d.w, smem);
}

// Rows of queries whose filter allows nothing: padding.  One wave per listed row.
__global__ __launch_bounds__(64) void exact_fill_rows_kernel(const uint32_t* __restrict__ list, uint32_t k, int64_t* __restrict__ out_ids,
                                                             float* __restrict__ out_dist) {
    const size_t o = (size_t)list[blockIdx.x] * k;
    for (uint32_t i = threadIdx.x; i < k; i += 64) {
        out_ids[o + i] = -1;
        out_dist[o + i] = FLT_MAX;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------
// How a batch of nq queries against m candidates is cut: launches of tile_q queries, each a grid of P parts x G groups.
struct ExactPlan {
    uint32_t Kp, C;       // pool geometry
    uint32_t gq;          // queries per group
    uint32_t tile_q;      // queries per launch (a multiple of gq unless it is the whole batch)
    uint32_t P, part;     // parts, candidates per part
    size_t pool_keys;     // P * tile_q * C
};

// Enough waves for two per SIMD; few parts when the queries alone fill the GPU (less scratch, fewer lists to merge), many when
// they do not -- but never more than kExactMaxParts: the merge kernel runs one merge per part and query.  Scratch above `budget` bytes: fewer queries per launch first, then fewer parts.
inline ExactPlan plan_exact(uint64_t m, uint32_t nq, uint32_t k, int num_cus, size_t budget) {
    ExactPlan pl{};
    pl.Kp = 64;
    while (pl.Kp < k) pl.Kp <<= 1;
    pl.C = 2 * pl.Kp;
    pl.gq = 128;
    const uint64_t waves = (uint64_t)std::max(1, num_cus) * 8, blocks = (m + 63) / 64;
    auto parts = [&](uint64_t want) {
        want = std::max<uint64_t>(1, std::min<uint64_t>({want, blocks, (uint64_t)kExactMaxParts}));
        pl.part = (uint32_t)((blocks + want - 1) / want * 64);
        pl.P = (uint32_t)((m + pl.part - 1) / pl.part);
        pl.pool_keys = (size_t)pl.P * pl.tile_q * pl.C;
    };
    pl.tile_q = nq;
    for (;;) {
        const uint64_t G = (pl.tile_q + pl.gq - 1) / pl.gq;
        parts((waves + G - 1) / G);
        if (pl.pool_keys * 8 <= budget || pl.tile_q <= pl.gq) break;
        pl.tile_q = std::max<uint32_t>(pl.gq, (pl.tile_q / 2 + pl.gq - 1) / pl.gq * pl.gq);
    }
    if (pl.pool_keys * 8 > budget) parts(budget / ((size_t)pl.tile_q * pl.C * 8));
    return pl;
}

// ---- per-query filters: grouping and the grouped plan (host only, no HIP call) -----------------------------------------
// Where a query of such a batch goes (the rules of takes_exact, per filter).
enum ExactRoute : uint8_t {
    kRoutePad = 0,        // its filter allows nothing: a padded row, no work
    kRouteScan = 1,       // the exact scan
    kRouteGraph = 2,      // the graph search
};

// Groups the n queries of a batch by filter: group f < F holds the queries with filter_of == f, group F those with -1.
// route[F + 1]; perm[n]: the queries ordered by group, inside a group in query order; seg[F + 2]: group g is
// perm[seg[g] .. seg[g + 1]).  popcount[F]: allowed ids of every filter.  Throws std::invalid_argument on a value outside [-1, F).
inline void filter_groups(const int32_t* filter_of, uint64_t n, const uint64_t* popcount, uint32_t F, uint64_t k, bool exact,
                          uint64_t exact_threshold, uint8_t* route, uint32_t* perm, uint32_t* seg) {
    for (uint32_t f = 0; f < F; ++f)
        route[f] = popcount[f] == 0 ? kRoutePad
                 : (exact || (exact_threshold > 0 && popcount[f] <= exact_threshold && k <= kExactMaxK)) ? kRouteScan : kRouteGraph;
    route[F] = exact ? kRouteScan : kRouteGraph;
    for (uint32_t g = 0; g < F + 2; ++g) seg[g] = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const int32_t f = filter_of[i];
        if (f < -1 || f >= (int64_t)F)
            throw std::invalid_argument("filter_of[" + std::to_string(i) + "] = " + std::to_string(f) + " is outside [-1, " +
                                        std::to_string(F) + ")");
        ++seg[(f < 0 ? F : (uint32_t)f) + 1];
    }
    for (uint32_t g = 0; g < F + 1; ++g) seg[g + 1] += seg[g];
    std::vector<uint32_t> at(seg, seg + F + 1);
    for (uint64_t i = 0; i < n; ++i) perm[at[filter_of[i] < 0 ? F : (uint32_t)filter_of[i]]++] = (uint32_t)i;
}

// One work item of the grouped scan as the planner states it (ExactItem is the device form).
struct ExactGroupItem {
    uint32_t seg, part;           // segment, part of the segment
    uint32_t c_lo, c_hi;          // candidates [c_lo, c_hi) of the segment
    uint32_t q_lo, q_cnt;         // queries [q_lo, q_lo + q_cnt) of the segment
    uint32_t pool;                // pool index inside the launch of (this part, query q_lo); query q_lo + i: pool + i
    uint32_t launch;
};
struct ExactGroupPlan {
    uint32_t Kp = 0, C = 0, gq = 0;
    std::vector<ExactGroupItem> items;        // ordered by (launch, segment, query group, part)
    std::vector<uint32_t> launch_items;       // [launches + 1]: launch l is items [launch_items[l], launch_items[l + 1])
    std::vector<uint32_t> launch_pools;       // [launches]: pools (of C keys) launch l uses
    std::vector<uint32_t> seg_parts;          // [segments]
    uint32_t max_pools = 0;
};

// Segment s: seg_m[s] candidates against seg_q[s] queries (one with no candidate or no query gets no item).  Every
// segment is cut into query groups of at most gq and into parts of whole 64-candidate blocks, at most kExactMaxParts.
// The parts are sized over ALL segments: about `waves` = two per SIMD work items of equal candidate-block count, so a
// small segment stays whole and a large one is cut as often as its share of the work says.  Pools: one per (part, query);
// a launch takes (segment, group) units in order while its pools fit the budget -- a unit whose parts alone would not
// fit gets fewer parts (one at least: like plan_exact, a budget below one group's pools is exceeded).
inline ExactGroupPlan plan_exact_groups(const uint64_t* seg_m, const uint64_t* seg_q, uint32_t n_seg, uint32_t k, int num_cus,
                                        size_t budget) {
    ExactGroupPlan pl;
    pl.Kp = 64;
    while (pl.Kp < k) pl.Kp <<= 1;
    pl.C = 2 * pl.Kp;
    pl.gq = 128;
    const uint64_t waves = (uint64_t)std::max(1, num_cus) * 8;
    const uint64_t budget_pools = std::max<uint64_t>(1, (uint64_t)budget / ((uint64_t)pl.C * 8));
    uint64_t total = 0;                       // candidate blocks x query groups
    for (uint32_t s = 0; s < n_seg; ++s)
        if (seg_m[s] && seg_q[s]) total += ((seg_m[s] + 63) / 64) * ((seg_q[s] + pl.gq - 1) / pl.gq);
    const uint64_t per = std::max<uint64_t>(1, (total + waves - 1) / waves);    // blocks per item
    pl.seg_parts.assign(n_seg, 0);
    pl.launch_items.push_back(0);
    uint64_t used = 0;
    uint32_t launch = 0;
    for (uint32_t s = 0; s < n_seg; ++s) {
        if (!seg_m[s] || !seg_q[s]) continue;
        const uint64_t m = seg_m[s], blocks = (m + 63) / 64, widest = std::min<uint64_t>(pl.gq, seg_q[s]);
        uint64_t want = std::min<uint64_t>({(blocks + per - 1) / per, blocks, (uint64_t)kExactMaxParts});
        want = std::max<uint64_t>(1, std::min<uint64_t>(want, budget_pools / widest));
        const uint32_t part = (uint32_t)((blocks + want - 1) / want * 64);
        const uint32_t P = (uint32_t)((m + part - 1) / part);
        pl.seg_parts[s] = P;
        for (uint64_t q0 = 0; q0 < seg_q[s]; q0 += pl.gq) {
            const uint32_t qc = (uint32_t)std::min<uint64_t>(pl.gq, seg_q[s] - q0);
            const uint64_t need = (uint64_t)P * qc;
            if (used && used + need > budget_pools) {
                pl.launch_items.push_back((uint32_t)pl.items.size());
                pl.launch_pools.push_back((uint32_t)used);
                used = 0;
                ++launch;
            }
            for (uint32_t p = 0; p < P; ++p)
                pl.items.push_back(ExactGroupItem{s, p, p * part, (uint32_t)std::min<uint64_t>(m, (uint64_t)(p + 1) * part), (uint32_t)q0, qc,
                                                  (uint32_t)(used + (uint64_t)p * qc), launch});
            used += need;
        }
    }
    if (used) {
        pl.launch_items.push_back((uint32_t)pl.items.size());
        pl.launch_pools.push_back((uint32_t)used);
    }
    for (uint32_t x : pl.launch_pools) pl.max_pools = std::max(pl.max_pools, x);
    return pl;
}

// Launches the <SD, CH> instantiation of a scan kernel (one wave per workgroup) that serves padded dimension D: the whole
// vector in registers at 128, 64 dimensions at a time at 1024, the generic 16 at any other.  Template arguments of the
// kernel behind <SD, CH> follow `args`.
#define CPH_LAUNCH_SCAN(KERNEL, D, grid, lds, st, args, ...)                                                           \
    do {                                                                                                               \
        if ((D) == 128) hipLaunchKernelGGL((KERNEL<128, 128, ##__VA_ARGS__>), grid, dim3(64), lds, st, args);          \
        else if ((D) == 1024) hipLaunchKernelGGL((KERNEL<1024, 64, ##__VA_ARGS__>), grid, dim3(64), lds, st, args);    \
        else hipLaunchKernelGGL((KERNEL<0, 16, ##__VA_ARGS__>), grid, dim3(64), lds, st, args);                        \
        HIP_CHECK(hipGetLastError());                                                                                  \
    } while (0)

}  // namespace cph
