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
__global__ __launch_bounds__(64) void exact_pad_kernel(const float* __restrict__ q, uint32_t nq, uint32_t nq_pad, uint32_t dim,
                                                       uint32_t D, float* __restrict__ qpad, float* __restrict__ qnorm,
                                                       unsigned long long* stats, unsigned long long n_exact) {
    __shared__ float s_q[2048];
    const int lane = threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) stats[kStatExact] = n_exact;
    for (uint32_t qi = blockIdx.x; qi < nq_pad; qi += gridDim.x) {
        for (uint32_t d = lane; d < D; d += 64) {
            const float x = (qi < nq && d < dim) ? q[(size_t)qi * dim + d] : 0.0f;
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

// ---- the scan ---------------------------------------------------------------------------------------------------------
struct ExactArgs {
    const float* raw;             // [n][D]
    const float* norm_sq;         // [n]
    const uint32_t* ids;          // [m] ascending internal ids, or null: candidate c is id c
    uint32_t m;                   // candidates
    uint32_t D;
    const float* qpad;            // [nq_pad][D]
    const float* qnorm;           // [nq_pad]
    uint32_t q_first, q_count;    // the queries of this launch
    uint32_t gq;                  // queries per group (a multiple of kExactQT)
    uint32_t part;                // candidates per part (a multiple of 64)
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

// SD: compile-time padded dimension (0: a.D, any power of two 16..2048); CH: dimensions a lane holds at a time (CH == SD:
// the whole vector, loaded once per 64 candidates).  Grid (P, G), one wave per workgroup; LDS: C keys + 2 gq words.
template <int SD, int CH>
__global__ __launch_bounds__(64) void exact_scan_kernel(ExactArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    uint32_t* s_thr = reinterpret_cast<uint32_t*>(sm + a.C);
    uint32_t* s_cnt = s_thr + a.gq;
    const int lane = threadIdx.x;
    const uint32_t D = SD ? (uint32_t)SD : a.D;
    const uint32_t p = blockIdx.x;
    const uint32_t c_lo = p * a.part, c_hi = min(a.m, c_lo + a.part);
    const uint32_t ql_lo = blockIdx.y * a.gq, ql_hi = min(a.q_count, ql_lo + a.gq);   // relative to q_first
    if (c_lo >= c_hi || ql_lo >= ql_hi) return;
    for (uint32_t i = lane; i < a.gq; i += 64) { s_thr[i] = 0xFFFFFFFFu; s_cnt[i] = 0; }
    __syncthreads();
    const exact_uniform_ptr qbase = (exact_uniform_ptr)(a.qpad + (size_t)(a.q_first + ql_lo) * D);
    const exact_uniform_ptr qnorms = (exact_uniform_ptr)(a.qnorm + a.q_first + ql_lo);
    unsigned long long* const pools = a.pools + ((size_t)p * a.q_count + ql_lo) * a.C;
    const uint32_t k = a.k, C = a.C;

    for (uint32_t cb = c_lo; cb < c_hi; cb += 64) {
        const bool valid = cb + lane < c_hi;
        const uint32_t cc = valid ? cb + lane : c_hi - 1;
        const uint32_t id = a.ids ? a.ids[cc] : cc;
        const float* __restrict__ row = a.raw + (size_t)id * D;
        const float nrm = a.norm_sq[id];
        float v[CH];
        if constexpr (SD == CH) exact_load_chunk<CH>(row, v);
        for (uint32_t qt = 0; qt < ql_hi - ql_lo; qt += kExactQT) {
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
                if (ql >= ql_hi - ql_lo) break;                    // (wave-uniform: the zero rows of the last tile)
                const float dot = ((acc[t][0] + acc[t][4]) + (acc[t][1] + acc[t][5])) + ((acc[t][2] + acc[t][6]) + (acc[t][3] + acc[t][7]));
                const uint32_t dbits = __float_as_uint(exact_from_dot(qnorms[ql], nrm, dot));
                const bool pass = valid && dbits <= s_thr[ql];
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
    for (uint32_t ql = 0; ql < ql_hi - ql_lo; ++ql) {
        uint32_t cnt = s_cnt[ql], thr;
        if (cnt) cnt = exact_compact(sm, pools + (size_t)ql * C, cnt, k, lane, thr);
        if (lane == 0) a.counts[(size_t)p * a.q_count + ql_lo + ql] = cnt;
    }
}

// One wave per query of the launch: the P sorted part lists -> out rows [k], ascending, ids through `rows` if given,
// padded with -1 / FLT_MAX.  LDS: C keys: the lower half holds the Kp smallest keys so far, ascending; a part's list is
// laid behind it in descending order and one bitonic merge (log C stages, not a sort) leaves all C ascending again.
__global__ __launch_bounds__(64) void exact_merge_kernel(const unsigned long long* __restrict__ pools, const uint32_t* __restrict__ counts,
                                                         uint32_t P, uint32_t q_first, uint32_t q_count, uint32_t k, uint32_t C,
                                                         const uint32_t* __restrict__ rows, int64_t* __restrict__ out_ids,
                                                         float* __restrict__ out_dist) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x, Kp = C / 2;
    for (uint32_t i = lane; i < Kp; i += 64) sm[i] = kExactNoKey;
    for (uint32_t p = 0; p < P; ++p) {
        const uint32_t cnt = counts[(size_t)p * q_count + q];       // <= k <= Kp
        const unsigned long long* pool = pools + ((size_t)p * q_count + q) * C;
        for (uint32_t i = lane; i < Kp; i += 64) sm[C - 1 - i] = i < cnt ? pool[i] : kExactNoKey;
        __syncthreads();
        exact_merge_keys(sm, C, lane);
    }
    __syncthreads();
    const size_t o = (size_t)(q_first + q) * k;
    for (uint32_t i = lane; i < k; i += 64) {
        const unsigned long long key = sm[i];
        const bool have = key != kExactNoKey;
        const uint32_t id = (uint32_t)key;
        out_ids[o + i] = have ? (int64_t)(rows ? rows[id] : id) : (int64_t)-1;
        out_dist[o + i] = have ? __uint_as_float((uint32_t)(key >> 32)) : FLT_MAX;
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

inline void launch_exact_scan(uint32_t D, dim3 grid, size_t lds, hipStream_t st, const ExactArgs& a) {
    if (D == 128) hipLaunchKernelGGL((exact_scan_kernel<128, 128>), grid, dim3(64), lds, st, a);
    else if (D == 1024) hipLaunchKernelGGL((exact_scan_kernel<1024, 64>), grid, dim3(64), lds, st, a);
    else hipLaunchKernelGGL((exact_scan_kernel<0, 16>), grid, dim3(64), lds, st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
