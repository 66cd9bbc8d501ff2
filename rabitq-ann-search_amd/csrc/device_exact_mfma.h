// device_exact_mfma.h — the "matrix" engine of the exact scan (cph_set_exact_engine): the matrix cores discard every
// candidate that provably cannot be in a query's top-k, the eight-chain candidate loop of device_exact.h re-scores the few
// that remain.  Every output byte is the vector engine's: MFMA never PRODUCES a distance here, it only prunes.
//
// Three stages on one stream:
//   1. exact_mfma_prefilter_kernel   nq x m x D on v_mfma_f32_32x32x2_f32; per (part, query) a pool of the candidates whose
//                                    approximate distance d^ is within the slack of the k-th smallest seen so far
//   2. exact_mfma_certify_kernel     one wave per query: folds the parts' pools under the same keep rule, runs THE
//                                    candidate loop (exact_scan_candidates) over the survivors' ids, writes the row with the
//                                    merge code of the vector engine
//   3. exact_scan_flagged_kernel /   the vector engine's scan and merge for the queries stage 1 or 2 could not certify
//      exact_merge_flagged_kernel    (flags[q] != 0); a wave whose group has no flagged query leaves at once
//
// The bound.  u = 2^-24, gamma(n) = n u / (1 - n u).  For a pair (q, b) let Qn, Bn be the real squared norms,
// S = sum |q_i b_i| <= (Qn + Bn) / 2, qn and bn the STORED float norms (each an fmaf reduction of at most D terms, so
// Qn + Bn <= (qn + bn) / (1 - gamma(D + 3)) =: N'), and T = qn - 2 q.b + bn in real arithmetic -- the number BOTH paths round.
//   prefilter  s^ starts at -bn / 2 (halving is exact) and takes the D products two per instruction.  This repository's
//              host model of the instruction (host_knn.h, byte-equal to the kNN kernels in tests/test_gpu_knn.py) is a chain
//              of D fmaf, one rounding per product; the bound does NOT rest on that: it budgets TWO roundings per product
//              (a product rounded before it is added) and two to spare, 2 D + 2 on any term's way:
//              |s^ - (q.b - bn / 2)| <= gamma(2 D + 2) (S + bn / 2);
//              d^ = max(fma(-2, s^, qn), 0), one more rounding of a number of magnitude <= |T| + 2 gamma(2 D + 2) (S + bn / 2):
//              |d^ - max(T, 0)| <= 2 gamma(2 D + 2) N' (1 + u) + 2 u N'            (|T| <= qn + bn + 2 S <= 2 N')
//   vector     dot^: eight chains of D / 8 fmaf from 0 and a 3-add tree, D / 8 + 3 roundings on any product's way:
//              |dot^ - q.b| <= gamma(D / 8 + 3) S;  d = max(fl(fl(qn + bn) - 2 dot^), 0) (or the contracted fma, which rounds
//              less):  |d - max(T, 0)| <= u N' + gamma(D / 8 + 3) N' + u (2 N' + u N' + gamma(D / 8 + 3) N')
//   (clamping at 0 moves neither further from the other: |max(a, 0) - max(b, 0)| <= |a - b|.)
//   together   |d^ - d| <= N' (2 gamma(2 D + 2) + gamma(D / 8 + 3) + 5 u) (1 + u)  <=  (4.125 D + 24) u (qn + bn):
//              2 (2 D + 2) + D / 8 + 3 + 5 = 4.125 D + 12, and the 12 on top pay for 1 / (1 - n u), 1 / (1 - gamma) and (1 + u)
//              at every D <= 2048 (together below 4 u (qn + bn)).
// bn <= bn_max, the largest norm_sq of the index' rows (reduced once per index state, exact_mfma_bnmax_kernel), so
// eps(qn, bn_max, D) = exact_matrix_slack (host_exact_mfma.h) holds for every candidate of a query, and the kernel needs one
// number per query.  A loose bound only costs survivors.
//
// The keep rule.  tau = the k-th smallest d^ among candidates seen; a candidate is kept iff d^ <= tau + 2 eps (the sum
// rounded up).  k candidates have d <= tau + eps, a rejected one has d > tau + eps -- strictly, so ties in d cannot be lost,
// and a stale (larger) tau only keeps more.  A compaction sorts a pool, sets tau and keeps EVERY key within the limit, not
// just k; where those do not leave room for another append of a full wave the query cannot be certified from a pool of
// this size and is flagged.  So is a query whose qnorm, eps or any d^ is not finite.  Keys are d^ bits << 32 | id, as
// in device_exact.h (d^ >= +0: unsigned order is numeric order).
//
// Prefilter geometry.  Grid (P parts of the candidate list, tiles of 128 queries), 256 threads: wave w owns query rows
// 32 w .. 32 w + 31 of the tile and all 128 columns of a candidate tile, so a row's pool, fill count and limit are touched by
// one wave only.  Operand staging follows knn_mfma_kernel (device_knn.h): K in chunks of 32 floats through two LDS images
// of [128][36] floats per operand, one ds_read_b128 per lane feeding four MFMAs, software-pipelined at half-chunk
// granularity; accumulators start at -|b|^2 / 2.  What differs: the B rows are GATHERED (candidate c is ids[c]; the ids of
// the tile after the one being fetched are loaded a chunk ahead, so no row load waits for its id), columns behind the
// part's end repeat its last candidate and are masked in the epilogue (so every accumulator stays finite and a non-finite
// d^ means what it says), D = 16 zero-fills the upper half of the query's K chunk, and the per-row selection state is a
// pool in HBM of the capacity of ExactPoolSink (C = 2 Kp), compacted through a C-key LDS buffer of the wave's own.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>

#include "device_exact.h"
#include "device_knn.h"
#include "host_exact_mfma.h"

namespace cph {

constexpr uint32_t kMxTile = 128;          // query rows per workgroup, candidate columns per tile
constexpr uint32_t kMxKC = 32;             // floats of K per LDS stage
constexpr uint32_t kMxLd = kMxKC + 4;
constexpr uint32_t kMxInfBits = 0x7F800000u;
// The prefilter counts candidates in 32 bits, a whole tile past the last one included: a longer list (which no index of
// fewer than 2^32 - 1 rows of 64 bytes or more can hold in HBM today) is the vector engine's.
constexpr uint64_t kMxMaxCandidates = 0xFFFFFFFFull - kMxTile + 1;

// ---- per index state: bn_max; per batch: eps and the flags ----------------------------------------------------------------
// *out = the largest norm_sq[0 .. n) as bits.  norm_sq >= +0, so unsigned order is numeric order and a NaN (or +inf) beats
// every number: a row that is not finite leaves a bn_max that is not, and every query is flagged.  ONE workgroup and a
// plain store: a batch in flight on another stream reads the old value or the new, and both bound its candidates.
__global__ __launch_bounds__(1024) void exact_mfma_bnmax_kernel(const float* __restrict__ norm_sq, uint64_t n, uint32_t* out) {
    __shared__ uint32_t s_max[16];
    uint32_t mx = 0;
    for (uint64_t i = threadIdx.x; i < n; i += 1024) mx = max(mx, __float_as_uint(norm_sq[i]));
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w) mx = max(mx, s_max[w]);
        *out = mx;
    }
}

__global__ __launch_bounds__(256) void exact_mfma_query_kernel(const float* __restrict__ qnorm, const uint32_t* __restrict__ bn_max,
                                                               uint32_t D, uint32_t nq, float* __restrict__ eps, uint32_t* __restrict__ flags) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const float qn = qnorm[q], e = exact_matrix_slack(qn, __uint_as_float(*bn_max), D);
    eps[q] = e;
    flags[q] = (fabsf(qn) <= FLT_MAX && fabsf(e) <= FLT_MAX) ? 0u : 1u;
}

// ---- what the pools of both kernels share ---------------------------------------------------------------------------------
// Orders the LDS accesses of ONE wave across its lanes (a row's state belongs to one wave; a wave's LDS operations
// complete in program order, the fences keep the compiler from moving them).
__device__ __forceinline__ void mx_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// tau + 2 eps, rounded up (the sum rounds to nearest: one ulp of margin, two given).
__device__ __forceinline__ float mx_limit(float tau, float eps2) { return (tau + eps2) * 0x1.000004p+0f; }

// sm[0 .. cnt) -> sorted ascending (bitonic, exact_sort_keys with the barrier of one wave); returns how many keys the keep
// rule keeps -- all while there are fewer than k -- and through lim_bits the bits of the new limit.  Whole wave, converged.
__device__ __forceinline__ uint32_t mx_sort_keep(unsigned long long* sm, uint32_t cnt, uint32_t k, float eps2, int lane,
                                                 uint32_t& lim_bits) {
    uint32_t N = 64;
    while (N < cnt) N <<= 1;
    for (uint32_t i = cnt + lane; i < N; i += 64) sm[i] = kExactNoKey;
    mx_wave_sync();
    for (uint32_t kk = 2; kk <= N; kk <<= 1)
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < N / 2; i += 64) {
                const uint32_t lo = ((i & ~(j - 1u)) << 1) | (i & (j - 1u)), hi = lo | j;
                const bool up = (lo & kk) == 0;
                const unsigned long long x = sm[lo], y = sm[hi];
                if ((x > y) == up) { sm[lo] = y; sm[hi] = x; }
            }
            mx_wave_sync();
        }
    if (cnt < k) { lim_bits = kMxInfBits; return cnt; }
    lim_bits = __float_as_uint(mx_limit(__uint_as_float((uint32_t)(sm[k - 1] >> 32)), eps2));
    uint32_t kept = 0;
    for (uint32_t i = lane; i < N; i += 64) kept += (uint32_t)__popcll(__ballot(i < cnt && (uint32_t)(sm[i] >> 32) <= lim_bits));
    return kept;
}

// ---- the operand pipeline of a (part, query tile) workgroup -----------------------------------------------------------------
// What "Prefilter geometry" above describes, up to the tile epilogue: the loop over the part's candidate tiles and K chunks,
// for the kernels that differ only in what they do with a finished tile (range_mfma_kernel, device_range_mfma.h).
struct MxTileArgs {
    const float* raw;             // [n][D]
    const float* norm_sq;         // [n]
    const float* qpad;            // padded query rows
    const float* qnorm;
    const uint32_t* ids;          // LIST: the ascending id list
    uint32_t D;
    uint32_t c_lo, c_hi;          // the part's candidates, c_lo < c_hi
    uint32_t q_row0, q_last;      // the tile's first padded query row; the last row a clamped fetch may read
};

struct MxOperandLds {
    float Qs[2][kMxTile * kMxLd]; // double-buffered operand images
    float Bs[2][kMxTile * kMxLd];
    float bn_s[2][256];           // |b|^2 of the tile's columns, by tile parity (first 128 of each; the second 128: where
                                  //   fetches past the end are staged)
};

// Whole workgroup of 256, converged.  epi.begin(qn) once, behind the barrier that publishes image(0) (and whatever LDS the
// caller wrote before the call); epi.tile(tile, acc, qn) per finished tile: acc[t][i] = q.b - |b|^2 / 2 of (row wrow +
// (i & 3) + 8 (i >> 2) + 4 h, column 128 tile + 32 t + c), qn[i] the rows' stored norms.  Columns behind c_hi repeat the
// part's last candidate, rows behind q_last the last query: the epilogue masks both.
template <bool LIST, class Epilogue>
__device__ __forceinline__ void mx_scan_tiles(const MxTileArgs& a, MxOperandLds& L, Epilogue& epi) {
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int h = lane >> 5, c = lane & 31;
    const uint32_t D = a.D, c_lo = a.c_lo, c_hi = a.c_hi;
    const uint32_t nchunk = D < kMxKC ? 1u : D / kMxKC;
    const uint32_t ntile = (c_hi - c_lo + kMxTile - 1) / kMxTile;
    const uint32_t srow = tid >> 3, skq = (tid & 7) * 4;
    const bool kzero = skq >= D;
    const uint32_t skl = kzero ? 0u : skq;
    const float* qsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qsrc[i] = a.qpad + (size_t)min(a.q_row0 + srow + 32 * i, a.q_last) * D + skl;
    auto cand_id = [&](uint32_t tile, uint32_t r) -> uint32_t {
        const uint32_t cc = (uint32_t)min((uint64_t)c_lo + tile * kMxTile + r, (uint64_t)c_hi - 1);
        if constexpr (LIST) return a.ids[cc];
        else return cc;
    };
    knn_f32x4 pq[4], pb[4];
    float pbn = 0.0f;
    uint32_t f_tile = 0, f_ch = 0;
    uint32_t f_tile_staged = 0;
    bool f_past = false, f_past_staged = false;
    uint32_t rid[4], nid[4], bid, nbid;
#pragma unroll
    for (int i = 0; i < 4; ++i) { rid[i] = cand_id(0, srow + 32 * i); nid[i] = cand_id(1, srow + 32 * i); }
    bid = cand_id(0, tid & (kMxTile - 1));
    nbid = cand_id(1, tid & (kMxTile - 1));
    auto fetch = [&]() {
        const uint32_t k0 = f_ch * kMxKC;
        f_tile_staged = f_tile;
        f_past_staged = f_past;
        pbn = a.norm_sq[bid];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const knn_f32x4 x = *reinterpret_cast<const knn_f32x4*>(qsrc[i] + k0);
            pq[i] = kzero ? knn_f32x4{0.0f, 0.0f, 0.0f, 0.0f} : x;
            pb[i] = *reinterpret_cast<const knn_f32x4*>(a.raw + (size_t)rid[i] * D + skl + k0);
        }
        const bool wrap = f_ch + 1 == nchunk;
        f_past = f_past || (wrap && f_tile + 1 == ntile);
        f_ch = wrap ? 0 : f_ch + 1;
        f_tile = (wrap && f_tile + 1 < ntile) ? f_tile + 1 : f_tile;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rid[i] = wrap ? nid[i] : rid[i];
            nid[i] = cand_id(f_tile + 1, srow + 32 * i);
        }
        bid = wrap ? nbid : bid;
        nbid = cand_id(f_tile + 1, tid & (kMxTile - 1));
    };
    auto stage = [&](int buf) {
        L.bn_s[f_tile_staged & 1][f_past_staged ? (tid | 128) : tid] = pbn;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<knn_f32x4*>(&L.Qs[buf][(srow + 32 * i) * kMxLd + skq]) = pq[i];
            *reinterpret_cast<knn_f32x4*>(&L.Bs[buf][(srow + 32 * i) * kMxLd + skq]) = pb[i];
        }
    };
    const int wrow = wave * 32;
    struct Ops { knn_f32x4 av[2], bv[2][4]; };
    auto read_ops = [&](int buf, int half, Ops& o) {
        const float* Qb = L.Qs[buf];
        const float* Bb = L.Bs[buf];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = 2 * half + jj;
            o.av[jj] = *reinterpret_cast<const knn_f32x4*>(&Qb[(wrow + c) * kMxLd + 8 * j + 4 * h]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                o.bv[jj][t] = *reinterpret_cast<const knn_f32x4*>(&Bb[(t * 32 + c) * kMxLd + 8 * j + 4 * h]);
        }
    };
    knn_f32x16 acc[4];
    auto mfma_half = [&](const Ops& o) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.av[jj].x, o.bv[jj][t].x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.av[jj].y, o.bv[jj][t].y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.av[jj].z, o.bv[jj][t].z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.av[jj].w, o.bv[jj][t].w, acc[t], 0, 0, 0);
            }
        }
    };
    float qn[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) qn[i] = a.qnorm[min(a.q_row0 + (uint32_t)(wrow + (i & 3) + 8 * (i >> 2) + 4 * h), a.q_last)];

    Ops op0, op1;
    fetch();
    stage(0);
    fetch();
    __syncthreads();
    epi.begin(qn);
    read_ops(0, 0, op0);
    int buf = 0;
    constexpr int kVmemGroups = LIST ? 13 : 9;
    for (uint32_t tile = 0; tile < ntile; ++tile)
    for (uint32_t ch = 0; ch < nchunk; ++ch) {
        if (ch == 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float init = -0.5f * L.bn_s[tile & 1][t * 32 + c];
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[t][i] = init;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        read_ops(buf, 1, op1);
        stage(buf ^ 1);
        fetch();
        mfma_half(op0);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write
        }
#pragma unroll
        for (int i = 0; i < kVmemGroups; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);   // VALU (addresses of the fetch)
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
        }
        if constexpr (kVmemGroups < 13) __builtin_amdgcn_sched_group_barrier(0x008, 13 - kVmemGroups, 0);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        buf ^= 1;
        read_ops(buf, 0, op0);
        mfma_half(op1);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 22, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (ch + 1 != nchunk) continue;
        epi.tile(tile, acc, qn);
    }
}

// ---- 1. the prefilter -------------------------------------------------------------------------------------------------------
struct MatrixArgs {
    const float* raw;             // [n][D]
    const float* norm_sq;         // [n]
    const float* qpad;            // [>= nq][D]
    const float* qnorm;           // [nq]
    const float* eps;             // [nq]
    const uint32_t* ids;          // [m] ascending internal ids (LIST), or null: candidate c is id c
    uint32_t m, D;                // candidates; padded dimension
    uint64_t part;                // candidates per part (a multiple of 128; 2^32 where one part holds 2^32 - 1 candidates)
    uint32_t nq, q_first, q_count;// the batch; the queries of this launch
    uint32_t k, C;
    unsigned long long* pools;    // [P][q_count][C]
    uint32_t* counts;             // [P][q_count]
    uint32_t* flags;              // [nq]
};

// Grid (P, ceil(q_count / 128)); dynamic LDS: 4 x C keys (a compaction buffer per wave).
template <bool LIST>
__global__ __launch_bounds__(256, 1) void exact_mfma_prefilter_kernel(MatrixArgs a) {
    __shared__ __align__(16) float Qs[2][kMxTile * kMxLd];       // double-buffered operand images
    __shared__ __align__(16) float Bs[2][kMxTile * kMxLd];
    __shared__ float bn_s[2][256];                               // |b|^2 of the tile's columns, by tile parity (first 128 of each;
                                                                 //   the second 128: where fetches past the end are staged)
    __shared__ uint32_t cnt[kMxTile];                            // per query row: keys in its pool,
    __shared__ float lim_s[kMxTile];                             //   its limit tau + 2 eps (-1: takes nothing),
    __shared__ float eps2_s[kMxTile];                            //   2 eps
    extern __shared__ __align__(16) unsigned char mx_smem[];

    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int h = lane >> 5, c = lane & 31;
    const uint64_t p_lo = (uint64_t)blockIdx.x * a.part;          // (64 bits: the last part's end may pass 2^32)
    const uint32_t c_lo = (uint32_t)min(p_lo, (uint64_t)a.m), c_hi = (uint32_t)min(p_lo + a.part, (uint64_t)a.m);
    const uint32_t ql0 = blockIdx.y * kMxTile;                   // first query of the tile, relative to q_first
    if (c_lo >= c_hi || ql0 >= a.q_count) return;
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(mx_smem) + (size_t)wave * a.C;
    const float INF = __builtin_inff();
    if (tid < (int)kMxTile) {
        const uint32_t ql = ql0 + (uint32_t)tid;
        const bool live = ql < a.q_count && a.flags[a.q_first + ql] == 0;        // (a flagged query is the fallback's)
        cnt[tid] = 0;
        lim_s[tid] = live ? INF : -1.0f;
        eps2_s[tid] = live ? 2.0f * a.eps[a.q_first + ql] : 0.0f;
    }

    const uint32_t D = a.D;
    const uint32_t nchunk = D < kMxKC ? 1u : D / kMxKC;
    const uint32_t ntile = (c_hi - c_lo + kMxTile - 1) / kMxTile;
    const uint32_t q_last = a.q_first + a.q_count - 1;

    // Staging: 4 x 16 B per operand per thread and chunk; element e = tid + 256 i -> row e >> 3, float4 e & 7 of the chunk.
    // Rows behind the end are clamped, not predicated (no branches between the MFMAs): a clamped query row's limit is -1,
    // a clamped candidate's column is masked in the epilogue.  D = 16: the float4s 4 .. 7 of the query chunk are zero (and
    // the candidate's are the row's first, any finite numbers).
    const uint32_t srow = tid >> 3, skq = (tid & 7) * 4;
    const bool kzero = skq >= D;
    const uint32_t skl = kzero ? 0u : skq;
    const float* qsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qsrc[i] = a.qpad + (size_t)min(a.q_first + ql0 + srow + 32 * i, q_last) * D + skl;
    // candidate (tile, r) of this part -> internal id
    auto cand_id = [&](uint32_t tile, uint32_t r) -> uint32_t {
        // (64 bits: the ids fetched ahead for the tile after the last one may pass 2^32 before the clamp)
        const uint32_t cc = (uint32_t)min((uint64_t)c_lo + tile * kMxTile + r, (uint64_t)c_hi - 1);
        if constexpr (LIST) return a.ids[cc];
        else return cc;
    };
    knn_f32x4 pq[4], pb[4];
    float pbn = 0.0f;                   // |b|^2 of column (tid & 127) of the tile being fetched
    uint32_t f_tile = 0, f_ch = 0;      // the chunk the next fetch() brings in (past the end: the last tile again, unused)
    uint32_t f_tile_staged = 0;
    bool f_past = false, f_past_staged = false;   // the fetch runs past the part's last chunk: its norms go to the spare half of bn_s
    uint32_t rid[4], nid[4], bid, nbid; // ids of the rows this thread stages, and of its norm column: the tile being fetched, the one after
#pragma unroll
    for (int i = 0; i < 4; ++i) { rid[i] = cand_id(0, srow + 32 * i); nid[i] = cand_id(1, srow + 32 * i); }
    bid = cand_id(0, tid & (kMxTile - 1));
    nbid = cand_id(1, tid & (kMxTile - 1));
    auto fetch = [&]() {
        const uint32_t k0 = f_ch * kMxKC;
        f_tile_staged = f_tile;
        f_past_staged = f_past;
        pbn = a.norm_sq[bid];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const knn_f32x4 x = *reinterpret_cast<const knn_f32x4*>(qsrc[i] + k0);
            pq[i] = kzero ? knn_f32x4{0.0f, 0.0f, 0.0f, 0.0f} : x;
            pb[i] = *reinterpret_cast<const knn_f32x4*>(a.raw + (size_t)rid[i] * D + skl + k0);
        }
        const bool wrap = f_ch + 1 == nchunk;
        f_past = f_past || (wrap && f_tile + 1 == ntile);
        f_ch = wrap ? 0 : f_ch + 1;
        f_tile = (wrap && f_tile + 1 < ntile) ? f_tile + 1 : f_tile;
        // (every chunk, no branch: a half is one basic block)  nid was loaded a fetch ago for the tile that is now f_tile
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rid[i] = wrap ? nid[i] : rid[i];
            nid[i] = cand_id(f_tile + 1, srow + 32 * i);
        }
        bid = wrap ? nbid : bid;
        nbid = cand_id(f_tile + 1, tid & (kMxTile - 1));
    };
    auto stage = [&](int buf) {         // what fetch() brought in -> image `buf` (and its tile's column norms)
        // A fetch past the end repeats the last tile's number with the ids of a tile that does not exist.  With one chunk per
        // tile (D <= 32) it is staged in the iteration that reads bn_s of the same parity, with no barrier in between: a wave
        // still in the epilogue of the tile before would start the last tile from another row's norm.  Such a fetch writes the
        // half of bn_s nobody reads (no branch: a half is one basic block).
        bn_s[f_tile_staged & 1][f_past_staged ? (tid | 128) : tid] = pbn;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<knn_f32x4*>(&Qs[buf][(srow + 32 * i) * kMxLd + skq]) = pq[i];
            *reinterpret_cast<knn_f32x4*>(&Bs[buf][(srow + 32 * i) * kMxLd + skq]) = pb[i];
        }
    };
    const int wrow = wave * 32;         // first tile row of this wave
    // operand registers of half a chunk: lane (h, c) reads its row's k = 8j + 4h .. + 3 for j = 2 half, 2 half + 1
    struct Ops { knn_f32x4 av[2], bv[2][4]; };
    auto read_ops = [&](int buf, int half, Ops& o) {
        const float* Qb = Qs[buf];
        const float* Bb = Bs[buf];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = 2 * half + jj;
            o.av[jj] = *reinterpret_cast<const knn_f32x4*>(&Qb[(wrow + c) * kMxLd + 8 * j + 4 * h]);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                o.bv[jj][t] = *reinterpret_cast<const knn_f32x4*>(&Bb[(t * 32 + c) * kMxLd + 8 * j + 4 * h]);
        }
    };
    knn_f32x16 acc[4];
    auto mfma_half = [&](const Ops& o) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.av[jj].x, o.bv[jj][t].x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.av[jj].y, o.bv[jj][t].y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.av[jj].z, o.bv[jj][t].z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(o.av[jj].w, o.bv[jj][t].w, acc[t], 0, 0, 0);
            }
        }
    };
    // this lane's 16 rows (C/D layout of the 32x32 MFMA: element i is row wrow + (i & 3) + 8 (i >> 2) + 4 h): norms, limits
    float qn[16], lm[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
        qn[i] = a.qnorm[min(a.q_first + ql0 + (uint32_t)(wrow + (i & 3) + 8 * (i >> 2) + 4 * h), q_last)];

    // prologue: image(0) staged and published, chunk 1 in flight, first-half operands of chunk 0 in registers
    Ops op0, op1;
    fetch();
    stage(0);
    fetch();
    __syncthreads();                    // image(0) and the row state are in place
#pragma unroll
    for (int i = 0; i < 16; ++i) lm[i] = lim_s[wrow + (i & 3) + 8 * (i >> 2) + 4 * h];
    read_ops(0, 0, op0);
    int buf = 0;
    constexpr int kVmemGroups = LIST ? 13 : 9;     // loads of a fetch: 8 rows and a norm, with a list 5 ids more (4 fit)
    for (uint32_t tile = 0; tile < ntile; ++tile)
    for (uint32_t ch = 0; ch < nchunk; ++ch) {
        if (ch == 0) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float init = -0.5f * bn_s[tile & 1][t * 32 + c];
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[t][i] = init;
            }
        }
        // ---- first half: MFMAs on op0; behind them op1 of this chunk, the staging of the next chunk, the fetch of the
        // one after
        __builtin_amdgcn_sched_barrier(0);
        read_ops(buf, 1, op1);
        stage(buf ^ 1);
        fetch();
        mfma_half(op0);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // DS read
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // DS write
        }
#pragma unroll
        for (int i = 0; i < kVmemGroups; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);   // VALU (addresses of the fetch)
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);   // VMEM read
        }
        if constexpr (kVmemGroups < 13) __builtin_amdgcn_sched_group_barrier(0x008, 13 - kVmemGroups, 0);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        buf ^= 1;
        // ---- second half: MFMAs on op1; behind them the first-half operands of the next chunk
        read_ops(buf, 0, op0);
        mfma_half(op1);
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 22, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (ch + 1 != nchunk) continue;

        // ---- tile finished: its 4 x (32 x 32) approximate distances against the rows' limits ----------------------------
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t col = c_lo + tile * kMxTile + t * 32 + c;     // this lane's candidate
            const bool ok = col < c_hi;
            // "is any of my 16 distances within its row's limit" as one max-reduction (sign of lim - d^ is exact), "is any
            // of them not finite" as one fma chain (x * 0 is 0 for every finite x, NaN otherwise)
            float dh[16], lead = -1.0f, z = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float d = __fmaf_rn(-2.0f, acc[t][i], qn[i]);
                z = __fmaf_rn(d, 0.0f, z);
                dh[i] = d > 0.0f ? d : 0.0f;
                lead = __builtin_fmaxf(lead, lm[i] - dh[i]);
            }
            if (__any(ok && !(z == 0.0f))) {                             // (rare) flag the rows that own them
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (ok && !(fabsf(__fmaf_rn(-2.0f, acc[t][i], qn[i])) <= FLT_MAX))
                        a.flags[min(a.q_first + ql0 + (uint32_t)(wrow + (i & 3) + 8 * (i >> 2) + 4 * h), q_last)] = 1u;
            }
            if (!__any(ok && lead >= 0.0f)) continue;
            const uint32_t id = cand_id(tile, t * 32 + c);
            bool compacted = false;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int rlo = wrow + (i & 3) + 8 * (i >> 2);
                const bool pass = ok && dh[i] <= lm[i];
                if (__ballot(pass) == 0) continue;
                const unsigned long long key = ((unsigned long long)__float_as_uint(dh[i]) << 32) | id;
                // the 32 lanes of a half share the row; the two halves take their turns (wave-uniform)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int rr = rlo + 4 * hh;
                    bool mine = pass && h == hh;
                    uint32_t mh = (uint32_t)(__ballot(mine) >> (32 * hh));
                    if (mh == 0) continue;
                    uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt[rr]);
                    unsigned long long* pool = a.pools + ((size_t)blockIdx.x * a.q_count + ql0 + rr) * a.C;
                    if (base + __popc(mh) > a.C) {
                        // the pool is full: sort, set tau, keep what the rule keeps, and look again
                        __threadfence();                         // the appended keys, written by single lanes, are visible
                        for (uint32_t x = lane; x < base; x += 64) sm[x] = pool[x];
                        uint32_t lb;
                        uint32_t kept = mx_sort_keep(sm, base, a.k, eps2_s[rr], lane, lb);
                        float nl = __uint_as_float(lb);
                        if (kept + 64 > a.C) {                   // no room for the next append: not certifiable here
                            if (lane == 0) a.flags[a.q_first + ql0 + rr] = 1u;
                            kept = 0;
                            nl = -1.0f;
                        }
                        for (uint32_t x = lane; x < kept; x += 64) pool[x] = sm[x];
                        if (lane == 0) lim_s[rr] = nl;
                        mx_wave_sync();
                        compacted = true;
                        mine = mine && dh[i] <= nl;
                        mh = (uint32_t)(__ballot(mine) >> (32 * hh));
                        base = kept;
                    }
                    if (mine) pool[base + __popc(mh & ((1u << c) - 1u))] = key;
                    if (lane == 0) cnt[rr] = base + __popc(mh);
                    mx_wave_sync();
                }
            }
            if (compacted) {
#pragma unroll
                for (int i = 0; i < 16; ++i) lm[i] = lim_s[wrow + (i & 3) + 8 * (i >> 2) + 4 * h];
            }
        }
    }
    // ---- the part is done: every pool of this wave cut once more; its fill count published ---------------------------------
    for (int r = 0; r < 32; ++r) {
        const uint32_t ql = ql0 + (uint32_t)(wrow + r);
        if (ql >= a.q_count) break;
        const size_t pi = (size_t)blockIdx.x * a.q_count + ql;
        unsigned long long* pool = a.pools + pi * a.C;
        uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt[wrow + r]);
        if (n > a.k) {
            __threadfence();
            for (uint32_t x = lane; x < n; x += 64) sm[x] = pool[x];
            uint32_t lb;
            n = mx_sort_keep(sm, n, a.k, eps2_s[wrow + r], lane, lb);
            for (uint32_t x = lane; x < n; x += 64) pool[x] = sm[x];
            mx_wave_sync();
        }
        if (lane == 0) a.counts[pi] = n;
    }
}

// ---- 2. certify and re-score --------------------------------------------------------------------------------------------------
// One query certified by one wave: the pools of its P parts (part p's is pool index first + p * stride) folded under the keep
// rule, the survivors through THE candidate loop into the query's one re-score pool (index ql of rpools / rcounts), the row
// to out row `out_row`.  q: the query's padded row (and its index in eps and flags).  LDS: C keys + 2 x kExactQT words (the
// ExactPoolSink of a group of kExactQT), C ids.  Shared by the certify kernels of the plain and the grouped scan.
struct MatrixCertifyCommon {
    ScanCommon s;                 // (gq, part, q_first, q_count: unused here)
    const float* eps;             // [nq]
    uint32_t k, C;
    const unsigned long long* pools;   // the prefilter's
    const uint32_t* counts;
    unsigned long long* rpools;   // [queries of the launch][C]      the re-score's: one list per query
    uint32_t* rcounts;            // [queries of the launch]
    uint32_t* flags;              // [nq]
    unsigned long long* stats;
    const uint32_t* rows;         // the row map, or null
    int64_t* out_ids;
    float* out_dist;
};

template <int SD, int CH>
__device__ __forceinline__ void mx_certify_query(const MatrixCertifyCommon& a, size_t first, uint32_t stride, uint32_t P, uint32_t ql,
                                                 uint32_t q, size_t out_row, unsigned char* smem) {
    const int lane = threadIdx.x;
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    if (a.flags[q]) return;                                       // (only this wave ever flags q from here on)
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    uint32_t* s_ids = reinterpret_cast<uint32_t*>(smem + (size_t)a.C * 8 + 2 * kExactQT * 4);
    const float eps2 = 2.0f * a.eps[q];
    // the fold: every part's keys past the running limit into one pool of C keys, cut by the keep rule when it is full
    uint32_t cnt = 0, lim = kMxInfBits;
    for (uint32_t p = 0; p < P; ++p) {
        const size_t pi = first + (size_t)p * stride;
        const uint32_t np = a.counts[pi];
        const unsigned long long* pool = a.pools + pi * a.C;
        for (uint32_t base = 0; base < np; base += 64) {
            const uint32_t i = base + lane;
            const unsigned long long key = i < np ? pool[i] : kExactNoKey;
            bool pass = i < np && (uint32_t)(key >> 32) <= lim;
            unsigned long long mask = __ballot(pass);
            if (mask == 0) continue;
            if (cnt + (uint32_t)__popcll(mask) > a.C) {
                cnt = mx_sort_keep(sm, cnt, a.k, eps2, lane, lim);
                if (cnt + 64 > a.C) {                             // the survivors do not fit: the fallback's query
                    if (lane == 0) a.flags[q] = 1u;
                    return;
                }
                pass = pass && (uint32_t)(key >> 32) <= lim;
                mask = __ballot(pass);
            }
            if (pass) sm[cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = key;
            cnt += (uint32_t)__popcll(mask);
            mx_wave_sync();
        }
    }
    cnt = mx_sort_keep(sm, cnt, a.k, eps2, lane, lim);
    for (uint32_t i = lane; i < cnt; i += 64) s_ids[i] = (uint32_t)sm[i];
    if (lane == 0) atomicAdd(a.stats + kStatMatrixSurvivors, (unsigned long long)cnt);
    __syncthreads();
    // the survivors through THE candidate loop, one live query: the bytes are formed where every exact distance is
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, ExactListSource{s_ids}, 0u, cnt, (exact_uniform_ptr)(a.s.qpad + (size_t)q * D),
                                  (exact_uniform_ptr)(a.s.qnorm + q), 1u,
                                  ExactPoolSink(smem, kExactQT, a.rpools + (size_t)ql * a.C, a.rcounts + ql, a.k, a.C));
    __threadfence();
    __syncthreads();
    exact_merge_query(a.rpools, a.rcounts, ql, 1u, 1u, a.k, a.C, a.rows, a.out_ids, a.out_dist, out_row, smem);
}

struct MatrixCertifyArgs {
    MatrixCertifyCommon c;        // (c.s.q_first, c.s.q_count: the queries of this launch; pools [P][q_count][C], counts [P][q_count])
    uint32_t P;
};

// One wave per query of the launch.
template <int SD, int CH>
__global__ __launch_bounds__(64) void exact_mfma_certify_kernel(MatrixCertifyArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t ql = blockIdx.x, q = a.c.s.q_first + ql;
    mx_certify_query<SD, CH>(a.c, ql, a.c.s.q_count, a.P, ql, q, q, smem);
}

// ---- 3. the fallback: the vector engine's scan and merge, for flagged queries only ---------------------------------------------
struct ExactFlaggedArgs {
    ExactArgs a;
    const uint32_t* flags;        // [nq]
};

template <int SD, int CH>
__global__ __launch_bounds__(64) void exact_scan_flagged_kernel(ExactFlaggedArgs f) {
    extern __shared__ __align__(16) unsigned char smem[];
    const ExactArgs& a = f.a;
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    const ScanCut c = scan_cut(a.s, a.m, D);
    if (c.c_lo >= c.c_hi || c.ql_lo >= c.ql_hi) return;
    bool any = false;
    for (uint32_t ql = c.ql_lo + threadIdx.x; ql < c.ql_hi; ql += 64) any = any || f.flags[a.s.q_first + ql] != 0;
    if (!__any(any)) return;
    const size_t pool = (size_t)blockIdx.x * a.s.q_count + c.ql_lo;
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, ExactListSource{a.ids}, c.c_lo, c.c_hi, c.q_rows, c.q_norms, c.ql_hi - c.ql_lo,
                                  ExactPoolSink(smem, a.s.gq, a.pools + pool * a.C, a.counts + pool, a.k, a.C));
}

__global__ __launch_bounds__(64) void exact_merge_flagged_kernel(const unsigned long long* __restrict__ pools, const uint32_t* __restrict__ counts,
                                                                 uint32_t P, uint32_t q_first, uint32_t q_count, uint32_t k, uint32_t C,
                                                                 const uint32_t* __restrict__ rows, const uint32_t* __restrict__ flags,
                                                                 unsigned long long* stats, int64_t* __restrict__ out_ids,
                                                                 float* __restrict__ out_dist) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (!flags[q_first + blockIdx.x]) return;
    if (threadIdx.x == 0) atomicAdd(stats + kStatMatrixRedo, 1ull);
    exact_merge_query(pools, counts, blockIdx.x, q_count, P, k, C, rows, out_ids, out_dist, (size_t)q_first + blockIdx.x, smem);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// How a matrix batch is cut: launches of tile_q queries (a multiple of 128 unless it is the whole batch), each a grid of
// P parts x tiles of 128 queries.  One workgroup per CU is resident (LDS), so two workgroups per CU are asked for: many parts
// when there are few query tiles, few when the tiles alone fill the GPU.  Scratch above `budget` bytes: fewer queries per
// launch first, then fewer parts.
struct MatrixPlan {
    uint32_t Kp, C;
    uint32_t tile_q;
    uint32_t P;
    uint64_t part;        // (2^32 where one part holds more than 2^32 - 128 candidates)
    size_t pool_keys;     // P * tile_q * C
};

inline MatrixPlan plan_exact_matrix(uint64_t m, uint32_t nq, uint32_t k, int num_cus, size_t budget) {
    MatrixPlan pl{};
    pl.Kp = 64;
    while (pl.Kp < k) pl.Kp <<= 1;
    pl.C = 2 * pl.Kp;
    const uint64_t wgs = (uint64_t)std::max(1, num_cus) * 2, blocks = (m + kMxTile - 1) / kMxTile;
    auto parts = [&](uint64_t want) {
        want = std::max<uint64_t>(1, std::min<uint64_t>({want, blocks, (uint64_t)kExactMaxParts}));
        pl.part = (blocks + want - 1) / want * kMxTile;
        pl.P = (uint32_t)((m + pl.part - 1) / pl.part);
        pl.pool_keys = (size_t)pl.P * pl.tile_q * pl.C;
    };
    pl.tile_q = nq;
    for (;;) {
        const uint64_t T = (pl.tile_q + kMxTile - 1) / kMxTile;
        parts((wgs + T - 1) / T);
        if (pl.pool_keys * 8 <= budget || pl.tile_q <= kMxTile) break;
        pl.tile_q = std::max<uint32_t>(kMxTile, (pl.tile_q / 2 + kMxTile - 1) / kMxTile * kMxTile);
    }
    if (pl.pool_keys * 8 > budget) parts(budget / ((size_t)pl.tile_q * pl.C * 8));
    return pl;
}

}  // namespace cph
