// device_fused.h — fused search (cph_search_fused*): several query vectors per query, the k best rows by the exact weighted sum
// of their distances to all of them.
//
// The statement is host_fused.h's.  Three kernels behind the ordinary search at k = C and exact_pad_kernel, on one stream:
//   union    fused_union_kernel: one 256-thread workgroup per query, over the E = L * C entries of the query's live rows and
//            P = the power of two >= max(E, 64).  A valid entry (0 <= id < n_ids) becomes the 64-bit word  id << 32 | t ,
//            everything else the all-ones word, which no entry has.  The bitonic sort of device_wg_primitives.h orders them by
//            (id, vector); a segment of equal high halves is one candidate, the distinct low halves inside it are its hits.
//            Segment heads and (id, vector) run heads by neighbour compares; every wave counts the heads of its quarter with
//            ballots, the four totals give the offsets, a second walk writes u_ids[segment] (ascending) and the index of every
//            segment's first run; hits = the difference of two neighbours of that array.  u_count = the segments.
//            LDS (fused_union_lds): 10 bytes per element of P plus 36: 80 KiB at P = 8,192.
//   scan     fused_scan_kernel<SD, CH>: a work item is (query i, G consecutive blocks of kFusedItemSlots = 64 union slots), one
//            wave; it stops at the first block at or behind u_count[i].  G is 1 while n * blocks stays at or below
//            kFusedScanGrid and grows with the batch from there, up to all blocks of a query: the union is far smaller than
//            T * C on real data, and a workgroup that only finds that out costs as much to dispatch as one that works
//            (measured: the kernel's time was 6.6 ns x the grid, profiles/fused_search.md).
//            The work is device_exact.h's candidate loop, exact_scan_candidates, with the list source over u_ids (everything allowed: the search applied filter and tombstones) and a sink that forms the
//            weighted sum: the arithmetic, and so every distance bit, is cph_exact_l2's.  The loop hands the sink one block of
//            64 candidates with ql ascending from 0 to L - 1 before it moves on, so a lane carries its own candidate's running
//            sum in an LDS word of its own: reset at ql == 0, s = fadd(s, fmul(w, d)) at each ql, stored to u_score at
//            ql == L - 1.  The query's weights wait in LDS too (one broadcast read per (ql, 64 candidates)): wave-uniform, and
//            neither they nor the sums cost a scalar register, which the query blocks of exact_fma_chunk all take.
//            The queries of the loop are the query's L padded rows, consecutive in the padded batch.  LDS: 512 bytes.
//   select   fused_select_kernel: one 256-thread workgroup per query.  One bitonic sort in LDS over the power of two >=
//            max(u_count, 64) of  orderable(score) << 32 | slot : the slots ascend with the ids, so this is (score, id) order.
//            A NaN score becomes the all-ones word: behind everything, never written.  It writes all three outputs, padding
//            included, ids through the row map if asked.  LDS: 8 bytes per sorted element, 64 KiB at 8,192.
// No MFMA (its accumulation order is another one), no inline asm beyond the empty ordering statements of exact_fma_chunk and
// the sink's.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>

#include "device_exact.h"
#include "device_wg_primitives.h"
#include "host_fused.h"

namespace cph {

struct FusedArgs {
    ScanCommon s;                          // raw, norm_sq, qpad [n * T + kExactQT][D], qnorm, D (the other fields: unused)
    const int64_t* cand;                   // [n][T][C] candidate rows: internal ids, -1 = padding
    const int32_t* n_vectors;              // [n] live vectors of every query (clamped to [1, T] here), or null: T
    const float* weights;                  // [n][T]
    uint32_t T, C, k;
    uint32_t n_ids;                        // ids at or above this are treated as padding (no search returns one)
    uint32_t G;                            // blocks of 64 union slots per work item of the scan (fused_scan sets it)
    uint32_t* u_ids;                       // [n][T * C] scratch: the union, ascending
    uint32_t* u_hits;                      // [n][T * C] scratch
    uint32_t* u_count;                     // [n] scratch
    float* u_score;                        // [n][T * C] scratch: exact weighted sums
    const uint32_t* rows;                  // row map or null
    int64_t* out_ids;                      // [n][k]
    float* out_score;                      // [n][k]
    int32_t* out_hits;                     // [n][k]
};

constexpr uint32_t kFusedItemSlots = 64;   // union slots per block of the scan: one block of the candidate loop
constexpr uint32_t kFusedScanGrid = 4096;  // work items the scan aims at: a larger batch gets more blocks per item (FusedArgs::G)

__device__ __forceinline__ uint32_t fused_live(const FusedArgs& a, size_t q) {
    if (!a.n_vectors) return a.T;
    const int32_t l = a.n_vectors[q];
    return l < 1 ? 1u : ((uint32_t)l > a.T ? a.T : (uint32_t)l);
}

// words u64 [P] | segment's first run u16 [P + 2] | counters u32 [8]
inline size_t fused_union_lds(uint32_t T, uint32_t C) {
    const size_t P = wg_sort_len(T * C);
    return P * 8 + (P + 2) * 2 + 8 * 4;
}

// Grid n, kWgSortThreads threads; LDS: fused_union_lds(T, C).
__global__ __launch_bounds__(kWgSortThreads) void fused_union_kernel(FusedArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t T = a.T, C = a.C, Pmax = wg_sort_len(T * C);
    unsigned long long* w = reinterpret_cast<unsigned long long*>(smem);
    uint16_t* sf = reinterpret_cast<uint16_t*>(w + Pmax);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(smem + (size_t)Pmax * 8 + (((size_t)Pmax + 2) * 2 + 3) / 4 * 4);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t q = blockIdx.x;
    const int64_t* __restrict__ qi = a.cand + q * T * C;
    const uint32_t L = fused_live(a, q);
    const uint32_t E = L * C, P = wg_sort_len(E);

    for (uint32_t e = tid; e < P; e += kWgSortThreads) {
        unsigned long long word = kSortNone;
        if (e < E) {
            const int64_t id = qi[e];
            if (id >= 0 && (unsigned long long)id < a.n_ids) word = ((unsigned long long)id << 32) | (e / C);
        }
        w[e] = word;
    }
    __syncthreads();
    wg_sort(w, P, tid);

    // wave v owns [v * span, (v + 1) * span) of the sorted words
    const uint32_t span = P / 4 < 64 ? 64 : P / 4;
    const uint32_t w_lo = wave * span < P ? wave * span : P, w_hi = w_lo + span < P ? w_lo + span : P;
    const unsigned long long below = (1ull << lane) - 1;
    uint32_t runs = 0, segs = 0;
    for (uint32_t base = w_lo; base < w_hi; base += 64) {
        const uint32_t i = base + lane;
        const unsigned long long x = w[i], pv = i ? w[i - 1] : kSortNone;
        const bool valid = x != kSortNone;
        const bool seg = valid && (i == 0 || (uint32_t)(pv >> 32) != (uint32_t)(x >> 32));
        const bool run = valid && (seg || pv != x);
        runs += (uint32_t)__popcll(__ballot(run));
        segs += (uint32_t)__popcll(__ballot(seg));
    }
    if (lane == 0) {
        cnt[wave] = runs;
        cnt[4 + wave] = segs;
    }
    __syncthreads();
    uint32_t r0 = 0, s0 = 0;
    for (uint32_t v = 0; v < wave; ++v) {
        r0 += cnt[v];
        s0 += cnt[4 + v];
    }
    const uint32_t n_runs = cnt[0] + cnt[1] + cnt[2] + cnt[3], n_segs = cnt[4] + cnt[5] + cnt[6] + cnt[7];
    uint32_t* __restrict__ u_ids = a.u_ids + q * T * C;
    uint32_t* __restrict__ u_hits = a.u_hits + q * T * C;
    for (uint32_t base = w_lo; base < w_hi; base += 64) {
        const uint32_t i = base + lane;
        const unsigned long long x = w[i], pv = i ? w[i - 1] : kSortNone;
        const bool valid = x != kSortNone;
        const bool seg = valid && (i == 0 || (uint32_t)(pv >> 32) != (uint32_t)(x >> 32));
        const bool run = valid && (seg || pv != x);
        const unsigned long long run_m = __ballot(run), seg_m = __ballot(seg);
        if (seg) {                                            // n_segs <= the valid entries <= E <= T * C
            const uint32_t s = s0 + (uint32_t)__popcll(seg_m & below);
            sf[s] = (uint16_t)(r0 + (uint32_t)__popcll(run_m & below));
            u_ids[s] = (uint32_t)(x >> 32);
        }
        r0 += (uint32_t)__popcll(run_m);
        s0 += (uint32_t)__popcll(seg_m);
    }
    if (tid == 0) {
        sf[n_segs] = (uint16_t)n_runs;
        a.u_count[q] = n_segs;
    }
    __syncthreads();
    for (uint32_t s = tid; s < n_segs; s += kWgSortThreads) u_hits[s] = (uint32_t)sf[s + 1] - (uint32_t)sf[s];
}

// The weighted sum of one block of 64 candidates: sm[lane] the lane's running sum, sw[t] the query's weights.  The workgroup
// is one wave; a lane touches its own sum only (the LDS operations of a wave complete in program order), and one barrier
// follows the weights where they are loaded.  A sink serves one block; the words it leaves are reset by the next one's ql == 0.
struct FusedSumSink {
    float* sm;
    const float* sw;
    float* score;                 // where the lane's candidate's score goes
    uint32_t last;                // L - 1

    __device__ __forceinline__ FusedSumSink(unsigned char* smem, uint32_t L, float* score_)
        : sm(reinterpret_cast<float*>(smem)), sw(sm + 64), score(score_), last(L - 1) {
        // the output address waits in vector registers until the last query: the loop's scalar registers are all taken by the
        // query blocks of exact_fma_chunk.  (An empty statement: it emits nothing.)
        asm volatile("" : "+v"(score));
    }

    // The weights of the work item's query, once, before its first block.
    __device__ __forceinline__ static void load_weights(unsigned char* smem, const float* weights, uint32_t L) {
        if (threadIdx.x < L) reinterpret_cast<float*>(smem)[64 + threadIdx.x] = weights[threadIdx.x];
        __syncthreads();
    }

    __device__ __forceinline__ void take(uint32_t ql, float d, uint32_t, bool live, int lane) const {
        const float s = __fadd_rn(ql == 0 ? 0.0f : sm[lane], __fmul_rn(sw[ql], d));
        if (ql == last) {
            if (live) *score = s;
        } else {
            sm[lane] = s;
        }
    }

    __device__ __forceinline__ void finish(uint32_t, int) const {}
};

// Grid n * ceil(blocks / G), blocks = ceil(T * C / kFusedItemSlots) (work item = i * ceil(blocks / G) + g), one wave per
// workgroup; LDS: 512 bytes.
template <int SD, int CH>
__global__ __launch_bounds__(64) void fused_scan_kernel(FusedArgs a) {
    __shared__ __align__(16) unsigned char smem[512];
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    const uint32_t TC = a.T * a.C, blocks = (TC + kFusedItemSlots - 1) / kFusedItemSlots, per_q = (blocks + a.G - 1) / a.G;
    const size_t q = blockIdx.x / per_q;
    const uint32_t b0 = (blockIdx.x - (uint32_t)q * per_q) * a.G;
    uint32_t U = a.u_count[q];
    if (U > TC) U = TC;
    if (b0 * kFusedItemSlots >= U) return;
    const uint32_t L = fused_live(a, q);
    const size_t row0 = q * a.T, slot0 = q * TC;
    FusedSumSink::load_weights(smem, a.weights + row0, L);
    for (uint32_t b = b0; b < b0 + a.G; ++b) {
        const uint32_t c_lo = b * kFusedItemSlots;
        if (c_lo >= U) break;
        const uint32_t c_hi = c_lo + kFusedItemSlots < U ? c_lo + kFusedItemSlots : U;
        exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, ExactListSource{a.u_ids + slot0}, c_lo, c_hi,
                                      (exact_uniform_ptr)(a.s.qpad + row0 * D), (exact_uniform_ptr)(a.s.qnorm + row0), L,
                                      FusedSumSink(smem, L, a.u_score + slot0 + c_lo + threadIdx.x));
    }
}

inline size_t fused_select_lds(uint32_t T, uint32_t C) { return (size_t)wg_sort_len(T * C) * 8; }

// Grid n, kWgSortThreads threads; LDS: fused_select_lds(T, C).
__global__ __launch_bounds__(kWgSortThreads) void fused_select_kernel(FusedArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* w = reinterpret_cast<unsigned long long*>(smem);
    const uint32_t TC = a.T * a.C, k = a.k, tid = threadIdx.x;
    const size_t q = blockIdx.x;
    uint32_t U = a.u_count[q];
    if (U > TC) U = TC;
    const uint32_t P = wg_sort_len(U);
    const uint32_t* __restrict__ u_ids = a.u_ids + q * TC;
    const uint32_t* __restrict__ u_hits = a.u_hits + q * TC;
    const float* __restrict__ u_score = a.u_score + q * TC;

    for (uint32_t s = tid; s < P; s += kWgSortThreads) {
        unsigned long long word = kSortNone;
        if (s < U) {
            const float sc = u_score[s];
            if (sc == sc) word = ((unsigned long long)orderable(sc) << 32) | s;
        }
        w[s] = word;
    }
    __syncthreads();
    wg_sort(w, P, tid);

    for (uint32_t o = tid; o < k; o += kWgSortThreads) {
        int64_t id = -1;
        int32_t hits = 0;
        uint32_t score = 0x7F7FFFFFu;                     // FLT_MAX
        const unsigned long long x = o < P ? w[o] : kSortNone;
        if (x != kSortNone) {
            const uint32_t s = (uint32_t)x, i = u_ids[s];
            id = a.rows ? (int64_t)a.rows[i] : (int64_t)i;
            hits = (int32_t)u_hits[s];
            score = __float_as_uint(from_orderable((uint32_t)(x >> 32)));
        }
        a.out_ids[q * k + o] = id;
        reinterpret_cast<uint32_t*>(a.out_score)[q * k + o] = score;
        a.out_hits[q * k + o] = hits;
    }
}

// A query of more than 2,048 entries needs more dynamic LDS than a plain launch accepts: the two functions' limits are raised
// to the largest shape's, once per device.
inline void fused_raise_lds(uint32_t T, uint32_t C, int device) {
    static std::atomic<bool> raised[64];
    if (fused_union_lds(T, C) <= 48 * 1024 || (device >= 0 && device < 64 && raised[device].load())) return;
    const uint32_t Tm = kFusedMaxVectors, Cm = kFusedMaxEntries / kFusedMaxVectors;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fused_union_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)fused_union_lds(Tm, Cm)));
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&fused_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)fused_select_lds(Tm, Cm)));
    if (device >= 0 && device < 64) raised[device].store(true);
}

// Enqueue the pass over n queries (n >= 1, n * T < 2^31) on `device`, the current device, on `st`; the padded rows and norms
// are in place.  scan() alone is what the pass timer brackets.
inline void fused_union(const FusedArgs& a, uint32_t n, int device, hipStream_t st) {
    fused_raise_lds(a.T, a.C, device);
    hipLaunchKernelGGL(fused_union_kernel, dim3(n), dim3(kWgSortThreads), fused_union_lds(a.T, a.C), st, a);
    HIP_CHECK(hipGetLastError());
}

inline void fused_scan(const FusedArgs& a, uint32_t n, hipStream_t st) {
    const uint32_t blocks = (a.T * a.C + kFusedItemSlots - 1) / kFusedItemSlots;
    FusedArgs b = a;
    b.G = (uint32_t)std::min<uint64_t>(blocks, std::max<uint64_t>(1, ((uint64_t)n * blocks + kFusedScanGrid - 1) / kFusedScanGrid));
    CPH_LAUNCH_SCAN(fused_scan_kernel, a.s.D, dim3(n * ((blocks + b.G - 1) / b.G)), 0, st, b);
}

inline void fused_select(const FusedArgs& a, uint32_t n, int device, hipStream_t st) {
    fused_raise_lds(a.T, a.C, device);
    hipLaunchKernelGGL(fused_select_kernel, dim3(n), dim3(kWgSortThreads), fused_select_lds(a.T, a.C), st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
