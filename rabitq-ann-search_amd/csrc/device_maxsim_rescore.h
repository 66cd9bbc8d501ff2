// device_maxsim_rescore.h — the exact rescoring stage of multi-vector search (cph_search_maxsim_rescored*): the R best keys
// of the lower-bound pass (device_maxsim.h at k = R) scored against ALL their allowed rows, and the k best of those.
//
// The statement is host_maxsim_rescore.h's.  Two kernels behind maxsim_rows_kernel and exact_pad_kernel, on one stream:
//   scan     maxsim_rescore_scan_kernel: a work item is (query i, candidate slot j), one wave.  Slots j >= found[i] return at
//            once.  The key's rows are a segment of the inverted key column (ids by (key, id); the distinct keys, ascending;
//            offsets), found by a wave-uniform bisection of the distinct keys.  The work is device_exact.h's candidate loop,
//            exact_scan_candidates, with a source that takes ids from the segment and asks the query's bitmap, and a sink that
//            keeps min(distance bits << 32 | id) per token: the arithmetic, and so every distance bit, is cph_exact_l2's.  The
//            queries of the loop are the query's n_tokens[i] padded token rows, consecutive in the padded batch.
//   sink     per-lane minima in LDS, [token][lane] 64-bit words (a half wave reads and writes 32 consecutive words, the
//            256-byte bank row: conflict-free), one read-compare-write per (token, 64 candidates); reduced across the wave once
//            per token in finish(), which also forms the sequential float32 sum.  LDS: 512 bytes per token, 32 KiB at T = 64.
//            (A wave reduction per take would cost six 64-bit exchange steps per token and 64 candidates, about a quarter of
//            the 128 FMAs a D = 128 pair costs; the LDS words cost three instructions.)
//   select   maxsim_rescore_select_kernel: one 256-thread workgroup per query.  Two bitonic sorts in LDS (wg_sort) over
//            the power of two >= max(found, 64): by (key ^ 0x80000000, slot), which ranks the keys, then by
//            (score bits, key rank, slot).  It writes all six outputs, padding included, rows through the row map if asked,
//            and certified from lb_{R-1}.  LDS: 10 bytes per sorted element, 10 KiB at R = 1,024.
// No MFMA (its accumulation order is another one), no inline asm beyond the empty ordering statements of exact_fma_chunk.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_exact.h"
#include "device_maxsim.h"
#include "device_wg_primitives.h"
#include "host_maxsim_rescore.h"

namespace cph {

// The inverted key column on the device.
struct KeyRowsDev {
    const uint32_t* ids;          // [size] ids by (key, id)
    const int32_t* keys;          // [n_keys] distinct keys, ascending
    const uint32_t* offsets;      // [n_keys + 1]
    uint32_t n_keys;
};

struct MaxsimRescoreArgs {
    ScanCommon s;                          // raw, norm_sq, qpad [n * T + kExactQT][D], qnorm, D (the other fields: unused)
    KeyRowsDev csr;
    const int32_t* cand_keys;              // [n][R]
    const float* cand_lb;                  // [n][R]
    const int32_t* cand_found;             // [n]
    const int32_t* n_tokens;               // [n] or null: T
    const int32_t* filter_of;              // [n] index into bitmaps, -1: `unfiltered`; null: every query uses `unfiltered`
    const uint32_t* const* bitmaps;        // table of bitmap pointers (filter_of != null)
    const uint32_t* unfiltered;            // the bitmap of a query without a filter of its own, or null: every id
    uint32_t T, R, k;
    uint32_t n_ids;
    float* sc_score;                       // [n][R] scratch: exact scores
    uint32_t* sc_rows;                     // [n][R][T] scratch: argmin ids
    const uint32_t* rows;                  // row map or null
    int32_t* out_keys;                     // [n][k]
    float* out_score;                      // [n][k]
    int32_t* out_hits;                     // [n][k]
    int64_t* out_rows;                     // [n][k][T]
    int32_t* out_found;                    // [n]
    int32_t* out_certified;                // [n]
};

__device__ __forceinline__ uint32_t maxsim_rescore_live(const MaxsimRescoreArgs& a, size_t q) {
    if (!a.n_tokens) return a.T;
    const int32_t l = a.n_tokens[q];
    return l < 1 ? 1u : ((uint32_t)l > a.T ? a.T : (uint32_t)l);
}

// Candidate c is ids[c] of the key's segment; an id may be selected when its bit is set in the query's bitmap.
struct KeySegmentSource {
    const uint32_t* ids;
    const uint32_t* allow;        // null: every id
    __device__ __forceinline__ uint32_t id(uint32_t c) const { return ids[c]; }
    __device__ __forceinline__ bool allowed(uint32_t id) const { return !allow || ((allow[id >> 5] >> (id & 31)) & 1u); }
};

// min (distance bits << 32 | id) per token: sm[token][lane].  The workgroup is one wave; every lane touches its own words
// only until finish(), so no barrier is needed before it (the LDS operations of a wave complete in program order).
struct TokenMinSink {
    unsigned long long* sm;
    float* score;                 // where the work item's score goes
    uint32_t* rows;               // [T] where its argmin ids go

    __device__ __forceinline__ TokenMinSink(unsigned char* smem, uint32_t L, float* score_, uint32_t* rows_)
        : sm(reinterpret_cast<unsigned long long*>(smem)), score(score_), rows(rows_) {
        // the two output addresses wait in vector registers until finish(): the loop's scalar registers are all taken by
        // the query blocks of exact_fma_chunk, and these four were the ones spilled.  (Empty statements: they emit nothing.)
        asm volatile("" : "+v"(score));
        asm volatile("" : "+v"(rows));
        for (uint32_t t = 0; t < L; ++t) sm[t * 64 + threadIdx.x] = kExactNoKey;
    }

    __device__ __forceinline__ void take(uint32_t ql, float d, uint32_t id, bool live, int lane) const {
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | id;
        unsigned long long* p = sm + ql * 64 + lane;
        if (live && key < *p) *p = key;
    }

    __device__ __forceinline__ void finish(uint32_t nqg, int lane) const {
        float sum = 0.0f;
        for (uint32_t t = 0; t < nqg; ++t) {
            unsigned long long x = sm[t * 64 + lane];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                const unsigned long long y = __shfl_xor(x, d);
                x = y < x ? y : x;
            }
            sum = __fadd_rn(sum, __uint_as_float((uint32_t)(x >> 32)));
            if (lane == 0) rows[t] = (uint32_t)x;
        }
        if (lane == 0) *score = sum;
    }
};

// Grid n * R (work item b = i * R + j), one wave per workgroup; LDS: 512 bytes per token.
template <int SD, int CH>
__global__ __launch_bounds__(64) void maxsim_rescore_scan_kernel(MaxsimRescoreArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    const size_t q = blockIdx.x / a.R;
    const uint32_t j = blockIdx.x - (uint32_t)q * a.R;
    const int32_t f = a.cand_found[q];
    if (f < 0 || j >= (uint32_t)f) return;
    const uint32_t L = maxsim_rescore_live(a, q);
    const int32_t key = a.cand_keys[q * a.R + j];
    uint32_t lo = 0, hi = a.csr.n_keys;                   // the first distinct key >= key
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.csr.keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    uint32_t c_lo = 0, c_hi = 0;                          // (a key the column does not hold: an empty segment)
    if (lo < a.csr.n_keys && a.csr.keys[lo] == key) {
        c_lo = a.csr.offsets[lo];
        c_hi = a.csr.offsets[lo + 1];
    }
    const uint32_t* allow = a.unfiltered;
    if (a.filter_of) {
        const int32_t fo = a.filter_of[q];
        if (fo >= 0) allow = a.bitmaps[fo];
    }
    const size_t row0 = q * a.T;
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, KeySegmentSource{a.csr.ids, allow}, c_lo, c_hi,
                                  (exact_uniform_ptr)(a.s.qpad + row0 * D), (exact_uniform_ptr)(a.s.qnorm + row0), L,
                                  TokenMinSink(smem, L, a.sc_score + q * a.R + j, a.sc_rows + (q * a.R + j) * a.T));
}

// words u64 [P] | key rank u16 [P]
inline size_t maxsim_rescore_select_lds(uint32_t R) { return (size_t)wg_sort_len(R) * 10; }

// Grid n, kMaxsimThreads threads; LDS: maxsim_rescore_select_lds(R).
__global__ __launch_bounds__(kMaxsimThreads) void maxsim_rescore_select_kernel(MaxsimRescoreArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t T = a.T, R = a.R, k = a.k, tid = threadIdx.x;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(smem);
    uint16_t* rank = reinterpret_cast<uint16_t*>(w + wg_sort_len(R));
    const size_t q = blockIdx.x;
    const int32_t fr = a.cand_found[q];
    const uint32_t f = fr < 0 ? 0u : ((uint32_t)fr > R ? R : (uint32_t)fr);
    const uint32_t L = maxsim_rescore_live(a, q), P = wg_sort_len(f);
    const int32_t* __restrict__ ck = a.cand_keys + q * R;
    const uint32_t* __restrict__ sc = reinterpret_cast<const uint32_t*>(a.sc_score) + q * R;

    for (uint32_t s = tid; s < P; s += kMaxsimThreads)
        w[s] = s < f ? ((unsigned long long)((uint32_t)ck[s] ^ 0x80000000u) << 32) | s : kSortNone;
    __syncthreads();
    wg_sort(w, P, tid);
    for (uint32_t p = tid; p < f; p += kMaxsimThreads) rank[(uint32_t)w[p]] = (uint16_t)p;
    __syncthreads();
    for (uint32_t s = tid; s < P; s += kMaxsimThreads)
        w[s] = s < f ? ((unsigned long long)sc[s] << 32) | ((uint32_t)rank[s] << 16) | s : kSortNone;
    __syncthreads();
    wg_sort(w, P, tid);

    const uint32_t found = k < f ? k : f;
    if (tid == 0) {
        uint32_t cert = found;
        if (f == R) {
            const float lb = a.cand_lb[q * R + R - 1];
            cert = 0;
            while (cert < found && __uint_as_float((uint32_t)(w[cert] >> 32)) < lb) ++cert;
        }
        a.out_found[q] = (int32_t)found;
        a.out_certified[q] = (int32_t)cert;
    }
    for (uint32_t o = tid; o < k; o += kMaxsimThreads) {
        int32_t key = 0, hits = 0;
        uint32_t score = 0x7F7FFFFFu;                     // FLT_MAX
        if (o < found) {
            const unsigned long long x = w[o];
            key = ck[(uint32_t)x & 0xFFFFu];
            hits = (int32_t)L;
            score = (uint32_t)(x >> 32);
        }
        a.out_keys[q * k + o] = key;
        reinterpret_cast<uint32_t*>(a.out_score)[q * k + o] = score;
        a.out_hits[q * k + o] = hits;
    }
    int64_t* __restrict__ out_rows = a.out_rows + q * k * T;
    for (uint32_t idx = tid; idx < k * T; idx += kMaxsimThreads) {
        const uint32_t o = idx / T, t = idx - o * T;
        int64_t val = -1;
        if (o < found && t < L) {
            const uint32_t id = a.sc_rows[(q * R + ((uint32_t)w[o] & 0xFFFFu)) * T + t];
            if (id < a.n_ids) val = a.rows ? (int64_t)a.rows[id] : (int64_t)id;
        }
        out_rows[idx] = val;
    }
}

// Enqueue the scan, then the select, over n queries (n >= 1, n * R < 2^31) on `st`; the padded rows and norms are in place.
inline void maxsim_rescore_scan(const MaxsimRescoreArgs& a, uint32_t n, hipStream_t st) {
    CPH_LAUNCH_SCAN(maxsim_rescore_scan_kernel, a.s.D, dim3(n * a.R), (size_t)a.T * 512, st, a);
}

inline void maxsim_rescore_select(const MaxsimRescoreArgs& a, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(maxsim_rescore_select_kernel, dim3(n), dim3(kMaxsimThreads), maxsim_rescore_select_lds(a.R), st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
