// device_maxsim_all.h — the exhaustive first stage of multi-vector search (cph_search_maxsim_all*): a matrix-core pass over
// every row of every key that leaves one certified lower bound per (query, key), and the selection of the R smallest.  The
// n * T * size distances never reach memory.  The statement, the bound and why it holds: host_maxsim_all.h.  What follows
// (exact_pad_kernel, maxsim_rescore_scan_kernel, maxsim_rescore_select_kernel) is device_maxsim_rescore.h's, unchanged.
//
// Kernels, on one stream, per chunk of queries (plan_maxsim_all):
//   eps     exact_mfma_query_kernel over the n * T token rows (device_exact_mfma.h)
//   pack    maxsim_all_pack_kernel: the token rows into the tile layout -- query q owns rows q Tp .. q Tp + Tp - 1, Tp = T
//           rounded up to a power of two, so a 128-row tile holds 128 / Tp whole queries; rows t >= n_tokens[q] are zero rows
//           (d^ = |b|^2: finite, never read); unbounded[q] = some live token's qnorm or eps is not finite
//   bounds  maxsim_all_mfma_kernel: grid (P parts, query tiles), 256 threads, mx_scan_tiles<LIST> over the inverted key
//           column (candidate c is csr.ids[c]).  Workgroup p bisects offsets[] for the first key at or behind column
//           p * part and (p + 1) * part: parts begin and end at KEY boundaries, no key straddles two workgroups.
//   select  maxsim_all_select_kernel: one workgroup per query over its table row
//
// The tile epilogue of `bounds`.  Wave w owns tile rows 32 w .. 32 w + 31 and all 128 columns, in four blocks of 32 columns;
// lane (h, c) holds 16 rows of column c of each block.  Per block:
//   1. the column's id, and ONE bitmap word per query the wave's rows belong to (32 / Tp of them, one from Tp = 32 on) -> a
//      32-bit mask "this column counts for wave row r"; columns behind the part's end have mask 0;
//   2. d^ = max(fma(-2, acc, qn), 0) per accumulator, +inf where the mask bit is clear; an allowed d^ that is not finite
//      marks the query unbounded and counts as 0;
//   3. the block is cut at the key boundaries inside it (offsets[], wave-uniform scalar loads: the boundaries are not staged
//      in LDS, a block rarely holds more than one).  Per segment the lanes inside it fold their 16 values into the lane's
//      running minima rm[16] of the OPEN key -- a key that spans blocks or tiles is carried in registers, 16 v_min per block;
//   4. where a key closes, the wave reduces rm across its 32 columns by a halving exchange (8 + 4 + 2 + 1 + 1 shuffles: each
//      step a lane keeps half of its rows) and writes rowmin[slot][row] to LDS; rm starts again at +inf;
//   5. after kMaxsimAllSlots closed keys (and at the part's end) the workgroup flushes: a barrier, then one thread per
//      (slot, query of the tile) walks the query's live rows IN TOKEN ORDER -- l_t = maxsim_all_term(rowmin, eps_t), the
//      sequential float32 sum -- and stores ONE word into table[query][key rank]; kMaxsimAllNone where token 0's minimum is
//      +inf (all live tokens of a query see the same columns).
// LDS: the operand images and column norms of mx_scan_tiles (75,776 B), rowmin [8 slots][128 rows] (4,096 B), the slots'
// key ranks (32 B), eps per tile row (512 B), the bitmap pointer (1,024 B) and live tokens (128 B) of every tile query:
// 81,568 B: two workgroups per CU would fit, the registers allow one (kMaxsimAllOccupancy).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "device_exact_mfma.h"
#include "device_maxsim_rescore.h"
#include "device_range_mfma.h"
#include "device_wg_primitives.h"
#include "host_maxsim_all.h"

namespace cph {

// Workgroups per CU the bounds kernel is compiled for.  Its LDS would let two fit, but at 256 registers the compiler spills
// 81 vector registers around the MFMA loop; at one workgroup per CU it spills none (profiles/maxsim_all.md).
constexpr int kMaxsimAllOccupancy = 1;
constexpr uint32_t kMaxsimAllSlots = 8;          // closed keys a workgroup gathers before it forms their bounds
constexpr uint32_t kMaxsimAllBuffer = 2048;      // words of the select kernel's LDS buffer (>= 2 * kMaxsimRescoreMax)

struct MaxsimAllArgs {
    MxTileArgs t;                         // raw, norm_sq, qpad / qnorm (packed), ids = csr.ids, D (the rest: per workgroup)
    const float* eps;                     // [n * Tp] packed
    KeyRowsDev csr;
    uint64_t part;
    const int32_t* n_tokens;              // [n] or null: T
    const int32_t* filter_of;             // as in MaxsimRescoreArgs
    const uint32_t* const* bitmaps;
    const uint32_t* unfiltered;
    uint32_t T, Tp, n;                    // n: queries of the call
    uint32_t q_first, q_count;            // the chunk
    uint32_t* unbounded;                  // [n]
    uint32_t* table;                      // [q_count][n_keys]
    uint32_t R;
    int32_t* cand_keys;                   // [n][R]
    float* cand_lb;                       // [n][R]
    int32_t* cand_found;                  // [n]
};

__device__ __forceinline__ uint32_t maxsim_all_live(const int32_t* n_tokens, uint32_t T, size_t q) {
    if (!n_tokens) return T;
    const int32_t l = n_tokens[q];
    return l < 1 ? 1u : ((uint32_t)l > T ? T : (uint32_t)l);
}

// ---- pack -----------------------------------------------------------------------------------------------------------------
// Grid n, 256 threads.  src / src_norm / src_eps / src_flags: the n * T token rows as pad_queries and exact_mfma_query_kernel
// left them.
__global__ __launch_bounds__(256) void maxsim_all_pack_kernel(const float* __restrict__ src, const float* __restrict__ src_norm,
                                                              const float* __restrict__ src_eps, const uint32_t* __restrict__ src_flags,
                                                              const int32_t* __restrict__ n_tokens, uint32_t T, uint32_t Tp, uint32_t D,
                                                              float* __restrict__ qp, float* __restrict__ qn, float* __restrict__ eps,
                                                              uint32_t* __restrict__ unbounded) {
    const size_t q = blockIdx.x;
    const uint32_t L = maxsim_all_live(n_tokens, T, q);
    for (uint32_t e = threadIdx.x; e < Tp * D; e += 256) {
        const uint32_t t = e / D;
        qp[q * Tp * D + e] = t < L ? src[(q * T + t) * D + (e - t * D)] : 0.0f;
    }
    if (threadIdx.x < Tp) {
        const uint32_t t = threadIdx.x;
        qn[q * Tp + t] = t < L ? src_norm[q * T + t] : 0.0f;
        eps[q * Tp + t] = t < L ? src_eps[q * T + t] : 0.0f;
    }
    if (threadIdx.x == 0) {
        uint32_t bad = 0;
        for (uint32_t t = 0; t < L; ++t) bad |= src_flags[q * T + t];
        unbounded[q] = bad;
    }
}

// ---- bounds ---------------------------------------------------------------------------------------------------------------
// The first index in [0, n_keys] whose offset is >= target (offsets[n_keys] = size closes the search).
__device__ __forceinline__ uint32_t maxsim_all_first_key(const uint32_t* __restrict__ offsets, uint32_t n_keys, uint64_t target) {
    uint32_t lo = 0, hi = n_keys;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)offsets[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct MaxsimAllLds {
    float rowmin[kMaxsimAllSlots][kMxTile];
    uint32_t slot_key[kMaxsimAllSlots];
    float eps[kMxTile];                   // per tile row
    const uint32_t* allow[kMxTile];       // per tile query: its bitmap, or null: every id
    uint8_t live[kMxTile];                // per tile query: live tokens, 0 behind the chunk's last query
};

struct MaxsimAllEpilogue {
    const MaxsimAllArgs& a;
    MaxsimAllLds& S;
    const uint32_t c_lo, c_hi;            // the part
    const uint32_t q0;                    // first query of the tile
    const uint32_t tp_shift;              // log2 Tp
    const int tid, wrow, h, c;
    uint32_t kcur, kend;                  // the open key: its rank, the column behind its last
    uint32_t slots;                       // closed keys waiting in rowmin
    float rm[16];

    __device__ __forceinline__ uint32_t wave_queries() const { return a.Tp >= 32 ? 1u : 32u >> tp_shift; }

    __device__ __forceinline__ void begin(const float (&)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) rm[i] = __builtin_inff();
    }

    // The wave's rows of the open key, reduced over its 32 columns -> rowmin[slot]; rm = +inf.
    __device__ __forceinline__ void close_rows(uint32_t slot) {
        float v8[8], v4[4], v2[2];
        const bool b16 = c & 16, b8 = c & 8, b4 = c & 4, b2 = c & 2;
#pragma unroll
        for (int j = 0; j < 8; ++j) v8[j] = fminf(b16 ? rm[j + 8] : rm[j], __shfl_xor(b16 ? rm[j] : rm[j + 8], 16));
#pragma unroll
        for (int j = 0; j < 4; ++j) v4[j] = fminf(b8 ? v8[j + 4] : v8[j], __shfl_xor(b8 ? v8[j] : v8[j + 4], 8));
#pragma unroll
        for (int j = 0; j < 2; ++j) v2[j] = fminf(b4 ? v4[j + 2] : v4[j], __shfl_xor(b4 ? v4[j] : v4[j + 2], 4));
        float v = fminf(b2 ? v2[1] : v2[0], __shfl_xor(b2 ? v2[0] : v2[1], 2));
        v = fminf(v, __shfl_xor(v, 1));
        const int i = (b2 ? 1 : 0) + (b4 ? 2 : 0) + (b8 ? 4 : 0) + (b16 ? 8 : 0);
        if (!(c & 1)) S.rowmin[slot][wrow + mx_acc_row(i, h)] = v;
#pragma unroll
        for (int j = 0; j < 16; ++j) rm[j] = __builtin_inff();
    }

    // Whole workgroup, converged: the bounds of the `slots` closed keys -> the table.
    __device__ __forceinline__ void flush() {
        __syncthreads();
        const uint32_t qpt = kMxTile >> tp_shift;
        for (uint32_t item = (uint32_t)tid; item < slots * qpt; item += 256) {
            const uint32_t s = item / qpt, ql = item - s * qpt, L = S.live[ql];
            if (L == 0) continue;
            const float* m = S.rowmin[s] + (ql << tp_shift);
            const float* e = S.eps + (ql << tp_shift);
            uint32_t word = kMaxsimAllNone;
            if (m[0] < __builtin_inff()) {
                float sum = 0.0f;
                for (uint32_t t = 0; t < L; ++t) sum = __fadd_rn(sum, maxsim_all_term(m[t], e[t]));
                word = __float_as_uint(sum);
            }
            a.table[(size_t)(q0 + ql - a.q_first) * a.csr.n_keys + S.slot_key[s]] = word;
        }
        __syncthreads();
        slots = 0;
    }

    __device__ __forceinline__ void tile(uint32_t tile, const knn_f32x16 (&acc)[4], const float (&qn)[16]) {
        const uint32_t ng = wave_queries(), g0 = (uint32_t)wrow >> tp_shift;
        const uint32_t gmask = a.Tp >= 32 ? 0xFFFFFFFFu : (1u << a.Tp) - 1u;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t b0 = c_lo + tile * kMxTile + (uint32_t)t * 32u;       // (size <= kMxMaxCandidates: no wrap)
            if (b0 >= c_hi) break;
            const uint32_t bend = min(b0 + 32u, c_hi), col = b0 + (uint32_t)c;
            uint32_t okrows = 0;
            if (col < c_hi) {
                const uint32_t id = a.t.ids[col];
                for (uint32_t g = 0; g < ng; ++g) {
                    const uint32_t* p = S.allow[g0 + g];
                    if (!p || ((p[id >> 5] >> (id & 31)) & 1u)) okrows |= gmask << (g << tp_shift);
                }
            }
            float dv[16];
            bool odd = false;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float d = __fmaf_rn(-2.0f, acc[t][i], qn[i]);
                const bool ok = (okrows >> mx_acc_row(i, h)) & 1u;
                const bool fin = fabsf(d) <= FLT_MAX;
                odd = odd || (ok && !fin);
                dv[i] = !ok ? __builtin_inff() : (fin && d > 0.0f ? d : 0.0f);
            }
            if (__any(odd)) {                                                    // (rare) the rows' queries cannot be bounded
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t ql = (uint32_t)(wrow + mx_acc_row(i, h)) >> tp_shift;
                    const bool ok = (okrows >> mx_acc_row(i, h)) & 1u;
                    if (ok && !(fabsf(__fmaf_rn(-2.0f, acc[t][i], qn[i])) <= FLT_MAX) && S.live[ql]) a.unbounded[q0 + ql] = 1u;
                }
            }
            uint32_t pos = b0;
            while (pos < bend) {
                const uint32_t send = min(kend, bend);
                const bool in = col >= pos && col < send;
#pragma unroll
                for (int i = 0; i < 16; ++i) rm[i] = fminf(rm[i], in ? dv[i] : __builtin_inff());
                if (kend <= bend) {                                              // the key closes here
                    close_rows(slots);
                    if (tid == 0) S.slot_key[slots] = kcur;
                    ++slots;
                    if (slots == kMaxsimAllSlots) flush();
                    ++kcur;
                    kend = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.csr.offsets[min(kcur + 1, a.csr.n_keys)]);
                }
                pos = send;
            }
        }
    }
};

// Grid (P, ceil(q_count * Tp / 128)), 256 threads, no dynamic LDS.
__global__ __launch_bounds__(256, kMaxsimAllOccupancy) void maxsim_all_mfma_kernel(MaxsimAllArgs a) {
    __shared__ __align__(16) MxOperandLds L;
    __shared__ MaxsimAllLds S;
    const int tid = threadIdx.x;
    uint32_t tp_shift = 0;
    while ((1u << tp_shift) < a.Tp) ++tp_shift;
    const uint32_t qpt = kMxTile >> tp_shift;
    const uint32_t q0 = a.q_first + blockIdx.y * qpt, q_end = a.q_first + a.q_count;
    if (q0 >= q_end) return;
    const uint32_t k_lo = maxsim_all_first_key(a.csr.offsets, a.csr.n_keys, (uint64_t)blockIdx.x * a.part);
    const uint32_t k_hi = blockIdx.x + 1 == gridDim.x ? a.csr.n_keys
                                                      : maxsim_all_first_key(a.csr.offsets, a.csr.n_keys, ((uint64_t)blockIdx.x + 1) * a.part);
    if (k_lo >= k_hi) return;                             // (a key longer than a part: the workgroup before owns it)
    const uint32_t c_lo = a.csr.offsets[k_lo], c_hi = a.csr.offsets[k_hi];
    if (tid < (int)kMxTile) {
        const uint32_t row = q0 * a.Tp + (uint32_t)tid, q = q0 + ((uint32_t)tid >> tp_shift);
        S.eps[tid] = q < q_end ? a.eps[row] : 0.0f;
        if ((uint32_t)tid < qpt) {
            const uint32_t qq = q0 + (uint32_t)tid;
            const uint32_t* p = a.unfiltered;
            if (qq < q_end && a.filter_of) {
                const int32_t fo = a.filter_of[qq];
                if (fo >= 0) p = a.bitmaps[fo];
            }
            S.allow[tid] = p;
            S.live[tid] = qq < q_end ? (uint8_t)maxsim_all_live(a.n_tokens, a.T, qq) : (uint8_t)0;
        }
    }
    MxTileArgs t = a.t;
    t.c_lo = c_lo;
    t.c_hi = c_hi;
    t.q_row0 = q0 * a.Tp;
    t.q_last = a.n * a.Tp - 1;
    const int lane = tid & 63;
    MaxsimAllEpilogue epi{a, S, c_lo, c_hi, q0, tp_shift, tid, (tid >> 6) * 32, lane >> 5, lane & 31, k_lo, a.csr.offsets[k_lo + 1], 0u, {}};
    mx_scan_tiles<true>(t, L, epi);
    if (epi.slots) epi.flush();
}

// ---- select ---------------------------------------------------------------------------------------------------------------
// Grid q_count, kWgSortThreads threads.  The R smallest words (bound bits << 32 | key rank) of the query's table row, skipping
// kMaxsimAllNone: bound >= +0, so unsigned order is numeric order, and rank ascending is key ascending.  Streaming: words
// below the threshold are appended to an LDS buffer; when the next stride might not fit, the buffer is sorted (wg_sort), cut
// to R and the R-th word becomes the threshold.  An unbounded query's bounds are rewritten as +0.0f first.  Correct for
// n_keys from 1 to 2^31 - 1 and for R larger than the number of keys.
__global__ __launch_bounds__(kWgSortThreads) void maxsim_all_select_kernel(MaxsimAllArgs a) {
    __shared__ unsigned long long w[kMaxsimAllBuffer];
    __shared__ uint32_t s_cnt;
    const uint32_t tid = threadIdx.x, R = a.R;
    const size_t q = (size_t)a.q_first + blockIdx.x;
    uint32_t* row = a.table + (size_t)blockIdx.x * a.csr.n_keys;
    const bool zero = a.unbounded[q] != 0;
    unsigned long long thr = kSortNone;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    auto cut = [&]() {                                    // whole workgroup: sort, keep R, set the threshold
        const uint32_t cnt = s_cnt;
        for (uint32_t i = cnt + tid; i < kMaxsimAllBuffer; i += kWgSortThreads) w[i] = kSortNone;
        __syncthreads();
        wg_sort(w, kMaxsimAllBuffer, tid);
        if (cnt >= R) thr = w[R - 1];
        __syncthreads();
        if (tid == 0) s_cnt = cnt < R ? cnt : R;
        __syncthreads();
    };
    for (uint64_t base = 0; base < a.csr.n_keys; base += kWgSortThreads) {
        // ONE decision per iteration: every thread reads the count behind the barrier that ends the iteration before, and a
        // barrier of its own keeps this iteration's appends behind the last of those reads.
        const bool full = s_cnt + kWgSortThreads > kMaxsimAllBuffer;
        __syncthreads();
        if (full) cut();
        const uint64_t r = base + tid;
        if (r < a.csr.n_keys) {
            uint32_t bits = row[r];
            if (bits != kMaxsimAllNone) {
                if (zero) row[r] = bits = 0u;
                const unsigned long long key = ((unsigned long long)bits << 32) | (uint32_t)r;
                if (key < thr) w[atomicAdd(&s_cnt, 1u)] = key;
            }
        }
        __syncthreads();
    }
    cut();
    const uint32_t found = s_cnt;
    for (uint32_t j = tid; j < found; j += kWgSortThreads) {
        a.cand_keys[q * R + j] = a.csr.keys[(uint32_t)w[j]];
        a.cand_lb[q * R + j] = __uint_as_float((uint32_t)(w[j] >> 32));
    }
    if (tid == 0) a.cand_found[q] = (int32_t)found;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
inline void maxsim_all_pack(const float* src, const float* src_norm, const float* src_eps, const uint32_t* src_flags, const MaxsimAllArgs& a,
                            float* qp, float* qn, float* eps, hipStream_t st) {
    hipLaunchKernelGGL(maxsim_all_pack_kernel, dim3(a.n), dim3(256), 0, st, src, src_norm, src_eps, src_flags, a.n_tokens, a.T, a.Tp, a.t.D, qp,
                       qn, eps, a.unbounded);
    HIP_CHECK(hipGetLastError());
}

// One chunk (a.q_first, a.q_count): the bounds of every (query, key) -> a.table.
inline void maxsim_all_bounds(const MaxsimAllArgs& a, uint32_t P, hipStream_t st) {
    const uint32_t tiles = (uint32_t)(((uint64_t)a.q_count * a.Tp + kMxTile - 1) / kMxTile);
    hipLaunchKernelGGL(maxsim_all_mfma_kernel, dim3(P, tiles), dim3(256), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

inline void maxsim_all_select(const MaxsimAllArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(maxsim_all_select_kernel, dim3(a.q_count), dim3(kWgSortThreads), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
