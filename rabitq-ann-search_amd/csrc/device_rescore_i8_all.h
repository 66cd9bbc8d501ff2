// device_rescore_i8_all.h — exhaustive int8 rescoring (cph_search_rescored_all): every query against EVERY row of an int8
// rescore object on the matrix cores, top-k selected on the device.  The score of a (query, row) pair is byte for byte what
// rescore_i8_kernel (device_rescore_i8.h) writes for it: H = sum h_i c_i and L = sum l_i c_i are integer sums, exact in any
// order, so v_mfma_i32_32x32x32_i8 makes them and the float epilogue is the statement's, one rounded instruction per
// operation.  No slack, no certification, no fallback.
//
// rescore_i8_all_pack_kernel, one workgroup per query of the padded batch: the prologue of rescore_i8_kernel (the same
// __device__ functions) into two int8 planes [n_pad][Kq] in global memory, zeros behind dim_full and in the rows behind n,
// and sq, qn and an ok flag per query.  Kq = rescore_all_kpad(row bytes) (host_rescore_all.h).
//
// rescore_i8_all_scan_kernel, grid (query tiles of 128) x (P row parts), the query tile the fast dimension: the workgroups
// resident at one time read the same row part.  256 threads; a step is 128 queries x 128 rows; wave w owns rows
// [32 w, 32 w + 32) of the step against all 128 queries and both planes: eight 32x32 int32 accumulators.
//   rows     no LDS: a row is used by one wave.  Lane l loads the 16-byte piece 2 kstep + (l >> 5) of row l & 31 with one
//            global load -- the A operand of the instruction as it lies in memory.  Four k-steps of loads are issued
//            together.  A piece at or behind the row's piece count and a row at or behind the object's size is zeros and
//            is not read.
//   queries  the B operands, from LDS: plane h [128][S] then plane l [128][S], S = KC + 16 bytes, KC the bytes of K held.
//            S / 16 is odd, so the sixteen lanes a 16-byte LDS read serves per cycle (queries q .. q + 15 at one k) fall on
//            sixteen different 16-byte bank groups: no conflict.  Kq <= 256: KC = Kq, staged once per workgroup.  Above: KC =
//            128, two buffers; chunk c + 1 is copied (global -> LDS) in front of the MFMAs of chunk c, one barrier per chunk.
//   epilogue in registers.  Accumulator register i of lane l is row 8 (i / 4) + 4 (l >> 5) + i % 4, query l & 31.  A lane
//            holds sq, qn and the bitmap pointer of its four queries for the whole part and fetches the scale and norm of
//            its sixteen rows once per step.  I = 128 H + L in 64 bits, rescore_i8_score.  One bitmap word per (query,
//            wave, step): blocks are id-aligned.  A null bitmap allows every id below the object's size.
//   select   per (part, query) a pool of C = 2 Kp words (orderable(score) << 32) | id in scratch (Kp = max(128, pow2(k)):
//            plan_rescore_all), its fill count and
//            threshold in LDS.  A lane whose word is not above the threshold takes a slot with an LDS atomic and stores.
//            After a step the workgroup sorts every pool fuller than C - 128 (wg_sort), cuts it to k and lowers the
//            threshold: a step adds at most 128 words per query, so no pool overflows.  After the last step every pool is
//            sorted and cut: the part's top k by (score, id).
//
// rescore_i8_all_select_kernel, one wave per query: exact_fold_parts (device_exact.h) folds the P lists, then score unfolded,
// ids through the row map, every slot of the three outputs written (`first` = FLT_MAX: there is no first stage).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <cstdint>

#include "device_exact.h"
#include "device_rescore_i8.h"
#include "host_rescore_all.h"

namespace cph {

typedef int rescore_all_v4i __attribute__((ext_vector_type(4)));
typedef int rescore_all_v16i __attribute__((ext_vector_type(16)));

struct RescoreAllArgs {
    RescoreStore s;                       // the int8 object
    const float* scales;                  // [n_ids]
    const float* fq;                      // [n][dim] full queries
    uint32_t n, n_pad, Kq;                // n_pad: n rounded up to the tile; Kq: bytes of a plane row
    uint32_t* hq;                         // [n_pad][Kq / 4]
    uint32_t* lq;
    float* sq;                            // [n_pad]
    float* qn;
    uint32_t* ok;
    const int32_t* filter_of;             // [n] or null; -1: `unfiltered`
    const uint32_t* const* bitmaps;
    const uint32_t* unfiltered;           // the bitmap of a query without a filter, or null: every id
    int ip;
    uint32_t k, C, P;
    uint64_t part;                        // rows per part, a multiple of 128
    uint32_t q_first, q_count;            // the queries of this launch (q_first: a multiple of the tile)
    unsigned long long* pools;            // [P][q_count][C]
    uint32_t* counts;                     // [P][q_count]
    const uint32_t* rows;                 // row map, or null
    int64_t* out_ids;                     // [n][k]
    float* out_score;
    float* out_first;
};

__host__ __device__ inline uint32_t rescore_all_chunk_bytes(uint32_t Kq) { return Kq <= kRescoreAllResident ? Kq : kRescoreAllChunk; }

inline size_t rescore_all_scan_lds(uint32_t Kq, uint32_t C) {
    const uint32_t KC = rescore_all_chunk_bytes(Kq);
    return (size_t)(Kq > KC ? 2 : 1) * 2 * kRescoreAllTile * (KC + 16) + (size_t)C * 8 + kRescoreAllTile * 8 + 16;
}

// Grid n_pad, kRescoreThreads threads.
__global__ __launch_bounds__(kRescoreThreads) void rescore_i8_all_pack_kernel(RescoreAllArgs a) {
    __shared__ unsigned long long red[8];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, words = a.Kq / 4, dim = a.s.dim;
    const size_t q = blockIdx.x;
    uint32_t* __restrict__ hq = a.hq + q * words;
    uint32_t* __restrict__ lq = a.lq + q * words;
    if (q >= a.n) {                                                           // a padding row of the last tile
        for (uint32_t i = tid; i < words; i += kRescoreThreads) {
            hq[i] = 0;
            lq[i] = 0;
        }
        if (tid == 0) {
            a.sq[q] = 0.0f;
            a.qn[q] = 0.0f;
            a.ok[q] = 0;
        }
        return;
    }
    const float* __restrict__ fq = a.fq + q * dim;
    uint32_t qbits = rescore_i8_query_max(fq, dim, tid);
    if (lane == 0) red[wave] = qbits;
    __syncthreads();
    qbits = max(max((uint32_t)red[0], (uint32_t)red[1]), max((uint32_t)red[2], (uint32_t)red[3]));
    const bool q_ok = qbits < 0x7F800000u;
    const float sq = __fdiv_rn(__uint_as_float(qbits), kRescoreI8QueryMax);
    unsigned long long t2 = 0;
    for (uint32_t i = tid; i < words; i += kRescoreThreads) {
        uint32_t hw, lw;
        rescore_i8_plane_words(fq, i, dim, q_ok && qbits != 0, sq, hw, lw, t2);
        hq[i] = hw;
        lq[i] = lw;
    }
    for (uint32_t d = 32; d; d >>= 1) t2 += __shfl_xor(t2, (int)d, 64);
    if (lane == 0) red[4 + wave] = t2;
    __syncthreads();
    if (tid == 0) {
        a.sq[q] = sq;
        a.qn[q] = rescore_i8_query_norm(sq, red[4] + red[5] + red[6] + red[7]);
        a.ok[q] = q_ok ? 1u : 0u;
    }
}

// Chunk `chunk` (KC bytes of K) of both planes of the tile's 128 queries -> buf: [2][128][KC + 16].
__device__ __forceinline__ void rescore_all_stage(const RescoreAllArgs& a, uint32_t q0, uint32_t chunk, uint32_t KC, unsigned char* buf,
                                                  uint32_t tid) {
    const uint32_t ppr = KC / 16, S = KC + 16;
    for (uint32_t idx = tid; idx < 2 * kRescoreAllTile * ppr; idx += kRescoreThreads) {
        const uint32_t r = idx / ppr, p = idx - r * ppr, q = r & (kRescoreAllTile - 1);
        const uint32_t* plane = (r >> 7) ? a.lq : a.hq;
        const uint4 v = *reinterpret_cast<const uint4*>(plane + ((size_t)(q0 + q) * a.Kq + (size_t)chunk * KC + p * 16) / 4);
        *reinterpret_cast<uint4*>(buf + (size_t)r * S + p * 16) = v;
    }
}

// pool[cnt] -> its min(cnt, k) smallest words, ascending, by the whole workgroup; the count and the threshold of query ql.
__device__ __forceinline__ void rescore_all_compact(unsigned long long* w, unsigned long long* pool, uint32_t* s_thr, uint32_t* s_cnt,
                                                    uint32_t ql, uint32_t cnt, uint32_t k, uint32_t C, uint32_t tid) {
    cnt = cnt < C ? cnt : C;
    for (uint32_t i = tid; i < C; i += kRescoreThreads)       // (past the CU's vector cache: other waves stored these words)
        w[i] = i < cnt ? __hip_atomic_load(pool + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kSortNone;
    __syncthreads();
    wg_sort(w, C, tid);
    const uint32_t kept = cnt < k ? cnt : k;
    for (uint32_t i = tid; i < kept; i += kRescoreThreads) pool[i] = w[i];
    if (tid == 0) {
        s_cnt[ql] = kept;
        s_thr[ql] = kept == k ? (uint32_t)(w[k - 1] >> 32) : 0xFFFFFFFFu;
    }
    __threadfence();
    __syncthreads();
}

// Grid (tiles of the launch, P), kRescoreThreads threads; LDS: rescore_all_scan_lds(Kq, C).
__global__ __launch_bounds__(kRescoreThreads) void rescore_i8_all_scan_kernel(RescoreAllArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, col = lane & 31u, half = lane >> 5;
    const uint32_t Kq = a.Kq, KC = rescore_all_chunk_bytes(Kq), NC = Kq / KC, nks = KC / 32, S = KC + 16;
    const uint32_t buf_bytes = 2 * kRescoreAllTile * S, C = a.C, k = a.k, n_ids = a.s.n_ids, pieces = a.s.pieces;
    unsigned char* planes = smem;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(smem + (size_t)(NC > 1 ? 2 : 1) * buf_bytes);
    uint32_t* s_thr = reinterpret_cast<uint32_t*>(w + C);
    uint32_t* s_cnt = s_thr + kRescoreAllTile;
    uint32_t* s_flag = s_cnt + kRescoreAllTile;
    const uint32_t ql0 = blockIdx.x * kRescoreAllTile;                    // first query of the tile, relative to q_first
    const uint32_t q0 = a.q_first + ql0;
    const uint64_t row_lo = (uint64_t)blockIdx.y * a.part;
    const uint64_t row_hi = min((uint64_t)n_ids, row_lo + a.part);
    if (row_lo >= row_hi) return;                                         // (uniform; the plan makes no such part)
    const uint32_t steps = (uint32_t)((row_hi - row_lo + kRescoreAllTile - 1) / kRescoreAllTile);
    const uint32_t trigger = C - kRescoreAllTile;                         // a pool at most this full takes a whole step
    const uint32_t nw = (n_ids + 31u) / 32u;

    // this lane's four queries: 32 t + col
    float sqv[4], qnv[4];
    const uint32_t* bm[4];
    bool valid[4];
    unsigned long long* pool[4];
#pragma unroll
    for (uint32_t t = 0; t < 4; ++t) {
        const uint32_t ql = ql0 + 32 * t + col, qa = a.q_first + ql;      // (qa < n_pad)
        valid[t] = ql < a.q_count && a.ok[qa] != 0;
        sqv[t] = a.sq[qa];
        qnv[t] = a.qn[qa];
        const uint32_t* p = a.unfiltered;
        if (ql < a.q_count && a.filter_of) {
            const int32_t fo = a.filter_of[qa];
            if (fo >= 0) p = a.bitmaps[fo];
        }
        bm[t] = p;
        pool[t] = a.pools + ((size_t)blockIdx.y * a.q_count + (ql < a.q_count ? ql : 0u)) * C;
    }
    for (uint32_t i = tid; i < kRescoreAllTile; i += kRescoreThreads) {
        s_thr[i] = 0xFFFFFFFFu;
        s_cnt[i] = 0;
    }
    if (tid == 0) *s_flag = 0;
    rescore_all_stage(a, q0, 0, KC, planes, tid);

    uint32_t it = 0;
    const uint32_t total = steps * NC;
    for (uint32_t step = 0; step < steps; ++step) {
        const uint32_t wave_row0 = (uint32_t)row_lo + step * kRescoreAllTile + wave * 32;      // a multiple of 32
        const uint32_t my_row = wave_row0 + col;
        const bool row_live = my_row < n_ids;
        const uint4* __restrict__ rowp = reinterpret_cast<const uint4*>(a.s.rows + (size_t)(row_live ? my_row : 0u) * a.s.stride);
        rescore_all_v16i acc_h[4], acc_l[4];
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                acc_h[t][i] = 0;
                acc_l[t][i] = 0;
            }
        }
        for (uint32_t c = 0; c < NC; ++c, ++it) {
            __syncthreads();                      // buffer it & 1 is staged; everyone is done with the other one
            if (NC > 1 && it + 1 < total) rescore_all_stage(a, q0, c + 1 < NC ? c + 1 : 0u, KC, planes + (size_t)((it + 1) & 1u) * buf_bytes, tid);
            const unsigned char* cur = planes + (NC > 1 ? (size_t)(it & 1u) * buf_bytes : 0);
            const unsigned char* bq = cur + (size_t)col * S + half * 16;
            const uint32_t piece0 = c * (KC / 16) + half;
            for (uint32_t g = 0; g < nks; g += 4) {                        // uniform
                rescore_all_v4i x[4];
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    const uint32_t piece = piece0 + 2 * (g + j);
                    x[j] = (rescore_all_v4i){0, 0, 0, 0};
                    if (row_live && g + j < nks && piece < pieces) {
                        const uint4 v = rowp[piece];
                        x[j] = (rescore_all_v4i){(int)v.x, (int)v.y, (int)v.z, (int)v.w};
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < 4; ++j) {
                    if (g + j >= nks) break;
                    const unsigned char* bk = bq + (g + j) * 32;
#pragma unroll
                    for (uint32_t t = 0; t < 4; ++t) {
                        const rescore_all_v4i bh = *reinterpret_cast<const rescore_all_v4i*>(bk + (size_t)(32 * t) * S);
                        const rescore_all_v4i bl = *reinterpret_cast<const rescore_all_v4i*>(bk + (size_t)(kRescoreAllTile + 32 * t) * S);
                        acc_h[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(x[j], bh, acc_h[t], 0, 0, 0);
                        acc_l[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(x[j], bl, acc_l[t], 0, 0, 0);
                    }
                }
            }
        }

        // the step's scores: this lane's sixteen rows against its four queries
        const uint32_t blk = wave_row0 >> 5;
        const uint32_t live_rows = wave_row0 >= n_ids ? 0u : (n_ids - wave_row0 >= 32u ? 0xFFFFFFFFu : (1u << (n_ids - wave_row0)) - 1u);
        float sc[16], xn[16];
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) {
            const uint32_t id = wave_row0 + 8 * (i / 4) + 4 * half + (i % 4);
            const bool live = id < n_ids;
            sc[i] = live ? a.scales[id] : 0.0f;
            xn[i] = (live && !a.ip) ? a.s.norms[id] : 0.0f;
        }
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            uint32_t mw = 0;
            if (valid[t] && blk < nw) mw = (bm[t] ? bm[t][blk] : 0xFFFFFFFFu) & live_rows;
            if (mw == 0) continue;
            const uint32_t ql = 32 * t + col, thr = s_thr[ql];
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t r = 8 * (i / 4) + 4 * half + (i % 4);
                if (!((mw >> r) & 1u)) continue;
                const long long I = 128ll * (long long)acc_h[t][i] + (long long)acc_l[t][i];
                const float score = rescore_i8_score(I, sc[i], sqv[t], qnv[t], xn[i], a.ip != 0);
                const uint32_t key = orderable(score);
                if (score != score || key > thr) continue;
                const uint32_t pos = atomicAdd(&s_cnt[ql], 1u);
                if (pos < C) pool[t][pos] = ((unsigned long long)key << 32) | (wave_row0 + r);
                if (pos + 1 > trigger) *s_flag = 1u;
            }
        }
        __threadfence();
        __syncthreads();
        if (*s_flag) {                                                     // uniform
            for (uint32_t ql = 0; ql < kRescoreAllTile; ++ql) {
                const uint32_t cnt = s_cnt[ql];
                if (cnt <= trigger) continue;
                rescore_all_compact(w, a.pools + ((size_t)blockIdx.y * a.q_count + ql0 + ql) * C, s_thr, s_cnt, ql, cnt, k, C, tid);
            }
            __syncthreads();                                               // every thread has read the flag
            if (tid == 0) *s_flag = 0;
        }
    }
    // every pool of the tile: sorted, cut to k
    __syncthreads();
    for (uint32_t ql = 0; ql < kRescoreAllTile && ql0 + ql < a.q_count; ++ql) {
        const uint32_t cnt = s_cnt[ql];
        const size_t pi = (size_t)blockIdx.y * a.q_count + ql0 + ql;
        if (cnt) rescore_all_compact(w, a.pools + pi * C, s_thr, s_cnt, ql, cnt, k, C, tid);
        if (tid == 0) a.counts[pi] = s_cnt[ql];
    }
}

// Grid q_count, one wave; LDS: C words.
__global__ __launch_bounds__(64) void rescore_i8_all_select_kernel(RescoreAllArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    const int lane = threadIdx.x;
    (void)exact_fold_parts(sm, a.pools, a.counts, blockIdx.x, a.q_count, a.P, a.C, lane);
    __syncthreads();
    const size_t o = ((size_t)a.q_first + blockIdx.x) * a.k;
    uint32_t* __restrict__ out_score = reinterpret_cast<uint32_t*>(a.out_score);
    uint32_t* __restrict__ out_first = reinterpret_cast<uint32_t*>(a.out_first);
    for (uint32_t i = lane; i < a.k; i += 64) {
        const unsigned long long word = sm[i];
        const bool have = word != kExactNoKey;
        const uint32_t id = (uint32_t)word;
        a.out_ids[o + i] = have ? (int64_t)(a.rows ? a.rows[id] : id) : (int64_t)-1;
        out_score[o + i] = have ? __float_as_uint(from_orderable((uint32_t)(word >> 32))) : 0x7F7FFFFFu;      // FLT_MAX
        out_first[o + i] = 0x7F7FFFFFu;
    }
}

// The yardstick of the scan's compute floor (cph_debug_mfma_i8_rate): `iters` rounds of eight independent
// v_mfma_i32_32x32x32_i8 per wave on register operands, nothing else; out[wave] keeps the result alive.
__global__ __launch_bounds__(kRescoreThreads) void rescore_all_mfma_rate_kernel(uint32_t iters, int* out) {
    rescore_all_v4i x = {(int)threadIdx.x, 1, 2, 3}, y = {3, 2, 1, (int)blockIdx.x};
    rescore_all_v16i acc[8];
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t)
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i) acc[t][i] = 0;
    for (uint32_t it = 0; it < iters; ++it) {
#pragma unroll
        for (uint32_t t = 0; t < 8; ++t) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(x, y, acc[t], 0, 0, 0);
    }
    int s = 0;
#pragma unroll
    for (uint32_t t = 0; t < 8; ++t) s += acc[t][0] + acc[t][15];
    out[(size_t)blockIdx.x * kRescoreThreads + threadIdx.x] = s;
}

// Enqueues the pack over the padded batch.
inline void rescore_i8_all_pack(const RescoreAllArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(rescore_i8_all_pack_kernel, dim3(a.n_pad), dim3(kRescoreThreads), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

// Enqueues the scan of the launch's queries [q_first, q_first + q_count).
inline void rescore_i8_all_scan(const RescoreAllArgs& a, int device, hipStream_t st) {
    static std::atomic<bool> raised[64];
    const size_t lds = rescore_all_scan_lds(a.Kq, a.C);
    if (lds > 48 * 1024 && !(device >= 0 && device < 64 && raised[device].load())) {
        const size_t most = std::max(rescore_all_scan_lds(kRescoreAllResident, 2 * kRescoreAllMaxK),
                                     rescore_all_scan_lds(2 * kRescoreAllResident, 2 * kRescoreAllMaxK));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&rescore_i8_all_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)most));
        if (device >= 0 && device < 64) raised[device].store(true);
    }
    const uint32_t tiles = (a.q_count + kRescoreAllTile - 1) / kRescoreAllTile;
    hipLaunchKernelGGL(rescore_i8_all_scan_kernel, dim3(tiles, a.P), dim3(kRescoreThreads), lds, st, a);
    HIP_CHECK(hipGetLastError());
}

inline void rescore_i8_all_select(const RescoreAllArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(rescore_i8_all_select_kernel, dim3(a.q_count), dim3(64), (size_t)a.C * 8, st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
