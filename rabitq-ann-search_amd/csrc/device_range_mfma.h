// device_range_mfma.h — the "matrix" engine of the exact range search (cph_set_exact_engine, cph_range_search_begin): the
// matrix cores discard every (query, id) pair that provably is not a hit, the candidate loop of device_exact.h re-scores
// the survivors and decides.  Every output byte is the vector engine's (device_range.h): MFMA never PRODUCES a distance
// here and never decides a hit, it only prunes.
//
// A range search suits the prefilter better than a top-k does: the threshold is known before the first tile.  A row's limit
// never moves, so there are no pools, no compaction, no keep rule, no flags and no fallback kernels: the tile epilogue is
// a comparison per accumulator.
//
// The limit.  eps(q) = exact_matrix_slack(qnorm, bn_max, D) >= |d^ - d| for every candidate of q (device_exact_mfma.h).
// lim(q) = range_matrix_limit(radius, eps) (host_exact_mfma.h) >= radius + eps.  A pair is discarded iff d^ is finite
// and d^ >= lim:  d >= d^ - eps >= lim - eps >= radius, not a hit.  A radius that admits nothing has lim = -1 (every
// d^ = max(.., 0) is >= it); an eps that is not finite has lim = NaN (no comparison holds: all survive).
//
// Stages, one stream:
//   eps      exact_mfma_query_kernel
//   count    range_mfma_kernel<LIST, false>: counts[q * P + p] = survivors of query q in part p
//   offsets  range_offsets over the nq * P counters -> soffs, slims; the host reads slims (the scratch size is data)
//   fill     range_mfma_kernel<LIST, true>: the survivors' ids at sids[soffs[q * P + p] ..], ascending in id
//   rescore  range_rescore_runs_kernel: a wave per run of <= kRangeRun survivors of one query: the distances through
//            exact_scan_candidates, `d < radius` (strict) decided on them, the run sorted in LDS and written to the arena;
//            hits[q] += the run's hits
//   merge    range_merge_pass_kernel for segments longer than a run, as in device_range.h (non-hits sort behind every hit)
//   offsets  range_offsets(hits, nq, 1) -> lims
//   emit     range_emit_hits_kernel (in cph_range_search_finish): the first hits[q] keys of every segment
//
// Geometry of range_mfma_kernel: that of the prefilter (grid (P parts, tiles of 128 queries), 256 threads, wave w owns query
// rows 32 w .. 32 w + 31 and all 128 columns of a candidate tile; mx_scan_tiles is the operand pipeline).  A lane keeps its 16
// rows' limits in registers from the first tile to the last.  Count: a ballot per accumulator element, its two half-wave popcounts
// added to the 32 counters of the wave's rows -- wave-uniform numbers in scalar registers, no lane holds any.  Fill: a 64-bit write position per row in LDS, owned by the row's wave; half-wave
// ballots give the lanes their places.  Tiles, column blocks and lanes ascend, so a segment is the same on every run.
// Both passes form the same d^ from the same instructions on the same operands, so the fill finds what the count counted;
// it still never writes behind a (query, part)'s counted end.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_exact_mfma.h"
#include "device_range.h"

namespace cph {

// Workgroups per CU the kernel is compiled for: 75 KiB of LDS each, two fit.  (profiles/range_matrix.md: resource usage
// of both settings.)
constexpr int kRangeMxOccupancy = 2;

struct RangeMatrixArgs {
    MxTileArgs t;                         // (c_lo, c_hi, q_row0, q_last: set per workgroup)
    const float* eps;                     // [nq]
    const float* radius;                  // [nq]
    uint32_t m;                           // candidates
    uint64_t part;                        // candidates per part (a multiple of 128)
    uint32_t P;
    uint32_t nq, q_first, q_count;        // the batch; the queries of this launch
    uint32_t* counts;                     // [nq][P]         count: written
    const unsigned long long* soffs;      // [nq * P + 1]    fill: read
    uint32_t* sids;                       // [survivors]     fill: written
};

// Row of accumulator element i of lane half h, relative to the wave's first row.
__device__ __forceinline__ int mx_acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

template <bool LIST, bool FILL>
struct RangeMatrixEpilogue {
    const RangeMatrixArgs& a;
    const uint32_t c_lo, c_hi, rows;      // the part; live rows of the tile (<= 128)
    unsigned long long* s_pos;            // [128] fill: next free index of sids per row
    unsigned long long* s_end;            // [128] fill: the (query, part)'s counted end
    const int wrow, h, c, lane;
    float lm[16];
    uint32_t cnt[16][2];                  // count: survivors per row (element i, half h), wave-uniform: scalar registers

    __device__ __forceinline__ void begin(const float (&)[16]) {
        const uint32_t q0 = a.q_first + blockIdx.y * kMxTile + (uint32_t)wrow;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t r = (uint32_t)(wrow + mx_acc_row(i, h));
            const uint32_t q = q0 + (uint32_t)mx_acc_row(i, h);
            lm[i] = r < rows ? range_matrix_limit(a.radius[q], a.eps[q]) : -1.0f;
            cnt[i][0] = cnt[i][1] = 0;
        }
    }

    // survives: not (d^ finite and d^ >= lim).  d = qn - 2 s is d^ before its clamp at 0, which no limit tells apart
    // (lim is -1, NaN or > 0).
    __device__ __forceinline__ static bool survives(float s, float qn, float lim) {
        const float d = __fmaf_rn(-2.0f, s, qn);
        return !(d >= lim && d < __builtin_inff());
    }

    __device__ __forceinline__ void tile(uint32_t tile, const knn_f32x16 (&acc)[4], const float (&qn)[16]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t col = c_lo + tile * kMxTile + t * 32 + c;
            const bool ok = col < c_hi;
            if constexpr (!FILL) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const unsigned long long mask = __ballot(ok && survives(acc[t][i], qn[i], lm[i]));
                    cnt[i][0] += (uint32_t)__popc((uint32_t)mask);
                    cnt[i][1] += (uint32_t)__popc((uint32_t)(mask >> 32));
                }
            } else {
                bool any = false;
#pragma unroll
                for (int i = 0; i < 16; ++i) any = any || survives(acc[t][i], qn[i], lm[i]);
                if (!__any(ok && any)) continue;
                uint32_t id = 0;
                if (ok) {
                    if constexpr (LIST) id = a.t.ids[col];
                    else id = col;
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const bool pass = ok && (uint32_t)(wrow + mx_acc_row(i, h)) < rows && survives(acc[t][i], qn[i], lm[i]);
                    if (__ballot(pass) == 0) continue;
                    // the 32 lanes of a half share the row; the two halves take their turns (wave-uniform)
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const int rr = wrow + mx_acc_row(i, hh);
                        const bool mine = pass && h == hh;
                        const uint32_t mh = (uint32_t)(__ballot(mine) >> (32 * hh));
                        if (mh == 0) continue;
                        const unsigned long long at = s_pos[rr], to = at + (uint32_t)__popc(mh & ((1u << c) - 1u));
                        if (mine && to < s_end[rr]) a.sids[to] = id;
                        if (lane == 0) s_pos[rr] = at + (uint32_t)__popc(mh);
                        mx_wave_sync();
                    }
                }
            }
        }
    }

    // count: lane (h, c < 16) writes the counter of its half's row of element c
    __device__ __forceinline__ void finish() {
        if constexpr (!FILL) {
            uint32_t mine = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) mine = c == i ? (h ? cnt[i][1] : cnt[i][0]) : mine;
            const uint32_t r = (uint32_t)(wrow + mx_acc_row(c & 15, h));
            if (c < 16 && r < rows)
                a.counts[(size_t)(a.q_first + blockIdx.y * kMxTile + r) * a.P + blockIdx.x] = mine;
        }
    }
};

// Grid (P, ceil(q_count / 128)), 256 threads, no dynamic LDS.
template <bool LIST, bool FILL>
__global__ __launch_bounds__(256, kRangeMxOccupancy) void range_mfma_kernel(RangeMatrixArgs a) {
    __shared__ __align__(16) MxOperandLds L;
    __shared__ unsigned long long s_pos[FILL ? kMxTile : 1], s_end[FILL ? kMxTile : 1];
    const int tid = threadIdx.x;
    const uint64_t p_lo = (uint64_t)blockIdx.x * a.part;
    const uint32_t c_lo = (uint32_t)min(p_lo, (uint64_t)a.m), c_hi = (uint32_t)min(p_lo + a.part, (uint64_t)a.m);
    const uint32_t ql0 = blockIdx.y * kMxTile;
    if (c_lo >= c_hi || ql0 >= a.q_count) return;       // (no part of the plan is empty: every counter is written)
    const uint32_t rows = min(kMxTile, a.q_count - ql0);
    if constexpr (FILL) {
        if (tid < (int)rows) {
            const size_t at = (size_t)(a.q_first + ql0 + (uint32_t)tid) * a.P + blockIdx.x;
            s_pos[tid] = a.soffs[at];
            s_end[tid] = a.soffs[at + 1];
        }
    }
    MxTileArgs t = a.t;
    t.c_lo = c_lo;
    t.c_hi = c_hi;
    t.q_row0 = a.q_first + ql0;
    t.q_last = a.q_first + a.q_count - 1;
    const int lane = tid & 63;
    RangeMatrixEpilogue<LIST, FILL> epi{a, c_lo, c_hi, rows, s_pos, s_end, (tid >> 6) * 32, lane >> 5, lane & 31, lane, {}, {}};
    mx_scan_tiles<LIST>(t, L, epi);
    epi.finish();
}

// ---- re-score: a wave per run ------------------------------------------------------------------------------------------------
// The sink of exact_scan_candidates for ONE query and the ids of one run: candidate block b's keys go to sm[64 b ..].  A
// hit (d < radius, strict; a NaN radius selects nothing) is distance bits << 32 | id, as everywhere.  A survivor that is
// not a hit is 0xFFFFFFFF << 32 | id: behind every hit, and unique -- range_merge_dest requires unique keys, a long
// segment can hold thousands of non-hits, and no id is 0xFFFFFFFF, so none of them is kExactNoKey, the padding of the sort.
// LDS: the keys, then the words {next block's first slot, hits}.
struct RangeRescoreSink {
    unsigned long long* sm;
    uint32_t* s_at;
    float radius;

    __device__ __forceinline__ void take(uint32_t, float d, uint32_t id, bool live, int lane) const {
        const uint32_t at = s_at[0];
        const bool hit = live && d < radius;
        const unsigned long long mask = __ballot(hit);
        sm[at + lane] = !live ? kExactNoKey : ((unsigned long long)(hit ? __float_as_uint(d) : 0xFFFFFFFFu) << 32) | id;
        if (lane == 0) {
            s_at[0] = at + 64;
            s_at[1] += (uint32_t)__popcll(mask);
        }
    }
    __device__ __forceinline__ void finish(uint32_t, int) const {}
};

struct RangeRescoreArgs {
    ScanCommon s;                         // (gq, part, q_first, q_count: unused)
    const float* radius;                  // [nq]
    const RangeRun* runs;                 // start, len (1 .. kRangeRun), reserved = the query
    const uint32_t* sids;                 // the survivors' ids; a query's segment ascending
    unsigned long long* arena;            // the keys, at the index of their id in sids
    uint32_t* hits;                       // [nq], zero before the launch
};

// One wave per run; dynamic LDS: the launch's longest run rounded up to a power of two (>= 64) keys, and 8 bytes.
template <int SD, int CH>
__global__ __launch_bounds__(64) void range_rescore_runs_kernel(RangeRescoreArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const RangeRun r = a.runs[blockIdx.x];
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    const int lane = threadIdx.x;
    const uint32_t q = r.reserved;
    uint32_t N = 64;
    while (N < r.len) N <<= 1;
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(smem);
    uint32_t* s_at = reinterpret_cast<uint32_t*>(smem + (size_t)N * 8);
    for (uint32_t i = lane; i < N; i += 64) sm[i] = kExactNoKey;
    if (lane < 2) s_at[lane] = 0;
    __syncthreads();
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, ExactListSource{a.sids + r.start}, 0u, r.len,
                                  (exact_uniform_ptr)(a.s.qpad + (size_t)q * D), (exact_uniform_ptr)(a.s.qnorm + q), 1u,
                                  RangeRescoreSink{sm, s_at, a.radius[q]});
    __syncthreads();
    const uint32_t nh = s_at[1];
    exact_sort_keys(sm, N, lane);
    unsigned long long* keys = a.arena + r.start;
    for (uint32_t i = lane; i < r.len; i += 64) keys[i] = sm[i];
    if (lane == 0 && nh) atomicAdd(a.hits + q, nh);
}

// One block per query: the first hits of its sorted segment -> ids (through `rows` if given) and distances at lims[q].  A
// segment longer than kRangeRun is read from `keys_long` (where its last merge pass left it), any other from `keys`.
__global__ __launch_bounds__(256) void range_emit_hits_kernel(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ keys_long,
                                                              const unsigned long long* __restrict__ slims, const unsigned long long* __restrict__ lims,
                                                              const uint32_t* __restrict__ rows, int64_t* __restrict__ out_ids,
                                                              float* __restrict__ out_dist) {
    const uint32_t q = blockIdx.x;
    const unsigned long long s0 = slims[q], lo = lims[q], nh = lims[q + 1] - lo;
    const unsigned long long* src = (slims[q + 1] - s0 > kRangeRun ? keys_long : keys) + s0;
    for (unsigned long long i = threadIdx.x; i < nh; i += 256) {
        const unsigned long long key = src[i];
        const uint32_t id = (uint32_t)key;
        out_ids[lo + i] = (int64_t)(rows ? rows[id] : id);
        out_dist[lo + i] = __uint_as_float((uint32_t)(key >> 32));
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// The work split: plan_exact_matrix's rule without the pool term -- two workgroups per CU asked for, many parts when there
// are few query tiles, few when the tiles alone fill the GPU, never more than kExactMaxParts.
struct RangeMatrixPlan {
    uint32_t P;
    uint64_t part;        // a multiple of 128
};

inline RangeMatrixPlan plan_range_matrix(uint64_t m, uint64_t nq, int num_cus) {
    RangeMatrixPlan pl{};
    const uint64_t wgs = (uint64_t)std::max(1, num_cus) * 2, blocks = (m + kMxTile - 1) / kMxTile;
    const uint64_t T = std::max<uint64_t>(1, (nq + kMxTile - 1) / kMxTile);
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>({(wgs + T - 1) / T, blocks, (uint64_t)kExactMaxParts}));
    pl.part = (blocks + want - 1) / want * kMxTile;
    pl.P = (uint32_t)std::max<uint64_t>(1, (m + pl.part - 1) / pl.part);
    return pl;
}

// The budget rule: a survivor costs its id (4 bytes) and its key (8), the key twice where a segment needs merge passes.
// A call whose survivors exceed the scratch budget continues on the vector route, from that route's count pass.
inline bool range_matrix_fits(uint64_t survivors, bool any_long, uint64_t budget) {
    return survivors <= budget / (any_long ? 20u : 12u);
}

}  // namespace cph
