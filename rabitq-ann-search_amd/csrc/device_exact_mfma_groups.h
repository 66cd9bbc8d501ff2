// device_exact_mfma_groups.h — the "matrix" engine (device_exact_mfma.h) for a batch with per-query filters: the scanned
// SEGMENTS of such a batch (a filter's id list, or the whole index, with the queries that name it: device_exact.h, the
// grouped scan) go through a grouped matrix-core prefilter and a grouped certify kernel.  The bound, the keep rule, the
// pool geometry and the operand pipeline are those of device_exact_mfma.h; nothing is re-derived here.  Every output byte
// is the vector engine's.
//
// Stages of one launch (a set of whole (segment, tile of <= 128 queries) units whose scratch fits the budget), one stream:
//   1. exact_mfma_prefilter_groups_kernel  a 1-D grid over a table of MatrixItems: one (segment, query tile, part of whole
//                                          128-candidate tiles) per workgroup of 256, mx_scan_tiles with the selection as the
//                                          tile epilogue
//   2. exact_mfma_certify_groups_kernel    one wave per query of the launch, driven by its descriptor: mx_certify_query over
//                                          the parts of its OWN segment, the row to the query's original batch row
// and behind every launch of the call
//   3. exact_scan_groups_flagged_kernel /  the grouped vector plan over the same segments, for the flagged queries only
//      exact_merge_groups_flagged_kernel
//
// LIST and non-LIST segments share ONE launch: an item's id list pointer is wave-uniform (scalar loads), the kernel
// branches on it once, in front of the pipeline, into the two instantiations of mx_scan_tiles.  Only the unfiltered queries
// of a call (-1) make a non-LIST segment, one at most; a launch of its own would leave its few workgroups running alone
// behind the LIST items instead of beside them.  The branch costs code size, no instruction in the tile loop.
//
// Pools: unit (segment, tile) of `rows` live queries and P parts owns P x rows consecutive pool indices of its launch; item
// (part p) has pool = base + p rows, row r of the tile the pool pool + r; query r's descriptor is (base + r, rows, P, its
// batch row) -- the layout of the grouped vector scan.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "device_exact_mfma.h"

namespace cph {

// A scanned segment of a per-query call takes the matrix kernels from this many queries on; a smaller one stays in the
// grouped vector scan of the same call.  The measured cut-over (profiles/exact_matrix_groups.md); 16 < it <= 128: at 16
// queries the vector engine wins, at one full tile the matrix engine does (profiles/exact_matrix.md).
constexpr uint32_t kMxGroupMinQueries = 64;
static_assert(16 < kMxGroupMinQueries && kMxGroupMinQueries <= kMxTile, "the cut-over lies between 16 queries and one tile");

struct MatrixItem {               // 32 bytes, read through scalar loads
    const uint32_t* ids;          // the segment's ascending id list, or null: candidate c is id c
    uint32_t c_lo, c_hi;          // candidates of this part, c_lo < c_hi, c_lo a multiple of 128
    uint32_t q_row0, q_rows;      // first padded query row of the tile, its live rows (1 .. 128)
    uint32_t pool;                // pool (and count) index of (this part, row q_row0); row q_row0 + r: pool + r
    uint32_t reserved;
};

struct MatrixGroupArgs {
    const float* raw;             // [n][D]
    const float* norm_sq;         // [n]
    const float* qpad;            // the padded scan rows (permuted: a segment's queries are consecutive)
    const float* qnorm;
    const float* eps;             // [scan rows]
    uint32_t D, k, C;
    unsigned long long* pools;    // [pools of the launch][C]
    uint32_t* counts;             // [pools of the launch]
    uint32_t* flags;              // [scan rows]
    const MatrixItem* items;      // [gridDim.x]
};

// The selection of exact_mfma_prefilter_kernel as the tile epilogue of mx_scan_tiles: per finished tile a compare per
// accumulator against its row's limit tau + 2 eps, ballot appends into the row's pool, mx_sort_keep on overflow, the flag
// where no append of a full half-wave pair fits or a d^ is not finite.  A row's state (cnt, lim_s) belongs to one wave.
template <bool LIST>
struct MatrixGroupEpilogue {
    const MatrixGroupArgs& a;
    const MatrixItem& it;
    uint32_t* cnt;                // [128] keys in the row's pool
    float* lim_s;                 // [128] the row's limit (-1: takes nothing)
    const float* eps2_s;          // [128] 2 eps
    unsigned long long* sm;       // the wave's compaction buffer, C keys
    const int wrow, h, c, lane;
    float lm[16];

    __device__ __forceinline__ uint32_t row_of(int i) const { return (uint32_t)(wrow + (i & 3) + 8 * (i >> 2) + 4 * h); }

    __device__ __forceinline__ void begin(const float (&)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) lm[i] = lim_s[row_of(i)];
    }

    __device__ __forceinline__ void tile(uint32_t tile, const knn_f32x16 (&acc)[4], const float (&qn)[16]) {
        const uint32_t q_last = it.q_row0 + it.q_rows - 1;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint64_t col = (uint64_t)it.c_lo + (uint64_t)tile * kMxTile + (uint32_t)(t * 32 + c);   // this lane's candidate
            const bool ok = col < it.c_hi;
            // "is any of my 16 distances within its row's limit" as one max-reduction, "is any of them not finite" as one
            // fma chain (x * 0 is 0 for every finite x, NaN otherwise)
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
                    if (ok && !(fabsf(__fmaf_rn(-2.0f, acc[t][i], qn[i])) <= FLT_MAX)) a.flags[min(it.q_row0 + row_of(i), q_last)] = 1u;
            }
            if (!__any(ok && lead >= 0.0f)) continue;
            uint32_t id = (uint32_t)min(col, (uint64_t)it.c_hi - 1);
            if constexpr (LIST) id = it.ids[id];
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
                    if (mh == 0) continue;                               // (a dead row's limit is -1: it never gets here)
                    uint32_t base = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt[rr]);
                    unsigned long long* pool = a.pools + ((size_t)it.pool + (uint32_t)rr) * a.C;
                    if (base + __popc(mh) > a.C) {
                        // the pool is full: sort, set tau, keep what the rule keeps, and look again
                        __threadfence();                                 // the appended keys, written by single lanes, are visible
                        for (uint32_t x = lane; x < base; x += 64) sm[x] = pool[x];
                        uint32_t lb;
                        uint32_t kept = mx_sort_keep(sm, base, a.k, eps2_s[rr], lane, lb);
                        float nl = __uint_as_float(lb);
                        if (kept + 64 > a.C) {                           // no room for the next append: not certifiable here
                            if (lane == 0) a.flags[it.q_row0 + (uint32_t)rr] = 1u;
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
                for (int i = 0; i < 16; ++i) lm[i] = lim_s[row_of(i)];
            }
        }
    }
};

template <bool LIST>
__device__ __forceinline__ void mx_group_item(const MatrixGroupArgs& a, const MatrixItem& it, MxOperandLds& L, uint32_t* cnt, float* lim_s,
                                              float* eps2_s, unsigned long long* sm) {
    const int lane = threadIdx.x & 63;
    MxTileArgs t{};
    t.raw = a.raw;
    t.norm_sq = a.norm_sq;
    t.qpad = a.qpad;
    t.qnorm = a.qnorm;
    t.ids = it.ids;
    t.D = a.D;
    t.c_lo = it.c_lo;
    t.c_hi = it.c_hi;
    t.q_row0 = it.q_row0;
    t.q_last = it.q_row0 + it.q_rows - 1;          // rows behind it are clamped to it: never another segment's query
    MatrixGroupEpilogue<LIST> epi{a, it, cnt, lim_s, eps2_s, sm, (int)(threadIdx.x >> 6) * 32, lane >> 5, lane & 31, lane, {}};
    mx_scan_tiles<LIST>(t, L, epi);
}

// Grid: the items of the launch; 256 threads; dynamic LDS: 4 x C keys (a compaction buffer per wave).  One workgroup per
// CU, as exact_mfma_prefilter_kernel (76 KiB of images and row state, up to 64 KiB of buffers).
__global__ __launch_bounds__(256, 1) void exact_mfma_prefilter_groups_kernel(MatrixGroupArgs a) {
    __shared__ __align__(16) MxOperandLds L;
    __shared__ uint32_t cnt[kMxTile];
    __shared__ float lim_s[kMxTile];
    __shared__ float eps2_s[kMxTile];
    extern __shared__ __align__(16) unsigned char mx_smem[];
    typedef __attribute__((address_space(4))) const uint32_t* word_ptr;
    const word_ptr w = (word_ptr)reinterpret_cast<const uint32_t*>(a.items + blockIdx.x);   // workgroup-uniform: scalar loads
    MatrixItem it;
    it.ids = reinterpret_cast<const uint32_t*>((uint64_t)w[0] | ((uint64_t)w[1] << 32));
    it.c_lo = w[2]; it.c_hi = w[3]; it.q_row0 = w[4]; it.q_rows = min(w[5], kMxTile); it.pool = w[6];
    if (it.c_lo >= it.c_hi || it.q_rows == 0) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned long long* sm = reinterpret_cast<unsigned long long*>(mx_smem) + (size_t)wave * a.C;
    if (tid < (int)kMxTile) {
        const uint32_t q = it.q_row0 + (uint32_t)tid;
        const bool live = (uint32_t)tid < it.q_rows && a.flags[q] == 0;          // (a flagged query is the fallback's)
        cnt[tid] = 0;
        lim_s[tid] = live ? __builtin_inff() : -1.0f;
        eps2_s[tid] = live ? 2.0f * a.eps[q] : 0.0f;
    }
    // (mx_scan_tiles publishes the row state with the barrier behind its first image)
    if (it.ids) mx_group_item<true>(a, it, L, cnt, lim_s, eps2_s, sm);
    else mx_group_item<false>(a, it, L, cnt, lim_s, eps2_s, sm);
    // the part is done: every pool of this wave cut once more; its fill count published
    const int wrow = wave * 32;
    for (int r = 0; r < 32; ++r) {
        if ((uint32_t)(wrow + r) >= it.q_rows) break;
        const size_t pi = (size_t)it.pool + (uint32_t)(wrow + r);
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

// ---- certify ------------------------------------------------------------------------------------------------------------------
struct MatrixCertifyGroupArgs {
    MatrixCertifyCommon c;        // (c.s.q_first: the first scan row of the launch; rpools, rcounts: indexed from it)
    const uint4* desc;            // [queries of the launch]: first pool, stride between its parts, parts of its segment, batch row
};

// One wave per query of the launch.  LDS: that of exact_mfma_certify_kernel.  The survivors' keys carry internal ids, so the
// segment's id list is not read again.
template <int SD, int CH>
__global__ __launch_bounds__(64) void exact_mfma_certify_groups_kernel(MatrixCertifyGroupArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint4 d = a.desc[blockIdx.x];
    mx_certify_query<SD, CH>(a.c, d.x, d.y, d.z, blockIdx.x, a.c.s.q_first + blockIdx.x, d.w, smem);
}

// ---- the fallback: the grouped vector scan and merge, for flagged queries only ---------------------------------------------------
struct ExactGroupFlaggedArgs {
    ExactGroupArgs a;
    const uint32_t* flags;        // [scan rows]
};

template <int SD, int CH>
__global__ __launch_bounds__(64) void exact_scan_groups_flagged_kernel(ExactGroupFlaggedArgs f) {
    extern __shared__ __align__(16) unsigned char smem[];
    const ExactGroupArgs& a = f.a;
    const ExactItem it = a.items[blockIdx.x];
    const uint32_t D = SD ? (uint32_t)SD : a.s.D;
    if (it.c_lo >= it.c_hi || it.q_cnt == 0) return;
    bool any = false;
    for (uint32_t j = threadIdx.x; j < it.q_cnt; j += 64) any = any || f.flags[it.q_lo + j] != 0;
    if (!__any(any)) return;
    exact_scan_candidates<SD, CH>(a.s.raw, a.s.norm_sq, D, ExactListSource{it.ids}, it.c_lo, it.c_hi,
                                  (exact_uniform_ptr)(a.s.qpad + (size_t)it.q_lo * D), (exact_uniform_ptr)(a.s.qnorm + it.q_lo), it.q_cnt,
                                  ExactPoolSink(smem, a.s.gq, a.pools + (size_t)it.pool * a.C, a.counts + it.pool, a.k, a.C));
}

// One wave per scan row of the launch; desc and flags start at the launch's first row.
__global__ __launch_bounds__(64) void exact_merge_groups_flagged_kernel(const unsigned long long* __restrict__ pools,
                                                                        const uint32_t* __restrict__ counts, const uint4* __restrict__ desc,
                                                                        uint32_t k, uint32_t C, const uint32_t* __restrict__ rows,
                                                                        const uint32_t* __restrict__ flags, unsigned long long* stats,
                                                                        int64_t* __restrict__ out_ids, float* __restrict__ out_dist) {
    extern __shared__ __align__(16) unsigned char smem[];
    if (!flags[blockIdx.x]) return;
    if (threadIdx.x == 0) atomicAdd(stats + kStatMatrixRedo, 1ull);
    const uint4 d = desc[blockIdx.x];
    exact_merge_query(pools, counts, d.x, d.y, d.z, k, C, rows, out_ids, out_dist, d.w, smem);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// plan_exact_matrix's rules per segment, as plan_exact_groups applies plan_exact's.  Segment s: seg_m[s] candidates against
// seg_q[s] queries (one with no candidate or no query gets no item: the caller zeroes the segments of the vector route).
// Every segment is cut into tiles of at most 128 queries and into parts of whole 128-candidate tiles, at most
// kExactMaxParts; the parts are sized over ALL segments, about two workgroups per CU of equal tile count.  The plan is an
// ExactGroupPlan with gq = 128: items ordered by (launch, segment, tile, part), a unit (segment, tile) of P parts and r rows
// takes P r pools.  A launch takes whole units while its scratch -- pools and counts, and the certify kernel's pool and
// count per query -- fits the budget; a unit that alone would not fit gets fewer parts (one at least).
inline size_t matrix_group_bytes(uint64_t pools, uint64_t rows, uint32_t C) { return (size_t)((pools + rows) * ((uint64_t)C * 8 + 4)); }

struct MatrixGroupPlan {
    ExactGroupPlan g;
    std::vector<uint32_t> launch_rows;        // [launches]: queries launch l certifies
    uint32_t max_rows = 0, max_parts = 0;
    size_t max_bytes = 0;                     // matrix_group_bytes of the largest launch
};

inline MatrixGroupPlan plan_exact_matrix_groups(const uint64_t* seg_m, const uint64_t* seg_q, uint32_t n_seg, uint32_t k, int num_cus,
                                                size_t budget) {
    MatrixGroupPlan mp;
    ExactGroupPlan& pl = mp.g;
    pl.Kp = 64;
    while (pl.Kp < k) pl.Kp <<= 1;
    pl.C = 2 * pl.Kp;
    pl.gq = kMxTile;
    const uint64_t wgs = (uint64_t)std::max(1, num_cus) * 2;
    const uint64_t budget_pools = std::max<uint64_t>(2, (uint64_t)budget / ((uint64_t)pl.C * 8 + 4));   // pools and certify pools
    uint64_t total = 0;                       // candidate tiles x query tiles
    for (uint32_t s = 0; s < n_seg; ++s)
        if (seg_m[s] && seg_q[s]) total += ((seg_m[s] + kMxTile - 1) / kMxTile) * ((seg_q[s] + kMxTile - 1) / kMxTile);
    const uint64_t per = std::max<uint64_t>(1, (total + wgs - 1) / wgs);         // candidate tiles per item
    pl.seg_parts.assign(n_seg, 0);
    pl.launch_items.push_back(0);
    uint64_t used = 0, rows = 0;
    uint32_t launch = 0;
    auto close = [&]() {
        pl.launch_items.push_back((uint32_t)pl.items.size());
        pl.launch_pools.push_back((uint32_t)used);
        mp.launch_rows.push_back((uint32_t)rows);
        mp.max_bytes = std::max(mp.max_bytes, matrix_group_bytes(used, rows, pl.C));
        mp.max_rows = std::max(mp.max_rows, (uint32_t)rows);
        used = rows = 0;
        ++launch;
    };
    for (uint32_t s = 0; s < n_seg; ++s) {
        if (!seg_m[s] || !seg_q[s]) continue;
        const uint64_t m = seg_m[s], blocks = (m + kMxTile - 1) / kMxTile, widest = std::min<uint64_t>(kMxTile, seg_q[s]);
        uint64_t want = std::min<uint64_t>({(blocks + per - 1) / per, blocks, (uint64_t)kExactMaxParts});
        want = std::max<uint64_t>(1, std::min<uint64_t>(want, budget_pools / widest - std::min<uint64_t>(1, budget_pools / widest)));
        const uint64_t part = (blocks + want - 1) / want * kMxTile;              // (64 bits: up to 2^32 - 128)
        const uint32_t P = (uint32_t)((m + part - 1) / part);
        pl.seg_parts[s] = P;
        mp.max_parts = std::max(mp.max_parts, P);
        for (uint64_t q0 = 0; q0 < seg_q[s]; q0 += kMxTile) {
            const uint32_t qc = (uint32_t)std::min<uint64_t>(kMxTile, seg_q[s] - q0);
            const uint64_t need = (uint64_t)P * qc;
            if (used && used + need + rows + qc > budget_pools) close();
            for (uint32_t p = 0; p < P; ++p)
                pl.items.push_back(ExactGroupItem{s, p, (uint32_t)(p * part), (uint32_t)std::min<uint64_t>(m, (uint64_t)(p + 1) * part),
                                                  (uint32_t)q0, qc, (uint32_t)(used + (uint64_t)p * qc), launch});
            used += need;
            rows += qc;
        }
    }
    if (used) close();
    pl.max_pools = 0;
    for (uint32_t x : pl.launch_pools) pl.max_pools = std::max(pl.max_pools, x);
    return mp;
}

}  // namespace cph
