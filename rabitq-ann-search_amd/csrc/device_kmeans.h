// device_kmeans.h — k-means (Lloyd) over the rows a finalized handle holds (cph_kmeans): the assignment on the matrix
// cores, certified against the vector arithmetic; the update as a stable counting sort and sequential sums.  Nothing here
// uses a floating-point atomic, and no result depends on the order in which workgroups run.
//
// The assignment of row x is DEFINED without the matrix cores: the centroid c with the smallest (d bits, c), where d has the
// bits cph_exact_l2 returns for query = centroid c, id = x (device_exact.h: eight chains over the padded rows, qnorm the
// same chains over the centroid, norm = norm_sq[x]).  The matrix cores only find, for most rows, a centroid that provably
// is that argmin:
//
//   1. kmeans_assign_mfma_kernel   n x k x D on v_mfma_f32_32x32x2_f32.  Grid: tiles of 128 ROWS, straight from the
//        resident row and norm arrays; every workgroup walks all centroid tiles of 128 columns through mx_scan_tiles
//        (device_exact_mfma.h: the rows are its "queries", the centroids its candidates, not a list).  The epilogue has
//        no pool, no selection state in HBM and no compaction: a lane keeps (best d^, its centroid, second-best d^) in
//        registers for each of its 16 rows across ALL tiles; behind the last tile one butterfly over the 32 lanes of a
//        half folds them per row.  Columns behind k repeat the last centroid and are masked (last tile only).
//        Certification (the bound of device_exact_mfma.h at k = 1): eps = exact_matrix_slack(norm_sq[x], cn_max, D),
//        cn_max the largest centroid norm; if second > (best + 2 eps) rounded up (mx_limit), every other centroid has
//        d >= d^ - eps > best d^ + eps >= d of the best column: the best column is the strict argmin of the vector
//        arithmetic.  "All numbers finite" is asked of the inputs: norm_sq[x] + cn_max <= FLT_MAX / 4 (false for a NaN)
//        bounds every product sum, every accumulator and every d^ of the row below FLT_MAX.  A live row that is not
//        certified is appended to the uncertain list (one integer atomic per wave, vector stores).
//   2. kmeans_resolve_kernel       one wave per 64 uncertain rows -- a lane owns a row, as in THE candidate loop
//        (exact_scan_candidates), whose "queries" here are all k centroids: the minimum by (distance bits, centroid id).
//   3. the update, a stable counting sort of the live rows by cluster and a sum per cluster:
//        kmeans_hist_kernel      per segment of rows (host_kmeans.h: kmeans_segments) a histogram [segments][k] with
//                                integer LDS atomics; also counts the rows whose assignment changed (moved[it])
//        kmeans_offsets_kernel   per cluster the exclusive scan over the segments; kmeans_starts_kernel the scan over clusters
//        kmeans_scatter_kernel   one wave per segment ranks its rows in id order: a cluster's members ascend by id
//        kmeans_reduce_kernel    workgroup (cluster, slice of 64 coordinates): lanes own coordinates, wave w sums members
//                                w, w + 4, ... sequentially, ((p0 + p1) + p2) + p3, one division (host_kmeans.h:
//                                kmeans_mean_host).  A cluster without members keeps its centroid.
//   4. kmeans_final_kernel         dist[i] = the exact_l2 bits of (assigned centroid, row i), counts; -1 / FLT_MAX for
//                                removed rows.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "device_exact.h"
#include "device_exact_mfma.h"
#include "device_range_mfma.h"
#include "host_kmeans.h"

namespace cph {

// Workgroups per CU the assign kernel is compiled for.  Two would fit by LDS (75 KiB each), but the 48 registers of a lane's
// (best, centroid, second) triples next to the operand pipeline do not fit in 256: at 2 the compiler spills 240 of them.
constexpr int kKmeansOccupancy = 1;

__device__ __forceinline__ bool kmeans_removed(const uint32_t* __restrict__ removed, uint32_t i) {
    return removed && ((removed[i >> 5] >> (i & 31)) & 1u);
}

// ---- set-up -------------------------------------------------------------------------------------------------------------------
// The call's counters to 0, the "previous" assignment to -1 (no row had one).
__global__ __launch_bounds__(256) void kmeans_reset_kernel(int32_t* __restrict__ prev, uint32_t n, uint32_t* __restrict__ unc_counts,
                                                           uint32_t passes, unsigned long long* __restrict__ moved, uint32_t iters,
                                                           unsigned long long* __restrict__ counts, uint32_t k) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) prev[i] = -1;
    if (i < passes) unc_counts[i] = 0;
    if (i < iters) moved[i] = 0;
    if (i < k) counts[i] = 0;
}

// cent[k + kExactQT][D]: row c = init row c zero-padded (ids null), or stored row ids[c]; the kExactQT rows behind k are
// zero (the resolve kernel's last query tile reads them).  One wave per row.
__global__ __launch_bounds__(64) void kmeans_seed_kernel(const float* __restrict__ init, const uint32_t* __restrict__ ids,
                                                         const float* __restrict__ raw, uint32_t k, uint32_t dim, uint32_t D,
                                                         float* __restrict__ cent) {
    const uint32_t c = blockIdx.x;
    for (uint32_t d = threadIdx.x; d < D; d += 64) {
        float x = 0.0f;
        if (c < k) x = ids ? raw[(size_t)ids[c] * D + d] : (d < dim ? init[(size_t)c * dim + d] : 0.0f);
        cent[(size_t)c * D + d] = x;
    }
}

// cnorm[c] = the query norm of centroid c: the eight chains and the tree of exact_pad_rows.  Eight lanes per centroid; the
// kExactQT entries behind k are 0.
__global__ __launch_bounds__(256) void kmeans_cnorm_kernel(const float* __restrict__ cent, uint32_t k, uint32_t D, float* __restrict__ cnorm) {
    const uint32_t c = blockIdx.x * 32 + (threadIdx.x >> 3), j = threadIdx.x & 7;
    const uint32_t cc = min(c, k + kExactQT - 1);                     // (whole groups stay converged for the exchange)
    float s = 0.0f;
    for (uint32_t i = j; i < D; i += 8) {
        const float x = cent[(size_t)cc * D + i];
        s = __fmaf_rn(x, x, s);
    }
    s = group_reduce8(s);
    if (j == 0 && c < k + kExactQT) cnorm[c] = s;
}

// ---- 1. the assignment on the matrix cores ----------------------------------------------------------------------------------
struct KmeansAssignArgs {
    MxTileArgs t;                         // raw / norm_sq: the centroids and their norms; qpad / qnorm: the rows and theirs
    const uint32_t* cn_max;               // bits of the largest centroid norm
    const uint32_t* removed;              // bitmap of removed rows, or null
    uint32_t n, k;
    int32_t* assign;                      // [n]  written for certified and removed rows
    uint32_t* unc_ids;                    // [n]  the uncertain rows, in any order
    uint32_t* unc_count;
};

struct KmeansAssignEpilogue {
    const KmeansAssignArgs& a;
    const int wrow, h, c;
    float best[16], second[16];
    uint32_t bidx[16];

    __device__ __forceinline__ void begin(const float (&)[16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            best[i] = second[i] = __builtin_inff();
            bidx[i] = 0;
        }
    }

    // Columns ascend inside a lane (tiles, then t), and only a strictly smaller d^ replaces the best: equal d^ leave
    // second == best, and the row goes to the vector arithmetic.
    template <bool MASK>
    __device__ __forceinline__ void fold(uint32_t tile, const knn_f32x16 (&acc)[4], const float (&qn)[16]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t col = tile * kMxTile + t * 32 + c;
            const bool ok = !MASK || col < a.k;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float d = __fmaf_rn(-2.0f, acc[t][i], qn[i]);
                float dh = d > 0.0f ? d : 0.0f;
                if (MASK) dh = ok ? dh : __builtin_inff();
                second[i] = __builtin_fminf(second[i], __builtin_fmaxf(best[i], dh));
                bidx[i] = dh < best[i] ? col : bidx[i];
                best[i] = __builtin_fminf(best[i], dh);
            }
        }
    }

    __device__ __forceinline__ void tile(uint32_t tile, const knn_f32x16 (&acc)[4], const float (&qn)[16]) {
        if ((tile + 1) * kMxTile > a.k) fold<true>(tile, acc, qn);       // (workgroup-uniform: the last tile)
        else fold<false>(tile, acc, qn);
    }

    // The 32 lanes of a half hold the columns of the same 16 rows: fold them (every lane ends with the row's triple),
    // then lane (h, c < 16) decides and writes the row of element c.
    __device__ __forceinline__ void finish() {
        float b = 0.0f, s = 0.0f;
        uint32_t x = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
#pragma unroll
            for (int d = 16; d > 0; d >>= 1) {
                const float ob = __shfl_xor(best[i], d), os = __shfl_xor(second[i], d);
                const uint32_t ox = (uint32_t)__shfl_xor((int)bidx[i], d);
                const bool other = ob < best[i] || (ob == best[i] && ox < bidx[i]);
                second[i] = __builtin_fminf(__builtin_fminf(second[i], os), __builtin_fmaxf(best[i], ob));
                bidx[i] = other ? ox : bidx[i];
                best[i] = other ? ob : best[i];
            }
            b = c == i ? best[i] : b;
            s = c == i ? second[i] : s;
            x = c == i ? bidx[i] : x;
        }
        const uint64_t row = (uint64_t)a.t.q_row0 + (uint32_t)(wrow + mx_acc_row(c & 15, h));
        const bool mine = c < 16 && row < a.n;
        const bool live = mine && !kmeans_removed(a.removed, (uint32_t)row);
        const float q = a.t.qnorm[min(row, (uint64_t)a.t.q_last)], cmax = __uint_as_float(*a.cn_max);
        const float eps2 = 2.0f * exact_matrix_slack(q, cmax, a.t.D);
        const bool certified = live && q + cmax <= FLT_MAX * 0.25f && s > mx_limit(b, eps2);
        if (mine && (certified || !live)) a.assign[row] = live ? (int32_t)x : -1;
        const bool uncertain = live && !certified;
        const unsigned long long mask = __ballot(uncertain);
        if (mask == 0) return;
        const int lane = (int)(threadIdx.x & 63);
        uint32_t base = 0;
        if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(a.unc_count, (uint32_t)__popcll(mask));
        base = (uint32_t)__shfl((int)base, __ffsll((long long)mask) - 1);
        if (uncertain) a.unc_ids[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)row;
    }
};

// Grid ceil(n / 128), 256 threads, no dynamic LDS.
__global__ __launch_bounds__(256, kKmeansOccupancy) void kmeans_assign_mfma_kernel(KmeansAssignArgs a) {
    __shared__ __align__(16) MxOperandLds L;
    const int tid = threadIdx.x, lane = tid & 63;
    MxTileArgs t = a.t;
    t.c_lo = 0;
    t.c_hi = a.k;
    t.q_row0 = blockIdx.x * kMxTile;
    t.q_last = a.n - 1;
    a.t = t;
    KmeansAssignEpilogue epi{a, (tid >> 6) * 32, lane >> 5, lane & 31, {}, {}, {}};
    mx_scan_tiles<false>(t, L, epi);
    epi.finish();
}

// ---- 2. the uncertain rows in the vector arithmetic -------------------------------------------------------------------------
// The sink of exact_scan_candidates for 64 rows (the loop's candidates) against all k centroids (its queries, in order):
// a lane keeps the smallest (distance bits << 32 | centroid) of its row and writes it behind the last centroid.
struct KmeansMinSink {
    int32_t* assign;
    uint32_t k;
    mutable unsigned long long best;

    __device__ __forceinline__ void take(uint32_t ql, float d, uint32_t id, bool live, int) const {
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | ql;
        best = (ql == 0 || key < best) ? key : best;
        if (ql + 1 == k && live) assign[id] = (int32_t)(uint32_t)best;
    }
    __device__ __forceinline__ void finish(uint32_t, int) const {}
};

struct KmeansResolveArgs {
    const float* raw;                     // the rows
    const float* norm_sq;
    const float* cent;                    // [k + kExactQT][D]
    const float* cnorm;                   // [k + kExactQT]
    const uint32_t* unc_ids;
    const uint32_t* unc_count;
    uint32_t D, k;
    int32_t* assign;
};

// Grid ceil(n / 64): the list's length is known on the device only, a wave behind its end leaves at once.
template <int SD, int CH>
__global__ __launch_bounds__(64) void kmeans_resolve_kernel(KmeansResolveArgs a) {
    const uint32_t D = SD ? (uint32_t)SD : a.D;
    const uint32_t count = *a.unc_count, c_lo = blockIdx.x * 64;
    if (c_lo >= count) return;
    exact_scan_candidates<SD, CH>(a.raw, a.norm_sq, D, ExactListSource{a.unc_ids}, c_lo, min(count, c_lo + 64), (exact_uniform_ptr)a.cent,
                                  (exact_uniform_ptr)a.cnorm, a.k, KmeansMinSink{a.assign, a.k, 0ull});
}

// ---- 3. the update ------------------------------------------------------------------------------------------------------------
// hist[s][c] = rows of segment s assigned to c; *moved += rows of the segment whose assignment differs from prev.
// Grid: segments; dynamic LDS: k words.
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int32_t* __restrict__ assign, const int32_t* __restrict__ prev, uint32_t n,
                                                          uint32_t seg_rows, uint32_t k, uint32_t* __restrict__ hist,
                                                          unsigned long long* moved) {
    extern __shared__ uint32_t km_bins[];
    for (uint32_t c = threadIdx.x; c < k; c += 256) km_bins[c] = 0;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * seg_rows, hi = min((uint64_t)n, lo + seg_rows);
    uint32_t changed = 0;
    for (uint64_t i0 = lo; i0 < hi; i0 += 256) {
        const uint64_t i = i0 + threadIdx.x;
        const int32_t c = i < hi ? assign[i] : -1;
        if (c >= 0) atomicAdd(&km_bins[c], 1u);
        changed += (uint32_t)__popcll(__ballot(i < hi && c != prev[i]));
    }
    if ((threadIdx.x & 63) == 0 && changed) atomicAdd(moved, (unsigned long long)changed);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < k; c += 256) hist[(size_t)blockIdx.x * k + c] = km_bins[c];
}

// hist[.][c] -> its exclusive scan over the segments; sizes[c] = the cluster's members.  One thread per cluster.
__global__ __launch_bounds__(256) void kmeans_offsets_kernel(uint32_t* __restrict__ hist, uint32_t segments, uint32_t k,
                                                             uint32_t* __restrict__ sizes) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= k) return;
    uint32_t run = 0;
    for (uint32_t s = 0; s < segments; ++s) {
        const uint32_t v = hist[(size_t)s * k + c];
        hist[(size_t)s * k + c] = run;
        run += v;
    }
    sizes[c] = run;
}

// starts[k + 1] = the exclusive scan of sizes[k].  ONE workgroup of 1024: a thread owns a run of consecutive clusters.
__global__ __launch_bounds__(1024) void kmeans_starts_kernel(const uint32_t* __restrict__ sizes, uint32_t k, uint32_t* __restrict__ starts) {
    __shared__ uint32_t s_wave[16];
    const uint32_t per = (k + 1023) / 1024, lo = min(k, threadIdx.x * per), hi = min(k, lo + per);
    uint32_t sum = 0;
    for (uint32_t c = lo; c < hi; ++c) sum += sizes[c];
    uint32_t x = sum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    uint32_t run = x - sum;
    for (int w = 0; w < wave; ++w) run += s_wave[w];
    for (uint32_t c = lo; c < hi; ++c) {
        starts[c] = run;
        run += sizes[c];
    }
    if (threadIdx.x == 1023) starts[k] = run;
}

// order[starts[c] + ...] = the members of cluster c, ascending by id.  Grid: segments, ONE wave each; dynamic LDS: k words,
// the next free slot of every cluster.  64 rows at a time, in id order; the lanes of one cluster take their places by
// ballot, cluster after cluster (at most 64 turns).
__global__ __launch_bounds__(64) void kmeans_scatter_kernel(const int32_t* __restrict__ assign, uint32_t n, uint32_t seg_rows, uint32_t k,
                                                            const uint32_t* __restrict__ hist, const uint32_t* __restrict__ starts,
                                                            uint32_t* __restrict__ order) {
    extern __shared__ uint32_t km_next[];
    const int lane = threadIdx.x;
    for (uint32_t c = lane; c < k; c += 64) km_next[c] = starts[c] + hist[(size_t)blockIdx.x * k + c];
    mx_wave_sync();
    const uint64_t lo = (uint64_t)blockIdx.x * seg_rows, hi = min((uint64_t)n, lo + seg_rows);
    for (uint64_t i0 = lo; i0 < hi; i0 += 64) {
        const uint64_t i = i0 + lane;
        const int32_t c = i < hi ? assign[i] : -1;
        unsigned long long todo = __ballot(c >= 0);
        while (todo) {
            const int first = __ffsll((long long)todo) - 1;
            const int32_t c0 = __shfl(c, first);
            const unsigned long long same = __ballot(c == c0);
            const uint32_t at = km_next[c0];
            if (c == c0) order[at + (uint32_t)__popcll(same & ((1ull << lane) - 1ull))] = (uint32_t)i;
            mx_wave_sync();
            if (lane == first) km_next[c0] = at + (uint32_t)__popcll(same);
            mx_wave_sync();
            todo &= ~same;
        }
    }
}

// Grid (k, max(1, D / 64)), 256 threads: kmeans_mean_host on the device.
__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const float* __restrict__ raw, uint32_t D, const uint32_t* __restrict__ order,
                                                            const uint32_t* __restrict__ starts, float* __restrict__ cent) {
    __shared__ float s_part[kKmeansWaves][64];
    const uint32_t c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t lo = starts[c], m = starts[c + 1] - lo;
    if (m == 0) return;                                               // (workgroup-uniform) an empty cluster keeps its centroid
    const uint32_t d = blockIdx.y * 64 + lane;
    const bool on = d < D;
    const float* col = raw + (on ? d : 0);
    const uint32_t* ids = order + lo;
    float p = 0.0f;
    uint32_t j = wave;
    for (; j + 3 * kKmeansWaves < m; j += 4 * kKmeansWaves) {         // four loads in flight, the additions in member order
        const uint32_t i0 = ids[j], i1 = ids[j + kKmeansWaves], i2 = ids[j + 2 * kKmeansWaves], i3 = ids[j + 3 * kKmeansWaves];
        const float x0 = col[(size_t)i0 * D], x1 = col[(size_t)i1 * D], x2 = col[(size_t)i2 * D], x3 = col[(size_t)i3 * D];
        p = p + x0;
        p = p + x1;
        p = p + x2;
        p = p + x3;
    }
    for (; j < m; j += kKmeansWaves) p = p + col[(size_t)ids[j] * D];
    s_part[wave][lane] = p;
    __syncthreads();
    if (wave == 0 && on)
        cent[(size_t)c * D + d] = (((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane]) / (float)m;
}

// ---- 4. the outputs -------------------------------------------------------------------------------------------------------------
// Eight lanes per row: dist[i] = exact_l2 (query = the assigned centroid, id = i): the chains of group_dot8, the centroid's
// query norm, norm_sq[i]; counts[c] += 1 (integer).  A removed row: -1 / FLT_MAX.
__global__ __launch_bounds__(256) void kmeans_final_kernel(const float* __restrict__ raw, const float* __restrict__ norm_sq,
                                                           const float* __restrict__ cent, const float* __restrict__ cnorm, uint32_t n,
                                                           uint32_t D, const int32_t* __restrict__ assign, int32_t* __restrict__ out_assign,
                                                           float* __restrict__ out_dist, unsigned long long* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * 32 + (threadIdx.x >> 3);
    const uint32_t j = threadIdx.x & 7;
    const uint64_t ii = min(i, (uint64_t)n - 1);                       // (whole groups stay converged for the exchange)
    const int32_t c = assign[ii];
    const float* q = cent + (size_t)(c < 0 ? 0 : c) * D;
    const float* v = raw + (size_t)ii * D;
    float s = 0.0f;
    for (uint32_t e = j; e < D; e += 8) s = __fmaf_rn(q[e], v[e], s);
    const float dot = group_reduce8(s);
    if (j != 0 || i >= n) return;
    out_assign[i] = c;
    out_dist[i] = c < 0 ? FLT_MAX : exact_from_dot(cnorm[c], norm_sq[i], dot);
    if (c >= 0) atomicAdd(counts + c, 1ull);
}

// out[k][dim] = the first dim coordinates of the centroids.
__global__ __launch_bounds__(256) void kmeans_export_kernel(const float* __restrict__ cent, uint32_t k, uint32_t dim, uint32_t D,
                                                            float* __restrict__ out) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (uint64_t)k * dim) return;
    out[e] = cent[(e / dim) * D + e % dim];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
struct KmeansBuffers {
    float* cent;                          // [k + kExactQT][D]
    float* cnorm;                         // [k + kExactQT]
    uint32_t* cn_max;
    int32_t* assign[2];                   // [n] each: this pass' and the one before
    uint32_t* unc_ids;                    // [n]
    uint32_t* unc_counts;                 // [iters + 1]
    uint32_t* hist;                       // [segments][k]
    uint32_t* sizes;                      // [k]
    uint32_t* starts;                     // [k + 1]
    uint32_t* order;                      // [n]
};

// One assignment pass on `st`: the centroid norms, their maximum, the matrix kernel (between `ev0` and `ev1` if given),
// the vector kernel for what it left.
inline void kmeans_assign(const float* raw, const float* norm_sq, const uint32_t* removed, uint32_t n, uint32_t k, uint32_t D,
                          const KmeansBuffers& b, int32_t* assign, uint32_t pass, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
    hipLaunchKernelGGL(kmeans_cnorm_kernel, dim3((k + kExactQT + 31) / 32), dim3(256), 0, st, (const float*)b.cent, k, D, b.cnorm);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(exact_mfma_bnmax_kernel, dim3(1), dim3(1024), 0, st, (const float*)b.cnorm, (uint64_t)k, b.cn_max);
    HIP_CHECK(hipGetLastError());
    KmeansAssignArgs a{};
    a.t.raw = b.cent;
    a.t.norm_sq = b.cnorm;
    a.t.qpad = raw;
    a.t.qnorm = norm_sq;
    a.t.D = D;
    a.cn_max = b.cn_max;
    a.removed = removed;
    a.n = n;
    a.k = k;
    a.assign = assign;
    a.unc_ids = b.unc_ids;
    a.unc_count = b.unc_counts + pass;
    if (ev0) HIP_CHECK(hipEventRecord(ev0, st));
    hipLaunchKernelGGL(kmeans_assign_mfma_kernel, dim3((n + kMxTile - 1) / kMxTile), dim3(256), 0, st, a);
    HIP_CHECK(hipGetLastError());
    if (ev1) HIP_CHECK(hipEventRecord(ev1, st));
    KmeansResolveArgs r{raw, norm_sq, b.cent, b.cnorm, b.unc_ids, b.unc_counts + pass, D, k, assign};
    CPH_LAUNCH_SCAN(kmeans_resolve_kernel, D, dim3((n + 63) / 64), 0, st, r);
}

// The update behind pass `it`: the centroids become the means of `assign`; moved[it] counts against `prev`.
inline void kmeans_update(const float* raw, uint32_t n, uint32_t k, uint32_t D, const KmeansBuffers& b, const int32_t* assign,
                          const int32_t* prev, unsigned long long* moved, hipStream_t st) {
    const KmeansSegments sg = kmeans_segments(n);
    hipLaunchKernelGGL(kmeans_hist_kernel, dim3(sg.count), dim3(256), (size_t)k * 4, st, assign, prev, n, sg.rows, k, b.hist, moved);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kmeans_offsets_kernel, dim3((k + 255) / 256), dim3(256), 0, st, b.hist, sg.count, k, b.sizes);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kmeans_starts_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)b.sizes, k, b.starts);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kmeans_scatter_kernel, dim3(sg.count), dim3(64), (size_t)k * 4, st, assign, n, sg.rows, k, (const uint32_t*)b.hist,
                       (const uint32_t*)b.starts, b.order);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(kmeans_reduce_kernel, dim3(k, D < 64 ? 1u : D / 64), dim3(256), 0, st, raw, D, (const uint32_t*)b.order,
                       (const uint32_t*)b.starts, b.cent);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
