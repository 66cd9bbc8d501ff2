// device_encode.h — per-query feeders on the GPU: query encoder + upper-layer greedy descent.
//
// GPU counterparts of
//   RandomHadamardRotation::apply_copy    encoder/rotation.hpp:34-51, transform/fht.hpp:23-57
//   encode_query_raw / build_lut          encoder/rabitq_encoder.hpp:73-79,98-136,197-209
//   Index::search prologue + greedy_search_layer  api/hnsw_index.hpp:174-202,468-474,617-638
// One wave per query.  Every butterfly output is a single add/sub, the scale is a single
// multiply and the quantiser is one explicit fma, so any schedule is bit-exact as long as the
// stage order and the reference's sign convention are kept; min/max carry the index of their
// first occurrence, reproducing the reference's sequential strict-compare scans.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "cph_core.h"
#include "device_fastscan.h"

namespace cph {

struct UpperLayerDev {       // CSR of one upper layer, nodes sorted ascending (find_edge)
    const uint32_t* nodes;   // [n_nodes]
    const uint32_t* offsets; // [n_nodes + 1]
    const uint32_t* nbrs;
    const uint32_t* row_of;  // [n] vertex -> first edge | degree << 26 (kInvalidNode if absent), or null:
                             // binary search over `nodes` + `offsets`
    const uint32_t* nbr_info;// [n_edges] row_of[nbrs[e]]: a hop's edges bring the next hop's (first edge, degree)
                             // with them; present exactly where row_of is
    uint32_t n_nodes;
};

constexpr int kMaxUpperLayers = 24;

struct EncodeArgs {
    const float* queries_raw;  // [nq][dim]
    uint32_t nq, dim, D, PW;
    const float* signs;        // [3][D]
    float norm_factor, inv_sqrt_d;
    // index (upper-layer descent)
    const float* raw;          // [n][D]
    uint64_t n;
    uint32_t entry;
    int32_t max_level;         // number of usable upper layers (0 = none)
    UpperLayerDev layers[kMaxUpperLayers];
    // outputs
    float* queries_padded;     // [nq][D]
    uint4* qmasks;             // [nq][PW]
    QueryHeader* qhdr;         // [nq]
    float* entry_dist;         // [nq] squared distance to the layer-0 entry (scheduling key), or null
};

__device__ __forceinline__ void wave_fht(float* x, uint32_t D, int lane) {
    for (uint32_t h = 1; h < D; h <<= 1) {
        for (uint32_t b = lane; b < D / 2; b += 64) {
            const uint32_t i = (b / h) * 2 * h + (b % h);
            const float lo = x[i], hi = x[i + h];
            x[i] = lo + hi;
            x[i + h] = (h < 8) ? (hi - lo) : (lo - hi);
        }
        __syncthreads();
    }
}

// 8 N elements of sum (q - v)^2 on a lane PAIR: half h = lane & 1 runs chains 4h .. 4h+3 of the eight group_l2sq8
// chains (chain c = elements c, c + 8, ... ascending, the order of chain_l2<16>).  `q` and `v` already point at
// element 4h of the part: one 64-bit base per lane, N dwordx4 loads at immediate offsets, all in flight together.
// The query comes from LDS through a ring of QR float4 (left to itself the compiler reads all N up front: 4 N
// more registers next to the 4 N of the loads).
template <int N, int QR>
__device__ __forceinline__ void pair_l2_part(const float* q_lds, const float* __restrict__ v, float (&c)[4]) {
    float4 r[N], q[QR];
#pragma unroll
    for (int j = 0; j < N; ++j) r[j] = *reinterpret_cast<const float4*>(v + 8 * j);
#pragma unroll
    for (int j = 0; j < QR; ++j) q[j] = *reinterpret_cast<const float4*>(q_lds + 8 * j);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const float4 qq = q[j % QR];
        const float d0 = qq.x - r[j].x, d1 = qq.y - r[j].y, d2 = qq.z - r[j].z, d3 = qq.w - r[j].w;
        c[0] = __fmaf_rn(d0, d0, c[0]);
        c[1] = __fmaf_rn(d1, d1, c[1]);
        c[2] = __fmaf_rn(d2, d2, c[2]);
        c[3] = __fmaf_rn(d3, d3, c[3]);
        if (j + QR < N) q[j % QR] = *reinterpret_cast<const float4*>(q_lds + 8 * (j + QR));
        __builtin_amdgcn_sched_barrier(0);
    }
}
// The pair's reduction: s_i = c_i + c_{i+4} (the partner holds the other four chains), then (s0 + s1) + (s2 + s3) --
// the tree ((c0+c4)+(c1+c5))+((c2+c6)+(c3+c7)) of group_reduce8; fp add is commutative, so both lanes of the pair
// end with the bits group_l2sq8 gives.
__device__ __forceinline__ float pair_reduce(const float (&c)[4]) {
    const float s0 = c[0] + dpp_mov<0xB1>(c[0]), s1 = c[1] + dpp_mov<0xB1>(c[1]);   // quad_perm [1,0,3,2]: lane ^ 1
    const float s2 = c[2] + dpp_mov<0xB1>(c[2]), s3 = c[3] + dpp_mov<0xB1>(c[3]);
    return (s0 + s1) + (s2 + s3);
}

// (distance, position) minimum of the descent: smallest distance, first stored position on a tie.
__device__ __forceinline__ void min_step(float& cand, uint32_t& pos, float od, uint32_t op) {
    if (od < cand || (od == cand && op < pos)) { cand = od; pos = op; }
}
template <int CTRL>
__device__ __forceinline__ void min_step_dpp(float& cand, uint32_t& pos) {
    min_step(cand, pos, dpp_mov<CTRL>(cand), (uint32_t)__builtin_amdgcn_update_dpp(0, (int)pos, CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float uniform_f32(float v) {   // a value every lane holds, moved to a scalar register
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// the minimum over the four rows of 16 lanes, each row already holding one value: scalar from here on
__device__ __forceinline__ void min_rows(float& cand, uint32_t& pos) {
    float bc = uniform_f32(cand);
    uint32_t bp = uniform_u32(pos);
#pragma unroll
    for (int r = 16; r < 64; r += 16)
        min_step(bc, bp, __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cand), r)),
                 (uint32_t)__builtin_amdgcn_readlane((int)pos, r));
    cand = bc;
    pos = bp;
}
// The lane index as a value the optimiser cannot see through (device_search.h's opaque_lane, which comes after this
// header): what a path derives from it (LDS and row offsets, group indices) is computed inside that path, not hoisted
// out of the enclosing loops and kept live across the load registers of the paired pass.
__device__ __forceinline__ int fresh_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// One layer's descriptor, read from the kernel-argument segment with scalar loads at a run-time index (indexing the
// by-value array instead makes the compiler keep all 24 descriptors in SGPRs and spill them).  EncodeArgs is
// encode_kernel's only argument, so it starts the segment.
__device__ __forceinline__ UpperLayerDev load_layer(int idx) {
    static_assert(sizeof(UpperLayerDev) == 48 && offsetof(UpperLayerDev, n_nodes) == 40, "six qwords per descriptor");
    using kbyte = const __attribute__((address_space(4))) unsigned char;
    using kqword = const __attribute__((address_space(4))) uint64_t;
    kbyte* seg = (kbyte*)__builtin_amdgcn_kernarg_segment_ptr();
    kqword* w = reinterpret_cast<kqword*>(seg + offsetof(EncodeArgs, layers) + (size_t)idx * sizeof(UpperLayerDev));
    UpperLayerDev L;
    L.nodes = reinterpret_cast<const uint32_t*>(w[0]);
    L.offsets = reinterpret_cast<const uint32_t*>(w[1]);
    L.nbrs = reinterpret_cast<const uint32_t*>(w[2]);
    L.row_of = reinterpret_cast<const uint32_t*>(w[3]);
    L.nbr_info = reinterpret_cast<const uint32_t*>(w[4]);
    L.n_nodes = (uint32_t)w[5];
    return L;
}

// LDS: raw padded query [D] | work buffer [D]
__host__ __device__ inline size_t encode_lds_bytes(uint32_t D) { return (size_t)D * 8; }

__global__ __launch_bounds__(64) void encode_kernel(EncodeArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    float* qv = reinterpret_cast<float*>(smem);
    float* x = qv + a.D;
    const uint32_t D = a.D;
    for (uint32_t qi = blockIdx.x; qi < a.nq; qi += gridDim.x) {
        const int lane = fresh_lane(threadIdx.x);   // per query: nothing lane-derived stays live from one to the next
        for (uint32_t d = lane; d < D; d += 64) {
            float v = d < a.dim ? a.queries_raw[(size_t)qi * a.dim + d] : 0.0f;
            qv[d] = v;
            x[d] = v;
            a.queries_padded[(size_t)qi * D + d] = v;
        }
        __syncthreads();
        // ---- rotation: 3 x (diag, FHT), then the deferred D^-1.5 normalisation ---------
        for (int l = 0; l < 3; ++l) {
            for (uint32_t d = lane; d < D; d += 64) x[d] = x[d] * a.signs[l * D + d];
            __syncthreads();
            wave_fht(x, D, lane);
        }
        for (uint32_t d = lane; d < D; d += 64) x[d] = x[d] * a.norm_factor;
        __syncthreads();
        // ---- min / max with first-occurrence semantics (rabitq_encoder.hpp:99-103) -------
        float vmin = x[lane < (int)D ? lane : 0], vmx = vmin;
        uint32_t imin = lane < (int)D ? lane : 0, imax = imin;
        for (uint32_t d = lane + 64; d < D; d += 64) {
            const float v = x[d];
            if (v < vmin) { vmin = v; imin = d; }
            if (v > vmx) { vmx = v; imax = d; }
        }
        for (int o = 1; o < 64; o <<= 1) {
            const float ov = __shfl_xor(vmin, o);
            const uint32_t oi = __shfl_xor(imin, o);
            if (ov < vmin || (ov == vmin && oi < imin)) { vmin = ov; imin = oi; }
            const float ow = __shfl_xor(vmx, o);
            const uint32_t oj = __shfl_xor(imax, o);
            if (ow > vmx || (ow == vmx && oj < imax)) { vmx = ow; imax = oj; }
        }
        const float vl = x[imin];     // exact bits of the first minimum (keeps the sign of zero)
        const float vh = x[imax];
        float delta = (vh - vl) / 15.0f;
        if (delta < kEpsTiny) delta = kEpsTiny;
        const float inv_delta = 1.0f / delta;
        // ---- 4-bit scalars, their sum, and the bit-sliced masks ---------------------------
        uint32_t usum = 0;
        for (uint32_t base = 0; base < D; base += 64) {
            const uint32_t d = base + lane;
            int u = 0;
            if (d < D) {
                u = (int)__fmaf_rn(x[d] - vl, inv_delta, 0.5f);
                u = u < 0 ? 0 : (u > 15 ? 15 : u);
            }
            usum += (uint32_t)u;
            const unsigned long long b0 = __ballot(u & 1), b1 = __ballot(u & 2), b2 = __ballot(u & 4),
                                     b3 = __ballot(u & 8);
            if (lane == 0) {
                const uint32_t w = base / 32;
                a.qmasks[(size_t)qi * a.PW + w] =
                    make_uint4((uint32_t)b0, (uint32_t)b1, (uint32_t)b2, (uint32_t)b3);
                if (w + 1 < a.PW)
                    a.qmasks[(size_t)qi * a.PW + w + 1] = make_uint4(
                        (uint32_t)(b0 >> 32), (uint32_t)(b1 >> 32), (uint32_t)(b2 >> 32), (uint32_t)(b3 >> 32));
            }
        }
        for (int o = 1; o < 64; o <<= 1) usum += __shfl_xor(usum, o);
        const float sum_qu = (float)usum;  // integer-valued partial sums: exact in any order
        const float df = (float)D;
        QueryHeader hd;
        // (every lane computed the same three: scalar registers carry them across the descent)
        hd.A = uniform_f32((2.0f * delta) * a.inv_sqrt_d);
        hd.B = uniform_f32((2.0f * vl) * a.inv_sqrt_d);
        hd.C = uniform_f32(-__fmaf_rn(df, vl, delta * sum_qu) * a.inv_sqrt_d);

        // ---- upper-layer greedy descent (api/hnsw_index.hpp:196-202,617-638) ---------------
        uint32_t ep = a.entry;
        float ep_dist = 0.0f;
        if (a.max_level > 0 && ep < a.n) {
            const bool paired = (D % 128u) == 0;
            for (int level = a.max_level; level >= 1; --level) {
                const UpperLayerDev Ly = load_layer(level - 1);
                // distance to the layer's entry: the previous layer's winner, whose distance is already
                // known (same query, same vector, same arithmetic => same float as recomputing it).
                // (Requesting the entry's vector ahead of the three rotation passes was tried: its 16 registers stay
                // live across the rotation's unrolled loops, 101 VGPRs and 4 waves per SIMD.  It is loaded here.)
                float best = (level == a.max_level)
                                 ? uniform_f32(group_l2sq8(qv, a.raw + (size_t)ep * D, D, fresh_lane(lane) & 7))
                                 : ep_dist;
                uint32_t best_id = ep;
                if (Ly.row_of) {
                    // dense vertex -> (first edge, degree) map: read once, for the vertex the layer is entered at.
                    // Every later hop gets its own from nbr_info, in the round trip that fetches the edges, so a
                    // hop is two dependent round trips: edges, then vectors.
                    uint32_t info = Ly.row_of[best_id];
                    while (info != kInvalidNode) {
                        const uint32_t beg = info & 0x03FFFFFFu, cnt = info >> 26;
                        float cand = 3.402823466e+38f;
                        uint32_t cand_pos = 0xFFFFFFFFu;
                        uint32_t mine = best_id, mine_info = kInvalidNode, src;
                        if (paired && cnt <= 32) {
                            // lanes 2p, 2p+1 own neighbour p and four of its eight chains each: the whole list in
                            // one pass.  Per 64 elements a lane has 8 dwordx4 loads (32 registers) in flight: two
                            // round trips per 128-element chunk, 79 VGPRs.  All 16 loads of a chunk together need
                            // 64 registers next to the ~34 that are live across the pass: 98 and up, 4-5 waves per
                            // SIMD, where an encoder wave no longer fits the 80 registers a search wave frees.
                            // (Eight lanes and 16 dword loads per neighbour, all passes together: 150 VGPRs.)
                            const int pl = fresh_lane(lane);
                            const uint32_t p = (uint32_t)pl >> 1;
                            const int half = pl & 1;
                            const bool have = p < cnt;
                            float c[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                            if (have) {
                                mine = Ly.nbrs[beg + p];
                                mine_info = Ly.nbr_info[beg + p];
                                const float* v = a.raw + (size_t)mine * D + 4 * half;
                                for (uint32_t base = 0; base < D; base += 64) pair_l2_part<8, 3>(qv + base + 4 * half, v + base, c);
                            }
                            const float d = pair_reduce(c);
                            if (have && d < cand) { cand = d; cand_pos = p; }
                            // both lanes of a pair agree; quads, rows of 16, then the four rows
                            min_step_dpp<0x4E>(cand, cand_pos);    // quad_perm [2,3,0,1]
                            min_step_dpp<0x124>(cand, cand_pos);   // row_ror:4
                            min_step_dpp<0x128>(cand, cand_pos);   // row_ror:8
                            min_rows(cand, cand_pos);
                            src = cand_pos * 2;
                        } else {
                            // more than 32 neighbours (row_of allows 62) or D not a multiple of 128: eight lanes per
                            // neighbour, eight neighbours per pass
                            const int sl = fresh_lane(lane);
                            if ((uint32_t)sl < cnt) {
                                mine = Ly.nbrs[beg + sl];
                                mine_info = Ly.nbr_info[beg + sl];
                            }
                            for (uint32_t base = 0; base < cnt; base += 8) {
                                const uint32_t pos = base + (sl >> 3);
                                const bool have = pos < cnt;
                                const uint32_t nb = (uint32_t)__shfl((int)mine, (int)(have ? pos : 0));
                                const float d = group_l2sq8(qv, a.raw + (size_t)(have ? nb : best_id) * D, D, sl & 7);
                                if (have && (d < cand || (d == cand && pos < cand_pos))) { cand = d; cand_pos = pos; }
                            }
                            for (int o = 8; o < 64; o <<= 1) {
                                const float od = __shfl_xor(cand, o);
                                const uint32_t op = __shfl_xor(cand_pos, o);
                                if (od < cand || (od == cand && op < cand_pos)) { cand = od; cand_pos = op; }
                            }
                            cand = uniform_f32(cand);
                            src = cand_pos = uniform_u32(cand_pos);
                        }
                        // every lane holds the same (cand, cand_pos) now; the winner's id and its (first edge,
                        // degree) come from the lane that loaded them
                        if (cand_pos == 0xFFFFFFFFu || !(cand < best)) break;
                        best = cand;
                        best_id = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)src);
                        info = (uint32_t)__builtin_amdgcn_readlane((int)mine_info, (int)src);
                    }
                } else {
                    bool improved = true;
                    while (improved) {
                        improved = false;
                        float cand = 3.402823466e+38f;
                        uint32_t cand_id = kInvalidNode;
                        uint32_t cand_pos = 0xFFFFFFFFu;
                        // find_edge: lower_bound over the sorted node list (uniform across lanes)
                        uint32_t lo = 0, hi = Ly.n_nodes;
                        while (lo < hi) {
                            const uint32_t mid = (lo + hi) >> 1;
                            if (Ly.nodes[mid] < best_id) lo = mid + 1; else hi = mid;
                        }
                        if (lo >= Ly.n_nodes || Ly.nodes[lo] != best_id) break;
                        const uint32_t beg = Ly.offsets[lo], end = Ly.offsets[lo + 1];
                        // neighbours in stored order; strict improvement => the first minimum wins
                        const int sl = fresh_lane(lane);
                        for (uint32_t base = beg; base < end; base += 8) {
                            const uint32_t pos = base + (sl >> 3);
                            const bool have = pos < end;
                            const uint32_t nb = have ? Ly.nbrs[pos] : best_id;
                            const float d = group_l2sq8(qv, a.raw + (size_t)nb * D, D, sl & 7);
                            if (have && (d < cand || (d == cand && pos < cand_pos))) {
                                cand = d; cand_id = nb; cand_pos = pos;
                            }
                        }
                        for (int o = 8; o < 64; o <<= 1) {
                            const float od = __shfl_xor(cand, o);
                            const uint32_t oi = __shfl_xor(cand_id, o);
                            const uint32_t op = __shfl_xor(cand_pos, o);
                            if (od < cand || (od == cand && op < cand_pos)) { cand = od; cand_id = oi; cand_pos = op; }
                        }
                        cand = uniform_f32(cand);          // (the same in every lane)
                        cand_id = uniform_u32(cand_id);
                        if (cand_id != kInvalidNode && cand < best) {
                            best = cand;
                            best_id = cand_id;
                            improved = true;
                        }
                    }
                }
                ep = best_id;
                ep_dist = best;
            }
        }
        hd.entry = ep;
        if (lane == 0) {
            a.qhdr[qi] = hd;
            if (a.entry_dist) a.entry_dist[qi] = ep_dist;
        }
        __syncthreads();
    }
}

// ---- launch order of a batch ------------------------------------------------------------
// Queries whose layer-0 entry is close tend to expand the most vertices (dense neighbourhoods:
// rank correlation -0.8 on the benchmark index), and a batch only a few times larger than the
// number of resident query slots ends when its last-started long query ends.  The work queue
// therefore hands queries out closest-entry-first: a counting sort on the top 14 bits of the
// (non-negative) float key, one workgroup, LDS histogram.  Any order gives the same results.
constexpr uint32_t kOrderBuckets = 16384;
__global__ __launch_bounds__(1024) void order_kernel(const float* __restrict__ key, uint32_t nq,
                                                     uint32_t* __restrict__ order) {
    __shared__ uint32_t hist[kOrderBuckets];
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x;
    for (uint32_t b = tid; b < kOrderBuckets; b += 1024) hist[b] = 0;
    __syncthreads();
    for (uint32_t i = tid; i < nq; i += 1024) {
        const uint32_t kb = __float_as_uint(key[i]);
        const uint32_t b = (kb & 0x80000000u) ? 0u : (kb >> 17);   // sign bit set (or NaN payloads) first
        atomicAdd(&hist[b < kOrderBuckets ? b : kOrderBuckets - 1], 1u);
    }
    __syncthreads();
    // exclusive prefix sum over the buckets: 16 consecutive buckets per thread
    uint32_t local[16], run = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) { local[j] = run; run += hist[tid * 16 + j]; }
    uint32_t inc = run;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(inc, o);
        if ((tid & 63) >= (uint32_t)o) inc += v;
    }
    if ((tid & 63) == 63) wsum[tid >> 6] = inc;
    __syncthreads();
    uint32_t base = inc - run;
    for (uint32_t w = 0; w < (tid >> 6); ++w) base += wsum[w];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) hist[tid * 16 + j] = base + local[j];
    __syncthreads();
    for (uint32_t i = tid; i < nq; i += 1024) {
        const uint32_t kb = __float_as_uint(key[i]);
        const uint32_t b = (kb & 0x80000000u) ? 0u : (kb >> 17);
        const uint32_t pos = atomicAdd(&hist[b < kOrderBuckets ? b : kOrderBuckets - 1], 1u);
        order[pos] = i;
    }
}

}  // namespace cph
