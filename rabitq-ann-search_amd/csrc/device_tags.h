// device_tags.h — tag filters (cph_filters_from_tags): m allowed-id bitmaps from one of the handle's tag columns in one
// pass.  A tag column is a CSR in internal-id order (lims[n + 1], tags ascending and distinct inside a row); test j is a
// set V_j of at most 64 values and a mode, and with c = |tags(row) & V_j| it allows the row when c > 0 (any), c == |V_j|
// (all) or c == 0 (none): one count and one compare for all three.
//
// One wave owns a tile of kTagTile = 256 consecutive rows = 8 bitmap words per filter; a block is four waves, four tiles,
// so the 32 words a block leaves per filter are one 128 B line.  The tile's tags tags[lims[r0] .. lims[r1]) are one
// contiguous span.  The wave stages it into its own LDS region once -- 16 B loads over the aligned body, 4 B loads at
// the two ends (the span starts wherever the previous row ended); it is placed at its offset modulo 4 so that the LDS
// stores are 16 B aligned too -- and then walks the filters of its chunk (blockIdx.y: kTagFilterChunk filters, so the
// column is read from HBM once per chunk, not once per filter) against LDS.  A span longer than the region (a tile of
// long rows: 256 rows of 1,024 tags are 1 MiB) is not staged: that wave reads its tags from global memory in the same
// loop (`walk` is instantiated for both address spaces; the choice is wave-uniform).
//
// Lane l owns row 64 g + l of group g = 0..3 of the tile.  The values of a test are wave-uniform: they are read through a
// const __restrict__ pointer at uniform indices (scalar loads), kTagTestPad = 4 at a time.  The host pads every test to a
// multiple of 4 with copies of its last value and the kernel ORs the four compares -- both sides are distinct, so a tag
// matches at most one value and the OR over a group is the group's count; the copies change nothing.  A row therefore
// costs len(row) x ceil(|V| / 4) LDS reads and len(row) x |V| (rounded up to 4) compares per filter.  __ballot of a group's
// 64 verdicts is two finished bitmap words; they are dropped into lanes 2 g and 2 g + 1 with two selects (noise next to the
// tag walk, unlike in the label kernel, where the walk is one range test), and after the four groups lanes 0..7 leave
// one 32 B store.  Rows at or above n have no verdict, so the bits of the last word behind n are clear, and every word
// below (n + 31) / 32 is written, zeros included: nothing depends on what the slab held.  The count of a filter over the
// tile is the popcount of the ballots -- a wave sum that is scalar already -- added to counts[j] with one atomicAdd per
// wave (counts zeroed by the launcher).  The one barrier sits between the staging and the walk, and no wave returns in
// front of it.  The host statement is host_index.h: tag_filters_host.
#pragma once
#include <hip/hip_runtime.h>

#include "device_buf.h"

namespace cph {

constexpr uint32_t kTagGroups = 4;                        // 64-row groups per wave
constexpr uint32_t kTagTile = 64 * kTagGroups;            // rows per wave: 2 * kTagGroups bitmap words per filter
constexpr uint32_t kTagFilterChunk = 64;                  // filters per blockIdx.y: the column is read once per chunk
constexpr uint32_t kTagBlock = 256;                       // threads per block: 4 waves, 4 tiles
constexpr uint32_t kTagLdsTags = 3072;                    // staged tags per wave, at most (12 KiB; a block holds 48 KiB)
constexpr uint32_t kTagMaxFilters = 65535u * kTagFilterChunk;   // filters per call: one launch, grid.y <= 65,535
constexpr uint32_t kTagValuePad = 4;                      // (= host_index.h: kTagTestPad) values per uniform load group

// One wave's filters against its rows.  src: the tags, rows at src[beg[g] .. end[g]) (LDS or global); ok: bit g = the
// lane's row of group g is below n.
template <class Src>
__device__ __forceinline__ void tag_walk(Src src, const uint32_t (&beg)[kTagGroups], const uint32_t (&end)[kTagGroups], uint32_t ok,
                                         const uint32_t* __restrict__ offs, const uint32_t* __restrict__ info,
                                         const int32_t* __restrict__ vals, uint32_t j0, uint32_t j1, uint32_t lane, uint64_t w,
                                         uint64_t nw, uint32_t* __restrict__ words, uint64_t stride,
                                         unsigned long long* __restrict__ counts) {
    for (uint32_t j = j0; j < j1; ++j) {
        const uint32_t vb = offs[j], ve = offs[j + 1], inf = info[j];
        const uint32_t mode = inf & 0xFFu, nv = inf >> 8;
        uint32_t mine = 0, total = 0;
#pragma unroll
        for (uint32_t g = 0; g < kTagGroups; ++g) {
            uint32_t c = 0;
            for (uint32_t v = vb; v < ve; v += kTagValuePad) {
                const int32_t v0 = vals[v], v1 = vals[v + 1], v2 = vals[v + 2], v3 = vals[v + 3];
                // (left to itself the compiler interleaves this loop by two: every compare result is an SGPR pair, and the
                // kernel then spills 24 SGPRs; as written it spills none)
#pragma clang loop vectorize(disable) interleave(disable)
                for (uint32_t t = beg[g]; t < end[g]; ++t) {
                    const int32_t x = src[t];
                    c += ((x == v0) | (x == v1) | (x == v2) | (x == v3)) ? 1u : 0u;
                }
            }
            const bool pass = ((ok >> g) & 1u) && (mode == 0 ? c > 0 : mode == 1 ? c == nv : c == 0);
            const unsigned long long b = __ballot(pass);
            mine = lane == 2 * g ? (uint32_t)b : lane == 2 * g + 1 ? (uint32_t)(b >> 32) : mine;
            total += (uint32_t)__popcll(b);
        }
        if (lane < 2 * kTagGroups && w < nw) words[(uint64_t)j * stride + w] = mine;
        if (lane == 0 && total) atomicAdd(&counts[j], (unsigned long long)total);
    }
}

// lims: [n + 1]; tags: [lims[n]], 16 B aligned (null when lims[n] == 0: then no span has an element and nothing is read);
// table: the tests (host_index.h: tag_tests_pack_host), values from table + vals_at; words: m bitmaps, filter j at words +
// j * stride (stride >= (n + 31) / 32 words); counts: [m].
__global__ __launch_bounds__(kTagBlock) void tag_filters_kernel(const uint32_t* __restrict__ lims, const int32_t* __restrict__ tags,
                                                                uint64_t n, const uint32_t* __restrict__ table, uint32_t vals_at,
                                                                uint32_t m, uint32_t* __restrict__ words, uint64_t stride,
                                                                unsigned long long* __restrict__ counts) {
    __shared__ int4 staged[kTagBlock / 64][kTagLdsTags / 4 + 1];     // (+ 1: the span sits at its offset modulo 4)
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t tile = (uint64_t)blockIdx.x * (kTagBlock / 64) + wave;
    const uint64_t r0 = tile * kTagTile < n ? tile * kTagTile : n, r1 = r0 + kTagTile < n ? r0 + kTagTile : n;
    const uint64_t s0 = lims[r0], s1 = lims[r1];           // the tile's span (a wave behind the last tile: r0 = r1 = n, empty);
    const uint64_t base = s0 & ~(uint64_t)3;               // 64-bit: s0 + lane must not wrap.  LDS element e - base holds tags[e]
    const bool fits = s1 - base <= kTagLdsTags + 4;
    int32_t* lds = reinterpret_cast<int32_t*>(staged[wave]);
    if (fits && s1 > s0) {
        const uint64_t up = (s0 + 3) & ~(uint64_t)3, down = s1 & ~(uint64_t)3;
        const uint64_t a0 = up < s1 ? up : s1;             // [s0, a0): the unaligned head, fewer than 4 tags
        const uint64_t a1 = down > a0 ? down : a0;         // [a0, a1): whole 16 B pieces; [a1, s1): the tail, fewer than 4
        if (s0 + lane < a0) lds[s0 + lane - base] = tags[s0 + lane];
        const int4* body = reinterpret_cast<const int4*>(tags + a0);
        int4* dst = reinterpret_cast<int4*>(lds + (a0 - base));
        for (uint32_t i = lane; i < (uint32_t)(a1 - a0) / 4; i += 64) dst[i] = body[i];
        if (a1 + lane < s1) lds[a1 + lane - base] = tags[a1 + lane];
    }
    __syncthreads();                                       // (every wave arrives: nothing above returns)
    if (r0 == r1) return;
    uint32_t beg[kTagGroups], end[kTagGroups], ok = 0;
    const uint32_t off = fits ? (uint32_t)base : 0u;
#pragma unroll
    for (uint32_t g = 0; g < kTagGroups; ++g) {
        const uint64_t r = r0 + 64 * g + lane;
        const bool in = r < r1;
        beg[g] = in ? lims[r] - off : 0u;
        end[g] = in ? lims[r + 1] - off : 0u;
        ok |= (in ? 1u : 0u) << g;
    }
    const uint32_t j0 = blockIdx.y * kTagFilterChunk;
    const uint32_t j1 = j0 + kTagFilterChunk < m ? j0 + kTagFilterChunk : m;
    const uint32_t* offs = table;
    const uint32_t* info = table + m + 1;
    const int32_t* vals = reinterpret_cast<const int32_t*>(table + vals_at);
    const uint64_t nw = (n + 31) / 32, w = tile * (2 * kTagGroups) + lane;
    if (fits) tag_walk(lds, beg, end, ok, offs, info, vals, j0, j1, lane, w, nw, words, stride, counts);
    else tag_walk(tags, beg, end, ok, offs, info, vals, j0, j1, lane, w, nw, words, stride, counts);
}

// Enqueues the pass on `st` (counts zeroed first); every pointer lives on the current device.  1 <= m <= kTagMaxFilters.
inline void tag_filters(const uint32_t* d_lims, const int32_t* d_tags, uint64_t n, const uint32_t* d_table, uint32_t vals_at, uint32_t m,
                        uint32_t* d_words, uint64_t stride, unsigned long long* d_counts, hipStream_t st) {
    HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)m * 8, st));
    if (n == 0) return;
    const uint64_t tiles = (n + kTagTile - 1) / kTagTile, per_block = kTagBlock / 64;
    const uint32_t gx = (uint32_t)((tiles + per_block - 1) / per_block);
    const uint32_t gy = (m + kTagFilterChunk - 1) / kTagFilterChunk;
    hipLaunchKernelGGL(tag_filters_kernel, dim3(gx, gy), dim3(kTagBlock), 0, st, d_lims, d_tags, n, d_table, vals_at, m, d_words, stride,
                       d_counts);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
