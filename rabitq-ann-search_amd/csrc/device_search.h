// device_search.h — persistent layer-0 beam search, one wavefront per query.
//
// GPU counterpart of rabitq_search::search (search/rabitq_search.hpp:60-277) and its
// helpers BoundedMaxHeap (:17-49) / BeamEntry (:53-58).  Results are bit-identical to the
// reference: the data-parallel parts (FastScan block, estimated-set probes, speculative
// exact L2 of every lane whose estimate beats the threshold at loop entry) run on all 64
// lanes; the beam's pop_heap is executed by the whole wave (beam_pop_wave); the
// order-dependent decisions of the 32-neighbour loop (:218-273) are taken by all lanes at
// once when no neighbour is reranked, and replayed by lane 0 in neighbour order otherwise --
// always with the reference's heap algorithms (std::push_heap / pop_heap / sort_heap element
// movement, so ties break identically).
//
// Observations that shape the kernel:
//  * every node enters the beam at most once (each push is guarded by the estimated-set
//    test), so the reference's second "visited" table is never observable — only the
//    estimated set is kept (a per-slot bitmap, cleared by un-marking the logged ids);
//  * in a non-warm-up expansion the result-heap threshold only decreases, so
//    {est < worst at loop entry} is a superset of the lanes the serial loop will rerank;
//  * an expansion whose neighbours are all estimated already has no observable effect beyond
//    the result-heap push of the popped vertex: its FastScan arithmetic is skipped;
//  * what bounds it depends on the workload: on the SIFT-like benchmark a launch lasts as long as its
//    longest query and the steady state shares the CU's one scalar unit between 24 waves; on the recall-gate workloads
//    (beams of thousands of entries, no id locality) it is HBM-bound on the bytes it actually moves.  Hence: no
//    software prefetch, the probe is a load (atomics only for new ids), shuffles are DPP / v_permlane32_swap, and
//    everything a lane can do without an exec-mask round trip on the scalar unit is done that way;
//  * on that steady state an issued instruction costs about what it is of the 520 per expansion, so the usual expansion
//    carries none it does not need (profiles/issue_diet.md): the LDS pop's path walk is straight-line, wave votes are
//    taken on bools (ballot64 / any64 / all64), the termination tests at the loop head are two votes with a branch each
//    instead of a verdict word, and under probe first the code registers of lanes that fetch nothing stay undefined;
//  * a query's first handful of expansions differ from the other ~260: the result heap fills, the slack schedule climbs
//    its levels.  The 4-bit probe-first instantiations therefore compile the expansion loop twice from one text
//    (device_search_expansion.inc, the body of expansion_loop below): a general copy every query starts in, and a
//    steady copy it moves to -- once, at a loop head -- in which a full result heap, the last slack level and an index
//    without repeated neighbour ids are compile-time facts.  There the exact-L2 and new-neighbour counts are derived at
//    query end (from the expansion count and the id log's length) instead of being carried per expansion.  Every
//    other instantiation includes the same text once, in the kernel itself (profiles/steady_loop.md).
#pragma once
#include <cstddef>
#include <type_traits>
#include <hip/hip_runtime.h>

#include "cph_core.h"
#include "device_fastscan.h"

namespace cph {

struct Result {
    uint32_t id;
    float dist;
};

// The statistics block of one batch (SearchArgs::stats): kStatWords u64 words.  Words [0, kStatFlushed) are counters summed
// over the batch's queries: every wave adds them up in LDS (s_tot) and flushes them when it leaves.
enum StatWord : int {
    kStatExpansions = 0,        // FastScan blocks
    kStatExact = 1,             // exact L2 evaluations
    kStatNew = 2,               // new neighbours
    kStatPushes = 3,            // beam pushes
    kStatSkips = 4,             // stage-2 skipped batches
    kStatReruns = 5,            // queries handed to the re-run launch (capacity overflow or stage-2 decision)
    kStatNoCounter = 6,         // never written (cph_last_search_stats reports the launches' device time in its place)
    kStatAllSeen = 7,           // expansions whose 32 neighbours were all estimated already
    kStatStage2Reruns = 8,      // those of kStatReruns that were handed over for a stage-2 decision (probe first)
    kStatStage2Undecided = 9,   // expansions whose stage-2 decision was left open (probe first)
    // -DCPH_PHASE_TIMERS / -DCPH_TRAFFIC_STATS / -DCPH_TAIL_CENSUS: eight cycle, traffic or arm counters take words
    // 8..15; the two stage-2 words are not flushed there (and read as 0 on the host)
    kStatDiag = 8,
#if defined(CPH_PHASE_TIMERS) || defined(CPH_TRAFFIC_STATS) || defined(CPH_TAIL_CENSUS)
    kStatFlushed = 8,
#else
    kStatFlushed = 10,
#endif
    kStatQueues = 16,           // from here on u32 words, indexed by StatQueueWord
    kStatWords = 20,
};
enum StatQueueWord : int {      // the u32 words at stats + kStatQueues
    kQueueMain = 0,             // work-queue counter of the main (or direct) launch
    kQueueRerunLen = 1,         // length of the re-run list
    kQueueRerun = 2,            // work-queue counter of the re-run launch
    // a batch with per-query filters runs two pairs of launches, one over the filtered queries, one over the unfiltered:
    // the second pair's three words
    kQueueSecond = 3,
};

struct SearchArgs {
    // index
    const uint8_t* blocks;
    const float* raw;       // [n][D]
    const float* norm_sq;   // [n]
    uint64_t n;
    DevLayout L;
    uint32_t flags;         // bit 0: some vertex repeats a neighbour id; bit 1: some list's length is not a multiple of 8
    // encoded queries
    const float* queries;   // [nq][D] zero-padded
    const uint4* qmasks;    // [nq][PW]
    const QueryHeader* qhdr;
    const uint32_t* todo;   // optional: query indices to run (launch order / re-run list), else 0..nq-1
    uint32_t nq;
    const uint32_t* nq_dev; // optional: the batch size lives in device memory (the overflow re-run's list length)
    uint32_t k;
    SearchConsts sc;
    // work queue + per-slot scratch
    uint32_t* counter;
    uint64_t cap;           // per-slot log/heap capacity
    uint64_t bm_words;      // per-slot bitmap words
    uint32_t* bitmaps;
    uint32_t* beam_pages;   // beam heap levels 8..12: kBeamPagesDwords per slot (beam_page_off)
    uint32_t* beam_tail;    // beam heap levels 13+: beam_tail_dwords(cap) per slot (beam_tail_off)
    uint32_t* log_ids;      // every newly estimated id, in discovery order (for un-marking)
    // outputs
    int64_t* out_ids;       // [nq][k]
    float* out_dist;        // [nq][k]
    uint32_t* out_count;    // [nq]
    uint32_t* status;       // [nq]
    unsigned long long* stats;  // [kStatWords], see StatWord
    // queries whose beam or id log outgrew `cap` are appended here and answered by the full-capacity
    // re-run launch that follows on the same stream (no host round trip)
    uint32_t* redo;         // [nq] or null
    uint32_t* redo_count;
    // optional (coalesced cph_search callers): done_flags[qi] = done_seq once query qi's results are visible to the HOST --
    // the outputs then live in pinned, device-mapped memory and every caller waits for its own query only
    uint32_t* done_flags;
    uint32_t done_seq;
    // filtered instantiations only (FILT): allowed-id bitmap, bit id & 31 of word id >> 5.  Behind everything older, so
    // that no offset of the fields above moves
    const uint32_t* allow;
    // optional: the row map, [n] (result ids in input rows, cph_set_result_ids): a result id i leaves as rows[i].  Null:
    // internal ids.  Read once per query, where the rows are written; the search itself knows internal ids only.
    const uint32_t* rows;
    // filter-table instantiations only (FTAB): a batch whose queries carry their own filters.  allow_tab[f] = the bitmap
    // of filter f, filter_of[qi] = the filter of query qi (every query such a launch runs has one); `allow` is unused.
    const uint32_t* const* allow_tab;
    const uint32_t* filter_of;
};

// Kernel arguments that are touched once per query (work queue, encoded-query arrays, outputs, statistics) are read from
// the kernarg segment where they are used instead of living in scalar registers across the expansion loop: the
// pointer is laundered through an empty asm so that the loads cannot be hoisted.  (With every argument resident the
// allocator spilled ~50 SGPRs to VGPR lanes -- 133 v_readlane reloads in the <4,128> instantiation; now 19 and 27.
// The reloads were mostly off the expansion loop's usual path: the kernel time did not change measurably.)
template <class T>
__device__ __forceinline__ T cold_arg(size_t offset) {
    typedef __attribute__((address_space(4))) const unsigned char kbyte;
    kbyte* p = (kbyte*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(__attribute__((address_space(4))) const T*)(p + offset);
}
#define CPH_COLD(field) cold_arg<decltype(SearchArgs::field)>(offsetof(SearchArgs, field))

// ---- libstdc++-compatible binary heaps ------------------------------------------------
// Result heap: max-heap on dist (std::less via SearchResult::operator<, core/types.hpp:16).
__device__ __forceinline__ void nn_sift_up(Result* h, uint32_t hole, uint32_t top, Result v) {
    while (hole > top) {
        uint32_t p = (hole - 1) >> 1;
        Result pv = h[p];
        if (!(pv.dist < v.dist)) break;
        h[hole] = pv;
        hole = p;
    }
    h[hole] = v;
}
__device__ __forceinline__ void nn_adjust(Result* h, uint32_t hole, uint32_t len, Result v) {
    const uint32_t top = hole;
    uint32_t child = hole;
    while (child < (len - 1) / 2) {
        child = 2 * (child + 1);
        Result r = h[child], l = h[child - 1];
        if (r.dist < l.dist) { --child; r = l; }
        h[hole] = r;
        hole = child;
    }
    if ((len & 1) == 0 && child == (len - 2) / 2) {
        child = 2 * (child + 1);
        h[hole] = h[child - 1];
        hole = child - 1;
    }
    nn_sift_up(h, hole, top, v);
}
// BoundedMaxHeap::push, rabitq_search.hpp:26-35
__device__ __forceinline__ void nn_push(Result* h, uint32_t& size, uint32_t k, Result r) {
    if (size < k) {
        nn_sift_up(h, size, 0, r);
        ++size;
    } else if (r.dist < h[0].dist) {
        if (size > 1) {
            Result v = h[size - 1];
            nn_adjust(h, 0, size - 1, v);   // pop_heap
        }
        nn_sift_up(h, size - 1, 0, r);      // back() = r; push_heap
    }
}
__device__ __forceinline__ void nn_sort(Result* h, uint32_t size) {  // std::sort_heap
    while (size > 1) {
        Result v = h[size - 1];
        h[size - 1] = h[0];
        nn_adjust(h, 0, size - 1, v);
        --size;
    }
}

// Beam: std::priority_queue<BeamEntry, vector, greater> — a heap whose comparator is
// "a.est > b.est" (rabitq_search.hpp:57,79-80).  The LOGICAL heap -- which entry sits at which heap index after
// every operation -- is libstdc++'s, move for move; where a heap index lives physically is ours to choose:
//
//   heap indices 0..254      (levels 0..7)   LDS, 16 B per entry: the levels every pop walks through
//   heap indices 255..8190   (levels 8..12)  HBM, PAGES: the 62 descendants of one level-7 node over the next five
//                                            levels are one contiguous block of 64 x 12 B {est, lower, id} (six
//                                            128-byte lines; entry r = the node's 1-based index inside that subtree,
//                                            entries 0 and 1 unused) -- a B-heap page.  A pop's window (the 62
//                                            candidates of its next five levels) is one coalesced 744-byte read that
//                                            brings the WHOLE entries, so the moves along the path need no second
//                                            round trip; a push finds all its ancestors of levels 8..11 in the first
//                                            three lines of one page
//   heap indices >= 8191     (levels 13+)    HBM, 12 B per entry in heap order behind the 128 pages
//
// (Round 2 kept the HBM part as 16-byte entries in heap order: a window's 62 keys were 248 useful bytes spread over
// nine to twelve lines in five places, and the moves re-read the path's entries in a second, dependent round trip.)
constexpr uint32_t kBeamLds = 255;                    // 8 full levels, 16 B per entry
constexpr uint32_t kBeamPaged = 8191;                 // heap indices below this and >= kBeamLds live in pages
constexpr uint32_t kPageDwords = 192;                 // 64 entries x 3 dwords
constexpr uint32_t kBeamPagesDwords = 128 * kPageDwords;   // one slot's pages: 96 KB
// The pages and the tails are two arrays: [slot][pages] is what spilled beams actually touch (a beam of the recall
// workload holds ~5,000 entries, 13,800 at most), dense -- 96 KB per slot, 600 MB for 6,144 slots -- instead of 96 KB
// at the head of every slot's (cap x 12 B)-sized region, i.e. one 2-MB translation per slot; the tails (heap indices
// >= 8191, sized by `cap`) are rarely touched.
__host__ __device__ inline size_t beam_tail_dwords(uint64_t cap) {   // per slot, a multiple of 32
    const size_t d = 3 * (size_t)(cap > kBeamPaged ? cap - kBeamPaged : 0) + 4;
    return (d + 31) & ~(size_t)31;
}

struct BeamEntry {
    float est, lower;
    uint32_t id;
};

// The lane id as a value the optimiser cannot see through.  Everything a routine derives from the lane id alone is
// loop-invariant, so the compiler computes it once per kernel and keeps it in a VGPR across the whole expansion loop -- for
// the spilled-beam routines that is a dozen registers the usual expansion never uses, i.e. spills, and a spill reload inside
// the loop is a vector-memory operation in the middle of the round trips the loop overlaps (it waits for all of them:
// scripts/loop_reloads.py counts them, the count has to stay at zero on the usual path).  Routines off the usual path
// start from a laundered copy: two or three cheap instructions recomputed where they are used.
__device__ __forceinline__ int opaque_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// Wave votes on a bool.  HIP's __ballot / __any / __all take an int: a condition that already sits in an SGPR pair is
// turned into 0 / 1 in a VGPR (v_cndmask) and compared again (v_cmp_ne), and __any / __all go through a library call that
// ends in a v_readfirstlane.  These read the mask where it is.
__device__ __forceinline__ unsigned long long ballot64(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool any64(bool p) { return ballot64(p) != 0ull; }
__device__ __forceinline__ bool all64(bool p) { return ballot64(!p) == 0ull; }

// The LDS part is addressed through address-space-3 pointers so that every access is a ds_*
// instruction (a generic pointer would make them flat_* accesses, which also wait on vmcnt).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// dword offset of heap index i (kBeamLds <= i < kBeamPaged) inside the slot's pages
__device__ __forceinline__ uint32_t beam_page_off(uint32_t i) {
    const uint32_t hp = i + 1;
    const uint32_t l = ((31u - (uint32_t)__builtin_clz(hp)) - 7u) & 7u;       // levels below the LDS part: 1..5
    const uint32_t r = (hp & ((1u << l) - 1u)) | (1u << l);                   // index inside the level-7 node's subtree
    return ((hp >> l) - 128u) * kPageDwords + 3u * r;
}
// dword offset of heap index i >= kBeamPaged inside the slot's tail
__device__ __forceinline__ uint32_t beam_tail_off(uint32_t i) { return 3u * (i - kBeamPaged); }

struct Beam {
    typedef uint4 E;
    lds_u32x4* l;   // LDS, [kBeamLds + 1]   {est bits, lower bits, id, -}
    uint32_t* gp;   // global, the slot's pages (beam_page_off)
    uint32_t* gt;   // global, the slot's tail (beam_tail_off)
    // the heap's comparator (std::greater on est: a min-heap) and the key of an entry
    static __device__ __forceinline__ bool before(float a, float b) { return a > b; }
    static __device__ __forceinline__ float key_of(uint4 e) { return __uint_as_float(e.x); }
    __device__ __forceinline__ uint4 lds(uint32_t i) const {
        const u32x4 t = l[i];
        return make_uint4(t.x, t.y, t.z, t.w);
    }
    __device__ __forceinline__ void lds_put(uint32_t i, uint4 v) const {
        u32x4 t;
        t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
        l[i] = t;
    }
    __device__ __forceinline__ float lds_key(uint32_t i) const {
        return reinterpret_cast<lds_f32*>(l)[4 * i];
    }
    // one 12-byte entry at a dword offset of the pages / of the tail
    static __device__ __forceinline__ uint4 load3(const uint32_t* p) {
        const u32x3 t = *reinterpret_cast<const u32x3 __attribute__((aligned(4)))*>(p);
        return make_uint4(t.x, t.y, t.z, 0u);
    }
    static __device__ __forceinline__ void store3(uint32_t* p, uint4 v) {
        u32x3 t;
        t.x = v.x; t.y = v.y; t.z = v.z;
        *reinterpret_cast<u32x3 __attribute__((aligned(4)))*>(p) = t;
    }
    __device__ __forceinline__ uint4 pload(uint32_t off) const { return load3(gp + off); }
    __device__ __forceinline__ void pstore(uint32_t off, uint4 v) const { store3(gp + off, v); }
    __device__ __forceinline__ uint4 tload(uint32_t off) const { return load3(gt + off); }
    __device__ __forceinline__ void tstore(uint32_t off, uint4 v) const { store3(gt + off, v); }
    __device__ __forceinline__ uint32_t* spill_ptr(uint32_t i) const {       // i >= kBeamLds
        return i < kBeamPaged ? gp + beam_page_off(i) : gt + beam_tail_off(i);
    }
    __device__ __forceinline__ uint4 raw(uint32_t i) const {
        uint4 v;
        if (i < kBeamLds) v = lds(i); else v = load3(spill_ptr(i));
        return v;
    }
    __device__ __forceinline__ void put(uint32_t i, uint4 v) const {
        if (i < kBeamLds) lds_put(i, v); else store3(spill_ptr(i), v);
    }
    __device__ __forceinline__ float raw_key(uint32_t i) const {
        float k;
        if (i < kBeamLds) k = lds_key(i); else k = __uint_as_float(*spill_ptr(i));
        return k;
    }
    __device__ __forceinline__ BeamEntry get(uint32_t i) const {
        const uint4 v = raw(i);
        return BeamEntry{__uint_as_float(v.x), __uint_as_float(v.y), v.z};
    }
};

// The result heap (BoundedMaxHeap, rabitq_search.hpp:17-49) as the wave-parallel heap routines see it: k entries
// {id, dist} of 8 bytes in LDS, comparator std::less on dist (a max-heap).
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
struct NnLds {
    typedef uint2 E;
    lds_u32x2* l;
    static __device__ __forceinline__ bool before(float a, float b) { return a < b; }
    static __device__ __forceinline__ float key_of(uint2 e) { return __uint_as_float(e.y); }
    __device__ __forceinline__ uint2 lds(uint32_t i) const {
        const u32x2 t = l[i];
        return make_uint2(t.x, t.y);
    }
    __device__ __forceinline__ void lds_put(uint32_t i, uint2 v) const {
        u32x2 t;
        t.x = v.x; t.y = v.y;
        l[i] = t;
    }
    __device__ __forceinline__ float lds_key(uint32_t i) const {
        return reinterpret_cast<lds_f32*>(l)[2 * i + 1];
    }
};
constexpr uint32_t kWaveHeapMax = 256;   // largest heap the wave-parallel pop handles (two ballot masks)

__device__ __forceinline__ uint4 beam_pack(const BeamEntry& e) {
    return make_uint4(__float_as_uint(e.est), __float_as_uint(e.lower), e.id, 0u);
}

// std::pop_heap of a beam that lives entirely in LDS (size <= kBeamLds), executed by the whole
// wave instead of one lane.  The element movement is libstdc++'s __adjust_heap + __push_heap
// (same comparisons, same operand order, so ties and NaNs resolve identically); only the
// schedule differs: every internal node's "which child moves up" comparison is evaluated at
// once (lane j <-> nodes j and j+64, one ballot each), the root-to-leaf path is then walked on
// wave-uniform bit masks with no memory access, and the moves along the path are one parallel
// LDS read plus one parallel write.  Two LDS round trips instead of one dependent round trip
// per heap level.
template <class H>
__device__ __forceinline__ void heap_pop_wave(const H& h, uint32_t size, int lane_in) {
#ifdef CPH_LAUNDER_HOT      // (A/B switch: the routines of the usual path recompute their lane arithmetic as well -- fewer VGPRs, more instructions)
    const int lane = opaque_lane(lane_in);
#else
    const int lane = lane_in;
#endif
    const uint32_t len = size - 1;                // heap length once the last element is taken out
    const typename H::E v = h.lds(len);            // the value __adjust_heap re-inserts
    const uint32_t nint = (len - 1) >> 1;         // nodes j < nint have both children below len
    // true: the left child moves up.  (Read by every lane -- entries up to index 128 / 256 exist in LDS whatever the heap
    // holds -- and masked afterwards: a predicated read costs an exec-mask save / restore, and the scalar unit is what
    // this kernel runs out of.)
    const bool b0 = H::before(h.lds_key(2 * lane + 2), h.lds_key(2 * lane + 1)) && (uint32_t)lane < nint;
    bool b1 = false;
    const unsigned long long m0 = ballot64(b0);
    unsigned long long m1 = 0;
    if (nint > 64) {
        if ((uint32_t)lane + 64 < nint) b1 = H::before(h.lds_key(2 * lane + 130), h.lds_key(2 * lane + 129));
        m1 = ballot64(b1);
    }
    // Walk on hp = hole + 1: taking the left child doubles it, the right child doubles it and adds 1,
    // so after d steps hp is the binary string "1 r0 r1 .. r(d-1)" of the choices and every node on
    // the path is a prefix of it -- p_t = (hp >> (d - t)) - 1.  The loop is scalar-only; each lane
    // then derives its own pair of path positions with two shifts.
    uint32_t hp = 1, d = 0;
    if (nint >= 1) {
        // Scalar walk, two instructions per level and no branch: with the mask shifted up by one, node hp - 1's bit sits
        // at position hp; s_bitcmp0 puts "the right child moves up" into SCC and s_addc turns hp into 2 hp + SCC.
        // The walk proper goes on while hp <= nint.  With L = floor(log2(nint)) its first L steps are certain (after t
        // steps hp < 2^(t+1) <= nint), step L + 1 is taken when the hp of step L is still <= nint, and there is no
        // further one.  So six steps are made whatever the heap holds -- nodes >= nint answer "right" (their bit is masked
        // to 0 above) and only lengthen the string behind the path, which stays its prefix -- and the depth
        // d = L + (hp_L <= nint) cuts the string back.  (Until now: a rolled loop with a compare and a taken branch per
        // level.)  Nodes 63..126 (hp = 64..127: d = 7, the last step of a heap of 131 to 255 entries) take their bit from
        // a second mask at position hp - 64, which is hp's low six bits -- all the instruction looks at.
        const unsigned long long ms0 = m0 << 1;
        asm volatile(
            "s_bitcmp0_b64 %[m], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[m], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[m], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[m], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[m], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[m], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]"
            : [hp] "+s"(hp)
            : [m] "s"(ms0)
            : "scc");
        if (__builtin_expect(nint < 64u, 1)) {
            const uint32_t L = 31u - (uint32_t)__builtin_clz(nint);
            const uint32_t hl = hp >> (6u - L);
            asm("s_cmp_le_u32 %[h], %[n]\n\ts_addc_u32 %[d], %[l], 0"      // d = L + (hp_L <= nint)
                : [d] "=s"(d)
                : [h] "s"(hl), [n] "s"(nint), [l] "s"(L)
                : "scc");
            hp >>= 6u - d;
        } else {                                   // L = 6
            d = 6;
            if (hp <= nint) {                      // 64 <= hp <= 126
                const unsigned long long ms1 = (m1 << 1) | (m0 >> 63);
                asm volatile(
                    "s_bitcmp0_b64 %[m], %[hp]\n\t"
                    "s_addc_u32 %[hp], %[hp], %[hp]"
                    : [hp] "+s"(hp)
                    : [m] "s"(ms1)
                    : "scc");
                d = 7;
            }
        }
    }
    if (2 * hp == len) {                           // a last node with a left child only: len even, hole == (len - 2) / 2
        hp = 2 * hp;
        ++d;
    }
    const uint32_t hole = hp - 1;                                   // p_d, where the walk ends
    const uint32_t t = (uint32_t)lane < d ? (uint32_t)lane : 0u;
    const uint32_t my_dst = (hp >> (d - t)) - 1;                    // p_t: lane t moves entry p_{t+1} into it
    const uint32_t my_src = (hp >> (d - t - ((uint32_t)lane < d ? 1u : 0u))) - 1;   // p_{t+1}
    // __push_heap: parent (now e_t) > v -> parent moves down.  Lanes >= d read p_1 (t = 0) and are masked out below.
    const typename H::E e = h.lds(my_src);
    const bool c = H::before(H::key_of(e), H::key_of(v));
    const unsigned long long stay = ~ballot64(c) & ((1ull << d) - 1ull);
    const uint32_t fin = stay ? 64u - (uint32_t)__builtin_clzll(stay) : 0u;   // v ends at p_fin
    if ((uint32_t)lane < fin) h.lds_put(my_dst, e);
    // p_fin = (hp >> (d - fin)) - 1 for every fin (= the hole when fin == d): one writer, one wave-uniform address, behind
    // the moves in program order (lane 0's own move, if any, went to p_0 != p_fin)
    if (lane == 0) h.lds_put((hp >> (d - fin)) - 1, v);
    (void)hole;
}

// std::push_heap of `v` at index `hole` (= the heap's size before the push) for a beam that stays inside the LDS
// levels, executed by the whole wave.  libstdc++'s __push_heap moves the hole up while the parent compares greater
// than the value; the ancestors of a leaf are known from its index alone -- p_t = ((hole + 1) >> t) - 1 -- so lane
// t - 1 reads ancestor p_t, all comparisons are made at once, the number of leading "parent moves down" answers m is
// a ballot and a count, and the moves are one parallel write: ancestors 1..m each drop one step along the path, the
// value lands on p_m.  One LDS read round trip and one write instead of one dependent round trip per heap level.
template <class H>
__device__ __forceinline__ void heap_push_wave(const H& h, uint32_t hole, typename H::E v, int lane_in) {
#ifdef CPH_LAUNDER_HOT
    const int lane = opaque_lane(lane_in);
#else
    const int lane = lane_in;
#endif
    const uint32_t hp = hole + 1;
    const uint32_t depth = 31u - (uint32_t)__builtin_clz(hp);          // ancestors of the leaf (0 for the root)
    const uint32_t t = (uint32_t)lane + 1;                              // lane t - 1 looks at ancestor p_t
    const bool on = t <= depth;
    const uint32_t pt = on ? (hp >> t) - 1 : 0u;
    const typename H::E e = h.lds(pt);                                 // (lanes past the root read it again and are masked)
    const bool down = on && H::before(H::key_of(e), H::key_of(v));
    const unsigned long long stop = ~ballot64(down);                   // first ancestor that stays (bits >= depth are set)
    const uint32_t m = (uint32_t)__builtin_ctzll(stop);                 // ancestors p_1..p_m move down
    if (t <= m) h.lds_put((hp >> (t - 1)) - 1, e);                      // p_t's entry to p_(t-1), p_0 = the leaf
    if ((uint32_t)lane == m) h.lds_put((hp >> m) - 1, v);              // (m <= depth <= 8 < 64: that lane exists)
}

// ---- the same two operations for a beam that has outgrown its LDS levels (entries kBeamLds.. live in HBM) --------
// A lane-0 sift is one dependent HBM round trip per heap level below the LDS part -- 5 to 10 of them per pop once a beam
// holds thousands of entries (the recall >= 0.95 workload keeps ~5,000 on average).  The moves stay libstdc++'s; the
// schedule becomes: (1) the 7 LDS levels are walked on ballot masks as in heap_pop_wave; (2) below them the wave reads
// the PAGE of the level-7 node it arrived at -- the 62 descendants of the next five levels, one whole entry per lane,
// one coalesced read -- decides every "which child moves up" of the window with one ballot and walks five levels on
// the mask; (3) the path is then a bit string, every lane knows its pair of positions, and the entries of levels 8..12
// that move are already in registers (handed to the path's lanes by ds_bpermute): one HBM round trip per pop, followed
// only by the stores.  Beams beyond 8,191 entries (6 % of that workload's pops) continue with windows of keys over the
// heap-ordered tail and fetch those levels' path entries in a second round trip.
// History: lane-0 sifts 334 ms per 10,000 queries of that workload; windows of keys over 16-byte entries in heap
// order + a dependent read of the path (round 2) 216 ms; pages (round 3): see DESIGN.md section 6.
__device__ __forceinline__ void beam_pop_hybrid(const Beam& h, uint32_t size, int lane_in) {
    const int lane = opaque_lane(lane_in);
    const uint32_t len = size - 1;                 // >= kBeamLds: the last element lives in HBM
    const uint4 v = Beam::load3(h.spill_ptr(len));       // the value __adjust_heap re-inserts (same address in every lane)
    // LDS levels 0..6: nodes 0..126, both children always inside the LDS part
    const bool b0 = Beam::before(h.lds_key(2 * lane + 2), h.lds_key(2 * lane + 1));
    const unsigned long long m0 = ballot64(b0);
    bool b1 = false;
    if (lane < 63) b1 = Beam::before(h.lds_key(2 * lane + 130), h.lds_key(2 * lane + 129));
    const unsigned long long m1 = ballot64(b1);
    uint32_t hp = 1, d = 7;                        // hp = hole + 1, the path as a bit string (see heap_pop_wave)
    {
        // seven steps, two scalar instructions each (heap_pop_wave's walk, unrolled: every node of levels 0..6 has both
        // children); the last one reads nodes 63..126 from the second mask at position hp - 64 = hp's low six bits
        const unsigned long long ms0 = m0 << 1, ms1 = (m1 << 1) | (m0 >> 63);
        asm volatile(
            "s_bitcmp0_b64 %[a], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[a], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[a], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[a], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[a], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[a], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]\n\t"
            "s_bitcmp0_b64 %[b], %[hp]\n\ts_addc_u32 %[hp], %[hp], %[hp]"
            : [hp] "+s"(hp)
            : [a] "s"(ms0), [b] "s"(ms1)
            : "scc");
    }
    // relative node of this lane inside a five-level window: 1-based, the window's root = 1, lanes 0..61 hold 2..63
    const uint32_t r = (uint32_t)lane + 2;
    const uint32_t dr = 31u - (uint32_t)__builtin_clz(r);
    // one window: E2 = pairs of children that both exist, M = "the left child moves up"; walks up to five levels.
    // The pair under relative node P sits in lanes 2P - 2 and 2P - 1; with both masks shifted up by two its bit is at
    // position 2P: per level s_lshl (2P), s_bitcmp1 (does the pair exist), branch, s_bitcmp0 + s_addc (P <- 2P + "right").
    auto walk = [&](float key, uint32_t idx) {
        const float key_r = __shfl_down(key, 1);   // even lanes hold left children, their right siblings sit one lane up
        const bool both = (lane & 1) == 0 && lane < 62 && idx + 1 < len;
        const unsigned long long E2 = ballot64(both) << 2;
        const unsigned long long M = ballot64(both && Beam::before(key_r, key)) << 2;
        uint32_t P = 1, tmp;
        asm volatile(
            "1:\n\t"
            "s_lshl_b32 %[t], %[P], 1\n\t"
            "s_bitcmp1_b64 %[e], %[t]\n\t"
            "s_cbranch_scc0 2f\n\t"
            "s_bitcmp0_b64 %[m], %[t]\n\t"
            "s_addc_u32 %[P], %[P], %[P]\n\t"
            "s_cmp_lt_u32 %[P], 32\n\t"
            "s_cbranch_scc1 1b\n\t"
            "2:"
            : [P] "+s"(P), [t] "=&s"(tmp)
            : [e] "s"(E2), [m] "s"(M)
            : "scc");
        const uint32_t steps = 31u - (uint32_t)__builtin_clz(P);
        hp = (hp << steps) | (P & ((1u << steps) - 1u));
        d += steps;
        return steps;
    };
    // levels 8..12: the page of the level-7 node (read whenever that node has a child at all, so that every path
    // entry of these levels -- including a last left-only child -- is in some lane's registers)
    const uint32_t pbase = (hp - 128u) * kPageDwords;     // wave-uniform: everything below addresses the page relative to it
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    uint32_t steps = 0;
    if (2 * hp - 1 < len) {
        const uint32_t idx = ((hp << dr) | (r & ((1u << dr) - 1u))) - 1u;
        if (lane < 62 && idx < len) w = h.pload(pbase + 3u * r);
        steps = walk(__uint_as_float(w.x), idx);
    }
    // levels 13+: windows of keys over the heap-ordered tail
    while (steps == 5 && 2 * hp < len) {
        const uint32_t idx = ((hp << dr) | (r & ((1u << dr) - 1u))) - 1u;
        float key = 0.0f;
        if (lane < 62 && idx < len) key = __uint_as_float(h.gt[beam_tail_off(idx)]);
        steps = walk(key, idx);
    }
    if (2 * hp == len) {                           // a last node with a left child only: len even, hole == (len - 2) / 2
        hp = 2 * hp;
        ++d;
    }
    // the moves (heap_pop_wave's second half; d <= 31 lanes take part).  Lane t moves the entry at p_(t+1) to p_t;
    // p_t sits on heap level t: LDS up to level 7, the page (relative node = the level's bits of the path string
    // under a leading one) up to level 12, the tail beyond.
    const uint32_t t = (uint32_t)lane < d ? (uint32_t)lane : 0u;
    const uint32_t dst_hp = hp >> (d - t);                                     // p_t + 1
    const uint32_t src_hp = hp >> (d - t - ((uint32_t)lane < d ? 1u : 0u));    // p_(t+1) + 1, level t + 1
    auto page_rel = [](uint32_t node_hp, uint32_t lvl) {                        // lvl = heap level - 7, 1..5
        return (node_hp & ((1u << lvl) - 1u)) | (1u << lvl);
    };
    auto put_level = [&](uint32_t level, uint32_t node_hp, uint4 val) {
        if (level <= 7) h.lds_put(node_hp - 1, val);
        else if (level <= 12) h.pstore(pbase + 3u * page_rel(node_hp, level - 7u), val);
        else h.tstore(beam_tail_off(node_hp - 1), val);
    };
    // sources on levels 8..12 come out of the window lane that read them: relative node -> lane r - 2
    const bool from_page = (uint32_t)lane < d && t >= 7 && t <= 11;
    const int page_lane = (int)page_rel(src_hp, from_page ? t - 6u : 1u) - 2;
    const uint4 pw = make_uint4((uint32_t)__shfl((int)w.x, page_lane), (uint32_t)__shfl((int)w.y, page_lane),
                                (uint32_t)__shfl((int)w.z, page_lane), 0u);
    uint4 e = v;
    bool c = false;
    if ((uint32_t)lane < d) {
        if (t < 7) e = h.lds(src_hp - 1);
        else if (t <= 11) e = pw;
        else e = h.tload(beam_tail_off(src_hp - 1));
        c = Beam::before(Beam::key_of(e), Beam::key_of(v));
    }
    const unsigned long long stay = ~ballot64(c) & ((1ull << d) - 1ull);
    const uint32_t fin = stay ? 64u - (uint32_t)__builtin_clzll(stay) : 0u;
    if ((uint32_t)lane < fin) put_level(t, dst_hp, e);
    if (fin == d) { if (lane == 0) put_level(d, hp, v); }
    else if ((uint32_t)lane == fin) put_level(t, dst_hp, v);
}

// std::push_heap of `v` at index `hole` >= kBeamLds: heap_push_wave on the hybrid accessors -- the ancestors of the
// leaf (LDS or HBM, by index) are read by one lane each, one round trip whatever the depth.  A leaf inside the pages
// (hole < 8191: the usual case) has all its HBM ancestors in its own page, at the leaf's relative index shifted right.
__device__ __forceinline__ void beam_push_hybrid(const Beam& h, uint32_t hole, uint4 v, int lane_in) {
    const int lane = opaque_lane(lane_in);
    const uint32_t hp = hole + 1;
    const uint32_t depth = 31u - (uint32_t)__builtin_clz(hp);
    const uint32_t t = (uint32_t)lane + 1;
    const bool on = t <= depth;
    uint4 e = v;
    bool down = false;
    if (hp <= kBeamPaged) {
        const uint32_t lvl = depth - 7u;                                       // 1..5 (wave-uniform, like everything up to rl)
        const uint32_t pbase = ((hp >> lvl) - 128u) * kPageDwords;
        const uint32_t rl = (hp & ((1u << lvl) - 1u)) | (1u << lvl);           // the leaf's relative index in its page
        // ancestor p_t sits on level depth - t: in the page while t < lvl (relative index rl >> t), in LDS above
        if (on) {
            if (t < lvl) e = h.pload(pbase + 3u * (rl >> t)); else e = h.lds((hp >> t) - 1);
            down = Beam::before(Beam::key_of(e), Beam::key_of(v));
        }
        const unsigned long long stop = ~ballot64(down);
        const uint32_t m = (uint32_t)__builtin_ctzll(stop);
        auto put_anc = [&](uint32_t s, uint4 val) {                            // ancestor p_s (s = 0: the leaf)
            if (s < lvl) h.pstore(pbase + 3u * (rl >> s), val); else h.lds_put((hp >> s) - 1, val);
        };
        if (t <= m) put_anc(t - 1, e);
        if ((uint32_t)lane == m) put_anc(m, v);
        return;
    }
    const uint32_t pt = on ? (hp >> t) - 1 : 0u;
    if (on) {
        e = h.raw(pt);
        down = Beam::before(Beam::key_of(e), Beam::key_of(v));
    }
    const unsigned long long stop = ~ballot64(down);
    const uint32_t m = (uint32_t)__builtin_ctzll(stop);
    if (t <= m) h.put((hp >> (t - 1)) - 1, e);
    if ((uint32_t)lane == m) h.put((hp >> m) - 1, v);
}

// BoundedMaxHeap::push (rabitq_search.hpp:26-35) by the whole wave; every argument is wave-uniform, `top` is the
// heap's current root key.  Same element movement as nn_push (which stays as the path for heaps too large for
// the two ballot masks of the wave-parallel pop).
// FULL: the caller knows that the heap is full (the steady expansion loop): the fill arm and its test are not compiled.
template <bool FULL = false>
__device__ __forceinline__ void nn_push_wave(const NnLds& w, Result* h, uint32_t& size, uint32_t k, uint32_t id, float dist,
                                             float top, int lane_in) {
#ifndef CPH_NO_LAUNDER_NN
    const int lane = opaque_lane(lane_in);     // (one expansion in four or fewer gets here: see opaque_lane)
#else
    const int lane = lane_in;
#endif
    const uint2 r = make_uint2(id, __float_as_uint(dist));
    // FULL: the heap's size is a loop invariant of the steady loop (= k).  Left visible, everything the pop derives from it
    // -- len, nint, its logarithm, the shift counts -- is hoisted in front of that loop and held in scalar registers across
    // every expansion, for the one in four that gets here: those registers are paid for with spills of the bases the usual
    // path reads (the blocks' base among them).  A laundered copy is recomputed where it is used.
    uint32_t sz = size;
    if constexpr (FULL) asm volatile("" : "+s"(sz));
    if (!FULL && sz < k) {
        if (sz < kWaveHeapMax) {
            heap_push_wave(w, sz, r, lane);
        } else {
            if (lane == 0) nn_sift_up(h, sz, 0, Result{id, dist});
            __builtin_amdgcn_wave_barrier();
        }
        ++size;
    } else if (dist < top) {
        if (sz <= kWaveHeapMax) {
            if (sz > 1) heap_pop_wave(w, sz, lane);            // std::pop_heap: the old last value sinks in from the root
            heap_push_wave(w, sz - 1, r, lane);                // back() = r; std::push_heap
        } else {
            if (lane == 0) {
                nn_adjust(h, 0, sz - 1, h[sz - 1]);
                nn_sift_up(h, sz - 1, 0, Result{id, dist});
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

__device__ __forceinline__ uint32_t bcast_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ float bcast_f32(float v) {
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(v)));
}

// LDS carve-up (bytes): qm[PW*16] | qv[D*4] | vec[512 or D*4] (popped vertex's vector, LDS-DMA target) |
// exact[128] | list[64] | slack[128] | ratio[16] | totals[80] | nn[k*8] |
// beam top levels (kBeamLds+1) x 16
constexpr uint32_t kLdsTail = 128 + 64 + 128 + 16 + 80;       // exact | list | slack | ratio | totals
// vec[] holds the popped vertex' whole vector in the instantiations with a compile-time D (LDS-DMA target)
__host__ __device__ inline uint32_t search_vec_bytes(uint32_t D, bool static_d) { return static_d ? D * 4 : 512; }
__host__ __device__ inline bool search_static_d(uint32_t D) { return D == 128 || D == 1024; }
__host__ __device__ inline size_t search_lds_bytes(uint32_t D, uint32_t PW, uint32_t k) {
    return (size_t)PW * 16 + (size_t)D * 4 + search_vec_bytes(D, search_static_d(D)) + kLdsTail +
           (((size_t)k * 8 + 15) & ~(size_t)15) + 16 * (kBeamLds + 1);
}

// LDS-DMA loads (global -> LDS, no VGPR destination), written as inline assembly on purpose: hipcc
// waits vmcnt(0) at every later load once it has issued one itself, which would serialise the
// neighbour-id wait behind the whole block.  The compiler therefore does not know about these
// loads; loads retire in order, so its own counted waits stay correct (merely conservative),
// and the one place that reads a DMA target waits explicitly.  LDS destination = M0 + lane * size.
// M0 is written inside the asm without appearing in the clobber list: it is a reserved register for
// LLVM's AMDGPU backend (clang warns that "m0" in a clobber list is not honoured); the backend never
// keeps a value live in it across other instructions -- every instruction that reads M0 gets its own
// copy glued directly in front of it -- so overwriting it here cannot be observed.
typedef __attribute__((address_space(3))) void lds_void;
__device__ __forceinline__ uint32_t lds_offset(const void* p) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_void*)p);
}
__device__ __forceinline__ void lds_dma16(const void* g, uint32_t lds_off) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds_off) : "memory");
}

// Waves per SIMD: 6 (<= 80 VGPRs) for the static D = 128 instantiations, 5 (<= 96 VGPRs) for the
// generic ones -- measured on MI355X
#ifndef CPH_SEARCH_WAVES_PER_SIMD
#define CPH_SEARCH_WAVES_PER_SIMD 5
#endif
#ifndef CPH_SEARCH_WAVES_PER_SIMD_128
#define CPH_SEARCH_WAVES_PER_SIMD_128 6
#endif
// D = 1024: the whole block's codes (up to 16 x 16 B per lane) are in flight at once: 2 waves per SIMD (3 spill:
// 7.4 against 5.2 ms per 1,000 queries at C3); LDS (query + vertex vector, 4 KB each) allows 11 per CU anyway
#ifndef CPH_SEARCH_WAVES_PER_SIMD_1024
#define CPH_SEARCH_WAVES_PER_SIMD_1024 2
#endif
#ifndef CPH_SEARCH_WAVES_PER_SIMD_128_NARROW
#define CPH_SEARCH_WAVES_PER_SIMD_128_NARROW CPH_SEARCH_WAVES_PER_SIMD_128
#endif
__host__ __device__ constexpr int search_waves_per_simd(int sd, int bw) {
    return sd == 128 ? (bw <= 2 ? CPH_SEARCH_WAVES_PER_SIMD_128_NARROW : CPH_SEARCH_WAVES_PER_SIMD_128)
                     : (sd == 1024 ? CPH_SEARCH_WAVES_PER_SIMD_1024 : CPH_SEARCH_WAVES_PER_SIMD);
}
// PF: the probe-first order of the loads (see the expansion loop).  The small-batch launch uses the instantiation without it:
// a handful of queries is a matter of latency, and the third dependent round trip costs a single query 10 % (565 -> 624 us).
// FILT: filtered search -- only ids whose bit is set in SearchArgs::allow enter the result heap (the reference's nn.push at
// its three call sites, gated; nothing else changes: every vertex is still estimated, reranked, pushed into the beam and
// expanded as before).  Instantiated without probe first only: its stage-2 hand-over is never combined with a filter.
// FTAB (with FILT): the bitmap is the query's own -- looked up in SearchArgs::allow_tab once, where the query is taken from
// the work queue, and kept in scalar registers; the expansion loop is the FILT one.  A FILT instantiation without FTAB
// reads SearchArgs::allow as ever.
template <int BW, int SD, bool PF = true, bool FILT = false, bool FTAB = false>
__global__ __launch_bounds__(64, search_waves_per_simd(SD, BW)) void search_kernel(SearchArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = threadIdx.x;
    const int li = lane & 31;
    const uint32_t D = SD ? SD : a.L.D;
    const uint32_t PW = SD ? (SD >= 32 ? SD / 32 : 1) : a.L.PW;
    const uint32_t k = a.k;
    uint4* qm = reinterpret_cast<uint4*>(smem);
    float* qv = reinterpret_cast<float*>(smem + (size_t)PW * 16);
    unsigned char* fixed = smem + (size_t)PW * 16 + (size_t)D * 4;
    float* s_vec = reinterpret_cast<float*>(fixed);
    constexpr uint32_t vsz = SD >= 128 ? (uint32_t)SD * 4u : 512u;
    float* s_exact = reinterpret_cast<float*>(fixed + vsz);
    uint8_t* s_list = fixed + vsz + 128;
    float* s_slack = reinterpret_cast<float*>(fixed + vsz + 192);
    double* s_ratio = reinterpret_cast<double*>(fixed + vsz + 320);   // [2]
    // The work counters of this wave's queries are summed here and reach the statistics line in HBM ONCE, when the wave
    // leaves: six atomics per query on one line from six thousand waves are a queue in the L2's atomic unit that every
    // query's first load has to wait behind (vmcnt counts them).
    unsigned long long* s_tot = reinterpret_cast<unsigned long long*>(fixed + vsz + 336);   // [10], indexed by StatWord
    if (lane < 10) s_tot[lane] = 0ull;
    Result* nn = reinterpret_cast<Result*>(fixed + vsz + kLdsTail);
    NnLds nnw;
    nnw.l = (lds_u32x2*)(fixed + vsz + kLdsTail);
    // the beam's LDS levels, 16-B aligned, addressed as LDS (address space 3)
    const uint32_t beam_off = PW * 16 + D * 4 + vsz + kLdsTail + ((k * 8 + 15) & ~15u);
    lds_u32x4* s_beam = (lds_u32x4*)(smem + beam_off);

    // LDS byte offset of s_vec for the DMA's M0: the dynamic LDS starts right behind the kernel's static
    // LDS (none here), so this is a compile-time constant -- a generic-to-LDS pointer cast would be
    // re-derived (with its null check) by ten scalar instructions in every expansion
    const uint32_t vec_off = __builtin_amdgcn_groupstaticsize() + PW * 16 + D * 4;
    const uint32_t slot = blockIdx.x;
    uint32_t* bm = CPH_COLD(bitmaps) + (size_t)slot * CPH_COLD(bm_words);
    uint32_t* logi = CPH_COLD(log_ids) + (size_t)slot * a.cap;
    Beam heap;
    heap.l = s_beam;
    heap.gp = CPH_COLD(beam_pages) + (size_t)slot * kBeamPagesDwords;
    heap.gt = CPH_COLD(beam_tail) + (size_t)slot * beam_tail_dwords(a.cap);
    const float FMAX = 3.402823466e+38f;
    if (lane < kMaxSlack) s_slack[lane] = a.sc.slack[lane];

    // No next-top prefetch (the reference has one, :124-128).  It was kept for batches that fit the resident slots
    // ("latency mode") until the end of round 2, when it measured as a loss at every batch size with the current kernel:
    // a single query 718 -> 622 us per call without it, 32 queries 960 -> 829 us, 2,000 queries 1,396 -> 1,129 us
    // (scripts/slot_fraction_sweep.py, scripts/single_query_latency.py) -- the ~40 % of predictions that a later push
    // invalidates cost bandwidth and issue slots, and the pop already runs under the block's own latency.  (Earlier:
    // switching it on when a larger batch starts to drain, or per query for the head or the tail of the launch order,
    // were 1-4 % slower on the 10k batch or far worse, profiles/r2_lat_sweep.jsonl.)
    // Hiding more latency per wave buys nothing either -- tried and measured on one box: issuing the next expansion's loads
    // before this expansion's beam pushes (the next top is known without doing them) 2.36 -> 2.46 ms per 10k queries; doing
    // the same at a second issue site made the register allocator copy the loaded registers at the loop head, i.e. wait
    // for them: 2.50 ms.  Round 4: raising the priority of a wave whose query has passed 200 / 300 / 400 expansions
    // (s_setprio; a launch lasts as long as its longest query) changed nothing either way.
    const uint32_t* nq_dev = CPH_COLD(nq_dev);
    const uint32_t nq = nq_dev ? *nq_dev : CPH_COLD(nq);
    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(CPH_COLD(counter), 1u);
        t = bcast_u32(t);
        if (t >= nq) break;
        const uint32_t* todo = CPH_COLD(todo);
        const uint32_t qi = todo ? todo[t] : t;

        {
            const uint4* qmasks = CPH_COLD(qmasks);
            const float* queries = CPH_COLD(queries);
            for (uint32_t w = lane; w < PW; w += 64) qm[w] = qm_lds_word(qmasks[(size_t)qi * PW + w], nib_codes<BW, SD>(a.L));
            for (uint32_t d = lane; d < D; d += 64) qv[d] = queries[(size_t)qi * D + d];
        }
        const QueryHeader hd = CPH_COLD(qhdr)[qi];
        const uint32_t* allow_q = nullptr;
        if constexpr (FTAB) allow_q = CPH_COLD(allow_tab)[CPH_COLD(filter_of)[qi]];
        __syncthreads();

        QP qp;
        qp.A = hd.A; qp.B = hd.B; qp.C = hd.C;
        {
            // The estimator's calibration constants as opaque scalar values: left as plain kernarg reads the compiler
            // re-reads them from the kernarg segment inside every expansion when it is short of scalar registers -- an
            // s_load + s_waitcnt lgkmcnt(0) three times on the dependent chain (1 % of the kernel's time).
            float af_a = a.sc.affine_a, af_b = a.sc.affine_b, fl = a.sc.ip_qo_floor;
            asm volatile("" : "+s"(af_a), "+s"(af_b), "+s"(fl));
            qp.affine_a = af_a; qp.affine_b = af_b; qp.floor = fl;
        }
        // (Not the blocks' base: the <4,128,true> instantiation used to re-read a.blocks at the head of every expansion,
        // and carrying it per query the same way cost four more SGPR spills inside the loop -- 1.6 % slower on C2.  With
        // the loop head below the allocator keeps it resident by itself; profiles/issue_diet.md.  With the expansion loop
        // compiled twice the re-read is back in both copies of <4,128,true>, and carrying the base per query still loses:
        // 15 -> 29 SGPR spills, 13.51 -> 13.69 ms per 100,000 queries; profiles/steady_loop.md.  With the steady copy's
        // push tail reshaped and two values fewer carried through the loop the allocator keeps the base resident
        // again: no s_load on the usual steady expansion, 15 -> 12 SGPR spills; profiles/steady_tail.md.)
        qp.slack = s_slack[0];
        const float gamma = a.sc.gamma;

        // query_norm_sq = dot(q, q)  (:88)
        float qnorm;
        {
            float c = 0.0f;
            for (uint32_t i = lane & 7; i < D; i += 8) c = __fmaf_rn(qv[i], qv[i], c);
            qnorm = bcast_f32(group_reduce8_lo(c));
        }

        // wave-uniform heap sizes (re-broadcast after every lane-0 section)
        uint32_t beam_size = 0, nn_size = 0;
        float gamma_q = gamma;
        // gamma-adaptation running sums live in LDS (touched only when a neighbour is reranked)
        if (lane == 0) { s_ratio[0] = 0.0; s_ratio[1] = 0.0; nn[0].dist = FMAX; }   // (an empty result heap reads as threshold FLT_MAX)
        uint32_t ratio_count = 0;
        // uniform state
        uint32_t log_count = 0;
        int slack_batch = 0;
        bool overflow = false, wipe = false, stage2_redo = false;
#ifdef CPH_ONE_LOOP      // (A/B switch: no steady copy anywhere)
        constexpr bool kTwoLoops = false;
#else
        // The expansion loop below is compiled twice where that was measured to pay and costs neither a wave nor a
        // spilled VGPR: the 4-bit probe-first instantiations of the main launch (C2: <4,128,true>, C3: <4,1024,true>).
        // Every other instantiation keeps one loop, its counters and the allocation it had -- the ones without probe
        // first gained two spilled VGPRs with a second copy and <2,128,true> went from 78 to 80 VGPRs
        // (profiles/steady_loop.md, section 2).
        constexpr bool kTwoLoops = PF && SD >= 128 && BW == 4;
#endif
        // With two loops, exact L2 evaluations and new neighbours are not counted per expansion: the entry and every
        // expansion evaluate one distance each, so st_exact counts the speculative reranks only -- touched in the rare
        // expansion that has candidates --, and every new neighbour is logged, so the id log's length knows their number.
        constexpr bool kDerivedCounters = kTwoLoops;
        // ... and state that only a rare arm changes is not carried through the loop at all: the speculative reranks are
        // added to the wave's total in LDS where they happen, and `wipe` is what the id log's length says (it only grows,
        // and goes on counting once the log is full).  Every value the loop carries is copied on its latch and on the
        // exits that leave it unchanged; these two were among them (profiles/steady_tail.md).
        constexpr bool kRareOffLoop = kTwoLoops;
        uint32_t st_exp = 0, st_exact = 0, st_new = 0, st_push = 0, st_skip = 0, st_allseen = 0;
        // probe first only: expansions where the reference's stage-2 decision is unobservable and was left open (the reference
        // may have skipped stage 2 there or not -- st_skip counts the skips that were decided)
        uint32_t st_undecided = 0;
#ifdef CPH_TRAFFIC_STATS
        // diagnostic build only: what the spilled beam and the estimated-set probe touch (stats[8..15])
        unsigned long long trf[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
#ifdef CPH_TAIL_CENSUS
        // diagnostic build only: which arm of the push tail the STEADY copy's expansions take (stats[8..15]; scripts/tail_census.py):
        // 0 append in LDS | 1 append onto a spilled beam | 2 single push onto a spilled beam, append skipped | 3 a push beats
        // its parent, serial pushes | 4 new neighbours, nothing to push | 5 more pushes than the beam can check, serial |
        // 6 candidates: the serial replay | 7 expansions that reach the lane-parallel arm
        unsigned long long tcs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define CPH_CENSUS(i) do { if constexpr (ST) tcs[i]++; } while (0)
#else
#define CPH_CENSUS(i) do {} while (0)
#endif
#ifdef CPH_PHASE_TIMERS
        unsigned long long tph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        unsigned long long tlast = clock64();
#define CPH_TICK_(i) do { unsigned long long tn_ = clock64(); tph[i] += tn_ - tlast; tlast = tn_; } while (0)
        // -DCPH_PHASE_TIMERS=2: finer buckets along one expansion's dependent chain (CPH_TICKF), for the latency-bound workloads:
        // 0 head + load issue | 1 pop (incl. its windows) | 2 rest of the block wait | 3 probe issue, exact distance, result push |
        // 4 estimator | 5 rest of the probe wait | 6 marking, candidates, speculative rerank | 7 beam pushes + loop tail
#if CPH_PHASE_TIMERS + 0 == 2
#define CPH_TICK(i) do {} while (0)
#define CPH_TICKF(i) CPH_TICK_(i)
#else
#define CPH_TICK(i) CPH_TICK_(i)
#define CPH_TICKF(i) do {} while (0)
#endif
#else
#define CPH_TICK(i) do {} while (0)
#define CPH_TICKF(i) do {} while (0)
#endif

        // entry: ep_est = exact_l2(ep); beam.push({ep_est, 0, ep}); mark estimated (:95-97)
        {
            const uint32_t ep = hd.entry;
            const float enorm = a.norm_sq[ep];
            float dot = group_dot8_lo(qv, a.raw + (size_t)ep * D, D, lane & 7);
            float ex = exact_from_dot(qnorm, enorm, dot);
            if constexpr (!kDerivedCounters) st_exact++;
            if (lane == 0) {
                logi[0] = ep;
                heap.put(0, beam_pack(BeamEntry{ex, 0.0f, ep}));
                atomicOr(&bm[ep >> 5], 1u << (ep & 31));
            }
            beam_size = 1;
            log_count = 1;
        }
        __syncthreads();

        // The expansion loop, compiled twice from this one text.  A query starts in the GENERAL copy (ST = false), which
        // knows nothing about the state.  At a loop head -- only there, once and one way -- it moves into the STEADY copy
        // (ST = true) when the result heap is full, the slack schedule has reached its last level and the index repeats
        // no neighbour id.  All three facts are final: nn_size never falls, slack_batch only rises, flags is the
        // index's.  So no event sends a query back: a spilled beam, a full id log (`wipe`), capacity overflow and the
        // stage-2 hand-over are handled in place, as they are in the general copy (the last two end the attempt; the
        // spilled-beam routines sit behind wave-uniform branches off the usual path, and a way back would keep the
        // general loop's state alive across the steady one -- scalar registers are what this kernel is short of).  In
        // the steady copy `full`, `warmup`, the fill arm of the result heap, the slack-level block and the repeated-id
        // screen are compile-time facts; qp.slack is a per-query scalar.  Returns true for "go on in the steady copy".
        // The text lives in device_search_expansion.inc.  Where there are two copies it is the body of a generic lambda
        // on a bool constant; where there is one it stands in the kernel itself, as it always did: wrapped in a lambda
        // these instantiations allocate differently, and four of them (<1,128,true> and three generic ones) spilled
        // one or two VGPRs more (profiles/steady_loop.md, section 2).
        if constexpr (kTwoLoops) {
            auto expansion_loop = [&](auto steady_c) __attribute__((always_inline)) -> bool {
                constexpr bool ST = decltype(steady_c)::value;
#define CPH_GO_STEADY return true
#include "device_search_expansion.inc"
#undef CPH_GO_STEADY
                return false;
            };
            if (expansion_loop(std::false_type{})) {
                // the slack level of every expansion from here on, as a scalar (the general copy re-reads its level from
                // LDS into a vector register in every expansion and waits for it on the dependent chain)
                if (a.sc.num_slack > 0) qp.slack = bcast_f32(s_slack[a.sc.num_slack - 1]);
                expansion_loop(std::true_type{});
            }
        } else {
            constexpr bool ST = false;
#define CPH_GO_STEADY do {} while (0)
#include "device_search_expansion.inc"
#undef CPH_GO_STEADY
        }

        // (an attempt that ends between the test and the addition has overflowed: it wipes in any case)
        if constexpr (kRareOffLoop) wipe = log_count > a.cap;
        // ---- results (:276; src/bindings.cpp:202-210) ----------------------------------
        if (lane == 0 && !overflow) nn_sort(nn, nn_size);
        const uint32_t nn_final = bcast_u32(nn_size);
        __syncthreads();
        if (!overflow) {
            int64_t* out_ids = CPH_COLD(out_ids);
            float* out_dist = CPH_COLD(out_dist);
            const uint32_t* rows = CPH_COLD(rows);
            for (uint32_t j = lane; j < k; j += 64) {
                if (j < nn_final) {
                    // (translated here and not by a pass behind the kernel: the done flag below tells a cph_search
                    // caller that its row is final)
                    out_ids[(size_t)qi * k + j] = (int64_t)(rows ? rows[nn[j].id] : nn[j].id);
                    out_dist[(size_t)qi * k + j] = nn[j].dist;
                } else {
                    out_ids[(size_t)qi * k + j] = -1;
                    out_dist[(size_t)qi * k + j] = FMAX;
                }
            }
        }
        if (lane == 0) {
            CPH_COLD(out_count)[qi] = nn_final;
            // bits 0..7: QueryStatus; bits 8..31: vertices expanded (per-query work, for load analysis)
            CPH_COLD(status)[qi] = (overflow ? kStatusOverflow : kStatusOk) | (st_exp << 8);
            s_tot[kStatExpansions] += st_exp;
            // derived: the entry, one per expansion, the speculative reranks; every logged id but the entry (the log goes
            // on counting after a wipe)
            s_tot[kStatExact] += kDerivedCounters ? 1u + st_exp + st_exact : st_exact;
            s_tot[kStatNew] += kDerivedCounters ? log_count - 1u : st_new;
            s_tot[kStatPushes] += st_push;
            s_tot[kStatSkips] += st_skip;
            s_tot[kStatAllSeen] += st_allseen;
            if (stage2_redo) s_tot[kStatStage2Reruns] += 1;
            s_tot[kStatStage2Undecided] += st_undecided;
#if defined(CPH_PHASE_TIMERS) || defined(CPH_TRAFFIC_STATS) || defined(CPH_TAIL_CENSUS)
            unsigned long long* stats = CPH_COLD(stats);
#endif
#ifdef CPH_TAIL_CENSUS
            for (int i = 0; i < 8; ++i) atomicAdd(&stats[kStatDiag + i], tcs[i]);
#endif
#ifdef CPH_PHASE_TIMERS
            for (int i = 0; i < 8; ++i) atomicAdd(&stats[kStatDiag + i], tph[i]);
#endif
#ifdef CPH_TRAFFIC_STATS
            for (int i = 0; i < 8; ++i) { if (i == 6) atomicMax(&stats[kStatDiag + i], trf[i]); else atomicAdd(&stats[kStatDiag + i], trf[i]); }
#endif
            if (overflow) {
                s_tot[kStatReruns] += 1;
                uint32_t* redo = CPH_COLD(redo);
                if (redo) redo[atomicAdd(CPH_COLD(redo_count), 1u)] = qi;
            }
        }
        if (uint32_t* done_flags = CPH_COLD(done_flags); done_flags != nullptr && !overflow) {
            __threadfence_system();      // every lane's result stores, and lane 0's count, before the flag
            if (lane == 0) __hip_atomic_store(&done_flags[qi], CPH_COLD(done_seq), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        // ---- clear the estimated set: un-mark the logged ids (or wipe after overflow) --
        __syncthreads();
        if (overflow || wipe) {
            const uint64_t bm_words = CPH_COLD(bm_words);
            for (uint64_t w = lane; w < bm_words; w += 64) bm[w] = 0u;
        } else {
            for (uint32_t j = lane; j < log_count; j += 64) bm[logi[j] >> 5] = 0u;
        }
        __syncthreads();
    }
    // the wave leaves: its totals go to the statistics line
    if (lane < kStatFlushed) {
        const unsigned long long v = s_tot[lane];
        // (an atomic add of a constant zero is turned into an atomic LOAD of the line by the compiler -- a synchronous
        // round trip; the values here are not constants, and zeros are skipped anyway)
        if (v != 0ull && lane != kStatNoCounter) atomicAdd(&CPH_COLD(stats)[lane], v);
    }
}

}  // namespace cph

