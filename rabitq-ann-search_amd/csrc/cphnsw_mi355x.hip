// cphnsw_mi355x.hip — C-ABI of the MI355X-native CP-HNSW hot path (include/cphnsw_mi355x.h).
//
// Host orchestration only; the arithmetic lives in device_fastscan.h / device_search.h /
// device_stream.h (GPU) and host_index.h (per-query feeders still on the host).
// The product path has no CPU fallback: without a HIP device every compute entry point
// fails with CPH_RUNTIME_ERROR.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/cphnsw_mi355x.h"
#include "cph_core.h"
#include "device_buf.h"
#include "device_encode.h"
#include "device_fastscan.h"
#include "device_search.h"
#include "device_stream.h"
#include "device_heap_test.h"
#include "device_estimator_test.h"
#include "device_relayout.h"
#include "device_rows.h"
#include "device_tombstone.h"
#include "device_labels.h"
#include "device_tags.h"
#include "device_facets.h"
#include "device_filter_ops.h"
#include "device_exact.h"
#include "device_range.h"
#include "device_tail.h"
#include "device_diverse.h"
#include "device_group.h"
#include "device_maxsim.h"
#include "device_maxsim_rescore.h"
#include "device_fused.h"
#include "device_rescore.h"
#include "device_normalize.h"
#include "device_ip.h"
#include "host_index.h"
#include "host_parallel.h"
#include "host_knn.h"
#include "search_coalescer.h"
#include "multi_device.h"
#include "partitioned.h"
#include "device_merge.h"
#include "native_file.h"
#include "builder_pipeline.h"

using namespace cph;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

struct InvalidArg : std::invalid_argument {
    using std::invalid_argument::invalid_argument;
};
struct NotImplemented : std::runtime_error {
    using std::runtime_error::runtime_error;
};

template <class F>
int guarded(F&& f) {
    try {
        f();
        return CPH_OK;
    } catch (const std::invalid_argument& e) {
        return fail(CPH_INVALID_ARGUMENT, e.what());
    } catch (const std::bad_alloc&) {
        return fail(CPH_OUT_OF_MEMORY, "out of memory");
    } catch (const NotImplemented& e) {
        return fail(CPH_NOT_IMPLEMENTED, e.what());
    } catch (const std::exception& e) {
        return fail(CPH_RUNTIME_ERROR, e.what());
    }
}

size_t next_pow2(size_t n) {
    size_t p = 1;
    while (p < n) p *= 2;
    return p;
}

// kernel dispatch over (bits, static D) of block_hook_kernel and fastscan_stream_kernel: D == 128 and D == 1024 (the
// BASELINE shapes) get instantiations with a compile-time D.  (The search kernel has its own table: launch_search_kernel.)
#define CPH_LAUNCH_BITS(KERNEL, bits, SDV, grid, block, lds, st, args)                            \
    do {                                                                                          \
        if ((bits) == 1) hipLaunchKernelGGL((KERNEL<1, SDV>), grid, block, lds, st, args);        \
        else if ((bits) == 2) hipLaunchKernelGGL((KERNEL<2, SDV>), grid, block, lds, st, args);   \
        else hipLaunchKernelGGL((KERNEL<4, SDV>), grid, block, lds, st, args);                    \
    } while (0)
#define CPH_LAUNCH(KERNEL, bits, D, grid, block, lds, st, args)                                   \
    do {                                                                                          \
        if ((D) == 128) CPH_LAUNCH_BITS(KERNEL, bits, 128, grid, block, lds, st, args);           \
        else if ((D) == 1024) CPH_LAUNCH_BITS(KERNEL, bits, 1024, grid, block, lds, st, args);    \
        else CPH_LAUNCH_BITS(KERNEL, bits, 0, grid, block, lds, st, args);                        \
        HIP_CHECK(hipGetLastError());                                                             \
    } while (0)

// Sets bit 1 of *flags when some vertex' neighbour list has a length that is not a multiple of 8: such a list ends in the
// reference's scalar tail (device_fastscan.h: TailLanes), which the probe-first search instantiation leaves out.
__global__ void scan_counts_kernel(const uint8_t* blocks, uint64_t n, uint32_t stride, uint32_t count_off, uint32_t* flags) {
    const uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t cnt = *reinterpret_cast<const uint32_t*>(blocks + v * stride + count_off);
    if (cnt & 7u) atomicOr(flags, 2u);
}

}  // namespace

// One in-flight batch: query staging, outputs, statistics and per-slot scratch.  A handle owns two,
// used alternately, so that a batch enqueued on one stream can start while the previous one (on
// another stream) is still draining its longest queries.
struct BatchSet {
    DevBuf<float> d_queries_raw, d_queries, d_entry_dist, d_dist;
    DevBuf<uint4> d_qmasks;
    DevBuf<QueryHeader> d_qhdr;
    DevBuf<int64_t> d_ids;
    DevBuf<uint32_t> d_count, d_status, d_order, d_redo;
    DevBuf<unsigned long long> d_stats;        // kStatWords u64 words: counters, then the work queues (device_search.h: StatWord)
    unsigned long long* pin_stats = nullptr;   // pinned host copy, written at the end of every batch
    // small batches (cph_search, cph_search_batch with a handful of queries): queries are read and results written by
    // the kernels straight from / to this pinned, device-mapped host buffer -- no copy commands at all
    uint8_t* pin_io = nullptr;
    uint8_t* pin_io_dev = nullptr;
    size_t pin_io_bytes = 0;
    // per-slot scratch (estimated-set bitmap, beam spill area, id log), `cap` entries per slot
    DevBuf<uint32_t> d_bitmaps, d_logids;
    DevBuf<uint32_t> d_beam, d_beam_tail;
    uint32_t slots = 0;
    uint64_t cap = 0;
    // full-capacity (n + 1) scratch of the overflow re-run launch
    DevBuf<uint32_t> r_bitmaps, r_logids;
    DevBuf<uint32_t> r_beam, r_beam_tail;
    uint32_t r_slots = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_done = nullptr;
    bool used = false;        // a batch has been enqueued on this set (ev_done is meaningful)
    uint32_t nq = 0;          // size of that batch
    uint32_t run_slots = 0;   // slots its search launch used
    uint64_t run_cap = 0;     // per-slot capacity that launch ran with (n + 1 on the full-capacity slots of the small-batch path)
    // exact batches (device_exact.h): padded queries and their norms, the (part, query) pools and their fill counts
    DevBuf<float> x_qpad, x_qnorm;
    DevBuf<unsigned long long> x_pools;
    DevBuf<uint32_t> x_counts;
    bool stats_in_hbm = false; // the last batch's statistics were not copied to pin_stats yet
    // batches with per-query filters (enqueue_filters): the call's tables -- scan descriptors, permutation, work lists,
    // filter_of, bitmap pointers -- travel as one staged table on the batch's stream.  d_redo2: the re-run list of the
    // batch's second pair of graph launches
    StagedTable tab;
    DevBuf<uint32_t> d_redo2;
    // cosine metric (metric_queries): the batch's normalised queries; an L2 handle never allocates it
    // (inner product: the augmented queries [nq][dim + 1], and m_c [nq] = |q|^2 + M2, what the epilogue subtracts)
    DevBuf<float> m_queries, m_c;
};
constexpr int kMaxBatchSets = 4;

// The device buffers of one range search (cph_range).  A handle keeps up to kRangeScratchKept idle ones for the next call.
struct RangeScratch {
    DevBuf<float> d_q, qpad, qnorm, d_rad, g_dist, o_dist;
    DevBuf<int64_t> g_ids, o_ids;
    DevBuf<uint32_t> counts;
    DevBuf<unsigned long long> offs, sums, d_lims, d_stats, arena, arena2;
    DevBuf<uint8_t> d_tab;
};
constexpr size_t kRangeScratchKept = 2;

// The device buffers of one search that re-ranks candidate rows (the re-rankers below), grouped by what owns them.  A handle
// owns kMaxBatchSets of these sets, used in turn and only ever grown (Reserve); a handle that never calls a feature
// allocates nothing for it.
constexpr int kMaxRerankOuts = 6;
struct RerankScratch {
    // the [n][C] candidate rows of the underlying search; `ev` follows the last kernel that touched the set, the next call
    // on it makes its stream wait for that
    struct Rows {
        DevBuf<int64_t> ids;
        DevBuf<float> dist;
        hipEvent_t ev = nullptr;
        bool used = false;
        ~Rows() { if (ev) (void)hipEventDestroy(ev); }
    } rows;
    // host form: the staged queries, the staged full queries of the rescored search, one byte buffer per output slot (RerankOuts)
    struct HostForm {
        DevBuf<float> q, fq;
        DevBuf<uint8_t> out[kMaxRerankOuts];
    } host;
    // the call's host tables (n_tokens; filter_of and bitmap pointers; weights and n_vectors): one copy command per call
    StagedTable tab;
    // rescored maxsim and fused: the token rows as the search saw them (q: cosine only), padded, with their norms
    struct Padded {
        DevBuf<float> q, qpad, qnorm;
        DevBuf<unsigned long long> stats;
    } pad;
    // rescored maxsim: the candidates of the lower-bound pass, the exact scores and argmin ids of every candidate slot
    struct Cand {
        DevBuf<int32_t> keys, hits, found;
        DevBuf<float> lb, score;
        DevBuf<uint32_t> rows;
    } cand;
    // fused: the union of every query's candidate rows and its exact weighted sums
    struct Union {
        DevBuf<uint32_t> ids, hits, count;
        DevBuf<float> score;
        void reserve(Reserve& r, size_t n, size_t slots) { r(ids, slots), r(hits, slots), r(score, slots), r(count, n); }
    } un;
    Reserve reserve() const { return Reserve{rows.ev, rows.used}; }      // growing: the set's previous batch must be done
};

// The inverted key column of one int32 column (host_maxsim_rescore.h: key_rows_host), resident: what the rescored maxsim
// search walks.  Made on the host on first use (or by cph_prepare_maxsim_rescore) and kept where its column lives: in the
// cph_group_keys object, or on the handle for the label column, where whatever changes the column drops it.
struct KeyRows {
    DevBuf<uint32_t> ids, offsets;
    DevBuf<int32_t> keys;
    uint32_t n_keys = 0;
    uint64_t size = 0;                         // ids it covers
    const int32_t* column = nullptr;           // the device column it was made from
};
constexpr uint64_t kSmallBatch = 32;        // batches up to this size take the copy-free path of cph_search / cph_search_batch
// The passes a handle can time (PassTimer).  kPassMaxsimRescore is the scan kernel of the rescored maxsim search alone, bracketed
// inside that search's pass; the pass as a whole goes by kPassUntimed, a timer nothing switches on.  kPassRescored: the
// rescoring kernel of cph_search_rescored* (device_rescore.h).  kPassFused: the scan kernel of fused search alone, bracketed the
// same way.
enum PassKind { kPassGrouped, kPassDiverse, kPassMaxsim, kPassLabels, kPassMaxsimRescore, kPassRescored, kPassFused, kPassTags, kPassFacets, kPassUntimed, kPassKinds };

// The facet dictionary of one column (cph_facet_*; device_facets.h): its distinct values ascending, on both sides, and one
// 32-bit code per row -- per CSR entry for a tag column -- on the device.  Made on first use, dropped when the column changes.
struct FacetDict {
    std::vector<int32_t> values;
    DevBuf<int32_t> d_values;
    DevBuf<uint32_t> codes;
};

// One row attribute of a handle, resident (host copy: host.cols, under the same id; a replica without host arrays holds
// the device copy only).  A dense column is vals[size] and no lims; a tag column is the canonical CSR lims[size + 1]
// (uint32) into vals, and vals stays unallocated while the column holds no tag at all.
struct RowColumn {
    DevBuf<int32_t> vals;
    DevBuf<uint32_t> lims;
    bool has = false;
    std::unique_ptr<FacetDict> facet;           // its facet dictionary, once asked for
};
constexpr uint32_t kLabelColumn = 0;

// An allowed-id bitmap on one device (cph_filter_create): bit id & 31 of word id >> 5, bits >= n_bits clear.
struct cph_filter {
    int device = 0;
    uint64_t n_bits = 0;
    uint64_t popcount = 0;
    DevBuf<uint32_t> words;
    // the same set as an ascending id list, for the exact scan: made on the first exact use (filter_id_list), reused after
    // that by every stream (they wait for ids_ev), freed with the filter
    mutable std::mutex ids_mu;
    mutable DevBuf<uint32_t> ids, ids_scratch;
    mutable hipEvent_t ids_ev = nullptr;
    // F & ~R for the handles with removed rows that used this filter (effective_filter): complete filters of their own
    // (bitmap, count, id list), keyed by the epoch of the handle's R -- a value no other state of any handle's R ever
    // has, so a remove makes the old entry unreachable and two handles with different R each find their own.  At most
    // kEffCached entries; one is only freed after the device has drained (EffDeleter): a batch in flight may read it.
    mutable std::mutex eff_mu;
    mutable std::vector<std::pair<uint64_t, std::shared_ptr<cph_filter>>> eff;
    // a filter of cph_filters_from_labels: `words` is a view into the one allocation that holds the bitmaps of all the
    // filters of that call, freed with the last of them
    std::shared_ptr<DevBuf<uint32_t>> slab;
    ~cph_filter() {
        if (ids_ev) (void)hipEventDestroy(ids_ev);
        if (slab) { words.p = nullptr; words.n = 0; }      // (not this filter's to free)
    }
};
constexpr size_t kEffCached = 4;
struct EffDeleter {
    void operator()(cph_filter* f) const {
        if (hipSetDevice(f->device) == hipSuccess) (void)hipDeviceSynchronize();
        delete f;
    }
};
static std::atomic<uint64_t> g_removed_epoch{0};

struct cph_index {
    // dim: the width of the rows the index stores and every kernel reads; dim_in: the width of the caller's rows and
    // queries (cph_dim).  They differ under the inner-product metric only (dim = dim_in + 1); D = next_pow2(dim).
    uint64_t dim = 0, dim_in = 0;
    uint32_t bits = 0;
    uint32_t D = 0;
    int device = 0;
    bool finalized = false;
    bool needs_build = false;          // build() done, finalize() pending
    // a replica of a cph_multi (cph_multi_replica hands it out): load, load_native, build, finalize and destroy refuse
    // it; a replica other than the first holds the host-side scalars of the index but none of its arrays (save,
    // save_native and get_vectors refuse it too)
    bool borrowed = false;
    bool host_less = false;
    // the metric (cph_set_metric, on an empty handle only).  Cosine: rows are normalised to squared norm 1/2 on the way in
    // (build, add) and queries on the way into every search (metric_queries), so the L2 kernels report 1 - cos.
    // metric_launches counts the launches of the normalisation kernel this handle made (cph_metric_stats): 0 under L2.
    uint32_t metric = CPH_METRIC_L2;
    uint64_t metric_launches = 0;
    // inner product (device_ip.h): rows are stored as [x, sqrt(M2 - |x|^2)], queries searched as [q, 0], and an epilogue
    // behind every batch turns the distances into -(q.x).  ip_bound: the caller's M2 (cph_set_ip_bound; 0: the largest
    // squared norm of the rows of the build call); ip_m2: the M2 of the rows the handle holds.
    float ip_bound = 0.0f, ip_m2 = 0.0f;
    std::vector<float> pending;        // vectors handed to build()
    uint64_t pending_n = 0;
    HostIndex host;
    DevLayout L{};
    SearchConsts sc{};
    uint32_t flags = 0;
    int num_cus = 256;
    bool waves_from_env = false;
    uint32_t waves_per_cu = 4 * CPH_SEARCH_WAVES_PER_SIMD;  // resident waves per CU (launch bounds of the search kernel)
    // device-resident index
    DevBuf<uint8_t> d_blocks;
    DevBuf<float> d_raw, d_norm;
    // the row map (input row of every internal id; host copy: host.rows), resident next to the norms; has_rows: the
    // index has one (a replica without host arrays holds the device copy only)
    DevBuf<uint32_t> d_rows;
    bool has_rows = false;
    bool ids_input = false;            // cph_set_result_ids: searches return input rows (needs has_rows)
    // the row attributes, by column id (facet_column): the label column (cph_set_labels; kLabelColumn), the attribute
    // columns (cph_set_column), the tag columns (cph_set_tags).  One lifecycle for all of them: install_column_locked,
    // sync_columns, replicate, the compact gather and the parts cut walk this array.  A handle that never saw a column
    // allocates nothing here.
    RowColumn cols[kFacetColumns];
    std::unique_ptr<KeyRows> label_rows;      // the label column inverted (rescored maxsim search), or none: made on first use
    // the call buffers of cph_filters_from_labels ([lo | hi] and the counts) and of cph_filters_from_tags (the tests and
    // the counts), which only grow
    DevBuf<int32_t> d_label_bounds;
    DevBuf<uint32_t> d_tag_tests;
    DevBuf<unsigned long long> d_label_counts, d_tag_counts;
    // facet counts (cph_facet_*): the call buffers -- the counter slab of at most facet_slab counters
    // (cph_debug_facet_slab; a single filter's U may exceed it), the filter table, the outputs of the top kernel -- which
    // only grow.  A handle that never called cph_facet_* allocates none of this.
    DevBuf<unsigned long long> d_facet_counts, d_facet_top_counts;
    DevBuf<const uint32_t*> d_facet_tab;
    DevBuf<int32_t> d_facet_top_values;
    DevBuf<uint32_t> d_facet_found;
    uint64_t facet_slab = kFacetSlabCounters;
    void drop_facets() { for (auto& c : cols) c.facet.reset(); }
    size_t exact_scratch_bytes = (size_t)1 << 30;   // pool scratch of one exact batch, at most (CPH_EXACT_SCRATCH_MB at creation): plan_exact
    uint64_t exact_threshold = 0;      // cph_set_exact_threshold: filtered batches with at most this many allowed ids are scanned exactly (0: never)
    // removed rows (cph_remove): R as a bitmap over internal ids, resident; its host copy and count are host.removed /
    // host.n_removed (what save_native writes).  rm_epoch names this state of R (g_removed_epoch); live = ~R as a filter,
    // what an unfiltered call of a handle with tombstones runs under.  tombstones: n_removed != 0, readable without the mutex.
    DevBuf<uint32_t> d_removed;
    DevBuf<unsigned long long> d_rm_count;
    uint64_t rm_epoch = 0;
    std::shared_ptr<cph_filter> live;
    std::atomic<bool> tombstones{false};
    // the tail (cph_add; device_tail.h): host.n / L stay the rows of the graph, `tail` rows live behind them at index
    // host.n + j of d_raw, d_norm, d_rows, the label column and d_removed, which then hold room for more rows than they carry
    // (tail_capacity).  tail_vecs: their host copy ([tail][dim], what cph_get_vectors and cph_compact read); the host label column
    // and host.removed cover the tail too, host.rows does not (a tail row is its own input row).  has_tail: tail != 0,
    // readable without the mutex.
    uint64_t tail = 0;
    std::vector<float> tail_vecs;
    std::atomic<bool> has_tail{false};
    // per-query feeders on the device: rotation signs + upper layers (CSR)
    DevBuf<float> d_signs;
    DevBuf<uint32_t> d_upper;          // all layers' nodes | offsets | nbrs, concatenated
    DevBuf<uint32_t> d_row_of;
    DevBuf<uint32_t> d_nbr_info;       // the mapped layers' row_of[nbrs[e]], layer after layer
    UpperLayerDev layers[kMaxUpperLayers];
    int32_t dev_max_level = 0;
    float norm_factor = 0.0f, inv_sqrt_d = 0.0f;
    // an index loaded from a native file keeps the mapping: vectors and own-code headers are served from it
    NativeMapping native_map;
    const uint8_t* own_view = nullptr;
    std::vector<uint8_t> own_store;    // own-code headers of an index built here (own_view points into it)
    // [0, kMaxBatchSets): the sets batches rotate over; behind them one private set per leader slot of cph_search
    BatchSet sets[kMaxBatchSets + kLeaderSlots];
    int n_sets = 2;                    // sets in rotation (cph_set_batch_sets): batches that may be in flight together
    int last_set = kMaxBatchSets - 1;  // the set handed out last (they take turns)
    int last_search = -1;              // the set the most recent search went to
    bool last_range = false;           // ... unless an exact range search came later: it uses no set, its one counter is
    uint64_t range_exact = 0;          //     kept here (cph_last_search_stats)
    std::vector<std::unique_ptr<RangeScratch>> range_scratch;   // idle buffers of finished range searches (under mu)
    RerankScratch rerank_scratch[kMaxBatchSets];                // buffers of the re-rankers, in rotation (under mu)
    int last_rerank = kMaxBatchSets - 1;
    // debug hooks cph_debug_time_grouped / _diverse / _maxsim / _label_filters: only while its timer is on is that pass
    // (over the candidate rows; over the label column) bracketed by the two events
    struct PassTimer {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;
        bool on = false, timed = false;
    } pass_timer[kPassKinds];
    uint64_t index_epoch = 0;          // counts the index swaps (begin_device_swap): a cph_range of an older index refuses to finish
    hipStream_t own_stream = nullptr;  // host-API calls (cph_search_batch, cph_search, hooks)
    bool order_queries = true;         // CPH_QUERY_ORDER=0 disables the closest-entry-first launch order
    // knobs
    uint32_t want_slots = 0;
    uint64_t want_cap = 0;
    uint64_t auto_cap = 0;             // grown when a batch had to re-run queries
    bool pf_off = false;               // probe first switched off: a batch sent > 2 % of its queries to the re-run launch for a stage-2 decision
    bool pf_dense = false;             // ... or suspended: the last batches found more than 6 new neighbours per expansion
    std::mutex mu;
    // concurrent cph_search callers (the reference: shared lock, T threads search in parallel, api/hnsw_index.hpp:172):
    // whoever finds no launch in flight leads one for everybody queued so far (search_coalescer.h: the policy, host only)
    SearchCoalescer coal;
    // a leader slot's resources: a stream, a pinned device-mapped I/O buffer and a batch set (sets[kMaxBatchSets + i])
    struct LeaderSlot {
        hipStream_t stream = nullptr;
        uint8_t* pin = nullptr;        // [flags kLeaderGroup x u32 | PinnedIo]
        uint8_t* pin_dev = nullptr;
        size_t pin_bytes = 0;
        uint32_t seq = 0;              // launch counter: the value the kernels write into the flags of THIS launch
        uint64_t cur_n = 0, cur_k = 0; // shape of the launch in flight (for the callers' own copies)
    } leaders[kLeaderSlots];

    void use_device() const { HIP_CHECK(hipSetDevice(device)); }
    uint64_t size() const { return host.n + tail; }         // ids a result, a filter or a label may name
};

namespace {

// The batch launch of this index runs the probe-first instantiation of the search kernel (D = 128, D = 1024): it sees only the new
// neighbours' codes, so a query whose stage-2 decision needs the others, and every index with short neighbour lists (flags
// bit 1: scalar tails), goes to the instantiation without it; so does a workload on which most neighbours are new (pf_dense).
bool probe_first(const cph_index* h) {
    return (h->L.D == 128 || h->L.D == 1024) && !(h->flags & 2u) && !h->pf_off && !h->pf_dense;
}

// The two stage-2 counters of a finished batch (w = kStatStage2Reruns / kStatStage2Undecided).  The diagnostic builds
// keep their cycle / traffic counters in those words and the kernel does not flush the two there: they read as 0.
uint64_t stage2_stat(const BatchSet& s, StatWord w) {
#if defined(CPH_PHASE_TIMERS) || defined(CPH_TRAFFIC_STATS) || defined(CPH_TAIL_CENSUS)
    (void)s; (void)w;
    return 0;
#else
    return s.pin_stats[w];
#endif
}

// What earlier batches taught the handle about its index: void once the index changes.
void reset_adaptation(cph_index* h) {
    h->auto_cap = 0;
    h->pf_off = false;
    h->pf_dense = false;
    h->last_search = -1;
    h->last_range = false;
}

// The host-side leftovers of the previous index: vectors waiting for finalize(), the native file's mapping, the own-code
// headers of an index built here.
void drop_host_state(cph_index* h) {
    h->needs_build = false;                       // api/hnsw_index.hpp:442
    std::vector<float>().swap(h->pending);
    h->pending_n = 0;
    h->native_map.reset();
    h->own_view = nullptr;
    std::vector<uint8_t>().swap(h->own_store);
    h->tail = 0;                                  // a load or a build ends the tail
    std::vector<float>().swap(h->tail_vecs);
    h->has_tail.store(false);
}

// After the host index changed: the device copy of its row map, or none -- and without a map the handle returns
// internal ids again.
void sync_row_map(cph_index* h) {
    const std::vector<uint32_t>& rows = h->host.rows;
    h->has_rows = !rows.empty();
    if (h->has_rows) {
        h->d_rows.alloc(rows.size());
        HIP_CHECK(hipMemcpy(h->d_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    } else {
        h->d_rows.release();
        h->ids_input = false;
    }
}

// ---- the column store: every row attribute of a handle under one id ----
void require_slot(uint32_t slot) {
    if (slot >= kMaxColumns) throw InvalidArg("column slot must be below " + std::to_string(kMaxColumns) + " (CPH_MAX_COLUMNS)");
}
void require_tag_slot(uint32_t slot) {
    if (slot >= kMaxTagColumns) throw InvalidArg("tag column slot must be below " + std::to_string(kMaxTagColumns) + " (CPH_MAX_TAG_COLUMNS)");
}

// The column id of (kind, slot) -- cph_index::cols, HostIndex::cols; refuses an unknown kind and a slot out of range.
uint32_t facet_column(int kind, uint32_t slot) {
    if (kind == CPH_FACET_LABEL) return kLabelColumn;
    if (kind == CPH_FACET_COLUMN) {
        require_slot(slot);
        return 1 + slot;
    }
    if (kind == CPH_FACET_TAGS) {
        require_tag_slot(slot);
        return 1 + kMaxColumns + slot;
    }
    throw InvalidArg("facet column kind must be CPH_FACET_LABEL, CPH_FACET_COLUMN or CPH_FACET_TAGS");
}
int column_kind(uint32_t col) { return col == kLabelColumn ? CPH_FACET_LABEL : col <= kMaxColumns ? CPH_FACET_COLUMN : CPH_FACET_TAGS; }
bool is_tags(uint32_t col) { return col > kMaxColumns; }

// The words of the three kinds in the messages of the calls they share.
struct ColumnWords {
    const char* plural;                          // "labels belong to ...", "labels of a partitioned index ..."
    const char* column;                          // "label column has ..."
    const char* by_row;                          // "... labels in input rows need cph_set_row_map"
    const char* setter;
};
const ColumnWords& words_of(uint32_t col) {
    static const ColumnWords kWords[3] = {{"labels", "label column", "labels in input rows need", "cph_set_labels"},
                                          {"columns", "column", "a column in input rows needs", "cph_set_column"},
                                          {"tags", "tag column", "tags in input rows need", "cph_set_tags"}};
    static_assert(CPH_FACET_LABEL == 0 && CPH_FACET_COLUMN == 1 && CPH_FACET_TAGS == 2, "kWords is indexed by kind");
    return kWords[column_kind(col)];
}
// "the index has no label column" / "... no column in slot 3" / "... no tag column in slot 1"; hint: what to call first.
std::string no_column(uint32_t col, bool hint) {
    const ColumnWords& w = words_of(col);
    std::string s = std::string("the index has no ") + w.column;
    if (col != kLabelColumn) s += " in slot " + std::to_string(col - (is_tags(col) ? 1 + kMaxColumns : 1));
    return hint ? s + ": call " + w.setter + " first" : s;
}
// The handle holds a column of this kind (CPH_FACET_COLUMN, CPH_FACET_TAGS).
bool has_columns(const cph_index* h, int kind) {
    for (uint32_t col = 0; col < kFacetColumns; ++col)
        if (column_kind(col) == kind && h->cols[col].has) return true;
    return false;
}

// The device copy of column `col`: *src in internal-id order, or (null) none.  The caller has made sure nothing reads the
// old one.  What was made from the old one goes with it.
void upload_column(cph_index* h, uint32_t col, const HostColumn* src) {
    RowColumn& c = h->cols[col];
    c.has = false;
    c.facet.reset();
    if (col == kLabelColumn) h->label_rows.reset();
    c.vals.release();
    c.lims.release();
    if (!src) return;
    auto up = [](auto& dev, const auto& host) {  // (no tag at all: the kernel gets a null base and never reads it)
        if (host.empty()) return;
        dev.alloc(host.size());
        HIP_CHECK(hipMemcpy(dev.p, host.data(), host.size() * sizeof(*dev.p), hipMemcpyHostToDevice));
    };
    up(c.lims, src->lims);
    up(c.vals, src->vals);
    c.has = true;
}

// After the host index changed: the device copy of every column it holds, or none (a load or a build leaves none).
void sync_columns(cph_index* h) {
    for (uint32_t col = 0; col < kFacetColumns; ++col) {
        const HostColumn& hc = h->host.cols[col];
        upload_column(h, col, hc.empty() ? nullptr : &hc);
    }
}

void quiesce(cph_index* h);

// The caller holds the handle mutex.  *src: the column over `size` rows in internal-id order, or null: the column goes.
// keep_host: *src moves into host.cols (what compact gathers from); a replica without host arrays keeps the device copy only.
void install_column_locked(cph_index* h, uint32_t col, HostColumn* src, bool keep_host) {
    h->use_device();
    quiesce(h);                                  // a batch in flight may be reading the old column
    upload_column(h, col, src);
    h->host.cols[col] = src && keep_host ? std::move(*src) : HostColumn();
}

hipStream_t own_stream(cph_index* h);

// F & ~R (allow null: ~R) of this handle as a filter of its own, made on the handle's stream and complete on return: the
// count is needed on the host, for the routing.
std::shared_ptr<cph_filter> make_live_filter(cph_index* h, const uint32_t* d_allow) {
    const uint64_t n = h->size(), nw = (n + 31) / 32;
    std::shared_ptr<cph_filter> e(new cph_filter(), EffDeleter());
    e->device = h->device;
    e->n_bits = n;
    e->words.alloc(std::max<uint64_t>(nw, 1));
    h->d_rm_count.alloc(1);
    hipStream_t st = own_stream(h);
    live_filter(d_allow, h->d_removed.p, n, e->words.p, h->d_rm_count.p, st);
    unsigned long long c = 0;
    HIP_CHECK(hipMemcpyAsync(&c, h->d_rm_count.p, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    e->popcount = c;
    return e;
}

// After host.removed changed (a remove, a load, a build): the resident copy of R, a new epoch, the ~R filter.  The
// caller holds the mutex and has waited for the batches in flight.
void sync_removed(cph_index* h) {
    HostIndex& hi = h->host;
    h->rm_epoch = ++g_removed_epoch;            // (first: whatever fails below, no filter's cache of the old state is found again)
    h->live.reset();
    if (hi.n_removed == 0) {
        std::vector<uint32_t>().swap(hi.removed);
        h->d_removed.release();
        h->tombstones.store(false);
        return;
    }
    h->tombstones.store(true);                  // (before the device work: a failure must not bring the rows back;
                                                //  effective_filter makes `live` when it is missing)
    const uint64_t nw = (h->size() + 31) / 32;
    h->d_removed.alloc(nw);
    HIP_CHECK(hipMemcpy(h->d_removed.p, hi.removed.data(), nw * 4, hipMemcpyHostToDevice));
    h->live = make_live_filter(h, nullptr);
}

// The filter a search of this handle runs under: the caller's (null: none) on a handle without removed rows, else
// F & ~R -- for f == null the handle's ~R.  The caller holds the handle mutex and keeps the returned pointer until its
// batch is enqueued.
std::shared_ptr<const cph_filter> effective_filter(cph_index* h, const cph_filter* f) {
    if (h->host.n_removed == 0) return std::shared_ptr<const cph_filter>(std::shared_ptr<const cph_filter>(), f);   // (aliasing: owns nothing)
    if (!f) {
        if (!h->live) h->live = make_live_filter(h, nullptr);       // (only after a failed sync_removed)
        return h->live;
    }
    std::lock_guard<std::mutex> lk(f->eff_mu);
    for (auto& e : f->eff)
        if (e.first == h->rm_epoch) return e.second;
    if (f->eff.size() >= kEffCached) f->eff.erase(f->eff.begin());
    std::shared_ptr<cph_filter> e = make_live_filter(h, f->words.p);
    f->eff.emplace_back(h->rm_epoch, e);
    return e;
}

// The stored vector (dim floats) of internal id `id` < size: a base row from the host index, a tail row from its host copy.
const float* row_vec(const cph_index* h, uint64_t id) {
    return id < h->host.n ? h->host.vec(id) : h->tail_vecs.data() + (id - h->host.n) * h->dim;
}

void require_finalized(cph_index* h) {
    // the reference does not check (it would hit the invalid-entry RuntimeError or garbage,
    // api/hnsw_index.hpp:203-205); we raise that error up front
    if (!h->finalized) throw std::runtime_error("Search failed: invalid entry point after finalize.");
}

void release_scratch(BatchSet& s) {
    s.d_bitmaps.release(); s.d_logids.release(); s.d_beam.release(); s.d_beam_tail.release();
    s.r_bitmaps.release(); s.r_logids.release(); s.r_beam.release(); s.r_beam_tail.release();
    s.x_qpad.release(); s.x_qnorm.release(); s.x_pools.release(); s.x_counts.release();
    s.m_queries.release(); s.m_c.release();
    s.slots = 0; s.cap = 0; s.r_slots = 0;
}

// Waits (on the host) until nothing enqueued on this handle is running any more.
void quiesce(cph_index* h) {
    for (auto& s : h->sets)
        if (s.used && s.ev_done) HIP_CHECK(hipEventSynchronize(s.ev_done));
    for (auto& gs : h->rerank_scratch)           // (the re-rank pass runs behind its batch's ev_done)
        if (gs.rows.used) HIP_CHECK(hipEventSynchronize(gs.rows.ev));
}

// ---- pass timers (cph_debug_time_*, cph_debug_last_*_us) --------------------------------------------------------------------
constexpr const char* kNoTimedPass[kPassKinds] = {
    "no timed grouped search has run on this handle (cph_debug_time_grouped)",
    "no timed diverse search has run on this handle (cph_debug_time_diverse)",
    "no timed maxsim search has run on this handle (cph_debug_time_maxsim)",
    "no timed label pass has run on this handle (cph_debug_time_label_filters)",
    "no timed rescored maxsim search has run on this handle (cph_debug_time_maxsim_rescore)",
    "no timed rescored search has run on this handle (cph_debug_time_rescored)",
    "no timed fused search has run on this handle (cph_debug_time_fused)",
    "no timed tag pass has run on this handle (cph_debug_time_tag_filters)",
    "no timed facet pass has run on this handle (cph_debug_time_facets)",
    "this pass is not timed",
};

// pass(), which enqueues on `st`, between the timer's two events while it is on.
template <class Pass>
void timed_pass(cph_index::PassTimer& t, hipStream_t st, Pass pass) {
    t.timed = false;
    if (t.on) HIP_CHECK(hipEventRecord(t.ev0, st));
    pass();
    if (t.on) HIP_CHECK(hipEventRecord(t.ev1, st));
    t.timed = t.on;
}

// cph_debug_time_*.
void pass_timer_switch(cph_index* h, PassKind kind, bool on) {
    if (!h) throw InvalidArg("null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->use_device();
    cph_index::PassTimer& t = h->pass_timer[kind];
    if (on && !t.ev0) HIP_CHECK(hipEventCreate(&t.ev0));
    if (on && !t.ev1) HIP_CHECK(hipEventCreate(&t.ev1));
    t.on = on;
    t.timed = false;
}

// cph_debug_last_*_us: device time of the last timed pass in microseconds; waits for it.
void pass_timer_us(cph_index* h, PassKind kind, double* us) {
    if (!h || !us) throw InvalidArg("null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    cph_index::PassTimer& t = h->pass_timer[kind];
    if (!t.timed) throw InvalidArg(kNoTimedPass[kind]);
    h->use_device();
    HIP_CHECK(hipEventSynchronize(t.ev1));
    float ms = 0.0f;
    HIP_CHECK(hipEventElapsedTime(&ms, t.ev0, t.ev1));
    *us = (double)ms * 1e3;
}

// The big arrays of a loaded index: blocks repacked into the device layout, vectors, norms.  (An index
// built here already has them in HBM: build::build_graph.)
void upload_arrays(cph_index* h) {
    h->use_device();
    quiesce(h);
    const HostIndex& hi = h->host;
    h->L = make_dev_layout((uint32_t)hi.D, (uint32_t)hi.bw);
    const size_t n = hi.n;
    const size_t stride = h->L.stride;
    h->d_blocks.alloc(n * stride + 64);
    h->d_raw.alloc(n * hi.D);
    h->d_norm.alloc(n);
    // repack in chunks through a staging buffer
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(n, (256u << 20) / stride));
    std::vector<uint8_t> stage(chunk * stride);
    for (size_t base = 0; base < n; base += chunk) {
        const size_t cnt = std::min(chunk, n - base);
        parallel_for(cnt, 256, [&](size_t lo, size_t hi_) {
            for (size_t v = lo; v < hi_; ++v)
                repack_ref_to_dev(hi.nb(base + v), hi.RL, h->L, &stage[v * stride]);
        });
        HIP_CHECK(hipMemcpy(h->d_blocks.p + base * stride, stage.data(), cnt * stride,
                            hipMemcpyHostToDevice));
    }
    relayout_blocks(h->d_blocks.p, n, h->L, true);   // storage layout -> resident layout (cph_core.h, `nib`)
    HIP_CHECK(hipMemcpy(h->d_raw.p, hi.raw.data(), n * hi.D * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(h->d_norm.p, hi.norm_sq.data(), n * 4, hipMemcpyHostToDevice));
}

// Everything else the query path needs on the device: search constants, rotation signs, upper layers.
void upload_feeders(cph_index* h) {
    h->use_device();
    quiesce(h);
    const HostIndex& hi = h->host;
    const size_t n = hi.n;
    h->L = make_dev_layout((uint32_t)hi.D, (uint32_t)hi.bw);
    h->sc = hi.consts();
    h->flags = hi.has_dup_neighbors ? 1u : 0u;
    if (n != 0) {   // bit 1: short lists with a scalar tail (counted on the device: the blocks of a built index never visit the host)
        DevBuf<uint32_t> d_flag(1);
        HIP_CHECK(hipMemset(d_flag.p, 0, 4));
        hipLaunchKernelGGL(scan_counts_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, nullptr, h->d_blocks.p, (uint64_t)n,
                           h->L.stride, h->L.count_off, d_flag.p);
        HIP_CHECK(hipGetLastError());
        uint32_t f = 0;
        HIP_CHECK(hipMemcpy(&f, d_flag.p, 4, hipMemcpyDeviceToHost));
        h->flags |= f & 2u;
    }
    // rotation signs and the scale factors of the query encoder (rabitq_encoder.hpp:37-39)
    h->d_signs.alloc(3 * hi.D);
    HIP_CHECK(hipMemcpy(h->d_signs.p, hi.rot.signs.data(), 3 * hi.D * 4, hipMemcpyHostToDevice));
    const float d = static_cast<float>(hi.D);
    h->norm_factor = 1.0f / (d * std::sqrt(d));
    h->inv_sqrt_d = 1.0f / std::sqrt(d);
    // upper layers as CSR (edges are stored sorted by node id, api/hnsw_index.hpp:152)
    const int nl = std::min<int>({(int)hi.upper.size(), (int)hi.max_level, kMaxUpperLayers});
    h->dev_max_level = hi.max_level > 0 ? nl : 0;
    std::vector<uint32_t> flat;
    std::vector<size_t> off_nodes(nl), off_offs(nl), off_nbrs(nl);
    for (int l = 0; l < nl; ++l) {
        const auto& layer = hi.upper[l];
        off_nodes[l] = flat.size();
        for (const auto& e : layer) flat.push_back(e.node);
        off_offs[l] = flat.size();
        uint32_t acc = 0;
        for (const auto& e : layer) { flat.push_back(acc); acc += (uint32_t)e.nbrs.size(); }
        flat.push_back(acc);
        off_nbrs[l] = flat.size();
        for (const auto& e : layer) flat.insert(flat.end(), e.nbrs.begin(), e.nbrs.end());
    }
    h->d_upper.alloc(flat.size() + 1);
    if (!flat.empty())
        HIP_CHECK(hipMemcpy(h->d_upper.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
    for (int l = 0; l < kMaxUpperLayers; ++l) h->layers[l] = UpperLayerDev{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    // dense vertex -> row maps for the layers where a binary search would be a long chain of
    // dependent loads (4 B x n each), and next to each mapped layer's edges the map entry of every
    // neighbour (4 B per edge): a hop's edges then bring the next hop's row with them
    int mapped = 0;
    size_t mapped_edges = 0;
    for (int l = 0; l < nl; ++l) {
        if (hi.upper[l].size() <= 16) continue;
        ++mapped;
        for (const auto& e : hi.upper[l]) mapped_edges += e.nbrs.size();
    }
    h->d_row_of.alloc((size_t)mapped * n + 1);
    h->d_nbr_info.alloc(mapped_edges + 1);
    std::vector<uint32_t> row_of, nbr_info;
    size_t info_off = 0;
    for (int l = 0, m = 0; l < nl; ++l) {
        const uint32_t* dmap = nullptr;
        const uint32_t* dinfo = nullptr;
        if (hi.upper[l].size() > 16) {
            // vertex -> first edge | degree << 26 (the encoder then needs neither `nodes` nor `offsets`)
            row_of.assign(n, kInvalidNode);
            uint64_t first = 0;
            bool fits = true;
            for (size_t r = 0; r < hi.upper[l].size(); ++r) {
                const uint64_t deg = hi.upper[l][r].nbrs.size();
                if (first >= (1u << 26) || deg > 62) { fits = false; break; }
                row_of[hi.upper[l][r].node] = (uint32_t)first | ((uint32_t)deg << 26);
                first += deg;
            }
            if (!fits) { h->layers[l] = UpperLayerDev{h->d_upper.p + off_nodes[l], h->d_upper.p + off_offs[l], h->d_upper.p + off_nbrs[l], nullptr, nullptr, (uint32_t)hi.upper[l].size()}; ++m; continue; }
            HIP_CHECK(hipMemcpy(h->d_row_of.p + (size_t)m * n, row_of.data(), n * 4, hipMemcpyHostToDevice));
            dmap = h->d_row_of.p + (size_t)m * n;
            ++m;
            // (a neighbour outside the index or the layer ends the descent there, as its missing row_of entry did)
            nbr_info.clear();
            for (const auto& e : hi.upper[l])
                for (const uint32_t nb : e.nbrs) nbr_info.push_back(nb < n ? row_of[nb] : kInvalidNode);
            if (info_off + nbr_info.size() > mapped_edges) throw std::runtime_error("upper layers: edge count changed during upload");
            if (!nbr_info.empty())
                HIP_CHECK(hipMemcpy(h->d_nbr_info.p + info_off, nbr_info.data(), nbr_info.size() * 4, hipMemcpyHostToDevice));
            dinfo = h->d_nbr_info.p + info_off;
            info_off += nbr_info.size();
        }
        h->layers[l] = UpperLayerDev{h->d_upper.p + off_nodes[l], h->d_upper.p + off_offs[l],
                                     h->d_upper.p + off_nbrs[l], dmap, dinfo, (uint32_t)hi.upper[l].size()};
    }
    for (auto& s : h->sets) release_scratch(s);
    reset_adaptation(h);
}

// The reference-layout image of an index that came from a native file: own-code headers from the mapping,
// neighbour blocks re-derived from the device blocks.
void materialize_search_data(cph_index* h) {
    HostIndex& hi = h->host;
    if (!hi.search_data.empty() || hi.n == 0) return;
    h->use_device();
    quiesce(h);
    const size_t n = hi.n, stride = h->L.stride, own_stride = hi.RL.nb_off;
    hi.search_data.assign(n * hi.RL.vertex_bytes, 0);
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(n, (512u << 20) / stride));
    std::vector<uint8_t> stage(chunk * stride);
    for (size_t base = 0; base < n; base += chunk) {
        const size_t c = std::min(chunk, n - base);
        download_blocks(h->d_blocks.p + base * stride, c, h->L, stage.data());
        parallel_for(c, 256, [&](size_t lo, size_t hi_) {
            for (size_t v = lo; v < hi_; ++v) {
                uint8_t* dst = &hi.search_data[(base + v) * hi.RL.vertex_bytes];
                if (h->own_view) std::memcpy(dst, h->own_view + (base + v) * own_stride, own_stride);
                repack_dev_to_ref(&stage[v * stride], h->L, hi.RL, dst + hi.RL.nb_off);
            }
        });
    }
}

// Picks the set for the next batch (the two alternate) and makes `st` wait for the batch that
// used it before.  If that batch had to re-run queries, later batches get a larger capacity.
void init_set(BatchSet& s) {
    if (s.ev0) return;
    HIP_CHECK(hipEventCreate(&s.ev0));
    HIP_CHECK(hipEventCreate(&s.ev1));
    HIP_CHECK(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&s.pin_stats), kStatWords * 8, hipHostMallocDefault));
    std::memset(s.pin_stats, 0, kStatWords * 8);
}

BatchSet& next_set(cph_index* h, hipStream_t st) {
    h->last_set = (h->last_set + 1) % h->n_sets;
    BatchSet& s = h->sets[h->last_set];
    init_set(s);
    // (either set's finished batch counts: the other set's is the more recent one)
    for (BatchSet& o : h->sets) {
        if (!(o.used && o.ev_done && !o.stats_in_hbm && hipEventQuery(o.ev_done) == hipSuccess)) continue;
        // queries re-run, and those of them that were re-run for a stage-2 decision (probe first), not for capacity
        const uint64_t reruns = o.pin_stats[kStatReruns], stage2_reruns = stage2_stat(o, kStatStage2Reruns);
        if (reruns > stage2_reruns && o.cap < h->host.n + 1)
            h->auto_cap = std::max<uint64_t>(h->auto_cap, std::min<uint64_t>(h->host.n + 1, o.cap * 4));
        if (stage2_reruns * 50 > o.nq) h->pf_off = true;
        // Probe first pays when few of a block's neighbours are new (C2: 3.3 of 32 -- 40 % of the code lines are never
        // fetched); on a workload where most expansions find new neighbours in every group of eight it only adds a
        // dependent round trip (Gaussian 1M at 4 bits: 9.7 new per expansion, 13 % slower with it).  Decided from the
        // finished batches' own counters, with hysteresis; results are the same either way.
        // Narrow codes have less to skip (512 B / 1 KB of codes against 2 KB) and lose the estimator's overlap with the
        // probe: their break-even is lower (2-bit: +12 % at 1.5 new per expansion, -3.5 % at 5.3; 1-bit: +8 % at 1.0).
        if (o.pin_stats[kStatExpansions] >= 10000) {
            const double new_per_exp = (double)o.pin_stats[kStatNew] / (double)o.pin_stats[kStatExpansions];
            const double off = h->bits == 4 ? 6.0 : 2.8, on = h->bits == 4 ? 4.5 : 2.2;
            if (new_per_exp > off) h->pf_dense = true;
            else if (new_per_exp < on) h->pf_dense = false;
        }
    }
    if (s.used) HIP_CHECK(hipStreamWaitEvent(st, s.ev_done, 0));
    return s;
}

// Encode the queries on the device (rotation, 4-bit scalars -> masks, coefficients) and run the
// upper-layer descent; d_raw_q = [nq][dim] raw queries already in HBM.
void stage_queries(cph_index* h, BatchSet& s, const float* d_raw_q, uint64_t nq, hipStream_t st) {
    const HostIndex& hi = h->host;
    const uint32_t D = (uint32_t)hi.D, PW = h->L.PW;
    if (hi.entry == kInvalidNode || hi.entry >= hi.n)
        throw std::runtime_error("Search failed: invalid entry point after finalize.");
    if (s.d_queries.n < nq * D || s.d_qmasks.n < nq * PW || s.d_qhdr.n < nq) {
        if (s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));   // growing: the old buffers must be idle
        s.d_queries.alloc(nq * D);
        s.d_qmasks.alloc(nq * PW);
        s.d_qhdr.alloc(nq);
        s.d_entry_dist.alloc(nq);
        s.d_order.alloc(nq);
    }
    EncodeArgs a{};
    a.queries_raw = d_raw_q;
    a.nq = (uint32_t)nq;
    a.dim = (uint32_t)hi.dim;
    a.D = D;
    a.PW = PW;
    a.signs = h->d_signs.p;
    a.norm_factor = h->norm_factor;
    a.inv_sqrt_d = h->inv_sqrt_d;
    a.raw = h->d_raw.p;
    a.n = hi.n;
    a.entry = hi.entry;
    a.max_level = h->dev_max_level;
    for (int l = 0; l < kMaxUpperLayers; ++l) a.layers[l] = h->layers[l];
    a.queries_padded = s.d_queries.p;
    a.qmasks = s.d_qmasks.p;
    a.qhdr = s.d_qhdr.p;
    a.entry_dist = s.d_entry_dist.p;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(nq, (uint64_t)h->num_cus * 32);
    hipLaunchKernelGGL(encode_kernel, dim3(grid), dim3(64), encode_lds_bytes(D), st, a);
    HIP_CHECK(hipGetLastError());
}

// host queries -> the set's staging buffer.  A batch's queries have the caller's width; the hooks, which hand their
// vector straight to the encoder, give one of the stored width (stored: the two differ under the inner product only).
const float* upload_queries(cph_index* h, BatchSet& s, const float* queries, uint64_t nq, hipStream_t st, bool stored = false) {
    const uint64_t width = stored ? h->dim : h->dim_in;
    if (s.d_queries_raw.n < nq * width) {
        if (s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));
        s.d_queries_raw.alloc(nq * width);
    }
    HIP_CHECK(hipMemcpyAsync(s.d_queries_raw.p, queries, nq * width * 4, hipMemcpyHostToDevice, st));
    return s.d_queries_raw.p;
}

// The queries a batch's kernels read: d_raw_q itself under L2 (no launch, no allocation, no event); under cosine the
// rows normalised to squared norm 1/2 (device_normalize.h) into the set's buffer, on the batch's stream.  Called once per
// batch, before the first reader of the raw queries; d_raw_q may be pinned host memory (the copy-free routes).  A bad
// query (zero, NaN, Inf) searches as the zero vector: the enqueue-only device form cannot refuse, so no form does.
const float* metric_queries(cph_index* h, BatchSet& s, const float* d_raw_q, uint64_t nq, hipStream_t st) {
    if (h->metric == CPH_METRIC_L2 || !d_raw_q || nq == 0) return d_raw_q;
    if (s.m_queries.n < nq * h->dim || (h->metric == CPH_METRIC_IP && s.m_c.n < nq)) {
        if (s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));   // growing: the old buffers must be idle
        s.m_queries.alloc(nq * h->dim);
        if (h->metric == CPH_METRIC_IP) s.m_c.alloc(nq);
    }
    if (h->metric == CPH_METRIC_IP) {
        // [q, 0] at the stored width, and c = |q|^2 + M2 for the batch's epilogue (metric_scores)
        ip_augment(d_raw_q, s.m_queries.p, nq, (uint32_t)h->dim_in, h->ip_m2, 0, s.m_c.p, nullptr, st);
        ++h->metric_launches;
        return s.m_queries.p;
    }
    normalize_rows(d_raw_q, s.m_queries.p, nq, (uint32_t)h->dim, (uint32_t)h->dim, (uint32_t)h->dim, nullptr, nullptr, st);
    ++h->metric_launches;
    return s.m_queries.p;
}

// The scores of an inner-product batch: dist = 0.5 * (dist - c) wherever the id is not padding (device_ip.h), enqueued on
// the batch's stream behind the last kernel that writes the result rows -- once per batch, on every route of
// search_batch_locked; the tables may be device memory or the pinned buffer of the copy-free route.  The set's
// completion event moves behind it: the next batch on this set may grow m_c.  Nothing under L2 and cosine.
void metric_scores(cph_index* h, BatchSet& s, int64_t* d_ids, float* d_dist, uint64_t nq, uint64_t k, hipStream_t st) {
    if (h->metric != CPH_METRIC_IP || nq == 0 || k == 0) return;
    ip_epilogue(d_ids, d_dist, nq, (uint32_t)k, s.m_c.p, st);
    ++h->metric_launches;
    HIP_CHECK(hipEventRecord(s.ev_done, st));
}

// Rows on their way into an inner-product index, on the device, in chunks: `out` ([n][dim_in + 1], host) holds
// [x, sqrt(M2 - |x|^2)].  bound == null: M2 is the largest squared norm of these rows, found by a pass over all of them
// (which also rejects bad rows) before the pass that writes; otherwise M2 = *bound and a row above it is refused.
// Returns M2.  A refusal leaves the handle as it was.  against_index: the bound is the M2 of the index the rows are
// added to (cph_add), which changes what the caller is told.
float ip_rows_in(cph_index* h, const float* vectors, uint64_t n, const float* bound, bool against_index, std::vector<float>& out) {
    h->use_device();
    const uint64_t dim = h->dim_in, sd = dim + 1;
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(n, ((uint64_t)256 << 20) / (sd * 4)));
    out.resize(n * sd);
    DevBuf<float> d_x(chunk * dim), d_o(chunk * sd);
    DevBuf<unsigned long long> d_cnt(3);
    DevBuf<unsigned int> d_m2(1);
    const unsigned long long init[3] = {0ull, 0ull, kIpNoRow};
    unsigned long long cnt[3] = {0ull, 0ull, kIpNoRow};
    hipStream_t st = own_stream(h);
    auto refuse = [&](const char* why) {
        const unsigned long long total = cnt[0] + cnt[1];
        throw InvalidArg("inner-product metric: row " + std::to_string(cnt[2]) + " " + why + " (" + std::to_string(total) + " such row" +
                         (total == 1 ? "" : "s") + " in this call): nothing was changed");
    };
    HIP_CHECK(hipMemcpyAsync(d_cnt.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    float m2 = bound ? *bound : 0.0f;
    const bool one_chunk = chunk >= n;
    if (!bound) {
        HIP_CHECK(hipMemsetAsync(d_m2.p, 0, 4, st));
        for (uint64_t base = 0; base < n; base += chunk) {
            const uint64_t c = std::min(chunk, n - base);
            HIP_CHECK(hipMemcpyAsync(d_x.p, vectors + base * dim, c * dim * 4, hipMemcpyHostToDevice, st));
            ip_max(d_x.p, c, (uint32_t)dim, base, d_m2.p, d_cnt.p, st);
            ++h->metric_launches;
            HIP_CHECK(hipStreamSynchronize(st));     // (the next chunk's upload overwrites d_x from pageable memory)
        }
        HIP_CHECK(hipMemcpyAsync(&m2, d_m2.p, 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (cnt[0]) refuse("holds a NaN or an Inf, or its squared norm overflows");
    }
    for (uint64_t base = 0; base < n; base += chunk) {
        const uint64_t c = std::min(chunk, n - base);
        if (bound || !one_chunk) HIP_CHECK(hipMemcpyAsync(d_x.p, vectors + base * dim, c * dim * 4, hipMemcpyHostToDevice, st));
        ip_augment(d_x.p, d_o.p, c, (uint32_t)dim, m2, base, nullptr, d_cnt.p, st);
        ++h->metric_launches;
        HIP_CHECK(hipMemcpyAsync(out.data() + base * sd, d_o.p, c * sd * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (cnt[0] + cnt[1]) {
        const std::string b = std::to_string(m2);
        if (cnt[0] && cnt[1]) refuse(("holds a NaN or an Inf, has an overflowing squared norm, or one above the bound " + b).c_str());
        if (cnt[0]) refuse("holds a NaN or an Inf, or its squared norm overflows");
        refuse(against_index ? ("has a squared norm above the bound " + b + " the index was built with: rebuild the index with a larger bound (max_norm)").c_str()
                             : ("has a squared norm above the bound " + b + " given for this index").c_str());
    }
    return m2;
}

// Rows on their way into a cosine index (cph_build, cph_add): normalised on the device, in chunks, into `out` ([n][dim],
// host).  A bad row refuses the call -- nothing of the handle has changed by then; row_base: the number of vectors[0] in
// the caller's numbering (a partitioned index reports global rows).
void normalize_rows_in(cph_index* h, const float* vectors, uint64_t n, uint64_t row_base, std::vector<float>& out) {
    h->use_device();
    const uint64_t dim = h->dim, chunk = std::max<uint64_t>(1, std::min<uint64_t>(n, ((uint64_t)256 << 20) / (dim * 4)));
    out.resize(n * dim);
    DevBuf<float> d_x(chunk * dim);
    DevBuf<unsigned long long> d_bad(2);
    const unsigned long long init[2] = {0ull, kNoBadRow};
    unsigned long long bad[2] = {0ull, kNoBadRow}, total = 0, first = kNoBadRow;
    hipStream_t st = own_stream(h);
    for (uint64_t base = 0; base < n; base += chunk) {
        const uint64_t c = std::min(chunk, n - base);
        HIP_CHECK(hipMemcpyAsync(d_bad.p, init, 16, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(d_x.p, vectors + base * dim, c * dim * 4, hipMemcpyHostToDevice, st));
        normalize_rows(d_x.p, d_x.p, c, (uint32_t)dim, (uint32_t)dim, (uint32_t)dim, d_bad.p, d_bad.p + 1, st);
        ++h->metric_launches;
        HIP_CHECK(hipMemcpyAsync(out.data() + base * dim, d_x.p, c * dim * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(bad, d_bad.p, 16, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        if (bad[0] && first == kNoBadRow) first = row_base + base + bad[1];
        total += bad[0];
    }
    if (total)
        throw InvalidArg("cosine metric: row " + std::to_string(first) + " has no direction (a zero row, NaN, Inf or an overflowing norm; " +
                         std::to_string(total) + " such row" + (total == 1 ? "" : "s") + " in this call): nothing was changed");
}

// (Re)allocates the per-slot scratch of a set; the set must be idle.
void ensure_scratch(cph_index* h, BatchSet& s, uint32_t slots, uint64_t cap, hipStream_t st) {
    const uint64_t n = h->host.n;
    const uint64_t bm_words = (n + 31) / 32;
    if (!(s.slots >= slots && s.cap == cap)) {
        if (s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));
        s.d_bitmaps.alloc((size_t)slots * bm_words);
        HIP_CHECK(hipMemsetAsync(s.d_bitmaps.p, 0, (size_t)slots * bm_words * 4, st));
        s.d_logids.alloc((size_t)slots * cap);
        s.d_beam.alloc((size_t)slots * kBeamPagesDwords);
        s.d_beam_tail.alloc((size_t)slots * beam_tail_dwords(cap));
        s.slots = slots;
        s.cap = cap;
    }
    // the re-run launch (capacity overflows; stage-2 decisions of the probe-first instantiation) needs room for every
    // vertex: a few full-capacity slots
    if ((cap < n + 1 || probe_first(h)) && s.r_slots == 0) {
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        const uint64_t per = (n + 1) * 4 + ((uint64_t)kBeamPagesDwords + beam_tail_dwords(n + 1)) * 4 + bm_words * 4;
        // (a leader slot's private set answers at most kLeaderGroup callers per launch)
        const uint64_t want = (&s - h->sets) >= kMaxBatchSets ? kLeaderGroup : kSmallBatch;
        const uint32_t rs = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)(free_b * 0.25) / per));
        s.r_bitmaps.alloc((size_t)rs * bm_words);
        HIP_CHECK(hipMemsetAsync(s.r_bitmaps.p, 0, (size_t)rs * bm_words * 4, st));
        s.r_logids.alloc((size_t)rs * (n + 1));
        s.r_beam.alloc((size_t)rs * kBeamPagesDwords);
        s.r_beam_tail.alloc((size_t)rs * beam_tail_dwords(n + 1));
        s.r_slots = rs;
    }
}

struct DoneFlags {          // per-query completion flags in pinned host memory (coalesced cph_search), or none
    uint32_t* flags = nullptr;
    uint32_t seq = 0;
};

// The launches of a batch (launch_search).
enum class Launch {
    Main,     // the batch on the set's slots (capacity s.cap); the only launch that may probe first
    Rerun,    // behind Main, on the full-capacity slots: the queries Main handed over (their list lives on the device)
    Direct,   // a batch small enough for the full-capacity slots, run there at once: nothing can overflow, no re-run
};

// The one table of search_kernel instantiations (33) and the only place that names them.
//   filtered (a filtered batch never probes first)          <BW, D or 0, false, true>
//   filtered, every query under its own filter              <BW, D or 0, false, true, true>
//   unfiltered, static D (128, 1024), probe first           <BW, D, true, false>      Launch::Main while probe_first(h)
//   unfiltered, static D, no probe first                    <BW, D, false, false>     re-run, direct, probe first off
//   unfiltered, any other D                                 <BW, 0, true, false>
// Without probe first the codes are fetched with the ids: no third dependent round trip for a handful of queries
// (latency, not traffic); it takes the stage-2 decisions the probe-first launch hands over, evaluates the scalar tails
// of short neighbour lists (flags bit 1) and serves the workloads on which probe first does not pay.
// The last row has no <BW, 0, false, false> twin: probe first exists for SD >= 128 only (device_search.h: kProbeFirst,
// kStaticLayout), so with SD = 0 the PF argument is inert and both values would be the same kernel compiled twice.
void launch_search_kernel(uint32_t bits, uint32_t D, bool pf, bool filtered, bool table_of_filters, uint32_t grid, size_t lds,
                          hipStream_t st, const SearchArgs& a) {
    using Kernel = void (*)(SearchArgs);
    // [bits 1, 2, 4][D other, 128, 1024][no probe first, probe first, filtered, filter table]
    static const Kernel table[3][3][4] = {
        {{search_kernel<1, 0, true, false>, search_kernel<1, 0, true, false>, search_kernel<1, 0, false, true>,
          search_kernel<1, 0, false, true, true>},
         {search_kernel<1, 128, false, false>, search_kernel<1, 128, true, false>, search_kernel<1, 128, false, true>,
          search_kernel<1, 128, false, true, true>},
         {search_kernel<1, 1024, false, false>, search_kernel<1, 1024, true, false>, search_kernel<1, 1024, false, true>,
          search_kernel<1, 1024, false, true, true>}},
        {{search_kernel<2, 0, true, false>, search_kernel<2, 0, true, false>, search_kernel<2, 0, false, true>,
          search_kernel<2, 0, false, true, true>},
         {search_kernel<2, 128, false, false>, search_kernel<2, 128, true, false>, search_kernel<2, 128, false, true>,
          search_kernel<2, 128, false, true, true>},
         {search_kernel<2, 1024, false, false>, search_kernel<2, 1024, true, false>, search_kernel<2, 1024, false, true>,
          search_kernel<2, 1024, false, true, true>}},
        {{search_kernel<4, 0, true, false>, search_kernel<4, 0, true, false>, search_kernel<4, 0, false, true>,
          search_kernel<4, 0, false, true, true>},
         {search_kernel<4, 128, false, false>, search_kernel<4, 128, true, false>, search_kernel<4, 128, false, true>,
          search_kernel<4, 128, false, true, true>},
         {search_kernel<4, 1024, false, false>, search_kernel<4, 1024, true, false>, search_kernel<4, 1024, false, true>,
          search_kernel<4, 1024, false, true, true>}},
    };
    const Kernel kernel = table[bits == 1 ? 0 : bits == 2 ? 1 : 2][D == 128 ? 1 : D == 1024 ? 2 : 0][table_of_filters ? 3 : filtered ? 2 : pf ? 1 : 0];
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, st, a);
    HIP_CHECK(hipGetLastError());
}

// One of the two pairs of graph launches of a batch with per-query filters (enqueue_filters): its queries, its three
// queue words and its re-run list; the filtered pair also names the tables of SearchArgs.
struct SubBatch {
    const uint32_t* todo = nullptr;                  // the pair's queries (null: all nq, in order)
    int queue = 0;                                   // first of its StatQueueWords
    uint32_t* redo = nullptr;
    const uint32_t* const* allow_tab = nullptr;
    const uint32_t* filter_of = nullptr;
};

// d_allow: the allowed-id bitmap of a filtered batch (cph_filter::words), or null.  sub: the launch belongs to a batch
// with per-query filters -- nq counts sub->todo.
void launch_search(cph_index* h, BatchSet& s, uint32_t nq, uint32_t k, int64_t* d_ids, float* d_dist, uint32_t* d_count,
                   const uint32_t* d_todo, Launch mode, hipStream_t st, DoneFlags done = DoneFlags(),
                   const uint32_t* d_allow = nullptr, const SubBatch* sub = nullptr) {
    const uint64_t n = h->host.n;
    const bool tab = sub && sub->allow_tab;
    const bool pf = mode == Launch::Main && d_allow == nullptr && !tab && probe_first(h);
    SearchArgs a{};
    a.allow = d_allow;
    if (tab) { a.allow_tab = sub->allow_tab; a.filter_of = sub->filter_of; }
    a.rows = h->ids_input ? h->d_rows.p : nullptr;
    a.done_flags = done.flags;
    a.done_seq = done.seq;
    a.blocks = h->d_blocks.p;
    a.raw = h->d_raw.p;
    a.norm_sq = h->d_norm.p;
    a.n = n;
    a.L = h->L;
    a.flags = h->flags;
    a.queries = s.d_queries.p;
    a.qmasks = s.d_qmasks.p;
    a.qhdr = s.d_qhdr.p;
    a.k = k;
    a.sc = h->sc;
    a.bm_words = (n + 31) / 32;
    a.out_ids = d_ids;
    a.out_dist = d_dist;
    a.out_count = d_count;
    a.status = s.d_status.p;
    a.stats = s.d_stats.p;
    if (mode == Launch::Main) {     // the set's own slots ...
        a.cap = s.cap;
        a.bitmaps = s.d_bitmaps.p;
        a.beam_pages = s.d_beam.p;
        a.beam_tail = s.d_beam_tail.p;
        a.log_ids = s.d_logids.p;
    } else {                        // ... or its full-capacity ones
        a.cap = n + 1;
        a.bitmaps = s.r_bitmaps.p;
        a.beam_pages = s.r_beam.p;
        a.beam_tail = s.r_beam_tail.p;
        a.log_ids = s.r_logids.p;
    }
    uint32_t* queue = reinterpret_cast<uint32_t*>(s.d_stats.p + kStatQueues) + (sub ? sub->queue : 0);   // StatQueueWord
    uint32_t* const d_redo = sub ? sub->redo : s.d_redo.p;
    uint32_t grid = 0;
    switch (mode) {
    case Launch::Main:
        a.todo = d_todo;
        a.nq = nq;
        a.counter = queue + kQueueMain;
        a.redo = (s.cap < n + 1 || pf) ? d_redo : nullptr;
        a.redo_count = queue + kQueueRerunLen;
        grid = std::min(s.run_slots, nq);
        break;
    case Launch::Rerun:
        a.todo = d_redo;
        a.nq_dev = queue + kQueueRerunLen;
        a.counter = queue + kQueueRerun;
        grid = s.r_slots;
        break;
    case Launch::Direct:
        a.todo = d_todo;
        a.nq = nq;
        a.counter = queue + kQueueMain;
        grid = nq;
        break;
    }
    const size_t lds = search_lds_bytes(h->L.D, h->L.PW, k);
    if (lds > 160 * 1024) throw InvalidArg("k too large for the on-chip result heap");
    launch_search_kernel(h->bits, h->L.D, pf, d_allow != nullptr, tab, grid, lds, st, a);
}

// Statistics block to pinned memory, completion event, bookkeeping: the tail of every enqueued batch.
void finish_batch(cph_index* h, BatchSet& s, hipStream_t st) {
    HIP_CHECK(hipEventRecord(s.ev1, st));
    // the statistics block lands in pinned host memory; it is only read when somebody asks.  (The private sets of the
    // cph_search leader slots leave it in HBM until then: their callers wait for the stream, and the copy command would
    // sit on that path -- nothing of theirs can overflow, so nobody reads the block unasked.)
    s.stats_in_hbm = (&s - h->sets) >= kMaxBatchSets;
    if (!s.stats_in_hbm) HIP_CHECK(hipMemcpyAsync(s.pin_stats, s.d_stats.p, kStatWords * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(s.ev_done, st));
    s.used = true;
    h->last_search = (int)(&s - h->sets);
    h->last_range = false;
}

// The slots and the per-slot capacity of a graph launch over nq queries (s.run_slots, s.run_cap; the set's scratch is
// (re)allocated to match); returns whether the launch order is closest-entry-first.
bool size_search(cph_index* h, BatchSet& s, uint32_t nq, uint32_t k, hipStream_t st) {
    const uint64_t n = h->host.n;
    // resident query slots: one wave each
    uint32_t wpc = h->waves_per_cu;
    if (!h->waves_from_env) {
        // registers (launch bounds of the instantiation) and LDS (160 KB per CU) both cap the resident waves
        wpc = 4 * (uint32_t)search_waves_per_simd(search_static_d(h->L.D) ? (int)h->L.D : 0, (int)h->bits);
        const size_t lds_wave = search_lds_bytes(h->L.D, h->L.PW, k);
        wpc = (uint32_t)std::max<size_t>(1, std::min<size_t>(wpc, (160u * 1024u) / lds_wave));
    }
    uint32_t max_slots = h->want_slots ? h->want_slots : (uint32_t)h->num_cus * wpc;
    // More than two sets in rotation: a batch gets exactly half of the resident slots, so that two batches run side by
    // side at full occupancy while the others queue behind them -- the drain of one is filled by the start of the
    // next-but-one (C2, 10k-query batches on four streams: 5.34 -> 5.61 M QPS; 2,560 / 3,584 / 4,096 slots per batch or
    // three sets all lose against two sets with every slot, profiles/r3_streams_sweep.md)
    if (!h->want_slots && h->n_sets > 2) max_slots = std::max<uint32_t>(64, max_slots / 2);
    // balanced rounds: every slot runs the same number of queries (10k queries on 4096 slots
    // would leave 56% of the slots idle during the third round)
    const uint32_t rounds = (nq + max_slots - 1) / max_slots;
    uint32_t slots = std::min<uint32_t>(nq, (nq + rounds - 1) / rounds);
    // ... unless the batch is launched longest-first (below): then every slot is worth having, the
    // short queries at the end of the order fill the gaps
    const bool ordered = h->dev_max_level > 0 && h->order_queries;
    if (ordered) {
        slots = std::min<uint32_t>(nq, max_slots);
        // A batch that fills more than half of the slots gains from a short queue: the order starts with the longest
        // queries, the last eighth -- the shortest -- fills the gaps they leave (C2, 6,144 slots: 4,000 queries
        // 1.37 -> 1.31 ms, 6,000 queries 1.65 -> 1.61 ms; below 3,000 queries all resident is 0-7 % faster;
        // scripts/slot_fraction_sweep.py, profiles/r2_slot_fraction.md)
        if (!h->want_slots && nq > max_slots / 2) slots = std::min<uint32_t>(max_slots, nq - nq / 8);
    }
    const uint64_t bm_bytes = ((n + 31) / 32) * 4;
    uint64_t cap = h->want_cap ? h->want_cap : std::max<uint64_t>(h->auto_cap, std::min<uint64_t>(n + 1, 1u << 16));
    cap = std::max<uint64_t>(64, std::min<uint64_t>(cap, n + 1));
    if (!(s.slots >= slots && s.cap == cap)) {
        // budget: at most 30% of what is free (plus what this set already holds) -- there are two sets
        size_t free_b = 0, total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        auto slot_bytes = [&](uint64_t c) { return c * 4 + ((uint64_t)kBeamPagesDwords + beam_tail_dwords(c)) * 4 + bm_bytes; };   // id log + beam spill + bitmap
        const uint64_t held = (uint64_t)s.slots * slot_bytes(s.cap);
        const uint64_t budget = (uint64_t)((free_b + held) * 0.3);
        while (slots > 64 && (uint64_t)slots * slot_bytes(cap) > budget) slots /= 2;
        while (cap > 4096 && (uint64_t)slots * slot_bytes(cap) > budget) cap /= 2;
    }
    ensure_scratch(h, s, slots, cap, st);
    slots = std::min(slots, s.slots);
    s.run_slots = slots;
    s.run_cap = s.cap;
    return ordered;
}

// ---- what the scans share on the host (device_exact.h) ----------------------------------------------------------------------
// Enqueues the pad pass of a scan: qpad[nq_pad][D] and qnorm[nq_pad] from the nq raw queries at d_q (d_perm, or null:
// exact_pad_rows), and n_exact, the batch's evaluation count, STORED into the statistics.
void pad_queries(const cph_index* h, const float* d_q, const uint32_t* d_perm, uint32_t nq, uint32_t nq_pad, float* qpad, float* qnorm,
                 unsigned long long* d_stats, unsigned long long n_exact, hipStream_t st) {
    const dim3 grid(std::min<uint32_t>(nq_pad, (uint32_t)h->num_cus * 16));
    if (d_perm) hipLaunchKernelGGL(exact_pad_groups_kernel, grid, dim3(64), 0, st, d_q, d_perm, nq, nq_pad, (uint32_t)h->dim, h->L.D, qpad, qnorm, d_stats, n_exact);
    else hipLaunchKernelGGL(exact_pad_kernel, grid, dim3(64), 0, st, d_q, nq, nq_pad, (uint32_t)h->dim, h->L.D, qpad, qnorm, d_stats, n_exact);
    HIP_CHECK(hipGetLastError());
}

// The fields every scan kernel's arguments share; q_first / q_count are set per launch.  part: 0 where the kernel's work
// items state the cut (the grouped scan).
ScanCommon scan_common(const cph_index* h, const float* qpad, const float* qnorm, uint32_t gq, uint32_t part) {
    ScanCommon s{};
    s.raw = h->d_raw.p;
    s.norm_sq = h->d_norm.p;
    s.qpad = qpad;
    s.qnorm = qnorm;
    s.D = h->L.D;
    s.gq = gq;
    s.part = part;
    return s;
}

// ---- the tail of a graph-routed batch (device_tail.h) ---------------------------------------------------------------------
// What every graph-routed entry refuses on a handle with a tail, before it touches the device.
void require_tail_k(const cph_index* h, uint64_t k) {
    if (h->tail && k > kExactMaxK)
        throw InvalidArg("the index holds " + std::to_string(h->tail) + " added rows, which a search scans exactly: k <= " +
                         std::to_string(kExactMaxK) + " (got k = " + std::to_string(k) + "); compact() the index first");
}

// First half, enqueued BEFORE the graph launch: the batch's padded queries and their norms (d_raw_q: [nq][dim] raw
// queries the device can read).  exact_pad_kernel STORES the scan's evaluation count -- every tail row against every
// query -- into the statistics word the graph launch then ADDS its own to.
ExactPlan tail_begin(cph_index* h, BatchSet& s, const float* d_raw_q, uint32_t nq, uint32_t k, hipStream_t st) {
    const uint32_t D = h->L.D;
    const uint32_t nq_pad = (nq + kExactQT - 1) / kExactQT * kExactQT;
    const ExactPlan pl = plan_exact(h->tail, nq, k, h->num_cus, h->exact_scratch_bytes);
    if (s.x_qpad.n < (size_t)nq_pad * D || s.x_qnorm.n < nq_pad || s.x_pools.n < pl.pool_keys || s.x_counts.n < (size_t)pl.P * pl.tile_q) {
        if (s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));   // growing: the old buffers must be idle
        s.x_qpad.alloc((size_t)nq_pad * D);
        s.x_qnorm.alloc(nq_pad);
        s.x_pools.alloc(pl.pool_keys);
        s.x_counts.alloc((size_t)pl.P * pl.tile_q);
    }
    pad_queries(h, d_raw_q, nullptr, nq, nq_pad, s.x_qpad.p, s.x_qnorm.p, s.d_stats.p, (unsigned long long)nq * h->tail, st);
    return pl;
}

// Second half, behind the graph launches: scan the tail under the batch's effective filter (d_allow null: every id) and
// fold the lists into the graph's rows, in place.  Nothing waits for the device.
void tail_finish(cph_index* h, BatchSet& s, const ExactPlan& pl, uint32_t nq, uint32_t k, const uint32_t* d_allow, int64_t* d_ids,
                 float* d_dist, uint32_t* d_count, DoneFlags done, hipStream_t st) {
    TailScanArgs a{};
    a.s = scan_common(h, s.x_qpad.p, s.x_qnorm.p, pl.gq, pl.part);
    a.allow = d_allow;
    a.base = (uint32_t)h->host.n;
    a.t = (uint32_t)h->tail;
    a.k = k;
    a.C = pl.C;
    a.pools = s.x_pools.p;
    a.counts = s.x_counts.p;
    TailFoldArgs f{};
    f.pools = s.x_pools.p;
    f.counts = s.x_counts.p;
    f.P = pl.P;
    f.k = k;
    f.C = pl.C;
    f.ids = d_ids;
    f.dist = d_dist;
    f.out_count = d_count;
    f.done_flags = done.flags;
    f.done_seq = done.seq;
    for (uint32_t q0 = 0; q0 < nq; q0 += pl.tile_q) {
        a.s.q_first = f.q_first = q0;
        a.s.q_count = f.q_count = std::min(pl.tile_q, nq - q0);
        CPH_LAUNCH_SCAN(tail_scan_kernel, a.s.D, dim3(pl.P, (f.q_count + pl.gq - 1) / pl.gq), (size_t)pl.C * 8 + (size_t)pl.gq * 8, st, a);
        tail_fold(f, st);
    }
}

// Core: queries already staged in the set; results into device buffers.  Everything is enqueued on
// `st` and nothing waits for the device: a query that outgrows its scratch is answered by the
// full-capacity re-run launch that always follows the main one (it finds an empty list otherwise).
// `filter` (null: unfiltered) restricts the result heap to its allowed ids; with no id allowed nothing is launched.
// On a handle with a tail the graph launches are the ones a handle without it makes; around them the tail's scan and
// fold (tail_begin / tail_finish), which need d_raw_q, the batch's raw queries.
void enqueue_search(cph_index* h, BatchSet& s, uint32_t nq, uint32_t k, int64_t* d_ids, float* d_dist,
                    hipStream_t st, uint32_t* d_count_out = nullptr, DoneFlags done = DoneFlags(),
                    const cph_filter* filter = nullptr, const float* d_raw_q = nullptr) {
    const uint64_t n = h->host.n;
    if (s.d_count.n < nq) {
        if (s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));
        s.d_count.alloc(nq);
        s.d_status.alloc(nq);
        s.d_redo.alloc(nq);
    }
    s.d_stats.alloc(kStatWords);
    HIP_CHECK(hipMemsetAsync(s.d_stats.p, 0, kStatWords * 8, st));
    if (filter && filter->popcount == 0) {
        // nothing can enter a result heap: every row is padding (-1 / FLT_MAX), no query expands anything -- the search
        // would have walked each query's whole connected component to find that out
        uint32_t* d_count = d_count_out ? d_count_out : s.d_count.p;
        HIP_CHECK(hipEventRecord(s.ev0, st));
        HIP_CHECK(hipMemsetAsync(d_ids, 0xFF, (size_t)nq * k * 8, st));
        HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_dist), (int)0x7F7FFFFF, (size_t)nq * k, st));
        HIP_CHECK(hipMemsetAsync(d_count, 0, (size_t)nq * 4, st));
        HIP_CHECK(hipMemsetAsync(s.d_status.p, 0, (size_t)nq * 4, st));
        s.run_slots = 0;
        s.run_cap = 0;
        s.nq = nq;
        finish_batch(h, s, st);
        return;
    }
    const uint32_t* d_allow = filter ? filter->words.p : nullptr;
    const bool ordered = size_search(h, s, nq, k, st);
    const uint32_t slots = s.run_slots;
    s.nq = nq;
    // closest-entry-first launch order (device_encode.h) when the batch outnumbers the slots
    const uint32_t* d_order = nullptr;
    if (nq > slots && ordered) {
        hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, st, s.d_entry_dist.p, nq, s.d_order.p);
        HIP_CHECK(hipGetLastError());
        d_order = s.d_order.p;
    }
    uint32_t* d_count = d_count_out ? d_count_out : s.d_count.p;
    HIP_CHECK(hipEventRecord(s.ev0, st));
    const bool tail = h->tail != 0;
    ExactPlan tail_plan{};
    if (tail) {
        if (!d_raw_q) throw std::runtime_error("a search of an index with added rows needs the raw queries");
        tail_plan = tail_begin(h, s, d_raw_q, nq, k, st);
    }
    const DoneFlags graph_done = tail ? DoneFlags() : done;      // (with a tail a row is final only after the fold)
    // (a filtered batch does not probe first: its re-run launch exists for capacity overflows only)
    const bool rerun = s.cap < n + 1 || (d_allow == nullptr && probe_first(h));
    if (rerun && nq <= s.r_slots && !h->want_cap && !h->want_slots) {   // (explicit search params keep the general path)
        // a handful of queries: straight onto the full-capacity slots -- one launch, nothing can overflow
        s.run_slots = nq;
        s.run_cap = n + 1;
        launch_search(h, s, nq, k, d_ids, d_dist, d_count, nullptr, Launch::Direct, st, graph_done, d_allow);
    } else {
        launch_search(h, s, nq, k, d_ids, d_dist, d_count, d_order, Launch::Main, st, graph_done, d_allow);
        if (rerun) launch_search(h, s, nq, k, d_ids, d_dist, d_count, nullptr, Launch::Rerun, st, graph_done, d_allow);
    }
    if (tail) tail_finish(h, s, tail_plan, nq, k, d_allow, d_ids, d_dist, d_count, done, st);
    finish_batch(h, s, st);
}

hipStream_t own_stream(cph_index* h) {
    if (!h->own_stream) HIP_CHECK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    return h->own_stream;
}

// A batch of `n` queries in a pinned, device-mapped host buffer, read and written by the kernels over PCIe:
// [prefix | ids n*k*8 | dist n*k*4 | counts n*4 | pad to 16 | queries n*dim*4].  prefix: 0 for a batch set's buffer,
// kFlagBytes (the per-query completion flags) for a leader slot's.  The accessors take the buffer's host or device address.
constexpr size_t kFlagBytes = kLeaderGroup * 4;
struct PinnedIo {
    size_t o_ids, o_dist, o_cnt, o_q, need;
    PinnedIo(uint64_t n, uint64_t k, uint64_t dim, size_t prefix) {
        o_ids = prefix;
        o_dist = o_ids + n * k * 8;
        o_cnt = o_dist + n * k * 4;
        o_q = (o_cnt + n * 4 + 15) & ~(size_t)15;
        need = o_q + n * dim * 4;
    }
    int64_t* ids(uint8_t* base) const { return reinterpret_cast<int64_t*>(base + o_ids); }
    float* dist(uint8_t* base) const { return reinterpret_cast<float*>(base + o_dist); }
    uint32_t* counts(uint8_t* base) const { return reinterpret_cast<uint32_t*>(base + o_cnt); }
    float* queries(uint8_t* base) const { return reinterpret_cast<float*>(base + o_q); }
};

// Replaces a pinned, device-mapped buffer that is smaller than `need` (its contents are lost; the caller knows that
// nothing in flight uses it) and says whether it did.
bool grow_pinned(uint8_t*& host, uint8_t*& dev, size_t& bytes, size_t need) {
    if (bytes >= need) return false;
    if (host) HIP_CHECK(hipHostFree(host));
    host = nullptr;
    bytes = 0;
    const size_t want = std::max<size_t>(need * 2, 64 * 1024);
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&host), want, hipHostMallocMapped | hipHostMallocCoherent));
    HIP_CHECK(hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0));
    bytes = want;
    return true;
}

void check_filter(const cph_index* h, const cph_filter* f) {
    if (f->device != h->device) throw InvalidArg("filter belongs to another device");
    if (f->n_bits != h->size())
        throw InvalidArg("filter covers " + std::to_string(f->n_bits) + " ids, the index holds " + std::to_string(h->size()));
}

// What every batch entry checks, under the handle mutex, before it touches the device; false: nothing to do ((n, 0)
// outputs: nothing to write; the entry point has been validated like search()'s).
bool batch_has_work(cph_index* h, const cph_filter* f, const float* queries, uint64_t n, uint64_t k, const int64_t* ids,
                    const float* dist) {
    require_finalized(h);
    if (f) check_filter(h, f);
    if (n == 0 || k == 0) return false;
    if (n > 0xFFFFFFFFull || k > 0xFFFFFFFFull) throw InvalidArg("batch too large");
    if (!queries || !ids || !dist) throw InvalidArg("null argument");
    return true;
}

// The filter's allowed ids as an ascending list on its device.  The first caller enqueues the compaction on its stream;
// every caller's stream waits for it.
const uint32_t* filter_id_list(const cph_filter* f, hipStream_t st) {
    std::lock_guard<std::mutex> lk(f->ids_mu);
    if (!f->ids_ev) {
        f->ids.alloc(f->popcount);
        f->ids_scratch.alloc((f->n_bits + kFilterSpan - 1) / kFilterSpan);
        filter_ids(f->words.p, f->n_bits, f->ids_scratch.p, f->ids.p, st);
        hipEvent_t ev = nullptr;
        HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(ev, st));
        f->ids_ev = ev;
    } else {
        HIP_CHECK(hipStreamWaitEvent(st, f->ids_ev, 0));
    }
    return f->ids.p;
}

// An exact batch (device_exact.h) in the place of enqueue_search: d_raw_q = [nq][dim] raw queries in HBM, results into
// device buffers, everything enqueued on `st`.  The candidates are the filter's ids (not empty), or every id.
void enqueue_exact(cph_index* h, BatchSet& s, const float* d_raw_q, uint32_t nq, uint32_t k, const cph_filter* filter,
                   int64_t* d_ids, float* d_dist, hipStream_t st) {
    const uint64_t n = h->size(), m = filter ? filter->popcount : n;     // (the tail rows: more candidates)
    const uint32_t D = h->L.D;
    const uint32_t nq_pad = (nq + kExactQT - 1) / kExactQT * kExactQT;
    const ExactPlan pl = plan_exact(m, nq, k, h->num_cus, h->exact_scratch_bytes);
    if (s.x_qpad.n < (size_t)nq_pad * D || s.x_pools.n < pl.pool_keys || s.x_counts.n < (size_t)pl.P * pl.tile_q || s.d_status.n < nq) {
        if (s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));   // growing: the old buffers must be idle
        s.x_qpad.alloc((size_t)nq_pad * D);
        s.x_qnorm.alloc(nq_pad);
        s.x_pools.alloc(pl.pool_keys);
        s.x_counts.alloc((size_t)pl.P * pl.tile_q);
        s.d_count.alloc(nq);
        s.d_status.alloc(nq);
        s.d_redo.alloc(nq);
    }
    const uint32_t* d_list = filter ? filter_id_list(filter, st) : nullptr;
    s.d_stats.alloc(kStatWords);
    HIP_CHECK(hipMemsetAsync(s.d_stats.p, 0, kStatWords * 8, st));
    HIP_CHECK(hipMemsetAsync(s.d_status.p, 0, (size_t)nq * 4, st));      // no query expands anything
    HIP_CHECK(hipEventRecord(s.ev0, st));
    pad_queries(h, d_raw_q, nullptr, nq, nq_pad, s.x_qpad.p, s.x_qnorm.p, s.d_stats.p, (unsigned long long)nq * m, st);
    ExactArgs a{};
    a.s = scan_common(h, s.x_qpad.p, s.x_qnorm.p, pl.gq, pl.part);
    a.ids = d_list;
    a.m = (uint32_t)m;
    a.k = k;
    a.C = pl.C;
    a.pools = s.x_pools.p;
    a.counts = s.x_counts.p;
    for (uint32_t q0 = 0; q0 < nq; q0 += pl.tile_q) {
        const uint32_t q_count = std::min(pl.tile_q, nq - q0);
        a.s.q_first = q0;
        a.s.q_count = q_count;
        CPH_LAUNCH_SCAN(exact_scan_kernel, D, dim3(pl.P, (q_count + pl.gq - 1) / pl.gq), (size_t)pl.C * 8 + (size_t)pl.gq * 8, st, a);
        hipLaunchKernelGGL(exact_merge_kernel, dim3(q_count), dim3(64), (size_t)pl.C * 8, st, (const unsigned long long*)s.x_pools.p,
                           (const uint32_t*)s.x_counts.p, pl.P, q0, q_count, k, pl.C,
                           (const uint32_t*)(h->ids_input ? h->d_rows.p : nullptr), d_ids, d_dist);
        HIP_CHECK(hipGetLastError());
    }
    s.run_slots = 0;
    s.run_cap = 0;
    s.nq = nq;
    finish_batch(h, s, st);
}

// Which path a batch takes.  Exact: asked for (cph_search_batch_exact*), or a filtered batch whose filter allows at most
// exact_threshold ids (and whose k the scan supports).  The empty filter keeps its no-launch padding path either way.
bool takes_exact(const cph_index* h, const cph_filter* f, uint64_t k, bool exact) {
    if (exact && k > kExactMaxK)
        throw InvalidArg("exact search supports k <= " + std::to_string(kExactMaxK) + ", got k = " + std::to_string(k));
    if (f && f->popcount == 0) return false;
    return exact || (f && h->exact_threshold > 0 && f->popcount <= h->exact_threshold && k <= kExactMaxK);
}

// One batch search, in every form the entry points offer.  Filter: cph_filter (on replicas filters[f * R + r] is filter f on
// replica r) or cph_parts_filter.  filter_of == null: F <= 1, one filter (filters[0]) or none for the whole batch;
// filter_of != null: per-query filters, filter_of[n] in host memory.
template <class Filter>
struct BatchCallT {
    const float* q = nullptr;                 // [n][dim]: host memory, or (on_device) device memory
    uint64_t n = 0, k = 0;
    const Filter* const* filters = nullptr;
    uint32_t F = 0;
    const int32_t* filter_of = nullptr;
    bool exact = false;
    int64_t* ids = nullptr;                   // [n][k], where the queries are
    float* dist = nullptr;
    bool on_device = false;                   // everything is enqueued on `stream`, nothing waits for the device
    hipStream_t stream = nullptr;
};
using BatchCall = BatchCallT<cph_filter>;

template <class Filter>
BatchCallT<Filter> batch_call(const float* q, uint64_t n, uint64_t k, const Filter* const* filters, uint32_t F, const int32_t* filter_of,
                              bool exact, int64_t* ids, float* dist, bool on_device = false, void* stream = nullptr) {
    return BatchCallT<Filter>{q, n, k, filters, F, filter_of, exact, ids, dist, on_device, reinterpret_cast<hipStream_t>(stream)};
}

// Every filter_of value is -1 or the number of a filter (F itself must stay an invalid value).
void check_filter_of(const int32_t* filter_of, uint64_t n, uint32_t F) {
    for (uint64_t i = 0; i < n; ++i)
        if (filter_of[i] < -1 || filter_of[i] >= (int64_t)F)
            throw InvalidArg("filter_of[" + std::to_string(i) + "] = " + std::to_string(filter_of[i]) + " is outside [-1, " +
                             std::to_string(F) + ")");
}

// ---- per-query filters: row i of the batch under filter filter_of[i] ------------------------------------------------------
// The grouping of such a batch (device_exact.h: filter_groups), made on the host before anything touches the device.
struct FilterGroups {
    std::vector<uint64_t> pop;         // [F] allowed ids of every filter
    std::vector<uint8_t> route;        // [F + 1] ExactRoute of every filter and, last, of the unfiltered queries
    std::vector<uint32_t> perm, seg;   // [n], [F + 2]
};

FilterGroups group_filters(const cph_index* h, const cph_filter* const* filters, uint32_t F, const int32_t* filter_of, uint64_t n,
                           uint64_t k, bool exact) {
    if (exact && k > kExactMaxK)
        throw InvalidArg("exact search supports k <= " + std::to_string(kExactMaxK) + ", got k = " + std::to_string(k));
    FilterGroups g;
    g.pop.resize(F);
    for (uint32_t f = 0; f < F; ++f) g.pop[f] = filters[f]->popcount;
    g.route.resize(F + 1);
    g.perm.resize(n);
    g.seg.resize(F + 2);
    filter_groups(filter_of, n, g.pop.data(), F, k, exact, h->exact_threshold, g.route.data(), g.perm.data(), g.seg.data());
    if (h->tail)
        for (uint32_t f = 0; f <= F; ++f)
            if (g.route[f] == kRouteGraph && g.seg[f + 1] != g.seg[f])
                throw NotImplemented("per-query filters on an index with added rows serve the scanned queries only (exact, or every "
                                     "filter at or below the exact threshold): a query of this batch would walk the graph; "
                                     "compact() the index first");
    return g;
}

// The per-query arguments of a handle with removed rows: every filter becomes F & ~R, the handle's ~R is appended and the
// queries with -1 are sent to it -- the call a caller without cph_remove would have had to make.  (Without removed rows:
// the arguments as they came.)
struct LiveFilters {
    std::vector<std::shared_ptr<const cph_filter>> hold;
    std::vector<const cph_filter*> list;
    std::vector<int32_t> of;
    const cph_filter* const* filters = nullptr;
    uint32_t F = 0;
    const int32_t* filter_of = nullptr;
};

void live_filters(cph_index* h, const cph_filter* const* filters, uint32_t F, const int32_t* filter_of, uint64_t n, LiveFilters& out) {
    out.filters = filters; out.F = F; out.filter_of = filter_of;
    if (h->host.n_removed == 0) return;
    check_filter_of(filter_of, n, F);              // (before -1 is renumbered)
    h->use_device();
    for (uint32_t f = 0; f < F; ++f) {
        out.hold.push_back(effective_filter(h, filters[f]));
        out.list.push_back(out.hold.back().get());
    }
    out.list.push_back(h->live.get());
    out.of.assign(filter_of, filter_of + n);
    for (int32_t& x : out.of)
        if (x < 0) x = (int32_t)F;
    out.filters = out.list.data(); out.F = F + 1; out.filter_of = out.of.data();
}

// What every entry with per-query filters checks, under the handle mutex, before it touches the device (batch_has_work).
bool filters_batch_has_work(cph_index* h, const cph_filter* const* filters, uint32_t F, const int32_t* filter_of, const float* queries,
                            uint64_t n, uint64_t k, const int64_t* ids, const float* dist) {
    require_finalized(h);
    if (F && !filters) throw InvalidArg("null argument");
    for (uint32_t f = 0; f < F; ++f) {
        if (!filters[f]) throw InvalidArg("null filter in the filter list");
        check_filter(h, filters[f]);
    }
    if (n == 0 || k == 0) return false;
    if (n > 0xFFFFFFFFull || k > 0xFFFFFFFFull) throw InvalidArg("batch too large");
    if (!queries || !ids || !dist || !filter_of) throw InvalidArg("null argument");
    return true;
}

// A batch with per-query filters in the place of enqueue_search / enqueue_exact: d_raw_q = [nq][dim] raw queries in HBM,
// results into device buffers, everything enqueued on `st`.  Per route (FilterGroups): padded rows are filled, scanned
// queries of ALL filters share one pad launch and one scan + merge launch pair per scratch budget (device_exact.h: the
// grouped scan), graph-searched queries run as two launch pairs -- the filtered ones through the filter-table
// instantiation, the unfiltered ones (-1) through the kernels of the plain call, so their rows and counters are those.
// One host wait: the tables are written into the set's pinned buffer, so the call first waits (StagedTable) until the copy of
// the tables this set carried the last time -- n_sets batches back -- has read it; nothing waits for a kernel.  As soon as
// one query takes the graph route, stage_queries encodes and descends ALL nq queries (the graph kernels index the staged
// queries by row), also the scanned and padded ones.
void enqueue_filters(cph_index* h, BatchSet& s, const float* d_raw_q, uint32_t nq, uint32_t k, const cph_filter* const* filters,
                     uint32_t F, const int32_t* filter_of, const FilterGroups& g, int64_t* d_ids, float* d_dist, hipStream_t st) {
    const uint64_t n = h->host.n;
    const uint32_t D = h->L.D;
    // the segments of the scan, the other routes' sizes
    std::vector<uint64_t> seg_m, seg_q;
    std::vector<uint32_t> seg_group, seg_first;
    uint32_t nqs = 0, n_pad = 0, n_gf = 0, n_gp = 0;
    unsigned long long n_exact = 0;
    for (uint32_t f = 0; f <= F; ++f) {
        const uint32_t cnt = g.seg[f + 1] - g.seg[f];
        if (!cnt) continue;
        if (g.route[f] == kRoutePad) n_pad += cnt;
        else if (g.route[f] == kRouteGraph) (f < F ? n_gf : n_gp) += cnt;
        else {
            seg_group.push_back(f);
            seg_m.push_back(f < F ? g.pop[f] : h->size());
            seg_q.push_back(cnt);
            seg_first.push_back(nqs);
            nqs += cnt;
            n_exact += (unsigned long long)cnt * seg_m.back();
        }
    }
    const ExactGroupPlan pl = plan_exact_groups(seg_m.data(), seg_q.data(), (uint32_t)seg_m.size(), k, h->num_cus, h->exact_scratch_bytes);
    const uint32_t nq_pad = nqs ? (nqs + kExactQT - 1) / kExactQT * kExactQT + kExactQT : 0;   // (a group's last tile reads up to 7 rows behind it)
    // the call's tables, one blob
    size_t need = 0;
    const size_t o_items = table_take(need, pl.items.size() * sizeof(ExactItem)), o_desc = table_take(need, (size_t)nqs * 16),
                 o_scanq = table_take(need, (size_t)nqs * 4), o_pad = table_take(need, (size_t)n_pad * 4),
                 o_gf = table_take(need, (size_t)n_gf * 4), o_gp = table_take(need, (size_t)n_gp * 4),
                 o_fof = table_take(need, n_gf ? (size_t)nq * 4 : 0), o_tab = table_take(need, n_gf ? (size_t)F * 8 : 0);
    need = std::max<size_t>(need, 16);
    Reserve r{s.ev_done, s.used};                                 // growing: the old buffers must be idle (one wait)
    uint8_t* const tb = s.tab.begin(need, r);
    const size_t pools = (size_t)pl.max_pools;
    r(s.x_qpad, (size_t)nq_pad * D);
    r(s.x_qnorm, nq_pad);
    r(s.x_pools, pools * pl.C);
    r(s.x_counts, pools);
    r(s.d_count, nq);
    r(s.d_status, nq);
    r(s.d_redo, nq);
    r(s.d_redo2, nq);
    // every scanned filter's id list: made once (filter_id_list), the stream waits for it
    std::vector<const uint32_t*> seg_ids(seg_m.size(), nullptr);
    for (size_t i = 0; i < seg_m.size(); ++i)
        if (seg_group[i] < F) seg_ids[i] = filter_id_list(filters[seg_group[i]], st);
    ExactItem* items = reinterpret_cast<ExactItem*>(tb + o_items);
    uint4* desc = reinterpret_cast<uint4*>(tb + o_desc);
    uint32_t* scanq = reinterpret_cast<uint32_t*>(tb + o_scanq);
    uint32_t *pad_rows = reinterpret_cast<uint32_t*>(tb + o_pad), *gf = reinterpret_cast<uint32_t*>(tb + o_gf),
             *gp = reinterpret_cast<uint32_t*>(tb + o_gp);
    for (size_t i = 0; i < seg_m.size(); ++i)
        std::memcpy(scanq + seg_first[i], g.perm.data() + g.seg[seg_group[i]], (size_t)seg_q[i] * 4);
    const size_t n_launch = pl.launch_pools.size();
    std::vector<uint32_t> l_qlo(n_launch, 0xFFFFFFFFu), l_qhi(n_launch, 0);       // scan positions every launch merges
    for (size_t i = 0; i < pl.items.size(); ++i) {
        const ExactGroupItem& it = pl.items[i];
        const uint32_t row0 = seg_first[it.seg] + it.q_lo;
        items[i] = ExactItem{seg_ids[it.seg], it.c_lo, it.c_hi, row0, it.q_cnt, it.pool, 0u};
        if (it.part != 0) continue;
        for (uint32_t j = 0; j < it.q_cnt; ++j) desc[row0 + j] = make_uint4(it.pool + j, it.q_cnt, pl.seg_parts[it.seg], scanq[row0 + j]);
        l_qlo[it.launch] = std::min(l_qlo[it.launch], row0);
        l_qhi[it.launch] = std::max(l_qhi[it.launch], row0 + it.q_cnt);
    }
    {
        uint32_t a_pad = 0, a_gf = 0, a_gp = 0;
        for (uint32_t i = 0; i < nq; ++i) {
            const uint32_t f = filter_of[i] < 0 ? F : (uint32_t)filter_of[i];
            if (g.route[f] == kRoutePad) pad_rows[a_pad++] = i;
            else if (g.route[f] == kRouteGraph) (f < F ? gf[a_gf++] : gp[a_gp++]) = i;
        }
    }
    if (n_gf) {
        std::memcpy(tb + o_fof, filter_of, (size_t)nq * 4);
        const uint32_t** tab = reinterpret_cast<const uint32_t**>(tb + o_tab);
        for (uint32_t f = 0; f < F; ++f) tab[f] = filters[f]->words.p;
    }
    const uint8_t* const dt = s.tab.send(need, st);

    s.d_stats.alloc(kStatWords);
    HIP_CHECK(hipMemsetAsync(s.d_stats.p, 0, kStatWords * 8, st));
    HIP_CHECK(hipMemsetAsync(s.d_status.p, 0, (size_t)nq * 4, st));      // scanned and padded queries expand nothing
    HIP_CHECK(hipMemsetAsync(s.d_count.p, 0, (size_t)nq * 4, st));
    HIP_CHECK(hipEventRecord(s.ev0, st));
    const uint32_t* d_rows = h->ids_input ? h->d_rows.p : nullptr;
    if (nqs) {
        pad_queries(h, d_raw_q, reinterpret_cast<const uint32_t*>(dt + o_scanq), nqs, nq_pad, s.x_qpad.p, s.x_qnorm.p, s.d_stats.p, n_exact, st);
        ExactGroupArgs a{};
        a.s = scan_common(h, s.x_qpad.p, s.x_qnorm.p, pl.gq, 0);
        a.k = k;
        a.C = pl.C;
        a.pools = s.x_pools.p;
        a.counts = s.x_counts.p;
        for (size_t l = 0; l < n_launch; ++l) {
            a.items = reinterpret_cast<const ExactItem*>(dt + o_items) + pl.launch_items[l];
            CPH_LAUNCH_SCAN(exact_scan_groups_kernel, D, dim3(pl.launch_items[l + 1] - pl.launch_items[l]), (size_t)pl.C * 8 + (size_t)pl.gq * 8, st, a);
            hipLaunchKernelGGL(exact_merge_groups_kernel, dim3(l_qhi[l] - l_qlo[l]), dim3(64), (size_t)pl.C * 8, st,
                               (const unsigned long long*)s.x_pools.p, (const uint32_t*)s.x_counts.p,
                               reinterpret_cast<const uint4*>(dt + o_desc) + l_qlo[l], k, pl.C, d_rows, d_ids, d_dist);
            HIP_CHECK(hipGetLastError());
        }
    }
    if (n_pad) {
        hipLaunchKernelGGL(exact_fill_rows_kernel, dim3(n_pad), dim3(64), 0, st, reinterpret_cast<const uint32_t*>(dt + o_pad), k, d_ids, d_dist);
        HIP_CHECK(hipGetLastError());
    }
    s.run_slots = 0;
    s.run_cap = 0;
    if (n_gf + n_gp) {
        stage_queries(h, s, d_raw_q, nq, st);
        const bool ordered = size_search(h, s, std::max(n_gf, n_gp), k, st);
        // a pair that holds the whole batch is launched closest entry first, like a plain batch; a part of it in query order
        const uint32_t* d_order = nullptr;
        if (std::max(n_gf, n_gp) == nq && nq > s.run_slots && ordered) {
            hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, st, s.d_entry_dist.p, nq, s.d_order.p);
            HIP_CHECK(hipGetLastError());
            d_order = s.d_order.p;
        }
        bool any_main = false;
        uint32_t direct_slots = 0;
        auto run = [&](uint32_t cnt, const uint32_t* list, SubBatch sub) {
            if (!cnt) return;
            sub.todo = cnt == nq ? d_order : list;
            // (as in enqueue_search: a filtered launch does not probe first, a handful of queries goes straight to the full-capacity slots)
            const bool rerun = s.cap < n + 1 || (!sub.allow_tab && probe_first(h));
            if (rerun && cnt <= s.r_slots && !h->want_cap && !h->want_slots) {
                direct_slots = std::max(direct_slots, cnt);
                launch_search(h, s, cnt, k, d_ids, d_dist, s.d_count.p, sub.todo, Launch::Direct, st, DoneFlags(), nullptr, &sub);
            } else {
                any_main = true;
                launch_search(h, s, cnt, k, d_ids, d_dist, s.d_count.p, sub.todo, Launch::Main, st, DoneFlags(), nullptr, &sub);
                if (rerun) launch_search(h, s, cnt, k, d_ids, d_dist, s.d_count.p, nullptr, Launch::Rerun, st, DoneFlags(), nullptr, &sub);
            }
        };
        SubBatch filtered, plain;
        filtered.queue = 0;
        filtered.redo = s.d_redo.p;
        filtered.allow_tab = reinterpret_cast<const uint32_t* const*>(dt + o_tab);
        filtered.filter_of = reinterpret_cast<const uint32_t*>(dt + o_fof);
        plain.queue = kQueueSecond;
        plain.redo = s.d_redo2.p;
        run(n_gf, reinterpret_cast<const uint32_t*>(dt + o_gf), filtered);
        run(n_gp, reinterpret_cast<const uint32_t*>(dt + o_gp), plain);
        if (!any_main) {      // only the full-capacity slots ran (enqueue_search's bookkeeping for that case): the larger of the two launches
            s.run_slots = direct_slots;
            s.run_cap = n + 1;
        }
    }
    s.nq = nq;
    finish_batch(h, s, st);
}

// The host form's I/O around `enqueue(d_q, d_ids, d_dist)`: the queries up (unless nothing will read them), result rows in
// the set's buffers, both copied back; the set is busy until the copies have landed, and the call waits for them.
template <class Enqueue>
void with_host_io(cph_index* h, BatchSet& s, const BatchCall& c, bool upload, hipStream_t st, Enqueue&& enqueue) {
    const uint64_t n = c.n, k = c.k;
    const float* d_q = upload ? upload_queries(h, s, c.q, n, st) : nullptr;
    if (s.d_ids.n < n * k) {
        if (s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));
        s.d_ids.alloc(n * k);
        s.d_dist.alloc(n * k);
    }
    enqueue(d_q, s.d_ids.p, s.d_dist.p);
    HIP_CHECK(hipMemcpyAsync(c.ids, s.d_ids.p, n * k * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(c.dist, s.d_dist.p, n * k * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipEventRecord(s.ev_done, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

// Every cph_search_batch* entry of one index; the caller holds the handle mutex.  The device form enqueues everything on the
// caller's stream.  Two routes, by the call's form and not by what it holds:
// * one filter or none (filter_of == null) -> enqueue_search, or enqueue_exact (takes_exact).  An empty filter launches
//   nothing (enqueue_search): no encoder, and its padding is written into device buffers by copy commands;
// * per-query filters -> enqueue_filters, over the handle's live filters and their grouping.
void search_batch_locked(cph_index* h, const BatchCall& c) {
    const uint64_t n = c.n, k = c.k;
    if (c.filter_of || c.F > 1) {                 // (F > 1 without filter_of: checked like a per-query call, refused if there is work)
        if (!filters_batch_has_work(h, c.filters, c.F, c.filter_of, c.q, n, k, c.ids, c.dist)) return;
        LiveFilters lf;
        live_filters(h, c.filters, c.F, c.filter_of, n, lf);
        const FilterGroups g = group_filters(h, lf.filters, lf.F, lf.filter_of, n, k, c.exact);
        h->use_device();
        hipStream_t st = c.on_device ? c.stream : own_stream(h);
        BatchSet& s = next_set(h, st);
        auto enqueue = [&](const float* d_q, int64_t* d_ids, float* d_dist) {
            d_q = metric_queries(h, s, d_q, n, st);
            enqueue_filters(h, s, d_q, (uint32_t)n, (uint32_t)k, lf.filters, lf.F, lf.filter_of, g, d_ids, d_dist, st);
            metric_scores(h, s, d_ids, d_dist, n, k, st);
        };
        if (c.on_device) enqueue(c.q, c.ids, c.dist);
        else with_host_io(h, s, c, true, st, enqueue);
        return;
    }
    if (c.F && !c.filters) throw InvalidArg("null argument");
    const cph_filter* f = c.F ? c.filters[0] : nullptr;
    if (!batch_has_work(h, f, c.q, n, k, c.ids, c.dist)) return;
    h->use_device();
    const std::shared_ptr<const cph_filter> eff = effective_filter(h, f);     // removed rows: F & ~R
    f = eff.get();
    const bool exact = takes_exact(h, f, k, c.exact);
    if (!exact) require_tail_k(h, k);
    hipStream_t st = c.on_device ? c.stream : own_stream(h);
    BatchSet& s = next_set(h, st);
    const bool empty = f && f->popcount == 0;     // (never exact: takes_exact)
    auto enqueue = [&](const float* d_q, int64_t* d_ids, float* d_dist) {
        if (!empty) d_q = metric_queries(h, s, d_q, n, st);
        if (exact) {
            enqueue_exact(h, s, d_q, (uint32_t)n, (uint32_t)k, f, d_ids, d_dist, st);
            return metric_scores(h, s, d_ids, d_dist, n, k, st);
        }
        if (!empty) stage_queries(h, s, d_q, n, st);
        enqueue_search(h, s, (uint32_t)n, (uint32_t)k, d_ids, d_dist, st, nullptr, DoneFlags(), f, d_q);
        if (!empty) metric_scores(h, s, d_ids, d_dist, n, k, st);      // (an empty filter's rows are padding, and no c was made)
    };
    if (c.on_device) return enqueue(c.q, c.ids, c.dist);
    if (!exact && !empty && n <= kSmallBatch && n * k <= (1u << 20)) {
        // a handful of queries: no copy commands, the kernels read the queries and write the results over PCIe
        const PinnedIo io(n, k, h->dim_in, 0);
        if (s.pin_io_bytes < io.need && s.used) HIP_CHECK(hipEventSynchronize(s.ev_done));   // growing: the old buffer must be idle
        grow_pinned(s.pin_io, s.pin_io_dev, s.pin_io_bytes, io.need);
        std::memcpy(io.queries(s.pin_io), c.q, n * h->dim_in * sizeof(float));
        const float* d_q = metric_queries(h, s, io.queries(s.pin_io_dev), n, st);    // (cosine: pinned rows in, HBM rows out)
        stage_queries(h, s, d_q, n, st);
        enqueue_search(h, s, (uint32_t)n, (uint32_t)k, io.ids(s.pin_io_dev), io.dist(s.pin_io_dev), st, io.counts(s.pin_io_dev),
                       DoneFlags(), f, d_q);
        metric_scores(h, s, io.ids(s.pin_io_dev), io.dist(s.pin_io_dev), n, k, st);      // (inner product: on the pinned rows)
        HIP_CHECK(hipStreamSynchronize(st));
        std::memcpy(c.ids, io.ids(s.pin_io), n * k * 8);
        std::memcpy(c.dist, io.dist(s.pin_io), n * k * 4);
        return;
    }
    with_host_io(h, s, c, !empty, st, enqueue);
}

void search_batch(cph_index* h, const BatchCall& c) {
    if (!h) throw InvalidArg("null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    search_batch_locked(h, c);
}


}  // namespace

// diagnostic build (-DCPH_SEARCH_TRACE): where a coalesced cph_search launch spends its host time
#ifdef CPH_SEARCH_TRACE
static std::atomic<uint64_t> g_tr[6];   // groups, callers, ns waiting for the handle mutex (per group), ns enqueuing (per group), ns each caller waited for its own query
static inline uint64_t now_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
#define CPH_TR(i, v) g_tr[i] += (v)
#else
#define CPH_TR(i, v) ((void)(v))
static inline uint64_t now_ns() { return 0; }
#endif

// ---------------------------------------------------------------------------------------
extern "C" {

const char* cph_last_error(void) { return g_err.c_str(); }
int cph_version(void) { return 118; }

int cph_create(uint64_t dim, uint64_t bits, int device, cph_index** out) {
    return guarded([&] {
        if (!out) throw InvalidArg("out must not be null");
        *out = nullptr;
        // src/bindings.cpp:100-113, :77-98; api/hnsw_index.hpp:90
        if (bits != 1 && bits != 2 && bits != 4)
            throw InvalidArg("Unsupported bits=" + std::to_string(bits) + ". Supported: 1, 2, 4.");
        const size_t pd = next_pow2(dim);
        if (dim == 0) throw InvalidArg("dim must be > 0");
        // (the reference pads only up to the next power of two; dims below 9 land on padded sizes it does not instantiate)
        if (pd < 16 || pd > 2048)
            throw InvalidArg("Unsupported dimension " + std::to_string(dim) + " (padded to " + std::to_string(pd) +
                             "). Supported padded dims: 16, 32, 64, 128, 256, 512, 1024, 2048.");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw std::runtime_error("No HIP device available: the MI355X path has no CPU fallback.");
        if (device < 0 || device >= ndev) throw InvalidArg("invalid device ordinal");
        auto* h = new cph_index();
        h->dim = dim;
        h->dim_in = dim;
        h->bits = (uint32_t)bits;
        h->D = (uint32_t)pd;
        h->device = device;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->num_cus = prop.multiProcessorCount;
        if (const char* e = getenv("CPH_QUERY_ORDER")) h->order_queries = atoi(e) != 0;
        if (const char* e = getenv("CPH_LEADER_SLOTS")) h->coal.n_slots = std::max(1, std::min(kLeaderSlots, atoi(e)));
        if (const char* e = getenv("CPH_EXACT_SCRATCH_MB")) h->exact_scratch_bytes = (size_t)std::max(1, atoi(e)) << 20;
        if (const char* e = getenv("CPH_GATHER_US")) h->coal.gather_us = std::max(0, atoi(e));
        if (const char* e = getenv("CPH_WAVES_PER_CU")) { h->waves_per_cu = (uint32_t)std::max(1, atoi(e)); h->waves_from_env = true; }
        *out = h;
    });
}

}  // extern "C"

// Refuses the lifecycle calls of a replica that a cph_multi owns (cph_multi_replica).
static void refuse_borrowed(const cph_index* h, const char* what) {
    if (h->borrowed)
        throw InvalidArg(std::string(what) + " on a replica of a multi-device index: call it on the multi-device handle");
}
// ... and the calls that need the host arrays on a replica that keeps none (every replica but the first).
static void refuse_host_less(const cph_index* h, const char* what) {
    if (h->host_less)
        throw InvalidArg(std::string(what) + " on a replica that keeps no host arrays: use replica 0");
}

static void destroy_index(cph_index* h) {
    (void)hipSetDevice(h->device);
    for (auto& s : h->sets) {
        if (s.used && s.ev_done) (void)hipEventSynchronize(s.ev_done);
        if (s.ev0) (void)hipEventDestroy(s.ev0);
        if (s.ev1) (void)hipEventDestroy(s.ev1);
        if (s.ev_done) (void)hipEventDestroy(s.ev_done);
        if (s.pin_stats) (void)hipHostFree(s.pin_stats);
        if (s.pin_io) (void)hipHostFree(s.pin_io);
    }
#ifdef CPH_SEARCH_TRACE
    if (g_tr[0]) fprintf(stderr, "[search trace] groups=%llu callers=%llu per group: mutex wait %.1f us, enqueue %.1f us; per caller: own-query wait %.1f us\n",
                         (unsigned long long)g_tr[0], (unsigned long long)g_tr[1], g_tr[2] / 1e3 / g_tr[0], g_tr[3] / 1e3 / g_tr[0], g_tr[4] / 1e3 / g_tr[1]);
    for (auto& x : g_tr) x = 0;
#endif
    for (auto& gs : h->rerank_scratch)
        if (gs.rows.used) (void)hipEventSynchronize(gs.rows.ev);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    for (auto& pt : h->pass_timer) {
        if (pt.ev0) (void)hipEventDestroy(pt.ev0);
        if (pt.ev1) (void)hipEventDestroy(pt.ev1);
    }
    for (auto& ls : h->leaders) {
        if (ls.stream) { (void)hipStreamSynchronize(ls.stream); (void)hipStreamDestroy(ls.stream); }
        if (ls.pin) (void)hipHostFree(ls.pin);
    }
    delete h;
}

extern "C" int cph_destroy(cph_index* h) {
    return guarded([&] {
        if (!h) return;
        refuse_borrowed(h, "cph_destroy");
        destroy_index(h);
    });
}

// Called once the new host-side index has been read and validated: from here until the end of a load the handle is
// not searchable, so a failed device allocation or copy leaves it unfinalized (an error on the next search) instead of
// finalized over null or stale device pointers.
static void begin_device_swap(cph_index* h) {
    h->use_device();
    quiesce(h);
    h->finalized = false;
    for (auto& s : h->sets) release_scratch(s);
    h->last_search = -1;
    h->last_range = false;
    h->range_scratch.clear();
    h->label_rows.reset();
    h->drop_facets();
    ++h->index_epoch;
}

// No file format carries a tail: a file written now would lose the added rows.
static void refuse_tail_file(const cph_index* h) {
    if (h->tail)
        throw std::runtime_error("No file format carries added rows (" + std::to_string(h->tail) +
                                 " here) and a file without them would lose them: compact() the index first.");
}

// The reference's file format has no place for the metric: a file written from a cosine handle would be searched as L2
// by whoever loads it, and a file loaded into one holds rows nobody normalised.
static const char* metric_name(uint32_t metric) { return metric == CPH_METRIC_IP ? "ip" : metric == CPH_METRIC_COSINE ? "cosine" : "l2"; }
static void refuse_metric_file(const cph_index* h, const char* what) {
    if (h->metric != CPH_METRIC_L2)
        throw InvalidArg(std::string(what) + ": the reference's file format cannot carry the " + (h->metric == CPH_METRIC_IP ? "inner-product (ip)" : "cosine") +
                         " metric: use save_native / load_native");
}
// The searches an inner-product handle does not serve yet: their results need an epilogue of their own shape (grouped,
// diverse, MaxSim), or a per-query radius map whose boundary rounding is not decided (range).  Refused before any output
// row is written.
static void refuse_ip(const cph_index* h, const char* what) {
    if (h->metric == CPH_METRIC_IP)
        throw InvalidArg(std::string(what) + " is not available under the inner-product (ip) metric");
}

// The encoder carries kMaxUpperLayers layer descriptors.  A file that uses more would be descended from layer
// kMaxUpperLayers starting at the file's entry vertex, where the reference starts at max_level: another walk, with no
// error.  Refused before the handle gives up its index.
static void refuse_deep_layers(const HostIndex& t) {
    const long long usable = std::min<long long>((long long)t.upper.size(), t.max_level);
    if (usable > kMaxUpperLayers)
        throw std::runtime_error("Index file uses " + std::to_string(usable) + " upper layers; the descent supports at most " +
                                 std::to_string(kMaxUpperLayers) + " (kMaxUpperLayers).");
}

static void load_v2(cph_index* h, const char* path) {
    std::lock_guard<std::mutex> lk(h->mu);
    refuse_metric_file(h, "load");
    HostIndex t;
    t.load(path, h->D, h->bits, h->dim);        // a file that fails to parse leaves the handle as it was
    refuse_deep_layers(t);                      // (... and so does one with more layers than the descent has)
    begin_device_swap(h);
    h->host = std::move(t);
    drop_host_state(h);
    upload_arrays(h);
    sync_row_map(h);                            // (a v2 file carries no row map)
    sync_columns(h);                             // (no file carries labels)
    sync_removed(h);                            // (... and no removed rows)
    upload_feeders(h);
    h->finalized = true;
}

extern "C" {

int cph_load(cph_index* h, const char* path) {
    return guarded([&] {
        if (!h || !path) throw InvalidArg("null argument");
        refuse_borrowed(h, "cph_load");
        load_v2(h, path);
    });
}

int cph_save(cph_index* h, const char* path) {
    return guarded([&] {
        if (!h || !path) throw InvalidArg("null argument");
        refuse_host_less(h, "cph_save");
        std::lock_guard<std::mutex> lk(h->mu);
        if (!h->finalized) throw std::runtime_error("Index must be finalized before saving.");
        refuse_metric_file(h, "save");
        if (h->host.n_removed != 0)
            throw std::runtime_error("The reference format cannot carry removed rows (" + std::to_string(h->host.n_removed) +
                                     " here) and a file without them would bring them back: compact() the index first, or use save_native.");
        refuse_tail_file(h);
        materialize_search_data(h);
        h->host.save(path);
    });
}

int cph_save_native(cph_index* h, const char* path) {
    return guarded([&] {
        if (!h || !path) throw InvalidArg("null argument");
        refuse_host_less(h, "cph_save_native");
        std::lock_guard<std::mutex> lk(h->mu);
        if (!h->finalized) throw std::runtime_error("Index must be finalized before saving.");
        refuse_tail_file(h);
        h->use_device();
        quiesce(h);
        const HostIndex& hi = h->host;
        const size_t n = hi.n, stride = h->L.stride, own_stride = hi.RL.nb_off;
        std::vector<uint8_t> blocks(n * stride), own;
        download_blocks(h->d_blocks.p, n, h->L, blocks.data());   // the file keeps the storage layout
        const uint8_t* own_p = h->own_view;
        if (!own_p) {
            own.resize(n * own_stride);
            for (size_t v = 0; v < n; ++v) std::memcpy(&own[v * own_stride], &hi.search_data[v * hi.RL.vertex_bytes], own_stride);
            own_p = own.data();
        }
        write_native(path, hi, (uint32_t)stride, own_p, (uint32_t)own_stride, blocks.data(), h->metric, h->metric == CPH_METRIC_IP ? &h->ip_m2 : nullptr);
    });
}

}  // extern "C"

// A native file read and validated (read_native), not yet anybody's index.
struct NativeLoaded {
    HostIndex t;
    NativeMapping map;
    NativeHeader nh;
    float ip_m2 = 0.0f;       // an inner-product file's bound
};

static void read_native_for(const cph_index* h, const char* path, NativeLoaded& out) {
    uint32_t metric = CPH_METRIC_L2;
    out.nh = read_native(path, h->D, h->bits, h->dim, out.t, out.map, &metric, &out.ip_m2);   // validates everything it maps
    if (metric != h->metric)
        throw InvalidArg(std::string("the file holds ") + metric_name(metric) + " rows and this handle's metric is " +
                         metric_name(h->metric) + ": load it into an index created with the file's metric");
    refuse_deep_layers(out.t);
}

// The handle gives up its index for the one in `in` (which is consumed).
static void install_native(cph_index* h, NativeLoaded& in) {
    std::lock_guard<std::mutex> lk(h->mu);
    HostIndex& t = in.t;
    NativeMapping& map = in.map;
    const NativeHeader nh = in.nh;
    begin_device_swap(h);
    h->host = std::move(t);
    drop_host_state(h);
    if (h->metric == CPH_METRIC_IP) h->ip_m2 = in.ip_m2;
    h->native_map = std::move(map);
    const uint8_t* base = static_cast<const uint8_t*>(h->native_map.base);
    h->own_view = base + nh.own_off;
    h->L = make_dev_layout((uint32_t)h->host.D, (uint32_t)h->host.bw);
    const size_t n = h->host.n;
    h->d_blocks.alloc(n * nh.stride + 64);
    h->d_raw.alloc(n * h->host.D);
    h->d_norm.alloc(n);
    HIP_CHECK(hipMemcpy(h->d_blocks.p, base + nh.blocks_off, n * (size_t)nh.stride, hipMemcpyHostToDevice));
    relayout_blocks(h->d_blocks.p, n, h->L, true);
    HIP_CHECK(hipMemcpy(h->d_raw.p, h->host.raw_view, n * h->host.D * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(h->d_norm.p, h->host.norm_sq.data(), n * 4, hipMemcpyHostToDevice));
    sync_row_map(h);
    sync_columns(h);
    sync_removed(h);                            // the file's removed rows, or none
    upload_feeders(h);
    h->finalized = true;
}

static void load_native_file(cph_index* h, const char* path) {
    NativeLoaded in;
    read_native_for(h, path, in);               // a file that fails to validate leaves the handle as it was
    install_native(h, in);
}

extern "C" {

int cph_load_native(cph_index* h, const char* path) {
    return guarded([&] {
        if (!h || !path) throw InvalidArg("null argument");
        refuse_borrowed(h, "cph_load_native");
        load_native_file(h, path);
    });
}

int cph_size(cph_index* h, uint64_t* n) {
    return guarded([&] { *n = h->needs_build ? h->pending_n : h->size(); });
}
int cph_dim(cph_index* h, uint64_t* dim) {
    return guarded([&] { *dim = h->dim_in; });
}
int cph_is_finalized(cph_index* h, int* flag) {
    return guarded([&] { *flag = h->finalized ? 1 : 0; });
}

}  // extern "C"

// What build() and finalize() refuse about the number of rows -- one statement, also asked by compact() BEFORE the
// handle gives up its index.
static void require_buildable(uint64_t n) {
    if (n == 0) throw InvalidArg("build requires at least one vector.");
}
static void require_finalizable(uint64_t n) {
    if (n == 0) throw std::runtime_error("Cannot finalize an empty index.");
    if (n < 50) throw std::runtime_error("Calibration requires at least 50 nodes.");
    if (n >= 0xFFFFFFFFull) throw InvalidArg("too many vectors");
}

// The one funnel behind cph_build, cph_multi_build, cph_parts_build and cph_compact.  as_given: the rows are stored as
// they are -- an L2 handle's, and under cosine the rows that are normalised already (compact's live rows: a second pass
// over a nearly-unit row changes bits; a partitioned build's, normalised in one go for the global row numbers).
// Otherwise a cosine handle normalises them first, and a bad row refuses the call with the handle as it was; an
// inner-product handle takes rows of dim_in coordinates, augments them (ip_rows_in) and refuses likewise.
static void build_pending(cph_index* h, const float* vectors, uint64_t n, bool as_given = false) {
    std::lock_guard<std::mutex> lk(h->mu);
    // api/hnsw_index.hpp:93-120: build() replaces any previous state
    require_buildable(n);
    if (!vectors) throw InvalidArg("null vectors");
    std::vector<float> unit;
    float m2 = h->ip_m2;                                  // (inner product, as_given: the rows keep the bound they were stored against)
    if (h->metric == CPH_METRIC_IP && !as_given) m2 = ip_rows_in(h, vectors, n, h->ip_bound != 0.0f ? &h->ip_bound : nullptr, false, unit);
    else if (h->metric != CPH_METRIC_L2 && !as_given) normalize_rows_in(h, vectors, n, 0, unit);
    h->use_device();
    quiesce(h);
    h->ip_m2 = m2;
    h->host = HostIndex();
    drop_host_state(h);
    h->finalized = false;
    ++h->index_epoch;
    h->d_blocks.release(); h->d_raw.release(); h->d_norm.release();
    sync_row_map(h);
    sync_columns(h);
    sync_removed(h);
    for (auto& s : h->sets) release_scratch(s);
    if (!unit.empty()) h->pending = std::move(unit);
    else h->pending.assign(vectors, vectors + n * h->dim);
    h->pending_n = n;
    h->needs_build = true;
}

static void finalize_build(cph_index* h) {
    std::lock_guard<std::mutex> lk(h->mu);
    // api/hnsw_index.hpp:122-166
    const uint64_t n = h->needs_build ? h->pending_n : h->host.n;
    if (n == 0) throw std::runtime_error("Cannot finalize an empty index.");
    if (!h->needs_build) throw std::runtime_error("Finalize called without a pending build.");
    require_finalizable(n);
    h->use_device();
    const bool verbose = getenv("CPH_BUILD_VERBOSE") != nullptr;
    quiesce(h);
    ++h->index_epoch;
    h->d_blocks.release(); h->d_raw.release(); h->d_norm.release();
    for (auto& s : h->sets) release_scratch(s);
    build::BuiltDevice dev;
    build::build_graph(h->host, dev, h->pending.data(), n, h->dim, h->D, h->bits, h->num_cus, verbose);
    std::vector<float>().swap(h->pending);
    h->pending_n = 0;
    h->needs_build = false;
    // the pipeline's device arrays are the searchable index: adopt them, no second upload
    h->d_blocks = std::move(dev.blocks);
    h->d_raw = std::move(dev.raw);
    h->d_norm = std::move(dev.norm);
    h->d_rows = std::move(dev.rows);           // the BFS renumbering, kept: host.rows is its host copy
    h->has_rows = true;
    h->native_map.reset();
    h->own_store = std::move(dev.own_host);
    h->own_view = h->own_store.data();
    upload_feeders(h);
    build::DeviceIndexView view{h->d_blocks.p, h->d_raw.p, h->d_signs.p, h->L, h->norm_factor, h->inv_sqrt_d};
    build::calibrate(h->host, view, h->num_cus, verbose);
    h->sc = h->host.consts();
    h->finalized = true;
}

extern "C" {

int cph_build(cph_index* h, const float* vectors, uint64_t n) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_build");
        build_pending(h, vectors, n);
    });
}

int cph_finalize(cph_index* h) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_finalize");
        finalize_build(h);
    });
}

int cph_knn_bruteforce(int device, const float* vectors, uint64_t n, uint64_t dim, const float* queries,
                       uint64_t nq, uint32_t* ids, float* dist) {
    return guarded([&] {
        if (!vectors || !ids || !dist || n == 0 || dim == 0) throw InvalidArg("bad arguments");
        if (n >= 0xFFFFFFFFull || nq >= 0xFFFFFFFFull) throw InvalidArg("too many rows");
        HIP_CHECK(hipSetDevice(device));
        const size_t D = std::max<size_t>(16, next_pow2(dim));
        auto pad = [&](const float* src, uint64_t rows, std::vector<float>& x, std::vector<float>& nrm) {
            x.assign(rows * D, 0.0f);
            nrm.resize(rows);
            parallel_for(rows, 1024, [&](size_t lo, size_t hi) {
                for (size_t i = lo; i < hi; ++i) {
                    std::memcpy(&x[i * D], src + i * dim, dim * 4);
                    float s = 0.0f;
                    for (uint64_t j = 0; j < dim; ++j) s = std::fmaf(x[i * D + j], x[i * D + j], s);
                    nrm[i] = s;
                }
            });
        };
        std::vector<float> x, nrm, q, qn;
        pad(vectors, n, x, nrm);
        if (queries) pad(queries, nq, q, qn);
        int cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) cus = prop.multiProcessorCount;
        build::gpu_knn(queries ? q.data() : nullptr, queries ? qn.data() : nullptr, nq, x.data(), nrm.data(), n, D,
                       cus, ids, dist);
    });
}

// ---- the exact-kNN kernels against their host statement (host_knn.h) ----------------------------------------------------
static_assert(kHostKnnK == (uint32_t)kKnnK && kHostKnnChunk == (uint32_t)kKnnKC && kHostKnnSymSample == kKnnSymSample &&
              kHostKnnSymRank == kKnnSymRank && kHostKnnSymCap == kKnnSymCap, "host_knn.h restates the constants of the kernels");

int cph_host_knn(const float* vectors, uint64_t n, uint64_t dim, const float* queries, uint64_t nq, const uint32_t* q_ids,
                 int exclude_self, int path, uint32_t* ids, float* dist, uint32_t* fallback_rows, uint32_t* cand_count) {
    return guarded([&] {
        knn_debug_check(vectors, n, dim, queries, nq, q_ids, exclude_self, path, ids, dist);
        const uint32_t redo = knn_host(vectors, n, dim, queries, nq, q_ids, path, ids, dist, path == 1 ? cand_count : nullptr);
        if (fallback_rows) *fallback_rows = redo;
    });
}

int cph_debug_knn(int device, const float* vectors, uint64_t n, uint64_t dim, const float* queries, uint64_t nq, const uint32_t* q_ids,
                  int exclude_self, int path, uint32_t blocks_per_launch, uint32_t* ids, float* dist, uint32_t* fallback_rows,
                  uint32_t* launches) {
    return guarded([&] {
        knn_debug_check(vectors, n, dim, queries, nq, q_ids, exclude_self, path, ids, dist);
        if (blocks_per_launch > 65536) throw InvalidArg("knn debug: blocks_per_launch <= 65536");
        HIP_CHECK(hipSetDevice(device));
        const size_t D = knn_padded_dim(dim);
        std::vector<float> x, nrm, q, qn;
        knn_pad_rows(vectors, n, dim, D, x, nrm);
        if (queries) knn_pad_rows(queries, nq, dim, D, q, qn);
        int cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) cus = prop.multiProcessorCount;
        const size_t rows = queries ? nq : n;
        uint32_t redo = 0, made = 0;
        DevBuf<float> d_x(n * D), d_norm(n), d_od(rows * kKnnK);
        DevBuf<uint32_t> d_oi(rows * kKnnK);
        HIP_CHECK(hipMemcpy(d_x.p, x.data(), n * D * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_norm.p, nrm.data(), n * 4, hipMemcpyHostToDevice));
        // (a row the kernels do not write would show: the model writes every slot)
        HIP_CHECK(hipMemset(d_oi.p, 0xA5, rows * kKnnK * 4));
        HIP_CHECK(hipMemset(d_od.p, 0xA5, rows * kKnnK * 4));
        if (!queries) {
            build::KnnKnobs knobs;
            knobs.path = path;
            knobs.blocks_per_launch = blocks_per_launch;
            knobs.fallback_rows = &redo;
            knobs.launches = &made;
            build::knn_self_device(d_x.p, d_norm.p, n, D, cus, d_oi.p, d_od.p, false, knobs);
        } else {
            DevBuf<float> d_q(nq * D), d_qn(nq);
            DevBuf<uint32_t> d_qi(q_ids ? nq : 1);
            HIP_CHECK(hipMemcpy(d_q.p, q.data(), nq * D * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_qn.p, qn.data(), nq * 4, hipMemcpyHostToDevice));
            if (q_ids) HIP_CHECK(hipMemcpy(d_qi.p, q_ids, nq * 4, hipMemcpyHostToDevice));
            build::knn_device(d_q.p, d_qn.p, nq, d_x.p, d_norm.p, n, D, q_ids != nullptr, cus, d_oi.p, d_od.p, q_ids ? d_qi.p : nullptr,
                              blocks_per_launch, &made);
        }
        HIP_CHECK(hipMemcpy(ids, d_oi.p, rows * kKnnK * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(dist, d_od.p, rows * kKnnK * 4, hipMemcpyDeviceToHost));
        if (fallback_rows) *fallback_rows = redo;
        if (launches) *launches = made;
    });
}

int cph_debug_heap_ops(int device, const uint8_t* ops, uint64_t n_ops, const float* keys, const uint32_t* ids, uint64_t n_push,
                       float* out_keys, uint32_t* out_ids, uint32_t* out_size) {
    return guarded([&] {
        if (!ops || !out_keys || !out_ids || !out_size || n_ops == 0 || n_ops > 0x7FFFFFFFull) throw InvalidArg("bad arguments");
        if (n_push && (!keys || !ids)) throw InvalidArg("bad arguments");
        uint64_t pushes = 0;
        for (uint64_t i = 0; i < n_ops; ++i) pushes += ops[i] ? 1 : 0;
        if (pushes != n_push) throw InvalidArg("n_push must equal the number of push operations");
        HIP_CHECK(hipSetDevice(device));
        DevBuf<uint8_t> d_ops(n_ops);
        DevBuf<float> d_keys(std::max<uint64_t>(1, n_push)), d_ok(std::max<uint64_t>(1, n_push));
        DevBuf<uint32_t> d_ids(std::max<uint64_t>(1, n_push)), d_oi(std::max<uint64_t>(1, n_push)), d_sz(1);
        DevBuf<uint32_t> d_spill(kBeamPagesDwords), d_spill_tail(beam_tail_dwords(std::max<uint64_t>(1, n_push) + 64));
        HIP_CHECK(hipMemcpy(d_ops.p, ops, n_ops, hipMemcpyHostToDevice));
        if (n_push) {
            HIP_CHECK(hipMemcpy(d_keys.p, keys, n_push * 4, hipMemcpyHostToDevice));
            HIP_CHECK(hipMemcpy(d_ids.p, ids, n_push * 4, hipMemcpyHostToDevice));
        }
        HeapTestArgs a{d_ops.p, d_keys.p, d_ids.p, (uint32_t)n_ops, d_spill.p, d_spill_tail.p, d_ok.p, d_oi.p, d_sz.p};
        hipLaunchKernelGGL(heap_selftest_kernel, dim3(1), dim3(64), 0, nullptr, a);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out_size, d_sz.p, 4, hipMemcpyDeviceToHost));
        if (*out_size > n_push) throw std::runtime_error("heap self-test: size out of range");
        if (*out_size) {
            HIP_CHECK(hipMemcpy(out_keys, d_ok.p, (size_t)*out_size * 4, hipMemcpyDeviceToHost));
            HIP_CHECK(hipMemcpy(out_ids, d_oi.p, (size_t)*out_size * 4, hipMemcpyDeviceToHost));
        }
    });
}

int cph_encode_edges(int device, uint64_t dim, uint64_t bits, const float* parent, const float* nbrs, uint64_t cnt,
                     uint8_t* values, float* aux, uint32_t* pops) {
    return guarded([&] {
        if (!parent || !nbrs || !values || !aux || !pops || cnt == 0 || cnt > 32 || dim == 0) throw InvalidArg("bad arguments");
        if (bits != 1 && bits != 2 && bits != 4) throw InvalidArg("bits must be 1, 2 or 4");
        const size_t D = std::max<size_t>(16, next_pow2(dim));
        if (D > 2048) throw InvalidArg("unsupported dimension");
        HIP_CHECK(hipSetDevice(device));
        const size_t n = cnt + 1;                       // vertex 0 = the parent, 1..cnt = its neighbours
        std::vector<float> x(n * D, 0.0f);
        std::memcpy(x.data(), parent, dim * 4);
        for (uint64_t e = 0; e < cnt; ++e) std::memcpy(&x[(e + 1) * D], nbrs + e * dim, dim * 4);
        std::vector<uint32_t> nbr(n * 32, kInvalidNode);
        for (uint64_t e = 0; e < cnt; ++e) nbr[e] = (uint32_t)(e + 1);
        Rotation rot;
        rot.init(D, 42);
        const DevLayout L = make_dev_layout((uint32_t)D, (uint32_t)bits);
        DevBuf<float> d_x(n * D), d_signs(3 * D), d_aux(n * 32 * 3);
        DevBuf<uint32_t> d_nbr(n * 32), d_pops(n * 32 * 2);
        DevBuf<uint8_t> d_blocks(n * L.stride), d_vals(n * 32 * D);
        HIP_CHECK(hipMemcpy(d_x.p, x.data(), n * D * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_nbr.p, nbr.data(), n * 32 * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_signs.p, rot.signs.data(), 3 * D * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(d_blocks.p, 0, n * L.stride));
        HIP_CHECK(hipMemset(d_vals.p, 0, n * 32 * D));
        HIP_CHECK(hipMemset(d_aux.p, 0, n * 32 * 3 * 4));
        HIP_CHECK(hipMemset(d_pops.p, 0, n * 32 * 2 * 4));
        build::EncodeArgsB a{};
        const float df = (float)D;
        a.x = d_x.p; a.nbr = d_nbr.p; a.n = n; a.dim = (uint32_t)dim; a.D = (uint32_t)D;
        a.signs = d_signs.p; a.norm_factor = 1.0f / (df * std::sqrt(df)); a.inv_sqrt_d = 1.0f / std::sqrt(df);
        a.L = L; a.blocks = d_blocks.p;
        a.dbg_values = d_vals.p; a.dbg_aux = d_aux.p; a.dbg_pops = d_pops.p;
        build::run_encode(bits, a, 1, 1);
        HIP_CHECK(hipMemcpy(values, d_vals.p, cnt * D, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(aux, d_aux.p, cnt * 3 * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(pops, d_pops.p, cnt * 2 * 4, hipMemcpyDeviceToHost));
    });
}

int cph_select_hook(int device, const float* x, uint64_t n, uint64_t D, uint32_t vertex, const uint32_t* fwd,
                    const uint32_t* rev, uint64_t n_rev, uint32_t R, float alpha, float tau, float alpha_max,
                    const float* err, uint32_t* out_ids, uint32_t* out_cnt) {
    return guarded([&] {
        if (!x || !fwd || !out_ids || !out_cnt || n == 0 || vertex >= n) throw InvalidArg("bad arguments");
        if (D < 16 || D > 2048 || (D & (D - 1))) throw InvalidArg("D must be a power of two in 16..2048");
        if (R == 0 || R > 32 || n_rev > 65536) throw InvalidArg("R must be 1..32 and n_rev <= 65536");
        if (n_rev && !rev) throw InvalidArg("bad arguments");
        for (int i = 0; i < 32; ++i)
            if (fwd[i] != kInvalidNode && fwd[i] >= n) throw InvalidArg("candidate out of range");
        for (uint64_t i = 0; i < n_rev; ++i)
            if (rev[i] >= n) throw InvalidArg("candidate out of range");
        HIP_CHECK(hipSetDevice(device));
        // one row: the vertex is row 0 of a one-row layer (row_ids = {vertex}), reverse candidates are row indices of
        // a table that maps them back to the given vertex ids
        DevBuf<float> d_x(n * D), d_err(n);
        DevBuf<uint32_t> d_fwd(32), d_rev(std::max<uint64_t>(1, n_rev)), d_rows(std::max<uint64_t>(1, n_rev) + 1), d_out(32), d_cnt(1);
        DevBuf<uint64_t> d_off(2);
        HIP_CHECK(hipMemcpy(d_x.p, x, n * D * 4, hipMemcpyHostToDevice));
        if (err) HIP_CHECK(hipMemcpy(d_err.p, err, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_fwd.p, fwd, 128, hipMemcpyHostToDevice));
        // row 0 = the vertex itself; reverse candidate i is "row i + 1", whose vertex id is rev[i]
        std::vector<uint32_t> rows(n_rev + 1), revrows(std::max<uint64_t>(1, n_rev));
        rows[0] = vertex;
        for (uint64_t i = 0; i < n_rev; ++i) { rows[i + 1] = rev[i]; revrows[i] = (uint32_t)(i + 1); }
        HIP_CHECK(hipMemcpy(d_rows.p, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_rev.p, revrows.data(), revrows.size() * 4, hipMemcpyHostToDevice));
        const uint64_t off[2] = {0, n_rev};
        HIP_CHECK(hipMemcpy(d_off.p, off, 16, hipMemcpyHostToDevice));
        build::SelectArgs a{};
        a.x = d_x.p; a.fwd = d_fwd.p; a.rev_off = d_off.p; a.rev = d_rev.p; a.row_ids = d_rows.p; a.err = err ? d_err.p : nullptr;
        a.rows = 1; a.D = (uint32_t)D; a.R = R; a.alpha = alpha; a.tau = tau; a.alpha_max = alpha_max;
        a.out = d_out.p; a.out_cnt = d_cnt.p;
        hipLaunchKernelGGL(build::select_kernel, dim3(1), dim3(64), build::select_lds(a.D), nullptr, a);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out_ids, d_out.p, 128, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(out_cnt, d_cnt.p, 4, hipMemcpyDeviceToHost));
    });
}

int cph_select_layer_hook(int device, const float* x, uint64_t n, uint64_t D, const uint32_t* knn, uint32_t R, float alpha,
                          float tau, float alpha_max, const float* err, uint32_t grid_cap, uint32_t* out_ids,
                          uint32_t* out_cnt, uint64_t* rev_off, uint32_t* rev) {
    return guarded([&] {
        if (!x || !knn || !out_ids || !out_cnt || n == 0 || n >= kInvalidNode) throw InvalidArg("bad arguments");
        if (D < 16 || D > 2048 || (D & (D - 1))) throw InvalidArg("D must be a power of two in 16..2048");
        if (R == 0 || R > 32) throw InvalidArg("R must be 1..32");
        for (uint64_t i = 0; i < n * 32; ++i)
            if (knn[i] != kInvalidNode && knn[i] >= n) throw InvalidArg("candidate out of range");
        HIP_CHECK(hipSetDevice(device));
        int cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) cus = prop.multiProcessorCount;
        DevBuf<float> d_x(n * D), d_err(n);
        DevBuf<uint32_t> d_knn(n * 32), d_out(n * 32), d_cnt(n);
        HIP_CHECK(hipMemcpy(d_x.p, x, n * D * 4, hipMemcpyHostToDevice));
        if (err) HIP_CHECK(hipMemcpy(d_err.p, err, n * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_knn.p, knn, n * 32 * 4, hipMemcpyHostToDevice));
        // the layer-0 call of build_graph: every vertex a row (row_ids null), the CSR built from the table
        const build::LayerParams lp{R, alpha, tau, alpha_max, err ? d_err.p : nullptr};
        build::LayerCsr csr;
        build::select_layer(d_x.p, D, d_knn.p, n, nullptr, lp, cus, d_out.p, d_cnt.p, &csr, grid_cap);
        HIP_CHECK(hipMemcpy(out_ids, d_out.p, n * 32 * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(out_cnt, d_cnt.p, n * 4, hipMemcpyDeviceToHost));
        if (rev_off) HIP_CHECK(hipMemcpy(rev_off, csr.off.p, (n + 1) * 8, hipMemcpyDeviceToHost));
        if (rev) {
            // at most n * 32 entries: one per valid entry of the table
            uint64_t total = 0;
            HIP_CHECK(hipMemcpy(&total, csr.off.p + n, 8, hipMemcpyDeviceToHost));
            if (total > n * 32) throw std::runtime_error("reverse CSR larger than the table");
            if (total) HIP_CHECK(hipMemcpy(rev, csr.rev.p, total * 4, hipMemcpyDeviceToHost));
        }
    });
}

int cph_calib_hook(cph_index* h, const float* queries, const uint32_t* start, uint64_t ns, float* rec, uint32_t* rec_cnt,
                   float* dqp) {
    return guarded([&] {
        if (!h || !queries || !start || !rec || !rec_cnt || !dqp || ns == 0 || ns > 0xFFFFFFull) throw InvalidArg("bad arguments");
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        for (uint64_t i = 0; i < ns; ++i)
            if (start[i] >= h->host.n) throw InvalidArg("start vertex out of range");
        h->use_device();
        hipStream_t st = own_stream(h);
        BatchSet& s = next_set(h, st);
        stage_queries(h, s, upload_queries(h, s, queries, ns, st, true), ns, st);     // the search's own encoder
        HIP_CHECK(hipEventRecord(s.ev_done, st));
        s.used = true;
        DevBuf<uint32_t> d_start(ns), d_rc(ns);
        DevBuf<float> d_rec(ns * 32 * 6), d_dqp(ns);
        HIP_CHECK(hipMemcpyAsync(d_start.p, start, ns * 4, hipMemcpyHostToDevice, st));
        build::CalibArgs c{};
        c.blocks = h->d_blocks.p; c.raw = h->d_raw.p; c.L = h->L; c.n = h->host.n;
        c.queries = s.d_queries.p; c.qmasks = s.d_qmasks.p; c.qhdr = s.d_qhdr.p;
        c.start = d_start.p; c.ns = (uint32_t)ns; c.rec = d_rec.p; c.rec_cnt = d_rc.p; c.dqp_out = d_dqp.p;
        const size_t lds = (size_t)h->L.PW * 16 + (size_t)h->L.D * 8;
        const dim3 grid((uint32_t)std::min<uint64_t>(ns, (uint64_t)h->num_cus * 16));
        if (h->bits == 1) hipLaunchKernelGGL(build::calib_kernel<1>, grid, dim3(64), lds, st, c);
        else if (h->bits == 2) hipLaunchKernelGGL(build::calib_kernel<2>, grid, dim3(64), lds, st, c);
        else hipLaunchKernelGGL(build::calib_kernel<4>, grid, dim3(64), lds, st, c);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(s.ev_done, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipMemcpy(rec, d_rec.p, ns * 32 * 6 * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(rec_cnt, d_rc.p, ns * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(dqp, d_dqp.p, ns * 4, hipMemcpyDeviceToHost));
    });
}

int cph_get_vectors(cph_index* h, uint64_t first, uint64_t count, float* out) {
    return guarded([&] {
        if (!h || !out) throw InvalidArg("null argument");
        refuse_host_less(h, "cph_get_vectors");
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        if (first > h->size() || count > h->size() - first) throw InvalidArg("vector range out of bounds");
        for (uint64_t i = 0; i < count; ++i)
            std::memcpy(out + i * h->dim, row_vec(h, first + i), h->dim * sizeof(float));
    });
}

int cph_set_search_params(cph_index* h, uint32_t slots, uint64_t beam_capacity) {
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        h->want_slots = slots;
        h->want_cap = beam_capacity;
    });
}

int cph_set_batch_sets(cph_index* h, uint32_t n_sets) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        if (n_sets < 1 || n_sets > (uint32_t)kMaxBatchSets) throw InvalidArg("n_sets must be 1.." + std::to_string(kMaxBatchSets));
        std::lock_guard<std::mutex> lk(h->mu);
        h->use_device();
        quiesce(h);
        for (int i = (int)n_sets; i < kMaxBatchSets; ++i) release_scratch(h->sets[i]);
        h->n_sets = (int)n_sets;
        h->last_set = (int)n_sets - 1;
    });
}

int cph_last_search_stats(cph_index* h, uint64_t out[12]) {
    return guarded([&] {
        if (!h || !out) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        for (int i = 0; i < 12; ++i) out[i] = 0;
        if (h->last_range) {                     // an exact range search: two passes over the candidates, nothing else
            out[kStatExact] = h->range_exact;
            return;
        }
        if (h->last_search < 0) return;
        BatchSet& s = h->sets[h->last_search];
        h->use_device();
        HIP_CHECK(hipEventSynchronize(s.ev_done));
        if (s.stats_in_hbm) {
            HIP_CHECK(hipMemcpy(s.pin_stats, s.d_stats.p, kStatWords * 8, hipMemcpyDeviceToHost));
            s.stats_in_hbm = false;
        }
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, s.ev0, s.ev1));
        // out[0..7] are the block's words kStatExpansions..kStatAllSeen, with the device time in the word no kernel writes
        for (int i = kStatExpansions; i <= kStatAllSeen; ++i) out[i] = s.pin_stats[i];
        out[kStatNoCounter] = (uint64_t)(ms * 1000.0);
        out[8] = s.run_slots;
        out[9] = s.run_cap;
        out[10] = stage2_stat(s, kStatStage2Reruns);
        out[11] = stage2_stat(s, kStatStage2Undecided);
#if defined(CPH_PHASE_TIMERS) || defined(CPH_TRAFFIC_STATS) || defined(CPH_TAIL_CENSUS)
        const unsigned long long* diag = s.pin_stats + kStatDiag;
#endif
#if CPH_PHASE_TIMERS + 0 == 2
        fprintf(stderr, "[fine cycles] head+issue=%llu pop=%llu block_wait=%llu probe_issue+exact+nnpush=%llu estimator=%llu probe_wait=%llu mark+cand=%llu pushes+tail=%llu\n",
                diag[0], diag[1], diag[2], diag[3], diag[4], diag[5], diag[6], diag[7]);
#elif defined(CPH_PHASE_TIMERS)
        fprintf(stderr, "[phase cycles] pop=%llu load+exact+nnpush=%llu sums+epi=%llu atomic+log+stage=%llu spec_exact=%llu replay=%llu tail=%llu other=%llu\n",
                diag[0], diag[1], diag[2], diag[3], diag[4], diag[5], diag[6], diag[7]);
#endif
#ifdef CPH_TAIL_CENSUS
        fprintf(stderr, "[tail census] lds_append=%llu spilled_append=%llu single_push_skips_append=%llu push_beats_parent=%llu nothing_to_push=%llu more_pushes_than_entries=%llu replay=%llu lane_parallel=%llu\n",
                diag[0], diag[1], diag[2], diag[3], diag[4], diag[5], diag[6], diag[7]);
#endif
#ifdef CPH_TRAFFIC_STATS
        fprintf(stderr, "[traffic] hybrid_pops=%llu windows=%llu hybrid_pushes=%llu hbm_appends=%llu probe_lines=%llu sum_beam_at_pop=%llu max_beam=%llu pops_beyond_8191=%llu\n",
                diag[0], diag[1], diag[2], diag[3], diag[4], diag[5], diag[6], diag[7]);
#endif
    });
}

int cph_last_query_expansions(cph_index* h, uint32_t* out, uint64_t n) {
    return guarded([&] {
        if (!h || !out) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        if (h->last_search < 0 || n != h->sets[h->last_search].nq)
            throw InvalidArg("n must equal the size of the last batch");
        BatchSet& s = h->sets[h->last_search];
        h->use_device();
        HIP_CHECK(hipEventSynchronize(s.ev_done));
        HIP_CHECK(hipMemcpy(out, s.d_status.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) out[i] >>= 8;
    });
}

int cph_synchronize(cph_index* h) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        h->use_device();
        quiesce(h);
    });
}

int cph_order_queries(cph_index* h, const float* keys, uint64_t n, uint32_t* order) {
    return guarded([&] {
        if (!h || !keys || !order) throw InvalidArg("null argument");
        if (n == 0 || n > 0xFFFFFFFFull) throw InvalidArg("bad n");
        std::lock_guard<std::mutex> lk(h->mu);
        h->use_device();
        DevBuf<float> dk;
        DevBuf<uint32_t> dord;
        dk.alloc(n);
        dord.alloc(n);
        HIP_CHECK(hipMemcpy(dk.p, keys, n * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(order_kernel, dim3(1), dim3(1024), 0, nullptr, dk.p, (uint32_t)n, dord.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(order, dord.p, n * 4, hipMemcpyDeviceToHost));
    });
}

int cph_search_batch(cph_index* h, const float* queries, uint64_t n, uint64_t k, int64_t* ids,
                     float* dist) {
    return cph_search_batch_filtered(h, queries, n, k, nullptr, ids, dist);
}

int cph_search_batch_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k,
                            int64_t* d_ids, float* d_dist, void* stream) {
    return cph_search_batch_device_filtered(h, d_queries, n, k, nullptr, d_ids, d_dist, stream);
}

// ---- filtered search --------------------------------------------------------------------
int cph_filter_create(cph_index* h, const uint32_t* words, uint64_t n_bits, cph_filter** out) {
    return guarded([&] {
        if (!h || !out || (!words && n_bits != 0)) throw InvalidArg("null argument");
        *out = nullptr;
        if (n_bits > 0xFFFFFFFFull) throw InvalidArg("filter too large");
        const uint64_t nw = (n_bits + 31) / 32;
        std::vector<uint32_t> w(words, words + nw);
        if (n_bits & 31) w[nw - 1] &= (1u << (n_bits & 31)) - 1u;   // bits behind the last id are never set
        uint64_t pc = 0;
        for (uint32_t x : w) pc += (uint64_t)__builtin_popcount(x);
        std::unique_ptr<cph_filter> f(new cph_filter());
        f->device = h->device;
        f->n_bits = n_bits;
        f->popcount = pc;
        h->use_device();
        f->words.alloc(std::max<uint64_t>(nw, 1));
        if (nw) HIP_CHECK(hipMemcpy(f->words.p, w.data(), nw * 4, hipMemcpyHostToDevice));
        *out = f.release();
    });
}

int cph_filter_destroy(cph_filter* f) {
    return guarded([&] {
        if (!f) return;
        std::unique_ptr<cph_filter> own(f);
        // batches enqueued with cph_search_batch_device_filtered may still read the bitmap
        HIP_CHECK(hipSetDevice(f->device));
        HIP_CHECK(hipDeviceSynchronize());
    });
}

int cph_search_batch_filtered(cph_index* h, const float* queries, uint64_t n, uint64_t k, const cph_filter* f,
                              int64_t* ids, float* dist) {
    return guarded([&] { search_batch(h, batch_call(queries, n, k, &f, f ? 1u : 0u, nullptr, false, ids, dist)); });
}

int cph_search_batch_device_filtered(cph_index* h, const float* d_queries, uint64_t n, uint64_t k, const cph_filter* f,
                                     int64_t* d_ids, float* d_dist, void* stream) {
    return guarded([&] { search_batch(h, batch_call(d_queries, n, k, &f, f ? 1u : 0u, nullptr, false, d_ids, d_dist, true, stream)); });
}

// ---- exact search -----------------------------------------------------------------------
int cph_search_batch_exact(cph_index* h, const float* queries, uint64_t n, uint64_t k, const cph_filter* f, int64_t* ids,
                           float* dist) {
    return guarded([&] { search_batch(h, batch_call(queries, n, k, &f, f ? 1u : 0u, nullptr, true, ids, dist)); });
}

int cph_search_batch_exact_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k, const cph_filter* f,
                                  int64_t* d_ids, float* d_dist, void* stream) {
    return guarded([&] { search_batch(h, batch_call(d_queries, n, k, &f, f ? 1u : 0u, nullptr, true, d_ids, d_dist, true, stream)); });
}

int cph_search_batch_filters(cph_index* h, const float* queries, uint64_t n, uint64_t k, const cph_filter* const* filters,
                             uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids, float* dist) {
    return guarded([&] { search_batch(h, batch_call(queries, n, k, filters, n_filters, filter_of, exact != 0, ids, dist)); });
}

int cph_search_batch_filters_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k, const cph_filter* const* filters,
                                    uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* d_ids, float* d_dist,
                                    void* stream) {
    return guarded([&] { search_batch(h, batch_call(d_queries, n, k, filters, n_filters, filter_of, exact != 0, d_ids, d_dist, true, stream)); });
}

int cph_host_filter_groups(const int32_t* filter_of, uint64_t n, const uint64_t* popcounts, uint32_t n_filters, uint64_t k, int exact,
                           uint64_t exact_threshold, uint8_t* routes, uint32_t* perm, uint32_t* seg) {
    return guarded([&] {
        if (!routes || !seg || (n && (!filter_of || !perm)) || (n_filters && !popcounts)) throw InvalidArg("null argument");
        if (n > 0xFFFFFFFFull) throw InvalidArg("batch too large");
        filter_groups(filter_of, n, popcounts, n_filters, k, exact != 0, exact_threshold, routes, perm, seg);
    });
}

int cph_host_exact_group_plan(const uint64_t* seg_candidates, const uint64_t* seg_queries, uint32_t n_segments, uint64_t k, int num_cus,
                              uint64_t scratch_bytes, uint32_t* items, uint64_t cap_items, uint64_t* out) {
    return guarded([&] {
        if (!out || (n_segments && (!seg_candidates || !seg_queries)) || (cap_items && !items)) throw InvalidArg("null argument");
        if (k == 0 || k > kExactMaxK) throw InvalidArg("exact plan: sizes out of range");
        for (uint32_t s = 0; s < n_segments; ++s)
            if (seg_candidates[s] > 0xFFFFFFFFull || seg_queries[s] > 0xFFFFFFFFull) throw InvalidArg("exact plan: sizes out of range");
        const ExactGroupPlan pl = plan_exact_groups(seg_candidates, seg_queries, n_segments, (uint32_t)k, num_cus, (size_t)scratch_bytes);
        out[0] = pl.items.size(); out[1] = pl.launch_pools.size(); out[2] = pl.gq; out[3] = pl.C;
        out[4] = (uint64_t)pl.max_pools * pl.C * 8; out[5] = 0;
        for (size_t i = 0; i < pl.items.size() && i < cap_items; ++i) {
            const ExactGroupItem& it = pl.items[i];
            const uint32_t row[8] = {it.seg, it.part, it.c_lo, it.c_hi, it.q_lo, it.q_cnt, it.pool, it.launch};
            std::memcpy(items + i * 8, row, sizeof(row));
        }
    });
}

int cph_set_exact_threshold(cph_index* h, uint64_t max_allowed) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        h->exact_threshold = max_allowed;
    });
}

int cph_host_filter_ids(const uint32_t* words, uint64_t n_bits, uint32_t* out_ids, uint64_t* out_count) {
    return guarded([&] {
        if (!out_count || (n_bits != 0 && !words)) throw InvalidArg("null argument");
        if (n_bits > 0xFFFFFFFFull) throw InvalidArg("filter too large");
        uint64_t pc = 0;
        for (uint64_t w = 0, nw = (n_bits + 31) / 32; w < nw; ++w) {
            uint32_t x = words[w];
            if (w == nw - 1 && (n_bits & 31)) x &= (1u << (n_bits & 31)) - 1u;
            pc += (uint64_t)__builtin_popcount(x);
        }
        if (pc != 0 && !out_ids) throw InvalidArg("null argument");
        *out_count = filter_ids_host(words, n_bits, out_ids);
    });
}

int cph_host_exact_plan(uint64_t candidates, uint64_t n_queries, uint64_t k, int num_cus, uint64_t scratch_bytes, uint64_t* out) {
    return guarded([&] {
        if (!out) throw InvalidArg("null argument");
        if (k == 0 || k > kExactMaxK || candidates == 0 || candidates > 0xFFFFFFFFull || n_queries == 0 || n_queries > 0xFFFFFFFFull)
            throw InvalidArg("exact plan: sizes out of range");
        const ExactPlan pl = plan_exact(candidates, (uint32_t)n_queries, (uint32_t)k, num_cus, (size_t)scratch_bytes);
        out[0] = pl.P; out[1] = pl.part; out[2] = pl.gq; out[3] = pl.tile_q; out[4] = pl.C; out[5] = (uint64_t)pl.pool_keys * 8;
    });
}

}  // extern "C"

// ---- range search: every allowed id closer than a radius, in CSR form (device_range.h) ----------------------------------
// Two steps, because the caller allocates the output: cph_range_search_begin counts (exact: the count pass and the offsets
// scan; graph route: an ordinary search into scratch rows, cut at the radius) and returns the total, cph_range_search_finish
// writes the segments.  The object owns its scratch (it takes no batch set; the buffers come from, and go back to, the
// handle's short free list, so that a call in steady state makes no hipMalloc and no hipFree -- a hipFree waits for the
// whole device) and holds the effective filter it began under: a cph_remove between the two steps does not change the
// answer.
struct cph_range {
    cph_index* h = nullptr;
    int device = 0;
    uint64_t epoch = 0;                        // h->index_epoch at begin
    uint64_t n = 0;                            // queries
    bool exact = true;
    uint32_t K = 0;                            // graph route: entries per scratch row
    hipStream_t st = nullptr;                  // the caller's (device form) or the handle's own
    bool in_flight = false;                    // something enqueued has not been waited for (a failure in between)
    bool finished = false;
    std::shared_ptr<const cph_filter> filt;    // the snapshot F & ~R (aliasing the caller's F on a handle without removed rows)
    uint64_t m = 0;                            // candidates
    const uint32_t* d_list = nullptr;          // their ascending ids, or null: every id
    RangePlan pl{};
    std::vector<int64_t> lims;                 // [n + 1]
    uint64_t total = 0;
    std::unique_ptr<RangeScratch> s;           // its device buffers: taken from the handle at begin, handed back by destroy
};

namespace {

void range_sync(cph_range* r) {
    HIP_CHECK(hipStreamSynchronize(r->st));
    r->in_flight = false;
}

// The scan launches of one pass over the queries [q_first, q_first + q_count): grid.y holds at most 65,535 groups.
template <bool kFill>
void range_scan_pass(cph_range* r, RangeArgs a, uint32_t q_first, uint32_t q_count) {
    const uint32_t per = 65535u * r->pl.gq;
    for (uint64_t q0 = q_first; q0 < (uint64_t)q_first + q_count; q0 += per) {
        a.s.q_first = (uint32_t)q0;
        a.s.q_count = (uint32_t)std::min<uint64_t>(per, (uint64_t)q_first + q_count - q0);
        // (the fill's arena index is relative to the TILE's first query, whichever launch writes it)
        CPH_LAUNCH_SCAN(range_scan_kernel, a.s.D, dim3(r->pl.P, (a.s.q_count + r->pl.gq - 1) / r->pl.gq), (size_t)r->pl.gq * 12, r->st, a, kFill);
    }
}

RangeArgs range_args(const cph_range* r) {
    RangeArgs a{};
    a.s = scan_common(r->h, r->s->qpad.p, r->s->qnorm.p, r->pl.gq, r->pl.part);
    a.ids = r->d_list;
    a.m = (uint32_t)r->m;
    a.radius = r->s->d_rad.p;
    a.P = r->pl.P;
    a.counts = r->s->counts.p;
    a.offs = r->s->offs.p;
    a.arena = r->s->arena.p;
    return a;
}

void range_begin(cph_index* h, const float* queries, bool q_dev, uint64_t n, const float* radius, const cph_filter* f, bool exact,
                 uint64_t K, void* stream, cph_range** out, uint64_t* total) {
    if (!h) throw InvalidArg("null handle");
    if (!out || !total) throw InvalidArg("null argument");
    *out = nullptr;
    *total = 0;
    std::lock_guard<std::mutex> lk(h->mu);
    refuse_ip(h, "range search");
    require_finalized(h);
    if (f) check_filter(h, f);
    if (n > 0xFFFFFFFFull) throw InvalidArg("batch too large");
    if (n && (!queries || !radius)) throw InvalidArg("null argument");
    if (!exact && (K == 0 || K > 0xFFFFFFFFull)) throw InvalidArg("the graph route of a range search needs max_results >= 1");
    h->use_device();
    std::unique_ptr<cph_range> r(new cph_range());
    r->h = h;
    r->device = h->device;
    r->epoch = h->index_epoch;
    r->n = n;
    r->exact = exact;
    r->K = (uint32_t)K;
    r->lims.assign(n + 1, 0);
    if (!h->range_scratch.empty()) {
        r->s = std::move(h->range_scratch.back());
        h->range_scratch.pop_back();
    } else {
        r->s.reset(new RangeScratch());
    }
    hipStream_t st = q_dev ? reinterpret_cast<hipStream_t>(stream) : own_stream(h);
    r->st = st;
    if (exact) {
        r->filt = effective_filter(h, f);                  // removed rows: F & ~R
        r->m = r->filt ? r->filt->popcount : h->size();
    }
    if (n == 0 || (exact && r->m == 0)) {                  // nothing to scan: every segment is empty
        if (exact) { h->last_range = true; h->range_exact = 0; }
        *out = r.release();
        return;
    }
    try {
        r->in_flight = true;
        r->s->d_rad.alloc(n);
        HIP_CHECK(hipMemcpyAsync(r->s->d_rad.p, radius, n * 4, hipMemcpyHostToDevice, st));
        const float* d_q = queries;
        if (!q_dev) {
            r->s->d_q.alloc(n * h->dim);
            HIP_CHECK(hipMemcpyAsync(r->s->d_q.p, queries, n * h->dim * 4, hipMemcpyHostToDevice, st));
            d_q = r->s->d_q.p;
        }
        if (exact && h->metric != CPH_METRIC_L2) {
            // cosine: the scan reads normalised queries (the graph route's are normalised by its own search_batch_locked);
            // into the call's own buffer -- in place when the queries were uploaded there
            r->s->d_q.alloc(n * h->dim);
            normalize_rows(d_q, r->s->d_q.p, n, (uint32_t)h->dim, (uint32_t)h->dim, (uint32_t)h->dim, nullptr, nullptr, st);
            ++h->metric_launches;
            d_q = r->s->d_q.p;
        }
        uint64_t n_cnt = n;
        uint32_t P = 1;
        if (!exact) {
            // the search itself, with all its routing, into scratch rows; then the cut
            r->s->g_ids.alloc(n * K);
            r->s->g_dist.alloc(n * K);
            r->s->counts.alloc(n);
            search_batch_locked(h, batch_call(d_q, n, K, &f, f ? 1u : 0u, nullptr, false, r->s->g_ids.p, r->s->g_dist.p, true, st));
            hipLaunchKernelGGL(range_cut_count_kernel, dim3((uint32_t)n), dim3(64), 0, st, (const int64_t*)r->s->g_ids.p, (const float*)r->s->g_dist.p,
                               (uint32_t)K, (const float*)r->s->d_rad.p, r->s->counts.p);
            HIP_CHECK(hipGetLastError());
        } else {
            const cph_filter* ef = r->filt.get();
            r->pl = plan_range(r->m, n, h->num_cus);
            P = r->pl.P;
            n_cnt = n * P;
            const uint32_t D = h->L.D;
            // Padded query rows.  exact_fma_chunk loads all kExactQT rows of a query tile, whatever the group holds, and a
            // fill launch starts its groups at a scratch tile's first query (range_tiles), which need not be a multiple of
            // kExactQT: the rows read end below q0 + roundup(n - q0) <= n + kExactQT - 1.  range_query_rows(n) holds them
            // all, zero behind n (cph_host_range_plan states it, the CPU tests check it against the tiles).
            const uint32_t nq_pad = (uint32_t)range_query_rows(n);
            r->s->qpad.alloc((size_t)nq_pad * D);
            r->s->qnorm.alloc(nq_pad);
            r->s->counts.alloc(n_cnt);
            r->s->d_stats.alloc(kStatWords);
            r->d_list = ef ? filter_id_list(ef, st) : nullptr;
            pad_queries(h, d_q, nullptr, (uint32_t)n, nq_pad, r->s->qpad.p, r->s->qnorm.p, r->s->d_stats.p, (unsigned long long)(2 * n * r->m), st);
            range_scan_pass<false>(r.get(), range_args(r.get()), 0, (uint32_t)n);
        }
        r->s->offs.alloc(n_cnt + 1);
        r->s->sums.alloc(n_cnt / kRangeScanSpan + 2);
        r->s->d_lims.alloc(n + 1);
        range_offsets(r->s->counts.p, n_cnt, P, r->s->sums.p, r->s->offs.p, r->s->d_lims.p, st);
        HIP_CHECK(hipMemcpyAsync(r->lims.data(), r->s->d_lims.p, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        range_sync(r.get());                               // the output size is data
    } catch (...) {
        if (r->in_flight) (void)hipStreamSynchronize(st);  // nothing may still read the buffers that go with r
        throw;
    }
    r->total = (uint64_t)r->lims[n];
    if (exact) { h->last_range = true; h->range_exact = 2 * n * r->m; }
    *total = r->total;
    *out = r.release();
}

// The sort tables of one tile, appended to `tab`: RangeRun[n_runs] | RangeLong[n_long]; returns the longest run / segment.
struct RangeTileTab {
    size_t o_runs = 0, o_long = 0;
    uint32_t n_runs = 0, n_long = 0, max_run = 0;
    uint64_t max_long = 0;
};

RangeTileTab range_tile_tables(const std::vector<int64_t>& lims, uint64_t lo, uint64_t hi, std::vector<uint8_t>& tab) {
    RangeTileTab t;
    std::vector<RangeRun> runs;
    std::vector<RangeLong> longs;
    const uint64_t base = (uint64_t)lims[lo];
    for (uint64_t q = lo; q < hi; ++q) {
        const uint64_t start = (uint64_t)lims[q] - base, len = (uint64_t)(lims[q + 1] - lims[q]);
        if (len > kRangeRun) {
            longs.push_back(RangeLong{start, len});
            t.max_long = std::max(t.max_long, len);
        }
        for (uint64_t o = 0; o < len; o += kRangeRun) {
            const uint32_t rl = (uint32_t)std::min<uint64_t>(kRangeRun, len - o);
            if (rl < 2) continue;
            runs.push_back(RangeRun{start + o, rl, 0});
            t.max_run = std::max(t.max_run, rl);
        }
    }
    t.n_runs = (uint32_t)runs.size();
    t.n_long = (uint32_t)longs.size();
    t.o_runs = tab.size();
    tab.insert(tab.end(), reinterpret_cast<const uint8_t*>(runs.data()), reinterpret_cast<const uint8_t*>(runs.data() + runs.size()));
    t.o_long = tab.size();
    tab.insert(tab.end(), reinterpret_cast<const uint8_t*>(longs.data()), reinterpret_cast<const uint8_t*>(longs.data() + longs.size()));
    return t;
}

void range_finish(cph_range* r, int64_t* lims_host, int64_t* ids, float* dist, bool on_dev) {
    if (!r || !lims_host) throw InvalidArg("null argument");
    cph_index* h = r->h;
    std::lock_guard<std::mutex> lk(h->mu);
    if (r->finished) throw InvalidArg("cph_range_search_finish was called on this object before");
    if (!h->finalized || h->index_epoch != r->epoch)
        throw std::runtime_error("The index changed between cph_range_search_begin and cph_range_search_finish.");
    std::memcpy(lims_host, r->lims.data(), (r->n + 1) * 8);
    if (r->total == 0) {
        r->finished = true;
        return;
    }
    if (!ids || !dist) throw InvalidArg("null argument");
    h->use_device();
    hipStream_t st = r->st;
    const uint64_t n = r->n;
    std::vector<uint8_t> tab;                              // (lives until the wait at the end: the copy may read it late)
    try {
        r->in_flight = true;
        int64_t* d_ids = ids;
        float* d_dist = dist;
        if (!on_dev) {
            r->s->o_ids.alloc(r->total);
            r->s->o_dist.alloc(r->total);
            d_ids = r->s->o_ids.p;
            d_dist = r->s->o_dist.p;
        }
        if (!r->exact) {
            hipLaunchKernelGGL(range_cut_emit_kernel, dim3((uint32_t)n), dim3(64), 0, st, (const int64_t*)r->s->g_ids.p, (const float*)r->s->g_dist.p,
                               r->K, (const float*)r->s->d_rad.p, (const unsigned long long*)r->s->d_lims.p, d_ids, d_dist);
            HIP_CHECK(hipGetLastError());
        } else {
            const std::vector<uint64_t> starts = range_tiles(r->lims.data(), n, h->exact_scratch_bytes);
            std::vector<RangeTileTab> tt;
            uint64_t max_keys = 0, max_keys_long = 0;
            for (size_t t = 0; t + 1 < starts.size(); ++t) {
                tt.push_back(range_tile_tables(r->lims, starts[t], starts[t + 1], tab));
                const uint64_t keys = (uint64_t)(r->lims[starts[t + 1]] - r->lims[starts[t]]);
                max_keys = std::max(max_keys, keys);
                if (tt.back().n_long) max_keys_long = std::max(max_keys_long, keys);
            }
            r->s->arena.alloc(max_keys);
            if (max_keys_long) r->s->arena2.alloc(max_keys_long);
            if (!tab.empty()) {
                r->s->d_tab.alloc(tab.size());
                HIP_CHECK(hipMemcpyAsync(r->s->d_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
            }
            const uint32_t* rows = h->ids_input ? h->d_rows.p : nullptr;
            for (size_t t = 0; t + 1 < starts.size(); ++t) {
                const uint64_t lo = starts[t], hi = starts[t + 1];
                const unsigned long long base = (unsigned long long)r->lims[lo];
                if ((uint64_t)r->lims[hi] == base) continue;           // no hit in the whole tile
                RangeArgs a = range_args(r);
                a.tile_base = base;
                range_scan_pass<true>(r, a, (uint32_t)lo, (uint32_t)(hi - lo));
                const RangeTileTab& x = tt[t];
                if (x.n_runs) {
                    uint32_t N = 64;
                    while (N < x.max_run) N <<= 1;
                    hipLaunchKernelGGL(range_sort_runs_kernel, dim3(x.n_runs), dim3(64), (size_t)N * 8, st,
                                       reinterpret_cast<const RangeRun*>(r->s->d_tab.p + x.o_runs), r->s->arena.p);
                    HIP_CHECK(hipGetLastError());
                }
                unsigned long long* src = r->s->arena.p;
                unsigned long long* dst = r->s->arena2.p;
                for (unsigned long long w = kRangeRun; x.n_long && w < x.max_long; w <<= 1) {
                    for (uint32_t s0 = 0; s0 < x.n_long; s0 += 65535u) {
                        const dim3 grid((uint32_t)((x.max_long + 255) / 256), std::min<uint32_t>(65535u, x.n_long - s0));
                        hipLaunchKernelGGL(range_merge_pass_kernel, grid, dim3(256), 0, st,
                                           reinterpret_cast<const RangeLong*>(r->s->d_tab.p + x.o_long) + s0, (const unsigned long long*)src, dst, w);
                        HIP_CHECK(hipGetLastError());
                    }
                    std::swap(src, dst);
                }
                hipLaunchKernelGGL(range_emit_kernel, dim3((uint32_t)(hi - lo)), dim3(256), 0, st, (const unsigned long long*)r->s->arena.p,
                                   (const unsigned long long*)src, (const unsigned long long*)r->s->d_lims.p, (uint32_t)lo, base, rows, d_ids, d_dist);
                HIP_CHECK(hipGetLastError());
            }
        }
        if (!on_dev) {
            HIP_CHECK(hipMemcpyAsync(ids, d_ids, r->total * 8, hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipMemcpyAsync(dist, d_dist, r->total * 4, hipMemcpyDeviceToHost, st));
        }
        range_sync(r);
    } catch (...) {
        if (r->in_flight) (void)hipStreamSynchronize(st);
        throw;
    }
    r->finished = true;
}

}  // namespace

extern "C" {

int cph_range_search_begin(cph_index* h, const void* queries, int queries_on_device, uint64_t n, const float* radius_host,
                           const cph_filter* filter, int exact, uint64_t max_results, void* stream, cph_range** out, uint64_t* total) {
    return guarded([&] {
        range_begin(h, static_cast<const float*>(queries), queries_on_device != 0, n, radius_host, filter, exact != 0, max_results, stream, out,
                    total);
    });
}

int cph_range_search_finish(cph_range* r, int64_t* lims_host, void* ids, void* dist, int results_on_device) {
    return guarded([&] { range_finish(r, lims_host, static_cast<int64_t*>(ids), static_cast<float*>(dist), results_on_device != 0); });
}

int cph_range_destroy(cph_range* r) {
    return guarded([&] {
        if (!r) return;
        std::unique_ptr<cph_range> own(r);
        if (r->in_flight) {                                // (only after a failure whose own wait failed too)
            HIP_CHECK(hipSetDevice(r->device));
            HIP_CHECK(hipDeviceSynchronize());
        }
        std::lock_guard<std::mutex> lk(r->h->mu);
        if (r->s && r->h->range_scratch.size() < kRangeScratchKept) r->h->range_scratch.push_back(std::move(r->s));
    });
}

int cph_host_range_plan(uint64_t candidates, uint64_t n_queries, int num_cus, uint64_t* out) {
    return guarded([&] {
        if (!out) throw InvalidArg("null argument");
        if (candidates == 0 || candidates > 0xFFFFFFFFull || n_queries == 0 || n_queries > 0xFFFFFFFFull)
            throw InvalidArg("range plan: sizes out of range");
        const RangePlan pl = plan_range(candidates, n_queries, num_cus);
        out[0] = pl.P; out[1] = pl.part; out[2] = pl.gq; out[3] = pl.run; out[4] = range_query_rows(n_queries);
    });
}

int cph_host_range_tiles(const int64_t* lims, uint64_t n, uint64_t budget_bytes, uint64_t* starts_out, uint64_t* n_tiles_out) {
    return guarded([&] {
        if (!lims || !n_tiles_out || (n && !starts_out)) throw InvalidArg("null argument");
        for (uint64_t i = 0; i < n; ++i)
            if (lims[i + 1] < lims[i]) throw InvalidArg("lims must not descend");
        const std::vector<uint64_t> starts = range_tiles(lims, n, budget_bytes);
        for (size_t i = 0; i < starts.size(); ++i) starts_out[i] = starts[i];
        *n_tiles_out = starts.empty() ? 0 : starts.size() - 1;
    });
}

int cph_host_range_merge_pass(const uint64_t* in, uint64_t* out, uint64_t len, uint64_t width) {
    return guarded([&] {
        if (len && (!in || !out)) throw InvalidArg("null argument");
        if (width == 0) throw InvalidArg("width must be >= 1");
        for (uint64_t i = 0; i < len; ++i)
            out[range_merge_dest(reinterpret_cast<const unsigned long long*>(in), len, width, i)] = in[i];
    });
}

}  // extern "C"

// ---- row map: ids in input rows ------------------------------------------------------------
// Installs (rows != null: validated by the caller) or removes the row map of a finalized handle.  keep_host: also as
// host.rows (what save_native writes); a replica without host arrays keeps the device copy only.
static void install_row_map(cph_index* h, const uint32_t* rows, uint64_t n, bool keep_host) {
    std::lock_guard<std::mutex> lk(h->mu);
    require_finalized(h);
    if (h->tail)
        throw InvalidArg("the index holds " + std::to_string(h->tail) + " added rows, whose input rows are their ids: compact() the "
                         "index before it gets another row map");
    if (rows && n != h->host.n)
        throw InvalidArg("row map has " + std::to_string(n) + " entries, the index holds " + std::to_string(h->host.n));
    h->use_device();
    quiesce(h);                                  // a batch in flight may be reading the old map
    if (!rows) {
        std::vector<uint32_t>().swap(h->host.rows);
        sync_row_map(h);
        return;
    }
    h->d_rows.alloc(n);
    HIP_CHECK(hipMemcpy(h->d_rows.p, rows, n * 4, hipMemcpyHostToDevice));
    if (keep_host) h->host.rows.assign(rows, rows + n);
    h->has_rows = true;
}

static void set_result_ids(cph_index* h, int space) {
    if (space != CPH_IDS_INTERNAL && space != CPH_IDS_INPUT) throw InvalidArg("result id space must be CPH_IDS_INTERNAL or CPH_IDS_INPUT");
    std::lock_guard<std::mutex> lk(h->mu);
    if (space == CPH_IDS_INPUT && !h->has_rows)
        throw InvalidArg("the index has no row map (it was loaded from a v2 file): results in input rows need cph_set_row_map");
    h->use_device();
    quiesce(h);
    h->ids_input = space == CPH_IDS_INPUT;
}

extern "C" {

int cph_has_row_map(cph_index* h, int* flag) {
    return guarded([&] {
        if (!h || !flag) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        *flag = h->finalized && h->has_rows ? 1 : 0;
    });
}

int cph_get_row_map(cph_index* h, uint64_t first, uint64_t count, uint32_t* out) {
    return guarded([&] {
        if (!h || (!out && count != 0)) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        if (!h->has_rows) throw InvalidArg("the index has no row map");
        if (first > h->size() || count > h->size() - first) throw InvalidArg("row map range out of bounds");
        if (count == 0) return;
        h->use_device();
        HIP_CHECK(hipMemcpy(out, h->d_rows.p + first, count * 4, hipMemcpyDeviceToHost));
    });
}

int cph_set_row_map(cph_index* h, const uint32_t* rows, uint64_t n) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_set_row_map");
        if (rows && !is_row_permutation(rows, n)) throw InvalidArg("row map must be a permutation of 0..n-1");
        install_row_map(h, rows, n, true);
    });
}

int cph_set_result_ids(cph_index* h, int space) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        set_result_ids(h, space);
    });
}

int cph_filter_create_rows(cph_index* h, const uint32_t* words, uint64_t n_bits, cph_filter** out) {
    return guarded([&] {
        if (!h || !out || (!words && n_bits != 0)) throw InvalidArg("null argument");
        *out = nullptr;
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        if (!h->has_rows) throw InvalidArg("the index has no row map: a filter in input rows needs one");
        if (n_bits != h->size())
            throw InvalidArg("filter covers " + std::to_string(n_bits) + " rows, the index holds " + std::to_string(h->size()));
        const uint64_t nw = (n_bits + 31) / 32;
        std::vector<uint32_t> w(words, words + nw);
        if (n_bits & 31) w[nw - 1] &= (1u << (n_bits & 31)) - 1u;
        uint64_t pc = 0;                             // (a permutation of the bits: the id bitmap has the same popcount)
        for (uint32_t x : w) pc += (uint64_t)__builtin_popcount(x);
        std::unique_ptr<cph_filter> f(new cph_filter());
        f->device = h->device;
        f->n_bits = n_bits;
        f->popcount = pc;
        h->use_device();
        f->words.alloc(std::max<uint64_t>(nw, 1));
        DevBuf<uint32_t> d_in(std::max<uint64_t>(nw, 1));
        hipStream_t st = own_stream(h);
        HIP_CHECK(hipMemcpyAsync(d_in.p, w.data(), nw * 4, hipMemcpyHostToDevice, st));
        rows_filter(d_in.p, h->d_rows.p, n_bits, f->words.p, st);
        HIP_CHECK(hipStreamSynchronize(st));
        *out = f.release();
    });
}

int cph_host_rows_filter(const uint32_t* words_in, const uint32_t* rows, uint64_t n, uint32_t* words_out) {
    return guarded([&] {
        if (n != 0 && (!words_in || !rows || !words_out)) throw InvalidArg("null argument");
        for (uint64_t i = 0; i < n; ++i)
            if (rows[i] >= n) throw InvalidArg("row out of range");
        rows_filter_host(words_in, rows, n, words_out);
    });
}

}  // extern "C"

// ---- row attributes and the filters made from them -----------------------------------------------------------------
// The label column and the attribute columns: one int32 per row (device_labels.h).  The tag columns: a set of int32 tags per
// row, a canonical CSR (device_tags.h).  All in internal-id order, resident; cph_filters_from_labels / _column / _tags turn
// them into ordinary cph_filter objects, many per device pass, so no search path learns anything new.
namespace {

// A column is given by its values (dense) or by its limits (tags: a column without a tag has no values); else it goes.
bool column_given(uint32_t col, const int32_t* vals, const uint64_t* lims) { return is_tags(col) ? lims != nullptr : vals != nullptr; }

std::string wrong_column_size(uint32_t col, uint64_t n, uint64_t size) {
    return std::string(words_of(col).column) + " has " + std::to_string(n) + (is_tags(col) ? " rows" : " entries") + ", the index holds " +
           std::to_string(size);
}

void require_column_target(const cph_index* h, uint32_t col, bool set, uint64_t n) {
    if (!h->finalized) throw InvalidArg(std::string(words_of(col).plural) + " belong to a finalized index: finalize or load it first");
    if (set && n != h->size()) throw InvalidArg(wrong_column_size(col, n, h->size()));
}

// The caller holds the handle mutex; the handle does not change.  A caller's column of n rows -- dense: vals[n]; tags:
// lims[n + 1] into vals, tags in any order -- as the handle stores it: in internal-id order (input rows go through
// host.rows; a tail row is its own input row), the tags of a row sorted and distinct (tags_canonical_host).
HostColumn column_to_store_locked(const cph_index* h, uint32_t col, const int32_t* vals, const uint64_t* lims, uint64_t n, int space) {
    require_column_target(h, col, true, n);
    const uint64_t nb = h->host.n;
    const bool by_row = space == CPH_IDS_INPUT;
    if (by_row && (!h->has_rows || h->host.rows.size() != nb))
        throw InvalidArg(std::string("the index has no row map (it was loaded from a v2 file): ") + words_of(col).by_row + " cph_set_row_map");
    HostColumn c;
    if (is_tags(col)) {
        tags_canonical_host(lims, vals, n, by_row ? h->host.rows.data() : nullptr, nb, c.lims, c.vals);
    } else if (by_row) {
        c.vals.resize(n);
        labels_to_internal_host(vals, h->host.rows.data(), nb, c.vals.data());
        std::copy(vals + nb, vals + n, c.vals.begin() + nb);
    } else {
        c.vals.assign(vals, vals + n);
    }
    return c;
}

void require_id_space(int space) {
    if (space != CPH_IDS_INTERNAL && space != CPH_IDS_INPUT) throw InvalidArg("id space must be CPH_IDS_INTERNAL or CPH_IDS_INPUT");
}

// cph_set_labels / cph_set_column / cph_set_tags on a handle that keeps its host arrays: rows in internal ids or in input rows.
void set_column(cph_index* h, uint32_t col, const int32_t* vals, const uint64_t* lims, uint64_t n, int space) {
    require_id_space(space);
    std::lock_guard<std::mutex> lk(h->mu);
    if (!column_given(col, vals, lims)) {
        require_column_target(h, col, false, 0);
        install_column_locked(h, col, nullptr, true);
        return;
    }
    HostColumn c = column_to_store_locked(h, col, vals, lims, n, space);
    install_column_locked(h, col, &c, true);
}

// The m filters of one device pass over n ids, all made or none: their bitmaps one behind the other in one allocation
// (`slab`, bitmap j at j * stride words), their counts as the pass left them (`counts`, copied back by the caller, who
// also makes the call's one wait).  The device is current.
struct FilterSlab {
    const uint64_t n, nw, stride;
    std::vector<std::unique_ptr<cph_filter>> made;
    std::shared_ptr<DevBuf<uint32_t>> slab;
    std::vector<unsigned long long> counts;
    FilterSlab(uint64_t n_bits, uint32_t m)
        : n(n_bits), nw((n_bits + 31) / 32), stride((std::max<uint64_t>(nw, 1) + 63) / 64 * 64),      // every bitmap starts on a 256 B line
          made(m), counts(m, 0) {
        for (auto& f : made) f.reset(new cph_filter());
        slab = std::make_shared<DevBuf<uint32_t>>((size_t)m * stride);
    }
    void finish(int device, cph_filter** out) {
        for (size_t j = 0; j < made.size(); ++j) {
            cph_filter* f = made[j].get();
            f->device = device;
            f->n_bits = n;
            f->popcount = counts[j];
            f->slab = slab;
            f->words.p = slab->p + j * stride;
            f->words.n = std::max<uint64_t>(nw, 1);
        }
        for (size_t j = 0; j < made.size(); ++j) out[j] = made[j].release();
    }
};

// cph_filters_from_labels / cph_filters_from_column: out[m] all made, or none.
void filters_from_labels(cph_index* h, uint32_t col, const int32_t* lo, const int32_t* hi, uint32_t m, cph_filter** out) {
    std::lock_guard<std::mutex> lk(h->mu);
    require_finalized(h);
    const RowColumn& c = h->cols[col];
    if (!c.has) throw InvalidArg(no_column(col, true));
    if (m > kLabelMaxFilters) throw InvalidArg("at most " + std::to_string(kLabelMaxFilters) + " label filters per call");
    h->use_device();
    FilterSlab fs(h->size(), m);
    h->d_label_bounds.alloc((size_t)2 * m);
    h->d_label_counts.alloc(m);
    hipStream_t st = own_stream(h);
    HIP_CHECK(hipMemcpyAsync(h->d_label_bounds.p, lo, (size_t)m * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(h->d_label_bounds.p + m, hi, (size_t)m * 4, hipMemcpyHostToDevice, st));
    timed_pass(h->pass_timer[kPassLabels], st, [&] {
        label_filters(c.vals.p, fs.n, h->d_label_bounds.p, h->d_label_bounds.p + m, m, fs.slab->p, fs.stride, h->d_label_counts.p, st);
    });
    HIP_CHECK(hipMemcpyAsync(fs.counts.data(), h->d_label_counts.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));         // the one wait of the call: the routing needs every count on the host
    fs.finish(h->device, out);
}

// cph_filters_from_tags: out[m] all made, or none.  The tests are canonical already.
void filters_from_tags(cph_index* h, uint32_t col, const std::vector<uint32_t>& table, size_t vals_at, uint32_t m, cph_filter** out) {
    std::lock_guard<std::mutex> lk(h->mu);
    require_finalized(h);
    const RowColumn& c = h->cols[col];
    if (!c.has) throw InvalidArg(no_column(col, true));
    h->use_device();
    FilterSlab fs(h->size(), m);
    h->d_tag_tests.alloc(table.size());
    h->d_tag_counts.alloc(m);
    hipStream_t st = own_stream(h);
    HIP_CHECK(hipMemcpyAsync(h->d_tag_tests.p, table.data(), table.size() * 4, hipMemcpyHostToDevice, st));
    timed_pass(h->pass_timer[kPassTags], st, [&] {
        tag_filters(c.lims.p, c.vals.p, fs.n, h->d_tag_tests.p, (uint32_t)vals_at, m, fs.slab->p, fs.stride, h->d_tag_counts.p, st);
    });
    HIP_CHECK(hipMemcpyAsync(fs.counts.data(), h->d_tag_counts.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));         // the one wait of the call: the routing needs every count on the host
    fs.finish(h->device, out);
}

// The caller's tests, canonical and packed for the kernel (before any handle is locked).
void pack_tag_tests(const uint32_t* test_lims, const int32_t* test_vals, const uint8_t* modes, uint32_t m, std::vector<uint32_t>& table,
                    size_t& vals_at) {
    if (m > kTagMaxFilters) throw InvalidArg("at most " + std::to_string(kTagMaxFilters) + " tag filters per call");
    std::vector<uint32_t> tl;
    std::vector<int32_t> tv;
    tag_tests_canonical_host(test_lims, test_vals, modes, m, tl, tv);
    tag_tests_pack_host(tl.data(), tv.data(), modes, m, table, vals_at);
}

// cph_has_labels / cph_has_column / cph_has_tags.
void column_flag(cph_index* h, int kind, uint32_t slot, int* flag) {
    if (!h || !flag) throw InvalidArg("null argument");
    const uint32_t col = facet_column(kind, slot);
    std::lock_guard<std::mutex> lk(h->mu);
    *flag = h->finalized && h->cols[col].has ? 1 : 0;
}

// cph_get_labels / cph_get_column.
void get_column(cph_index* h, uint32_t col, uint64_t first, uint64_t count, int32_t* out) {
    if (!h || (!out && count != 0)) throw InvalidArg("null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    require_finalized(h);
    if (!h->cols[col].has) throw InvalidArg(no_column(col, false));
    if (first > h->size() || count > h->size() - first) throw InvalidArg(col == kLabelColumn ? "label range out of bounds" : "column range out of bounds");
    if (count == 0) return;
    h->use_device();
    HIP_CHECK(hipMemcpy(out, h->cols[col].vals.p + first, count * 4, hipMemcpyDeviceToHost));
}

// cph_filters_from_labels / cph_filters_from_column: the checks of the entry.
void filters_from_labels_entry(cph_index* h, int kind, uint32_t slot, const int32_t* lo, const int32_t* hi, uint32_t m, cph_filter** out) {
    if (m == 0) return;
    if (!out) throw InvalidArg("null argument");
    std::fill(out, out + m, nullptr);
    if (!h || !lo || !hi) throw InvalidArg("null argument");
    filters_from_labels(h, facet_column(kind, slot), lo, hi, m, out);
}

}  // namespace

extern "C" {

int cph_set_labels(cph_index* h, const int32_t* labels, uint64_t n, int space) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_set_labels");
        set_column(h, kLabelColumn, labels, nullptr, n, space);
    });
}

int cph_has_labels(cph_index* h, int* flag) {
    return guarded([&] { column_flag(h, CPH_FACET_LABEL, 0, flag); });
}

int cph_get_labels(cph_index* h, uint64_t first, uint64_t count, int32_t* out) {
    return guarded([&] { get_column(h, kLabelColumn, first, count, out); });
}

int cph_set_column(cph_index* h, uint32_t slot, const int32_t* values, uint64_t n, int space) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_set_column");
        set_column(h, facet_column(CPH_FACET_COLUMN, slot), values, nullptr, n, space);
    });
}

int cph_has_column(cph_index* h, uint32_t slot, int* flag) {
    return guarded([&] { column_flag(h, CPH_FACET_COLUMN, slot, flag); });
}

int cph_get_column(cph_index* h, uint32_t slot, uint64_t first, uint64_t count, int32_t* out) {
    return guarded([&] { get_column(h, facet_column(CPH_FACET_COLUMN, slot), first, count, out); });
}

int cph_filters_from_column(cph_index* h, uint32_t slot, const int32_t* lo, const int32_t* hi, uint32_t m, cph_filter** out) {
    return guarded([&] { filters_from_labels_entry(h, CPH_FACET_COLUMN, slot, lo, hi, m, out); });
}

int cph_filters_from_labels(cph_index* h, const int32_t* lo, const int32_t* hi, uint32_t m, cph_filter** out) {
    return guarded([&] { filters_from_labels_entry(h, CPH_FACET_LABEL, 0, lo, hi, m, out); });
}

int cph_debug_time_label_filters(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassLabels, on != 0); });
}

int cph_debug_last_label_filters_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassLabels, us); });
}

int cph_filter_export(const cph_filter* f, uint32_t* words, uint64_t* count) {
    return guarded([&] {
        if (!f) throw InvalidArg("null filter");
        const uint64_t nw = (f->n_bits + 31) / 32;
        if (count) *count = f->popcount;
        if (!words || nw == 0) return;               // (the count alone: no device call)
        HIP_CHECK(hipSetDevice(f->device));
        HIP_CHECK(hipMemcpy(words, f->words.p, nw * 4, hipMemcpyDeviceToHost));
    });
}

int cph_host_label_filters(const int32_t* labels, uint64_t n, const int32_t* lo, const int32_t* hi, uint32_t m, uint32_t* words_out,
                           uint64_t* counts_out) {
    return guarded([&] {
        if (m == 0) return;
        if ((n != 0 && (!labels || !words_out)) || !lo || !hi || !counts_out) throw InvalidArg("null argument");
        if (n > 0xFFFFFFFFull) throw InvalidArg("filter too large");
        label_filters_host(labels, n, lo, hi, m, words_out, counts_out);
    });
}

int cph_set_tags(cph_index* h, uint32_t slot, const uint64_t* lims, const int32_t* tags, uint64_t n, int space) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_set_tags");
        set_column(h, facet_column(CPH_FACET_TAGS, slot), tags, lims, n, space);
    });
}

int cph_has_tags(cph_index* h, uint32_t slot, int* flag) {
    return guarded([&] { column_flag(h, CPH_FACET_TAGS, slot, flag); });
}

int cph_get_tags(cph_index* h, uint32_t slot, uint64_t first, uint64_t count, uint64_t* lims_out, int32_t* tags_out) {
    return guarded([&] {
        if (!h || !lims_out) throw InvalidArg("null argument");
        const uint32_t col = facet_column(CPH_FACET_TAGS, slot);
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        const RowColumn& c = h->cols[col];
        if (!c.has) throw InvalidArg(no_column(col, false));
        if (first > h->size() || count > h->size() - first) throw InvalidArg("tag row range out of bounds");
        h->use_device();
        std::vector<uint32_t> lims(count + 1);
        HIP_CHECK(hipMemcpy(lims.data(), c.lims.p + first, (count + 1) * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i <= count; ++i) lims_out[i] = (uint64_t)(lims[i] - lims[0]);
        if (tags_out && lims[count] != lims[0])
            HIP_CHECK(hipMemcpy(tags_out, c.vals.p + lims[0], (size_t)(lims[count] - lims[0]) * 4, hipMemcpyDeviceToHost));
    });
}

int cph_filters_from_tags(cph_index* h, uint32_t slot, const uint32_t* test_lims, const int32_t* test_vals, const uint8_t* modes, uint32_t m,
                          cph_filter** out) {
    return guarded([&] {
        if (m == 0) return;
        if (!out) throw InvalidArg("null argument");
        std::fill(out, out + m, nullptr);
        if (!h || !test_lims || !modes) throw InvalidArg("null argument");
        const uint32_t col = facet_column(CPH_FACET_TAGS, slot);
        std::vector<uint32_t> table;
        size_t vals_at = 0;
        pack_tag_tests(test_lims, test_vals, modes, m, table, vals_at);
        filters_from_tags(h, col, table, vals_at, m, out);
    });
}

int cph_debug_time_tag_filters(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassTags, on != 0); });
}

int cph_debug_last_tag_filters_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassTags, us); });
}

int cph_host_tag_filters(const uint32_t* lims, const int32_t* tags, uint64_t n, const uint32_t* test_lims, const int32_t* test_vals,
                         const uint8_t* modes, uint32_t m, uint32_t* words_out, uint64_t* counts_out) {
    return guarded([&] {
        if (m == 0) return;
        if (!lims || (n != 0 && !words_out) || !test_lims || !modes || !counts_out) throw InvalidArg("null argument");
        if (n > 0xFFFFFFFFull) throw InvalidArg("filter too large");
        std::vector<uint64_t> wide(lims, lims + n + 1);
        std::vector<uint32_t> cl, tl;
        std::vector<int32_t> cv, tv;
        tags_canonical_host(wide.data(), tags, n, nullptr, 0, cl, cv);
        tag_tests_canonical_host(test_lims, test_vals, modes, m, tl, tv);
        tag_filters_host(cl.data(), cv.data(), n, tl.data(), tv.data(), modes, m, words_out, counts_out);
    });
}

}  // extern "C"

// ---- facet counts (device_facets.h) -------------------------------------------------------------
// Rows per distinct value of one column under m filters at once: a dictionary per column (made on first use, dropped
// with the column), one counting launch per group of filters, and for `top` one selection launch behind it.
namespace {

// The caller holds the handle mutex.  The dictionary of the column, made now if it is not there: from the host copy of
// the column if that is complete, or (a replica without host arrays) from a copy of the resident one.
FacetDict& facet_dict_locked(cph_index* h, int kind, uint32_t slot) {
    const uint32_t col = facet_column(kind, slot);
    if (!h->finalized) throw InvalidArg("facets belong to a finalized index: finalize or load it first");
    RowColumn& c = h->cols[col];
    if (!c.has) throw InvalidArg(no_column(col, true));
    if (c.facet) return *c.facet;
    h->use_device();
    const uint64_t n = h->size();
    const HostColumn& hc = h->host.cols[col];
    std::vector<int32_t> fetched;
    if (!hc.covers(n)) {
        uint32_t entries = (uint32_t)n;          // dense: one per row; tags: where the last row ends
        if (c.lims.p) HIP_CHECK(hipMemcpy(&entries, c.lims.p + n, 4, hipMemcpyDeviceToHost));
        fetched.resize(entries);
        if (entries) HIP_CHECK(hipMemcpy(fetched.data(), c.vals.p, (size_t)entries * 4, hipMemcpyDeviceToHost));
    }
    const std::vector<int32_t>& src = hc.covers(n) ? hc.vals : fetched;
    std::unique_ptr<FacetDict> d(new FacetDict());
    std::vector<uint32_t> codes;
    facet_dictionary_host(src.data(), src.size(), d->values, codes);
    d->codes.alloc(codes.size());
    d->d_values.alloc(d->values.size());
    if (!codes.empty()) HIP_CHECK(hipMemcpy(d->codes.p, codes.data(), codes.size() * 4, hipMemcpyHostToDevice));
    if (!d->values.empty()) HIP_CHECK(hipMemcpy(d->d_values.p, d->values.data(), d->values.size() * 4, hipMemcpyHostToDevice));
    c.facet = std::move(d);
    return *c.facet;
}

// cph_facet_counts (K == 0: counts_out [m][U]) and cph_facet_top (K >= 1: values_out / counts_out [m][K], found_out [m]).
// Every refusal comes before the first write.  filters: m entries, or null with m == 1; a null entry is "all live rows".
void facet_query(cph_index* h, int kind, uint32_t slot, const cph_filter* const* filters, uint32_t m, uint32_t K, bool top,
                 int32_t* values_out, uint64_t* counts_out, uint32_t* found_out) {
    if (!h) throw InvalidArg("null handle");
    if (top && (K < 1 || K > kFacetTopMax)) throw InvalidArg("facet top must lie in [1, " + std::to_string(kFacetTopMax) + "]");
    if (!filters && m > 1) throw InvalidArg("a null filter list stands for one filter (all live rows): m must be 1");
    std::lock_guard<std::mutex> lk(h->mu);
    facet_column(kind, slot);
    if (!h->finalized) throw InvalidArg("facets belong to a finalized index: finalize or load it first");
    for (uint32_t j = 0; filters && j < m; ++j)
        if (filters[j]) check_filter(h, filters[j]);
    FacetDict& d = facet_dict_locked(h, kind, slot);
    if (m == 0) return;
    if (top ? !values_out || !counts_out || !found_out : (!counts_out && !d.values.empty())) throw InvalidArg("null argument");
    const uint64_t n = h->size();
    const uint32_t U = (uint32_t)d.values.size();
    if (U == 0) {                                   // (an empty index, a tag column without a tag: nothing to launch)
        if (top) {
            std::fill(values_out, values_out + (size_t)m * K, 0);
            std::fill(counts_out, counts_out + (size_t)m * K, 0ull);
            std::fill(found_out, found_out + m, 0u);
        }
        return;
    }
    h->use_device();
    std::vector<std::shared_ptr<const cph_filter>> hold(m);      // F & ~R of a handle with removed rows; null: no bitmap is read
    std::vector<const uint32_t*> tab(m);
    bool any = false;
    for (uint32_t j = 0; j < m; ++j) {
        hold[j] = effective_filter(h, filters ? filters[j] : nullptr);
        tab[j] = hold[j] ? hold[j]->words.p : nullptr;
        any = any || tab[j];
    }
    const uint32_t group = (uint32_t)std::min<uint64_t>({std::max<uint64_t>(h->facet_slab / U, 1), (uint64_t)kFacetMaxFilters, (uint64_t)m});
    const uint32_t* d_lims = h->cols[facet_column(kind, slot)].lims.p;      // (a dense column has none)
    h->d_facet_counts.alloc((size_t)group * U);
    hipStream_t st = own_stream(h);
    if (any) {
        h->d_facet_tab.alloc(m);
        HIP_CHECK(hipMemcpyAsync(h->d_facet_tab.p, tab.data(), (size_t)m * sizeof(tab[0]), hipMemcpyHostToDevice, st));
    }
    if (top) {
        h->d_facet_top_values.alloc((size_t)m * K);
        h->d_facet_top_counts.alloc((size_t)m * K);
        h->d_facet_found.alloc(m);
    }
    std::vector<unsigned long long> staged(top ? (size_t)m * K : 0);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "counters go out as they are");
    // (with more than one group the copies back of all but the last sit inside the timed bracket: the slab is reused)
    timed_pass(h->pass_timer[kPassFacets], st, [&] {
        for (uint32_t g0 = 0; g0 < m; g0 += group) {
            const uint32_t mg = std::min(group, m - g0);
            facet_counts(d.codes.p, d_lims, n, U, any ? h->d_facet_tab.p + g0 : nullptr, mg, h->d_facet_counts.p, kFacetAuto, st);
            if (top)
                facet_top(h->d_facet_counts.p, U, d.d_values.p, mg, K, h->d_facet_top_values.p + (size_t)g0 * K,
                          h->d_facet_top_counts.p + (size_t)g0 * K, h->d_facet_found.p + g0, st);
            else if (g0 + mg < m)
                HIP_CHECK(hipMemcpyAsync(counts_out + (size_t)g0 * U, h->d_facet_counts.p, (size_t)mg * U * 8, hipMemcpyDeviceToHost, st));
        }
    });
    if (top) {
        HIP_CHECK(hipMemcpyAsync(values_out, h->d_facet_top_values.p, (size_t)m * K * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(staged.data(), h->d_facet_top_counts.p, (size_t)m * K * 8, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(found_out, h->d_facet_found.p, (size_t)m * 4, hipMemcpyDeviceToHost, st));
    } else {
        const uint32_t g0 = (m - 1) / group * group;
        HIP_CHECK(hipMemcpyAsync(counts_out + (size_t)g0 * U, h->d_facet_counts.p, (size_t)(m - g0) * U * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));            // the one wait of the call
    if (top) std::copy(staged.begin(), staged.end(), counts_out);
}

// The host-only statements' column: dense (lims null: n_entries == n) or a caller's CSR, canonicalised like cph_set_tags.
struct HostFacetColumn {
    std::vector<uint32_t> lims;                    // tag column: canonical; empty for a dense one
    std::vector<int32_t> values;
    std::vector<uint32_t> codes;
    bool tags = false;
};
void host_facet_column(const int32_t* column, uint64_t n_entries, const uint64_t* lims, uint64_t n, HostFacetColumn& c) {
    if (n >= 0xFFFFFFFFull) throw InvalidArg("facet counts cover fewer than 2^32 - 1 rows");
    c.tags = lims != nullptr;
    if (!lims) {
        if (n_entries != n) throw InvalidArg("a dense facet column has one entry per row");
        facet_dictionary_host(column, n, c.values, c.codes);
        return;
    }
    if (lims[n] != n_entries) throw InvalidArg("facet limits end at " + std::to_string(lims[n]) + ", the column holds " + std::to_string(n_entries));
    std::vector<int32_t> cv;
    tags_canonical_host(lims, column, n, nullptr, 0, c.lims, cv);
    facet_dictionary_host(cv.data(), cv.size(), c.values, c.codes);
}

// words: m bitmaps of (n + 31) / 32 words one behind the other, or null: every filter is "every row".
std::vector<uint64_t> host_facet_counts(const HostFacetColumn& c, uint64_t n, const uint32_t* words, const uint32_t* removed, uint32_t m) {
    const uint64_t nw = (n + 31) / 32, U = c.values.size();
    std::vector<const uint32_t*> fs(m, nullptr);
    for (uint32_t j = 0; words && j < m; ++j) fs[j] = words + (size_t)j * nw;
    std::vector<uint64_t> counts((size_t)m * U);
    facet_counts_host(c.codes.data(), c.tags ? c.lims.data() : nullptr, n, U, words ? fs.data() : nullptr, removed, m, counts.data());
    return counts;
}

}  // namespace

extern "C" {

int cph_facet_onchip_limit(void) { return (int)kFacetLdsBins; }
uint64_t cph_facet_slab_counters(void) { return kFacetSlabCounters; }

int cph_facet_prepare(cph_index* h, int kind, uint32_t slot) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        facet_dict_locked(h, kind, slot);
    });
}

int cph_facet_values(cph_index* h, int kind, uint32_t slot, uint64_t* U, int32_t* values) {
    return guarded([&] {
        if (!h || !U) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        const FacetDict& d = facet_dict_locked(h, kind, slot);
        *U = d.values.size();
        if (values) std::copy(d.values.begin(), d.values.end(), values);
    });
}

int cph_facet_counts(cph_index* h, int kind, uint32_t slot, const cph_filter* const* filters, uint32_t m, uint64_t* counts_out) {
    return guarded([&] { facet_query(h, kind, slot, filters, m, 0, false, nullptr, counts_out, nullptr); });
}

int cph_facet_top(cph_index* h, int kind, uint32_t slot, const cph_filter* const* filters, uint32_t m, uint32_t K, int32_t* values_out,
                  uint64_t* counts_out, uint32_t* found_out) {
    return guarded([&] { facet_query(h, kind, slot, filters, m, K, true, values_out, counts_out, found_out); });
}

int cph_debug_time_facets(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassFacets, on != 0); });
}

int cph_debug_last_facets_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassFacets, us); });
}

int cph_debug_facet_slab(cph_index* h, uint64_t counters) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        h->facet_slab = counters ? counters : kFacetSlabCounters;
    });
}

int cph_host_facet_values(const int32_t* column, uint64_t n_entries, const uint64_t* lims, uint64_t n, uint64_t* U, int32_t* values) {
    return guarded([&] {
        if (!U || (n_entries != 0 && !column)) throw InvalidArg("null argument");
        HostFacetColumn c;
        host_facet_column(column, n_entries, lims, n, c);
        *U = c.values.size();
        if (values) std::copy(c.values.begin(), c.values.end(), values);
    });
}

int cph_host_facet_counts(const int32_t* column, uint64_t n_entries, const uint64_t* lims, uint64_t n, const uint32_t* words,
                          const uint32_t* removed, uint32_t m, uint64_t* counts_out) {
    return guarded([&] {
        if (n_entries != 0 && !column) throw InvalidArg("null argument");
        HostFacetColumn c;
        host_facet_column(column, n_entries, lims, n, c);
        if (m == 0 || c.values.empty()) return;
        if (!counts_out) throw InvalidArg("null argument");
        const std::vector<uint64_t> counts = host_facet_counts(c, n, words, removed, m);
        std::copy(counts.begin(), counts.end(), counts_out);
    });
}

int cph_host_facet_top(const int32_t* column, uint64_t n_entries, const uint64_t* lims, uint64_t n, const uint32_t* words,
                       const uint32_t* removed, uint32_t m, uint32_t K, int32_t* values_out, uint64_t* counts_out, uint32_t* found_out) {
    return guarded([&] {
        if (K < 1 || K > kFacetTopMax) throw InvalidArg("facet top must lie in [1, " + std::to_string(kFacetTopMax) + "]");
        if (n_entries != 0 && !column) throw InvalidArg("null argument");
        HostFacetColumn c;
        host_facet_column(column, n_entries, lims, n, c);
        if (m == 0) return;
        if (!values_out || !counts_out || !found_out) throw InvalidArg("null argument");
        const std::vector<uint64_t> counts = host_facet_counts(c, n, words, removed, m);
        const uint64_t U = c.values.size();
        for (uint32_t j = 0; j < m; ++j)
            facet_top_host(counts.data() + (size_t)j * U, c.values.data(), U, K, values_out + (size_t)j * K, counts_out + (size_t)j * K,
                           found_out + j);
    });
}

// The production launcher on host arrays: codes[n_entries] (< U), lims[n + 1] for a tag column (null: dense, n_entries ==
// n), words: m bitmaps of (n + 31) / 32 words (null: no bitmap at all, every filter is "every row"), uploaded at the slab
// stride.  counts_out: [m * U + CPH_FACET_HOOK_GUARD]: the counters, then the guard words behind them as the device left
// them; everything starts as 0xA5 bytes.
int cph_facet_hook(int device, const uint32_t* codes, uint64_t n_entries, const uint32_t* lims, uint64_t n, uint32_t U,
                   const uint32_t* words, uint32_t m, int path, uint64_t* counts_out, double* kernel_us) {
    return guarded([&] {
        if (m == 0) return;
        if (!counts_out || (n_entries != 0 && !codes)) throw InvalidArg("null argument");
        if (n >= 0xFFFFFFFFull || n_entries > 0xFFFFFFFFull) throw InvalidArg("facet counts cover fewer than 2^32 - 1 rows");
        if (U == 0 || m > kFacetMaxFilters) throw InvalidArg("the hook takes U >= 1 and at most " + std::to_string(kFacetMaxFilters) + " filters");
        if ((uint64_t)m * U > (1ull << 28)) throw InvalidArg("the hook takes at most 2^28 counters");
        if (lims) {                                  // every index the kernel forms is checked here, on the host
            if (lims[0] != 0) throw InvalidArg("facet limits must start at 0");
            for (uint64_t i = 0; i < n; ++i)
                if (lims[i + 1] < lims[i]) throw InvalidArg("facet limits must not decrease (row " + std::to_string(i) + ")");
            if (lims[n] != n_entries) throw InvalidArg("facet limits end at " + std::to_string(lims[n]) + ", the column holds " + std::to_string(n_entries));
        } else if (n_entries != n) {
            throw InvalidArg("a dense facet column has one entry per row");
        }
        for (uint64_t e = 0; e < n_entries; ++e)
            if (codes[e] >= U) throw InvalidArg("facet code out of range (entry " + std::to_string(e) + ")");
        facet_plan(n, U, m, path);                   // (refuses an unknown path, and the on-chip one above its limit)
        HIP_CHECK(hipSetDevice(device));
        const uint64_t nw = (n + 31) / 32, stride = (std::max<uint64_t>(nw, 1) + 63) / 64 * 64;
        const size_t total = (size_t)m * U + CPH_FACET_HOOK_GUARD;
        DevBuf<uint32_t> d_codes(std::max<uint64_t>(n_entries, 1)), d_lims(lims ? n + 1 : 1), d_words(words ? (size_t)m * stride : 1);
        DevBuf<unsigned long long> d_counts(total);
        DevBuf<const uint32_t*> d_tab(m);
        HIP_CHECK(hipMemset(d_counts.p, 0xA5, total * 8));
        if (n_entries) HIP_CHECK(hipMemcpy(d_codes.p, codes, n_entries * 4, hipMemcpyHostToDevice));
        if (lims) HIP_CHECK(hipMemcpy(d_lims.p, lims, (n + 1) * 4, hipMemcpyHostToDevice));
        if (words) {
            HIP_CHECK(hipMemset(d_words.p, 0xA5, (size_t)m * stride * 4));      // (what lies between the bitmaps must not count)
            std::vector<const uint32_t*> tab(m);
            for (uint32_t j = 0; j < m; ++j) {
                tab[j] = d_words.p + (size_t)j * stride;
                if (nw) HIP_CHECK(hipMemcpy(d_words.p + (size_t)j * stride, words + (size_t)j * nw, nw * 4, hipMemcpyHostToDevice));
            }
            HIP_CHECK(hipMemcpy(d_tab.p, tab.data(), (size_t)m * sizeof(tab[0]), hipMemcpyHostToDevice));
        }
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIP_CHECK(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); throw std::runtime_error("hipEventCreate failed"); }
        try {
            HIP_CHECK(hipEventRecord(e0, nullptr));
            facet_counts(d_codes.p, lims ? d_lims.p : nullptr, n, U, words ? d_tab.p : nullptr, m, d_counts.p, path, nullptr);
            HIP_CHECK(hipEventRecord(e1, nullptr));
            HIP_CHECK(hipDeviceSynchronize());
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (kernel_us) *kernel_us = (double)ms * 1e3;
        } catch (...) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            throw;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        HIP_CHECK(hipMemcpy(counts_out, d_counts.p, total * 8, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"

extern "C" {

// ---- filter algebra (cph_filters_combine; device_filter_ops.h) ----
// What a combine call needs on its device and keeps for the next one: a stream of its own (no handle is involved), the
// operand tables and the counts, which only grow.  One call per device at a time (mu).  Never freed: the HIP runtime
// may be gone before a static destructor runs.
struct CombineCtx {
    std::mutex mu;
    hipStream_t stream = nullptr;
    DevBuf<const uint32_t*> tab;
    DevBuf<unsigned long long> counts;
};
static CombineCtx* combine_ctx(int device) {
    static std::mutex mu;
    static std::vector<std::pair<int, CombineCtx*>> all;
    std::lock_guard<std::mutex> lk(mu);
    for (auto& e : all)
        if (e.first == device) return e.second;
    all.emplace_back(device, new CombineCtx());
    return all.back().second;
}

static void check_combine_shape(int op, uint32_t m, const void* b, uint32_t n_b) {
    if (op < 0 || op >= kFilterOps) throw InvalidArg("unknown filter op " + std::to_string(op));
    if (op == kFilterNot) {
        if (n_b != 0 || b) throw InvalidArg("NOT takes one operand list: b must be NULL and n_b 0");
    } else if (!b || (n_b != m && n_b != 1)) {
        throw InvalidArg("the second operand list holds one filter per first operand or exactly one (got " + std::to_string(n_b) +
                         " for " + std::to_string(m) + ")");
    }
}

// cph_filters_combine on one device: out[m] all made, or none.  The operands are complete bitmaps (every call that makes
// a filter waits for it), so nothing is waited for before the launch.
static void filters_combine(int op, const cph_filter* const* a, uint32_t m, const cph_filter* const* b, uint32_t n_b,
                            cph_filter** out) {
    check_combine_shape(op, m, b, n_b);
    for (uint32_t j = 0; j < m; ++j)
        if (!a[j]) throw InvalidArg("null filter");
    for (uint32_t j = 0; j < n_b; ++j)
        if (!b[j]) throw InvalidArg("null filter");
    const int device = a[0]->device;
    const uint64_t n = a[0]->n_bits;
    auto same = [&](const cph_filter* f) {
        if (f->n_bits != n)
            throw InvalidArg("filters of different sizes cannot be combined (" + std::to_string(f->n_bits) + " and " + std::to_string(n) + " ids)");
        if (f->device != device) throw InvalidArg("filters on different devices cannot be combined");
    };
    for (uint32_t j = 0; j < m; ++j) same(a[j]);
    for (uint32_t j = 0; j < n_b; ++j) same(b[j]);
    HIP_CHECK(hipSetDevice(device));
    FilterSlab fs(n, m);
    if (n != 0) {
        CombineCtx* cx = combine_ctx(device);
        std::lock_guard<std::mutex> lk(cx->mu);
        if (!cx->stream) HIP_CHECK(hipStreamCreateWithFlags(&cx->stream, hipStreamNonBlocking));
        std::vector<const uint32_t*> pa(m), pb(n_b);
        for (uint32_t j = 0; j < m; ++j) pa[j] = a[j]->words.p;
        for (uint32_t j = 0; j < n_b; ++j) pb[j] = b[j]->words.p;
        combine_tables(pa.data(), m, pb.data(), n_b, cx->tab, cx->stream);
        cx->counts.alloc(m);
        filter_combine(op, cx->tab.p, n_b ? cx->tab.p + m : nullptr, n_b == 1, n, m, fs.slab->p, fs.stride, cx->counts.p, cx->stream);
        HIP_CHECK(hipMemcpyAsync(fs.counts.data(), cx->counts.p, (size_t)m * 8, hipMemcpyDeviceToHost, cx->stream));
        HIP_CHECK(hipStreamSynchronize(cx->stream));     // the one wait of the call: the routing needs every count on the host
    }
    fs.finish(device, out);
}

int cph_filters_combine(int op, const cph_filter* const* a, uint32_t m, const cph_filter* const* b, uint32_t n_b, cph_filter** out) {
    return guarded([&] {
        if (m == 0) return;
        if (!out) throw InvalidArg("null argument");
        std::fill(out, out + m, nullptr);
        if (!a) throw InvalidArg("null argument");
        filters_combine(op, a, m, b, n_b, out);
    });
}

static void check_combine_host_args(int op, const uint32_t* a_words, const uint32_t* b_words, uint64_t n_bits, const uint32_t* words_out,
                                    const uint64_t* counts_out) {
    if (op < 0 || op >= kFilterOps) throw InvalidArg("unknown filter op " + std::to_string(op));
    if (n_bits > 0xFFFFFFFFull) throw InvalidArg("filter too large");
    if (!counts_out || (n_bits != 0 && (!a_words || !words_out))) throw InvalidArg("null argument");
    if (op == kFilterNot ? b_words != nullptr : (n_bits != 0 && !b_words))
        throw InvalidArg(op == kFilterNot ? "NOT takes one operand: b_words must be NULL" : "null argument");
}

int cph_host_filter_combine(int op, const uint32_t* a_words, const uint32_t* b_words, int b_broadcast, uint64_t n_bits, uint32_t m,
                            uint32_t* words_out, uint64_t* counts_out) {
    return guarded([&] {
        if (m == 0) return;
        check_combine_host_args(op, a_words, b_words, n_bits, words_out, counts_out);
        filter_combine_host(op, a_words, b_words, b_broadcast != 0, n_bits, m, words_out, counts_out);
    });
}

int cph_filter_combine_hook(int device, int op, const uint32_t* a_words, const uint32_t* b_words, int b_broadcast, uint64_t n_bits,
                            uint32_t m, uint32_t* words_out, uint64_t* counts_out, double* kernel_us) {
    return guarded([&] {
        if (m == 0) return;
        check_combine_host_args(op, a_words, b_words, n_bits, words_out, counts_out);
        HIP_CHECK(hipSetDevice(device));
        const uint64_t nw = (n_bits + 31) / 32, stride = (std::max<uint64_t>(nw, 1) + 63) / 64 * 64;
        const uint32_t n_b = op == kFilterNot ? 0u : b_broadcast ? 1u : m;
        // every operand in a slab of its own stride, like a label-filter view; the outputs start as 0xA5 bytes, so
        // every word the kernel leaves alone shows
        DevBuf<uint32_t> d_a((size_t)m * stride), d_b((size_t)std::max(n_b, 1u) * stride), d_out((size_t)m * stride);
        DevBuf<unsigned long long> d_counts(m);
        DevBuf<const uint32_t*> tab;
        HIP_CHECK(hipMemset(d_out.p, 0xA5, (size_t)m * stride * 4));
        HIP_CHECK(hipMemset(d_counts.p, 0xA5, (size_t)m * 8));
        std::vector<const uint32_t*> pa(m), pb(n_b);
        for (uint32_t j = 0; j < m; ++j) {
            pa[j] = d_a.p + (size_t)j * stride;
            if (nw) HIP_CHECK(hipMemcpy(d_a.p + (size_t)j * stride, a_words + (size_t)j * nw, nw * 4, hipMemcpyHostToDevice));
        }
        for (uint32_t j = 0; j < n_b; ++j) {
            pb[j] = d_b.p + (size_t)j * stride;
            if (nw) HIP_CHECK(hipMemcpy(d_b.p + (size_t)j * stride, b_words + (size_t)j * nw, nw * 4, hipMemcpyHostToDevice));
        }
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HIP_CHECK(hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); throw std::runtime_error("hipEventCreate failed"); }
        try {
            combine_tables(pa.data(), m, pb.data(), n_b, tab, nullptr);
            HIP_CHECK(hipEventRecord(e0, nullptr));
            filter_combine(op, tab.p, n_b ? tab.p + m : nullptr, n_b == 1, n_bits, m, d_out.p, stride, d_counts.p, nullptr);
            HIP_CHECK(hipEventRecord(e1, nullptr));
            HIP_CHECK(hipDeviceSynchronize());
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (kernel_us) *kernel_us = (double)ms * 1e3;
        } catch (...) {
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            throw;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        for (uint32_t j = 0; j < m && nw; ++j)
            HIP_CHECK(hipMemcpy(words_out + (size_t)j * nw, d_out.p + (size_t)j * stride, nw * 4, hipMemcpyDeviceToHost));
        std::vector<unsigned long long> counts(m);
        HIP_CHECK(hipMemcpy(counts.data(), d_counts.p, (size_t)m * 8, hipMemcpyDeviceToHost));
        std::copy(counts.begin(), counts.end(), counts_out);
    });
}

// One launch for up to kLeaderGroup single-query callers with the same k: queries gathered into the leader slot's
// pinned, device-mapped buffer, the copy-free small-batch path on the slot's own stream.  The handle mutex is held while
// the launch is ENQUEUED, not while it runs: the next leader's launch (other slot, other stream, its own batch set)
// overlaps this one.  Nobody waits for the launch as a whole: the kernels raise a flag per query in the pinned buffer
// once its results are visible to the host, and every caller waits for its own (wait_search_one).
static void launch_search_group(cph_index* h, cph_index::LeaderSlot& ls, const std::vector<SearchReq*>& group) {
    const uint64_t n = group.size(), kk = group[0]->k;
    const uint64_t t0 = now_ns();
    std::lock_guard<std::mutex> lk(h->mu);
    const uint64_t t1 = now_ns();
    require_finalized(h);
    h->use_device();
    if (!ls.stream) HIP_CHECK(hipStreamCreateWithFlags(&ls.stream, hipStreamNonBlocking));
    const PinnedIo io(n, kk, h->dim, kFlagBytes);
    // (no wait for the set's last batch: the slot is ours alone, nothing in flight reads the old buffer)
    if (grow_pinned(ls.pin, ls.pin_dev, ls.pin_bytes, io.need)) std::memset(ls.pin, 0, kFlagBytes);
    for (uint64_t i = 0; i < n; ++i) std::memcpy(io.queries(ls.pin) + i * h->dim, group[i]->query, h->dim * sizeof(float));
    if (++ls.seq == 0) ls.seq = 1;                                     // (a flag never holds a future launch's number)
    ls.cur_n = n; ls.cur_k = kk;
    BatchSet& s = h->sets[kMaxBatchSets + (&ls - h->leaders)];         // the slot's own set: its launches are ordered by its stream
    init_set(s);
    const float* d_q = metric_queries(h, s, io.queries(ls.pin_dev), n, ls.stream);             // (cosine: normalised into the slot's set)
    stage_queries(h, s, d_q, n, ls.stream);                                                    // the encoder reads the queries over PCIe
    DoneFlags done;
    done.flags = reinterpret_cast<uint32_t*>(ls.pin_dev);
    done.seq = ls.seq;
    // (a handle with removed rows sends its single queries through the batch path, cph_search; a launch that was gathered
    // while the first row was being removed still runs under ~R)
    // (... and so does a handle with added rows; a launch gathered during the first cph_add scans and folds the tail)
    require_tail_k(h, kk);
    enqueue_search(h, s, (uint32_t)n, (uint32_t)kk, io.ids(ls.pin_dev), io.dist(ls.pin_dev), ls.stream, io.counts(ls.pin_dev), done,
                   h->live.get(), d_q);   // ... the search writes the results back
    CPH_TR(0, 1); CPH_TR(1, n); CPH_TR(2, t1 - t0); CPH_TR(3, now_ns() - t1);
}

// Caller `index` of the launch in flight on this slot: wait for ITS query's flag, copy ITS rows out.  A launch lasts as
// long as its longest query; a caller does not have to.  Polls the flag (pinned host memory, written by the kernel behind
// a system-scope fence), looks at the stream every thousand polls so that a launch that died cannot hang its callers,
// and gives the core away once it has spun for a while.
static void wait_search_one(cph_index* h, cph_index::LeaderSlot& ls, uint32_t index, SearchReq& r) {
    const uint64_t t0 = now_ns();
    const uint32_t seq = ls.seq;
    const uint64_t n = ls.cur_n, kk = ls.cur_k;
    const uint32_t* flag = reinterpret_cast<const uint32_t*>(ls.pin) + index;
    const auto spin_start = std::chrono::steady_clock::now();
    bool dev_set = false;
    for (uint64_t it = 1;; ++it) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) break;
        if ((it & 1023) == 0) {
            if (!dev_set) { HIP_CHECK(hipSetDevice(h->device)); dev_set = true; }
            const hipError_t e = hipStreamQuery(ls.stream);
            if (e == hipSuccess) {                 // the stream is idle: the flag is there now, or it never will be
                if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq) break;
                throw std::runtime_error("search launch finished without an answer for this query");
            }
            if (e != hipErrorNotReady) HIP_CHECK(e);
            if (std::chrono::steady_clock::now() - spin_start > std::chrono::microseconds(300)) std::this_thread::yield();
        } else {
            __builtin_ia32_pause();
        }
    }
    const PinnedIo io(n, kk, h->dim, kFlagBytes);
    // the reference returns every result it found (<= max(k,1)); the caller's buffers hold max(k,1) entries
    const uint32_t cnt = io.counts(ls.pin)[index];
    std::memcpy(r.ids, io.ids(ls.pin) + (size_t)index * kk, (size_t)cnt * 8);
    std::memcpy(r.dist, io.dist(ls.pin) + (size_t)index * kk, (size_t)cnt * 4);
    *r.m = cnt;
    CPH_TR(4, now_ns() - t0);
}

int cph_search(cph_index* h, const float* query, uint64_t k, int64_t* ids, float* dist,
               uint64_t* m) {
    SearchReq r{};
    const int rc = guarded([&] {
        if (!h) throw InvalidArg("null handle");
        if (!query || !ids || !dist || !m) throw InvalidArg("null argument");
        const uint64_t kk = std::max<uint64_t>(k, 1);  // api/hnsw_index.hpp:187
        if (kk > 0xFFFFFFFFull) throw InvalidArg("k too large");
        if (h->tombstones.load(std::memory_order_acquire) || h->has_tail.load(std::memory_order_acquire) || h->metric == CPH_METRIC_IP) {
            // inner product: the coalesced path raises a query's completion flag from inside the search kernel, before an
            // epilogue could have run: a batch of one instead (the metric is fixed before the handle holds rows);
            // removed rows: a batch of one through the filtered path under ~R (what a search with filter= does); added
            // rows: a batch of one, so that the tail's scan and fold follow the graph launch
            std::vector<int64_t> ri(kk);
            std::vector<float> rd(kk);
            search_batch(h, batch_call<cph_filter>(query, 1, kk, nullptr, 0, nullptr, false, ri.data(), rd.data()));
            uint64_t cnt = 0;
            for (uint64_t i = 0; i < kk; ++i) cnt += ri[i] >= 0 ? 1 : 0;
            for (uint64_t i = 0, o = 0; i < kk; ++i)
                if (ri[i] >= 0) { ids[o] = ri[i]; dist[o] = rd[i]; ++o; }
            *m = cnt;
            return;
        }
        r.query = query; r.k = kk; r.ids = ids; r.dist = dist; r.m = m;
        // concurrent callers are gathered into shared launches (search_coalescer.h); the status codes it records are cph_status
        h->coal.submit(r,
                       [&](int slot, const std::vector<SearchReq*>& group) { launch_search_group(h, h->leaders[slot], group); },
                       [&](int slot, uint32_t index, SearchReq& me) { wait_search_one(h, h->leaders[slot], index, me); });
    });
    if (rc != CPH_OK) return rc;
    return r.rc == CPH_OK ? CPH_OK : fail(r.rc, r.err);
}

// ---- hooks ---------------------------------------------------------------------------
int cph_encode_query(cph_index* h, const float* query, uint8_t* lut, float* coeffs) {
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);  // the device encoder lives with the loaded index
        h->use_device();
        hipStream_t st = own_stream(h);
        BatchSet& s = next_set(h, st);
        stage_queries(h, s, upload_queries(h, s, query, 1, st, true), 1, st);
        HIP_CHECK(hipEventRecord(s.ev_done, st));
        s.used = true;
        HIP_CHECK(hipStreamSynchronize(st));
        const uint32_t D = h->D, PW = h->L.PW;
        std::vector<uint32_t> masks(PW * 4);
        QueryHeader hd;
        HIP_CHECK(hipMemcpy(masks.data(), s.d_qmasks.p, PW * 16, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(&hd, s.d_qhdr.p, sizeof(hd), hipMemcpyDeviceToHost));
        std::vector<uint8_t> qu(D);
        for (uint32_t d = 0; d < D; ++d) {
            uint8_t u = 0;
            for (int j = 0; j < 4; ++j) u |= (uint8_t)(((masks[(d / 32) * 4 + j] >> (d % 32)) & 1u) << j);
            qu[d] = u;
        }
        qu_to_lut(qu.data(), D, lut);
        coeffs[0] = hd.A; coeffs[1] = hd.B; coeffs[2] = hd.C;
    });
}

int cph_entry_point(cph_index* h, const float* query, uint32_t* entry) {
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        h->use_device();
        hipStream_t st = own_stream(h);
        BatchSet& s = next_set(h, st);
        stage_queries(h, s, upload_queries(h, s, query, 1, st, true), 1, st);
        HIP_CHECK(hipEventRecord(s.ev_done, st));
        s.used = true;
        HIP_CHECK(hipStreamSynchronize(st));
        QueryHeader hd;
        HIP_CHECK(hipMemcpy(&hd, s.d_qhdr.p, sizeof(hd), hipMemcpyDeviceToHost));
        *entry = hd.entry;
    });
}

int cph_fastscan_block(cph_index* h, const uint8_t* lut, const float* qparams, uint32_t vertex,
                       float dist_qp_sq, float worst, int nn_full, uint32_t* sums, uint32_t* msb,
                       float* est, float* lower, float* lower_stage1) {
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        if (vertex >= h->host.n) throw InvalidArg("vertex out of range");      // (a vertex of the graph: an added row has no block)
        h->use_device();
        const uint32_t D = h->D, PW = h->L.PW;
        std::vector<uint8_t> qu(D);
        lut_to_qu(lut, D, qu.data());
        std::vector<uint32_t> masks(PW * 4);
        qu_to_masks(qu.data(), D, masks.data());
        DevBuf<uint4> d_mask;
        DevBuf<uint32_t> d_u;
        DevBuf<float> d_f;
        d_mask.alloc(PW);
        d_u.alloc(64);
        d_f.alloc(96);
        HIP_CHECK(hipMemcpy(d_mask.p, masks.data(), PW * 16, hipMemcpyHostToDevice));
        BlockHookArgs a{};
        a.blk = h->d_blocks.p + (size_t)vertex * h->L.stride;
        a.L = h->L;
        a.qmask = d_mask.p;
        a.qp = QP{qparams[0], qparams[1], qparams[2], qparams[3], qparams[4], qparams[5], qparams[6]};
        a.dqp = dist_qp_sq;
        a.worst = worst;
        a.nn_full = nn_full;
        a.sums = d_u.p; a.msb = d_u.p + 32;
        a.est = d_f.p; a.lower = d_f.p + 32; a.lower1 = d_f.p + 64;
        CPH_LAUNCH(block_hook_kernel, h->bits, D, dim3(1), dim3(64), (size_t)PW * 16, nullptr, a);
        HIP_CHECK(hipDeviceSynchronize());
        uint32_t hu[64];
        float hf[96];
        HIP_CHECK(hipMemcpy(hu, d_u.p, sizeof(hu), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(hf, d_f.p, sizeof(hf), hipMemcpyDeviceToHost));
        std::memcpy(sums, hu, 128); std::memcpy(msb, hu + 32, 128);
        std::memcpy(est, hf, 128); std::memcpy(lower, hf + 32, 128);
        std::memcpy(lower_stage1, hf + 64, 128);
    });
}

int cph_debug_estimator(cph_index* h, const uint8_t* lut, const float* qparams, uint32_t first, uint32_t count, const float* dqp,
                        uint32_t n_dqp, const float* force, const uint32_t* fmask, uint32_t n_sets, uint32_t* out) {
    return guarded([&] {
        if (!lut || !qparams || !dqp || !force || !fmask || !out) throw InvalidArg("bad arguments");
        if (count == 0 || count > 1024 || n_dqp == 0 || n_dqp > 64 || n_sets == 0 || n_sets > 64) throw InvalidArg("bad arguments");
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        if (h->bits < 2) throw InvalidArg("the N-bit estimator: bits must be 2 or 4");
        if ((uint64_t)first + count > h->host.n) throw InvalidArg("vertex out of range");     // (vertices of the graph, like cph_fastscan_block)
        h->use_device();
        const uint32_t D = h->D, PW = h->L.PW;
        std::vector<uint8_t> qu(D);
        lut_to_qu(lut, D, qu.data());
        std::vector<uint32_t> masks(PW * 4);
        qu_to_masks(qu.data(), D, masks.data());
        const size_t words = (size_t)count * n_sets * n_dqp * 6 * 32;
        DevBuf<uint4> d_mask(PW);
        DevBuf<float> d_dqp(n_dqp), d_force((size_t)n_sets * 3);
        DevBuf<uint32_t> d_fmask(n_sets), d_out(words);
        HIP_CHECK(hipMemcpy(d_mask.p, masks.data(), PW * 16, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_dqp.p, dqp, n_dqp * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_force.p, force, (size_t)n_sets * 12, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_fmask.p, fmask, n_sets * 4, hipMemcpyHostToDevice));
        EstimatorTestArgs a{};
        a.blocks = h->d_blocks.p + (size_t)first * h->L.stride;
        a.L = h->L;
        a.qmask = d_mask.p;
        a.qp = QP{qparams[0], qparams[1], qparams[2], qparams[3], qparams[4], qparams[5], qparams[6]};
        a.dqp = d_dqp.p; a.force = d_force.p; a.fmask = d_fmask.p;
        a.n_dqp = n_dqp; a.n_sets = n_sets;
        a.out = d_out.p;
        CPH_LAUNCH(estimator_selftest_kernel, h->bits, D, dim3(count), dim3(64), (size_t)PW * 16, nullptr, a);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, d_out.p, words * 4, hipMemcpyDeviceToHost));
    });
}

int cph_exact_l2(cph_index* h, const float* query, const uint32_t* ids, uint64_t n, float* out) {
    return guarded([&] {
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        if (n == 0) return;
        for (uint64_t i = 0; i < n; ++i)
            if (ids[i] >= h->size()) throw InvalidArg("id out of range");
        h->use_device();
        const uint32_t D = h->D;
        std::vector<float> buf(D, 0.0f);
        std::memcpy(buf.data(), query, h->dim * sizeof(float));
        DevBuf<float> d_q, d_out;
        DevBuf<uint32_t> d_i;
        d_q.alloc(D); d_out.alloc(n); d_i.alloc(n);
        HIP_CHECK(hipMemcpy(d_q.p, buf.data(), D * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_i.p, ids, n * 4, hipMemcpyHostToDevice));
        const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 7) / 8, 1024);
        hipLaunchKernelGGL(exact_l2_hook_kernel, dim3(grid), dim3(64), (size_t)D * 4, nullptr, d_q.p,
                           h->d_raw.p, h->d_norm.p, d_i.p, n, D, d_out.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpy(out, d_out.p, n * 4, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"

// ---- host-only hooks -------------------------------------------------------------------------
extern "C" {

int cph_host_rewrite_index(const char* path_in, const char* path_out) {
    return guarded([&] {
        if (!path_in || !path_out) throw InvalidArg("null argument");
        // peek the header for the parameters a handle would carry
        FILE* f = std::fopen(path_in, "rb");
        if (!f) throw std::runtime_error(std::string("Cannot open file for reading: ") + path_in);
        uint8_t hdr[28];
        const size_t got = std::fread(hdr, 1, sizeof(hdr), f);
        std::fclose(f);
        if (got != sizeof(hdr)) throw std::runtime_error(std::string("Read error or truncated file: ") + path_in);
        uint32_t D, bw, dim;
        std::memcpy(&D, hdr + 12, 4); std::memcpy(&bw, hdr + 20, 4); std::memcpy(&dim, hdr + 24, 4);
        HostIndex hi;
        hi.load(path_in, D, bw, dim);
        hi.save(path_out);
    });
}

int cph_host_repack_block(uint32_t D, uint32_t bits, const uint8_t* ref_block, uint8_t* dev_block,
                          uint64_t* dev_bytes, uint8_t* ref_roundtrip) {
    return guarded([&] {
        if (bits != 1 && bits != 2 && bits != 4) throw InvalidArg("bits must be 1, 2 or 4");
        if (D < 16 || D > 2048 || (D & (D - 1))) throw InvalidArg("D must be a power of two in 16..2048");
        const DevLayout L = make_dev_layout(D, bits);
        const RefLayout RL = make_ref_layout(D, bits);
        repack_ref_to_dev(ref_block, RL, L, dev_block);
        if (dev_bytes) *dev_bytes = L.stride;
        if (ref_roundtrip) repack_dev_to_ref(dev_block, L, RL, ref_roundtrip);
    });
}

int cph_host_relayout_block(uint32_t D, uint32_t bits, const uint8_t* dev_block, uint8_t* resident_block,
                            uint8_t* dev_roundtrip) {
    return guarded([&] {
        if (bits != 1 && bits != 2 && bits != 4) throw InvalidArg("bits must be 1, 2 or 4");
        if (D < 16 || D > 2048 || (D & (D - 1))) throw InvalidArg("D must be a power of two in 16..2048");
        if (!dev_block || !resident_block) throw InvalidArg("null block");
        const DevLayout L = make_dev_layout(D, bits);
        block_plane_to_nib(dev_block, L, resident_block);
        if (dev_roundtrip) block_nib_to_plane(resident_block, L, dev_roundtrip);
    });
}

int cph_export_blocks(cph_index* h, uint64_t first, uint64_t count, int resident, uint8_t* out) {
    return guarded([&] {
        if (!h || !out) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        if (!h->finalized) throw std::runtime_error("Index must be finalized.");
        if (first > h->host.n || count > h->host.n - first) throw InvalidArg("block range out of bounds");      // (blocks of the graph: added rows have none)
        h->use_device();
        quiesce(h);
        const uint8_t* src = h->d_blocks.p + first * h->L.stride;
        if (resident) HIP_CHECK(hipMemcpy(out, src, count * h->L.stride, hipMemcpyDeviceToHost));
        else download_blocks(src, count, h->L, out);
    });
}

int cph_host_encode_query(uint64_t dim, const float* query, uint8_t* lut, float* coeffs, uint32_t* masks) {
    return guarded([&] {
        const size_t D = std::max<size_t>(16, next_pow2(dim));
        if (dim == 0 || D > 2048) throw InvalidArg("unsupported dimension");
        Rotation rot;
        rot.init(D, 42);
        std::vector<float> buf(D, 0.0f);
        std::memcpy(buf.data(), query, dim * sizeof(float));
        EncodedQuery eq;
        encode_query(rot, buf.data(), eq);
        if (lut) qu_to_lut(eq.qu.data(), D, lut);
        if (coeffs) { coeffs[0] = eq.A; coeffs[1] = eq.B; coeffs[2] = eq.C; }
        if (masks) qu_to_masks(eq.qu.data(), D, masks);
    });
}

}  // extern "C"

// ---- streaming FastScan benchmark object ---------------------------------------------------
struct cph_stream {
    int device = 0;
    DevLayout L{};
    RefLayout RL{};
    uint64_t n_blocks = 0;
    DevBuf<uint8_t> d_blocks;
    DevBuf<uint4> d_mask;
    DevBuf<float> d_sink;
    std::vector<uint8_t> lut;
    QP qp{};
    float dqp = 0.0f;
    int num_cus = 256;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace {

__device__ __forceinline__ uint32_t mix32(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return (uint32_t)x;
}

// Fills device-layout blocks with seeded random codes and consistent aux data.
__global__ __launch_bounds__(64) void stream_fill_kernel(uint8_t* blocks, uint64_t n_blocks,
                                                         DevLayout L, uint64_t seed) {
    const int lane = threadIdx.x;
    const int i = lane & 31, h = lane >> 5;
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        uint8_t* blk = blocks + b * L.stride;
        uint32_t pc[4] = {0, 0, 0, 0};  // popcount per plane of neighbour i (this lane's share)
        const uint32_t T = L.BW * L.PW;
        const uint32_t valid_bits = L.D >= 32 ? 32 : L.D;
        const uint32_t vmask = valid_bits == 32 ? 0xFFFFFFFFu : ((1u << valid_bits) - 1u);
        for (uint32_t t = h; t < T; t += 2) {  // the two lanes of a neighbour split its dwords
            const uint32_t plane = t / L.PW;
            uint32_t v = mix32(seed ^ (b * 0x9E3779B97F4A7C15ULL) ^ ((uint64_t)(t * 32 + i) << 20)) & vmask;
            size_t off;
            if (L.wide) {
                const uint32_t ck = t / 4, e = t % 4;
                const uint32_t hh = (L.NH == 2) ? ck / L.CPL : 0;
                const uint32_t k = (L.NH == 2) ? ck % L.CPL : ck;
                off = ((size_t)(k * L.NH * 32 + hh * 32 + i) * 16 + e * 4);
            } else {
                off = ((size_t)t * 32 + i) * 4;
            }
            *reinterpret_cast<uint32_t*>(blk + off) = v;
            const uint32_t c = __popc(v);
            if (plane == 0) pc[0] += c; else if (plane == 1) pc[1] += c;
            else if (plane == 2) pc[2] += c; else pc[3] += c;
        }
        for (int p = 0; p < 4; ++p) pc[p] += __shfl_xor(pc[p], 32);
        if (lane < 32) {
            uint32_t wp = 0;
            for (uint32_t p = 0; p < L.BW; ++p) wp += pc[p] << (L.BW - 1 - p);
            const uint32_t r0 = mix32(seed ^ (b * 1315423911ULL) ^ (0x1000 + i));
            const uint32_t r1 = mix32(seed ^ (b * 2654435761ULL) ^ (0x2000 + i));
            const uint32_t r2 = mix32(seed ^ (b * 40503ULL) ^ (0x3000 + i));
            float nop = 1.0f + 19.0f * (r0 >> 8) * (1.0f / 16777216.0f);
            float ipqo = 0.5f + 0.4f * (r1 >> 8) * (1.0f / 16777216.0f);
            float ipcp = -0.5f + (r2 >> 8) * (1.0f / 16777216.0f);
            uint4 aux = make_uint4(__float_as_uint(nop), __float_as_uint(ipqo), __float_as_uint(ipcp),
                                   (pc[0] & 0xFFFFu) | ((wp & 0xFFFFu) << 16));
            reinterpret_cast<uint4*>(blk + L.aux_off)[i] = aux;
            reinterpret_cast<uint32_t*>(blk + L.ids_off)[i] = mix32(seed ^ b ^ ((uint64_t)i << 40)) >> 1;
            if (lane == 0) *reinterpret_cast<uint32_t*>(blk + L.count_off) = 32u;
        }
    }
}

void stream_launch(cph_stream* s, float* out_est, float* out_lower, uint64_t first, uint64_t count,
                   hipStream_t st) {
    StreamArgs a{};
    a.blocks = s->d_blocks.p;
    a.n_blocks = s->n_blocks;
    a.L = s->L;
    a.qmask = s->d_mask.p;
    a.qp = s->qp;
    a.dqp = s->dqp;
    a.sink = s->d_sink.p;
    a.out_est = out_est;
    a.out_lower = out_lower;
    a.first = first;
    a.count = count;
    static const int mult = getenv("CPH_STREAM_GRID_MULT") ? atoi(getenv("CPH_STREAM_GRID_MULT")) : 32;
    const uint32_t grid = (uint32_t)s->num_cus * mult;
    static const bool pair = !(getenv("CPH_STREAM_PAIR") && atoi(getenv("CPH_STREAM_PAIR")) == 0);
    if (pair && s->L.D == 128 && s->L.BW <= 2) {
        // narrow codes: two blocks per wave iteration, one per lane half (device_stream.h)
        if (s->L.BW == 1) hipLaunchKernelGGL((fastscan_stream_pair_kernel<1>), dim3(grid), dim3(256), 64, st, a);
        else hipLaunchKernelGGL((fastscan_stream_pair_kernel<2>), dim3(grid), dim3(256), 64, st, a);
        HIP_CHECK(hipGetLastError());
        return;
    }
    // (the instantiation with a compile-time D = 1024 holds a whole 16-KB block in registers twice over and loses
    // its occupancy: 0.63 against 0.75 of peak for the runtime-D loop -- the stream kernel uses the latter there)
    const uint32_t dsel = s->L.D == 128 ? 128u : 0u;
    CPH_LAUNCH(fastscan_stream_kernel, s->L.BW, dsel, dim3(grid), dim3(256), (size_t)s->L.PW * 16, st, a);
}

}  // namespace

extern "C" {

int cph_fastscan_stream_create(int device, uint32_t D, uint32_t bits, uint64_t n_blocks,
                               uint64_t seed, cph_stream** out, uint64_t* block_bytes) {
    return guarded([&] {
        *out = nullptr;
        if (bits != 1 && bits != 2 && bits != 4) throw InvalidArg("bits must be 1, 2 or 4");
        if (D < 16 || D > 2048 || (D & (D - 1))) throw InvalidArg("D must be a power of two in 16..2048");
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw std::runtime_error("No HIP device available: the MI355X path has no CPU fallback.");
        HIP_CHECK(hipSetDevice(device));
        auto s = std::unique_ptr<cph_stream>(new cph_stream());
        s->device = device;
        s->L = make_dev_layout(D, bits);
        s->RL = make_ref_layout(D, bits);
        s->n_blocks = n_blocks;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) s->num_cus = prop.multiProcessorCount;
        s->d_blocks.alloc(n_blocks * s->L.stride + 64);
        s->d_mask.alloc(s->L.PW);
        s->d_sink.alloc((size_t)s->num_cus * 64 * 4);
        HIP_CHECK(hipMemset(s->d_sink.p, 0, s->d_sink.n * sizeof(float)));
        hipLaunchKernelGGL(stream_fill_kernel, dim3(s->num_cus * 16), dim3(64), 0, nullptr,
                           s->d_blocks.p, n_blocks, s->L, seed);
        HIP_CHECK(hipGetLastError());
        relayout_blocks(s->d_blocks.p, n_blocks, s->L, true);   // filled in the storage layout
        // one seeded query: random rotated vector -> 4-bit scalars -> masks / LUT / coefficients
        std::mt19937_64 rng(seed * 7919 + 13);
        std::normal_distribution<float> nd(0.0f, 1.0f);
        std::vector<float> q(D);
        for (auto& x : q) x = nd(rng);
        Rotation rot;
        rot.init(D, 42);
        EncodedQuery eq;
        encode_query(rot, q.data(), eq);
        s->lut.resize(D / 4 * 16);
        qu_to_lut(eq.qu.data(), D, s->lut.data());
        std::vector<uint32_t> masks(s->L.PW * 4);
        qu_to_masks(eq.qu.data(), D, masks.data());
        HIP_CHECK(hipMemcpy(s->d_mask.p, masks.data(), masks.size() * 4, hipMemcpyHostToDevice));
        s->qp = QP{eq.A, eq.B, eq.C, 1.0f, 0.0f, 0.0f, 0.05f};
        s->dqp = 140.0f;
        HIP_CHECK(hipEventCreate(&s->ev0));
        HIP_CHECK(hipEventCreate(&s->ev1));
        HIP_CHECK(hipDeviceSynchronize());
        if (block_bytes) *block_bytes = s->L.stride;
        *out = s.release();
    });
}

int cph_fastscan_stream_run(cph_stream* s, int reps, double* avg_ms, double* checksum) {
    return guarded([&] {
        HIP_CHECK(hipSetDevice(s->device));
        if (reps < 1) reps = 1;
        hipStream_t st = nullptr;
        HIP_CHECK(hipEventRecord(s->ev0, st));
        for (int r = 0; r < reps; ++r) stream_launch(s, nullptr, nullptr, 0, 0, st);
        HIP_CHECK(hipEventRecord(s->ev1, st));
        HIP_CHECK(hipEventSynchronize(s->ev1));
        float ms = 0.0f;
        HIP_CHECK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        if (avg_ms) *avg_ms = (double)ms / reps;
        if (checksum) {
            std::vector<float> sink(s->d_sink.n);
            HIP_CHECK(hipMemcpy(sink.data(), s->d_sink.p, sink.size() * 4, hipMemcpyDeviceToHost));
            double t = 0.0;
            for (float x : sink) t += x;
            *checksum = t;
        }
    });
}

int cph_fastscan_stream_export(cph_stream* s, uint64_t first, uint64_t count, uint8_t* ref_blocks,
                               uint8_t* lut, float* qparams, float* dist_qp_sq) {
    return guarded([&] {
        HIP_CHECK(hipSetDevice(s->device));
        if (first + count > s->n_blocks) throw InvalidArg("block range out of bounds");
        if (count && ref_blocks) {
            std::vector<uint8_t> dev(count * s->L.stride);
            download_blocks(s->d_blocks.p + first * s->L.stride, count, s->L, dev.data());
            parallel_for(count, 1024, [&](size_t lo, size_t hi) {
                for (size_t b = lo; b < hi; ++b)
                    repack_dev_to_ref(&dev[b * s->L.stride], s->L, s->RL, ref_blocks + b * s->RL.nb_bytes);
            });
        }
        if (lut) std::memcpy(lut, s->lut.data(), s->lut.size());
        if (qparams) {
            qparams[0] = s->qp.A; qparams[1] = s->qp.B; qparams[2] = s->qp.C;
            qparams[3] = s->qp.affine_a; qparams[4] = s->qp.affine_b; qparams[5] = s->qp.floor;
            qparams[6] = s->qp.slack;
        }
        if (dist_qp_sq) *dist_qp_sq = s->dqp;
    });
}

int cph_fastscan_stream_eval(cph_stream* s, uint64_t first, uint64_t count, float* est, float* lower) {
    return guarded([&] {
        HIP_CHECK(hipSetDevice(s->device));
        if (first + count > s->n_blocks) throw InvalidArg("block range out of bounds");
        if (!count) return;
        DevBuf<float> d_e, d_l;
        d_e.alloc(count * 32);
        d_l.alloc(count * 32);
        stream_launch(s, d_e.p, d_l.p, first, count, nullptr);
        HIP_CHECK(hipMemcpy(est, d_e.p, count * 128, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(lower, d_l.p, count * 128, hipMemcpyDeviceToHost));
    });
}

int cph_fastscan_stream_destroy(cph_stream* s) {
    return guarded([&] {
        if (!s) return;
        (void)hipSetDevice(s->device);
        if (s->ev0) (void)hipEventDestroy(s->ev0);
        if (s->ev1) (void)hipEventDestroy(s->ev1);
        delete s;
    });
}

}  // extern "C"

// ---- one index on several devices: in-process replicas (cph_multi_*, multi_device.h) ------------------------------
// Every replica is a complete cph_index on its device.  Lifecycle calls run on replica 0 (the only one with host
// arrays), then replicas 1..N-1 receive replica 0's device arrays by device-to-device copy.  A batch is split into
// contiguous shards, one per replica, each answered by the existing single-device cph_search_batch[_filtered] on that
// replica's persistent worker thread, straight into the caller's rows.
struct cph_multi {
    std::vector<cph_index*> reps;             // reps[i] on devices[i]; owned (destroy_index)
    std::unique_ptr<ReplicaPool> pool;        // one worker thread per replica
    std::shared_mutex life;                   // searches hold it shared; load / build / finalize / destroy exclusively
    std::atomic<uint64_t> rr{0};              // round robin: whole (small) batches and single queries
    std::atomic<uint64_t> min_shard{kDefaultMinShard};
    std::mutex last_mu;
    std::vector<Shard> last_plan;             // the shards of the last successful cph_multi_search_batch[_filtered]
    ~cph_multi() {
        pool.reset();                         // joins the workers
        for (cph_index* h : reps) destroy_index(h);
    }
};

namespace {

[[noreturn]] void raise_status(int rc, const std::string& msg) {
    if (rc == CPH_INVALID_ARGUMENT) throw InvalidArg(msg);
    if (rc == CPH_OUT_OF_MEMORY) throw std::bad_alloc();
    throw std::runtime_error(msg);
}
void check_rc(int rc) {
    if (rc != CPH_OK) raise_status(rc, g_err);
}

// The host-side scalars of an index (what the search path reads: sizes, entry point, calibration), none of its arrays.
HostIndex host_scalars(const HostIndex& s) {
    HostIndex t;
    t.D = s.D; t.bw = s.bw; t.dim = s.dim; t.n = s.n;
    t.max_level = s.max_level;
    t.entry = s.entry;
    t.upper_tau = s.upper_tau; t.upper_alpha = s.upper_alpha;
    t.mL = s.mL;
    t.seed = s.seed;
    std::memcpy(t.calib, s.calib, sizeof(t.calib));
    std::memcpy(t.profile, s.profile, sizeof(t.profile));
    t.RL = s.RL;
    t.has_dup_neighbors = s.has_dup_neighbors;
    return t;
}

// dst becomes a searchable copy of the finalized src: src's resident device arrays (blocks in the resident layout,
// vectors, norms, the row map, rotation signs, upper layers, their vertex -> row tables and per-edge rows) copied device to device (no peer access needed), its search
// scalars copied, the upper-layer pointers rebased onto dst's own buffers.  dst keeps no host arrays.
void replicate(cph_index* src, cph_index* dst) {
    std::lock_guard<std::mutex> ls(src->mu), ld(dst->mu);
    if (!src->finalized) throw std::runtime_error("replicate: the first replica is not finalized");
    src->use_device();
    HIP_CHECK(hipDeviceSynchronize());          // whatever wrote the source arrays has landed
    begin_device_swap(dst);
    dst->host = host_scalars(src->host);
    dst->host.removed = src->host.removed;      // every replica answers without the removed rows
    dst->host.n_removed = src->host.n_removed;
    drop_host_state(dst);
    dst->L = src->L;
    dst->sc = src->sc;
    dst->flags = src->flags;
    dst->dev_max_level = src->dev_max_level;
    dst->norm_factor = src->norm_factor;
    dst->inv_sqrt_d = src->inv_sqrt_d;
    dst->ip_m2 = src->ip_m2;                    // every replica holds M2: its queries and scores are made against it
    hipStream_t st = own_stream(dst);
    auto copy = [&](auto& d, const auto& s) {
        d.alloc(s.n);
        if (s.n) HIP_CHECK(hipMemcpyPeerAsync(d.p, dst->device, s.p, src->device, s.n * sizeof(*s.p), st));
    };
    copy(dst->d_blocks, src->d_blocks);
    copy(dst->d_raw, src->d_raw);
    copy(dst->d_norm, src->d_norm);
    if (src->has_rows) copy(dst->d_rows, src->d_rows);
    else dst->d_rows.release();
    dst->has_rows = src->has_rows;
    dst->ids_input = dst->ids_input && dst->has_rows;
    for (uint32_t col = 0; col < kFacetColumns; ++col) {                // (compact carries the columns; a load or finalize has none)
        const RowColumn& from = src->cols[col];
        RowColumn& to = dst->cols[col];                                 // (its dictionary went in begin_device_swap)
        to.vals.release();
        to.lims.release();
        if (from.vals.p) copy(to.vals, from.vals);                      // (a column that is not there holds neither buffer,
        if (from.lims.p) copy(to.lims, from.lims);                      //  a dense one no limits, one without a tag no values)
        to.has = from.has;
    }
    copy(dst->d_signs, src->d_signs);
    copy(dst->d_upper, src->d_upper);
    copy(dst->d_row_of, src->d_row_of);
    copy(dst->d_nbr_info, src->d_nbr_info);
    HIP_CHECK(hipStreamSynchronize(st));
    sync_removed(dst);
    auto rebase = [](const uint32_t* p, const DevBuf<uint32_t>& from, const DevBuf<uint32_t>& to) -> const uint32_t* {
        return p ? to.p + (p - from.p) : nullptr;
    };
    for (int l = 0; l < kMaxUpperLayers; ++l) {
        const UpperLayerDev& s = src->layers[l];
        dst->layers[l] = UpperLayerDev{rebase(s.nodes, src->d_upper, dst->d_upper), rebase(s.offsets, src->d_upper, dst->d_upper),
                                       rebase(s.nbrs, src->d_upper, dst->d_upper), rebase(s.row_of, src->d_row_of, dst->d_row_of),
                                       rebase(s.nbr_info, src->d_nbr_info, dst->d_nbr_info), s.n_nodes};
    }
    reset_adaptation(dst);
    dst->finalized = true;
}

// A lifecycle call: `first` on replica 0, then every other replica copies it.  If it fails after replica 0 gave up
// its old index, no replica stays searchable (they would answer from different indexes).
template <class F>
void multi_lifecycle(cph_multi* m, F&& first) {
    std::unique_lock<std::shared_mutex> lk(m->life);
    cph_index* r0 = m->reps[0];
    bool first_done = false;
    try {
        first(r0);
        first_done = true;
        for (size_t i = 1; i < m->reps.size(); ++i) replicate(r0, m->reps[i]);
    } catch (...) {
        if (first_done || !r0->finalized)
            for (cph_index* h : m->reps) {
                std::lock_guard<std::mutex> g(h->mu);
                h->finalized = false;
            }
        throw;
    }
}

size_t shard_index(const std::vector<Shard>& plan, const Shard& s) {
    for (size_t i = 0; i < plan.size(); ++i)
        if (plan[i].replica == s.replica && plan[i].lo == s.lo && plan[i].hi == s.hi) return i;
    throw std::runtime_error("shard not in the plan");
}

// Runs call(shard, its index in the plan) -> cph_status on every shard's worker; a failing shard's status and message
// (thread-local on the worker: `call` has just made the failing cph_* call there) are raised on this thread.
template <class Call>
void run_shards(cph_multi* m, const std::vector<Shard>& plan, Call&& call) {
    std::string err;
    const int rc = m->pool->run(plan, [&](const Shard& s, std::string& e) {
        const int r = call(s, shard_index(plan, s));
        if (r != CPH_OK) e = g_err;
        return r;
    }, err);
    if (rc != CPH_OK) raise_status(rc, err);
}

// The replica fan-out of every batch entry of a cph_multi, all of it before any shard runs (a refusal must not leave half of
// the rows written): under the shared lock, per_replica_check(h, r) on every finalized replica under its mutex (null: no
// replica is visited, every shard's own entry checks its handle), then has_work() -- the checks that need no replica;
// false: nothing to do, and the round robin does not advance.  Then the shards (run_shards); the plan is returned and,
// on success only, becomes the handle's last plan.
using ReplicaCheck = std::function<void(cph_index*, uint32_t)>;
template <class HasWork, class Call>
std::vector<Shard> multi_fan_out(cph_multi* m, uint64_t n, const ReplicaCheck& per_replica_check, HasWork&& has_work, Call&& per_shard_call) {
    if (!m) throw InvalidArg("null handle");
    std::shared_lock<std::shared_mutex> lk(m->life);
    const uint32_t R = (uint32_t)m->reps.size();
    for (uint32_t r = 0; r < R && per_replica_check; ++r) {
        cph_index* h = m->reps[r];
        std::lock_guard<std::mutex> g(h->mu);
        require_finalized(h);
        per_replica_check(h, r);
    }
    if (!has_work()) return {};
    const std::vector<Shard> plan = plan_shards(n, R, m->min_shard.load(), (uint32_t)(m->rr.fetch_add(1) % R));
    run_shards(m, plan, per_shard_call);
    std::lock_guard<std::mutex> g(m->last_mu);
    m->last_plan = plan;
    return plan;
}

// The F filters of replica r in a cph_multi filter list (filters[f * R + r]), as the single-index entries take them.
std::vector<const cph_filter*> replica_filters(const cph_filter* const* filters, uint32_t F, uint32_t R, uint32_t r) {
    std::vector<const cph_filter*> fr(F);
    for (uint32_t f = 0; f < F; ++f) fr[f] = filters[(size_t)f * R + r];
    return fr;
}
void check_replica_filters(cph_index* h, const cph_filter* const* filters, uint32_t F, uint32_t R, uint32_t r) {
    for (const cph_filter* f : replica_filters(filters, F, R, r)) {
        if (!f) throw InvalidArg("a filtered multi-device search needs one filter per replica");
        check_filter(h, f);
    }
}

// cph_multi_search_batch[_filtered | _exact | _filters]: filter_of is sliced with the queries.  The unfiltered call visits
// no replica beforehand.
void multi_search_batch(cph_multi* m, const BatchCall& c) {
    if (!m) throw InvalidArg("null handle");
    const uint64_t n = c.n, k = c.k;
    const uint32_t R = (uint32_t)m->reps.size();
    if (c.F && !c.filters) throw InvalidArg("null argument");
    ReplicaCheck check;
    if (c.F || c.filter_of) check = [&](cph_index* h, uint32_t r) { check_replica_filters(h, c.filters, c.F, R, r); };
    multi_fan_out(m, n, check, [&] {
        if (n && k && !c.filter_of && c.F > 1) throw InvalidArg("null argument");
        if (n && k && c.filter_of) check_filter_of(c.filter_of, n, c.F);
        return true;
    }, [&](const Shard& s, size_t) {
        const std::vector<const cph_filter*> fr = replica_filters(c.filters, c.F, R, s.replica);
        const float* q = c.q ? c.q + s.lo * m->reps[0]->dim_in : nullptr;
        int64_t* oi = c.ids ? c.ids + s.lo * k : nullptr;
        float* od = c.dist ? c.dist + s.lo * k : nullptr;
        cph_index* h = m->reps[s.replica];
        if (c.filter_of) return cph_search_batch_filters(h, q, s.hi - s.lo, k, fr.data(), c.F, c.filter_of + s.lo, c.exact ? 1 : 0, oi, od);
        const cph_filter* f = c.F ? fr[0] : nullptr;
        return c.exact ? cph_search_batch_exact(h, q, s.hi - s.lo, k, f, oi, od) : cph_search_batch_filtered(h, q, s.hi - s.lo, k, f, oi, od);
    });
}

template <class F>
int multi_shared(cph_multi* m, F&& f) {
    if (!m) return fail(CPH_INVALID_ARGUMENT, "null handle");
    std::shared_lock<std::shared_mutex> lk(m->life);
    return f();
}

}  // namespace

extern "C" {

int cph_multi_create(uint64_t dim, uint64_t bits, const int* devices, uint32_t n_dev, cph_multi** out) {
    return guarded([&] {
        if (!out) throw InvalidArg("out must not be null");
        *out = nullptr;
        if (!devices) throw InvalidArg("devices must not be null");
        if (n_dev < 1 || n_dev > kMaxReplicas) throw InvalidArg("n_dev must be 1.." + std::to_string(kMaxReplicas));
        std::unique_ptr<cph_multi> m(new cph_multi());
        for (uint32_t i = 0; i < n_dev; ++i) {
            cph_index* h = nullptr;
            check_rc(cph_create(dim, bits, devices[i], &h));
            h->borrowed = true;
            h->host_less = i > 0;
            m->reps.push_back(h);
        }
        cph_multi* raw = m.get();
        m->pool.reset(new ReplicaPool(n_dev, [raw](uint32_t r) { (void)hipSetDevice(raw->reps[r]->device); }));
        *out = m.release();
    });
}

int cph_multi_destroy(cph_multi* m) {
    return guarded([&] {
        if (!m) return;
        { std::unique_lock<std::shared_mutex> lk(m->life); }   // searches in flight finish first
        delete m;
    });
}

int cph_multi_load(cph_multi* m, const char* path) {
    return guarded([&] {
        if (!m || !path) throw InvalidArg("null argument");
        multi_lifecycle(m, [&](cph_index* r0) { load_v2(r0, path); });
    });
}

int cph_multi_load_native(cph_multi* m, const char* path) {
    return guarded([&] {
        if (!m || !path) throw InvalidArg("null argument");
        multi_lifecycle(m, [&](cph_index* r0) { load_native_file(r0, path); });
    });
}

int cph_multi_save(cph_multi* m, const char* path) {
    return multi_shared(m, [&] { return cph_save(m->reps[0], path); });
}

int cph_multi_save_native(cph_multi* m, const char* path) {
    return multi_shared(m, [&] { return cph_save_native(m->reps[0], path); });
}

int cph_multi_build(cph_multi* m, const float* vectors, uint64_t n) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::unique_lock<std::shared_mutex> lk(m->life);
        build_pending(m->reps[0], vectors, n);
        for (size_t i = 1; i < m->reps.size(); ++i) {   // the old index goes from every replica (finalize copies the new one)
            cph_index* h = m->reps[i];
            std::lock_guard<std::mutex> g(h->mu);
            begin_device_swap(h);
            h->d_blocks.release(); h->d_raw.release(); h->d_norm.release();
            h->host = HostIndex();
            sync_row_map(h);
            sync_columns(h);
            sync_removed(h);
        }
    });
}

int cph_multi_finalize(cph_multi* m) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        multi_lifecycle(m, [&](cph_index* r0) { finalize_build(r0); });
    });
}

int cph_multi_size(cph_multi* m, uint64_t* n) {
    return multi_shared(m, [&] { return cph_size(m->reps[0], n); });
}

int cph_multi_is_finalized(cph_multi* m, int* flag) {
    return multi_shared(m, [&] { return cph_is_finalized(m->reps[0], flag); });
}

int cph_multi_search_batch(cph_multi* m, const float* queries, uint64_t n, uint64_t k, int64_t* ids, float* dist) {
    return cph_multi_search_batch_filtered(m, queries, n, k, nullptr, ids, dist);
}

// (f: one filter per replica, the layout of a list of one filter)
int cph_multi_search_batch_filtered(cph_multi* m, const float* queries, uint64_t n, uint64_t k,
                                    const cph_filter* const* f, int64_t* ids, float* dist) {
    return guarded([&] { multi_search_batch(m, batch_call(queries, n, k, f, f ? 1u : 0u, nullptr, false, ids, dist)); });
}

int cph_multi_search_batch_exact(cph_multi* m, const float* queries, uint64_t n, uint64_t k, const cph_filter* const* f,
                                 int64_t* ids, float* dist) {
    return guarded([&] { multi_search_batch(m, batch_call(queries, n, k, f, f ? 1u : 0u, nullptr, true, ids, dist)); });
}

int cph_multi_search_batch_filters(cph_multi* m, const float* queries, uint64_t n, uint64_t k, const cph_filter* const* filters,
                                   uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids, float* dist) {
    return guarded([&] { multi_search_batch(m, batch_call(queries, n, k, filters, n_filters, filter_of, exact != 0, ids, dist)); });
}

int cph_multi_set_exact_threshold(cph_multi* m, uint64_t max_allowed) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::shared_lock<std::shared_mutex> lk(m->life);
        for (cph_index* h : m->reps) check_rc(cph_set_exact_threshold(h, max_allowed));
    });
}

int cph_multi_search(cph_multi* m, const float* query, uint64_t k, int64_t* ids, float* dist, uint64_t* count) {
    // one replica per caller, round robin: that replica's coalescer gathers its callers (its error text is ours:
    // cph_search runs on this thread)
    return multi_shared(m, [&] { return cph_search(m->reps[m->rr.fetch_add(1) % m->reps.size()], query, k, ids, dist, count); });
}

int cph_multi_has_row_map(cph_multi* m, int* flag) {
    return multi_shared(m, [&] { return cph_has_row_map(m->reps[0], flag); });
}

int cph_multi_set_row_map(cph_multi* m, const uint32_t* rows, uint64_t n) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        if (rows && !is_row_permutation(rows, n)) throw InvalidArg("row map must be a permutation of 0..n-1");
        std::unique_lock<std::shared_mutex> lk(m->life);     // searches in flight finish first
        for (size_t i = 0; i < m->reps.size(); ++i) install_row_map(m->reps[i], rows, n, i == 0);
    });
}

int cph_multi_set_result_ids(cph_multi* m, int space) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::unique_lock<std::shared_mutex> lk(m->life);
        for (cph_index* h : m->reps) set_result_ids(h, space);
    });
}

int cph_multi_set_min_shard(cph_multi* m, uint64_t q) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        if (q == 0) throw InvalidArg("min_shard must be >= 1");
        m->min_shard.store(q);
    });
}

int cph_multi_last_search_stats(cph_multi* m, uint64_t out[12]) {
    return guarded([&] {
        if (!m || !out) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        std::vector<Shard> plan;
        {
            std::lock_guard<std::mutex> g(m->last_mu);
            plan = m->last_plan;
        }
        uint64_t acc[12] = {};
        for (const Shard& s : plan) {
            uint64_t w[12];
            check_rc(cph_last_search_stats(m->reps[s.replica], w));
            for (int i = 0; i < 12; ++i)
                acc[i] = (i == 6 || i == 9) ? std::max(acc[i], w[i]) : acc[i] + w[i];   // kernel_us, capacity: the max
        }
        std::memcpy(out, acc, sizeof(acc));
    });
}

int cph_multi_last_query_expansions(cph_multi* m, uint32_t* out, uint64_t n) {
    return guarded([&] {
        if (!m || !out) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        std::vector<Shard> plan;
        {
            std::lock_guard<std::mutex> g(m->last_mu);
            plan = m->last_plan;
        }
        if (plan.empty() || plan.back().hi != n) throw InvalidArg("n must equal the size of the last batch");
        for (const Shard& s : plan)
            if (s.hi > s.lo) check_rc(cph_last_query_expansions(m->reps[s.replica], out + s.lo, s.hi - s.lo));
    });
}

int cph_multi_num_replicas(cph_multi* m, uint32_t* n) {
    return guarded([&] {
        if (!m || !n) throw InvalidArg("null argument");
        *n = (uint32_t)m->reps.size();
    });
}

int cph_multi_replica(cph_multi* m, uint32_t i, cph_index** out) {
    return guarded([&] {
        if (!m || !out) throw InvalidArg("null argument");
        if (i >= m->reps.size()) throw InvalidArg("replica index out of range");
        *out = m->reps[i];
    });
}

}  // extern "C"

// ---- range search on replicas ---------------------------------------------------------------------------------------------
// The host form over plan_shards: every shard runs the single-device two-step protocol on its replica's worker, begin
// sums the totals, finish lets every shard write behind the hits of the shards before it.
struct cph_multi_range {
    cph_multi* m = nullptr;
    uint64_t n = 0, total = 0;
    std::vector<Shard> plan;
    std::vector<cph_range*> parts;             // one per shard
    std::vector<uint64_t> first;               // hits before shard i
    ~cph_multi_range() {
        for (cph_range* r : parts) (void)cph_range_destroy(r);
    }
};

extern "C" {

int cph_multi_range_search_begin(cph_multi* m, const float* queries, uint64_t n, const float* radius_host, const cph_filter* const* f,
                                 int exact, uint64_t max_results, cph_multi_range** out, uint64_t* total) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        if (!out || !total) throw InvalidArg("null argument");
        *out = nullptr;
        *total = 0;
        refuse_ip(m->reps[0], "range search");
        const uint32_t R = (uint32_t)m->reps.size();
        const uint64_t dim = m->reps[0]->dim;
        std::unique_ptr<cph_multi_range> mr(new cph_multi_range());
        mr->m = m;
        mr->n = n;
        mr->parts.assign(R, nullptr);             // (a plan has at most R shards)
        std::vector<uint64_t> totals(R, 0);
        mr->plan = multi_fan_out(m, n, [&](cph_index* h, uint32_t r) { check_replica_filters(h, f, f ? 1 : 0, R, r); }, [&] {
            if (n && (!queries || !radius_host)) throw InvalidArg("null argument");
            return true;
        }, [&](const Shard& s, size_t i) {
            return cph_range_search_begin(m->reps[s.replica], queries ? queries + s.lo * dim : nullptr, 0, s.hi - s.lo,
                                          radius_host ? radius_host + s.lo : nullptr, f ? f[s.replica] : nullptr, exact, max_results,
                                          nullptr, &mr->parts[i], &totals[i]);
        });
        mr->parts.resize(mr->plan.size());
        mr->first.assign(mr->plan.size() + 1, 0);
        for (size_t i = 0; i < mr->plan.size(); ++i) mr->first[i + 1] = mr->first[i] + totals[i];
        mr->total = mr->first.back();
        *total = mr->total;
        *out = mr.release();
    });
}

int cph_multi_range_search_finish(cph_multi_range* mr, int64_t* lims_host, int64_t* ids, float* dist) {
    return guarded([&] {
        if (!mr || !lims_host) throw InvalidArg("null argument");
        if (mr->total && (!ids || !dist)) throw InvalidArg("null argument");
        cph_multi* m = mr->m;
        std::shared_lock<std::shared_mutex> lk(m->life);
        run_shards(m, mr->plan, [&](const Shard& s, size_t i) {
            std::vector<int64_t> local(s.hi - s.lo + 1);
            const uint64_t at = mr->first[i];
            const int r = cph_range_search_finish(mr->parts[i], local.data(), ids ? ids + at : nullptr, dist ? dist + at : nullptr, 0);
            for (uint64_t j = 0; r == CPH_OK && j < s.hi - s.lo; ++j) lims_host[s.lo + j] = (int64_t)at + local[j];
            return r;
        });
        lims_host[mr->n] = (int64_t)mr->total;
    });
}

int cph_multi_range_destroy(cph_multi_range* mr) {
    return guarded([&] { delete mr; });
}

}  // extern "C"

// ---- one index split across several devices: parts (cph_parts_*, partitioned.h, device_merge.h) ---------------------
// Every part is a complete, ordinary cph_index over a contiguous slice of the input rows, on its own device, returning
// slice-local input rows (CPH_IDS_INPUT).  A search sends the whole batch to every part at once, each on its part's
// persistent worker thread through the existing cph_search_batch_device* entry points, gathers the P result rows on the
// home device (devices[0]) and merges them there with merge_parts_kernel, which also adds every part's first row.
struct cph_parts_filter {
    std::vector<cph_filter*> f;               // f[p]: the slice of part p, made with cph_filter_create_rows on that part
    uint64_t n_bits = 0;                      // rows of the whole index
    ~cph_parts_filter() {
        for (cph_filter* x : f) (void)cph_filter_destroy(x);
    }
};

namespace {

// One part's side of a search: a stream on the part's device and, for a part that does not live on the home device,
// the queries and its rows there, plus the pinned bounce buffer of a pair of devices without peer access.
struct PartScratch {
    hipStream_t st = nullptr;
    DevBuf<float> d_q, d_dist;
    DevBuf<int64_t> d_ids;
    uint8_t* pin = nullptr;
    size_t pin_bytes = 0;
    int peer = -1;                            // peer access between this part's device and the home device: -1 not asked yet
};

}  // namespace

struct cph_parts {
    std::vector<cph_index*> parts;            // parts[p] on devices[p]; owned (destroy_index)
    std::vector<int> devices;
    std::vector<uint64_t> bounds;             // [P + 1]: part p holds input rows [bounds[p], bounds[p + 1]); zeros before build
    std::unique_ptr<ReplicaPool> pool;        // one worker thread per part
    std::shared_mutex life;                   // searches hold it shared; build / finalize / load_native / destroy exclusively
    std::mutex search_mu;                     // one search at a time: the buffers below belong to the handle
    std::vector<PartScratch> scratch;
    // on the home device
    DevBuf<float> h_q, h_part_dist, h_out_dist;
    DevBuf<int64_t> h_part_ids, h_out_ids, h_lo;
    hipStream_t h_st = nullptr;
    hipEvent_t ev_q = nullptr, ev_m0 = nullptr, ev_m1 = nullptr;   // queries ready; around the merge kernel (ev_m1: merged)
    bool merged = false;                      // ev_m0 / ev_m1 have been recorded
    uint64_t last_n = 0;                      // size of the last batch
    ~cph_parts() {
        pool.reset();                         // joins the workers
        for (size_t p = 0; p < scratch.size(); ++p) {
            (void)hipSetDevice(devices[p]);
            if (scratch[p].st) { (void)hipStreamSynchronize(scratch[p].st); (void)hipStreamDestroy(scratch[p].st); }
            if (scratch[p].pin) (void)hipHostFree(scratch[p].pin);
        }
        if (!devices.empty()) (void)hipSetDevice(devices[0]);
        if (ev_m1 && merged) (void)hipEventSynchronize(ev_m1);
        if (h_st) (void)hipStreamDestroy(h_st);
        for (hipEvent_t e : {ev_q, ev_m0, ev_m1})
            if (e) (void)hipEventDestroy(e);
        for (cph_index* h : parts) destroy_index(h);
    }
};

namespace {

std::string part_file(const char* path, uint32_t p, uint32_t P) {
    return std::string(path) + ".p" + std::to_string(p) + "of" + std::to_string(P);
}

bool parts_finalized(cph_parts* m) {
    for (cph_index* h : m->parts) {
        std::lock_guard<std::mutex> g(h->mu);
        if (!h->finalized) return false;
    }
    return true;
}

// After a successful finalize / load_native: the bounds are the prefix sums of the part sizes; lo[P] goes to the home device.
void parts_set_bounds(cph_parts* m) {
    const uint32_t P = (uint32_t)m->parts.size();
    std::vector<int64_t> lo(P);
    m->bounds.assign(P + 1, 0);
    for (uint32_t p = 0; p < P; ++p) {
        lo[p] = (int64_t)m->bounds[p];
        m->bounds[p + 1] = m->bounds[p] + m->parts[p]->host.n;
    }
    HIP_CHECK(hipSetDevice(m->devices[0]));
    if (m->merged) HIP_CHECK(hipEventSynchronize(m->ev_m1));
    m->h_lo.alloc(P);
    HIP_CHECK(hipMemcpy(m->h_lo.p, lo.data(), P * sizeof(int64_t), hipMemcpyHostToDevice));
    m->last_n = 0;
}

// Peer access between a part's device and the home device, asked once per part (before its first search off the home
// device, so that every later decision of that call sees the answer).
void resolve_peer(PartScratch& s, int my_dev, int home_dev) {
    if (s.peer >= 0) return;
    int a = 0, b = 0;
    HIP_CHECK(hipDeviceCanAccessPeer(&a, my_dev, home_dev));
    HIP_CHECK(hipDeviceCanAccessPeer(&b, home_dev, my_dev));
    s.peer = (a && b) ? 1 : 0;
}

// `bytes` from src on src_dev to dst on dst_dev, called on a part's worker whose stream `s.st` lives on one of the two.
// With peer access: a peer copy enqueued on s.st.  Without: through pinned host memory, blocking, after s.st has been
// synchronised (partitioned.h: cross_device_copy); a source that another device's stream wrote (the queries) the caller
// has waited for.  Returns with the worker's device current.
void copy_between(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, PartScratch& s, int my_dev, int home_dev) {
    if (bytes == 0) return;
    resolve_peer(s, my_dev, home_dev);
    CrossDeviceCopy ops;
    ops.peer_async = [&] { HIP_CHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, s.st)); };
    // the blocking copies below run on the null stream, which does not wait for s.st (non-blocking): whatever this
    // worker enqueued there -- the search that writes the rows -- has to be complete before the source is read
    ops.sync_source = [&] { HIP_CHECK(hipStreamSynchronize(s.st)); };
    ops.to_host = [&] {
        if (s.pin_bytes < bytes) {
            if (s.pin) HIP_CHECK(hipHostFree(s.pin));
            s.pin = nullptr;
            s.pin_bytes = 0;
            HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&s.pin), bytes, hipHostMallocPortable));
            s.pin_bytes = bytes;
        }
        HIP_CHECK(hipSetDevice(src_dev));
        HIP_CHECK(hipMemcpy(s.pin, src, bytes, hipMemcpyDeviceToHost));
    };
    ops.from_host = [&] {
        HIP_CHECK(hipSetDevice(dst_dev));
        HIP_CHECK(hipMemcpy(dst, s.pin, bytes, hipMemcpyHostToDevice));
        HIP_CHECK(hipSetDevice(my_dev));
    };
    cross_device_copy(s.peer == 1, ops);
}

// One search of a partitioned index, in every form the entry points offer (on_device: queries and results on the home
// device, the merge enqueued on `stream`).
using PartsCall = BatchCallT<cph_parts_filter>;

void check_parts_filter(cph_parts* m, const cph_parts_filter* f) {
    if (!f) throw InvalidArg("null filter");
    if (f->f.size() != m->parts.size()) throw InvalidArg("filter was made for an index with another number of parts");
    if (f->n_bits != m->bounds.back())
        throw InvalidArg("filter covers " + std::to_string(f->n_bits) + " rows, the index holds " + std::to_string(m->bounds.back()));
}

void parts_search(cph_parts* m, const PartsCall& c) {
    if (!m) throw InvalidArg("null handle");
    std::shared_lock<std::shared_mutex> lk(m->life);
    std::lock_guard<std::mutex> one(m->search_mu);
    const uint32_t P = (uint32_t)m->parts.size();
    const uint64_t n = c.n, k = c.k, dim = m->parts[0]->dim;
    for (uint32_t p = 0; p < P; ++p) {
        cph_index* h = m->parts[p];
        std::lock_guard<std::mutex> g(h->mu);
        require_finalized(h);
        if (!h->ids_input)
            throw InvalidArg("part(" + std::to_string(p) + ") was switched to internal ids: a partitioned index needs its parts in input rows");
    }
    if (c.F && !c.filters) throw InvalidArg("null argument");
    for (uint32_t f = 0; f < c.F; ++f) check_parts_filter(m, c.filters[f]);
    if (n && k && !c.filter_of && c.F > 1) throw InvalidArg("null argument");
    if (n && k && c.filter_of) check_filter_of(c.filter_of, n, c.F);
    if (c.exact && k > kExactMaxK)
        throw InvalidArg("exact search supports k <= " + std::to_string(kExactMaxK) + ", got k = " + std::to_string(k));
    if (n == 0 || k == 0) return;
    if (n > 0xFFFFFFFFull || k >= (1ull << 27) || n * k > (1ull << 40)) throw InvalidArg("batch too large");
    if (!c.q || !c.ids || !c.dist) throw InvalidArg("null argument");

    const int home = m->devices[0];
    HIP_CHECK(hipSetDevice(home));
    if (m->merged) HIP_CHECK(hipEventSynchronize(m->ev_m1));     // the last merge has read the part rows
    if (!m->h_st) {
        HIP_CHECK(hipStreamCreateWithFlags(&m->h_st, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&m->ev_q, hipEventDisableTiming));
        HIP_CHECK(hipEventCreate(&m->ev_m0));
        HIP_CHECK(hipEventCreate(&m->ev_m1));
    }
    m->h_part_ids.alloc((size_t)P * n * k);
    m->h_part_dist.alloc((size_t)P * n * k);
    const float* q_home = c.q;
    hipStream_t mst = c.stream;
    int64_t* out_ids = c.ids;
    float* out_dist = c.dist;
    if (c.on_device) {
        HIP_CHECK(hipEventRecord(m->ev_q, c.stream));
    } else {
        m->h_q.alloc(n * dim);
        m->h_out_ids.alloc(n * k);
        m->h_out_dist.alloc(n * k);
        mst = m->h_st;
        HIP_CHECK(hipMemcpyAsync(m->h_q.p, c.q, n * dim * sizeof(float), hipMemcpyHostToDevice, mst));
        HIP_CHECK(hipEventRecord(m->ev_q, mst));
        q_home = m->h_q.p;
        out_ids = m->h_out_ids.p;
        out_dist = m->h_out_dist.p;
    }

    std::string err;
    const int rc = run_on_parts(*m->pool, P, [&](uint32_t p, std::string& e) -> int {
        cph_index* h = m->parts[p];
        PartScratch& s = m->scratch[p];
        const int dev = m->devices[p];
        HIP_CHECK(hipSetDevice(dev));
        if (!s.st) HIP_CHECK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking));
        // on every way out, an exception included: nothing this part enqueued may still write into the handle's buffers
        // (or read the caller's queries) once the call has returned
        struct Drain {
            hipStream_t st;
            ~Drain() { (void)hipStreamSynchronize(st); }
        } drain{s.st};
        if (dev != home) resolve_peer(s, dev, home);
        int64_t* h_ids = m->h_part_ids.p + (size_t)p * n * k;
        float* h_dist = m->h_part_dist.p + (size_t)p * n * k;
        const float* dq = q_home;
        int64_t* oi = h_ids;
        float* od = h_dist;
        if (dev == home) {
            HIP_CHECK(hipStreamWaitEvent(s.st, m->ev_q, 0));
        } else {
            s.d_q.alloc(n * dim);
            s.d_ids.alloc(n * k);
            s.d_dist.alloc(n * k);
            if (c.on_device) {
                HIP_CHECK(hipEventSynchronize(m->ev_q));
                copy_between(s.d_q.p, dev, q_home, home, n * dim * sizeof(float), s, dev, home);
            } else {
                HIP_CHECK(hipMemcpyAsync(s.d_q.p, c.q, n * dim * sizeof(float), hipMemcpyHostToDevice, s.st));
            }
            dq = s.d_q.p;
            oi = s.d_ids.p;
            od = s.d_dist.p;
        }
        std::vector<const cph_filter*> fr(c.F);
        for (uint32_t f = 0; f < c.F; ++f) fr[f] = c.filters[f]->f[p];
        const cph_filter* one = c.F ? fr[0] : nullptr;
        const int r = c.filter_of ? cph_search_batch_filters_device(h, dq, n, k, fr.data(), c.F, c.filter_of, c.exact ? 1 : 0, oi, od, s.st)
                      : c.exact   ? cph_search_batch_exact_device(h, dq, n, k, one, oi, od, s.st)
                                  : cph_search_batch_device_filtered(h, dq, n, k, one, oi, od, s.st);
        if (r != CPH_OK) {
            e = g_err;                            // (thread-local: this worker's message)
            return r;
        }
        if (dev != home) {
            copy_between(h_ids, home, oi, dev, n * k * sizeof(int64_t), s, dev, home);
            copy_between(h_dist, home, od, dev, n * k * sizeof(float), s, dev, home);
        }
        HIP_CHECK(hipStreamSynchronize(s.st));
        return CPH_OK;
    }, err);
    if (rc != CPH_OK) raise_status(rc, err);

    // every part's rows are on the home device: the merge, then (host form) one copy of [n][k] out
    HIP_CHECK(hipSetDevice(home));
    HIP_CHECK(hipEventRecord(m->ev_m0, mst));
    merge_parts(m->h_part_ids.p, m->h_part_dist.p, P, (uint32_t)n, (uint32_t)k, m->h_lo.p, out_ids, out_dist, mst);
    HIP_CHECK(hipEventRecord(m->ev_m1, mst));
    m->merged = true;
    m->last_n = n;
    if (!c.on_device) {
        HIP_CHECK(hipMemcpyAsync(c.ids, out_ids, n * k * sizeof(int64_t), hipMemcpyDeviceToHost, mst));
        HIP_CHECK(hipMemcpyAsync(c.dist, out_dist, n * k * sizeof(float), hipMemcpyDeviceToHost, mst));
        HIP_CHECK(hipStreamSynchronize(mst));
    }
}

}  // namespace

extern "C" {

int cph_parts_create(uint64_t dim, uint64_t bits, const int* devices, uint32_t n_dev, cph_parts** out) {
    return guarded([&] {
        if (!out) throw InvalidArg("out must not be null");
        *out = nullptr;
        if (!devices) throw InvalidArg("devices must not be null");
        if (n_dev < 1 || n_dev > kMaxReplicas) throw InvalidArg("n_dev must be 1.." + std::to_string(kMaxReplicas));
        std::unique_ptr<cph_parts> m(new cph_parts());
        for (uint32_t i = 0; i < n_dev; ++i) {
            cph_index* h = nullptr;
            check_rc(cph_create(dim, bits, devices[i], &h));
            h->borrowed = true;
            m->parts.push_back(h);
            m->devices.push_back(devices[i]);
        }
        m->bounds.assign(n_dev + 1, 0);
        m->scratch.resize(n_dev);
        cph_parts* raw = m.get();
        m->pool.reset(new ReplicaPool(n_dev, [raw](uint32_t p) { (void)hipSetDevice(raw->devices[p]); }));
        *out = m.release();
    });
}

int cph_parts_destroy(cph_parts* m) {
    return guarded([&] {
        if (!m) return;
        { std::unique_lock<std::shared_mutex> lk(m->life); }   // searches in flight finish first
        delete m;
    });
}

}  // extern "C"

// cph_parts_build; as_given: the rows are stored as they are (cph_parts_compact's live rows under cosine, build_pending).
static void parts_build(cph_parts* m, const float* vectors, uint64_t n, bool as_given) {
    if (!m) throw InvalidArg("null handle");
    const uint32_t P = (uint32_t)m->parts.size();
    if (n < kMinPartRows * P)
        throw InvalidArg("a partitioned index needs at least " + std::to_string(kMinPartRows) + " rows per part: " +
                         std::to_string(n) + " rows for " + std::to_string(P) + " parts");
    if (!vectors) throw InvalidArg("null vectors");
    std::unique_lock<std::shared_mutex> lk(m->life);
    const std::vector<uint64_t> b = all_part_bounds(n, P);
    // cosine: every row is normalised before any part gives up its index -- a bad row refuses the whole call, by its
    // global number
    std::vector<float> unit;
    if (m->parts[0]->metric != CPH_METRIC_L2 && !as_given) {
        std::lock_guard<std::mutex> g(m->parts[0]->mu);
        normalize_rows_in(m->parts[0], vectors, n, 0, unit);
        vectors = unit.data();
    }
    for (uint32_t p = 0; p < P; ++p) build_pending(m->parts[p], vectors + b[p] * m->parts[p]->dim, b[p + 1] - b[p], true);
    m->bounds = b;
}

extern "C" {

int cph_parts_build(cph_parts* m, const float* vectors, uint64_t n) {
    return guarded([&] { parts_build(m, vectors, n, false); });
}

int cph_parts_finalize(cph_parts* m) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::unique_lock<std::shared_mutex> lk(m->life);
        const uint32_t P = (uint32_t)m->parts.size();
        std::string err;
        const int rc = run_on_parts(*m->pool, P, [&](uint32_t p, std::string&) -> int {
            HostThreadsShare share(P);            // P builders at once: each takes 1 / P of the host threads
            finalize_build(m->parts[p]);
            set_result_ids(m->parts[p], CPH_IDS_INPUT);
            return CPH_OK;
        }, err);
        if (rc != CPH_OK) raise_status(rc, err);
        parts_set_bounds(m);
    });
}

int cph_parts_size(cph_parts* m, uint64_t* n) {
    return guarded([&] {
        if (!m || !n) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        *n = 0;
        for (cph_index* h : m->parts) {
            uint64_t x = 0;
            check_rc(cph_size(h, &x));
            *n += x;
        }
    });
}

int cph_parts_is_finalized(cph_parts* m, int* flag) {
    return guarded([&] {
        if (!m || !flag) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        *flag = parts_finalized(m) ? 1 : 0;
    });
}

int cph_parts_num_parts(cph_parts* m, uint32_t* n) {
    return guarded([&] {
        if (!m || !n) throw InvalidArg("null argument");
        *n = (uint32_t)m->parts.size();
    });
}

int cph_parts_part(cph_parts* m, uint32_t i, cph_index** out) {
    return guarded([&] {
        if (!m || !out) throw InvalidArg("null argument");
        if (i >= m->parts.size()) throw InvalidArg("part index out of range");
        *out = m->parts[i];
    });
}

int cph_parts_bounds(cph_parts* m, uint64_t* out) {
    return guarded([&] {
        if (!m || !out) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        std::copy(m->bounds.begin(), m->bounds.end(), out);
    });
}

int cph_parts_save_native(cph_parts* m, const char* path) {
    return guarded([&] {
        if (!m || !path) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        if (!parts_finalized(m)) throw std::runtime_error("Index must be finalized before saving.");
        const uint32_t P = (uint32_t)m->parts.size();
        for (uint32_t p = 0; p < P; ++p) check_rc(cph_save_native(m->parts[p], part_file(path, p, P).c_str()));
    });
}

int cph_parts_load_native(cph_parts* m, const char* path) {
    return guarded([&] {
        if (!m || !path) throw InvalidArg("null argument");
        std::unique_lock<std::shared_mutex> lk(m->life);
        const uint32_t P = (uint32_t)m->parts.size();
        // every file is read and validated before any part gives up its index: a failure leaves the handle untouched
        std::vector<NativeLoaded> loaded(P);
        for (uint32_t p = 0; p < P; ++p) {
            const std::string file = part_file(path, p, P);
            try {
                read_native_for(m->parts[p], file.c_str(), loaded[p]);
                if (loaded[p].t.rows.size() != loaded[p].t.n || loaded[p].t.n == 0)
                    throw std::runtime_error("the part holds no row map (a partitioned index speaks input rows only)");
            } catch (const std::bad_alloc&) {
                throw;
            } catch (const std::exception& e) {
                throw InvalidArg("part " + std::to_string(p) + " of " + std::to_string(P) + " (" + file + "): " + e.what() +
                                 " -- a partitioned index loads the files of save_native on a handle with the same number of parts");
            }
        }
        // the validated files are installed as they were read (no second read).  What can still fail here is the device
        // (allocation, copies): then the parts already replaced stay replaced, every part is marked unfinalized and the
        // handle is not searchable until the next successful load_native or finalize
        try {
            for (uint32_t p = 0; p < P; ++p) {
                install_native(m->parts[p], loaded[p]);
                set_result_ids(m->parts[p], CPH_IDS_INPUT);
            }
            parts_set_bounds(m);
        } catch (...) {
            for (cph_index* h : m->parts) {
                std::lock_guard<std::mutex> g(h->mu);
                h->finalized = false;
            }
            throw;
        }
    });
}

int cph_parts_set_exact_threshold(cph_parts* m, uint64_t max_allowed) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::shared_lock<std::shared_mutex> lk(m->life);
        for (cph_index* h : m->parts) check_rc(cph_set_exact_threshold(h, max_allowed));
    });
}

int cph_parts_filter_create_rows(cph_parts* m, const uint32_t* words, uint64_t n_bits, cph_parts_filter** out) {
    return guarded([&] {
        if (!m || !out || (!words && n_bits != 0)) throw InvalidArg("null argument");
        *out = nullptr;
        std::shared_lock<std::shared_mutex> lk(m->life);
        if (!parts_finalized(m)) throw std::runtime_error("Search failed: invalid entry point after finalize.");
        if (n_bits != m->bounds.back())
            throw InvalidArg("filter covers " + std::to_string(n_bits) + " rows, the index holds " + std::to_string(m->bounds.back()));
        std::unique_ptr<cph_parts_filter> f(new cph_parts_filter());
        f->n_bits = n_bits;
        for (size_t p = 0; p < m->parts.size(); ++p) {
            const std::vector<uint32_t> w = cut_mask(words, m->bounds[p], m->bounds[p + 1]);
            cph_filter* x = nullptr;
            check_rc(cph_filter_create_rows(m->parts[p], w.data(), m->bounds[p + 1] - m->bounds[p], &x));
            f->f.push_back(x);
        }
        *out = f.release();
    });
}

int cph_parts_filter_destroy(cph_parts_filter* f) {
    return guarded([&] { delete f; });
}

int cph_parts_search_batch(cph_parts* m, const float* queries, uint64_t n, uint64_t k, int64_t* ids, float* dist) {
    return cph_parts_search_batch_filtered(m, queries, n, k, nullptr, ids, dist);
}

int cph_parts_search_batch_filtered(cph_parts* m, const float* queries, uint64_t n, uint64_t k, const cph_parts_filter* f,
                                    int64_t* ids, float* dist) {
    return guarded([&] { parts_search(m, batch_call(queries, n, k, &f, f ? 1u : 0u, nullptr, false, ids, dist)); });
}

int cph_parts_search_batch_exact(cph_parts* m, const float* queries, uint64_t n, uint64_t k, const cph_parts_filter* f,
                                 int64_t* ids, float* dist) {
    return guarded([&] { parts_search(m, batch_call(queries, n, k, &f, f ? 1u : 0u, nullptr, true, ids, dist)); });
}

int cph_parts_search_batch_filters(cph_parts* m, const float* queries, uint64_t n, uint64_t k,
                                   const cph_parts_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact,
                                   int64_t* ids, float* dist) {
    return guarded([&] { parts_search(m, batch_call(queries, n, k, filters, n_filters, filter_of, exact != 0, ids, dist)); });
}

int cph_parts_search_batch_device(cph_parts* m, const float* d_queries, uint64_t n, uint64_t k, int64_t* d_ids, float* d_dist,
                                  void* stream) {
    return cph_parts_search_batch_device_filtered(m, d_queries, n, k, nullptr, d_ids, d_dist, stream);
}

int cph_parts_search_batch_device_filtered(cph_parts* m, const float* d_queries, uint64_t n, uint64_t k, const cph_parts_filter* f,
                                           int64_t* d_ids, float* d_dist, void* stream) {
    return guarded([&] { parts_search(m, batch_call(d_queries, n, k, &f, f ? 1u : 0u, nullptr, false, d_ids, d_dist, true, stream)); });
}

int cph_parts_search_batch_exact_device(cph_parts* m, const float* d_queries, uint64_t n, uint64_t k, const cph_parts_filter* f,
                                        int64_t* d_ids, float* d_dist, void* stream) {
    return guarded([&] { parts_search(m, batch_call(d_queries, n, k, &f, f ? 1u : 0u, nullptr, true, d_ids, d_dist, true, stream)); });
}

int cph_parts_search_batch_filters_device(cph_parts* m, const float* d_queries, uint64_t n, uint64_t k,
                                          const cph_parts_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                                          int exact, int64_t* d_ids, float* d_dist, void* stream) {
    return guarded([&] {
        parts_search(m, batch_call(d_queries, n, k, filters, n_filters, filter_of, exact != 0, d_ids, d_dist, true, stream));
    });
}

int cph_parts_search(cph_parts* m, const float* query, uint64_t k, int64_t* ids, float* dist, uint64_t* count) {
    return guarded([&] {
        if (!m || !query || !ids || !dist || !count) throw InvalidArg("null argument");
        const uint64_t kk = std::max<uint64_t>(k, 1);
        std::vector<int64_t> ri(kk);
        std::vector<float> rd(kk);
        parts_search(m, batch_call<cph_parts_filter>(query, 1, kk, nullptr, 0, nullptr, false, ri.data(), rd.data()));
        uint64_t cnt = 0;
        while (cnt < kk && ri[cnt] >= 0) ++cnt;       // the merge keeps padding last
        std::copy(ri.begin(), ri.begin() + cnt, ids);
        std::copy(rd.begin(), rd.begin() + cnt, dist);
        *count = cnt;
    });
}

int cph_parts_last_search_stats(cph_parts* m, uint64_t out[13]) {
    return guarded([&] {
        if (!m || !out) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        std::lock_guard<std::mutex> one(m->search_mu);
        uint64_t acc[13] = {};
        if (m->last_n) {
            for (cph_index* h : m->parts) {
                uint64_t w[12];
                check_rc(cph_last_search_stats(h, w));
                for (int i = 0; i < 12; ++i)
                    acc[i] = (i == 6 || i == 9) ? std::max(acc[i], w[i]) : acc[i] + w[i];   // kernel_us, capacity: the max
            }
            HIP_CHECK(hipSetDevice(m->devices[0]));
            HIP_CHECK(hipEventSynchronize(m->ev_m1));
            float ms = 0.0f;
            HIP_CHECK(hipEventElapsedTime(&ms, m->ev_m0, m->ev_m1));
            acc[12] = (uint64_t)(ms * 1000.0);
        }
        std::memcpy(out, acc, sizeof(acc));
    });
}

int cph_parts_last_query_expansions(cph_parts* m, uint32_t* out, uint64_t n) {
    return guarded([&] {
        if (!m || !out) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        std::lock_guard<std::mutex> one(m->search_mu);
        if (m->last_n == 0 || n != m->last_n) throw InvalidArg("n must equal the size of the last batch");
        std::vector<uint32_t> w(n);
        std::fill(out, out + n, 0u);
        for (cph_index* h : m->parts) {
            check_rc(cph_last_query_expansions(h, w.data(), n));
            for (uint64_t i = 0; i < n; ++i) out[i] += w[i];
        }
    });
}

int cph_merge_rows_hook(int device, const int64_t* ids, const float* dist, uint32_t P, uint64_t n, uint64_t k, const int64_t* lo,
                        int64_t* out_ids, float* out_dist) {
    return guarded([&] {
        if (!ids || !dist || !lo || !out_ids || !out_dist) throw InvalidArg("null argument");
        if (P < 1 || P > kMaxReplicas) throw InvalidArg("P must be 1.." + std::to_string(kMaxReplicas));
        if (n < 1 || n > 0xFFFFFFFFull || k < 1 || k >= (1ull << 27) || n * k > (1ull << 32)) throw InvalidArg("merge: sizes out of range");
        HIP_CHECK(hipSetDevice(device));
        const size_t rows = (size_t)n * k;
        DevBuf<int64_t> d_ids(P * rows), d_out_ids(rows), d_lo(P);
        DevBuf<float> d_dist(P * rows), d_out_dist(rows);
        HIP_CHECK(hipMemcpy(d_ids.p, ids, P * rows * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_dist.p, dist, P * rows * sizeof(float), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_lo.p, lo, P * sizeof(int64_t), hipMemcpyHostToDevice));
        // (the caller's output arrives first: a slot the kernel left out would keep what the caller put there)
        HIP_CHECK(hipMemcpy(d_out_ids.p, out_ids, rows * sizeof(int64_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_out_dist.p, out_dist, rows * sizeof(float), hipMemcpyHostToDevice));
        merge_parts(d_ids.p, d_dist.p, P, (uint32_t)n, (uint32_t)k, d_lo.p, d_out_ids.p, d_out_dist.p, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out_ids, d_out_ids.p, rows * sizeof(int64_t), hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(out_dist, d_out_dist.p, rows * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int cph_host_part_bounds(uint64_t n, uint32_t P, uint64_t* out) {
    return guarded([&] {
        if (!out) throw InvalidArg("null argument");
        if (P < 1 || P > kMaxReplicas) throw InvalidArg("P must be 1.." + std::to_string(kMaxReplicas));
        const std::vector<uint64_t> b = all_part_bounds(n, P);
        std::copy(b.begin(), b.end(), out);
    });
}

}  // extern "C"

// ---- removed rows: tombstones and compact() (cph_remove, cph_compact; device_tombstone.h) ---------------------------------
// R lives on the handle as a resident bitmap over internal ids (host copy: host.removed).  The search kernels are not
// told: every search entry substitutes the effective filter F & ~R (effective_filter) and runs the filtered, exact or
// per-query path as it is.
namespace {

// cph_remove on one handle: ids in internal ids or (space == CPH_IDS_INPUT) input rows, validated before anything
// changes; returns the number of ids newly removed.
uint64_t remove_ids(cph_index* h, const int64_t* ids, uint64_t m, int space) {
    if (space != CPH_IDS_INTERNAL && space != CPH_IDS_INPUT) throw InvalidArg("id space must be CPH_IDS_INTERNAL or CPH_IDS_INPUT");
    if (m && !ids) throw InvalidArg("null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    require_finalized(h);
    if (space == CPH_IDS_INPUT && !h->has_rows)
        throw InvalidArg("the index has no row map (it was loaded from a v2 file): removing input rows needs cph_set_row_map");
    const uint64_t n = h->size(), nw = (n + 31) / 32;
    std::vector<uint32_t> list(m);
    for (uint64_t i = 0; i < m; ++i) {
        if (ids[i] < 0 || (uint64_t)ids[i] >= n)
            throw InvalidArg("remove: id " + std::to_string(ids[i]) + " is outside [0, " + std::to_string(n) + ")");
        list[i] = (uint32_t)ids[i];
    }
    h->use_device();
    quiesce(h);                                  // a batch in flight may be reading R, or a filter made from it
    if (m == 0) return 0;
    hipStream_t st = own_stream(h);
    DevBuf<uint32_t> d_list(m), d_mark(nw), d_conv;
    HIP_CHECK(hipMemcpyAsync(d_list.p, list.data(), m * 4, hipMemcpyHostToDevice, st));
    mark_ids(d_list.p, m, n, d_mark.p, st);
    const uint32_t* d_fresh = d_mark.p;
    if (space == CPH_IDS_INPUT) {                // a row bitmap: through the row map, like a filter in input rows
        d_conv.alloc(nw);
        rows_filter(d_mark.p, h->d_rows.p, n, d_conv.p, st);
        d_fresh = d_conv.p;
    }
    // the new R is folded in a scratch copy: until everything below has succeeded, the handle's R (resident bitmap, host
    // copy, count, epoch, cached filters) is the old one, all of it
    DevBuf<uint32_t> d_next(nw);
    if (h->host.n_removed == 0) HIP_CHECK(hipMemsetAsync(d_next.p, 0, nw * 4, st));
    else HIP_CHECK(hipMemcpyAsync(d_next.p, h->d_removed.p, nw * 4, hipMemcpyDeviceToDevice, st));
    h->d_rm_count.alloc(1);
    fold_removed(d_next.p, d_fresh, n, h->d_rm_count.p, st);
    unsigned long long newly = 0;
    std::vector<uint32_t> next(nw);
    HIP_CHECK(hipMemcpyAsync(&newly, h->d_rm_count.p, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(next.data(), d_next.p, nw * 4, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    if (newly == 0) return 0;
    h->host.removed.swap(next);                  // (nothing below this line and above sync_removed throws)
    h->host.n_removed += newly;
    sync_removed(h);                             // uploads the host copy: the resident bitmap is made from what save_native writes
    return newly;
}

// One column of the live rows as compact gathers it, in the form the setters take: vals, and for a tag column lims (without
// the leading 0 until set_live_columns adds it).  has: the handle holds the column, which a tag column over zero live rows
// could not show otherwise.
struct LiveColumn {
    std::vector<int32_t> vals;
    std::vector<uint64_t> lims;
    bool has = false;
};
using LiveColumns = LiveColumn[kFacetColumns];

// The live vectors of a finalized handle in input-row order (internal-id order without a row map), appended to `vecs`
// (dim floats each); map[i] (the caller's, `n` entries from map_first on) = first_new + rank of the live row, -1 for a
// removed one, indexed by input row (by_row) or by internal id.  cols (may be null): the live rows' values in every column
// the handle holds, appended in the same order.  Returns the number of live rows.
uint64_t gather_live(cph_index* h, std::vector<float>& vecs, int64_t* map, bool by_row, int64_t first_new, LiveColumns* cols = nullptr) {
    const HostIndex& hi = h->host;
    const uint64_t n = hi.n, size = h->size();
    const bool rows = h->has_rows && hi.rows.size() == n;
    if (by_row && !rows) throw InvalidArg("the index has no row map");
    std::vector<uint32_t> id_of_row(n);
    for (uint64_t i = 0; i < n; ++i) id_of_row[rows ? hi.rows[i] : i] = (uint32_t)i;
    uint64_t live = 0;
    for (uint64_t r = 0; r < size; ++r) {        // the base rows, then the added rows in id order (each its own input row)
        const uint32_t id = r < n ? id_of_row[r] : (uint32_t)r;
        const bool gone = hi.n_removed != 0 && ((hi.removed[id >> 5] >> (id & 31)) & 1u);
        map[by_row ? r : id] = gone ? -1 : first_new + (int64_t)live;
        if (gone) continue;
        vecs.insert(vecs.end(), row_vec(h, id), row_vec(h, id) + hi.dim);
        for (uint32_t col = 0; cols && col < kFacetColumns; ++col) {
            const HostColumn& hc = hi.cols[col];
            if (!hc.covers(size)) continue;
            LiveColumn& to = (*cols)[col];
            to.has = true;
            to.vals.insert(to.vals.end(), hc.vals.begin() + hc.row_begin(id), hc.vals.begin() + hc.row_end(id));
            if (is_tags(col)) to.lims.push_back(to.vals.size());
        }
        ++live;
    }
    return live;
}

// After a compact: the gathered columns go back in.  New input row j holds the values of the live row it came from; set(col,
// vals, lims) is the caller's setter over input rows.
template <class Set>
void set_live_columns(LiveColumns& cols, Set&& set) {
    for (uint32_t col = 0; col < kFacetColumns; ++col) {
        LiveColumn& c = cols[col];
        if (!c.has) continue;
        if (is_tags(col)) c.lims.insert(c.lims.begin(), 0);
        set(col, c.vals.data(), is_tags(col) ? c.lims.data() : nullptr);
    }
}

// cph_compact on one handle (a lifecycle call, like build + finalize).
void compact_index(cph_index* h, int64_t* old_to_new) {
    if (!old_to_new) throw InvalidArg("null argument");
    refuse_host_less(h, "cph_compact");
    std::vector<float> vecs;
    LiveColumns cols;                            // the live rows' values in every column, in the order of the new input rows
    uint64_t live = 0;
    bool was_input = false;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        // the builder's own refusals, before the handle gives anything up
        live = h->size() - h->host.n_removed;
        require_buildable(live);
        require_finalizable(live);
        was_input = h->ids_input;
        vecs.reserve(live * h->dim);
        std::vector<int64_t> map(h->size());
        gather_live(h, vecs, map.data(), was_input, 0, &cols);
        std::copy(map.begin(), map.end(), old_to_new);
    }
    build_pending(h, vecs.data(), live, true);   // (cosine: the live rows are unit-half rows already)
    std::vector<float>().swap(vecs);
    finalize_build(h);
    if (was_input) set_result_ids(h, CPH_IDS_INPUT);
    set_live_columns(cols, [&](uint32_t col, const int32_t* vals, const uint64_t* lims) { set_column(h, col, vals, lims, live, CPH_IDS_INPUT); });
}

}  // namespace

extern "C" {

int cph_remove(cph_index* h, const int64_t* ids, uint64_t m, int space, uint64_t* newly) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_remove");
        const uint64_t c = remove_ids(h, ids, m, space);
        if (newly) *newly = c;
    });
}

int cph_live_count(cph_index* h, uint64_t* n) {
    return guarded([&] {
        if (!h || !n) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        *n = h->needs_build ? h->pending_n : h->size() - h->host.n_removed;
    });
}

int cph_get_removed(cph_index* h, uint32_t* words) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        const uint64_t nw = (h->size() + 31) / 32;
        if (nw && !words) throw InvalidArg("null argument");
        if (h->host.n_removed == 0) std::fill(words, words + nw, 0u);
        else std::copy(h->host.removed.begin(), h->host.removed.end(), words);
    });
}

int cph_compact(cph_index* h, int64_t* old_to_new) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_compact");
        compact_index(h, old_to_new);
    });
}

}  // extern "C"

// ---- added rows: the tail (cph_add; device_tail.h) -------------------------------------------------------------------------
namespace {

// Makes `b` hold `want` elements, keeping its first `keep`; the copy runs on `st`, which has drained before the old
// buffer is freed.
template <class T>
void grow_keep(DevBuf<T>& b, size_t keep, size_t want, hipStream_t st) {
    if (b.p && b.n >= want) return;
    DevBuf<T> nb(want);
    if (keep) HIP_CHECK(hipMemcpyAsync(nb.p, b.p, keep * sizeof(T), hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    b = std::move(nb);
}

// cph_add on one handle; returns the id of the first new row.
uint64_t add_rows(cph_index* h, const float* vectors, uint64_t m, const int32_t* labels) {
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->finalized) throw InvalidArg("rows are added to a finalized index: finalize or load it first");
    const uint64_t size = h->size(), need = size + m;
    if (m == 0) return size;
    if (!vectors) throw InvalidArg("null vectors");
    RowColumn& lab = h->cols[kLabelColumn];
    std::vector<int32_t>& host_labels = h->host.cols[kLabelColumn].vals;
    if ((labels != nullptr) != lab.has)
        throw InvalidArg(lab.has ? "the index has a label column: the added rows need labels"
                                       : "the index has no label column: labels for the added rows have nowhere to go");
    if (has_columns(h, CPH_FACET_COLUMN))
        throw InvalidArg("the index holds attribute columns and the added rows would have no values in them: drop the columns "
                         "(cph_set_column with NULL), add, then set them again at the new size");
    if (has_columns(h, CPH_FACET_TAGS))
        throw InvalidArg("the index holds tag columns and the added rows would have no tags in them: drop the columns "
                         "(cph_set_tags with NULL), add, then set them again at the new size");
    if (need >= 0xFFFFFFFFull) throw InvalidArg("too many vectors");
    std::vector<float> unit;                     // cosine: the rows as the index stores them (a bad row refuses the call here)
    if (h->metric == CPH_METRIC_IP) {            // (inner product: against the M2 of the index)
        ip_rows_in(h, vectors, m, &h->ip_m2, true, unit);
        vectors = unit.data();
    } else if (h->metric != CPH_METRIC_L2) {
        normalize_rows_in(h, vectors, m, 0, unit);
        vectors = unit.data();
    }
    h->use_device();
    quiesce(h);                                  // a batch in flight reads the arrays that may move
    h->label_rows.reset();                       // the inverted label column covers `size` ids: the next rescored call rebuilds it
    lab.facet.reset();                           // ... and so does the label column's facet dictionary
    HostIndex& hi = h->host;
    const uint64_t D = h->L.D, dim = h->dim, nw = (need + 31) / 32;
    const bool removed = hi.n_removed != 0;
    // everything that can fail comes first: host room, device room, the device pass; the handle changes after that
    h->tail_vecs.reserve((h->tail + m) * dim);
    if (lab.has) host_labels.reserve(need);
    if (removed) hi.removed.reserve(nw);
    hipStream_t st = own_stream(h);
    const uint64_t cap = tail_capacity(std::min<uint64_t>(h->d_raw.n / D, h->d_norm.n), need);
    grow_keep(h->d_raw, size * D, cap * D, st);
    grow_keep(h->d_norm, size, cap, st);
    if (h->has_rows) grow_keep(h->d_rows, size, cap, st);
    if (lab.has) grow_keep(lab.vals, size, cap, st);
    if (removed) grow_keep(h->d_removed, (size + 31) / 32, (cap + 31) / 32, st);
    DevBuf<float> d_src(m * dim);
    DevBuf<int32_t> d_lab(labels ? m : 0);
    HIP_CHECK(hipMemcpyAsync(d_src.p, vectors, m * dim * 4, hipMemcpyHostToDevice, st));
    if (labels) HIP_CHECK(hipMemcpyAsync(d_lab.p, labels, m * 4, hipMemcpyHostToDevice, st));
    if (removed) {                               // whole words behind the old last one: clear, whatever the buffer held
        const uint64_t w0 = (size + 31) / 32;
        if (nw > w0) HIP_CHECK(hipMemsetAsync(h->d_removed.p + w0, 0, (nw - w0) * 4, st));
    }
    TailAppendArgs a{};
    a.src = d_src.p;
    a.src_labels = labels ? d_lab.p : nullptr;
    a.first = size;
    a.m = m;
    a.dim = (uint32_t)dim;
    a.D = (uint32_t)D;
    a.raw = h->d_raw.p;
    a.norm_sq = h->d_norm.p;
    a.rows = h->has_rows ? h->d_rows.p : nullptr;
    a.labels = labels ? lab.vals.p : nullptr;
    a.removed = removed ? h->d_removed.p : nullptr;
    tail_append(a, st);
    HIP_CHECK(hipStreamSynchronize(st));
    // (nothing below throws before the handle is consistent again: the room was reserved above)
    h->tail_vecs.insert(h->tail_vecs.end(), vectors, vectors + m * dim);
    if (lab.has && host_labels.size() == size) host_labels.insert(host_labels.end(), labels, labels + m);
    if (removed) {
        if (size & 31) hi.removed[(size - 1) >> 5] &= (1u << (size & 31)) - 1u;
        hi.removed.resize(nw, 0u);
    }
    h->tail += m;
    h->has_tail.store(true);
    if (removed) {                               // R has another size: a new state, so no cached F & ~R of the old size is found again
        h->rm_epoch = ++g_removed_epoch;
        h->live.reset();
        h->live = make_live_filter(h, nullptr);
    }
    return size;
}

}  // namespace

extern "C" {

int cph_add(cph_index* h, const float* vectors, uint64_t m, const int32_t* labels, int64_t* first_id) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_add");
        const uint64_t first = add_rows(h, vectors, m, labels);
        if (first_id) *first_id = (int64_t)first;
    });
}

int cph_tail_count(cph_index* h, uint64_t* t) {
    return guarded([&] {
        if (!h || !t) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        *t = h->tail;
    });
}

static void check_tail_fold_args(const int64_t* g_ids, const float* g_dist, uint64_t n, uint64_t k, const uint64_t* pools,
                                 const uint32_t* counts, uint32_t P, uint32_t C, const int64_t* out_ids, const float* out_dist) {
    if (!g_ids || !g_dist || !pools || !counts || !out_ids || !out_dist) throw InvalidArg("null argument");
    if (P < 1 || P > kExactMaxParts) throw InvalidArg("P must be 1.." + std::to_string(kExactMaxParts));
    if (n < 1 || n > 0xFFFFFFFFull || k < 1 || k > kExactMaxK) throw InvalidArg("fold: sizes out of range");
    if (C < 128 || C > 4 * kExactMaxK || (C & (C - 1)) || k > C / 2) throw InvalidArg("C must be a power of two, 128 <= C and 2 k <= C");
    for (uint64_t i = 0; i < (uint64_t)P * n; ++i)
        if (counts[i] > k) throw InvalidArg("a tail list holds more than k keys");
}

int cph_tail_fold_hook(int device, const int64_t* g_ids, const float* g_dist, uint64_t n, uint64_t k, const uint64_t* pools,
                       const uint32_t* counts, uint32_t P, uint32_t C, int64_t* out_ids, float* out_dist) {
    return guarded([&] {
        check_tail_fold_args(g_ids, g_dist, n, k, pools, counts, P, C, out_ids, out_dist);
        HIP_CHECK(hipSetDevice(device));
        const size_t rows = (size_t)n * k, lists = (size_t)P * n;
        DevBuf<int64_t> d_ids(rows);
        DevBuf<float> d_dist(rows);
        DevBuf<unsigned long long> d_pools(lists * C);
        DevBuf<uint32_t> d_counts(lists);
        HIP_CHECK(hipMemcpy(d_ids.p, g_ids, rows * 8, hipMemcpyHostToDevice));      // the graph's rows: folded in place, as the library does
        HIP_CHECK(hipMemcpy(d_dist.p, g_dist, rows * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_pools.p, pools, lists * C * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_counts.p, counts, lists * 4, hipMemcpyHostToDevice));
        TailFoldArgs f{};
        f.pools = d_pools.p;
        f.counts = d_counts.p;
        f.P = P;
        f.q_first = 0;
        f.q_count = (uint32_t)n;
        f.k = (uint32_t)k;
        f.C = C;
        f.ids = d_ids.p;
        f.dist = d_dist.p;
        tail_fold(f, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out_ids, d_ids.p, rows * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(out_dist, d_dist.p, rows * 4, hipMemcpyDeviceToHost));
    });
}

int cph_host_tail_fold(const int64_t* g_ids, const float* g_dist, uint64_t n, uint64_t k, const uint64_t* pools, const uint32_t* counts,
                       uint32_t P, uint32_t C, int64_t* out_ids, float* out_dist) {
    return guarded([&] {
        check_tail_fold_args(g_ids, g_dist, n, k, pools, counts, P, C, out_ids, out_dist);
        tail_fold_host(g_ids, g_dist, n, k, pools, counts, P, C, out_ids, out_dist);
    });
}

int cph_host_tail_capacity(uint64_t capacity, uint64_t need, uint64_t* out) {
    return guarded([&] {
        if (!out) throw InvalidArg("null argument");
        *out = tail_capacity(capacity, need);
    });
}

int cph_host_live_filter(const uint32_t* words_f, const uint32_t* words_removed, uint64_t n, uint32_t* words_out, uint64_t* count_out) {
    return guarded([&] {
        if (n != 0 && (!words_removed || !words_out)) throw InvalidArg("null argument");
        if (n > 0xFFFFFFFFull) throw InvalidArg("filter too large");
        const uint64_t c = live_filter_host(words_f, words_removed, n, words_out);
        if (count_out) *count_out = c;
    });
}

int cph_multi_remove(cph_multi* m, const int64_t* ids, uint64_t cnt, int space, uint64_t* newly) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::unique_lock<std::shared_mutex> lk(m->life);     // searches in flight finish first; the next one sees R on every replica
        uint64_t c = 0;
        for (size_t i = 0; i < m->reps.size(); ++i) {        // (replica 0 validates: a bad id changes no replica)
            const uint64_t ci = remove_ids(m->reps[i], ids, cnt, space);
            if (i == 0) c = ci;
        }
        if (newly) *newly = c;
    });
}

int cph_multi_live_count(cph_multi* m, uint64_t* n) {
    return multi_shared(m, [&] { return cph_live_count(m->reps[0], n); });
}

int cph_multi_get_removed(cph_multi* m, uint32_t* words) {
    return multi_shared(m, [&] { return cph_get_removed(m->reps[0], words); });
}

int cph_multi_compact(cph_multi* m, int64_t* old_to_new) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        multi_lifecycle(m, [&](cph_index* r0) { compact_index(r0, old_to_new); });
    });
}

int cph_parts_remove(cph_parts* m, const int64_t* ids, uint64_t cnt, uint64_t* newly) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        if (cnt && !ids) throw InvalidArg("null argument");
        std::unique_lock<std::shared_mutex> lk(m->life);
        if (!parts_finalized(m)) throw std::runtime_error("Search failed: invalid entry point after finalize.");
        const uint32_t P = (uint32_t)m->parts.size();
        const uint64_t total = m->bounds.back();
        std::vector<std::vector<int64_t>> cut(P);            // global input rows, cut at the part bounds
        for (uint64_t i = 0; i < cnt; ++i) {
            if (ids[i] < 0 || (uint64_t)ids[i] >= total)
                throw InvalidArg("remove: id " + std::to_string(ids[i]) + " is outside [0, " + std::to_string(total) + ")");
            const uint32_t p = (uint32_t)(std::upper_bound(m->bounds.begin(), m->bounds.end(), (uint64_t)ids[i]) - m->bounds.begin()) - 1;
            cut[p].push_back(ids[i] - (int64_t)m->bounds[p]);
        }
        uint64_t c = 0;
        for (uint32_t p = 0; p < P; ++p) c += remove_ids(m->parts[p], cut[p].data(), cut[p].size(), CPH_IDS_INPUT);
        if (newly) *newly = c;
    });
}

int cph_parts_live_count(cph_parts* m, uint64_t* n) {
    return guarded([&] {
        if (!m || !n) throw InvalidArg("null argument");
        std::shared_lock<std::shared_mutex> lk(m->life);
        *n = 0;
        for (cph_index* h : m->parts) {
            uint64_t x = 0;
            check_rc(cph_live_count(h, &x));
            *n += x;
        }
    });
}

int cph_parts_get_removed(cph_parts* m, uint32_t* words) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::shared_lock<std::shared_mutex> lk(m->life);
        if (!parts_finalized(m)) throw std::runtime_error("Search failed: invalid entry point after finalize.");
        const uint64_t total = m->bounds.back();
        if (total && !words) throw InvalidArg("null argument");
        std::fill(words, words + (total + 31) / 32, 0u);
        for (size_t p = 0; p < m->parts.size(); ++p) {
            cph_index* h = m->parts[p];
            std::lock_guard<std::mutex> g(h->mu);
            const HostIndex& hi = h->host;
            if (hi.n_removed == 0) continue;
            for (uint64_t i = 0; i < hi.n; ++i)
                if ((hi.removed[i >> 5] >> (i & 31)) & 1u) {
                    const uint64_t r = m->bounds[p] + hi.rows[i];
                    words[r >> 5] |= 1u << (r & 31);
                }
        }
    });
}

}  // extern "C"

// ---- the columns of replicas and parts ----
namespace {

// A setter over several handles, all or none: ask(h) on every handle under its mutex before any of them changes, then
// change(i, h) on each, under its mutex too; when one throws, the column goes from every handle.
template <class Ask, class Change>
void set_column_on_all(const std::vector<cph_index*>& hs, uint32_t col, Ask&& ask, Change&& change) {
    for (cph_index* h : hs) {
        std::lock_guard<std::mutex> g(h->mu);
        ask(h);
    }
    try {
        for (size_t i = 0; i < hs.size(); ++i) {
            std::lock_guard<std::mutex> g(hs[i]->mu);
            change(i, hs[i]);
        }
    } catch (...) {                                      // (a refused row or a device failure: no handle keeps a column the others lack)
        for (cph_index* h : hs) {
            std::lock_guard<std::mutex> g(h->mu);
            try { install_column_locked(h, col, nullptr, false); } catch (...) {}
        }
        throw;
    }
}

// cph_multi_set_labels / _set_column / _set_tags: replica 0 validates the rest and makes the stored form once (input rows
// moved to internal order, tag rows canonical) before anything changes; the others receive its host copy.
void multi_set_column(cph_multi* m, uint32_t col, const int32_t* vals, const uint64_t* lims, uint64_t n, int space) {
    std::unique_lock<std::shared_mutex> lk(m->life);     // searches in flight finish first
    cph_index* r0 = m->reps[0];
    const bool set = column_given(col, vals, lims);
    HostColumn c;
    set_column_on_all(
        m->reps, col,
        [&](cph_index* h) {
            require_column_target(h, col, set, n);
            if (h != r0) return;
            require_id_space(space);
            if (set) c = column_to_store_locked(r0, col, vals, lims, n, space);
        },
        [&](size_t i, cph_index* h) { install_column_locked(h, col, !set ? nullptr : i == 0 ? &c : &r0->host.cols[col], i == 0); });
}

// cph_parts_set_labels / _set_column / _set_tags: a column over GLOBAL input rows, cut at the part bounds (tag limits rebased).
void parts_set_column(cph_parts* m, uint32_t col, const int32_t* vals, const uint64_t* lims, uint64_t n) {
    if (!m) throw InvalidArg("null handle");
    const ColumnWords& w = words_of(col);
    std::unique_lock<std::shared_mutex> lk(m->life);
    if (!parts_finalized(m)) throw InvalidArg(std::string(w.plural) + " belong to a finalized index: finalize or load it first");
    const bool set = column_given(col, vals, lims);
    if (set && n != m->bounds.back()) throw InvalidArg(wrong_column_size(col, n, m->bounds.back()));
    if (set && lims) {
        if (lims[0] != 0) throw InvalidArg("tag limits must start at 0");      // (before the cut rebases them)
        for (uint64_t i = 0; i < n; ++i)
            if (lims[i + 1] < lims[i]) throw InvalidArg("tag limits must not decrease (row " + std::to_string(i) + ")");
        if (lims[n] != 0 && !vals) throw InvalidArg("null tags");
    }
    std::vector<uint64_t> cut;
    set_column_on_all(
        m->parts, col,
        [&](cph_index* h) {
            if (set && (!h->has_rows || h->host.rows.size() != h->host.n))
                throw InvalidArg(std::string("a part has no row map: ") + w.plural + " of a partitioned index are given in input rows");
        },
        [&](size_t p, cph_index* h) {
            if (!set) {
                require_column_target(h, col, false, 0);
                install_column_locked(h, col, nullptr, true);
                return;
            }
            const uint64_t b0 = m->bounds[p], b1 = m->bounds[p + 1];
            if (lims) {
                cut.assign(lims + b0, lims + b1 + 1);
                for (uint64_t& x : cut) x -= lims[b0];
            }
            HostColumn c = column_to_store_locked(h, col, vals ? vals + (lims ? lims[b0] : b0) : nullptr, lims ? cut.data() : nullptr, b1 - b0, CPH_IDS_INPUT);
            install_column_locked(h, col, &c, true);
        });
}

// ---- the filters of a partitioned index, made part by part ----
// cnt parts filters from their per-part slices: make(p, slice) makes part p's cnt filters on that part's device, all or
// none.  All made, or none: what earlier parts made goes with `made` (a cph_parts_filter destroys its slices).
template <class Make>
void parts_filters_from_slices(size_t P, uint64_t n_bits, uint32_t cnt, cph_parts_filter** out, Make&& make) {
    std::vector<std::unique_ptr<cph_parts_filter>> made(cnt);
    for (auto& f : made) {
        f.reset(new cph_parts_filter());
        f->n_bits = n_bits;
        f->f.reserve(P);
    }
    std::vector<cph_filter*> slice(cnt);
    for (size_t p = 0; p < P; ++p) {
        make(p, slice.data());
        for (uint32_t j = 0; j < cnt; ++j) made[j]->f.push_back(slice[j]);
    }
    for (uint32_t j = 0; j < cnt; ++j) out[j] = made[j].release();
}

// cph_parts_filters_from_labels / cph_parts_filters_from_column: every part evaluates its own slice of the column.
void parts_filters_from_column(cph_parts* m, int kind, uint32_t slot, const int32_t* lo, const int32_t* hi, uint32_t cnt,
                               cph_parts_filter** out) {
    const uint32_t col = facet_column(kind, slot);
    if (cnt == 0) return;
    if (!out) throw InvalidArg("null argument");
    std::fill(out, out + cnt, nullptr);
    if (!m || !lo || !hi) throw InvalidArg("null argument");
    std::shared_lock<std::shared_mutex> lk(m->life);
    if (!parts_finalized(m)) throw std::runtime_error("Search failed: invalid entry point after finalize.");
    parts_filters_from_slices(m->parts.size(), m->bounds.back(), cnt, out,
                              [&](size_t p, cph_filter** slice) { filters_from_labels(m->parts[p], col, lo, hi, cnt, slice); });
}

}  // namespace

extern "C" {

int cph_parts_compact(cph_parts* m, int64_t* old_to_new) {
    return guarded([&] {
        if (!m || !old_to_new) throw InvalidArg("null argument");
        std::vector<float> vecs;
        LiveColumns cols;                         // the live rows' values in every column, in global row order (every part has a column, or none)
        uint64_t live = 0;
        {
            std::unique_lock<std::shared_mutex> lk(m->life);
            if (!parts_finalized(m)) throw std::runtime_error("Search failed: invalid entry point after finalize.");
            const uint32_t P = (uint32_t)m->parts.size();
            std::vector<int64_t> map(m->bounds.back());
            for (uint32_t p = 0; p < P; ++p) {
                cph_index* h = m->parts[p];
                std::lock_guard<std::mutex> g(h->mu);
                live += gather_live(h, vecs, map.data() + m->bounds[p], true, (int64_t)live, &cols);
            }
            if (live < kMinPartRows * P)      // cph_parts_build's own refusal, before any part gives up its index
                throw InvalidArg("a partitioned index needs at least " + std::to_string(kMinPartRows) + " rows per part: " +
                                 std::to_string(live) + " rows for " + std::to_string(P) + " parts");
            std::copy(map.begin(), map.end(), old_to_new);
        }
        parts_build(m, vecs.data(), live, true);              // the live rows, cut again by cph_host_part_bounds
        std::vector<float>().swap(vecs);
        check_rc(cph_parts_finalize(m));
        set_live_columns(cols, [&](uint32_t col, const int32_t* vals, const uint64_t* lims) { parts_set_column(m, col, vals, lims, live); });      // cut again at the new bounds
    });
}

int cph_multi_set_labels(cph_multi* m, const int32_t* labels, uint64_t n, int space) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        multi_set_column(m, kLabelColumn, labels, nullptr, n, space);
    });
}

int cph_multi_set_column(cph_multi* m, uint32_t slot, const int32_t* values, uint64_t n, int space) {
    return guarded([&] {
        const uint32_t col = facet_column(CPH_FACET_COLUMN, slot);
        if (!m) throw InvalidArg("null handle");
        multi_set_column(m, col, values, nullptr, n, space);
    });
}

int cph_multi_set_tags(cph_multi* m, uint32_t slot, const uint64_t* lims, const int32_t* tags, uint64_t n, int space) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        multi_set_column(m, facet_column(CPH_FACET_TAGS, slot), tags, lims, n, space);
    });
}

int cph_parts_set_labels(cph_parts* m, const int32_t* labels, uint64_t n) {
    return guarded([&] { parts_set_column(m, kLabelColumn, labels, nullptr, n); });
}

int cph_parts_set_column(cph_parts* m, uint32_t slot, const int32_t* values, uint64_t n) {
    return guarded([&] { parts_set_column(m, facet_column(CPH_FACET_COLUMN, slot), values, nullptr, n); });
}

int cph_parts_set_tags(cph_parts* m, uint32_t slot, const uint64_t* lims, const int32_t* tags, uint64_t n) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        parts_set_column(m, facet_column(CPH_FACET_TAGS, slot), tags, lims, n);
    });
}

int cph_parts_filters_from_labels(cph_parts* m, const int32_t* lo, const int32_t* hi, uint32_t cnt, cph_parts_filter** out) {
    return guarded([&] { parts_filters_from_column(m, CPH_FACET_LABEL, 0, lo, hi, cnt, out); });
}

int cph_parts_filters_from_column(cph_parts* m, uint32_t slot, const int32_t* lo, const int32_t* hi, uint32_t cnt, cph_parts_filter** out) {
    return guarded([&] { parts_filters_from_column(m, CPH_FACET_COLUMN, slot, lo, hi, cnt, out); });
}

int cph_parts_filters_from_tags(cph_parts* m, uint32_t slot, const uint32_t* test_lims, const int32_t* test_vals, const uint8_t* modes,
                                uint32_t cnt, cph_parts_filter** out) {
    return guarded([&] {
        if (cnt == 0) return;
        if (!out) throw InvalidArg("null argument");
        std::fill(out, out + cnt, nullptr);
        if (!m || !test_lims || !modes) throw InvalidArg("null argument");
        const uint32_t col = facet_column(CPH_FACET_TAGS, slot);
        std::vector<uint32_t> table;
        size_t vals_at = 0;
        pack_tag_tests(test_lims, test_vals, modes, cnt, table, vals_at);
        std::shared_lock<std::shared_mutex> lk(m->life);
        if (!parts_finalized(m)) throw std::runtime_error("Search failed: invalid entry point after finalize.");
        parts_filters_from_slices(m->parts.size(), m->bounds.back(), cnt, out,
                                  [&](size_t p, cph_filter** slice) { filters_from_tags(m->parts[p], col, table, vals_at, cnt, slice); });
    });
}

// Part p of every operand, combined on part p's device (filters_combine).  All made, or none.
int cph_parts_filters_combine(int op, const cph_parts_filter* const* a, uint32_t cnt, const cph_parts_filter* const* b, uint32_t n_b,
                              cph_parts_filter** out) {
    return guarded([&] {
        if (cnt == 0) return;
        if (!out) throw InvalidArg("null argument");
        std::fill(out, out + cnt, nullptr);
        if (!a) throw InvalidArg("null argument");
        check_combine_shape(op, cnt, b, n_b);
        for (uint32_t j = 0; j < cnt; ++j)
            if (!a[j]) throw InvalidArg("null filter");
        for (uint32_t j = 0; j < n_b; ++j)
            if (!b[j]) throw InvalidArg("null filter");
        const size_t P = a[0]->f.size();
        const uint64_t n_bits = a[0]->n_bits;
        auto same = [&](const cph_parts_filter* f) {
            if (f->f.size() != P) throw InvalidArg("filters with different part counts cannot be combined");
            if (f->n_bits != n_bits) throw InvalidArg("filters of different sizes cannot be combined");
        };
        for (uint32_t j = 0; j < cnt; ++j) same(a[j]);
        for (uint32_t j = 0; j < n_b; ++j) same(b[j]);
        std::vector<const cph_filter*> ap(cnt), bp(n_b);
        parts_filters_from_slices(P, n_bits, cnt, out, [&](size_t p, cph_filter** slice) {
            for (uint32_t j = 0; j < cnt; ++j) ap[j] = a[j]->f[p];
            for (uint32_t j = 0; j < n_b; ++j) bp[j] = b[j]->f[p];
            filters_combine(op, ap.data(), cnt, n_b ? bp.data() : nullptr, n_b, slice);
        });
    });
}

int cph_parts_filter_count(const cph_parts_filter* f, uint64_t* count) {
    return guarded([&] {
        if (!f || !count) throw InvalidArg("null argument");
        *count = 0;
        for (const cph_filter* x : f->f) *count += x->popcount;
    });
}

}  // extern "C"

// ---- searches that re-rank candidate rows: grouped, diverse, maxsim (device_group.h, device_diverse.h, device_maxsim.h) ----
// One entry path for the three: an ordinary search at k = C into scratch rows the handle owns, then one kernel over those
// rows on the same stream.  The rows hold INTERNAL ids whatever the handle returns (the keys are looked up by internal
// id); the row map is applied where an id is written.  Nothing here waits for the device in the _device form.  A
// re-ranker is a small struct (GroupedSearch, DiverseSearch, MaxsimSearch, MaxsimRescoredSearch, FusedSearch, RescoredSearch): its
// scalars, its checks (check_on: those that need the handle a call runs on), its output table, what the host form stages
// besides the queries (stage) and its pass; the entries, the scratch, the replica fan-out and the hooks below are written
// once over that.  (MaxsimRescoredSearch's pass is four launches, and the first one on a key column waits for the device:
// key_rows.)
struct cph_group_keys {
    cph_index* h = nullptr;                    // the handle it was made for ...
    uint64_t epoch = 0;                        // ... and the index that handle held then (index_epoch)
    int device = 0;
    uint64_t size = 0;                         // ids it covers
    DevBuf<int32_t> keys;                      // [size], internal-id order
    mutable std::unique_ptr<KeyRows> rows;     // the column inverted (rescored maxsim search): made on first use under the handle mutex
};

namespace {

// While it lives, searches of the handle write internal ids.  The caller holds the handle mutex from before its
// construction until after its destruction, so no other call observes the change.
struct InternalIdsScope {
    cph_index* h;
    bool was;
    explicit InternalIdsScope(cph_index* h_) : h(h_), was(h_->ids_input) { h->ids_input = false; }
    ~InternalIdsScope() { h->ids_input = was; }
};

// The outputs of one re-ranker call, in the order of its C signature: where each goes and how many bytes of it a query
// has.  Every walk over "the outputs" -- the null check, the scratch reservation, the copy-back of the host form, the
// per-shard offsets of the replica form, the hooks' poison fill and download -- walks this table.
struct RerankOuts {
    struct Out { void* p; size_t stride; } o[kMaxRerankOuts];
    int count;
    bool all() const {
        for (int i = 0; i < count; ++i)
            if (!o[i].p) return false;
        return true;
    }
    template <class T> T* at(int i) const { return static_cast<T*>(o[i].p); }
};

// What a re-ranker call carries besides the re-ranker's own scalars.
struct RerankCall {
    const float* q;
    uint64_t n;
    const cph_filter* const* filters;
    uint32_t F;
    const int32_t* filter_of;
    bool exact;
    RerankOuts out;
};

void check_filter_args(const RerankCall& c) {
    if (c.F && !c.filters) throw InvalidArg("null argument");
    if (!c.filter_of && c.F > 1) throw InvalidArg("several filters need filter_of (the filter of every query)");
}

void check_batch_size(uint64_t n) {
    if (n > 0x7FFFFFFFull) throw InvalidArg("batch too large");
}

// The key column of a grouped or maxsim call: the keys object (checked against the handle), else the label column.
const int32_t* group_key_column(const cph_index* h, const cph_group_keys* keys) {
    if (!keys) {
        if (!h->cols[kLabelColumn].has) throw InvalidArg("grouped search needs keys: the index has no label column (cph_set_labels) and no keys object was given");
        return h->cols[kLabelColumn].vals.p;
    }
    if (keys->device != h->device) throw InvalidArg("group keys belong to another device");
    if (keys->size != h->size())
        throw InvalidArg("group keys cover " + std::to_string(keys->size) + " ids, the index holds " + std::to_string(h->size()));
    if (keys->h != h || keys->epoch != h->index_epoch)
        throw InvalidArg("group keys were made for another index (a load, build or compact invalidates them)");
    return keys->keys.p;
}

// The ordinary search at k = C into the rows of `gs`, in internal ids, then pass(), which enqueues one kernel over those
// rows, bracketed by the timer's events while it is on; everything on `st`.  The caller holds the handle mutex and has set
// the device.
template <class Pass>
void search_rows_then_pass(cph_index* h, RerankScratch& gs, const float* d_queries, uint64_t n, uint64_t C, const cph_filter* const* filters,
                           uint32_t F, const int32_t* filter_of, bool exact, cph_index::PassTimer& timer, hipStream_t st, Pass pass) {
    RerankScratch::Rows& rows = gs.rows;
    if (!rows.ev) HIP_CHECK(hipEventCreateWithFlags(&rows.ev, hipEventDisableTiming));
    Reserve r = gs.reserve();
    r(rows.ids, n * C);
    r(rows.dist, n * C);
    if (rows.used) HIP_CHECK(hipStreamWaitEvent(st, rows.ev, 0));    // the rows' previous batch, maybe on another stream
    try {
        {
            InternalIdsScope internal(h);
            search_batch_locked(h, batch_call(d_queries, n, C, filters, F, filter_of, exact, rows.ids.p, rows.dist.p, true, st));
        }
        timed_pass(timer, st, pass);
    } catch (...) {
        (void)hipEventRecord(rows.ev, st);                        // whatever was enqueued may still write the rows
        rows.used = true;
        throw;
    }
    HIP_CHECK(hipEventRecord(rows.ev, st));
    rows.used = true;
}

RerankScratch& next_rerank_scratch(cph_index* h) {
    h->last_rerank = (h->last_rerank + 1) % kMaxBatchSets;
    return h->rerank_scratch[h->last_rerank];
}

// The one place the host-form buffers of a set grow: the staged queries and one buffer per slot of the table, each on its
// own.  -> the table at the set's device addresses.
RerankOuts reserve_rerank_scratch(RerankScratch& gs, size_t q_floats, uint64_t n, const RerankOuts& host) {
    Reserve r = gs.reserve();
    r(gs.host.q, q_floats);
    RerankOuts dev = host;
    for (int i = 0; i < host.count; ++i) dev.o[i].p = r(gs.host.out[i], n * host.o[i].stride);
    return dev;
}

// ---- the three re-rankers ----
void check_group_shape(uint64_t k, uint64_t g, uint64_t C) {
    if (k < 1 || g < 1) throw InvalidArg("grouped search needs k >= 1 and group_size >= 1");
    if (C > kGroupMaxCandidates)
        throw InvalidArg("grouped search supports candidates <= " + std::to_string(kGroupMaxCandidates) + ", got " + std::to_string(C));
    if (k > C || g > C || k * g > C)
        throw InvalidArg("grouped search needs k * group_size <= candidates (got " + std::to_string(k) + " * " + std::to_string(g) +
                         " > " + std::to_string(C) + ")");
}

void check_group_rows_args(const int64_t* ids, const float* dist, uint64_t n, uint64_t C, const int32_t* key_of, uint64_t n_keys,
                           uint64_t k, uint64_t g, const RerankOuts& o) {
    if (!ids || !dist || !key_of || !o.all()) throw InvalidArg("null argument");
    if (C < 1) throw InvalidArg("group rows: candidates must be >= 1");
    check_group_shape(k, g, C);
    if (n < 1 || n > 0x7FFFFFFFull || n_keys < 1 || n_keys > 0xFFFFFFFFull) throw InvalidArg("group rows: sizes out of range");
    for (uint64_t i = 0; i < n * C; ++i)
        if (ids[i] >= 0 && (uint64_t)ids[i] >= n_keys) throw InvalidArg("group rows: id out of range");
}

GroupArgs group_args(const int64_t* r_ids, const float* r_dist, uint64_t C, uint64_t k, uint64_t g, const int32_t* d_key_of, uint64_t n_ids,
                     const uint32_t* d_rows, const RerankOuts& o) {
    GroupArgs a{};
    a.ids = r_ids;
    a.dist = r_dist;
    a.C = (uint32_t)C;
    a.k = (uint32_t)k;
    a.g = (uint32_t)g;
    a.key_of = d_key_of;
    a.n_ids = (uint32_t)n_ids;
    a.rows = d_rows;
    a.out_ids = o.at<int64_t>(0);
    a.out_dist = o.at<float>(1);
    a.out_keys = o.at<int32_t>(2);
    a.out_counts = o.at<int32_t>(3);
    a.out_complete = o.at<uint8_t>(4);
    return a;
}

struct GroupedSearch {
    uint64_t k, g, C;
    static constexpr PassKind kind = kPassGrouped;
    static constexpr bool keyed = true;
    static constexpr const char* name = "grouped";
    uint64_t tokens() const { return 1; }
    void check_shape() const {
        if (C < 1) throw InvalidArg("grouped search needs candidates >= 1");
        check_group_shape(k, g, C);
    }
    void check_batch(uint64_t n) const { check_batch_size(n); }
    void check_inputs(uint64_t) const {}
    void check_on(const cph_index*, uint32_t) const {}
    void stage(RerankScratch&, uint64_t, hipStream_t) const {}
    RerankOuts outs(int64_t* ids, float* dist, int32_t* keys, int32_t* counts, uint8_t* complete) const {
        return {{{ids, 8 * k * g}, {dist, 4 * k * g}, {keys, 4 * k}, {counts, 4 * k}, {complete, 1}}, 5};
    }
    void pass(cph_index* h, RerankScratch& gs, uint64_t n, const int32_t* d_key_of, const float*, const RerankOuts& o, hipStream_t st) const {
        group_rows(group_args(gs.rows.ids.p, gs.rows.dist.p, C, k, g, d_key_of, h->size(), h->ids_input ? h->d_rows.p : nullptr, o), (uint32_t)n, st);
    }
};

// (An id at or above n_ids in given rows is no error: the statement counts it as padding.)
void check_diverse_shape(uint64_t k, uint64_t C, float lam) {
    if (k < 1) throw InvalidArg("diverse search needs k >= 1");
    if (C > kDiverseMaxCandidates)
        throw InvalidArg("diverse search supports candidates <= " + std::to_string(kDiverseMaxCandidates) + ", got " + std::to_string(C));
    if (C < k) throw InvalidArg("diverse search needs k <= candidates (got " + std::to_string(k) + " > " + std::to_string(C) + ")");
    if (!(lam >= 0.0f && lam <= 1.0f)) throw InvalidArg("diverse search needs lam in [0, 1]");
}

void check_diverse_rows_args(const int64_t* ids, const float* dist, uint64_t n, uint64_t C, uint64_t n_ids, uint64_t k, float lam,
                             const RerankOuts& o) {
    if (!ids || !dist || !o.all()) throw InvalidArg("null argument");
    check_diverse_shape(k, C, lam);
    if (n < 1 || n > 0x7FFFFFFFull || n_ids < 1 || n_ids > 0xFFFFFFFFull) throw InvalidArg("diverse rows: sizes out of range");
}

DiverseArgs diverse_args(const cph_index* h, const int64_t* r_ids, const float* r_dist, uint64_t C, uint64_t k, float lam, const RerankOuts& o) {
    DiverseArgs a{};
    a.ids = r_ids;
    a.dist = r_dist;
    a.C = (uint32_t)C;
    a.k = (uint32_t)k;
    a.a = lam;
    a.b = 1.0f - lam;
    a.raw = h->d_raw.p;
    a.norm_sq = h->d_norm.p;
    a.n_ids = (uint32_t)h->size();
    a.D = h->D;
    a.rows = h->ids_input ? h->d_rows.p : nullptr;
    a.out_ids = o.at<int64_t>(0);
    a.out_dist = o.at<float>(1);
    a.out_gap = o.at<float>(2);
    return a;
}

// The pass runs against the handle's resident vectors and norms.
struct DiverseSearch {
    uint64_t k;
    float lam;
    uint64_t C;
    static constexpr PassKind kind = kPassDiverse;
    static constexpr bool keyed = false;
    static constexpr const char* name = "diverse";
    uint64_t tokens() const { return 1; }
    void check_shape() const { check_diverse_shape(k, C, lam); }
    void check_batch(uint64_t n) const { check_batch_size(n); }
    void check_inputs(uint64_t) const {}
    void check_on(const cph_index*, uint32_t) const {}
    void stage(RerankScratch&, uint64_t, hipStream_t) const {}
    RerankOuts outs(int64_t* ids, float* dist, float* gap) const { return {{{ids, 8 * k}, {dist, 4 * k}, {gap, 4 * k}}, 3}; }
    void pass(cph_index* h, RerankScratch& gs, uint64_t n, const int32_t*, const float*, const RerankOuts& o, hipStream_t st) const {
        diverse_rows(diverse_args(h, gs.rows.ids.p, gs.rows.dist.p, C, k, lam, o), (uint32_t)n, st);
    }
};

void check_maxsim_shape(uint64_t T, uint64_t C, uint64_t k) {
    if (T < 1 || T > kMaxsimMaxTokens)
        throw InvalidArg("maxsim search supports 1 <= tokens <= " + std::to_string(kMaxsimMaxTokens) + ", got " + std::to_string(T));
    if (C < 1 || C > kMaxsimMaxCandidates)
        throw InvalidArg("maxsim search supports 1 <= candidates <= " + std::to_string(kMaxsimMaxCandidates) + ", got " + std::to_string(C));
    if (T * C > kMaxsimMaxEntries)
        throw InvalidArg("maxsim search needs tokens * candidates <= " + std::to_string(kMaxsimMaxEntries) + " (got " + std::to_string(T) +
                         " * " + std::to_string(C) + ")");
    if (k < 1 || k > kMaxsimMaxK) throw InvalidArg("maxsim search supports 1 <= k <= " + std::to_string(kMaxsimMaxK) + ", got " + std::to_string(k));
}

void check_maxsim_tokens(const int32_t* n_tokens, uint64_t n, uint64_t T) {
    for (uint64_t i = 0; n_tokens && i < n; ++i)
        if (n_tokens[i] < 1 || (uint64_t)n_tokens[i] > T)
            throw InvalidArg("n_tokens[" + std::to_string(i) + "] = " + std::to_string(n_tokens[i]) + " is outside [1, " + std::to_string(T) + "]");
}

void check_maxsim_batch(uint64_t n, uint64_t T) {
    if (n > 0x7FFFFFFFull || n * T > 0x7FFFFFFFull)
        throw InvalidArg("batch too large: maxsim search needs n * tokens <= 2147483647 (got " + std::to_string(n) + " * " + std::to_string(T) + ")");
}

void check_maxsim_rows_args(const int64_t* ids, const float* dist, uint64_t n, uint64_t T, const int32_t* n_tokens, uint64_t C,
                            const int32_t* key_of, uint64_t n_keys, uint64_t k, const RerankOuts& o) {
    if (!ids || !dist || !key_of || !o.all()) throw InvalidArg("null argument");
    check_maxsim_shape(T, C, k);
    check_maxsim_batch(n, T);
    if (n < 1 || n_keys < 1 || n_keys > 0xFFFFFFFFull) throw InvalidArg("maxsim rows: sizes out of range");
    check_maxsim_tokens(n_tokens, n, T);
}

MaxsimArgs maxsim_args(const int64_t* r_ids, const float* r_dist, const int32_t* d_tokens, uint64_t T, uint64_t C, uint64_t k,
                       const int32_t* d_key_of, uint64_t n_ids, const uint32_t* d_rows, const RerankOuts& o) {
    MaxsimArgs a{};
    a.ids = r_ids;
    a.dist = r_dist;
    a.n_tokens = d_tokens;
    a.T = (uint32_t)T;
    a.C = (uint32_t)C;
    a.k = (uint32_t)k;
    a.key_of = d_key_of;
    a.n_ids = (uint32_t)n_ids;
    a.rows = d_rows;
    a.out_keys = o.at<int32_t>(0);
    a.out_score = o.at<float>(1);
    a.out_hits = o.at<int32_t>(2);
    a.out_rows = o.at<int64_t>(3);
    a.out_found = o.at<int32_t>(4);
    return a;
}

// The queries are [n][T][dim]: the n * T token rows are one ordinary batch, and the pass joins the T rows of every query
// by key.  n_tokens is on the host (null: every token is live) and travels as the set's staged table: one host wait, for the
// copy of the table this set carried the last time, never for a kernel -- unless the buffers have to grow.  (The pass runs
// after `st` has been made to wait for the set's previous batch, whose kernels read the table.)
struct MaxsimSearch {
    uint64_t T;
    const int32_t* n_tokens;
    uint64_t k, C;
    static constexpr PassKind kind = kPassMaxsim;
    static constexpr bool keyed = true;
    static constexpr const char* name = "maxsim";
    uint64_t tokens() const { return T; }
    void check_shape() const { check_maxsim_shape(T, C, k); }
    void check_batch(uint64_t n) const { check_maxsim_batch(n, T); }
    void check_inputs(uint64_t n) const { check_maxsim_tokens(n_tokens, n, T); }
    void check_on(const cph_index*, uint32_t) const {}
    void stage(RerankScratch&, uint64_t, hipStream_t) const {}
    RerankOuts outs(int32_t* keys, float* score, int32_t* hits, int64_t* rows, int32_t* found) const {
        return {{{keys, 4 * k}, {score, 4 * k}, {hits, 4 * k}, {rows, 8 * k * T}, {found, 4}}, 5};
    }
    void pass(cph_index* h, RerankScratch& gs, uint64_t n, const int32_t* d_key_of, const float*, const RerankOuts& o, hipStream_t st) const {
        const int32_t* d_tokens = nullptr;
        if (n_tokens) {
            Reserve r = gs.reserve();
            std::memcpy(gs.tab.begin(n * 4, r), n_tokens, n * 4);
            d_tokens = reinterpret_cast<const int32_t*>(gs.tab.send(n * 4, st));
        }
        maxsim_rows(maxsim_args(gs.rows.ids.p, gs.rows.dist.p, d_tokens, T, C, k, d_key_of, h->size(), h->ids_input ? h->d_rows.p : nullptr, o),
                    (uint32_t)n, h->device, st);
    }
};

// ---- maxsim with exact rescoring (device_maxsim_rescore.h, host_maxsim_rescore.h) ----
void check_maxsim_rescore_shape(uint64_t T, uint64_t C, uint64_t k, uint64_t R) {
    check_maxsim_shape(T, C, k);
    if (R < k || R > kMaxsimRescoreMax)
        throw InvalidArg("maxsim search supports k <= rescore <= " + std::to_string(kMaxsimRescoreMax) + ", got rescore = " + std::to_string(R) +
                         " at k = " + std::to_string(k));
}

void check_maxsim_rescore_batch(uint64_t n, uint64_t T, uint64_t R) {
    check_maxsim_batch(n, T);
    if (n * R > 0x7FFFFFFFull)
        throw InvalidArg("batch too large: rescored maxsim search needs n * rescore <= 2147483647 (got " + std::to_string(n) + " * " +
                         std::to_string(R) + ")");
}

// The inverted column of a rescored call's keys: the cached one, or made now -- a download of the column, a host sort and an
// upload, which WAIT for the device (the one exception to enqueue-only; cph_prepare_maxsim_rescore makes it ahead of time).
// The caller holds the handle mutex and has set the device.
const KeyRows& key_rows(cph_index* h, const cph_group_keys* keys, const int32_t* d_key_of) {
    std::unique_ptr<KeyRows>& slot = keys ? keys->rows : h->label_rows;
    const uint64_t size = h->size();
    if (slot && slot->size == size && slot->column == d_key_of) return *slot;
    if (slot) quiesce(h);                                 // (a batch in flight may read the one that goes)
    slot.reset();
    std::vector<int32_t> col(size), ukeys(size);
    std::vector<uint32_t> ids(size), offs(size + 1);
    if (size) HIP_CHECK(hipMemcpy(col.data(), d_key_of, size * 4, hipMemcpyDeviceToHost));
    const uint64_t nk = key_rows_host(col.data(), size, ids.data(), ukeys.data(), offs.data());
    std::unique_ptr<KeyRows> kr(new KeyRows());
    kr->ids.alloc(std::max<uint64_t>(size, 1));
    kr->keys.alloc(std::max<uint64_t>(nk, 1));
    kr->offsets.alloc(nk + 1);
    if (size) HIP_CHECK(hipMemcpy(kr->ids.p, ids.data(), size * 4, hipMemcpyHostToDevice));
    if (nk) HIP_CHECK(hipMemcpy(kr->keys.p, ukeys.data(), nk * 4, hipMemcpyHostToDevice));
    HIP_CHECK(hipMemcpy(kr->offsets.p, offs.data(), (nk + 1) * 4, hipMemcpyHostToDevice));
    kr->n_keys = (uint32_t)nk;
    kr->size = size;
    kr->column = d_key_of;
    slot = std::move(kr);
    return *slot;
}

// What a rescored maxsim call sends from the host: n_tokens, and the filter a query runs under -- filter_of and the table of
// bitmap pointers -- as one staged table ([F pointers | n x int32 | n x int32], every piece only if the call has it) on `st`;
// the one host wait is for the copy this set carried the last time.  `hold` keeps the effective filters (F & ~R) until the
// call is enqueued.  Called from the pass: `st` already waits for the set's previous batch.
struct RescoreTables {
    const int32_t* d_tokens = nullptr;
    const int32_t* d_filter_of = nullptr;
    const uint32_t* const* d_bitmaps = nullptr;
    const uint32_t* unfiltered = nullptr;
    std::vector<std::shared_ptr<const cph_filter>> hold;
};

void send_rescore_tables(cph_index* h, RerankScratch& gs, Reserve& r, const int32_t* n_tokens, const cph_filter* const* filters, uint32_t F,
                         const int32_t* filter_of, uint64_t n, hipStream_t st, RescoreTables& out) {
    auto words = [&](const cph_filter* f) -> const uint32_t* {
        out.hold.push_back(effective_filter(h, f));
        return out.hold.back() ? out.hold.back()->words.p : nullptr;
    };
    out.unfiltered = words(!filter_of && F ? filters[0] : nullptr);
    size_t need = 0;
    const size_t o_ptr = table_take(need, filter_of ? (size_t)F * 8 : 0), o_fof = table_take(need, filter_of ? n * 4 : 0),
                 o_tok = table_take(need, n_tokens ? n * 4 : 0);
    if (!need) return;
    uint8_t* const tb = gs.tab.begin(need, r);
    if (filter_of) {
        for (uint32_t f = 0; f < F; ++f) {
            const uint64_t p = reinterpret_cast<uint64_t>(words(filters[f]));
            std::memcpy(tb + o_ptr + (size_t)f * 8, &p, 8);
        }
        std::memcpy(tb + o_fof, filter_of, n * 4);
    }
    if (n_tokens) std::memcpy(tb + o_tok, n_tokens, n * 4);
    const uint8_t* const dt = gs.tab.send(need, st);
    if (filter_of) {
        out.d_bitmaps = reinterpret_cast<const uint32_t* const*>(dt + o_ptr);
        out.d_filter_of = reinterpret_cast<const int32_t*>(dt + o_fof);
    }
    if (n_tokens) out.d_tokens = reinterpret_cast<const int32_t*>(dt + o_tok);
}

MaxsimRescoreArgs maxsim_rescore_args(const cph_index* h, const KeyRows& kr, const RerankScratch::Padded& p, const RerankScratch::Cand& c,
                                      const RescoreTables& t, uint64_t T, uint64_t R, uint64_t k, const RerankOuts& o) {
    MaxsimRescoreArgs a{};
    a.s.raw = h->d_raw.p;
    a.s.norm_sq = h->d_norm.p;
    a.s.qpad = p.qpad.p;
    a.s.qnorm = p.qnorm.p;
    a.s.D = h->L.D;
    a.csr = KeyRowsDev{kr.ids.p, kr.keys.p, kr.offsets.p, kr.n_keys};
    a.cand_keys = c.keys.p;
    a.cand_lb = c.lb.p;
    a.cand_found = c.found.p;
    a.n_tokens = t.d_tokens;
    a.filter_of = t.d_filter_of;
    a.bitmaps = t.d_bitmaps;
    a.unfiltered = t.unfiltered;
    a.T = (uint32_t)T;
    a.R = (uint32_t)R;
    a.k = (uint32_t)k;
    a.n_ids = (uint32_t)h->size();
    a.sc_score = c.score.p;
    a.sc_rows = c.rows.p;
    a.rows = h->ids_input ? h->d_rows.p : nullptr;
    a.out_keys = o.at<int32_t>(0);
    a.out_score = o.at<float>(1);
    a.out_hits = o.at<int32_t>(2);
    a.out_rows = o.at<int64_t>(3);
    a.out_found = o.at<int32_t>(4);
    a.out_certified = o.at<int32_t>(5);
    return a;
}

// `rows` token rows as the search saw them (cosine: normalised into p.q), padded with their norms into the buffers of `p`,
// which grow as they must; on `st` (rescored maxsim and fused search).
void pad_rescore_tokens(cph_index* h, Reserve& r, RerankScratch::Padded& p, const float* d_tokens_raw, uint64_t rows, hipStream_t st) {
    const float* src = d_tokens_raw;
    if (h->metric == CPH_METRIC_COSINE) {
        normalize_rows(d_tokens_raw, r(p.q, rows * h->dim), rows, (uint32_t)h->dim, (uint32_t)h->dim, (uint32_t)h->dim, nullptr, nullptr, st);
        src = p.q.p;
    }
    r(p.qpad, (rows + kExactQT) * h->L.D);
    r(p.qnorm, rows + kExactQT);
    pad_queries(h, src, nullptr, (uint32_t)rows, (uint32_t)rows + kExactQT, p.qpad.p, p.qnorm.p, r(p.stats, kStatWords), 0, st);
}

// The lower-bound pass at k = R into the set's scratch, then the pad, the scan and the select.  The call's filters and keys
// object ride along: the exact terms run under the same effective filters as the search.
struct MaxsimRescoredSearch {
    uint64_t T;
    const int32_t* n_tokens;
    uint64_t k, C, R;
    const cph_group_keys* keys_obj;
    const cph_filter* const* filters;
    uint32_t F;
    const int32_t* filter_of;
    static constexpr PassKind kind = kPassUntimed;       // (the scan kernel alone is timed, inside the pass)
    static constexpr bool keyed = true;
    static constexpr const char* name = "maxsim";
    uint64_t tokens() const { return T; }
    void check_shape() const { check_maxsim_rescore_shape(T, C, k, R); }
    void check_batch(uint64_t n) const { check_maxsim_rescore_batch(n, T, R); }
    void check_inputs(uint64_t n) const { check_maxsim_tokens(n_tokens, n, T); }
    void check_on(const cph_index*, uint32_t) const {}
    void stage(RerankScratch&, uint64_t, hipStream_t) const {}
    RerankOuts outs(int32_t* keys, float* score, int32_t* hits, int64_t* rows, int32_t* found, int32_t* certified) const {
        return {{{keys, 4 * k}, {score, 4 * k}, {hits, 4 * k}, {rows, 8 * k * T}, {found, 4}, {certified, 4}}, 6};
    }
    void pass(cph_index* h, RerankScratch& gs, uint64_t n, const int32_t* d_key_of, const float* d_queries, const RerankOuts& o,
              hipStream_t st) const {
        const KeyRows& kr = key_rows(h, keys_obj, d_key_of);
        Reserve r = gs.reserve();
        RerankScratch::Cand& c = gs.cand;
        const size_t nr = n * R;
        const RerankOuts cand = {{{r(c.keys, nr), 4 * R}, {r(c.lb, nr), 4 * R}, {r(c.hits, nr), 4 * R}, {nullptr, 0}, {r(c.found, n), 4}}, 5};
        r(c.score, nr);
        r(c.rows, nr * T);
        RescoreTables rt;
        send_rescore_tables(h, gs, r, n_tokens, filters, F, filter_of, n, st, rt);
        maxsim_rows(maxsim_args(gs.rows.ids.p, gs.rows.dist.p, rt.d_tokens, T, C, R, d_key_of, h->size(), nullptr, cand), (uint32_t)n, h->device, st);
        pad_rescore_tokens(h, r, gs.pad, d_queries, n * T, st);
        const MaxsimRescoreArgs a = maxsim_rescore_args(h, kr, gs.pad, c, rt, T, R, k, o);
        timed_pass(h->pass_timer[kPassMaxsimRescore], st, [&] { maxsim_rescore_scan(a, (uint32_t)n, st); });
        maxsim_rescore_select(a, (uint32_t)n, st);
    }
};

// ---- fused search: several vectors per query, exact weighted-sum top-k (device_fused.h, host_fused.h) ----
void check_fused_shape(uint64_t T, uint64_t C, uint64_t k) {
    if (T < 1 || T > kFusedMaxVectors)
        throw InvalidArg("fused search supports 1 <= vectors <= " + std::to_string(kFusedMaxVectors) + ", got " + std::to_string(T));
    if (C < 1 || C > kFusedMaxCandidates)
        throw InvalidArg("fused search supports 1 <= candidates <= " + std::to_string(kFusedMaxCandidates) + ", got " + std::to_string(C));
    if (T * C > kFusedMaxEntries)
        throw InvalidArg("fused search needs vectors * candidates <= " + std::to_string(kFusedMaxEntries) + " (got " + std::to_string(T) +
                         " * " + std::to_string(C) + ")");
    if (k < 1 || k > kFusedMaxK || k > T * C)
        throw InvalidArg("fused search supports 1 <= k <= min(" + std::to_string(kFusedMaxK) + ", vectors * candidates), got " +
                         std::to_string(k));
}

// n * vectors is the batch of the underlying search; the scan's grid is one workgroup per block of union slots.
void check_fused_batch(uint64_t n, uint64_t T, uint64_t C) {
    if (n > 0x7FFFFFFFull || n * T > 0x7FFFFFFFull)
        throw InvalidArg("batch too large: fused search needs n * vectors <= 2147483647 (got " + std::to_string(n) + " * " + std::to_string(T) + ")");
    if (n * ((T * C + kFusedItemSlots - 1) / kFusedItemSlots) > 0x7FFFFFFFull)
        throw InvalidArg("batch too large: fused search needs n * ceil(vectors * candidates / 64) <= 2147483647");
}

void check_fused_inputs(const int32_t* n_vectors, const float* weights, uint64_t n, uint64_t T) {
    for (uint64_t i = 0; n_vectors && i < n; ++i)
        if (n_vectors[i] < 1 || (uint64_t)n_vectors[i] > T)
            throw InvalidArg("n_vectors[" + std::to_string(i) + "] = " + std::to_string(n_vectors[i]) + " is outside [1, " + std::to_string(T) + "]");
    for (uint64_t i = 0; weights && i < n * T; ++i)
        if (!std::isfinite(weights[i]))
            throw InvalidArg("weights[" + std::to_string(i / T) + "][" + std::to_string(i % T) + "] is not finite");
}

// n_vectors and the weights are host data and travel as the set's staged table ([n * T floats | n x int32]; null weights:
// ones) on `st`; the one host wait is for the copy this set carried the last time.  Called from the pass: `st` already waits
// for the set's previous batch.
struct FusedHostData {
    const float* d_weights = nullptr;
    const int32_t* d_n_vectors = nullptr;
};

FusedHostData send_fused_host_data(RerankScratch& gs, Reserve& r, const int32_t* n_vectors, const float* weights, uint64_t n, uint64_t T,
                                   hipStream_t st) {
    size_t need = 0;
    const size_t o_w = table_take(need, n * T * 4), o_nv = table_take(need, n_vectors ? n * 4 : 0);
    uint8_t* const tb = gs.tab.begin(need, r);
    if (weights) std::memcpy(tb + o_w, weights, n * T * 4);
    else std::fill_n(reinterpret_cast<float*>(tb + o_w), n * T, 1.0f);
    if (n_vectors) std::memcpy(tb + o_nv, n_vectors, n * 4);
    const uint8_t* const dt = gs.tab.send(need, st);
    return {reinterpret_cast<const float*>(dt + o_w), n_vectors ? reinterpret_cast<const int32_t*>(dt + o_nv) : nullptr};
}

FusedArgs fused_args(const cph_index* h, const int64_t* cand, const RerankScratch::Padded& p, const FusedHostData& hd, uint64_t T, uint64_t C,
                     uint64_t k, const RerankScratch::Union& u, const RerankOuts& o) {
    FusedArgs a{};
    a.s.raw = h->d_raw.p;
    a.s.norm_sq = h->d_norm.p;
    a.s.qpad = p.qpad.p;
    a.s.qnorm = p.qnorm.p;
    a.s.D = h->L.D;
    a.cand = cand;
    a.n_vectors = hd.d_n_vectors;
    a.weights = hd.d_weights;
    a.T = (uint32_t)T;
    a.C = (uint32_t)C;
    a.k = (uint32_t)k;
    a.n_ids = (uint32_t)h->size();
    a.u_ids = u.ids.p;
    a.u_hits = u.hits.p;
    a.u_count = u.count.p;
    a.u_score = u.score.p;
    a.rows = h->ids_input ? h->d_rows.p : nullptr;
    a.out_ids = o.at<int64_t>(0);
    a.out_score = o.at<float>(1);
    a.out_hits = o.at<int32_t>(2);
    return a;
}

// The queries are [n][T][dim]: the n * T vectors are one ordinary batch at k = C; the pass forms every query's union, scores it
// exactly against all live vectors and selects.  n_vectors and weights are on the host (null: all T live; every weight 1).
struct FusedSearch {
    uint64_t T;
    const int32_t* n_vectors;
    const float* weights;
    uint64_t k, C;
    static constexpr PassKind kind = kPassUntimed;       // (the scan kernel alone is timed, inside the pass)
    static constexpr bool keyed = false;
    static constexpr const char* name = "fused";
    uint64_t tokens() const { return T; }
    void check_shape() const { check_fused_shape(T, C, k); }
    void check_batch(uint64_t n) const { check_fused_batch(n, T, C); }
    void check_inputs(uint64_t n) const { check_fused_inputs(n_vectors, weights, n, T); }
    void check_on(const cph_index*, uint32_t) const {}
    void stage(RerankScratch&, uint64_t, hipStream_t) const {}
    RerankOuts outs(int64_t* ids, float* score, int32_t* hits) const { return {{{ids, 8 * k}, {score, 4 * k}, {hits, 4 * k}}, 3}; }
    void pass(cph_index* h, RerankScratch& gs, uint64_t n, const int32_t*, const float* d_queries, const RerankOuts& o, hipStream_t st) const {
        Reserve r = gs.reserve();
        gs.un.reserve(r, n, n * T * C);
        const FusedHostData hd = send_fused_host_data(gs, r, n_vectors, weights, n, T, st);
        pad_rescore_tokens(h, r, gs.pad, d_queries, n * T, st);
        const FusedArgs a = fused_args(h, gs.rows.ids.p, gs.pad, hd, T, C, k, gs.un, o);
        fused_union(a, (uint32_t)n, h->device, st);
        timed_pass(h->pass_timer[kPassFused], st, [&] { fused_scan(a, (uint32_t)n, st); });
        fused_select(a, (uint32_t)n, h->device, st);
    }
};

// ---- the entries, once ----
// What every form checks under the mutex before it touches the device; false: n == 0, nothing to do.
template <class Rerank>
bool rerank_has_work(cph_index* h, const Rerank& f, const RerankCall& c) {
    require_finalized(h);
    f.check_shape();
    check_filter_args(c);
    f.check_batch(c.n);
    if (c.n == 0) return false;
    if (!c.q || !c.out.all()) throw InvalidArg("null argument");
    f.check_inputs(c.n);
    return true;
}

// The body of both single-handle forms: d_queries and the outputs `o` in device memory, filter_of on the host (a query's
// filter serves its T tokens).
template <class Rerank>
void rerank_locked(cph_index* h, RerankScratch& gs, const Rerank& f, const RerankCall& c, const float* d_queries, const int32_t* d_key_of,
                   const RerankOuts& o, hipStream_t st) {
    const uint64_t T = f.tokens();
    std::vector<int32_t> token_filter;
    if (c.filter_of && T > 1) {
        token_filter.resize(c.n * T);
        for (uint64_t i = 0; i < c.n; ++i) std::fill_n(token_filter.begin() + i * T, T, c.filter_of[i]);
    }
    search_rows_then_pass(h, gs, d_queries, c.n * T, f.C, c.filters, c.F, token_filter.empty() ? c.filter_of : token_filter.data(), c.exact,
                          h->pass_timer[Rerank::kind], st, [&] { f.pass(h, gs, c.n, d_key_of, d_queries, o, st); });
}

// cph_search_X (stream == null: queries and outputs on the host, staged through the scratch set, and the call waits) and
// cph_search_X_device (*stream: everything in device memory, enqueued only).
template <class Rerank>
void rerank_search(cph_index* h, const Rerank& f, const RerankCall& c, const cph_group_keys* keys, void* const* stream = nullptr) {
    if (!h) throw InvalidArg("null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    refuse_ip(h, (std::string(Rerank::name) + " search").c_str());
    if (!rerank_has_work(h, f, c)) return;
    f.check_on(h, 0);
    const int32_t* d_key_of = Rerank::keyed ? group_key_column(h, keys) : nullptr;
    h->use_device();
    if (stream) return rerank_locked(h, next_rerank_scratch(h), f, c, c.q, d_key_of, c.out, reinterpret_cast<hipStream_t>(*stream));
    hipStream_t st = own_stream(h);
    RerankScratch& gs = next_rerank_scratch(h);
    const size_t q_floats = (size_t)c.n * f.tokens() * h->dim;
    const RerankOuts dev = reserve_rerank_scratch(gs, q_floats, c.n, c.out);
    HIP_CHECK(hipMemcpyAsync(gs.host.q.p, c.q, q_floats * 4, hipMemcpyHostToDevice, st));
    f.stage(gs, c.n, st);
    rerank_locked(h, gs, f, c, gs.host.q.p, d_key_of, dev, st);
    for (int i = 0; i < dev.count; ++i) HIP_CHECK(hipMemcpyAsync(c.out.o[i].p, dev.o[i].p, c.n * dev.o[i].stride, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
}

// cph_multi_search_X: sharded by query, never inside one.  keys[r] = the keys object of replica r (or keys == null: every
// replica's label column), filters[f * R + r] = filter f on replica r; the queries, filter_of and the outputs are sliced
// by shard, and shard_call(replica, the shard's call, its keys object, its first query) makes the re-ranker's own
// cph_search_X call on it.
template <class Rerank, class ShardCall>
void rerank_multi(cph_multi* m, const Rerank& f, const RerankCall& c, const cph_group_keys* const* keys, ShardCall shard_call) {
    if (!m) throw InvalidArg("null handle");
    const uint32_t R = (uint32_t)m->reps.size();
    refuse_ip(m->reps[0], (std::string(Rerank::name) + " search").c_str());
    const uint64_t q_floats = f.tokens() * m->reps[0]->dim;
    check_filter_args(c);
    multi_fan_out(m, c.n, [&](cph_index* h, uint32_t r) {
        if (rerank_has_work(h, f, c)) f.check_on(h, r);
        if (Rerank::keyed) {
            if (keys && !keys[r]) throw InvalidArg(std::string("a ") + Rerank::name + " multi-device search needs one keys object per replica");
            (void)group_key_column(h, keys ? keys[r] : nullptr);
        }
        check_replica_filters(h, c.filters, c.F, R, r);
    }, [&] {
        if (c.n && c.filter_of) check_filter_of(c.filter_of, c.n, c.F);
        return c.n != 0;
    }, [&](const Shard& s, size_t) {
        const std::vector<const cph_filter*> fr = replica_filters(c.filters, c.F, R, s.replica);
        RerankCall sub = c;
        sub.q = c.q ? c.q + s.lo * q_floats : nullptr;
        sub.n = s.hi - s.lo;
        sub.filters = c.F ? fr.data() : nullptr;
        sub.filter_of = c.filter_of ? c.filter_of + s.lo : nullptr;
        for (int i = 0; i < c.out.count; ++i)
            sub.out.o[i].p = c.out.o[i].p ? static_cast<char*>(c.out.o[i].p) + s.lo * c.out.o[i].stride : nullptr;
        return shard_call(m->reps[s.replica], sub, keys ? keys[s.replica] : nullptr, s.lo);
    });
}

// ---- what the kernel hooks share ----
// A host array on the device (null: one element nobody reads).
template <class T>
DevBuf<T> uploaded(const T* src, size_t n) {
    DevBuf<T> d(src ? n : 1);
    if (src) HIP_CHECK(hipMemcpy(d.p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

// Device twins of a hook's outputs that start as 0xA5 bytes (every slot the kernel leaves alone shows): `dev` is the table
// the kernel writes, download() waits for the device and fills the host arrays.
struct PoisonedOuts {
    const RerankOuts host;
    const uint64_t n;
    DevBuf<uint8_t> buf[kMaxRerankOuts];
    RerankOuts dev;
    PoisonedOuts(const RerankOuts& host_, uint64_t n_) : host(host_), n(n_), dev(host_) {
        for (int i = 0; i < host.count; ++i) {
            buf[i].alloc(n * host.o[i].stride);
            HIP_CHECK(hipMemset(buf[i].p, 0xA5, n * host.o[i].stride));
            dev.o[i].p = buf[i].p;
        }
    }
    void download() {
        HIP_CHECK(hipDeviceSynchronize());
        for (int i = 0; i < host.count; ++i) HIP_CHECK(hipMemcpy(host.o[i].p, buf[i].p, n * host.o[i].stride, hipMemcpyDeviceToHost));
    }
};

}  // namespace

extern "C" {

int cph_group_keys_create(cph_index* h, const int32_t* keys, uint64_t size, int space, cph_group_keys** out) {
    return guarded([&] {
        if (!out) throw InvalidArg("null argument");
        *out = nullptr;
        if (!h || (!keys && size != 0)) throw InvalidArg("null argument");
        if (space != CPH_IDS_INTERNAL && space != CPH_IDS_INPUT) throw InvalidArg("id space must be CPH_IDS_INTERNAL or CPH_IDS_INPUT");
        std::lock_guard<std::mutex> lk(h->mu);
        if (!h->finalized) throw InvalidArg("group keys belong to a finalized index: finalize or load it first");
        if (size != h->size())
            throw InvalidArg("group keys have " + std::to_string(size) + " entries, the index holds " + std::to_string(h->size()));
        h->use_device();
        std::vector<int32_t> internal;
        const int32_t* src = keys;
        if (space == CPH_IDS_INPUT) {
            const uint64_t nb = h->host.n;
            if (!h->has_rows) throw InvalidArg("the index has no row map (it was loaded from a v2 file): keys in input rows need cph_set_row_map");
            std::vector<uint32_t> rows(h->host.rows);
            if (rows.size() != nb) {                       // a replica without host arrays: its device copy
                rows.resize(nb);
                if (nb) HIP_CHECK(hipMemcpy(rows.data(), h->d_rows.p, nb * 4, hipMemcpyDeviceToHost));
            }
            internal.resize(size);
            labels_to_internal_host(keys, rows.data(), nb, internal.data());
            std::copy(keys + nb, keys + size, internal.begin() + nb);      // (a tail row is its own input row)
            src = internal.data();
        }
        std::unique_ptr<cph_group_keys> gk(new cph_group_keys());
        gk->h = h;
        gk->epoch = h->index_epoch;
        gk->device = h->device;
        gk->size = size;
        gk->keys.alloc(std::max<uint64_t>(size, 1));
        if (size) HIP_CHECK(hipMemcpy(gk->keys.p, src, size * 4, hipMemcpyHostToDevice));
        *out = gk.release();
    });
}

int cph_group_keys_destroy(cph_group_keys* keys) {
    return guarded([&] {
        if (!keys) return;
        std::unique_ptr<cph_group_keys> own(keys);
        if (hipSetDevice(keys->device) == hipSuccess) (void)hipDeviceSynchronize();     // a batch in flight may read the column
    });
}

// ---- grouped search: the k best key groups, up to g rows of each (host_group.h) ----
int cph_search_grouped(cph_index* h, const float* queries, uint64_t n, uint64_t k, uint64_t group_size, uint64_t candidates,
                       const cph_group_keys* keys, const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                       int exact, int64_t* ids, float* dist, int32_t* group_keys, int32_t* counts, uint8_t* complete) {
    return guarded([&] {
        const GroupedSearch f{k, group_size, candidates};
        rerank_search(h, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(ids, dist, group_keys, counts, complete)}, keys);
    });
}

int cph_search_grouped_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k, uint64_t group_size, uint64_t candidates,
                              const cph_group_keys* keys, const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                              int exact, int64_t* d_ids, float* d_dist, int32_t* d_group_keys, int32_t* d_counts, uint8_t* d_complete,
                              void* stream) {
    return guarded([&] {
        const GroupedSearch f{k, group_size, candidates};
        rerank_search(h, f, {d_queries, n, filters, n_filters, filter_of, exact != 0, f.outs(d_ids, d_dist, d_group_keys, d_counts, d_complete)},
                      keys, &stream);
    });
}

int cph_multi_search_grouped(cph_multi* m, const float* queries, uint64_t n, uint64_t k, uint64_t group_size, uint64_t candidates,
                             const cph_group_keys* const* keys, const cph_filter* const* filters, uint32_t n_filters,
                             const int32_t* filter_of, int exact, int64_t* ids, float* dist, int32_t* group_keys, int32_t* counts,
                             uint8_t* complete) {
    return guarded([&] {
        const GroupedSearch f{k, group_size, candidates};
        rerank_multi(m, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(ids, dist, group_keys, counts, complete)}, keys,
                     [&](cph_index* h, const RerankCall& s, const cph_group_keys* key, uint64_t) {
            return cph_search_grouped(h, s.q, s.n, k, group_size, candidates, key, s.filters, s.F, s.filter_of, s.exact ? 1 : 0,
                                      s.out.at<int64_t>(0), s.out.at<float>(1), s.out.at<int32_t>(2), s.out.at<int32_t>(3),
                                      s.out.at<uint8_t>(4));
        });
    });
}

int cph_debug_time_grouped(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassGrouped, on != 0); });
}

int cph_debug_last_group_rows_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassGrouped, us); });
}

int cph_group_rows_hook(int device, const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const int32_t* key_of,
                        uint64_t n_keys, const uint32_t* rows, uint64_t k, uint64_t group_size, int64_t* out_ids, float* out_dist,
                        int32_t* out_keys, int32_t* out_counts, uint8_t* out_complete) {
    return guarded([&] {
        const RerankOuts o = GroupedSearch{k, group_size, candidates}.outs(out_ids, out_dist, out_keys, out_counts, out_complete);
        check_group_rows_args(ids, dist, n, candidates, key_of, n_keys, k, group_size, o);
        HIP_CHECK(hipSetDevice(device));
        const DevBuf<int64_t> d_ids = uploaded(ids, n * candidates);
        const DevBuf<float> d_dist = uploaded(dist, n * candidates);
        const DevBuf<int32_t> d_key_of = uploaded(key_of, n_keys);
        const DevBuf<uint32_t> d_rows = uploaded(rows, n_keys);
        PoisonedOuts po(o, n);
        group_rows(group_args(d_ids.p, d_dist.p, candidates, k, group_size, d_key_of.p, n_keys, rows ? d_rows.p : nullptr, po.dev), (uint32_t)n,
                   nullptr);
        po.download();
    });
}

int cph_host_group_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const int32_t* key_of, uint64_t n_keys,
                        const uint32_t* rows, uint64_t k, uint64_t group_size, int64_t* out_ids, float* out_dist, int32_t* out_keys,
                        int32_t* out_counts, uint8_t* out_complete) {
    return guarded([&] {
        check_group_rows_args(ids, dist, n, candidates, key_of, n_keys, k, group_size,
                              GroupedSearch{k, group_size, candidates}.outs(out_ids, out_dist, out_keys, out_counts, out_complete));
        group_rows_host(ids, dist, n, (uint32_t)candidates, key_of, rows, (uint32_t)k, (uint32_t)group_size, out_ids, out_dist, out_keys,
                        out_counts, out_complete);
    });
}

// ---- diversified search: MMR re-ranking of a candidate row (host_diverse.h) ----
int cph_search_diverse(cph_index* h, const float* queries, uint64_t n, uint64_t k, float lam, uint64_t candidates,
                       const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids, float* dist,
                       float* gap) {
    return guarded([&] {
        const DiverseSearch f{k, lam, candidates};
        rerank_search(h, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(ids, dist, gap)}, nullptr);
    });
}

int cph_search_diverse_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k, float lam, uint64_t candidates,
                              const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* d_ids,
                              float* d_dist, float* d_gap, void* stream) {
    return guarded([&] {
        const DiverseSearch f{k, lam, candidates};
        rerank_search(h, f, {d_queries, n, filters, n_filters, filter_of, exact != 0, f.outs(d_ids, d_dist, d_gap)}, nullptr, &stream);
    });
}

int cph_multi_search_diverse(cph_multi* m, const float* queries, uint64_t n, uint64_t k, float lam, uint64_t candidates,
                             const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids,
                             float* dist, float* gap) {
    return guarded([&] {
        const DiverseSearch f{k, lam, candidates};
        rerank_multi(m, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(ids, dist, gap)}, nullptr,
                     [&](cph_index* h, const RerankCall& s, const cph_group_keys*, uint64_t) {
            return cph_search_diverse(h, s.q, s.n, k, lam, candidates, s.filters, s.F, s.filter_of, s.exact ? 1 : 0, s.out.at<int64_t>(0),
                                      s.out.at<float>(1), s.out.at<float>(2));
        });
    });
}

int cph_debug_time_diverse(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassDiverse, on != 0); });
}

int cph_debug_last_diverse_rows_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassDiverse, us); });
}

int cph_diverse_rows_hook(cph_index* h, const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, uint64_t k, float lam,
                          int64_t* out_ids, float* out_dist, float* out_gap) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        const RerankOuts o = DiverseSearch{k, lam, candidates}.outs(out_ids, out_dist, out_gap);
        check_diverse_rows_args(ids, dist, n, candidates, h->size(), k, lam, o);
        h->use_device();
        const DevBuf<int64_t> d_ids = uploaded(ids, n * candidates);
        const DevBuf<float> d_dist = uploaded(dist, n * candidates);
        PoisonedOuts po(o, n);
        diverse_rows(diverse_args(h, d_ids.p, d_dist.p, candidates, k, lam, po.dev), (uint32_t)n, nullptr);
        po.download();
    });
}

int cph_host_diverse_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const float* raw, const float* norm_sq,
                          uint64_t n_ids, uint64_t D, const uint32_t* rows, uint64_t k, float lam, int64_t* out_ids, float* out_dist,
                          float* out_gap) {
    return guarded([&] {
        if (!raw || !norm_sq) throw InvalidArg("null argument");
        if (D < 8 || D > 0xFFFFFFFFull || (D & 7)) throw InvalidArg("diverse rows: D must be a multiple of 8");
        check_diverse_rows_args(ids, dist, n, candidates, n_ids, k, lam, DiverseSearch{k, lam, candidates}.outs(out_ids, out_dist, out_gap));
        diverse_rows_host(ids, dist, n, (uint32_t)candidates, raw, norm_sq, n_ids, (uint32_t)D, rows, (uint32_t)k, lam, out_ids, out_dist,
                          out_gap);
    });
}

// ---- multi-vector search: MaxSim over key groups (host_maxsim.h) ----
int cph_search_maxsim(cph_index* h, const float* queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                      uint64_t candidates, const cph_group_keys* keys, const cph_filter* const* filters, uint32_t n_filters,
                      const int32_t* filter_of, int exact, int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows,
                      int32_t* out_found) {
    return guarded([&] {
        const MaxsimSearch f{tokens, n_tokens, k, candidates};
        rerank_search(h, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(out_keys, out_score, out_hits, out_rows, out_found)},
                      keys);
    });
}

int cph_search_maxsim_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                             uint64_t candidates, const cph_group_keys* keys, const cph_filter* const* filters, uint32_t n_filters,
                             const int32_t* filter_of, int exact, int32_t* d_keys, float* d_score, int32_t* d_hits, int64_t* d_rows,
                             int32_t* d_found, void* stream) {
    return guarded([&] {
        const MaxsimSearch f{tokens, n_tokens, k, candidates};
        rerank_search(h, f, {d_queries, n, filters, n_filters, filter_of, exact != 0, f.outs(d_keys, d_score, d_hits, d_rows, d_found)}, keys,
                      &stream);
    });
}

int cph_multi_search_maxsim(cph_multi* m, const float* queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                            uint64_t candidates, const cph_group_keys* const* keys, const cph_filter* const* filters, uint32_t n_filters,
                            const int32_t* filter_of, int exact, int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows,
                            int32_t* out_found) {
    return guarded([&] {
        const MaxsimSearch f{tokens, n_tokens, k, candidates};
        rerank_multi(m, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(out_keys, out_score, out_hits, out_rows, out_found)},
                     keys, [&](cph_index* h, const RerankCall& s, const cph_group_keys* key, uint64_t lo) {
            return cph_search_maxsim(h, s.q, s.n, tokens, n_tokens ? n_tokens + lo : nullptr, k, candidates, key, s.filters, s.F, s.filter_of,
                                     s.exact ? 1 : 0, s.out.at<int32_t>(0), s.out.at<float>(1), s.out.at<int32_t>(2), s.out.at<int64_t>(3),
                                     s.out.at<int32_t>(4));
        });
    });
}

int cph_debug_time_maxsim(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassMaxsim, on != 0); });
}

int cph_debug_last_maxsim_rows_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassMaxsim, us); });
}

int cph_maxsim_rows_hook(int device, const int64_t* ids, const float* dist, uint64_t n, uint64_t tokens, const int32_t* n_tokens,
                         uint64_t candidates, const int32_t* key_of, uint64_t n_keys, const uint32_t* rows, uint64_t k, int32_t* out_keys,
                         float* out_score, int32_t* out_hits, int64_t* out_rows, int32_t* out_found) {
    return guarded([&] {
        const RerankOuts o = MaxsimSearch{tokens, n_tokens, k, candidates}.outs(out_keys, out_score, out_hits, out_rows, out_found);
        check_maxsim_rows_args(ids, dist, n, tokens, n_tokens, candidates, key_of, n_keys, k, o);
        HIP_CHECK(hipSetDevice(device));
        const DevBuf<int64_t> d_ids = uploaded(ids, n * tokens * candidates);
        const DevBuf<float> d_dist = uploaded(dist, n * tokens * candidates);
        const DevBuf<int32_t> d_key_of = uploaded(key_of, n_keys), d_tok = uploaded(n_tokens, n);
        const DevBuf<uint32_t> d_rows = uploaded(rows, n_keys);
        PoisonedOuts po(o, n);
        maxsim_rows(maxsim_args(d_ids.p, d_dist.p, n_tokens ? d_tok.p : nullptr, tokens, candidates, k, d_key_of.p, n_keys,
                                rows ? d_rows.p : nullptr, po.dev),
                    (uint32_t)n, device, nullptr);
        po.download();
    });
}

int cph_host_maxsim_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t candidates,
                         const int32_t* key_of, uint64_t n_keys, const uint32_t* rows, uint64_t k, int32_t* out_keys, float* out_score,
                         int32_t* out_hits, int64_t* out_rows, int32_t* out_found) {
    return guarded([&] {
        check_maxsim_rows_args(ids, dist, n, tokens, n_tokens, candidates, key_of, n_keys, k,
                               MaxsimSearch{tokens, n_tokens, k, candidates}.outs(out_keys, out_score, out_hits, out_rows, out_found));
        maxsim_rows_host(ids, dist, n, (uint32_t)tokens, n_tokens, (uint32_t)candidates, key_of, n_keys, rows, (uint32_t)k, out_keys,
                         out_score, out_hits, out_rows, out_found);
    });
}

// ---- multi-vector search with exact rescoring of the best R keys (host_maxsim_rescore.h) ----
int cph_search_maxsim_rescored(cph_index* h, const float* queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                               uint64_t candidates, uint64_t rescore, const cph_group_keys* keys, const cph_filter* const* filters,
                               uint32_t n_filters, const int32_t* filter_of, int exact, int32_t* out_keys, float* out_score,
                               int32_t* out_hits, int64_t* out_rows, int32_t* out_found, int32_t* out_certified) {
    return guarded([&] {
        const MaxsimRescoredSearch f{tokens, n_tokens, k, candidates, rescore, keys, filters, n_filters, filter_of};
        rerank_search(h, f, {queries, n, filters, n_filters, filter_of, exact != 0,
                             f.outs(out_keys, out_score, out_hits, out_rows, out_found, out_certified)}, keys);
    });
}

int cph_search_maxsim_rescored_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                                      uint64_t candidates, uint64_t rescore, const cph_group_keys* keys, const cph_filter* const* filters,
                                      uint32_t n_filters, const int32_t* filter_of, int exact, int32_t* d_keys, float* d_score,
                                      int32_t* d_hits, int64_t* d_rows, int32_t* d_found, int32_t* d_certified, void* stream) {
    return guarded([&] {
        const MaxsimRescoredSearch f{tokens, n_tokens, k, candidates, rescore, keys, filters, n_filters, filter_of};
        rerank_search(h, f, {d_queries, n, filters, n_filters, filter_of, exact != 0, f.outs(d_keys, d_score, d_hits, d_rows, d_found, d_certified)},
                      keys, &stream);
    });
}

int cph_multi_search_maxsim_rescored(cph_multi* m, const float* queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                                     uint64_t candidates, uint64_t rescore, const cph_group_keys* const* keys,
                                     const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact,
                                     int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows, int32_t* out_found,
                                     int32_t* out_certified) {
    return guarded([&] {
        const MaxsimRescoredSearch f{tokens, n_tokens, k, candidates, rescore, nullptr, filters, n_filters, filter_of};
        rerank_multi(m, f, {queries, n, filters, n_filters, filter_of, exact != 0,
                            f.outs(out_keys, out_score, out_hits, out_rows, out_found, out_certified)},
                     keys, [&](cph_index* h, const RerankCall& s, const cph_group_keys* key, uint64_t lo) {
            return cph_search_maxsim_rescored(h, s.q, s.n, tokens, n_tokens ? n_tokens + lo : nullptr, k, candidates, rescore, key, s.filters, s.F,
                                              s.filter_of, s.exact ? 1 : 0, s.out.at<int32_t>(0), s.out.at<float>(1), s.out.at<int32_t>(2),
                                              s.out.at<int64_t>(3), s.out.at<int32_t>(4), s.out.at<int32_t>(5));
        });
    });
}

int cph_prepare_maxsim_rescore(cph_index* h, const cph_group_keys* keys) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        refuse_ip(h, "maxsim search");
        require_finalized(h);
        const int32_t* d_key_of = group_key_column(h, keys);
        h->use_device();
        (void)key_rows(h, keys, d_key_of);
    });
}

int cph_debug_time_maxsim_rescore(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassMaxsimRescore, on != 0); });
}

int cph_debug_last_maxsim_rescore_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassMaxsimRescore, us); });
}

static void check_maxsim_rescore_args(const int32_t* cand_keys, const float* cand_lb, const int32_t* cand_found, uint64_t n, uint64_t R,
                                      const float* tokens, uint64_t T, const int32_t* n_tokens, uint64_t k, const RerankOuts& o) {
    if (!cand_keys || !cand_lb || !cand_found || !tokens || !o.all()) throw InvalidArg("null argument");
    check_maxsim_rescore_shape(T, 1, k, R);
    if (n < 1) throw InvalidArg("maxsim rescore: sizes out of range");
    check_maxsim_rescore_batch(n, T, R);
    check_maxsim_tokens(n_tokens, n, T);
    for (uint64_t i = 0; i < n; ++i)
        if (cand_found[i] < 0 || (uint64_t)cand_found[i] > R)
            throw InvalidArg("cand_found[" + std::to_string(i) + "] = " + std::to_string(cand_found[i]) + " is outside [0, " + std::to_string(R) + "]");
}

int cph_maxsim_rescore_hook(cph_index* h, const int32_t* cand_keys, const float* cand_lb, const int32_t* cand_found, uint64_t n,
                            uint64_t rescore, const float* tokens, uint64_t n_tok, const int32_t* n_tokens, const cph_group_keys* keys,
                            const uint32_t* allow, uint64_t k, int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows,
                            int32_t* out_found, int32_t* out_certified) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        refuse_ip(h, "maxsim search");
        require_finalized(h);
        const MaxsimRescoredSearch f{n_tok, n_tokens, k, 1, rescore, keys, nullptr, 0, nullptr};
        const RerankOuts o = f.outs(out_keys, out_score, out_hits, out_rows, out_found, out_certified);
        check_maxsim_rescore_args(cand_keys, cand_lb, cand_found, n, rescore, tokens, n_tok, n_tokens, k, o);
        const int32_t* d_key_of = group_key_column(h, keys);
        h->use_device();
        const KeyRows& kr = key_rows(h, keys, d_key_of);
        const uint64_t T = n_tok, R = rescore, rows = n * T, nw = (h->size() + 31) / 32;
        RerankScratch::Padded pad;
        RerankScratch::Cand c;
        c.keys = uploaded(cand_keys, n * R);
        c.found = uploaded(cand_found, n);
        c.lb = uploaded(cand_lb, n * R);
        c.score.alloc(n * R);
        c.rows.alloc(n * R * T);
        const DevBuf<int32_t> d_tok = uploaded(n_tokens, n);
        const DevBuf<float> d_q = uploaded(tokens, rows * h->dim);
        const DevBuf<uint32_t> d_allow = uploaded(allow, n * nw);
        std::vector<uint64_t> ptrs(n);
        std::vector<int32_t> of(n);
        for (uint64_t i = 0; i < n; ++i) {
            ptrs[i] = reinterpret_cast<uint64_t>(d_allow.p + i * nw);
            of[i] = (int32_t)i;
        }
        const DevBuf<uint64_t> d_ptrs = uploaded(allow ? ptrs.data() : nullptr, n);
        const DevBuf<int32_t> d_of = uploaded(allow ? of.data() : nullptr, n);
        RescoreTables rt;
        if (n_tokens) rt.d_tokens = d_tok.p;
        if (allow) rt.d_filter_of = d_of.p;
        if (allow) rt.d_bitmaps = reinterpret_cast<const uint32_t* const*>(d_ptrs.p);
        PoisonedOuts po(o, n);
        Reserve fresh{nullptr, false};
        pad_rescore_tokens(h, fresh, pad, d_q.p, rows, nullptr);
        const MaxsimRescoreArgs a = maxsim_rescore_args(h, kr, pad, c, rt, T, R, k, po.dev);
        maxsim_rescore_scan(a, (uint32_t)n, nullptr);
        maxsim_rescore_select(a, (uint32_t)n, nullptr);
        po.download();
    });
}

int cph_host_maxsim_rescore(const int32_t* cand_keys, const float* cand_lb, const int32_t* cand_found, uint64_t n, uint64_t rescore,
                            const float* tokens, uint64_t n_tok, uint64_t dim, const int32_t* n_tokens, const float* raw,
                            const float* norm_sq, uint64_t n_ids, uint64_t D, const int32_t* key_of, const uint32_t* allow,
                            const uint32_t* rows, uint64_t k, int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows,
                            int32_t* out_found, int32_t* out_certified) {
    return guarded([&] {
        if (!raw || !norm_sq || !key_of) throw InvalidArg("null argument");
        if (D < 8 || D > 0xFFFFFFFFull || (D & 7) || dim < 1 || dim > D) throw InvalidArg("maxsim rescore: D must be a multiple of 8 and dim <= D");
        if (n_ids < 1 || n_ids > 0xFFFFFFFFull) throw InvalidArg("maxsim rescore: sizes out of range");
        const MaxsimRescoredSearch f{n_tok, n_tokens, k, 1, rescore, nullptr, nullptr, 0, nullptr};
        check_maxsim_rescore_args(cand_keys, cand_lb, cand_found, n, rescore, tokens, n_tok, n_tokens, k,
                                  f.outs(out_keys, out_score, out_hits, out_rows, out_found, out_certified));
        maxsim_rescore_host(cand_keys, cand_lb, cand_found, n, (uint32_t)rescore, tokens, (uint32_t)n_tok, (uint32_t)dim, n_tokens, raw, norm_sq,
                            n_ids, (uint32_t)D, key_of, allow, rows, (uint32_t)k, out_keys, out_score, out_hits, out_rows, out_found,
                            out_certified);
    });
}

int cph_host_key_rows(const int32_t* keys, uint64_t n, uint32_t* out_ids, int32_t* out_keys, uint32_t* out_offsets, uint64_t* out_n_keys) {
    return guarded([&] {
        if (!out_offsets || !out_n_keys || (n != 0 && (!keys || !out_ids || !out_keys))) throw InvalidArg("null argument");
        if (n > 0xFFFFFFFEull) throw InvalidArg("key rows: too many ids");
        *out_n_keys = key_rows_host(keys, n, out_ids, out_keys, out_offsets);
    });
}

// ---- fused search: several query vectors per query, exact weighted-sum top-k (host_fused.h) ----
int cph_search_fused(cph_index* h, const float* queries, uint64_t n, uint64_t vectors, const int32_t* n_vectors, const float* weights,
                     uint64_t k, uint64_t candidates, const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                     int exact, int64_t* ids, float* score, int32_t* hits) {
    return guarded([&] {
        const FusedSearch f{vectors, n_vectors, weights, k, candidates};
        rerank_search(h, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(ids, score, hits)}, nullptr);
    });
}

int cph_search_fused_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t vectors, const int32_t* n_vectors,
                            const float* weights, uint64_t k, uint64_t candidates, const cph_filter* const* filters, uint32_t n_filters,
                            const int32_t* filter_of, int exact, int64_t* d_ids, float* d_score, int32_t* d_hits, void* stream) {
    return guarded([&] {
        const FusedSearch f{vectors, n_vectors, weights, k, candidates};
        rerank_search(h, f, {d_queries, n, filters, n_filters, filter_of, exact != 0, f.outs(d_ids, d_score, d_hits)}, nullptr, &stream);
    });
}

int cph_multi_search_fused(cph_multi* m, const float* queries, uint64_t n, uint64_t vectors, const int32_t* n_vectors, const float* weights,
                           uint64_t k, uint64_t candidates, const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                           int exact, int64_t* ids, float* score, int32_t* hits) {
    return guarded([&] {
        const FusedSearch f{vectors, n_vectors, weights, k, candidates};
        rerank_multi(m, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(ids, score, hits)}, nullptr,
                     [&](cph_index* h, const RerankCall& s, const cph_group_keys*, uint64_t lo) {
            return cph_search_fused(h, s.q, s.n, vectors, n_vectors ? n_vectors + lo : nullptr, weights ? weights + lo * vectors : nullptr, k,
                                    candidates, s.filters, s.F, s.filter_of, s.exact ? 1 : 0, s.out.at<int64_t>(0), s.out.at<float>(1),
                                    s.out.at<int32_t>(2));
        });
    });
}

int cph_debug_time_fused(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassFused, on != 0); });
}

int cph_debug_last_fused_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassFused, us); });
}

static void check_fused_rows_args(const int64_t* cand_ids, const float* queries, uint64_t n, uint64_t T, const int32_t* n_vectors,
                                  const float* weights, uint64_t C, uint64_t k, const RerankOuts& o) {
    if (!cand_ids || !queries || !o.all()) throw InvalidArg("null argument");
    check_fused_shape(T, C, k);
    if (n < 1) throw InvalidArg("fused rows: sizes out of range");
    check_fused_batch(n, T, C);
    check_fused_inputs(n_vectors, weights, n, T);
}

int cph_fused_rows_hook(cph_index* h, const int64_t* cand_ids, const float* queries, uint64_t n, uint64_t vectors, const int32_t* n_vectors,
                        const float* weights, uint64_t candidates, uint64_t k, int64_t* out_ids, float* out_score, int32_t* out_hits) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        refuse_ip(h, "fused search");
        require_finalized(h);
        const uint64_t T = vectors, C = candidates, rows = n * T;
        const FusedSearch f{T, n_vectors, weights, k, C};
        const RerankOuts o = f.outs(out_ids, out_score, out_hits);
        check_fused_rows_args(cand_ids, queries, n, T, n_vectors, weights, C, k, o);
        h->use_device();
        std::vector<float> ones;
        if (!weights) ones.assign(rows, 1.0f);
        const DevBuf<int64_t> d_cand = uploaded(cand_ids, rows * C);
        const DevBuf<float> d_q = uploaded(queries, rows * h->dim), d_w = uploaded(weights ? weights : ones.data(), rows);
        const DevBuf<int32_t> d_nv = uploaded(n_vectors, n);
        RerankScratch::Padded pad;
        RerankScratch::Union u;
        PoisonedOuts po(o, n);
        Reserve fresh{nullptr, false};
        u.reserve(fresh, n, rows * C);
        pad_rescore_tokens(h, fresh, pad, d_q.p, rows, nullptr);
        const FusedArgs a = fused_args(h, d_cand.p, pad, {d_w.p, n_vectors ? d_nv.p : nullptr}, T, C, k, u, po.dev);
        fused_union(a, (uint32_t)n, h->device, nullptr);
        fused_scan(a, (uint32_t)n, nullptr);
        fused_select(a, (uint32_t)n, h->device, nullptr);
        po.download();
    });
}

int cph_host_fused_rows(const int64_t* cand_ids, uint64_t n, uint64_t vectors, const int32_t* n_vectors, const float* weights,
                        uint64_t candidates, const float* queries_padded, const float* raw, const float* norm_sq, uint64_t n_ids, uint64_t D,
                        const uint32_t* rows, uint64_t k, int64_t* out_ids, float* out_score, int32_t* out_hits) {
    return guarded([&] {
        if (!raw || !norm_sq) throw InvalidArg("null argument");
        if (D < 8 || D > 0xFFFFFFFFull || (D & 7)) throw InvalidArg("fused rows: D must be a multiple of 8");
        if (n_ids < 1 || n_ids > 0xFFFFFFFFull) throw InvalidArg("fused rows: sizes out of range");
        const FusedSearch f{vectors, n_vectors, weights, k, candidates};
        check_fused_rows_args(cand_ids, queries_padded, n, vectors, n_vectors, weights, candidates, k, f.outs(out_ids, out_score, out_hits));
        fused_rows_host(cand_ids, n, (uint32_t)vectors, n_vectors, weights, (uint32_t)candidates, queries_padded, raw, norm_sq, n_ids,
                        (uint32_t)D, rows, (uint32_t)k, out_ids, out_score, out_hits);
    });
}

}  // extern "C"

// ---- two-stage search: rescoring against resident full-size rows (device_rescore.h, host_rescore.h) --------------------
// A fourth re-ranker on the entry path above.  What is new is its second resident matrix, a cph_rescore_vectors object
// with the lifetime rules of cph_group_keys: one handle, one index_epoch, one device.
struct cph_rescore_vectors {
    cph_index* h = nullptr;
    uint64_t epoch = 0;
    int device = 0;
    uint64_t size = 0;                         // ids it covers
    uint32_t dim = 0;                          // dim_full
    bool f32 = false, ip = false;
    RescoreLayout L{};
    DevBuf<uint8_t> rows;                      // [size][L.stride], internal-id order
    DevBuf<float> norms;                       // [size]
};

namespace {

RescoreStore rescore_store(const cph_rescore_vectors* rv) {
    return RescoreStore{rv->rows.p, rv->norms.p, (uint32_t)rv->size, rv->dim, rv->L.stride, rv->L.pieces, rv->L.padded, rv->L.G, rv->L.log2G};
}

void check_rescore_layout_args(uint64_t dim_full, int dtype, int metric) {
    if (dim_full < 1 || dim_full > kRescoreMaxDim)
        throw InvalidArg("rescore vectors support 1 <= dim_full <= " + std::to_string(kRescoreMaxDim) + ", got " + std::to_string(dim_full));
    if (dtype != CPH_RESCORE_FLOAT16 && dtype != CPH_RESCORE_FLOAT32)
        throw InvalidArg("rescore vectors are stored as CPH_RESCORE_FLOAT16 = 0 or CPH_RESCORE_FLOAT32 = 1");
    if (metric != CPH_RESCORE_L2 && metric != CPH_RESCORE_IP) throw InvalidArg("the metric of rescore vectors is CPH_RESCORE_L2 = 0 or CPH_RESCORE_IP = 1");
}

void refuse_bad_rescore_rows(uint64_t bad, unsigned long long first) {
    if (!bad) return;
    throw InvalidArg("rescore vectors: row " + std::to_string(first) + " holds a NaN or an Inf, a value that overflows float16, or its squared "
                     "norm overflows (" + std::to_string(bad) + " such row" + (bad == 1 ? "" : "s") + " in this call): no object was made");
}

// The object of a rescored call against the handle it runs on.
void check_rescore_vectors(const cph_index* h, const cph_rescore_vectors* rv) {
    if (!rv) throw InvalidArg("rescored search needs a rescore vectors object (cph_rescore_vectors_create)");
    if (rv->device != h->device) throw InvalidArg("rescore vectors belong to another device");
    if (rv->size != h->size())
        throw InvalidArg("rescore vectors cover " + std::to_string(rv->size) + " ids, the index holds " + std::to_string(h->size()));
    if (rv->h != h || rv->epoch != h->index_epoch)
        throw InvalidArg("rescore vectors were made for another index (a load, build or compact invalidates them)");
}

void check_rescore_shape(uint64_t k, uint64_t C) {
    if (k < 1) throw InvalidArg("rescored search needs k >= 1");
    if (C > kRescoreMaxCandidates)
        throw InvalidArg("rescored search supports candidates <= " + std::to_string(kRescoreMaxCandidates) + ", got " + std::to_string(C));
    if (C < k) throw InvalidArg("rescored search needs k <= candidates (got " + std::to_string(k) + " > " + std::to_string(C) + ")");
}

RescoreArgs rescore_args(const RescoreStore& s, bool ip, const int64_t* r_ids, const float* r_dist, const float* d_fq, uint64_t C, uint64_t k,
                         const uint32_t* d_rows, const RerankOuts& o) {
    RescoreArgs a{};
    a.ids = r_ids;
    a.dist = r_dist;
    a.fq = d_fq;
    a.C = (uint32_t)C;
    a.k = (uint32_t)k;
    a.s = s;
    a.ip = ip ? 1 : 0;
    a.rows = d_rows;
    a.out_ids = o.at<int64_t>(0);
    a.out_score = o.at<float>(1);
    a.out_first = o.at<float>(2);
    return a;
}

// vectors[r]: the object of replica r (one handle: r = 0).  full_q: [n][dim_full], on the host (host form: staged into
// the scratch set before the search is enqueued, so that the timed pass is the kernel alone) or on the device.
struct RescoredSearch {
    uint64_t k, C;
    const cph_rescore_vectors* const* vectors;
    const float* full_q;
    uint64_t dim_full;
    bool host_form;
    static constexpr PassKind kind = kPassRescored;
    static constexpr bool keyed = false;
    static constexpr const char* name = "rescored";
    uint64_t tokens() const { return 1; }
    void check_shape() const { check_rescore_shape(k, C); }
    void check_batch(uint64_t n) const { check_batch_size(n); }
    void check_inputs(uint64_t) const {
        if (!full_q) throw InvalidArg("null argument");
    }
    void check_on(const cph_index* h, uint32_t r) const {
        if (!vectors) throw InvalidArg("rescored search needs a rescore vectors object (cph_rescore_vectors_create)");
        check_rescore_vectors(h, vectors[r]);
        if (dim_full != vectors[r]->dim)
            throw InvalidArg("full queries have " + std::to_string(dim_full) + " coordinates, the rescore vectors " + std::to_string(vectors[r]->dim));
    }
    void stage(RerankScratch& gs, uint64_t n, hipStream_t st) const {
        const size_t floats = (size_t)n * dim_full;
        HIP_CHECK(hipMemcpyAsync(gs.reserve()(gs.host.fq, floats), full_q, floats * 4, hipMemcpyHostToDevice, st));
    }
    RerankOuts outs(int64_t* ids, float* score, float* first) const { return {{{ids, 8 * k}, {score, 4 * k}, {first, 4 * k}}, 3}; }
    void pass(cph_index* h, RerankScratch& gs, uint64_t n, const int32_t*, const float*, const RerankOuts& o, hipStream_t st) const {
        const cph_rescore_vectors* rv = vectors[0];
        rescore_rows(rescore_args(rescore_store(rv), rv->ip, gs.rows.ids.p, gs.rows.dist.p, host_form ? gs.host.fq.p : full_q, C, k,
                                  h->ids_input ? h->d_rows.p : nullptr, o),
                     rv->f32, (uint32_t)n, st);
    }
};

void check_rescore_rows_args(const int64_t* ids, const float* dist, uint64_t n, uint64_t C, const float* fq, uint64_t k, const RerankOuts& o) {
    if (!ids || !dist || !fq || !o.all()) throw InvalidArg("null argument");
    check_rescore_shape(k, C);
    if (n < 1 || n > 0x7FFFFFFFull) throw InvalidArg("rescore rows: sizes out of range");
}

}  // namespace

extern "C" {

int cph_rescore_vectors_create(cph_index* h, const float* rows, uint64_t size, uint64_t dim_full, int space, int dtype, int metric,
                               cph_rescore_vectors** out) {
    return guarded([&] {
        if (!out) throw InvalidArg("null argument");
        *out = nullptr;
        if (!h || (!rows && size != 0)) throw InvalidArg("null argument");
        if (space != CPH_IDS_INTERNAL && space != CPH_IDS_INPUT) throw InvalidArg("id space must be CPH_IDS_INTERNAL or CPH_IDS_INPUT");
        check_rescore_layout_args(dim_full, dtype, metric);
        std::lock_guard<std::mutex> lk(h->mu);
        if (!h->finalized) throw InvalidArg("rescore vectors belong to a finalized index: finalize or load it first");
        if (size != h->size())
            throw InvalidArg("rescore vectors have " + std::to_string(size) + " rows, the index holds " + std::to_string(h->size()));
        if (size > 0xFFFFFFFEull) throw InvalidArg("rescore vectors: too many rows");
        h->use_device();
        DevBuf<uint32_t> d_inv;
        if (space == CPH_IDS_INPUT) {
            const uint64_t nb = h->host.n;
            if (!h->has_rows) throw InvalidArg("the index has no row map (it was loaded from a v2 file): rows in input order need cph_set_row_map");
            std::vector<uint32_t> map(h->host.rows);
            if (map.size() != nb) {                       // a replica without host arrays: its device copy
                map.resize(nb);
                if (nb) HIP_CHECK(hipMemcpy(map.data(), h->d_rows.p, nb * 4, hipMemcpyDeviceToHost));
            }
            const std::vector<uint32_t> inv = rescore_inverse_rows(map.data(), nb, size);
            d_inv.alloc(std::max<uint64_t>(size, 1));
            if (size) HIP_CHECK(hipMemcpy(d_inv.p, inv.data(), size * 4, hipMemcpyHostToDevice));
        }
        std::unique_ptr<cph_rescore_vectors> rv(new cph_rescore_vectors());
        rv->h = h;
        rv->epoch = h->index_epoch;
        rv->device = h->device;
        rv->size = size;
        rv->dim = (uint32_t)dim_full;
        rv->f32 = dtype == CPH_RESCORE_FLOAT32;
        rv->ip = metric == CPH_RESCORE_IP;
        rv->L = rescore_layout(rv->dim, rv->f32);
        rv->rows.alloc(std::max<uint64_t>(size, 1) * rv->L.stride);
        rv->norms.alloc(std::max<uint64_t>(size, 1));
        const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(size, ((uint64_t)256 << 20) / (dim_full * 4)));
        DevBuf<float> d_x(chunk * dim_full);
        DevBuf<unsigned long long> d_cnt(2);
        const unsigned long long init[2] = {0ull, kRescoreNoRow};
        unsigned long long cnt[2] = {0ull, kRescoreNoRow};
        hipStream_t st = own_stream(h);
        HIP_CHECK(hipMemcpyAsync(d_cnt.p, init, sizeof(init), hipMemcpyHostToDevice, st));
        const RescoreStore s = rescore_store(rv.get());
        for (uint64_t base = 0; base < size; base += chunk) {
            const uint64_t c = std::min(chunk, size - base);
            HIP_CHECK(hipMemcpyAsync(d_x.p, rows + base * dim_full, c * dim_full * 4, hipMemcpyHostToDevice, st));
            rescore_rows_in(d_x.p, c, base, space == CPH_IDS_INPUT ? d_inv.p : nullptr, s, rv->f32, rv->rows.p, rv->norms.p, d_cnt.p, st);
            HIP_CHECK(hipStreamSynchronize(st));          // (the next chunk's upload overwrites d_x from pageable memory)
        }
        HIP_CHECK(hipMemcpyAsync(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        refuse_bad_rescore_rows(cnt[0], cnt[1]);
        *out = rv.release();
    });
}

int cph_rescore_vectors_destroy(cph_rescore_vectors* rv) {
    return guarded([&] {
        if (!rv) return;
        std::unique_ptr<cph_rescore_vectors> own(rv);
        if (hipSetDevice(rv->device) == hipSuccess) (void)hipDeviceSynchronize();       // a batch in flight may read the rows
    });
}

int cph_rescore_vectors_info(const cph_rescore_vectors* rv, uint64_t* size, uint64_t* dim_full, int* dtype, int* metric, uint64_t* row_bytes,
                             uint64_t* nbytes) {
    return guarded([&] {
        if (!rv || !size || !dim_full || !dtype || !metric || !row_bytes || !nbytes) throw InvalidArg("null argument");
        *size = rv->size;
        *dim_full = rv->dim;
        *dtype = rv->f32 ? CPH_RESCORE_FLOAT32 : CPH_RESCORE_FLOAT16;
        *metric = rv->ip ? CPH_RESCORE_IP : CPH_RESCORE_L2;
        *row_bytes = rv->L.stride;
        *nbytes = rv->size * ((uint64_t)rv->L.stride + 4);
    });
}

int cph_rescore_vectors_get(const cph_rescore_vectors* rv, uint64_t first, uint64_t count, void* rows_out, float* norms_out) {
    return guarded([&] {
        if (!rv || (count != 0 && (!rows_out || !norms_out))) throw InvalidArg("null argument");
        if (first > rv->size || count > rv->size - first) throw InvalidArg("rescore vectors: rows out of range");
        if (count == 0) return;
        HIP_CHECK(hipSetDevice(rv->device));
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(rows_out, rv->rows.p + first * rv->L.stride, count * rv->L.stride, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(norms_out, rv->norms.p + first, count * 4, hipMemcpyDeviceToHost));
    });
}

int cph_search_rescored(cph_index* h, const float* queries, uint64_t n, const float* full_queries, uint64_t dim_full, uint64_t k,
                        uint64_t candidates, const cph_rescore_vectors* vectors, const cph_filter* const* filters, uint32_t n_filters,
                        const int32_t* filter_of, int exact, int64_t* ids, float* score, float* first) {
    return guarded([&] {
        const RescoredSearch f{k, candidates, vectors ? &vectors : nullptr, full_queries, dim_full, true};
        rerank_search(h, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(ids, score, first)}, nullptr);
    });
}

int cph_search_rescored_device(cph_index* h, const float* d_queries, uint64_t n, const float* d_full_queries, uint64_t dim_full, uint64_t k,
                               uint64_t candidates, const cph_rescore_vectors* vectors, const cph_filter* const* filters, uint32_t n_filters,
                               const int32_t* filter_of, int exact, int64_t* d_ids, float* d_score, float* d_first, void* stream) {
    return guarded([&] {
        const RescoredSearch f{k, candidates, vectors ? &vectors : nullptr, d_full_queries, dim_full, false};
        rerank_search(h, f, {d_queries, n, filters, n_filters, filter_of, exact != 0, f.outs(d_ids, d_score, d_first)}, nullptr, &stream);
    });
}

int cph_multi_search_rescored(cph_multi* m, const float* queries, uint64_t n, const float* full_queries, uint64_t dim_full, uint64_t k,
                              uint64_t candidates, const cph_rescore_vectors* const* vectors, const cph_filter* const* filters,
                              uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids, float* score, float* first) {
    return guarded([&] {
        if (m && vectors)
            for (size_t r = 0; r < m->reps.size(); ++r)
                if (!vectors[r]) throw InvalidArg("a rescored multi-device search needs one rescore vectors object per replica");
        const RescoredSearch f{k, candidates, vectors, full_queries, dim_full, true};
        rerank_multi(m, f, {queries, n, filters, n_filters, filter_of, exact != 0, f.outs(ids, score, first)}, nullptr,
                     [&](cph_index* h, const RerankCall& s, const cph_group_keys*, uint64_t lo) {
            uint32_t r = 0;
            while (m->reps[r] != h) ++r;
            return cph_search_rescored(h, s.q, s.n, full_queries + lo * dim_full, dim_full, k, candidates, vectors[r], s.filters, s.F,
                                       s.filter_of, s.exact ? 1 : 0, s.out.at<int64_t>(0), s.out.at<float>(1), s.out.at<float>(2));
        });
    });
}

int cph_debug_time_rescored(cph_index* h, int on) {
    return guarded([&] { pass_timer_switch(h, kPassRescored, on != 0); });
}

int cph_debug_last_rescored_us(cph_index* h, double* us) {
    return guarded([&] { pass_timer_us(h, kPassRescored, us); });
}

int cph_rescore_rows_hook(cph_index* h, const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const float* full_queries,
                          const cph_rescore_vectors* vectors, uint64_t k, int64_t* out_ids, float* out_score, float* out_first) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        std::lock_guard<std::mutex> lk(h->mu);
        require_finalized(h);
        check_rescore_vectors(h, vectors);
        const RerankOuts o = RescoredSearch{k, candidates, &vectors, full_queries, vectors->dim, true}.outs(out_ids, out_score, out_first);
        check_rescore_rows_args(ids, dist, n, candidates, full_queries, k, o);
        h->use_device();
        const DevBuf<int64_t> d_ids = uploaded(ids, n * candidates);
        const DevBuf<float> d_dist = uploaded(dist, n * candidates);
        const DevBuf<float> d_fq = uploaded(full_queries, n * vectors->dim);
        PoisonedOuts po(o, n);
        rescore_rows(rescore_args(rescore_store(vectors), vectors->ip, d_ids.p, d_dist.p, d_fq.p, candidates, k,
                                  h->ids_input ? h->d_rows.p : nullptr, po.dev),
                     vectors->f32, (uint32_t)n, nullptr);
        po.download();
    });
}

int cph_host_rescore_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const float* full_queries,
                          uint64_t dim_full, const void* stored, const float* norms, uint64_t n_ids, int dtype, int metric,
                          const uint32_t* rows, uint64_t k, int64_t* out_ids, float* out_score, float* out_first) {
    return guarded([&] {
        if (!stored || !norms) throw InvalidArg("null argument");
        check_rescore_layout_args(dim_full, dtype, metric);
        if (n_ids < 1 || n_ids > 0xFFFFFFFEull) throw InvalidArg("rescore rows: sizes out of range");
        const RescoredSearch f{k, candidates, nullptr, full_queries, dim_full, true};
        check_rescore_rows_args(ids, dist, n, candidates, full_queries, k, f.outs(out_ids, out_score, out_first));
        rescore_rows_host(ids, dist, n, (uint32_t)candidates, full_queries, (uint32_t)dim_full, static_cast<const uint8_t*>(stored), norms,
                          n_ids, dtype == CPH_RESCORE_FLOAT32, metric == CPH_RESCORE_IP, rows, (uint32_t)k, out_ids, out_score, out_first);
    });
}

int cph_host_rescore_rows_in(const float* rows_in, uint64_t n, uint64_t dim_full, int dtype, const uint32_t* row_map, uint64_t n_map,
                             void* stored, float* norms, uint64_t* bad, uint64_t* first_bad) {
    return guarded([&] {
        if (!rows_in || !stored || !norms || !bad || !first_bad) throw InvalidArg("null argument");
        check_rescore_layout_args(dim_full, dtype, CPH_RESCORE_L2);
        if (n < 1 || n > 0xFFFFFFFEull || n_map > n) throw InvalidArg("rescore rows in: sizes out of range");
        std::vector<uint32_t> inv;
        if (row_map) inv = rescore_inverse_rows(row_map, n_map, n);
        unsigned long long fb = kRescoreNoRow;
        *bad = rescore_rows_in_host(rows_in, n, (uint32_t)dim_full, dtype == CPH_RESCORE_FLOAT32, row_map ? inv.data() : nullptr,
                                    static_cast<uint8_t*>(stored), norms, &fb);
        *first_bad = fb;
    });
}

}  // extern "C"


// ---- the metric (cph_set_metric; device_normalize.h) -------------------------------------------------------------------

// Settable on an empty handle only: nothing built, pending or loaded -- the rows of an index are stored for one metric.
// The inner product stores one coordinate more than the caller gives: dim = dim_in + 1, and D follows it.
// cph_set_metric keeps the contract it had before the inner product existed -- it takes L2 and cosine and refuses every
// other value, 2 included -- so CPH_METRIC_IP comes in through its own entry, cph_set_metric_ip (with_ip).
static void set_metric(cph_index* h, int metric, bool with_ip = false) {
    if (metric == CPH_METRIC_IP && !with_ip)
        throw InvalidArg("metric 2 (CPH_METRIC_IP, the inner product) changes the widths of the handle and is set with cph_set_metric_ip / "
                         "cph_multi_set_metric_ip; cph_set_metric takes CPH_METRIC_L2 = 0 and CPH_METRIC_COSINE = 1");
    if (metric != CPH_METRIC_L2 && metric != CPH_METRIC_COSINE && metric != CPH_METRIC_IP)
        throw InvalidArg("unknown metric " + std::to_string(metric) + " (CPH_METRIC_L2 = 0, CPH_METRIC_COSINE = 1)");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->finalized || h->needs_build || h->host.n != 0)
        throw InvalidArg(std::string("the metric is set on an empty handle, before build or load: this one holds ") + metric_name(h->metric) +
                         " rows");
    const uint64_t stored = h->dim_in + (metric == CPH_METRIC_IP ? 1 : 0);
    const size_t pd = next_pow2(stored);
    if (pd > 2048)
        throw InvalidArg("inner-product (ip) metric: the index stores dim + 1 = " + std::to_string(stored) + " coordinates, padded to " +
                         std::to_string(pd) + "; supported padded dims end at 2048 (dim <= 2047)");
    h->metric = (uint32_t)metric;
    h->dim = stored;
    h->D = (uint32_t)pd;
    if (metric != CPH_METRIC_IP) h->ip_bound = 0.0f;
    h->ip_m2 = 0.0f;
}

static void set_ip_bound(cph_index* h, float max_sq_norm) {
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->metric != CPH_METRIC_IP) throw InvalidArg(std::string("the bound belongs to the inner-product (ip) metric: this handle's metric is ") + metric_name(h->metric));
    if (h->finalized || h->needs_build || h->host.n != 0) throw InvalidArg("the inner-product bound is set on an empty handle, before build or load");
    if (!(max_sq_norm >= 0.0f && max_sq_norm < std::numeric_limits<float>::infinity()))
        throw InvalidArg("the inner-product bound is a finite squared norm >= 0 (0: from the rows of the build call)");
    h->ip_bound = max_sq_norm;
}

static void check_ip_args(const float* x, uint64_t n, uint64_t dim, const float* out, int mode, const float* c, float max_sq_norm) {
    if (n && (!x || !out)) throw InvalidArg("null argument");
    if (dim < 1 || dim >= 0xFFFFFFFFull) throw InvalidArg("ip augment: dim out of range");
    if (mode < 0 || mode > 2) throw InvalidArg("ip augment: mode is 0 (rows, given bound), 1 (rows, bound from the data) or 2 (queries)");
    if (mode == 2 && n && !c) throw InvalidArg("null argument");
    if (mode != 1 && !(max_sq_norm >= 0.0f && max_sq_norm < std::numeric_limits<float>::infinity())) throw InvalidArg("ip augment: the bound is a finite squared norm >= 0");
    if (n > 0x7FFFFFFFull / (dim + 1)) throw InvalidArg("ip augment: too many elements for the hook");
}

static void check_normalize_args(const float* x, uint64_t n, uint64_t dim, const float* out) {
    if (n && (!x || !out)) throw InvalidArg("null argument");
    if (dim < 1 || dim > 0xFFFFFFFFull) throw InvalidArg("normalize rows: dim out of range");
}

extern "C" {

int cph_set_metric(cph_index* h, int metric) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_set_metric");
        set_metric(h, metric);
    });
}

int cph_get_metric(cph_index* h, int* metric) {
    return guarded([&] {
        if (!h || !metric) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        *metric = (int)h->metric;
    });
}

int cph_multi_set_metric(cph_multi* m, int metric) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::unique_lock<std::shared_mutex> lk(m->life);
        set_metric(m->reps[0], metric);                      // (replica 0 holds the state that decides; the others follow it)
        for (size_t i = 1; i < m->reps.size(); ++i) set_metric(m->reps[i], metric);      // (the widths follow the metric on every replica)
    });
}

int cph_set_metric_ip(cph_index* h) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_set_metric_ip");
        set_metric(h, CPH_METRIC_IP, true);
    });
}

int cph_multi_set_metric_ip(cph_multi* m) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::unique_lock<std::shared_mutex> lk(m->life);
        for (cph_index* h : m->reps) set_metric(h, CPH_METRIC_IP, true);     // (replica 0 first: it holds the state that decides)
    });
}

int cph_set_ip_bound(cph_index* h, float max_sq_norm) {
    return guarded([&] {
        if (!h) throw InvalidArg("null handle");
        refuse_borrowed(h, "cph_set_ip_bound");
        set_ip_bound(h, max_sq_norm);
    });
}

int cph_get_ip_bound(cph_index* h, float* m2) {
    return guarded([&] {
        if (!h || !m2) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        if (h->metric != CPH_METRIC_IP) throw InvalidArg(std::string("the bound belongs to the inner-product (ip) metric: this handle's metric is ") + metric_name(h->metric));
        *m2 = h->finalized || h->needs_build ? h->ip_m2 : h->ip_bound;
    });
}

int cph_multi_set_ip_bound(cph_multi* m, float max_sq_norm) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::unique_lock<std::shared_mutex> lk(m->life);
        for (cph_index* h : m->reps) set_ip_bound(h, max_sq_norm);
    });
}

int cph_multi_get_ip_bound(cph_multi* m, float* m2) {
    return multi_shared(m, [&] { return cph_get_ip_bound(m->reps[0], m2); });
}

int cph_parts_set_metric(cph_parts* m, int metric) {
    return guarded([&] {
        if (!m) throw InvalidArg("null handle");
        std::unique_lock<std::shared_mutex> lk(m->life);
        for (cph_index* h : m->parts) {                      // every part is asked before any of them changes
            std::lock_guard<std::mutex> g(h->mu);
            if (h->finalized || h->needs_build || h->host.n != 0)
                throw InvalidArg("the metric is set on an empty handle, before build or load");
        }
        // (the parts would each find an M2 of their own, and the merged scores would not compare: a follow-up)
        if (metric == CPH_METRIC_IP) throw InvalidArg("a partitioned index does not take the inner-product (ip) metric: its parts need one global bound");
        for (cph_index* h : m->parts) set_metric(h, metric);
    });
}

int cph_metric_stats(cph_index* h, uint64_t out[2]) {
    return guarded([&] {
        if (!h || !out) throw InvalidArg("null argument");
        std::lock_guard<std::mutex> lk(h->mu);
        out[0] = h->metric_launches;
        out[1] = 0;
        for (const BatchSet& s : h->sets) out[1] += (s.m_queries.n + s.m_c.n) * sizeof(float);
    });
}

int cph_normalize_rows_hook(int device, const float* x, uint64_t n, uint64_t dim, float* out, uint64_t* bad_count, uint64_t* first_bad) {
    return guarded([&] {
        check_normalize_args(x, n, dim, out);
        if (bad_count) *bad_count = 0;
        if (first_bad) *first_bad = kNoBadRow;
        if (n == 0) return;
        if (n > 0xFFFFFFFFull / dim) throw InvalidArg("normalize rows: too many elements for the hook");
        HIP_CHECK(hipSetDevice(device));
        const size_t cells = (size_t)n * dim;
        const bool in_place = out == x;
        DevBuf<float> d_in(cells), d_out(in_place ? 0 : cells);
        DevBuf<unsigned long long> d_bad(2);
        const unsigned long long init[2] = {0ull, kNoBadRow};
        unsigned long long bad[2] = {0ull, kNoBadRow};
        HIP_CHECK(hipMemcpy(d_in.p, x, cells * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_bad.p, init, 16, hipMemcpyHostToDevice));
        // (the outputs start as 0xA5 bytes: every slot the kernel leaves alone shows)
        if (!in_place) HIP_CHECK(hipMemset(d_out.p, 0xA5, cells * 4));
        float* d_o = in_place ? d_in.p : d_out.p;
        normalize_rows(d_in.p, d_o, n, (uint32_t)dim, (uint32_t)dim, (uint32_t)dim, d_bad.p, d_bad.p + 1, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, d_o, cells * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(bad, d_bad.p, 16, hipMemcpyDeviceToHost));
        if (bad_count) *bad_count = bad[0];
        if (first_bad) *first_bad = bad[1];
    });
}

int cph_host_normalize_rows(const float* x, uint64_t n, uint64_t dim, float* out, uint64_t* bad_count, uint64_t* first_bad) {
    return guarded([&] {
        check_normalize_args(x, n, dim, out);
        normalize_rows_host(x, n, (uint32_t)dim, out, bad_count, first_bad);
    });
}

// Test hooks of the inner-product kernels (device_ip.h) on host arrays; cph_host_ip_* are the host statement (host_ip.h).
int cph_ip_augment_hook(int device, const float* x, uint64_t n, uint64_t dim, int mode, float max_sq_norm, float* out, float* c, float* m2,
                        uint64_t counters[3]) {
    return guarded([&] {
        check_ip_args(x, n, dim, out, mode, c, max_sq_norm);
        if (counters) { counters[0] = 0; counters[1] = 0; counters[2] = kIpNoRow; }
        if (m2) *m2 = mode == 1 ? 0.0f : max_sq_norm;
        if (n == 0) return;
        HIP_CHECK(hipSetDevice(device));
        const size_t cells = (size_t)n * dim, ocells = (size_t)n * (dim + 1);
        DevBuf<float> d_in(cells), d_out(ocells), d_c(n);
        DevBuf<unsigned long long> d_cnt(3);
        DevBuf<unsigned int> d_m2(1);
        const unsigned long long init[3] = {0ull, 0ull, kIpNoRow};
        unsigned long long cnt[3] = {0ull, 0ull, kIpNoRow};
        HIP_CHECK(hipMemcpy(d_in.p, x, cells * 4, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_cnt.p, init, sizeof(init), hipMemcpyHostToDevice));
        // (the outputs start as 0xA5 bytes: every slot the kernel leaves alone shows)
        HIP_CHECK(hipMemset(d_out.p, 0xA5, ocells * 4));
        HIP_CHECK(hipMemset(d_c.p, 0xA5, n * 4));
        float bound = max_sq_norm;
        if (mode == 1) {
            HIP_CHECK(hipMemset(d_m2.p, 0, 4));
            ip_max(d_in.p, n, (uint32_t)dim, 0, d_m2.p, nullptr, nullptr);       // (the second pass counts the bad rows)
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(&bound, d_m2.p, 4, hipMemcpyDeviceToHost));
        }
        ip_augment(d_in.p, d_out.p, n, (uint32_t)dim, bound, 0, mode == 2 ? d_c.p : nullptr, d_cnt.p, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(out, d_out.p, ocells * 4, hipMemcpyDeviceToHost));
        if (c) HIP_CHECK(hipMemcpy(c, d_c.p, n * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(cnt, d_cnt.p, sizeof(cnt), hipMemcpyDeviceToHost));
        if (m2) *m2 = bound;
        if (counters) { counters[0] = cnt[0]; counters[1] = cnt[1]; counters[2] = cnt[2]; }
    });
}

static void check_ip_epilogue_args(const int64_t* ids, const float* dist, uint64_t n, uint64_t k, const float* c) {
    if (n && k && (!ids || !dist || !c)) throw InvalidArg("null argument");
    if (k > 0xFFFFFFFFull || (k && n > 0x7FFFFFFFull / k)) throw InvalidArg("ip epilogue: table too large for the hook");
}

// pinned != 0: the tables live in pinned, device-mapped host memory (what the small-batch route hands the kernel).
int cph_ip_epilogue_hook(int device, const int64_t* ids, float* dist, uint64_t n, uint64_t k, const float* c, int pinned) {
    return guarded([&] {
        check_ip_epilogue_args(ids, dist, n, k, c);
        if (n == 0 || k == 0) return;
        HIP_CHECK(hipSetDevice(device));
        const size_t cells = (size_t)n * k;
        DevBuf<float> d_c(n);
        HIP_CHECK(hipMemcpy(d_c.p, c, n * 4, hipMemcpyHostToDevice));
        if (pinned) {
            uint8_t* pin = nullptr;
            uint8_t* pin_dev = nullptr;
            size_t bytes = 0;
            grow_pinned(pin, pin_dev, bytes, cells * 12);
            std::memcpy(pin, ids, cells * 8);
            std::memcpy(pin + cells * 8, dist, cells * 4);
            hipError_t e = hipSuccess;
            try {
                ip_epilogue(reinterpret_cast<const int64_t*>(pin_dev), reinterpret_cast<float*>(pin_dev + cells * 8), n, (uint32_t)k, d_c.p, nullptr);
                e = hipDeviceSynchronize();
            } catch (...) {
                (void)hipHostFree(pin);
                throw;
            }
            if (e == hipSuccess) std::memcpy(dist, pin + cells * 8, cells * 4);
            (void)hipHostFree(pin);
            HIP_CHECK(e);
            return;
        }
        DevBuf<int64_t> d_ids(cells);
        DevBuf<float> d_dist(cells);
        HIP_CHECK(hipMemcpy(d_ids.p, ids, cells * 8, hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(d_dist.p, dist, cells * 4, hipMemcpyHostToDevice));
        ip_epilogue(d_ids.p, d_dist.p, n, (uint32_t)k, d_c.p, nullptr);
        HIP_CHECK(hipDeviceSynchronize());
        HIP_CHECK(hipMemcpy(dist, d_dist.p, cells * 4, hipMemcpyDeviceToHost));
    });
}

int cph_host_ip_augment(const float* x, uint64_t n, uint64_t dim, int mode, float max_sq_norm, float* out, float* c, float* m2, uint64_t counters[3]) {
    return guarded([&] {
        check_ip_args(x, n, dim, out, mode, c, max_sq_norm);
        if (counters) { counters[0] = 0; counters[1] = 0; counters[2] = kIpNoRow; }
        const float bound = mode == 1 ? ip_max_sq_norm_host(x, n, (uint32_t)dim, nullptr) : max_sq_norm;
        ip_augment_host(x, n, (uint32_t)dim, bound, out, mode == 2 ? c : nullptr, counters);
        if (m2) *m2 = bound;
    });
}

int cph_host_ip_epilogue(const int64_t* ids, float* dist, uint64_t n, uint64_t k, const float* c) {
    return guarded([&] {
        check_ip_epilogue_args(ids, dist, n, k, c);
        ip_epilogue_host(ids, dist, n, k, c);
    });
}

}  // extern "C"
