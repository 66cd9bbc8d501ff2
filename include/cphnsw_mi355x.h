/* cphnsw_mi355x.h — C-ABI of the MI355X-native CP-HNSW layer-0 hot path.
 *
 * One shared library (libcphnsw_mi355x.so, built by hipcc for gfx950) replaces, for the
 * query-time path only, what the reference binds through pybind11 in
 * src/bindings.cpp:115-240 (class `cphnsw._core.CPIndex`):
 *
 *   reference interface (file:line)                      this header
 *   ---------------------------------------------------  ------------------------------
 *   CPIndex(dim, bits)          src/bindings.cpp:77-123   cph_create
 *   ~CPIndex                                             cph_destroy
 *   .load(path)                 src/bindings.cpp:227-232  cph_load   (v2 file, api/hnsw_index.hpp:305-443)
 *   .save(path)                 src/bindings.cpp:220-225  cph_save   (api/hnsw_index.hpp:217-303)
 *   .search(query,k)            src/bindings.cpp:146-175  cph_search
 *   .search_batch(queries,k)    src/bindings.cpp:177-218  cph_search_batch / cph_search_batch_device
 *   .size/.dim/.is_finalized    src/bindings.cpp:234-239  cph_size / cph_dim / cph_is_finalized
 *   .build/.finalize            src/bindings.cpp:125-144  cph_build / cph_finalize
 *
 * Kernel-level hooks (parity tests and the roofline benchmark; they expose the units the
 * reference implements in distance/fastscan_kernel.hpp, core/memory.hpp and
 * encoder/rabitq_encoder.hpp):
 *   cph_encode_query, cph_entry_point, cph_fastscan_block, cph_exact_l2, cph_fastscan_stream_*.
 *
 * Conventions: plain pointers and sizes only; every function returns a cph_status; on
 * failure cph_last_error() (thread-local) holds the message the reference would have
 * thrown.  CPH_INVALID_ARGUMENT maps to Python ValueError (std::invalid_argument),
 * CPH_RUNTIME_ERROR to RuntimeError (std::runtime_error), CPH_OUT_OF_MEMORY to MemoryError.
 * The caller owns all buffers; the library owns the handle.  A handle is bound to one HIP
 * device (cph_multi_*: one index replicated on several devices, one call).  Threads: every entry point may be called from any thread.  Concurrent cph_search callers on one handle
 * are COALESCED into shared launches (the reference answers them in parallel under a shared lock,
 * src/bindings.cpp:146-175, api/hnsw_index.hpp:172): a caller that finds a free leader slot takes everybody queued
 * so far with the same k into one launch; each waits for its own query only and gets its own rows.  The other entry points serialise on the handle
 * (cph_search_batch_device only while it enqueues).  Knobs: CPH_LEADER_SLOTS (default 3), CPH_GATHER_US (80).
 * Ids: by default searches return, and filters speak of, the reference's internal (post-BFS-reorder) node ids.  An index
 * built here keeps the builder's row map (internal id -> row of the array given to cph_build); with it a handle can
 * return input rows instead (cph_set_result_ids) and take filters in input rows (cph_filter_create_rows).  The map is
 * saved by cph_save_native; cph_save writes the reference's v2 format, which cannot carry it and silently drops it:
 * an index loaded from a v2 file has no map until cph_set_row_map supplies one.  cph_get_vectors and the kernel-level
 * hooks (cph_entry_point, cph_fastscan_block, cph_exact_l2, cph_export_blocks) always use internal ids.
 */
#ifndef CPHNSW_MI355X_H
#define CPHNSW_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cph_index cph_index;

typedef enum {
    CPH_OK = 0,
    CPH_INVALID_ARGUMENT = 1,
    CPH_RUNTIME_ERROR = 2,
    CPH_OUT_OF_MEMORY = 3,
    CPH_NOT_IMPLEMENTED = 4
} cph_status;

/* Thread-local message of the last failing call on this thread. */
const char* cph_last_error(void);

/* Library/ABI version (major*100 + minor). */
int cph_version(void);

/* ---- lifecycle ------------------------------------------------------------------- */
/* dim > 0, next_pow2(dim) in {16..2048}, bits in {1,2,4}; device = HIP device ordinal. */
int cph_create(uint64_t dim, uint64_t bits, int device, cph_index** out);
int cph_destroy(cph_index* h);

int cph_load(cph_index* h, const char* path);
int cph_save(cph_index* h, const char* path);
/* GPU-native index file (csrc/native_file.h): the device block layout, vectors and norms as the GPU reads
 * them, so loading is an mmap plus two host-to-device copies instead of the v2 file's per-vertex
 * re-layout.  A handle loaded this way can still write a v2 file (cph_save) for the reference. */
int cph_save_native(cph_index* h, const char* path);
int cph_load_native(cph_index* h, const char* path);
int cph_size(cph_index* h, uint64_t* n);
int cph_dim(cph_index* h, uint64_t* dim);
int cph_is_finalized(cph_index* h, int* flag);

/* Index construction (api/hnsw_index.hpp:93-166).  build() copies the
 * n x dim float32 vectors; finalize() builds the index on the GPU (exact 32-NN on the matrix cores,
 * reverse edges + neighbour selection, per-edge RaBitQ codes written straight into the search layout,
 * upper layers, calibration sampling; csrc/builder.h).  The edge encoder is bit-exact with the
 * reference's; the graph has statistical parity (the reference's own build depends on its thread count). */
int cph_build(cph_index* h, const float* vectors, uint64_t n);
int cph_finalize(cph_index* h);
/* Construction / ground-truth hook: exact 32 nearest neighbours (squared L2, ascending) by brute
 * force on the matrix cores (v_mfma_f32_32x32x2_f32: exact f32).  queries == NULL: of every row of
 * vectors[n][dim] against the other rows (self excluded) -- the working lists the reference obtains
 * from NNDescent (graph/graph_refinement.hpp:455-515; distances core/memory.hpp:65-79), ids/dist
 * [n][32].  queries != NULL: of queries[nq][dim] against vectors[n][dim], ids/dist [nq][32].  Rows
 * with fewer than 32 candidates are padded with 0xFFFFFFFF / FLT_MAX. */
int cph_knn_bruteforce(int device, const float* vectors, uint64_t n, uint64_t dim, const float* queries,
                       uint64_t nq, uint32_t* ids, float* dist);
/* Test entries of the exact-kNN kernels (tests only, like grid_cap above).  cph_debug_knn runs the kernels behind
 * cph_knn_bruteforce with the choices the production path makes from the size laid open; cph_host_knn is their host
 * statement (csrc/host_knn.h, no HIP call, callable without a GPU), whose ids and distances the kernels equal byte for byte.
 *   queries == NULL: the self-join of vectors[n][dim] (a row never lists itself; nq = 0, q_ids = NULL, exclude_self ignored);
 *   queries != NULL: queries[nq][dim] against vectors; exclude_self = 0: nothing is excluded and q_ids is NULL;
 *   exclude_self = 1: row i never lists column q_ids[i] (q_ids[nq], every entry < n) -- the form the join's fallback uses.
 *   path: 0 = the two-pass kernel (knn_mfma_kernel); 1 = the symmetric join (device_knn_sym.h), refused unless this is a
 *   self-join with 1024 <= n <= 4096 and a padded D >= 64.  dim <= 2048.
 *   blocks_per_launch: 0 = the production slicing, else the number of 128-row blocks per launch of the two-pass kernel and
 *   the number of workgroups per launch of the join.
 * ids/dist [rows][32] as cph_knn_bruteforce writes them; *fallback_rows = rows the join answered through its fallback
 * (0 on path 0); *launches = launches made of the kernel that path names; cand_count[n] (cph_host_knn on path 1, may be NULL) = the
 * join's candidates per row.  The pointers to single values may be NULL. */
int cph_debug_knn(int device, const float* vectors, uint64_t n, uint64_t dim, const float* queries, uint64_t nq,
                  const uint32_t* q_ids, int exclude_self, int path, uint32_t blocks_per_launch, uint32_t* ids, float* dist,
                  uint32_t* fallback_rows, uint32_t* launches);
int cph_host_knn(const float* vectors, uint64_t n, uint64_t dim, const float* queries, uint64_t nq, const uint32_t* q_ids,
                 int exclude_self, int path, uint32_t* ids, float* dist, uint32_t* fallback_rows, uint32_t* cand_count);

/* Construction hook: the data-side encoder of one vertex' edges on the GPU (the kernel finalize() runs
 * for every vertex; encoder/rabitq_encoder.hpp:138-181, 287-323, 371-467): parent and cnt <= 32
 * neighbours (dim floats each) -> values u8[cnt][D] (code value per dimension), aux f32[cnt][3] =
 * {nop, ip_qo, ip_cp}, pops u32[cnt][2] = {msb popcount, weighted popcount}. */
int cph_encode_edges(int device, uint64_t dim, uint64_t bits, const float* parent, const float* nbrs, uint64_t cnt,
                     uint8_t* values, float* aux, uint32_t* pops);

/* Construction hook: the neighbour-selection kernel on ONE vertex with a given candidate list -- the rule of
 * graph/neighbor_selection.hpp:21-88 (select_neighbors_alpha_cng), deterministic on a fixed list.  x = [n][D] padded
 * vectors, fwd = 32 forward candidates (0xFFFFFFFF = none), rev = up to 65,536 further candidates (the reverse edges),
 * err = per-vertex margin terms or null.  out_ids = 32 selected ids (0xFFFFFFFF padded), *out_cnt = how many.
 * Up to 96 reverse edges all candidates are considered; beyond that the vertex is a hub and the kernel keeps the
 * nearest 64 unique candidates (ties by id) of fwd and rev together, whatever the order of rev. */
int cph_select_hook(int device, const float* x, uint64_t n, uint64_t D, uint32_t vertex, const uint32_t* fwd,
                    const uint32_t* rev, uint64_t n_rev, uint32_t R, float alpha, float tau, float alpha_max,
                    const float* err, uint32_t* out_ids, uint32_t* out_cnt);

/* Construction hook: layer-0 selection of a WHOLE table as finalize() launches it -- the reverse CSR built from
 * knn[n][32] (0xFFFFFFFF = none; every other id < n), then the selection kernel over all n rows on the production
 * grid (grid_cap = 0) or on at most grid_cap workgroups, so that one workgroup walks many rows.  out_ids[n][32]
 * (0xFFFFFFFF padded), out_cnt[n]; rev_off[n + 1] / rev[n * 32] (either may be null) receive the reverse CSR the
 * kernel read: rev_off[n] entries of rev are written, each segment in the order the fill's atomics produced. */
int cph_select_layer_hook(int device, const float* x, uint64_t n, uint64_t D, const uint32_t* knn, uint32_t R, float alpha,
                          float tau, float alpha_max, const float* err, uint32_t grid_cap, uint32_t* out_ids,
                          uint32_t* out_cnt, uint64_t* rev_off, uint32_t* rev);

/* Construction hook: the calibration sampler (api/hnsw_index.hpp:770-1040 gathers the same quantities) on given sample
 * queries [ns][dim] and start vertices: per sample one greedy hop, then per edge of the vertex arrived at
 * rec[ns][32][6] = {nop, ip_est_raw - ip_cp, max(|ip_qo|, 1e-10), <q - p, o - p> / nop, |q - o|^2, ip_qo};
 * rec_cnt[ns] = valid edges, dqp[ns] = exact |q - p|^2. */
int cph_calib_hook(cph_index* h, const float* queries, const uint32_t* start, uint64_t ns, float* rec, uint32_t* rec_cnt,
                   float* dqp);

/* Self-test hook for the beam's heap routines (wave-parallel std::push_heap / std::pop_heap with the first 255
 * entries in LDS and the rest in HBM, search/rabitq_search.hpp:53-58, :79-80): runs `ops` (1 = push the next
 * (key, id), 0 = pop) on one wave and returns the heap array; the test compares it with libstdc++'s on the same
 * sequence.  out_keys / out_ids hold n_push entries. */
int cph_debug_heap_ops(int device, const uint8_t* ops, uint64_t n_ops, const float* keys, const uint32_t* ids, uint64_t n_push,
                       float* out_keys, uint32_t* out_ids, uint32_t* out_size);

/* Self-test hook for the N-bit estimator of the search kernels' expansion (csrc/device_estimator_test.h): for the
 * neighbour blocks of vertices [first, first + count) of a finalized 2- or 4-bit index, every set s of forced aux values
 * (force[n_sets][3] = nop, ip_qo, ip_cp, put into every lane of the block where bit 0 / 1 / 2 of fmask[s] is set; the
 * block's own value otherwise) and every squared distance dqp[j], out[block][s][j][6][32] holds the bits of the stage-1
 * bound, the stage-2 bound and the estimate as the expansion evaluates them (lower_bounds_split + stage2_est_only inside
 * 1e-12 <= dqp < +inf), then the same three from stage1_lower + stage2_est, which cph_fastscan_block runs.  lut and
 * qparams as for cph_fastscan_block.  count <= 1024, n_dqp <= 64, n_sets <= 64. */
int cph_debug_estimator(cph_index* h, const uint8_t* lut, const float* qparams, uint32_t first, uint32_t count, const float* dqp,
                        uint32_t n_dqp, const float* force, const uint32_t* fmask, uint32_t n_sets, uint32_t* out);

/* ---- search ---------------------------------------------------------------------- */
/* queries: host, row-major [n][dim] float32.  ids/dist: host, [n][k], rows shorter than k
 * padded with -1 / FLT_MAX (src/bindings.cpp:202-210). */
int cph_search_batch(cph_index* h, const float* queries, uint64_t n, uint64_t k,
                     int64_t* ids, float* dist);

/* Same, but queries/ids/dist are DEVICE pointers on the handle's device and the work is
 * enqueued on `stream` (a hipStream_t; NULL = default stream).  Nothing is copied to the host and
 * the call returns after enqueueing, always: a query that outgrows its scratch capacity is
 * answered exactly by a full-capacity re-run launch enqueued behind the main one.  The results are
 * complete when `stream` reaches the point behind this call.  A handle keeps two sets of batch
 * scratch and uses them alternately, so two batches enqueued on two different streams run
 * concurrently (the second fills the GPU while the first drains its longest queries); a third
 * call waits, on its stream, for the batch that used its set before.  d_queries must stay valid
 * until the batch has run. */
int cph_search_batch_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k,
                            int64_t* d_ids, float* d_dist, void* stream);
/* Blocks the calling host thread until every batch enqueued on this handle has finished. */
int cph_synchronize(cph_index* h);

/* ---- filtered search ------------------------------------------------------------- */
/* An allowed-id bitmap, uploaded once to the handle's device: bit (id & 31) of words[id >> 5] set = id may be
 * returned.  Ids are the internal (post-reorder) ids the searches return.  n_bits must equal the size of the index
 * the filter is used with (checked at every search); bits behind n_bits are ignored.  The filter records its
 * popcount: a search with no id allowed returns padding without launching anything. */
typedef struct cph_filter cph_filter;
int cph_filter_create(cph_index* h, const uint32_t* words, uint64_t n_bits, cph_filter** out);
/* Waits for the filter's device (batches enqueued with cph_search_batch_device_filtered may still read the
 * bitmap), then frees it.  NULL is a no-op. */
int cph_filter_destroy(cph_filter* f);
/* cph_search_batch / cph_search_batch_device restricted to the allowed ids: the reference search in which only
 * allowed ids may enter the result heap (its nn.push at the popped vertex, the warm-up and the reranked neighbours,
 * gated); every other step is unchanged -- vertices outside the set are still estimated, reranked, pushed into the
 * beam and expanded, and the warm-up, the lower-bound pruning, DABS and the gamma termination follow the result
 * heap of allowed ids.  Rows with fewer than k allowed ids reached are padded with -1 / FLT_MAX.  f = NULL is the
 * unfiltered call; a filter made for an index of another size or on another device fails with
 * CPH_INVALID_ARGUMENT.  These batches never take the probe-first instantiation; cph_last_search_stats and
 * cph_last_query_expansions report them as any other batch. */
int cph_search_batch_filtered(cph_index* h, const float* queries, uint64_t n, uint64_t k, const cph_filter* f,
                              int64_t* ids, float* dist);
int cph_search_batch_device_filtered(cph_index* h, const float* d_queries, uint64_t n, uint64_t k,
                                     const cph_filter* f, int64_t* d_ids, float* d_dist, void* stream);

/* ---- exact search ---------------------------------------------------------------------- */
/* Brute force over the allowed ids (f = NULL: over every id) on the fp32 VALU, instead of the graph search: each row
 * holds the k nearest allowed ids, exactly.  A distance has the bits cph_exact_l2 returns for the pair -- the bits the
 * graph search returns for the same id.  Rows are in ascending distance, equal distance bits in ascending INTERNAL id
 * (also under CPH_IDS_INPUT, where the ids are translated as the rows are written); an id appears at most once; rows with
 * fewer than k allowed ids are padded with -1 / FLT_MAX.  k <= 1024 (CPH_INVALID_ARGUMENT above).  The filter checks are
 * those of the filtered calls; an empty filter returns padding without a launch.  The _device form only enqueues, takes a
 * batch set in rotation like cph_search_batch_device, and its filter must outlive it as there (cph_filter_destroy waits).
 * The filter's ascending id list is made on the device at its first exact use and kept until the filter is destroyed.
 * Afterwards cph_last_search_stats reports [0] = 0, [1] = n x candidates, [6] = device time, every other word 0;
 * cph_last_query_expansions returns zeros. */
int cph_search_batch_exact(cph_index* h, const float* queries, uint64_t n, uint64_t k, const cph_filter* f,
                           int64_t* ids, float* dist);
int cph_search_batch_exact_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k, const cph_filter* f,
                                  int64_t* d_ids, float* d_dist, void* stream);
/* Cut-over of the filtered entry points (cph_search_batch_filtered, cph_search_batch_device_filtered and, through them,
 * the multi form): a filter that allows at most max_allowed ids (and a k <= 1024) takes the exact path.  Default 0: never,
 * every call does what it did before. */
int cph_set_exact_threshold(cph_index* h, uint64_t max_allowed);

/* ---- range search ----------------------------------------------------------------------- */
/* Every allowed id closer than a radius, in CSR form: lims[n + 1] (lims[0] = 0), query i owns ids / dist
 * [lims[i], lims[i + 1]).  An id is a hit iff dist < radius[i], compared as float32 against the squared-L2 values the
 * searches return (strict: FAISS's rule for L2; distances are >= +0, so a radius <= 0 or NaN selects nothing and +inf
 * every candidate).  Two steps, because the caller allocates the output:
 *
 * cph_range_search_begin   queries: [n][dim] in host memory, or (queries_on_device != 0) on the handle's device, then
 *     `stream` is the caller's stream (the host form runs on the handle's own stream and ignores it).  radius_host[n] is
 *     host memory in both forms.  exact != 0: the candidates are the filter's ids (NULL: every id) minus the removed rows,
 *     as in cph_search_batch_exact, scanned with its arithmetic: every hit is returned (no cap), each segment ascends by
 *     (distance bits, INTERNAL id), no id twice, distances are the bytes of the exact search.  exact == 0: the graph route,
 *     needs max_results = K >= 1: segment i = the entries of row i of cph_search_batch_filtered(queries, K, filter) with
 *     id >= 0 and dist < radius[i], in row order, the same bytes; that call, with all its routing, is enqueued into scratch
 *     rows.  Runs the count pass (the search) and the offsets scan, WAITS for the sizes and returns *total = lims[n] and
 *     the object.  The object owns its scratch (no batch set) and holds the effective filter: a cph_remove between the
 *     two steps does not change the answer; a load, build or compact does (finish then fails with CPH_RUNTIME_ERROR).
 *     n == 0 and a filter that allows nothing give *total = 0 without a scan launch.
 * cph_range_search_finish  lims_host[n + 1]: host memory; ids[total], dist[total]: host memory, or device memory
 *     (results_on_device != 0).  The queries are cut into consecutive tiles whose keys (twice when a segment is longer
 *     than one LDS sort) fit the exact scratch budget (CPH_EXACT_SCRATCH_MB; a single query may exceed it); per tile the
 *     fill pass, the segmented sort and the emit run on the stream of begin.  Under CPH_IDS_INPUT ids are translated as
 *     they are written; the order stays the internal-id order.  WAITS for its kernels (and copies) before it returns.
 *     Once per object.  With *total == 0 ids and dist may be NULL.
 * cph_range_destroy        frees the object (NULL: no-op); nothing of it is in flight after begin / finish returned.
 *     Its device buffers go back to the handle, which keeps those of two finished calls for the next ones (an index
 *     swap frees them): in steady state a call makes no hipMalloc and no hipFree of its own.  The handle must outlive
 *     the object (destroy it first); on a handle without removed rows the caller's filter must outlive finish.
 *     Both steps hold the handle mutex, host waits included: other calls on the same handle queue behind them.
 *
 * cph_last_search_stats after an exact range search: [1] = 2 x n x candidates (two passes), every other word 0; after
 * the graph route: those of the underlying search. */
typedef struct cph_range cph_range;
int cph_range_search_begin(cph_index* h, const void* queries, int queries_on_device, uint64_t n, const float* radius_host,
                           const cph_filter* filter, int exact, uint64_t max_results, void* stream, cph_range** out,
                           uint64_t* total);
int cph_range_search_finish(cph_range* r, int64_t* lims_host, void* ids, void* dist, int results_on_device);
int cph_range_destroy(cph_range* r);
/* Host statements of the range search (no HIP call).  cph_host_range_plan: out[5] = parts, candidates per part (a
 * multiple of 64), queries per group, keys of one LDS sort, rows of the padded query array (a fill launch starts at a
 * tile's first query and reads whole tiles of 8 rows: every row it can touch lies below this count).  cph_host_range_tiles: the tiles finish cuts n queries with
 * these lims into under budget_bytes: starts_out[*n_tiles_out + 1] (room for n + 1), tile t = queries [starts[t],
 * starts[t + 1]).  cph_host_range_merge_pass: one merge pass of width `width` over a segment of `len` unique keys that
 * is sorted in runs of `width`: out = the segment sorted in runs of 2 x width. */
int cph_host_range_plan(uint64_t candidates, uint64_t n_queries, int num_cus, uint64_t* out);
int cph_host_range_tiles(const int64_t* lims, uint64_t n, uint64_t budget_bytes, uint64_t* starts_out, uint64_t* n_tiles_out);
int cph_host_range_merge_pass(const uint64_t* in, uint64_t* out, uint64_t len, uint64_t width);

/* ---- grouped search --------------------------------------------------------------------- */
/* The k best key groups of every query, up to group_size rows of each (group-by / collapse): rows that share a key -- the
 * chunks of a document, the products of a seller -- answer as one group.  key_of[id] is an int32 per INTERNAL id: the
 * handle's label column (cph_set_labels), or a cph_group_keys object when the labels mean something else.
 *
 * A query's candidate row is what the ordinary search returns for it at k = candidates (C): C entries ascending by
 * (distance, id), padded with -1 / FLT_MAX -- cph_search_batch_filtered / _exact / _filters with the same filters, exact
 * flag, exact threshold, removed rows and tail, with all their routing and all their refusals (per-query filters that
 * would walk the graph of an index with a tail are CPH_NOT_IMPLEMENTED here too).  The row is walked front to back:
 *   - padding is skipped;
 *   - an id that occurred earlier in the row is skipped (a graph row can hold an id twice, a grouped answer cannot);
 *   - an entry whose key has no group opens one at the next group index while fewer than k groups exist;
 *   - an entry whose key has a group with fewer than group_size members is appended to it;
 *   - every other entry is dropped.
 * So groups are ordered by their best member, members ascend, ties keep the order of the underlying search.  Keys are
 * compared as values over the whole int32 range: INT32_MIN, INT32_MAX, 0 and -1 are ordinary keys, none is a sentinel.
 *
 * Outputs per query (g = group_size): ids [k][g] int64, padded with -1 (internal ids; under CPH_IDS_INPUT input rows,
 * translated where a member is written); dist [k][g] float32, padded with FLT_MAX, else the bytes of the candidate row;
 * group_keys [k] int32 and counts [k] int32 (members per group), both 0 where there is no group; complete uint8 =
 * (k groups exist and each has g members) or (the row holds fewer than C entries that are not padding: the underlying
 * search ran dry and a longer row would add nothing).  complete is a function of the row alone; with exact != 0 and
 * complete == 1 the answer is the exact grouped top-k over the allowed ids.  complete == 0 at C = 1024 means that the
 * 1,024 nearest candidates did not fill the groups (a few keys own most near rows): the groups returned are still the
 * best of those candidates.
 *
 * Limits: 1 <= k, 1 <= group_size, k * group_size <= candidates <= 1024 (the longest row of the exact route and of a
 * tail's graph route).  filters / n_filters / filter_of: filter_of == NULL takes n_filters 0 (unfiltered) or 1 (one filter
 * for the batch); else per-query filters as in cph_search_batch_filters.  CPH_INVALID_ARGUMENT: NULL pointers, a shape
 * outside the limits, no label column and no keys object, a keys object of another size, device or index.
 *
 * The work: under the handle mutex the search runs at k = C into scratch rows the handle owns (four sets in rotation,
 * only ever grown: a call in steady state makes no hipMalloc and no hipFree), written in internal ids whatever the
 * handle's result id space is (nothing of the handle is changed once the call returns); then ONE launch of
 * group_rows_kernel (csrc/device_group.h) on the same stream writes all five outputs, padding included.
 * cph_search_grouped takes and returns host arrays; cph_search_grouped_device takes device pointers and a stream and
 * waits for nothing (filters and the keys object must outlive the batch; their destroy calls wait).
 * cph_last_search_stats afterwards: those of the underlying search.
 *
 * cph_group_keys_create  keys[size]: one int32 per row, size == cph_size (else CPH_INVALID_ARGUMENT), in internal ids or in
 *     input rows (space = CPH_IDS_INPUT: needs a row map; moved to internal order once, on the host).  The object is
 *     resident on the handle's device and serves that handle only.  It covers `size` ids: after a cph_add it is refused
 *     with the size message a filter gets; a load, build or compact invalidates it (refused as made for another index).
 * cph_group_keys_destroy waits for the device, then frees; NULL is a no-op.
 * Partitioned indexes have no grouped search: every part has its own internal ids and its own slice of the labels. */
typedef struct cph_group_keys cph_group_keys;
int cph_group_keys_create(cph_index* h, const int32_t* keys, uint64_t size, int space, cph_group_keys** out);
int cph_group_keys_destroy(cph_group_keys* keys);
int cph_search_grouped(cph_index* h, const float* queries, uint64_t n, uint64_t k, uint64_t group_size, uint64_t candidates,
                       const cph_group_keys* keys, const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                       int exact, int64_t* ids, float* dist, int32_t* group_keys, int32_t* counts, uint8_t* complete);
int cph_search_grouped_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k, uint64_t group_size, uint64_t candidates,
                              const cph_group_keys* keys, const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                              int exact, int64_t* d_ids, float* d_dist, int32_t* d_group_keys, int32_t* d_counts, uint8_t* d_complete,
                              void* stream);
/* Debug hooks of the measurement script (scripts/grouped_sweep.py), not for production use: while switched on, the
 * group_rows_kernel launch of every grouped search of this handle is bracketed by two HIP events on the call's stream;
 * _us waits for the second event and returns the device time of the last such launch in microseconds, or
 * CPH_INVALID_ARGUMENT when none ran.  Off by default: the call then records no event of this kind. */
int cph_debug_time_grouped(cph_index* h, int on);
int cph_debug_last_group_rows_us(cph_index* h, double* us);
/* Test hook: group_rows_kernel on given rows (host arrays).  ids / dist [n][candidates]; key_of [n_keys]; rows [n_keys] or
 * NULL; every id >= 0 must be < n_keys (CPH_INVALID_ARGUMENT).  The device outputs start as 0xA5 bytes, so a slot the
 * kernel left alone shows.  cph_host_group_rows is the host statement (csrc/host_group.h, no HIP call). */
int cph_group_rows_hook(int device, const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const int32_t* key_of,
                        uint64_t n_keys, const uint32_t* rows, uint64_t k, uint64_t group_size, int64_t* out_ids, float* out_dist,
                        int32_t* out_keys, int32_t* out_counts, uint8_t* out_complete);
int cph_host_group_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const int32_t* key_of, uint64_t n_keys,
                        const uint32_t* rows, uint64_t k, uint64_t group_size, int64_t* out_ids, float* out_dist, int32_t* out_keys,
                        int32_t* out_counts, uint8_t* out_complete);

/* ---- diversified search ------------------------------------------------------------------ */
/* k results per query that are close to the query AND not copies of each other: maximal marginal relevance (MMR) over a
 * candidate row, on the device.  A query's candidate row is what the ordinary search returns for it at k = candidates
 * (C), exactly as for grouped search above: same filters, exact flag, exact threshold, removed rows, tail, routing and
 * refusals.  The statement (csrc/host_diverse.h is its host form, tests/diverse_model.py its numpy form):
 *   - walk the row front to back, skip padding and ids that occurred earlier in the row; the survivors are the
 *     candidates, each with its position j in the row and its relevance r_j = dist[j] (bits kept);
 *   - a = lam, b = 1.0f - a (float32, rounded once);
 *   - d(s, j) has the bits cph_exact_l2 returns for query = the stored row of internal id s and id = j: eight FMA chains
 *     over the zero-padded rows reduced ((c0+c4)+(c1+c5))+((c2+c6)+(c3+c7)), qnorm = the same chains over s * s, norm =
 *     the stored norm of j.  It is not symmetric in its bits; the order of the arguments is as written;
 *   - pick 0 is the first candidate; for pick t >= 1 every unpicked candidate has m_j = min over picked s of d(s, j) and
 *     score_j = (a * r_j) - (b * m_j), three separately rounded float32 operations; the smallest score is picked, equal
 *     scores (+0 == -0) go to the lower row position; k picks, or until the candidates run out.
 * Outputs per query, in pick order (NOT ascending): ids [k] int64, padded with -1 (internal ids; under CPH_IDS_INPUT input
 * rows, translated where a pick is written); dist [k] = r of the pick; gap [k] = m of the pick when it was taken, FLT_MAX
 * for pick 0; dist and gap are padded with FLT_MAX.  lam = 1 gives the first k non-repeated entries of the row, lam = 0 a
 * farthest-point walk over the candidates.
 *
 * Limits: 1 <= k <= candidates <= 1024, 0 <= lam <= 1 (NaN is refused).  CPH_INVALID_ARGUMENT: NULL pointers, a shape or
 * lam outside the limits, every refusal of the underlying search; nothing is written then.
 *
 * The work: as for grouped search -- under the handle mutex the search runs at k = C into the same scratch rows (four
 * sets in rotation, only ever grown; no hipMalloc and no hipFree in steady state), in internal ids; then ONE launch of
 * diverse_rows_kernel (csrc/device_diverse.h) on the same stream reads the handle's resident vectors and norms and writes
 * all three outputs, padding included.  cph_search_diverse takes and returns host arrays; cph_search_diverse_device takes
 * device pointers and a stream and waits for nothing.  cph_last_search_stats afterwards: those of the underlying search
 * ONLY; the kernel's pair distances are not counted as exact distances.
 * Partitioned indexes have no diverse search: every part has its own internal ids. */
int cph_search_diverse(cph_index* h, const float* queries, uint64_t n, uint64_t k, float lam, uint64_t candidates,
                       const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids, float* dist,
                       float* gap);
int cph_search_diverse_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k, float lam, uint64_t candidates,
                              const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* d_ids,
                              float* d_dist, float* d_gap, void* stream);
/* Debug hooks of the measurement script (scripts/diverse_sweep.py), as cph_debug_time_grouped / _last_group_rows_us: the
 * diverse_rows_kernel launch of every diverse search of this handle between two HIP events while switched on. */
int cph_debug_time_diverse(cph_index* h, int on);
int cph_debug_last_diverse_rows_us(cph_index* h, double* us);
/* Test hook: diverse_rows_kernel on given rows (host arrays ids / dist [n][candidates], internal ids; an id at or above
 * cph_size counts as padding) against the vectors and norms of the handle; ids are written through the row map under
 * CPH_IDS_INPUT.  The device outputs start as 0xA5 bytes, so a slot the kernel left alone shows.
 * cph_host_diverse_rows is the host statement (csrc/host_diverse.h, no HIP call) over raw [n_ids][D] (zero-padded rows, D a
 * multiple of 8) and norm_sq [n_ids]; rows [n_ids] or NULL. */
int cph_diverse_rows_hook(cph_index* h, const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, uint64_t k, float lam,
                          int64_t* out_ids, float* out_dist, float* out_gap);
int cph_host_diverse_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const float* raw, const float* norm_sq,
                          uint64_t n_ids, uint64_t D, const uint32_t* rows, uint64_t k, float lam, int64_t* out_ids, float* out_dist,
                          float* out_gap);

/* ---- multi-vector search (late interaction, MaxSim) ---------------------------------------- */
/* A query is `tokens` (T) vectors, of which the first n_tokens[i] (L, 1 <= L <= T; n_tokens == NULL: all T) are live:
 * the token embeddings of a ColBERT- or ColPali-style retriever.  The answer is the k keys (documents; key_of as for
 * grouped search: the label column, or a cph_group_keys object) that minimise the sum, over the live tokens, of the
 * token's best row of the key.  Under CPH_METRIC_COSINE a distance is 1 - cos, so the MaxSim similarity of a returned key
 * is n_tokens - score.
 *
 * queries is [n][T][dim]: the n * T token rows are ONE ordinary batch, searched at k = candidates (C) exactly as the rows
 * of a grouped search are -- same filters, exact flag, exact threshold, removed rows, tail, metric, routing and refusals;
 * filter_of[i] serves all T tokens of query i (the entry expands it).  The tokens t >= L are searched with the batch and
 * then ignored entirely.  The statement over the T candidate rows of one query (csrc/host_maxsim.h is its host form,
 * tests/maxsim_model.py its numpy form); an entry is valid when 0 <= id < cph_size, and everything but the sum and the
 * final order is defined by position, so that no float comparison is ambiguous:
 *   - floor_t = the distance of the last valid entry of row t, +0.0f when the row has none;
 *   - for a key that occurs in a valid entry of a live row, pos_t(key) = the lowest position of row t whose entry has the
 *     key, if any; term_t(key) = the distance there, else floor_t; hits(key) = the live t that have a pos_t(key);
 *   - score(key): s = +0.0f; for t = 0 .. L-1: s = s + term_t(key) -- float32, in that order;
 *   - the min(k, distinct keys) keys with the smallest (score as a float value, key as a signed int32), in that order.
 * Outputs per query: out_keys [k] int32, out_score [k] float32, out_hits [k] int32, out_rows [k][T] int64 = the id at
 * pos_t(key) (internal ids; under CPH_IDS_INPUT input rows, translated where it is written), -1 where token t has no row
 * of the key or t >= L; out_found int32 = the keys returned.  Padding: key 0, score FLT_MAX, hits 0, rows -1.  Every int32
 * value is an ordinary key.
 *
 * What the score means: floor_t is the C-th distance of token t, and a row of the key that the search did not return for
 * t is no closer than that.  With exact != 0, score(key) is therefore a LOWER BOUND of the true
 * sum_t min_{row of key, allowed} dist(q_t, row) (in float32 too: float addition is monotone), and EQUAL to it where
 * hits == L: hits is this call's counterpart of `complete` in cph_search_grouped.  With exact != 0 and C at least the
 * number of allowed rows the answer is the exact MaxSim top-k.  Nothing is re-run at a larger C, and missing (key, token)
 * pairs are not re-scored against the stored vectors.
 *
 * Limits: 1 <= T <= 64, 1 <= C <= 1024, T * C <= 8192, 1 <= k <= 1024, n * T <= 2^31 - 1, 1 <= n_tokens[i] <= T (host
 * array in both forms); anything else is CPH_INVALID_ARGUMENT with a message that names the limit, as are NULL pointers,
 * no label column and no keys object, a keys object of another size, device or index.
 *
 * The work: as for grouped search -- under the handle mutex the search runs at k = C into the same scratch rows (n * T of
 * them; four sets in rotation, only ever grown), in internal ids; then ONE launch of maxsim_rows_kernel
 * (csrc/device_maxsim.h), one workgroup per query, on the same stream writes all five outputs, padding included.
 * cph_search_maxsim takes and returns host arrays; cph_search_maxsim_device takes device pointers (queries and outputs)
 * and a stream and waits for no kernel (n_tokens travels through a pinned buffer of the scratch set: the one host wait is
 * for the COPY of the lengths that set carried four calls earlier).  An index that never calls these entries launches and
 * allocates what it did before.  cph_last_search_stats afterwards: those of the underlying search.
 * Partitioned indexes have no maxsim search: every part has its own internal ids and its own slice of the labels. */
int cph_search_maxsim(cph_index* h, const float* queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                      uint64_t candidates, const cph_group_keys* keys, const cph_filter* const* filters, uint32_t n_filters,
                      const int32_t* filter_of, int exact, int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows,
                      int32_t* out_found);
int cph_search_maxsim_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                             uint64_t candidates, const cph_group_keys* keys, const cph_filter* const* filters, uint32_t n_filters,
                             const int32_t* filter_of, int exact, int32_t* d_keys, float* d_score, int32_t* d_hits, int64_t* d_rows,
                             int32_t* d_found, void* stream);
/* Debug hooks of the measurement script (scripts/maxsim_sweep.py), as cph_debug_time_grouped / _last_group_rows_us: the
 * maxsim_rows_kernel launch of every maxsim search of this handle (with the copy of n_tokens, when one is given) between
 * two HIP events while switched on. */
int cph_debug_time_maxsim(cph_index* h, int on);
int cph_debug_last_maxsim_rows_us(cph_index* h, double* us);
/* Test hook: maxsim_rows_kernel on given rows (host arrays).  ids / dist [n][tokens][candidates]; n_tokens [n] or NULL;
 * key_of [n_keys]; rows [n_keys] or NULL; an id outside [0, n_keys) counts as padding.  The device outputs start as 0xA5
 * bytes, so a slot the kernel left alone shows.  cph_host_maxsim_rows is the host statement (csrc/host_maxsim.h, no HIP
 * call). */
int cph_maxsim_rows_hook(int device, const int64_t* ids, const float* dist, uint64_t n, uint64_t tokens, const int32_t* n_tokens,
                         uint64_t candidates, const int32_t* key_of, uint64_t n_keys, const uint32_t* rows, uint64_t k, int32_t* out_keys,
                         float* out_score, int32_t* out_hits, int64_t* out_rows, int32_t* out_found);
int cph_host_maxsim_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t candidates,
                         const int32_t* key_of, uint64_t n_keys, const uint32_t* rows, uint64_t k, int32_t* out_keys, float* out_score,
                         int32_t* out_hits, int64_t* out_rows, int32_t* out_found);

/* ---- multi-vector search with exact rescoring (not in the reference) ---------------------- */
/* cph_search_maxsim followed by the second stage of a late-interaction retriever: the best `rescore` = R keys of the
 * lower-bound statement (k <= R <= 1024; the other limits are those of cph_search_maxsim) are scored against ALL their
 * allowed rows, and the k best of those are returned.  csrc/host_maxsim_rescore.h is the host form of the statement,
 * tests/maxsim_rescore_model.py its numpy form:
 *   candidates  the cph_search_maxsim statement at k = R over the same token rows, C, filters, exact flag, routing, removed
 *               rows and tail: f = found <= R keys with their lower bounds lb_j, in (lb, key) order; they stay in scratch;
 *   A_i(key)    the ids < cph_size with that key whose bit is set in query i's effective filter (the caller's filter for
 *               that query AND not removed, tail rows included; every id when there is neither);
 *   best_t      per candidate and live token t: min over id in A_i(key) of (bits(d(q_t, id)), id) as an unsigned pair; d has
 *               the bytes cph_exact_l2 returns for the pair, the token vector being the one the search saw (cosine: after
 *               the normalise kernel); d >= +0, so equal distances go to the lowest internal id;
 *   score       ((+0.0f + d_0) + d_1) + ... over t < n_tokens[i], float32, in that order;
 *   answer      the min(k, f) candidates with the smallest (score, key), in that order: keys, score, hits (= n_tokens[i] in
 *               every real slot), rows[t] = the argmin id (input rows under CPH_IDS_INPUT; -1 for t >= n_tokens[i]), found;
 *               padding as in cph_search_maxsim;
 *   certified   [n] int32: the number of leading answer slots whose score is strictly below lb_{R-1}, or found[i] when
 *               f < R.  Every key outside the candidates has a lower bound >= lb_{R-1}, so with exact != 0 those leading
 *               slots are the true MaxSim top slots over the allowed rows, in the true order.  With a graph-routed search
 *               the bound is relative to the candidate rows the search returned, not to the whole index.
 * The work, on the call's stream: maxsim_rows_kernel at k = R into scratch, exact_pad_kernel over the token rows, then
 * maxsim_rescore_scan_kernel (one wave per (query, candidate)) and maxsim_rescore_select_kernel (one workgroup per query),
 * csrc/device_maxsim_rescore.h.  The scan walks an INVERTED KEY COLUMN (ids by (key, id), distinct keys, offsets), built on
 * the host -- a download of the column, a sort, an upload -- once per column and cached where the column lives: in the
 * cph_group_keys object, or on the handle for the label column, where cph_set_labels, cph_add, cph_compact, a load and a
 * build drop it.  Building it WAITS for the device: the one exception to "the _device form only enqueues";
 * cph_prepare_maxsim_rescore(h, keys) (keys == NULL: the label column) builds it ahead of time.  A handle that never
 * rescored allocates nothing for it.  The inner-product metric and partitioned indexes are refused as for cph_search_maxsim. */
int cph_search_maxsim_rescored(cph_index* h, const float* queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                               uint64_t candidates, uint64_t rescore, const cph_group_keys* keys, const cph_filter* const* filters,
                               uint32_t n_filters, const int32_t* filter_of, int exact, int32_t* out_keys, float* out_score,
                               int32_t* out_hits, int64_t* out_rows, int32_t* out_found, int32_t* out_certified);
int cph_search_maxsim_rescored_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                                      uint64_t candidates, uint64_t rescore, const cph_group_keys* keys, const cph_filter* const* filters,
                                      uint32_t n_filters, const int32_t* filter_of, int exact, int32_t* d_keys, float* d_score,
                                      int32_t* d_hits, int64_t* d_rows, int32_t* d_found, int32_t* d_certified, void* stream);
int cph_prepare_maxsim_rescore(cph_index* h, const cph_group_keys* keys);
/* Debug hooks of the measurement script (scripts/maxsim_rescore_sweep.py): the launch of maxsim_rescore_scan_kernel alone
 * between two HIP events while switched on. */
int cph_debug_time_maxsim_rescore(cph_index* h, int on);
int cph_debug_last_maxsim_rescore_us(cph_index* h, double* us);
/* Test hook: the pad, scan and select kernels on given candidates (host arrays) against the vectors of h.  cand_keys /
 * cand_lb [n][rescore], cand_found [n] in [0, rescore]; tokens [n][n_tok][dim]; n_tokens [n] or NULL; keys: a keys object of
 * h or NULL (the label column); allow: [n][(cph_size + 31) / 32] bitmap words, one bitmap per query, or NULL (every id).
 * The device outputs start as 0xA5 bytes.  cph_host_maxsim_rescore is the host statement (no HIP call) over raw
 * [n_ids][D] zero-padded rows and their norms; cph_host_key_rows the host routine that inverts a key column: out_ids [n],
 * out_keys [n] (the first *out_n_keys are written), out_offsets [n + 1] (the first *out_n_keys + 1). */
int cph_maxsim_rescore_hook(cph_index* h, const int32_t* cand_keys, const float* cand_lb, const int32_t* cand_found, uint64_t n,
                            uint64_t rescore, const float* tokens, uint64_t n_tok, const int32_t* n_tokens, const cph_group_keys* keys,
                            const uint32_t* allow, uint64_t k, int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows,
                            int32_t* out_found, int32_t* out_certified);
int cph_host_maxsim_rescore(const int32_t* cand_keys, const float* cand_lb, const int32_t* cand_found, uint64_t n, uint64_t rescore,
                            const float* tokens, uint64_t n_tok, uint64_t dim, const int32_t* n_tokens, const float* raw,
                            const float* norm_sq, uint64_t n_ids, uint64_t D, const int32_t* key_of, const uint32_t* allow,
                            const uint32_t* rows, uint64_t k, int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows,
                            int32_t* out_found, int32_t* out_certified);
int cph_host_key_rows(const int32_t* keys, uint64_t n, uint32_t* out_ids, int32_t* out_keys, uint32_t* out_offsets, uint64_t* out_n_keys);

/* ---- fused search: several query vectors per query, exact weighted-sum top-k (ABI 115) ----- */
/* queries is [n][vectors][dim]: T = vectors query vectors per query (rewrites of one question, liked and disliked examples, an
 * image and a text vector) of which the first L = n_vectors[i] are live (1 <= L <= T; NULL: all T), with weights [n][T],
 * float32, finite, any sign (NULL: every weight 1).  One ranked list of ROWS per query comes back.  csrc/host_fused.h is the
 * host form of the statement, tests/fused_model.py its numpy form:
 *   candidates  the n * T vectors run as ONE ordinary search at k = C = candidates -- same routing, filters, exact flag,
 *               per-query filters (filter_of[i] serves all T vectors of query i), removed and added rows, cosine
 *               normalisation.  The candidates of query i are the DISTINCT ids that occur in the rows of its live vectors;
 *               hits(x) = the live vectors whose row holds x.  The distances of that search are used for nothing else;
 *   score       d_t(x) has the bytes cph_exact_l2 returns for vector t as the search saw it and id x, for EVERY live t;
 *               s = +0.0f; for t = 0 .. L-1: s = fadd(s, fmul(w[i][t], d_t(x))), each rounded once, no contraction.  A
 *               candidate whose s is a NaN (overflow under weights of both signs) is dropped;
 *   answer      the k best by (s, internal id) ascending: ids [n][k] int64 (input rows under CPH_IDS_INPUT), score [n][k],
 *               hits [n][k] int32; unused slots are -1 / FLT_MAX / 0.  Every slot is written by the pass.
 * Limits (those of cph_search_maxsim): 1 <= T <= 64, 1 <= C <= 1024, T * C <= 8192, 1 <= k <= min(1024, T * C),
 * n * T <= 2^31 - 1 (and n * ceil(T * C / 64) <= 2^31 - 1, the scan's grid).  With T = 1 and weight 1 the answer is the first
 * k distinct ids of cph_search_batch at k = C wherever that search's distance bytes are cph_exact_l2's.
 * The work, on the call's stream behind the search: exact_pad_kernel over the vectors, fused_union_kernel (one workgroup per
 * query: sort and collapse the candidate rows), fused_scan_kernel (one wave per (query, 64 candidates): the exact sums) and
 * fused_select_kernel (one workgroup per query), csrc/device_fused.h.  n_vectors and weights are host memory in both forms;
 * the _device form only enqueues: they travel through a pinned buffer of the scratch set, and the call waits on the host only
 * for the copy that set carried the last time.  The inner-product metric is refused; a partitioned index has no such entry
 * (use the parts).  Every refusal happens before an output is written.  A handle that never calls it allocates nothing. */
int cph_search_fused(cph_index* h, const float* queries, uint64_t n, uint64_t vectors, const int32_t* n_vectors, const float* weights,
                     uint64_t k, uint64_t candidates, const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                     int exact, int64_t* ids, float* score, int32_t* hits);
int cph_search_fused_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t vectors, const int32_t* n_vectors,
                            const float* weights, uint64_t k, uint64_t candidates, const cph_filter* const* filters, uint32_t n_filters,
                            const int32_t* filter_of, int exact, int64_t* d_ids, float* d_score, int32_t* d_hits, void* stream);
/* Debug hooks of the measurement script (scripts/fused_sweep.py): the launch of fused_scan_kernel alone between two HIP events
 * while switched on. */
int cph_debug_time_fused(cph_index* h, int on);
int cph_debug_last_fused_us(cph_index* h, double* us);
/* Test hook: the pad, union, scan and select kernels on given candidate rows (host arrays, cand_ids [n * vectors][candidates],
 * internal ids, -1 padding) and queries [n][vectors][dim] against the vectors of h; ids go through the row map under
 * CPH_IDS_INPUT.  The device outputs start as 0xA5 bytes.  cph_host_fused_rows is the host statement (no HIP call) over
 * queries_padded [n][vectors][D] (the vectors as the search saw them, zero-padded), raw [n_ids][D] zero-padded rows, their norms
 * and an optional row map. */
int cph_fused_rows_hook(cph_index* h, const int64_t* cand_ids, const float* queries, uint64_t n, uint64_t vectors, const int32_t* n_vectors,
                        const float* weights, uint64_t candidates, uint64_t k, int64_t* out_ids, float* out_score, int32_t* out_hits);
int cph_host_fused_rows(const int64_t* cand_ids, uint64_t n, uint64_t vectors, const int32_t* n_vectors, const float* weights,
                        uint64_t candidates, const float* queries_padded, const float* raw, const float* norm_sq, uint64_t n_ids, uint64_t D,
                        const uint32_t* rows, uint64_t k, int64_t* out_ids, float* out_score, int32_t* out_hits);

/* ---- per-query filters ------------------------------------------------------------------ */
/* One batch, a different allowed set per query: query i is searched under filters[filter_of[i]], or unfiltered where
 * filter_of[i] == -1 (any other value outside [0, n_filters) is CPH_INVALID_ARGUMENT; every filter is checked like the
 * one of cph_search_batch_filtered).  Row i holds the bytes the single-filter call returns for that query and that
 * filter.  Routing is per query, by the rules of the single-filter entries: an empty filter gives a padded row; exact != 0
 * sends every query to the exact scan (k <= 1024; -1 scans the whole index); otherwise a filter at or below the exact
 * threshold (and a k <= 1024) is scanned, every other filter and -1 take the graph search.  All scanned queries of the
 * call share one pad, one scan and one merge launch (per scratch budget), all graph-searched filtered queries one launch
 * pair, the unfiltered ones another.  Statistics: the counters are the sums of what the separate single-filter calls
 * report, cph_last_query_expansions is 0 for scanned and padded rows, kernel_us covers the whole call.
 * filter_of is host memory in both forms (the routing needs every filter's size on the host).  The _device form only
 * enqueues: the call's tables travel through a pinned buffer of the batch set; the filters must outlive the batch.  It
 * waits for no kernel, but before it rewrites that buffer it waits on the host until the copy of the tables the same
 * batch set carried the last time (as many batches back as there are sets) has read it. */
int cph_search_batch_filters(cph_index* h, const float* queries, uint64_t n, uint64_t k, const cph_filter* const* filters,
                             uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids, float* dist);
int cph_search_batch_filters_device(cph_index* h, const float* d_queries, uint64_t n, uint64_t k,
                                    const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact,
                                    int64_t* d_ids, float* d_dist, void* stream);

/* The same bitmap contract as cph_filter_create, but bit r speaks of INPUT ROW r (the handle needs a row map, else
 * CPH_INVALID_ARGUMENT; n_bits must equal the size of the index).  The device converts it once, through the row map,
 * into an ordinary cph_filter (an internal-id bitmap), usable with every filtered entry point and with any result id
 * space.  A later cph_set_row_map does not change filters made before it. */
int cph_filter_create_rows(cph_index* h, const uint32_t* words, uint64_t n_bits, cph_filter** out);

/* ---- ids in input rows ------------------------------------------------------------ */
/* The row map: rows[i] = 0-based row, in the array given to cph_build, of internal id i; a permutation of 0..n-1.
 * cph_finalize keeps it (host copy and device copy, 4 B per vertex), cph_save_native / cph_load_native carry it (native
 * file format 2: format 1 plus a `rows` section, laid out so that a library that knows format 1 only still loads and
 * searches the file; an index without a map is written as format 1), cph_load (v2 file) leaves the handle without one. */
int cph_has_row_map(cph_index* h, int* flag);
int cph_get_row_map(cph_index* h, uint64_t first, uint64_t count, uint32_t* out);
/* For an index that came from a v2 file and whose owner has the map from elsewhere: n must equal the size of the index
 * and rows must be a permutation of 0..n-1 (CPH_INVALID_ARGUMENT otherwise).  rows == NULL removes the map (and puts the
 * handle back to CPH_IDS_INTERNAL).  Waits for everything enqueued on the handle. */
int cph_set_row_map(cph_index* h, const uint32_t* rows, uint64_t n);
/* The id space of the results of EVERY search entry point of this handle (a property of the handle, read when a search
 * is enqueued; waits for everything enqueued before, like cph_set_batch_sets).  CPH_IDS_INPUT: ids leave the GPU as input
 * rows (padding stays -1); distances, counts and statistics are those of CPH_IDS_INTERNAL.  CPH_IDS_INPUT on a handle
 * without a row map fails with CPH_INVALID_ARGUMENT; losing the map (cph_load of a v2 file, cph_set_row_map(NULL),
 * cph_build) puts the handle back to CPH_IDS_INTERNAL. */
enum { CPH_IDS_INTERNAL = 0, CPH_IDS_INPUT = 1 };
int cph_set_result_ids(cph_index* h, int space);

/* ---- removed rows: tombstones and compact() --------------------------------------------- */
/* A finalized handle carries a set R of removed INTERNAL ids, empty by default.  A removed row is a tombstone: it stays
 * in the graph and is still walked, but can never enter a result.  With R not empty EVERY search entry point returns the
 * bytes (ids, distances, padding) the same call returns on the same index with R empty under the filter F & ~R, F being
 * the caller's filter, or every id: cph_search_batch[_device] and their _filtered, _exact and _filters forms, the exact
 * threshold (compared with the count of F & ~R), an empty F & ~R (padded rows, no launch), filter_of == -1 (~R); the
 * counters of cph_last_search_stats other than kernel_us, and cph_last_query_expansions, are those of that filtered
 * call.  cph_search on such a handle runs as a batch of one through the filtered path (not coalesced).  The search
 * kernels are not involved: the price of the first removed row is that unfiltered batches leave the probe-first
 * instantiation.  With R empty nothing changes: launches, results, statistics and the bytes of
 * cph_save_native are those of a handle that never heard of cph_remove.  cph_size is unchanged by a remove (ids keep
 * their meaning, a filter's n_bits is still the size); cph_live_count = size - |R|.
 *
 * cph_remove   ids[m]: host array, internal ids (space = CPH_IDS_INTERNAL) or input rows (CPH_IDS_INPUT; needs a row
 *              map).  An id outside [0, size) is CPH_INVALID_ARGUMENT and changes nothing; duplicates and ids removed
 *              before are fine.  *newly (may be NULL) = ids newly removed.  Waits for everything enqueued on the handle
 *              (like cph_set_row_map), then updates the resident bitmap with the kernels of csrc/device_tombstone.h.
 * filters      a cph_filter made before a remove observes it at its next use: it caches F & ~R with its count and its
 *              exact-scan id list per state of R (the first use after a remove computes it on the handle's own stream
 *              and waits for the count), so one filter may serve two handles of one size with different R.  A cached
 *              bitmap is freed only after the device has drained: a filter keeps four, and the first use under a fifth
 *              state of R waits for the whole device, also in the _device entry points that otherwise only enqueue.
 * R ends       with cph_build, cph_load (v2) and cph_compact; cph_load_native takes the file's R; cph_set_row_map and
 *              cph_set_result_ids do not touch it.
 * files        cph_save_native writes R, when it is not empty, as native format 3 (format 1 or 2 plus a `removed`
 *              section, csrc/native_file.h), which a library that knows formats 1 and 2 only REFUSES instead of loading
 *              the file with the rows back.  cph_save (the reference's v2 format, which cannot carry R) fails with
 *              CPH_RUNTIME_ERROR on a handle with removed rows: compact first, or save natively.
 * cph_get_removed  words[(size + 31) / 32]: R as a bitmap over internal ids.
 * cph_compact  rebuilds the index from the live rows with the builder of cph_build + cph_finalize: the live vectors in
 *              input-row order (internal-id order without a row map).  old_to_new[old size]: the new input row of every
 *              old id, in the handle's result id space (cph_set_result_ids), -1 for removed ids.  Afterwards size ==
 *              live_count, R is empty, the handle has a fresh row map and keeps CPH_IDS_INPUT if it had it.  With R
 *              empty it still rebuilds.  Fewer live rows than the builder takes is the builder's own error and leaves
 *              the handle as it was. */
int cph_remove(cph_index* h, const int64_t* ids, uint64_t m, int space, uint64_t* newly);
int cph_live_count(cph_index* h, uint64_t* n);
int cph_get_removed(cph_index* h, uint32_t* words);
int cph_compact(cph_index* h, int64_t* old_to_new);

/* ---- added rows: the tail ---------------------------------------------------------------- */
/* A finalized handle holds n_b BASE rows, the rows of its graph, and behind them t >= 0 TAIL rows (cph_add): a flat
 * segment of fp32 rows that no graph, block or code knows of.  size = n_b + t; tail row j has id n_b + j in internal ids
 * AND in input rows (it is its own input row: the row map is extended by the identity).  With t == 0 nothing changes:
 * launches, results, statistics and the bytes of cph_save_native are those of a handle that never heard of cph_add.
 *
 * cph_add      vectors[m][dim]: host array; labels[m]: required iff the handle has a label column, else NULL.
 *              *first_id (may be NULL) = id of the first new row = size before the call; the rows get consecutive ids.
 *              Holds the handle mutex, waits for everything enqueued on the handle (like cph_remove), uploads the rows
 *              and runs one device pass (csrc/device_tail.h: tail_append_kernel) that zero-pads each row, writes its
 *              norm with the builder's arithmetic (the same floats get the norm bits cph_build gives them), extends the
 *              row map, the label column and the removed bitmap (clear bits).  The resident arrays grow amortised (half
 *              as much again, a device-to-device copy).  With removed rows present the handle takes a new state of R:
 *              filters cached F & ~R again at their next use.  m == 0 is a no-op.  CPH_INVALID_ARGUMENT: not finalized,
 *              NULL vectors, labels given without a column or missing with one, size + m >= 2^32 - 1, a borrowed
 *              replica or part handle (like cph_set_row_map).  cph_multi_* and cph_parts_* have no add.
 * cph_tail_count  *t; cph_size returns n_b + t.
 * ids          every call that names ids ranges over size: cph_remove, cph_get_removed, cph_live_count, cph_get_row_map,
 *              cph_get_labels, cph_set_labels, cph_get_vectors, cph_exact_l2, cph_filters_from_labels.  A filter's n_bits
 *              must equal the size, so a filter made before an add is refused afterwards; bit n_b + j speaks of tail row
 *              j in cph_filter_create and in cph_filter_create_rows.  cph_fastscan_block and cph_export_blocks name
 *              vertices of the graph: ids < n_b only.
 * exact routes cph_search_batch_exact*, the exact threshold (compared with the allowed count over ALL ids), the exact
 *              cph_range_search_* and the scanned queries of cph_search_batch_filters*: the tail rows are more
 *              candidates, nothing else changes; the order is (distance bits, internal id), tail ids are the largest.
 * graph route  cph_search_batch[_device][_filtered], cph_search and the exact == 0 range search through them: row i is
 *              the first k entries of the stable merge of G_i then T_i.  G_i: the row the same call returns on the same
 *              handle before any add, under the effective filter restricted to the base rows (bytes, duplicates and
 *              padding included; already in input rows under CPH_IDS_INPUT).  T_i: the exact top-k of the allowed tail
 *              rows, ascending by (distance bits, id), distances with the bits of cph_exact_l2.  Entries are compared as
 *              float values, the graph entry first where they are equal, padding last -- numpy:
 *              argsort(concatenate([G_i, T_i]), kind="stable")[:k].  The graph launch is the one a handle without a tail
 *              makes (same instantiation, probe first included; same counters; same cph_last_query_expansions);
 *              cph_last_search_stats [1] grows by n x t (the scan evaluates every tail row and masks by the filter) and
 *              [6] covers all launches.  Tail rows are found exactly: recall does not fall as the tail grows, time does.
 *              A filter that allows nothing launches nothing, tail included.  cph_search runs as a batch of one (not
 *              coalesced), as on a handle with removed rows.  The _device forms still only enqueue.
 * refused      while t > 0, each message naming cph_compact: cph_save and cph_save_native (CPH_RUNTIME_ERROR: no file
 *              format carries a tail), cph_set_row_map (CPH_INVALID_ARGUMENT), graph-routed calls with k > 1024
 *              (CPH_INVALID_ARGUMENT: the scan's limit), cph_search_batch_filters[_device] when a query would take the
 *              graph route (CPH_NOT_IMPLEMENTED; fine when every query is scanned or padded).
 * the tail ends  with cph_build, cph_load, cph_load_native and cph_compact.  cph_compact rebuilds from the live rows, the
 *              tail included: base rows in input-row order, then tail rows in id order; old_to_new[old size]; labels
 *              carried over; afterwards t == 0. */
int cph_add(cph_index* h, const float* vectors, uint64_t m, const int32_t* labels, int64_t* first_id);
int cph_tail_count(cph_index* h, uint64_t* t);
/* Test hook: tail_fold_kernel on given rows (host arrays).  g_ids / g_dist [n][k]: graph rows, ascending in distance,
 * padding (-1 / FLT_MAX) last; pools[P][n][C]: keys (distance bits << 32 | id), each list ascending; counts[P][n], each
 * <= k: the lists as the tail scan leaves them.  C: a power of two, 128 <= C, 2 k <= C; k <= 1024; P <= 256.  The rows are
 * uploaded and folded in place, as the library does, then copied to out_ids / out_dist [n][k].  cph_host_tail_fold is
 * the host statement (no HIP call); cph_host_tail_capacity: *out = rows the resident arrays hold room for once `need`
 * rows no longer fit into `capacity` (csrc/host_tail.h). */
int cph_tail_fold_hook(int device, const int64_t* g_ids, const float* g_dist, uint64_t n, uint64_t k, const uint64_t* pools,
                       const uint32_t* counts, uint32_t P, uint32_t C, int64_t* out_ids, float* out_dist);
int cph_host_tail_fold(const int64_t* g_ids, const float* g_dist, uint64_t n, uint64_t k, const uint64_t* pools,
                       const uint32_t* counts, uint32_t P, uint32_t C, int64_t* out_ids, float* out_dist);
int cph_host_tail_capacity(uint64_t capacity, uint64_t need, uint64_t* out);

/* ---- label column and label filters ------------------------------------------------------- */
/* A finalized handle may carry one int32 label per row (a tenant, a category, a day), resident on its device in
 * internal-id order (4 B per vertex, next to the row map), so that "rows whose label is t" becomes a filter without a
 * host-built bitmap: cph_filters_from_labels makes many filters in one device pass (csrc/device_labels.h).
 *
 * cph_set_labels   labels[n]: one int32 per row, n == size (else CPH_INVALID_ARGUMENT), in internal ids
 *                  (CPH_IDS_INTERNAL) or input rows (CPH_IDS_INPUT; needs a row map, else CPH_INVALID_ARGUMENT; moved to
 *                  internal order once, on the host).  NULL (n ignored) removes the column.  A handle that is not
 *                  finalized is CPH_INVALID_ARGUMENT; a borrowed replica or part handle is refused like cph_set_row_map.
 *                  Holds the handle mutex; filters made before keep their bits.
 * lifetime         the column ends with cph_build, cph_load and cph_load_native (no file carries it: cph_save_native
 *                  writes the bytes it writes without one; the caller keeps the array and sets it again after a load);
 *                  it survives cph_remove, cph_set_row_map and cph_set_result_ids; cph_compact carries it over: new input
 *                  row j has the label of the live row it came from.
 * cph_get_labels   labels of internal ids [first, first + count), like cph_get_row_map. */
int cph_set_labels(cph_index* h, const int32_t* labels, uint64_t n, int space);
int cph_has_labels(cph_index* h, int* flag);
int cph_get_labels(cph_index* h, uint64_t first, uint64_t count, int32_t* out);
/* m filters at once: filter j allows the ids whose label x satisfies lo[j] <= x <= hi[j] (signed, both ends inclusive;
 * lo[j] > hi[j]: the empty filter).  out[m] receives ordinary cph_filter objects (bitmap on the handle's device, bits
 * behind size clear, popcount counted on the device), usable with every filtered entry point and destroyed one by one
 * with cph_filter_destroy; their bitmaps share one device allocation, which goes with the last of them.  The call waits
 * once, for the m counts.  All or nothing: on failure nothing is left allocated and out[] is all NULL.  m == 0 is a
 * no-op.  Needs a label column (CPH_INVALID_ARGUMENT without; also for m above 65,535 x 64).  Allowed on a borrowed replica or part handle. */
int cph_filters_from_labels(cph_index* h, const int32_t* lo, const int32_t* hi, uint32_t m, cph_filter** out);
/* Debug hooks of the measurement script (scripts/label_filter_sweep.py), not for production use: while switched on,
 * every cph_filters_from_labels pass of this handle is bracketed by two HIP events on the handle's (private) stream;
 * _us returns the device time of the last such pass (the memset of the counts and the kernel) in microseconds, or
 * CPH_INVALID_ARGUMENT when none ran.  Off by default: the call then records no event. */
int cph_debug_time_label_filters(cph_index* h, int on);
int cph_debug_last_label_filters_us(cph_index* h, double* us);
/* The bitmap and count of any cph_filter, back on the host: words[(n_bits + 31) / 32].  Either of words and count
 * may be NULL (the count alone makes no device call). */
int cph_filter_export(const cph_filter* f, uint32_t* words, uint64_t* count);
/* Host statement of cph_filters_from_labels (no HIP call): words_out[m][(n + 31) / 32], counts_out[m]. */
int cph_host_label_filters(const int32_t* labels, uint64_t n, const int32_t* lo, const int32_t* hi, uint32_t m,
                           uint32_t* words_out, uint64_t* counts_out);

/* ---- filter algebra: AND / OR / ANDNOT / XOR / NOT of filters, on the device ------------------- */
/* out[j] = a[j] OP b[j] for m filters in one device pass (csrc/device_filter_ops.h): the bitmap holds exactly the bits of
 * the word-wise operation with the bits at or above n_bits clear, and popcount is counted on the device, as
 * cph_filter_create counts a host bitmap.  b: n_b = m filters, or n_b = 1 filter that every j is combined with
 * (broadcast: m tenant bitmaps AND one common mask), or b NULL and n_b = 0 for CPH_FILTER_NOT (~a[j]).  ANDNOT is
 * a & ~b.  Removed rows are not special: NOT sets their bits, and every search still runs under "filter AND not
 * removed" like under any other filter.
 *
 * No handle: a filter knows its device and n_bits, and its bitmap is complete when the call that made it returns.  The
 * call runs on a stream of its own on the filters' device, copies the m counts back and waits once.  out[m] receives
 * ordinary, immutable cph_filter objects (usable with every filtered entry point and as operands of further combines,
 * destroyed one by one with cph_filter_destroy; their bitmaps share one device allocation, which goes with the last of
 * them).  The operands are never modified (id lists and cached effective filters hang off them) and must stay alive
 * for the duration of the call only.  All or nothing: on failure out[] is all NULL.  m == 0 returns CPH_OK and touches
 * nothing; n_bits == 0 yields empty filters without a launch.
 * CPH_INVALID_ARGUMENT: a NULL entry, operands of different n_bits or on different devices (parts: with different part
 * counts), n_b outside {m, 1} (NOT: {0}, with b NULL), an unknown op.
 * The parts form combines part p of every operand on part p's device. */
enum { CPH_FILTER_AND = 0, CPH_FILTER_OR = 1, CPH_FILTER_ANDNOT = 2, CPH_FILTER_XOR = 3, CPH_FILTER_NOT = 4 };
int cph_filters_combine(int op, const cph_filter* const* a, uint32_t m, const cph_filter* const* b, uint32_t n_b, cph_filter** out);
/* Host statement of the combine pass (plain C++, no HIP call): a_words[m][nw], b_words[m][nw] or, with b_broadcast,
 * [1][nw] (NULL for NOT), nw = (n_bits + 31) / 32; words_out[m][nw], counts_out[m].  Dirty bits behind n_bits in the
 * inputs reach neither. */
int cph_host_filter_combine(int op, const uint32_t* a_words, const uint32_t* b_words, int b_broadcast, uint64_t n_bits, uint32_t m,
                            uint32_t* words_out, uint64_t* counts_out);
/* Test hook: the production launcher on host arrays (same layout as cph_host_filter_combine): uploads every operand into
 * a slab at a 256 B stride, launches between two HIP events into an output slab pre-filled with 0xA5 bytes, downloads.
 * kernel_us (may be NULL): device time of the memset of the counts and the kernel. */
int cph_filter_combine_hook(int device, int op, const uint32_t* a_words, const uint32_t* b_words, int b_broadcast, uint64_t n_bits,
                            uint32_t m, uint32_t* words_out, uint64_t* counts_out, double* kernel_us);

/* ---- attribute columns ------------------------------------------------------------------- */
/* Up to CPH_MAX_COLUMNS more int32 columns next to the label column, addressed by slot: resident in internal-id order,
 * 4 B per row each.  cph_set_column / cph_has_column / cph_get_column are cph_set_labels / cph_has_labels /
 * cph_get_labels for the slot (values NULL drops it), and cph_filters_from_column is cph_filters_from_labels reading the
 * slot: the same kernel, range semantics, slab and single wait.  Lifecycle as for labels: build, load and load_native
 * drop every column (no file carries them); remove, set_row_map and set_result_ids leave them; compact carries them
 * (parts cut them again at the new bounds); replicas copy them.  cph_add on a handle that holds columns is
 * CPH_INVALID_ARGUMENT (the new rows would have no values: drop the columns, add, set them again at the new size);
 * cph_set_column on an index that already has a tail works, with n == size.  A slot >= CPH_MAX_COLUMNS is
 * CPH_INVALID_ARGUMENT. */
enum { CPH_MAX_COLUMNS = 8 };
int cph_set_column(cph_index* h, uint32_t slot, const int32_t* values, uint64_t n, int space);
int cph_has_column(cph_index* h, uint32_t slot, int* flag);
int cph_get_column(cph_index* h, uint32_t slot, uint64_t first, uint64_t count, int32_t* out);
int cph_filters_from_column(cph_index* h, uint32_t slot, const int32_t* lo, const int32_t* hi, uint32_t m, cph_filter** out);

/* ---- tag columns -------------------------------------------------------------------------- */
/* Set-valued attributes (the groups allowed to read a document, the topics of a chunk, the languages of a page): up to
 * CPH_MAX_TAG_COLUMNS columns, addressed by slot, each giving every row a SET of int32 tags (possibly empty).  A column is
 * resident on the device in internal-id order as a CSR: lims[n + 1] (uint32, lims[0] = 0) and tags[lims[n]], ascending
 * and distinct inside a row (4 (n + 1) + 4 nnz bytes).  A tag test is a set V of int32 values and a mode; with c(row)
 * the number of the row's tags that are in V it allows the row when
 *   CPH_TAGS_ANY   c > 0          CPH_TAGS_ALL   c == |V|          CPH_TAGS_NONE   c == 0
 * (both sides are distinct, so `all` by count is exact).  An empty V: nothing for any, every row for all and none; a
 * row without tags passes none, and all only for an empty V.  Tags compare as int32: INT32_MIN and INT32_MAX are
 * ordinary tags.
 *
 * cph_set_tags     lims[n + 1]: a non-decreasing CSR from 0 (64-bit on this side), n == size; tags[lims[n]] (may be
 *                  NULL when lims[n] == 0).  Rows in internal ids or input rows (`space`, as in cph_set_labels; the
 *                  host gathers input rows to internal order through the row map).  The rows may hold duplicates and
 *                  be unsorted: the host sorts and dedups every row before the upload.  lims == NULL drops the slot.
 *                  CPH_INVALID_ARGUMENT: slot >= CPH_MAX_TAG_COLUMNS, n != size, a lims that does not start at 0 or
 *                  decreases, more than CPH_MAX_TAGS_PER_ROW distinct tags in a row, 2^32 tags or more after dedup,
 *                  a handle that is not finalized, a borrowed replica or part handle.
 * cph_get_tags     the canonical rows of internal ids [first, first + count): lims_out[count + 1] rebased to 0 and
 *                  tags_out[lims_out[count]]; tags_out == NULL asks for the limits only.
 * cph_filters_from_tags   m tests at once, test j = values test_vals[test_lims[j] .. test_lims[j + 1]) (any order,
 *                  duplicates allowed: canonicalised on the host) under modes[j].  One upload of the tests, zeroed
 *                  counters, ONE launch over the column (csrc/device_tags.h), one copy back of the counts, one wait; the
 *                  m bitmaps share one slab at a 256 B-aligned stride, as in cph_filters_from_labels, and come out as
 *                  ordinary cph_filter objects (all made, or none).  m == 0 is a no-op.  CPH_INVALID_ARGUMENT: no
 *                  column in the slot, a mode above CPH_TAGS_NONE, more than CPH_MAX_TAG_TEST_VALUES distinct values
 *                  in a test, m above 65,535 x 64.  Allowed on a borrowed replica or part handle.
 * lifetime         exactly that of the attribute columns: cph_build, cph_load and cph_load_native drop every tag
 *                  column (no file carries them); cph_remove, cph_set_row_map and cph_set_result_ids leave them;
 *                  cph_compact carries them (the live rows' CSR is gathered again on the host); replicas copy them;
 *                  cph_add on a handle that holds a tag column is CPH_INVALID_ARGUMENT.  An index that never called
 *                  cph_set_tags allocates and launches nothing for them. */
enum { CPH_MAX_TAG_COLUMNS = 4, CPH_MAX_TAGS_PER_ROW = 1024, CPH_MAX_TAG_TEST_VALUES = 64 };
enum { CPH_TAGS_ANY = 0, CPH_TAGS_ALL = 1, CPH_TAGS_NONE = 2 };
int cph_set_tags(cph_index* h, uint32_t slot, const uint64_t* lims, const int32_t* tags, uint64_t n, int space);
int cph_has_tags(cph_index* h, uint32_t slot, int* flag);
int cph_get_tags(cph_index* h, uint32_t slot, uint64_t first, uint64_t count, uint64_t* lims_out, int32_t* tags_out);
int cph_filters_from_tags(cph_index* h, uint32_t slot, const uint32_t* test_lims, const int32_t* test_vals, const uint8_t* modes,
                          uint32_t m, cph_filter** out);
/* Debug hooks of the measurement script (scripts/tag_filter_sweep.py), as cph_debug_time_label_filters: while on, every
 * cph_filters_from_tags pass of this handle (the memset of the counts and the kernel) is bracketed by two HIP events. */
int cph_debug_time_tag_filters(cph_index* h, int on);
int cph_debug_last_tag_filters_us(cph_index* h, double* us);
/* Host statement of cph_set_tags + cph_filters_from_tags (no HIP call): the column and the tests are canonicalised with
 * the same refusals, then words_out[m][(n + 31) / 32] and counts_out[m]. */
int cph_host_tag_filters(const uint32_t* lims, const int32_t* tags, uint64_t n, const uint32_t* test_lims, const int32_t* test_vals,
                         const uint8_t* modes, uint32_t m, uint32_t* words_out, uint64_t* counts_out);

/* ---- facet counts --------------------------------------------------------------------------- */
/* Rows per distinct value of one column, under m filters at once (a terms aggregation: rows per tenant, per year, per
 * ACL group among the rows a filter allows).  The column is named by (kind, slot): CPH_FACET_LABEL (slot ignored), an
 * int32 column slot (CPH_FACET_COLUMN) or a tag column slot (CPH_FACET_TAGS).  Every column gets a DICTIONARY on first
 * use: its distinct values ascending as int32 (INT32_MIN and INT32_MAX are ordinary; removed rows are included, so the
 * list does not change under cph_remove; a tag column: the distinct tags of all rows), and one 32-bit code per row -- per
 * CSR entry for a tag column -- resident on the device (4 B each).  U, the number of values, may be 0 (an index of size
 * 0, a tag column whose rows are all empty).  The dictionary is dropped wherever the column changes (cph_set_labels,
 * cph_set_column, cph_set_tags, cph_add for the label column, cph_compact, cph_build, cph_load, cph_load_native) and
 * survives cph_remove, cph_set_row_map and cph_set_result_ids; a replica makes its own when asked.  A handle that never
 * calls cph_facet_* allocates and launches nothing for facets.
 *
 * counts[j][u] = the rows i < size that filter j allows, that are not removed, and whose value is values[u] -- for a tag
 * column: whose set holds values[u], so a row counts once per tag it holds and a row without tags adds nothing.
 * Filters are internal-id bitmaps (any cph_filter of this size and device); every one goes through F & ~R on a handle
 * with removed rows; a NULL entry, or filters == NULL with m == 1, means all live rows -- on a handle without removed
 * rows that reads no bitmap at all.
 *
 * cph_facet_prepare   makes the dictionary now instead of on the first call.
 * cph_facet_values    *U, and with values != NULL the U values.
 * cph_facet_counts    counts_out[m][U] (uint64).  One launch per group of filters (csrc/device_facets.h): up to 8,192
 *                     values (cph_facet_onchip_limit) a workgroup counts into LDS histograms and flushes its non-zero
 *                     bins with one 64-bit atomic each; above that, 64-bit global atomics.  Counters are 64-bit: no size
 *                     the handle accepts overflows them.  The device slab of one launch holds at most 2^22 counters (32
 *                     MiB; cph_facet_slab_counters): when m * U exceeds that the filters are walked in groups (a single
 *                     filter always gets its U counters).  One wait, for the outputs -- plus, on a handle with removed rows,
 *                     one pass and one wait per filter whose F & ~R is not cached yet (the first use after a
 *                     cph_remove, as in the search entries).  The caller sizes counts_out from cph_facet_values and must
 *                     not change the column in between.  m == 0 is a no-op.
 * cph_facet_top       per filter the K values (1 <= K <= 1024) with the largest non-zero counts, count descending and
 *                     ties by value ascending: values_out[m][K], counts_out[m][K], found_out[j] = min(K, values with a
 *                     non-zero count); slots at and behind found_out[j] hold value 0 and count 0.  A second launch, one
 *                     workgroup per filter, selects on the device: only m * K pairs travel.
 * CPH_INVALID_ARGUMENT, every output untouched: an unknown kind, a slot out of range or without a column, a handle that is
 *                     not finalized, a filter of another size or device, filters == NULL with m > 1, K outside [1, 1024].
 *                     Allowed on a borrowed replica or part handle. */
enum { CPH_FACET_LABEL = 0, CPH_FACET_COLUMN = 1, CPH_FACET_TAGS = 2 };
enum { CPH_FACET_PATH_AUTO = 0, CPH_FACET_PATH_ONCHIP = 1, CPH_FACET_PATH_GLOBAL = 2 };
enum { CPH_FACET_HOOK_GUARD = 64 };
int cph_facet_onchip_limit(void);
uint64_t cph_facet_slab_counters(void);
int cph_facet_prepare(cph_index* h, int kind, uint32_t slot);
int cph_facet_values(cph_index* h, int kind, uint32_t slot, uint64_t* U, int32_t* values);
int cph_facet_counts(cph_index* h, int kind, uint32_t slot, const cph_filter* const* filters, uint32_t m, uint64_t* counts_out);
int cph_facet_top(cph_index* h, int kind, uint32_t slot, const cph_filter* const* filters, uint32_t m, uint32_t K, int32_t* values_out,
                  uint64_t* counts_out, uint32_t* found_out);
/* Debug hooks, as cph_debug_time_tag_filters: while on, the launches of every cph_facet_counts / cph_facet_top of this
 * handle are bracketed by two HIP events (off by default; no event is recorded while off).  cph_debug_facet_slab lowers
 * the slab bound of this handle to `counters` (0: the default again), so that the group walk shows at small shapes. */
int cph_debug_time_facets(cph_index* h, int on);
int cph_debug_last_facets_us(cph_index* h, double* us);
int cph_debug_facet_slab(cph_index* h, uint64_t counters);
/* Host statements (no HIP call).  column: one int32 per row (lims == NULL, n_entries == n), or the tags of a CSR
 * lims[n + 1] (64-bit, canonicalised like cph_set_tags, with its refusals).  words: m bitmaps of (n + 31) / 32 words one
 * behind the other, or NULL (every filter allows every row); removed: a bitmap of removed rows, or NULL.  The outputs
 * are those of cph_facet_values / cph_facet_counts / cph_facet_top. */
int cph_host_facet_values(const int32_t* column, uint64_t n_entries, const uint64_t* lims, uint64_t n, uint64_t* U, int32_t* values);
int cph_host_facet_counts(const int32_t* column, uint64_t n_entries, const uint64_t* lims, uint64_t n, const uint32_t* words,
                          const uint32_t* removed, uint32_t m, uint64_t* counts_out);
int cph_host_facet_top(const int32_t* column, uint64_t n_entries, const uint64_t* lims, uint64_t n, const uint32_t* words,
                       const uint32_t* removed, uint32_t m, uint32_t K, int32_t* values_out, uint64_t* counts_out, uint32_t* found_out);
/* The production counting launcher on host arrays: codes[n_entries] (each < U), lims[n + 1] (uint32) for a tag column or
 * NULL for a dense one, words as above (uploaded at the 256 B-aligned slab stride; NULL: no bitmap is read).  `path`
 * forces the on-chip or the global counting path, or leaves the choice to the launcher (CPH_FACET_PATH_*; on-chip above
 * cph_facet_onchip_limit() is refused).  counts_out[m * U + CPH_FACET_HOOK_GUARD]: the device output is pre-filled with
 * 0xA5 bytes; the m * U counters come back, then the guard words behind them as the device left them. */
int cph_facet_hook(int device, const uint32_t* codes, uint64_t n_entries, const uint32_t* lims, uint64_t n, uint32_t U,
                   const uint32_t* words, uint32_t m, int path, uint64_t* counts_out, double* kernel_us);

/* Single query; writes m <= max(k,1) results (unpadded, src/bindings.cpp:146-175). */
int cph_search(cph_index* h, const float* query, uint64_t k, int64_t* ids, float* dist,
               uint64_t* m);

/* Stored vectors of internal ids [first, first+count) (dim floats each, row-major), whatever the result id space.
 * The reference never exposes its BFS permutation: for an index without a row map a harness recovers
 * internal -> input row numbers by matching these rows against its own base vectors. */
int cph_get_vectors(cph_index* h, uint64_t first, uint64_t count, float* out);

/* Batch scratch sets in rotation (default 2, at most 4): that many batches enqueued on different streams can be in
 * flight together, each on its own slots -- with fewer slots per batch (cph_set_search_params) the drain of one batch
 * is filled by the others.  Waits for everything enqueued on the handle. */
int cph_set_batch_sets(cph_index* h, uint32_t n_sets);

/* Tuning knobs (0 = automatic): resident query slots and per-slot beam capacity. */
int cph_set_search_params(cph_index* h, uint32_t slots, uint64_t beam_capacity);

/* Per-batch work counters of the last search enqueued on this handle (sums over queries; waits
 * for that batch): out[0]=expansions (FastScan blocks), [1]=exact L2 evaluations, [2]=new
 * neighbours, [3]=beam pushes, [4]=stage-2 skipped batches, [5]=queries re-run after a capacity
 * overflow, [6]=device time of the search launches in microseconds (HIP events on the launch
 * stream; with two batches in flight it includes the time shared with the other one),
 * [7]=expansions whose 32 neighbours were all estimated already, [8]=resident query slots used,
 * [9]=per-slot capacity that launch ran with, and for the probe-first instantiations (D = 128 and D = 1024 batch launches), which fetch
 * only the NEW neighbours' codes: [10]=queries (of [5]) handed to the re-run launch because the reference's stage-2
 * decision needed the rest of a block, [11]=expansions where that decision is unobservable and was left open -- there
 * [4] counts only the skips that were decided, a lower bound of the reference's counter (0 / exact for every other
 * instantiation). */
int cph_last_search_stats(cph_index* h, uint64_t out[12]);
/* Vertices expanded by each query of the last batch (its first pass); n = that batch's size. */
int cph_last_query_expansions(cph_index* index, uint32_t* out, uint64_t n);
/* Launch order of a batch (hook of the counting sort that hands queries out closest-entry-first):
 * order[n] = permutation of 0..n-1, ascending in the top 14 bits of the non-negative float keys. */
int cph_order_queries(cph_index* index, const float* keys, uint64_t n, uint32_t* order);

/* ---- one index on several devices (in-process replicas; csrc/multi_device.h) ----------------------------------- */
/* The reference's search_batch uses every host core in one call; a cph_multi uses several GPUs (or several replicas
 * on one GPU) in one call, with no launcher and no collective.  The index is replicated on every listed device,
 * queries are split into contiguous shards, each shard runs the single-device cph_search_batch[_filtered] on its
 * replica, and results land straight in the caller's rows: byte-identical to a single-device handle.
 *
 *   create   devices[n_dev]: HIP ordinals, 1 <= n_dev <= 16, duplicates allowed (several replicas on one GPU).
 *   load / load_native / finalize
 *            run once on replica 0 (the file is read and parsed, or mapped, once; the builder runs on replica 0);
 *            replicas 1..N-1 then receive replica 0's resident device arrays by device-to-device copy.  Host memory
 *            for the index is held once: only replica 0 keeps host arrays.  If a call fails after replica 0 gave up
 *            its previous index, no replica is searchable until the next successful load / finalize.
 *   save / save_native
 *            from replica 0: the same bytes as cph_save / cph_save_native.
 *   build    pending vectors on replica 0; the previous index leaves every replica.
 *   search_batch[_filtered]
 *            queries split into shards whose sizes differ by at most one, none smaller than min_shard
 *            (cph_multi_set_min_shard; default 1024); fewer than 2 * min_shard queries go whole to one replica, round
 *            robin.  Each shard runs on its replica's persistent worker thread; the call returns when every shard has
 *            finished, also on error (no worker touches ids / dist afterwards).  On failure the status and
 *            cph_last_error() text (on the calling thread) are those of the lowest-numbered failing replica.
 *            f[n_dev]: one filter per replica, each made with cph_filter_create on that replica (NULL = unfiltered).
 *   search   one single query, routed to one replica (round robin), whose coalescer gathers it with that replica's
 *            other callers: the same answer as cph_search.
 *   last_search_stats / last_query_expansions
 *            over the replicas of the last search_batch[_filtered]: words 0-5, 7, 8, 10, 11 summed, 6 (kernel_us)
 *            and 9 (capacity) the maximum; expansions concatenated in query order.
 *   has_row_map / set_row_map / set_result_ids
 *            the row map lives on replica 0 (host copy) and, resident, on every replica: set_row_map validates once and
 *            hands it to all of them, set_result_ids switches all of them; both wait for the searches in flight.
 *            Filters in input rows: cph_filter_create_rows on each borrowed replica handle.
 *   replica  borrowed handle of replica i (owned by m; never destroyed by the caller): cph_search_batch_device on that
 *            device, cph_filter_create, cph_set_search_params / cph_set_batch_sets, the hooks.  cph_load,
 *            cph_load_native, cph_build, cph_finalize, cph_set_row_map and cph_destroy on it fail with CPH_INVALID_ARGUMENT; on
 *            replicas other than 0 so do cph_save, cph_save_native and cph_get_vectors (no host arrays).
 * Threads: search_batch[_filtered] and search may be called concurrently from any number of threads; load,
 * load_native, build, finalize and destroy wait for the searches in flight on the multi handle. */
typedef struct cph_multi cph_multi;
int cph_multi_create(uint64_t dim, uint64_t bits, const int* devices, uint32_t n_dev, cph_multi** out);
int cph_multi_destroy(cph_multi* m);
int cph_multi_load(cph_multi* m, const char* path);
int cph_multi_load_native(cph_multi* m, const char* path);
int cph_multi_save(cph_multi* m, const char* path);
int cph_multi_save_native(cph_multi* m, const char* path);
int cph_multi_build(cph_multi* m, const float* vectors, uint64_t n);
int cph_multi_finalize(cph_multi* m);
int cph_multi_size(cph_multi* m, uint64_t* n);
int cph_multi_is_finalized(cph_multi* m, int* flag);
int cph_multi_search_batch(cph_multi* m, const float* queries, uint64_t n, uint64_t k, int64_t* ids, float* dist);
int cph_multi_search_batch_filtered(cph_multi* m, const float* queries, uint64_t n, uint64_t k,
                                    const cph_filter* const* f, int64_t* ids, float* dist);
/* cph_search_batch_exact sharded like cph_multi_search_batch_filtered; f = NULL, or one filter per replica. */
int cph_multi_search_batch_exact(cph_multi* m, const float* queries, uint64_t n, uint64_t k,
                                 const cph_filter* const* f, int64_t* ids, float* dist);
/* cph_search_batch_filters sharded like cph_multi_search_batch_filtered: filters[f * n_dev + r] = filter f on replica r;
 * the shards are contiguous and filter_of is sliced with the queries. */
int cph_multi_search_batch_filters(cph_multi* m, const float* queries, uint64_t n, uint64_t k, const cph_filter* const* filters,
                                   uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids, float* dist);
/* The range search (host form) over the same shards: every shard runs cph_range_search_begin / _finish on its replica's
 * worker; begin sums the totals, finish writes every shard's segments behind those of the shards before it.  The bytes are
 * those of one device.  f = NULL, or one filter per replica.  (The device form is the single-device call on a replica.)
 * Destroy the object before the multi handle. */
typedef struct cph_multi_range cph_multi_range;
int cph_multi_range_search_begin(cph_multi* m, const float* queries, uint64_t n, const float* radius_host,
                                 const cph_filter* const* f, int exact, uint64_t max_results, cph_multi_range** out,
                                 uint64_t* total);
int cph_multi_range_search_finish(cph_multi_range* r, int64_t* lims_host, int64_t* ids, float* dist);
int cph_multi_range_destroy(cph_multi_range* r);
/* cph_search_grouped over the same shards, every shard on its replica's worker; the bytes are those of one device.
 * keys: NULL (every replica's label column) or one cph_group_keys per replica, keys[r] made with cph_multi_replica(m, r);
 * filters[f * R + r] = filter f on replica r (R replicas), as in cph_multi_search_batch_filters; filter_of == NULL takes
 * n_filters 0 or 1.  Every replica is asked before any shard runs: a refusal leaves no row written. */
int cph_multi_search_grouped(cph_multi* m, const float* queries, uint64_t n, uint64_t k, uint64_t group_size, uint64_t candidates,
                             const cph_group_keys* const* keys, const cph_filter* const* filters, uint32_t n_filters,
                             const int32_t* filter_of, int exact, int64_t* ids, float* dist, int32_t* group_keys, int32_t* counts,
                             uint8_t* complete);
/* cph_search_diverse over the same shards (plan_shards), every shard on its replica's worker; the bytes are those of one
 * device.  filters[f * R + r] = filter f on replica r; every replica is asked before any shard runs. */
int cph_multi_search_diverse(cph_multi* m, const float* queries, uint64_t n, uint64_t k, float lam, uint64_t candidates,
                             const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids,
                             float* dist, float* gap);
/* cph_search_maxsim over the same shards: the QUERIES are sharded (plan_shards over n), never the tokens of one query;
 * n_tokens and filter_of are sliced with them, every shard runs on its replica's worker, the bytes are those of one
 * device.  keys and filters as in cph_multi_search_grouped; every replica is asked before any shard runs. */
int cph_multi_search_maxsim(cph_multi* m, const float* queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                            uint64_t candidates, const cph_group_keys* const* keys, const cph_filter* const* filters, uint32_t n_filters,
                            const int32_t* filter_of, int exact, int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows,
                            int32_t* out_found);
/* cph_search_maxsim_rescored over the same shards; every replica keeps an inverted key column of its own. */
int cph_multi_search_maxsim_rescored(cph_multi* m, const float* queries, uint64_t n, uint64_t tokens, const int32_t* n_tokens, uint64_t k,
                                     uint64_t candidates, uint64_t rescore, const cph_group_keys* const* keys,
                                     const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact,
                                     int32_t* out_keys, float* out_score, int32_t* out_hits, int64_t* out_rows, int32_t* out_found,
                                     int32_t* out_certified);
/* cph_search_fused, sharded by query (never inside one query's vectors): n_vectors, weights, filter_of and the outputs are
 * sliced by shard; filters[f * R + r] as in cph_multi_search_grouped.  The bytes are those of one device. */
int cph_multi_search_fused(cph_multi* m, const float* queries, uint64_t n, uint64_t vectors, const int32_t* n_vectors, const float* weights,
                           uint64_t k, uint64_t candidates, const cph_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                           int exact, int64_t* ids, float* score, int32_t* hits);
int cph_multi_set_exact_threshold(cph_multi* m, uint64_t max_allowed);
int cph_multi_search(cph_multi* m, const float* query, uint64_t k, int64_t* ids, float* dist, uint64_t* count);
int cph_multi_has_row_map(cph_multi* m, int* flag);
int cph_multi_set_row_map(cph_multi* m, const uint32_t* rows, uint64_t n);
int cph_multi_set_result_ids(cph_multi* m, int space);
int cph_multi_set_min_shard(cph_multi* m, uint64_t q);
int cph_multi_last_search_stats(cph_multi* m, uint64_t out[12]);
int cph_multi_last_query_expansions(cph_multi* m, uint32_t* out, uint64_t n);
/* cph_remove on every replica before the call returns (it waits for the searches in flight); live_count / get_removed from
 * replica 0; compact on replica 0, then copied to the others like finalize.  cph_remove / cph_compact on a borrowed replica
 * handle fail with CPH_INVALID_ARGUMENT. */
int cph_multi_remove(cph_multi* m, const int64_t* ids, uint64_t cnt, int space, uint64_t* newly);
int cph_multi_live_count(cph_multi* m, uint64_t* n);
int cph_multi_get_removed(cph_multi* m, uint32_t* words);
int cph_multi_compact(cph_multi* m, int64_t* old_to_new);
int cph_multi_num_replicas(cph_multi* m, uint32_t* n);
int cph_multi_replica(cph_multi* m, uint32_t i, cph_index** out);

/* ---- one index split across several devices (parts; csrc/partitioned.h, csrc/device_merge.h) ------------------- */
/* A cph_multi replicates: more queries per second, the same capacity and the same build time.  A cph_parts PARTITIONS
 * (what FAISS calls IndexShards): part p is an ordinary single-device index over the contiguous input rows
 * [lo_p, hi_p) on devices[p] (ordinals may repeat), every query goes to all parts, and their rows are merged.
 *
 *   create   devices[n_dev]: HIP ordinals, 1 <= n_dev <= 16.  devices[0] is the home device: the merge runs there.
 *   build    n rows: part p gets rows [n/P * p + min(p, n % P), ...): contiguous, sizes differ by at most one
 *            (cph_host_part_bounds).  n < 64 * P is CPH_INVALID_ARGUMENT.
 *   finalize every part's builder at once, each on its part's worker thread, with 1 / P of the host threads
 *            (CPH_BUILD_THREADS or its default, divided by P).
 *   ids      input rows only: every id is lo_p + (the part's input row).  There is no internal id space across parts.
 *   search_batch[_filtered | _exact | _filters]
 *            every part searches the whole batch with the caller's k (the existing cph_search_batch_device* of the part,
 *            CPH_IDS_INPUT, on the part's worker thread); the P rows of a query travel to the home device (a peer copy
 *            where hipDeviceCanAccessPeer allows it, else through pinned host memory) and row i of the answer is the
 *            first k entries of their STABLE MERGE in part order: ascending distance compared as float values, equal
 *            distances lower part first, inside a part the part's own order (numpy: argsort(concatenate(rows),
 *            kind="stable")[:k]).  Padding (-1 / FLT_MAX) sorts last and stays padding; a part's duplicate slots pass
 *            through; distance bytes are the part's.  _exact: the exact global top-k, equal distance bits ordered by part,
 *            then by the part's internal id.  The exact threshold (set_exact_threshold) is compared with the PART's
 *            allowed count; a part whose slice of a filter is empty returns padding without a launch.
 *   search_batch_device (and the _filtered, _exact_device, _filters_device forms)
 *            queries and results on the home device.  The call waits ON THE HOST for the searches of all parts, then
 *            enqueues the merge on `stream` and returns: the results are complete in stream order.  filter_of is host
 *            memory.
 *   search   a batch of one through all parts (not the coalesced path of cph_search); *count results, unpadded.
 *   filter_create_rows
 *            words = allowed-row bitmap over ALL input rows (n_bits = size).  It is cut at the part bounds and every
 *            part gets cph_filter_create_rows on its slice; the object holds the P filters.
 *   last_search_stats
 *            out[0..11] as cph_last_search_stats, summed over the parts, kernel_us ([6]) and capacity ([9]) the maximum;
 *            out[12] = device time of the merge kernel in microseconds.  last_query_expansions: summed per query.
 *   save_native / load_native
 *            one ordinary format-2 native file per part, `path`.p<i>of<P>.  load_native validates all P files first: a
 *            missing file (also: saved with another number of parts), a wrong dim or bits, or a part without a row map
 *            is CPH_INVALID_ARGUMENT and leaves the handle as it was; the validated files are then installed as read.  A
 *            device failure during that (out of memory) leaves no part searchable until the next successful load_native
 *            or finalize.  There is no v2 form: that format holds one graph and no row map.
 *   part     borrowed handle of part i (owned by m): searches, filters, hooks, cph_get_row_map, cph_get_vectors in the
 *            part's own spaces.  cph_load*, cph_build, cph_finalize, cph_set_row_map and cph_destroy on it fail; switching
 *            it to CPH_IDS_INTERNAL makes the searches of m fail until it is switched back.
 *   bounds   out[P + 1]: part p holds input rows [out[p], out[p + 1]).
 * Threads: searches on one handle run one after the other; build, finalize, load_native and destroy wait for them. */
typedef struct cph_parts cph_parts;
typedef struct cph_parts_filter cph_parts_filter;
int cph_parts_create(uint64_t dim, uint64_t bits, const int* devices, uint32_t n_dev, cph_parts** out);
int cph_parts_destroy(cph_parts* m);
int cph_parts_build(cph_parts* m, const float* vectors, uint64_t n);
int cph_parts_finalize(cph_parts* m);
int cph_parts_size(cph_parts* m, uint64_t* n);
int cph_parts_is_finalized(cph_parts* m, int* flag);
int cph_parts_save_native(cph_parts* m, const char* path);
int cph_parts_load_native(cph_parts* m, const char* path);
int cph_parts_search_batch(cph_parts* m, const float* queries, uint64_t n, uint64_t k, int64_t* ids, float* dist);
int cph_parts_search_batch_filtered(cph_parts* m, const float* queries, uint64_t n, uint64_t k, const cph_parts_filter* f,
                                    int64_t* ids, float* dist);
int cph_parts_search_batch_exact(cph_parts* m, const float* queries, uint64_t n, uint64_t k, const cph_parts_filter* f,
                                 int64_t* ids, float* dist);
int cph_parts_search_batch_filters(cph_parts* m, const float* queries, uint64_t n, uint64_t k,
                                   const cph_parts_filter* const* filters, uint32_t n_filters, const int32_t* filter_of, int exact,
                                   int64_t* ids, float* dist);
int cph_parts_search_batch_device(cph_parts* m, const float* d_queries, uint64_t n, uint64_t k, int64_t* d_ids, float* d_dist,
                                  void* stream);
int cph_parts_search_batch_device_filtered(cph_parts* m, const float* d_queries, uint64_t n, uint64_t k, const cph_parts_filter* f,
                                           int64_t* d_ids, float* d_dist, void* stream);
int cph_parts_search_batch_exact_device(cph_parts* m, const float* d_queries, uint64_t n, uint64_t k, const cph_parts_filter* f,
                                        int64_t* d_ids, float* d_dist, void* stream);
int cph_parts_search_batch_filters_device(cph_parts* m, const float* d_queries, uint64_t n, uint64_t k,
                                          const cph_parts_filter* const* filters, uint32_t n_filters, const int32_t* filter_of,
                                          int exact, int64_t* d_ids, float* d_dist, void* stream);
int cph_parts_search(cph_parts* m, const float* query, uint64_t k, int64_t* ids, float* dist, uint64_t* count);
int cph_parts_set_exact_threshold(cph_parts* m, uint64_t max_allowed);
int cph_parts_filter_create_rows(cph_parts* m, const uint32_t* words, uint64_t n_bits, cph_parts_filter** out);
int cph_parts_filter_destroy(cph_parts_filter* f);
int cph_parts_last_search_stats(cph_parts* m, uint64_t out[13]);
int cph_parts_last_query_expansions(cph_parts* m, uint32_t* out, uint64_t n);
/* Removed rows of a partitioned index: ids are GLOBAL input rows, cut at the part bounds; every part keeps its own R (a
 * part whose rows are all removed returns padding without a launch).  get_removed: words[(size + 31) / 32] over global
 * input rows.  compact: a full cph_parts_build + cph_parts_finalize of the live rows in row order, so the parts are cut
 * again by cph_host_part_bounds; old_to_new[old size] in global rows; fewer live rows than cph_parts_build takes is its
 * error and leaves the handle as it was. */
int cph_parts_remove(cph_parts* m, const int64_t* ids, uint64_t cnt, uint64_t* newly);
int cph_parts_live_count(cph_parts* m, uint64_t* n);
int cph_parts_get_removed(cph_parts* m, uint32_t* words);
int cph_parts_compact(cph_parts* m, int64_t* old_to_new);
/* The label column (cph_set_labels) of replicas and parts.  Replicas: the column on every replica (waits for the
 * searches in flight); the per-replica filters are made with cph_filters_from_labels on each borrowed replica handle.
 * Both set calls ask every replica / part first and change none when one refuses (a part without a row map).  Parts: labels[n] over GLOBAL input rows, cut at the part
 * bounds; cph_parts_filters_from_labels lets every part evaluate its own slice (a part in which no row matches holds an
 * empty filter and returns padding without a launch); cph_parts_filter_count: allowed rows over all parts.  finalize,
 * load* and build drop the column on every replica and part; cph_multi_compact and cph_parts_compact carry it (parts cut
 * it again at the new bounds). */
int cph_multi_set_labels(cph_multi* m, const int32_t* labels, uint64_t n, int space);
int cph_parts_set_labels(cph_parts* m, const int32_t* labels, uint64_t n);
int cph_parts_filters_from_labels(cph_parts* m, const int32_t* lo, const int32_t* hi, uint32_t cnt, cph_parts_filter** out);
int cph_parts_filter_count(const cph_parts_filter* f, uint64_t* count);
/* The attribute columns (cph_set_column) and the filter algebra (cph_filters_combine) of replicas and parts, exactly as
 * the label calls above: one slot on every replica; values[n] over GLOBAL input rows cut at the part bounds; every part
 * evaluates its own slice; part p of every operand is combined on part p's device.  The per-replica forms of
 * cph_filters_from_column and cph_filters_combine are the single-handle calls on each replica's handle and filters. */
int cph_multi_set_column(cph_multi* m, uint32_t slot, const int32_t* values, uint64_t n, int space);
int cph_parts_set_column(cph_parts* m, uint32_t slot, const int32_t* values, uint64_t n);
int cph_parts_filters_from_column(cph_parts* m, uint32_t slot, const int32_t* lo, const int32_t* hi, uint32_t cnt, cph_parts_filter** out);

/* The tag columns (cph_set_tags) of replicas and parts, as the column calls above: one slot on every replica (the
 * canonical column is made once); lims[n + 1] / tags over GLOBAL input rows, cut at the part bounds with the limits
 * rebased; every part evaluates its own slice.  cph_multi_compact and cph_parts_compact carry the columns. */
int cph_multi_set_tags(cph_multi* m, uint32_t slot, const uint64_t* lims, const int32_t* tags, uint64_t n, int space);
int cph_parts_set_tags(cph_parts* m, uint32_t slot, const uint64_t* lims, const int32_t* tags, uint64_t n);
int cph_parts_filters_from_tags(cph_parts* m, uint32_t slot, const uint32_t* test_lims, const int32_t* test_vals, const uint8_t* modes,
                                uint32_t cnt, cph_parts_filter** out);
int cph_parts_filters_combine(int op, const cph_parts_filter* const* a, uint32_t m, const cph_parts_filter* const* b, uint32_t n_b,
                              cph_parts_filter** out);
int cph_parts_num_parts(cph_parts* m, uint32_t* n);
int cph_parts_part(cph_parts* m, uint32_t i, cph_index** out);
int cph_parts_bounds(cph_parts* m, uint64_t* out);
/* Test hook: merge_parts_kernel on given rows (host arrays): ids / dist [P][n][k], every row ascending in distance,
 * lo[P]; out_ids / out_dist [n][k] are uploaded first, so a slot the kernel did not write keeps the caller's value.
 * 1 <= P <= 16, n >= 1, k >= 1. */
int cph_merge_rows_hook(int device, const int64_t* ids, const float* dist, uint32_t P, uint64_t n, uint64_t k, const int64_t* lo,
                        int64_t* out_ids, float* out_dist);

/* ---- kernel-level hooks ------------------------------------------------------------ */
/* Query encoder (encoder/rabitq_encoder.hpp:73-79,98-136,197-209): lut = u8[D/4][16] in
 * the reference's LUT format, coeffs = {coeff_fastscan, coeff_popcount, coeff_constant}. */
int cph_encode_query(cph_index* h, const float* query, uint8_t* lut, float* coeffs);

/* Upper-layer greedy descent (api/hnsw_index.hpp:196-202,617-638): layer-0 entry id. */
int cph_entry_point(cph_index* h, const float* query, uint32_t* entry);

/* One 32-neighbour FastScan block on the GPU for vertex `vertex` of the loaded index:
 * sums[32] (1-bit: plane sum; N-bit: weighted N-bit sum), msb[32] (plane-0 sum),
 * est[32]/lower[32] as search consumes them (stage-2 skip applied when nn_full != 0 and
 * no stage-1 lower bound is below `worst`: est = FLT_MAX, lower = stage-1 bound),
 * lower_stage1[32] (convert_msb_to_lower_bounds; == lower for 1-bit).
 * qparams = {coeff_fastscan, coeff_popcount, coeff_constant, affine_a, affine_b,
 * ip_qo_floor, dot_slack}.  (distance/fastscan_kernel.hpp:17-425,
 * search/rabitq_search.hpp:159-206) */
int cph_fastscan_block(cph_index* h, const uint8_t* lut, const float* qparams,
                       uint32_t vertex, float dist_qp_sq, float worst, int nn_full,
                       uint32_t* sums, uint32_t* msb, float* est, float* lower,
                       float* lower_stage1);

/* Exact L2 (search/rabitq_search.hpp:90-93, core/memory.hpp:81-95) of `query` against
 * nodes ids[0..n). */
int cph_exact_l2(cph_index* h, const float* query, const uint32_t* ids, uint64_t n,
                 float* out);

/* Streaming FastScan roofline benchmark on synthetic neighbour blocks (no graph).
 * create: allocates n_blocks device blocks of layout (D,bits) filled with seeded random
 * valid codes/aux.  run: `reps` passes over all blocks with one encoded query, both
 * N-bit stages per block; writes the average kernel time per pass (HIP events on the
 * launch stream), and a checksum.  block_bytes = device bytes per block. */
typedef struct cph_stream cph_stream;
int cph_fastscan_stream_create(int device, uint32_t D, uint32_t bits, uint64_t n_blocks,
                               uint64_t seed, cph_stream** out, uint64_t* block_bytes);
int cph_fastscan_stream_run(cph_stream* s, int reps, double* avg_ms, double* checksum);
/* Copies block `i` out in the REFERENCE neighbour-block layout
 * (distance/fastscan_layout.hpp:51-92,114-155) and the query (lut u8[D/4][16], 7 qparams,
 * dist_qp_sq) so a CPU implementation can be run on identical inputs. */
int cph_fastscan_stream_export(cph_stream* s, uint64_t first, uint64_t count,
                               uint8_t* ref_blocks, uint8_t* lut, float* qparams,
                               float* dist_qp_sq);
/* est/lower of block i as computed by the stream kernel (for parity checks). */
int cph_fastscan_stream_eval(cph_stream* s, uint64_t first, uint64_t count, float* est,
                             float* lower);
int cph_fastscan_stream_destroy(cph_stream* s);

/* ---- host-only hooks (no HIP call; used by the CPU test tier) --------------------------------- */
/* Reads a v2 index file with the library's reader and writes it back with its writer. */
int cph_host_rewrite_index(const char* path_in, const char* path_out);
/* Repacks one reference-layout neighbour block (distance/fastscan_layout.hpp:51-155) into the device
 * layout (dev_block, *dev_bytes bytes) and back into `ref_roundtrip`. */
int cph_host_repack_block(uint32_t D, uint32_t bits, const uint8_t* ref_block, uint8_t* dev_block,
                          uint64_t* dev_bytes, uint8_t* ref_roundtrip);
/* Host restatement of the device re-layout: one device block in the storage layout (what cph_host_repack_block
 * writes) -> the layout it is resident in on the GPU (4-bit codes at D >= 128: neighbour-major nibbles; every other
 * format: unchanged), and back into `dev_roundtrip` (optional).  All three are dev_bytes long. */
int cph_host_relayout_block(uint32_t D, uint32_t bits, const uint8_t* dev_block, uint8_t* resident_block,
                            uint8_t* dev_roundtrip);
/* Copies device blocks [first, first + count) of a finalized index to `out` (count x dev_bytes): as they are
 * resident on the GPU (resident != 0), or converted back to the storage layout by the device (resident == 0). */
int cph_export_blocks(cph_index* h, uint64_t first, uint64_t count, int resident, uint8_t* out);
/* Host mirror of the query encoder (the device encoder is cph_encode_query): lut u8[D/4][16],
 * coeffs[3], masks u32[max(1,D/32)][4] (the bit-sliced form the kernels consume). */
int cph_host_encode_query(uint64_t dim, const float* query, uint8_t* lut, float* coeffs, uint32_t* masks);
/* Host statement of the conversion in cph_filter_create_rows: bit i of words_out = bit rows[i] of words_in for the n
 * internal ids (both bitmaps (n + 31) / 32 words; bits of the last output word behind n are clear).  Every rows[i] must
 * be < n. */
int cph_host_rows_filter(const uint32_t* words_in, const uint32_t* rows, uint64_t n, uint32_t* words_out);

/* Host statement of the effective filter of a handle with removed rows (csrc/device_tombstone.h: live_filter_kernel):
 * words_out = words_f & ~words_removed over n ids (words_f NULL: every id), all bitmaps (n + 31) / 32 words; bits of the
 * last word behind n are ignored in both inputs and clear in the output; *count_out (may be NULL) = ids left. */
int cph_host_live_filter(const uint32_t* words_f, const uint32_t* words_removed, uint64_t n, uint32_t* words_out,
                         uint64_t* count_out);

/* Host statement of the compaction the exact search runs on a filter: out_ids = the set bits of words (bit id & 31 of
 * word id >> 5, bits behind n_bits ignored) in ascending order, *out_count = how many.  out_ids holds popcount entries. */
int cph_host_filter_ids(const uint32_t* words, uint64_t n_bits, uint32_t* out_ids, uint64_t* out_count);
/* How an exact batch of n_queries against `candidates` ids is cut on a device of num_cus compute units with at most
 * scratch_bytes of pool scratch (the planner the exact entry points run; 1 <= k <= 1024): out[6] = parts, candidates per
 * part, queries per group, queries per launch, keys per pool, pool bytes.  More than one part: the merge kernel folds the
 * parts' lists; queries per launch < n_queries: the batch is tiled inside the call. */
int cph_host_exact_plan(uint64_t candidates, uint64_t n_queries, uint64_t k, int num_cus, uint64_t scratch_bytes, uint64_t* out);
/* The grouping of a batch with per-query filters (no HIP call).  popcounts[n_filters] = allowed ids of every filter.
 * routes[n_filters + 1]: 0 padded row, 1 exact scan, 2 graph search, per filter and, last, for the queries with -1.
 * perm[n]: the queries ordered by filter (those with -1 last), inside a filter in query order; seg[n_filters + 2]: the
 * queries of filter f are perm[seg[f] .. seg[f + 1]), the unfiltered ones the last segment. */
int cph_host_filter_groups(const int32_t* filter_of, uint64_t n, const uint64_t* popcounts, uint32_t n_filters, uint64_t k,
                           int exact, uint64_t exact_threshold, uint8_t* routes, uint32_t* perm, uint32_t* seg);
/* The work-item table of the grouped scan (no HIP call): segment s = seg_candidates[s] ids against seg_queries[s]
 * queries; 1 <= k <= 1024.  out[6] = items, launches, queries per group, pool capacity C in keys, pool bytes of the
 * largest launch, 0.  items (may be NULL with cap_items 0, to size the table): the first cap_items rows of 8 words --
 * segment, part, first candidate, end candidate, first query of the segment, queries, pool index inside the launch of
 * (part, first query), launch.  A segment has at most 256 parts; a launch's pools stay within scratch_bytes unless one
 * query group of one part alone exceeds it. */
int cph_host_exact_group_plan(const uint64_t* seg_candidates, const uint64_t* seg_queries, uint32_t n_segments, uint64_t k,
                              int num_cus, uint64_t scratch_bytes, uint32_t* items, uint64_t cap_items, uint64_t* out);
/* The part bounds of a partitioned index (no HIP call): out[P + 1], part p of P over n rows holds the input rows
 * [out[p], out[p + 1]); 1 <= P <= 16. */
int cph_host_part_bounds(uint64_t n, uint32_t P, uint64_t* out);

/* ---- the metric -------------------------------------------------------------------------- */
/* CPH_METRIC_L2 (the default): distances are squared L2.  CPH_METRIC_COSINE: distances are 1 - cos(q, x).
 *
 * A cosine index stores x~ = x / sqrt(2 |x|^2), so |x~|^2 = 1/2, and gives queries the same treatment; then
 * || q~ - x~ ||^2 = 1/2 + 1/2 - (q.x) / (|q||x|) = 1 - cos(q, x), and every search of the library -- graph, exact, tail,
 * range, grouped, diverse, replicas, parts, single query -- reports the cosine distance with the kernels of the L2
 * metric: smaller is better, radii of cph_range are in 1 - cos, ties and padding mean what they meant.  One kernel
 * (csrc/device_normalize.h) normalises rows on the way in and queries on the way into every search, one launch per
 * batch on the batch's stream; an L2 handle launches and allocates nothing for it.  Its arithmetic is fixed (fp32): lane
 * l of 64 sums x[j] * x[j] over j = l, l + 64, ... (product and sum rounded separately), a xor butterfly (32, 16, 8, 4,
 * 2, 1) gives s, t = sqrt(s + s), out[j] = x[j] / t, both correctly rounded.  Scaling a row by a power of two changes no
 * output bit.
 *
 * cph_set_metric / cph_multi_set_metric / cph_parts_set_metric: on an empty handle only (nothing built, pending or
 *     loaded); later calls are CPH_INVALID_ARGUMENT.  The multi and parts forms set every replica / part.
 * rows in: cph_build, cph_multi_build, cph_parts_build and cph_add normalise the rows; what the index stores, returns
 *     from cph_get_vectors, writes to files and replicates are the normalised rows.  A row without a direction -- all
 *     zero, a NaN or Inf in it, a squared norm that overflows fp32 -- refuses the call with CPH_INVALID_ARGUMENT; the
 *     message names the first such row (of the call's array; a partitioned index: the global row) and their count, and
 *     the handle is as it was.  cph_compact passes its live rows through as they are.
 * queries in: a query without a direction is searched as the zero vector -- every distance is then the stored squared
 *     norm of the row, about 0.5 -- and no call refuses it: the device forms only enqueue and cannot.
 * hooks: cph_encode_query, cph_entry_point, cph_exact_l2, cph_fastscan_block and the calibration hooks act on the
 *     vector as given; they do not normalise.
 * files: cph_save_native writes the metric as a trailing record (format 4, csrc/native_file.h) that older readers
 *     refuse; an L2 index is written byte for byte as before and a file without the record is L2.  cph_load_native
 *     refuses a file whose metric is not the handle's.  cph_save / cph_load (the reference's format, which has no place
 *     for a metric) are refused on a cosine handle. */
enum { CPH_METRIC_L2 = 0, CPH_METRIC_COSINE = 1 };
int cph_set_metric(cph_index* h, int metric);
int cph_get_metric(cph_index* h, int* metric);
int cph_multi_set_metric(cph_multi* m, int metric);
int cph_parts_set_metric(cph_parts* m, int metric);
/* out[0] = launches of the normalisation kernel this handle has made (rows and queries), out[1] = bytes of normalised-
 * query buffers its batch sets hold.  Both stay 0 on an L2 handle.  Counted on the host, not timed. */
int cph_metric_stats(cph_index* h, uint64_t out[2]);
/* Test hook: the kernel on host arrays x, out [n][dim] (out == x: in place; otherwise the device output starts as 0xA5
 * bytes, so a slot the kernel left alone shows).  bad_count: rows without a direction (written as +0.0f); first_bad: the
 * lowest such row, UINT64_MAX when there is none.  cph_host_normalize_rows is the host statement
 * (csrc/host_normalize.h, no HIP call). */
int cph_normalize_rows_hook(int device, const float* x, uint64_t n, uint64_t dim, float* out, uint64_t* bad_count, uint64_t* first_bad);
int cph_host_normalize_rows(const float* x, uint64_t n, uint64_t dim, float* out, uint64_t* bad_count, uint64_t* first_bad);

/* ---- the inner-product metric ---------------------------------------------------------------- */
/* CPH_METRIC_IP: maximum inner product search.  Every search returns score = -(q.x): smaller is better and rows ascend,
 * as with the other metrics; ties and padding (-1 / FLT_MAX) mean what they meant.
 *
 * With M2 >= max |x|^2 the index stores x~ = [x, sqrt(M2 - |x|^2)], dim + 1 coordinates, and searches q~ = [q, 0]:
 * |q~ - x~|^2 = |q|^2 + M2 - 2 q.x falls as q.x grows, so the graph, exact, tail and filter kernels of the L2 metric rank
 * by inner product as they stand.  One kernel in front of them (csrc/device_ip.h) augments rows on the way in and queries
 * on the way into every batch, where it also writes c = |q|^2 + M2 per query; one kernel behind them turns every
 * distance whose id is not padding into 0.5 * (d - c), one subtraction and one multiplication, each rounded once.  Both
 * run on the batch's stream, once per batch; cph_search_batch_device stays enqueue-only.  |x|^2 is the cosine metric's
 * sum (64 lane sums, xor butterfly), the root is correctly rounded, and the first dim stored coordinates are the
 * caller's bits.
 *
 * widths: cph_set_metric_ip / cph_multi_set_metric_ip, on an empty handle only, make the metric CPH_METRIC_IP (what
 *     cph_get_metric reports and files carry), the stored width dim + 1 and the padded width next_pow2(dim + 1); they
 *     refuse when that exceeds 2048, so dim is 8..2047.  (cph_set_metric itself keeps taking L2 and cosine only and
 *     refuses 2 like every other value, as it did before this metric existed: callers and tests rely on that.)  The extra coordinate is free wherever
 *     dim is not a power of two and doubles the padded width at dim = 16, 32, ..., 1024.  cph_dim keeps reporting the
 *     caller's dim; rows and queries come in at that width.
 * bound: cph_set_ip_bound(h, M2) on an empty IP handle; 0 (the default) takes the largest |x|^2 of the rows of the
 *     cph_build call, found on the device.  cph_get_ip_bound: the M2 of the rows the handle holds (before a build: the
 *     bound set).  Every replica holds it; cph_compact keeps it and does not augment again.
 * rows in: cph_build, cph_multi_build and cph_add refuse (CPH_INVALID_ARGUMENT, naming the first such row and the count,
 *     the handle as it was) a row with a NaN, an Inf or an overflowing |x|^2, and a row with |x|^2 > M2; cph_add checks
 *     against the M2 of the index, which only a rebuild with a larger bound raises.  A zero row is a good row.  What the
 *     index stores, replicates, writes to files and returns from cph_get_vectors are the stored rows, dim + 1 wide.
 * queries in: a query with a NaN, an Inf or an overflowing norm searches as the zero vector with c = M2 (every score is
 *     then 0 up to rounding); no call refuses it.
 * single queries: cph_search runs as a batch of one (the coalesced path hands a row to its caller from inside the search
 *     kernel, before an epilogue could run).
 * hooks: cph_encode_query, cph_entry_point, cph_exact_l2, cph_fastscan_block and the calibration hooks act on vectors of
 *     the stored width as given.
 * not served yet, refused with CPH_INVALID_ARGUMENT before any output is written: cph_range_*, cph_search_grouped*,
 *     cph_search_diverse*, cph_search_maxsim* (and their multi forms), cph_parts_set_metric(CPH_METRIC_IP), cph_save and
 *     cph_load.
 * files: cph_save_native writes format 5 (csrc/native_file.h): format 4's record with version 5, metric 2, M2 and a zero
 *     word, which every older reader refuses; cph_load_native restores M2 and refuses a file of another metric.
 * cph_metric_stats counts the launches of both kernels and the bytes of the augmented-query and c buffers. */
enum { CPH_METRIC_IP = 2 };
int cph_set_metric_ip(cph_index* h);
int cph_multi_set_metric_ip(cph_multi* m);
int cph_set_ip_bound(cph_index* h, float max_sq_norm);
int cph_get_ip_bound(cph_index* h, float* m2);
int cph_multi_set_ip_bound(cph_multi* m, float max_sq_norm);
int cph_multi_get_ip_bound(cph_multi* m, float* m2);
/* Test hooks: the kernels on host arrays.  x [n][dim] -> out [n][dim + 1]; mode 0: rows against max_sq_norm, 1: rows
 * against the largest |x|^2 of the good rows of x (found by the max pass), 2: queries, which also write c [n] (c may be
 * null otherwise).  The device outputs start as 0xA5 bytes.  *m2: the bound used; counters = {bad rows, rows over the
 * bound, the lowest row of either kind or UINT64_MAX}.  The epilogue hook rewrites dist [n][k] in place; pinned != 0
 * runs it on pinned, device-mapped host memory.  cph_host_ip_* are the host statement (csrc/host_ip.h, no HIP call). */
int cph_ip_augment_hook(int device, const float* x, uint64_t n, uint64_t dim, int mode, float max_sq_norm, float* out, float* c, float* m2, uint64_t counters[3]);
int cph_ip_epilogue_hook(int device, const int64_t* ids, float* dist, uint64_t n, uint64_t k, const float* c, int pinned);
int cph_host_ip_augment(const float* x, uint64_t n, uint64_t dim, int mode, float max_sq_norm, float* out, float* c, float* m2, uint64_t counters[3]);
int cph_host_ip_epilogue(const int64_t* ids, float* dist, uint64_t n, uint64_t k, const float* c);

/* ---- two-stage search: rescoring candidates against resident full-size rows (not in the reference) ----
 * For embeddings whose prefix is itself a usable embedding: the index holds the first cph_dim coordinates, a
 * cph_rescore_vectors object the full dim_full coordinates of the same rows, and one call runs the ordinary search at
 * k = candidates and rescores those candidates against the full rows on the device, on the same stream.  Filters,
 * exact, per-query filters, removed rows, the tail, both id spaces, the cosine metric and the refusals are those of the
 * search underneath.  The statement is csrc/host_rescore.h (host form) and tests/rescore_model.py (numpy form).
 *
 * cph_rescore_vectors_create  rows [size][dim_full] float32 (host), size == cph_size, 1 <= dim_full <= 8192, indexed by
 *     internal ids or by input rows (space = CPH_IDS_INPUT: needs a row map; the inverse of the map is made once on the
 *     host and rescore_rows_in_kernel writes every row at its internal position).  dtype: how the rows are stored,
 *     CPH_RESCORE_FLOAT16 (round to nearest even) or CPH_RESCORE_FLOAT32; the row stride is padded with zeros to a
 *     multiple of 16 bytes, and one float32 squared norm per row is summed from the stored values.  metric:
 *     CPH_RESCORE_L2 or CPH_RESCORE_IP -- it belongs to the object, not to the index (cosine: normalise rows and full
 *     queries and use CPH_RESCORE_IP).  The rows are uploaded in chunks of at most 256 MB.  A row that holds a NaN or an
 *     Inf, a value that overflows float16, or whose squared norm overflows refuses the call (CPH_INVALID_ARGUMENT: the
 *     lowest such row and their number); no object exists then and nothing stays allocated.
 *     The object is resident on the handle's device and follows the rules of cph_group_keys: it serves the handle and
 *     the index it was made for (a load, build or compact invalidates it: "made for another index"; after cph_add it is
 *     refused with the size message), another device refuses it, cph_save_native does not carry it.
 * cph_rescore_vectors_destroy waits for the device, then frees; NULL is a no-op.
 * cph_rescore_vectors_info    size, dim_full, dtype, metric, the stored bytes of a row and the device bytes of the object.
 * cph_rescore_vectors_get     the stored bytes of rows [first, first + count): rows_out [count][row bytes], norms_out
 *     [count]; waits for the device.
 *
 * cph_search_rescored  queries [n][cph_dim] go to the graph, full_queries [n][dim_full] to the rescoring (dim_full must
 *     be the object's); both pointers are always given (a Matryoshka caller passes the prefixes as `queries`).
 *     k <= candidates <= 1024.  Per query, over its candidate row (internal ids, -1 / FLT_MAX padding): padding, ids at
 *     or above cph_size and every occurrence of an id after its first are dropped; each survivor is scored in float32,
 *     every product and sum rounded on its own, in the sum shape csrc/host_rescore.h states (a pure function of dim_full
 *     and dtype) -- L2: max(0, (|q|^2 + |x|^2) - 2 q.x), IP: -(q.x); a NaN score is dropped; the k best by (score,
 *     internal id) ascending are returned: ids [k] int64 (input rows under CPH_IDS_INPUT), score [k], first [k] = the
 *     candidate's first-stage distance bytes; unused slots are -1 / FLT_MAX / FLT_MAX.  A query whose |q|^2 is not < inf
 *     gets a row of padding.  rescore_rows_kernel (csrc/device_rescore.h), one workgroup per query, writes every slot.
 *     cph_search_rescored takes and returns host arrays and waits; cph_search_rescored_device takes device pointers
 *     and only enqueues on `stream`.  Refused before any output is written: an inner-product index, a stale, foreign or
 *     wrong-size object, k > candidates, candidates > 1024, a dim_full that is not the object's.  Partitioned indexes
 *     have no rescored search: every part has its own internal ids.
 * cph_multi_search_rescored  the same over the shards of a replicated index; vectors[r] = the object made on
 *     cph_multi_replica(m, r); the bytes are those of one device.
 * cph_debug_time_rescored / cph_debug_last_rescored_us  as cph_debug_time_diverse: the rescore_rows_kernel launch of every
 *     rescored search of this handle between two HIP events while switched on.
 * Test hooks: cph_rescore_rows_hook runs the kernel on given host candidate rows (ids / dist [n][candidates]) and full
 *     queries [n][dim_full of the object]; the device outputs start as 0xA5 bytes.  cph_host_rescore_rows is the host
 *     statement over stored rows and norms as cph_rescore_vectors_get returns them; cph_host_rescore_rows_in the host
 *     statement of the conversion, the scatter and the norms (row_map [n_map]: rows arrive in input order and row
 *     row_map[i] goes to position i, rows at or above n_map stay where they are; NULL: internal order); *bad = the
 *     number of refused rows, *first_bad the lowest (UINT64_MAX: none).  Neither makes a HIP call. */
enum { CPH_RESCORE_FLOAT16 = 0, CPH_RESCORE_FLOAT32 = 1 };
enum { CPH_RESCORE_L2 = 0, CPH_RESCORE_IP = 1 };
typedef struct cph_rescore_vectors cph_rescore_vectors;
int cph_rescore_vectors_create(cph_index* h, const float* rows, uint64_t size, uint64_t dim_full, int space, int dtype, int metric,
                               cph_rescore_vectors** out);
int cph_rescore_vectors_destroy(cph_rescore_vectors* rv);
int cph_rescore_vectors_info(const cph_rescore_vectors* rv, uint64_t* size, uint64_t* dim_full, int* dtype, int* metric, uint64_t* row_bytes,
                             uint64_t* nbytes);
int cph_rescore_vectors_get(const cph_rescore_vectors* rv, uint64_t first, uint64_t count, void* rows_out, float* norms_out);
int cph_search_rescored(cph_index* h, const float* queries, uint64_t n, const float* full_queries, uint64_t dim_full, uint64_t k,
                        uint64_t candidates, const cph_rescore_vectors* vectors, const cph_filter* const* filters, uint32_t n_filters,
                        const int32_t* filter_of, int exact, int64_t* ids, float* score, float* first);
int cph_search_rescored_device(cph_index* h, const float* d_queries, uint64_t n, const float* d_full_queries, uint64_t dim_full, uint64_t k,
                               uint64_t candidates, const cph_rescore_vectors* vectors, const cph_filter* const* filters, uint32_t n_filters,
                               const int32_t* filter_of, int exact, int64_t* d_ids, float* d_score, float* d_first, void* stream);
int cph_multi_search_rescored(cph_multi* m, const float* queries, uint64_t n, const float* full_queries, uint64_t dim_full, uint64_t k,
                              uint64_t candidates, const cph_rescore_vectors* const* vectors, const cph_filter* const* filters,
                              uint32_t n_filters, const int32_t* filter_of, int exact, int64_t* ids, float* score, float* first);
int cph_debug_time_rescored(cph_index* h, int on);
int cph_debug_last_rescored_us(cph_index* h, double* us);
int cph_rescore_rows_hook(cph_index* h, const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const float* full_queries,
                          const cph_rescore_vectors* vectors, uint64_t k, int64_t* out_ids, float* out_score, float* out_first);
int cph_host_rescore_rows(const int64_t* ids, const float* dist, uint64_t n, uint64_t candidates, const float* full_queries,
                          uint64_t dim_full, const void* stored, const float* norms, uint64_t n_ids, int dtype, int metric,
                          const uint32_t* rows, uint64_t k, int64_t* out_ids, float* out_score, float* out_first);
int cph_host_rescore_rows_in(const float* rows_in, uint64_t n, uint64_t dim_full, int dtype, const uint32_t* row_map, uint64_t n_map,
                             void* stored, float* norms, uint64_t* bad, uint64_t* first_bad);

#ifdef __cplusplus
}
#endif
#endif /* CPHNSW_MI355X_H */
