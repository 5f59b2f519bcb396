/*
 * vdb.h — C-ABI of the MI355X (gfx950) brute-force vector-search core.
 *
 * This is the drop-in boundary for the hot path of Theseus-AT/mlx-vector-db.
 * The reference has no FFI of its own: its "operator slot" is the Python
 * callable `MLXVectorStore._compiled_similarity_fn(query, vectors) -> scores[N]`
 * followed by `mx.argsort(...)[:k]`
 * (reference service/optimized_vector_store.py:31-48, :149-192, :211-213) and
 * the batched variant in performance/mlx_optimized.py:59-88, :217-248.
 * Each entry point below names the reference interface it replaces.
 * A ctypes binding (mlx-vector-db_amd/service/_vdb.py) is the host side; the
 * binding a maintainer would add to the reference is shown in INTEGRATION.md.
 *
 * Conventions
 *   - Every function returns an int32 status (VDB_OK = 0, negative = error
 *     class); vdb_last_error() returns a thread-local message for the last
 *     failing call on the calling thread.
 *   - Plain pointers and sizes only.  `mem` says whether the query / output
 *     pointers of a call are host (VDB_MEM_HOST) or device (VDB_MEM_DEVICE)
 *     memory.  Device-memory calls are stream-ordered on `stream` (a
 *     hipStream_t; NULL = the null stream, which orders with PyTorch's default
 *     stream) and return without waiting: the results are in device memory
 *     once the stream reaches that point (the exactness certificate is
 *     checked and any fallback queued on the device, see vdb_index_search).
 *     Host-memory calls run on `stream` or, if NULL, on a stream of the
 *     per-search workspace they take (so concurrent host-memory searches from
 *     several threads overlap on the device) and return when the results are
 *     in host memory.
 *   - The library never frees caller memory.  An index owns its device-resident
 *     corpus: row-major fp32 rows (the exact rerank), the int8
 *     candidate copy in MFMA operand tiles (two planes, the default pass) with
 *     its row-major hi plane and column sums, and -- for the bf16 / fp32
 *     precisions, or under auto only once a search first runs a split pass --
 *     a split-bf16 (fp32) candidate copy; plus a per-call workspace pool.
 *   - All entry points are thread-safe; searches on one index may run from
 *     several threads at once (the reference serves from a 4-thread executor,
 *     api/routes/vectors.py:43).
 *
 * Result contract:
 *   cosine    score = (q/max(|q|,1e-8)) . (x/max(|x|,1e-8))   higher first
 *   euclidean score = sqrt(sum((x-q)^2))                        lower first
 *   Ranking is by the exact (fp64, canonical summation order) value with ties
 *   broken by the lower row index; returned scores are that value rounded to
 *   fp32.  Rows beyond the number of eligible rows are returned as index -1.
 */
#ifndef VDB_H
#define VDB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    VDB_OK = 0,
    VDB_ERR_INVALID = -1,     /* bad argument -> Python ValueError          */
    VDB_ERR_HIP = -2,         /* HIP runtime error -> RuntimeError          */
    VDB_ERR_OOM = -3,         /* device allocation failed                   */
    VDB_ERR_NONFINITE = -4,   /* NaN/Inf in vectors or queries -> ValueError */
    VDB_ERR_UNSUPPORTED = -5, /* e.g. metric "dot_product" (reference raises,
                                 service/optimized_vector_store.py:153-154)   */
    VDB_ERR_NODEVICE = -6     /* no gfx950 device visible                    */
};

enum { VDB_METRIC_COSINE = 0, VDB_METRIC_EUCLIDEAN = 1, VDB_METRIC_DOT = 2 /* operator slot only */ };
enum { VDB_MEM_HOST = 0, VDB_MEM_DEVICE = 1 };

/* Candidate-pass arithmetic for an index (vdb_index_set_param "precision").
 * The returned results are identical for all (the exact fp64 rerank decides);
 * only the speed of the candidate pass differs.
 *   VDB_PREC_FP32    fp32 v_mfma_f32_32x32x2_f32 (MFMA-bound, 157 TF peak)
 *   VDB_PREC_BF16X3  split-bf16 "x3": x = hi + lo, q = hi + lo,
 *                    x.q ~ xh.qh + xh.ql + xl.qh on v_mfma_f32_32x32x16_bf16,
 *                    fp32 accumulate; error bound of the same order as fp32
 *                    (HBM-bound).  Keeps a split copy of the corpus (same bytes
 *                    as the fp32 copy).
 *   VDB_PREC_BF16    the hi plane of the split copy only: x.q ~ xh.qh + xh.ql,
 *                    half the corpus bytes per search; the certificate adds a bound
 *                    of the corpus rounding q.(x - bf16(x)) measured at ingest:
 *                    min(|q| R, |q - c d| R + |c| M), R the largest row residual,
 *                    d the normalised mean row of the first add, M the largest
 *                    |d.(x - bf16(x))|, c = q.d, so it is wider
 *                    and takes a larger candidate margin.
 *   VDB_PREC_I8      an int8 copy of the CENTRED rows z = y - mu (y the scored row, mu the
 *                    mean row of the first add), 16-bit fixed point in two planes
 *                    z ~ s_x (xh + xl/256); the query 16-bit fixed point per batch.  I8
 *                    reads the hi plane only (1 byte per element, a quarter of the fp32
 *                    copy): x.q ~ s_x s_q (xh.qh + xh.ql/256) on v_mfma_i32_32x32x32_i8
 *                    (exact integer sums, twice the K of a bf16 MFMA per cycle); the
 *                    certificate adds the measured row rounding (as BF16: Cauchy-Schwarz or
 *                    along d) and each query's own rounding (vdb_scan8_kernel.h).
 *   VDB_PREC_I8X3    both planes (2 bytes per element): xh.qh + (xh.ql + xl.qh)/256, an
 *                    error bound of bf16x3's order at half its bytes and MFMA cycles.
 *   VDB_PREC_AUTO    (default) per batch, on the int8 copy (knob "auto_int8" = 1, the
 *                    default; start value from VDB_AUTO_I8): I8 for k <= 16, I8X3 for k > 16
 *                    (a one-plane pass would need 256 candidates per query there); on the split
 *                    copy (auto_int8 = 0): BF16 / BF16X3.  A host-memory search re-passes its
 *                    uncertified one-plane queries (at most 1/8 of the batch, at most 64) in
 *                    BF16X3 as one gathered sub-search and keeps its precision; more than that
 *                    reruns the batch in BF16X3 and starts a HOLD on the next precision down
 *                    the list I8 -> BF16 -> BF16X3 (an I8X3 failure: its batch takes the exact
 *                    path, the hold runs BF16X3) for the next 16 searches, doubling per failed
 *                    probe up to 2048 (reset by 64 certified searches, or when the rows change).
 *                    A device-memory search sees its fallback counts a search or more late (no
 *                    host sync): its flagged queries take the device-gated exact path and the
 *                    next search starts the hold.  Stats "repass_queries", "auto_hold",
 *                    "auto_hold8". */
/*   VDB_PREC_I8Q     the int8 copy's xh plane (1 byte per element) against the 16-bit query:
 *                    xh.qh + xh.ql / 256, two int8 MFMAs per group.  AUTO's pass for L2 with
 *                    16 < k <= 100 (KP = 256) until a batch flags more than 1/8 of its queries
 *                    (then I8X3 for good, stat "i8q_off"). */
enum { VDB_PREC_FP32 = 0, VDB_PREC_BF16X3 = 1, VDB_PREC_BF16 = 2, VDB_PREC_AUTO = 3, VDB_PREC_I8 = 4, VDB_PREC_I8X3 = 5,
       VDB_PREC_I8Q = 6 };

typedef struct vdb_index vdb_index;

/* --- library -------------------------------------------------------------- */
const char* vdb_last_error(void);
int32_t vdb_version(void);
/* Number of visible HIP devices (0 on a host without a GPU). */
int32_t vdb_device_count(int32_t* n);

/* --- index lifecycle -------------------------------------------------------
 * Replaces MLXVectorStore's corpus state `self._vectors` (mx.array [N,D] f32)
 * and `_compile_critical_functions` (service/optimized_vector_store.py:59-83,
 * :211-213).  metric: VDB_METRIC_*.  Any other metric -> VDB_ERR_UNSUPPORTED,
 * matching the reference, where "dot_product" leaves no operator and every
 * query raises. */
int32_t vdb_index_create(int32_t dim, int32_t metric, int32_t device, vdb_index** out);
int32_t vdb_index_destroy(vdb_index* idx);
/* Pre-size the device corpus for `rows` rows (capacity otherwise doubles). */
int32_t vdb_index_reserve(vdb_index* idx, int64_t rows);
/* Knobs.  "precision" (VDB_PREC_*; default VDB_PREC_AUTO), "margin" (extra candidates
 * per query), "force_exact" (0/1), "no_fallback" (diagnostics: flagged queries keep the
 * approximate order), "timing" (0/1: HIP events around the candidate pass; stats "scan_ns",
 * "pipeline_ns", "timed_searches").  Tuning knobs the bench's A/B runs use (results identical,
 * speed differs): "n_wg" (candidate-pass workgroups), "scan_variant" / "scan_variant_bf16x3"
 * (fp32 / split pass tilings), "scan_sync" (0 auto, 1 per-step barrier, 2 flag-gated
 * compaction rounds), "scan_q4" (split pass 128-query shape, -1 auto / 0 / 1), "scan_qlds"
 * (-1 auto: query block in LDS when it fits, 0 never), "scan_wide" (the wide int8 passes, all
 * queries of a batch in one workgroup's registers: -1 auto from 65 536 rows -- rows of <= 128
 * dims with > 256 queries, or <= 256 up to 2.5M rows; I8 cosine rows of 512..1536 dims with
 * <= 256 queries (1536: <= 16 or > 96) -- 0 off, 1 whenever the shape allows),
 * "scan_checksum" (1 default, 0 off, 2 also I8X3's L sums), "pilot_tiles", "pilot_rank",
 * "finish_split", "finish_small" (-1 auto: the finish's 4-wave form beside a long-row
 * wide scan for batches of >= 32, 0 off, 1 on), "i8_refine", "i8_narrow", "device_repass", "auto_int8", "auto_i8q",
 * "dir_bound" (0: BF16 certificate with |q| R only), "remove_chunk" / "update_chunk" (rows per
 * chunk of vdb_index_remove's scratch / vdb_index_update's staging, 0 = by bytes), "subset_wgs"
 * (workgroups per query of vdb_index_search_rows, 0 = auto; its stats "subset_searches",
 * "subset_queries", "subset_rows", "subset_bad_ids" are described there; vdb_index_search_range's
 * are "range_searches", "range_queries"), "group_fetch" (rows vdb_index_search_groups' inner
 * search fetches, 0 = auto, 1..200) and "group_force_exact" (0/1; its stats "group_rows",
 * "group_sets", "group_searches", "group_queries", "group_fallback_queries" are described
 * there; vdb_index_search_mmr's are "mmr_searches", "mmr_queries"; vdb_index_search_recommend's
 * "recommend_searches", "recommend_queries", "recommend_bad_queries"; vdb_index_search_fused's
 * "fused_searches", "fused_sets", "fused_bad_sets"; vdb_index_search_maxsim's "maxsim_searches",
 * "maxsim_sets", "maxsim_bad_sets", "maxsim_skipped_rows") and "sparse_wgs" (workgroups per query
 * of vdb_index_search_sparse, 0 = auto; the sparse and hybrid calls' stats "sparse_rows",
 * "sparse_nnz", "sparse_sets", "sparse_searches", "sparse_queries", "sparse_bad_queries",
 * "hybrid_searches", "hybrid_queries" are described there) and "hybrid_sum_wgs" (workgroups per
 * query of vdb_index_search_hybrid_sum, 0 = auto, 1..512; its stats "hybrid_sum_searches",
 * "hybrid_sum_queries" are described there).  The numeric columns and predicate masks have no
 * knob; their stats "column_slots", "column_sets", "filter_calls", "filter_preds" are described at
 * vdb_index_filter_mask.  Stats also: "searches", "queries",
 * "fallback_queries", "overflow_queries", "inconsistent_queries", "repass_queries",
 * "capacity", "count", "device_bytes", "precision", "searches_fp32" / "searches_bf16x3" /
 * "searches_bf16" / "searches_i8" / "searches_i8x3" / "searches_i8q" (candidate passes run in
 * each; with VDB_PREC_AUTO these show its choices), "searches_q4", "searches_wide",
 * "auto_int8", "i8q_off", "i8_wide", "split_copy", "split_copy_builds", "rows_removed",
 * "rows_updated". */
int32_t vdb_index_set_param(vdb_index* idx, const char* name, int64_t value);
int32_t vdb_index_get_stat(const vdb_index* idx, const char* name, int64_t* value);

/* --- ingest ------------------------------------------------------------------
 * Replaces MLXVectorStore.add_vectors' `mx.concatenate([old, new])`
 * (service/optimized_vector_store.py:96-106; mlx_optimized.py:127-137).
 * Appends n rows of `dim` fp32 (row-major) in place (capacity doubling), packs
 * them into the MFMA-tiled layout and computes the per-row norms once.
 * Non-finite input -> VDB_ERR_NONFINITE and nothing is appended.  Device-memory rows
 * (mem = VDB_MEM_DEVICE) are read after the work queued on `stream` so far (NULL = the
 * null stream); the call returns when the rows are ingested (the source may be reused). */
int32_t vdb_index_add(vdb_index* idx, const float* vectors, int64_t n, int32_t mem, void* stream);
int32_t vdb_index_count(const vdb_index* idx, int64_t* n);
/* Replaces MLXVectorStore.clear (service/optimized_vector_store.py:198-209). */
int32_t vdb_index_clear(vdb_index* idx);
/* Remove the rows whose bit is set in remove_mask (ceil(count/32) uint32 words, bit r of word
 * r/32 = row r; same layout and memory kinds as the search's row_mask; bits at or past
 * count are ignored).  Surviving rows keep their order and move down: row r becomes
 * r - (removed rows below r).  *n_removed (optional) = rows removed.  Returns when done.
 * Replaces: nothing in the reference server, which cannot delete; the counterpart is its
 * Python SDK's delete_vectors_by_metadata (sdk/python/mlx_vector_db_client.py:292-303,
 * POST /vectors/delete).  The rows are compacted on the device (a stable gather driven by the
 * bitmap, DESIGN.md "Deleting rows") and the candidate copies of the moved rows rebuilt from
 * them with the centring row, quantisation step and residual direction left as they are; the
 * capacity stays.  Waits for the searches queued on this index first; a device-memory mask is
 * read after the work queued on `stream`.  A mask with no bit set below count touches nothing;
 * one that removes every row leaves the index as a clear does.  Knob "remove_chunk" (rows per
 * chunk of the gather's scratch, 0 = sized by bytes); stat "rows_removed" (cumulative).  A
 * graph built before a remove or a clear is stale for good (search and add report it), even
 * once later adds bring the count back. */
int32_t vdb_index_remove(vdb_index* idx, const uint32_t* remove_mask, int32_t mem, void* stream,
                         int64_t* n_removed);
/* Update rows in place: row rows[i] becomes vectors[i] (i < n; vectors [n][dim] row-major fp32,
 * rows n ids in [0, count), pairwise distinct, any order).  mem: VDB_MEM_HOST or VDB_MEM_DEVICE,
 * both pointers of the same kind; device-memory arguments are read after the work queued on
 * `stream` (NULL = the null stream).  Returns when done; count and capacity stay; n == 0 is
 * VDB_OK and touches nothing.
 * Replaces: nothing in the reference's store, which cannot change a vector it holds; the
 * counterpart is the `upsert` its own benchmark calls on the database it compares itself with
 * (benchmarks/benchmark_app.py:104).  Without this call: vdb_index_remove + vdb_index_add, which
 * compacts and renumbers every row above the first removed one.
 * All or nothing: an id outside [0, count) or a repeated id -> VDB_ERR_INVALID, a NaN or Inf in
 * vectors -> VDB_ERR_NONFINITE, and the index is exactly as it was (rows, norms, candidate
 * copies, column sums, running maxima).  An update overwrites live rows, so validation is a pass
 * of its own before the first write: one kernel per staged chunk checks range, finiteness and
 * repeats (a ceil(count/32)-word scratch bitmap), the host reads the flags (one sync), then the
 * apply is queued.  A host-memory call of more than one staging chunk therefore sends its rows
 * to the device twice, once to validate and once to apply.
 * The apply rewrites, for the updated rows only, the fp32 row and its row terms, the candidate
 * copies the current precision reads (the lazily built split copy included) and the int8 copy's
 * column sums (old bytes out, new bytes in); the centring row, quantisation step and residual
 * direction stay as they are and the running maxima are only raised (DESIGN.md "Updating rows").
 * Waits for the searches queued on this index first.  Knob "update_chunk" (rows per staging
 * chunk, 0 = sized by bytes at 256 MiB as an add's staging); stat "rows_updated" (cumulative).
 * A graph built before an update is stale (search and add report it). */
int32_t vdb_index_update(vdb_index* idx, const int64_t* rows, const float* vectors, int64_t n, int32_t mem,
                         void* stream);
/* Copy rows [start, start+n) back out, row-major fp32, to host memory (used for
 * vectors.npz persistence, service/optimized_vector_store.py:218-223). */
int32_t vdb_index_get_vectors(vdb_index* idx, int64_t start, int64_t n, float* out_host);

/* --- search ------------------------------------------------------------------
 * Replaces `_brute_force_search`: similarity fn + mx.argsort(...)[:k] + gather
 * (service/optimized_vector_store.py:149-192) for B=1, and
 * `optimized_batch_similarity_search` (performance/mlx_optimized.py:217-248)
 * for B>1.
 *   queries      [n_queries, dim] fp32 row-major (host or device per `mem`)
 *   k            1..1024 results per query (min(k, eligible rows) are valid)
 *   row_mask     NULL, or a bitmap of ceil(count/32) uint32 words (bit r of
 *                word r/32 = row r eligible): the metadata filter
 *                (service/optimized_vector_store.py:159-167); same memory kind
 *                as `mem`.
 *   out_scores   [n_queries, k] fp32 (cosine similarity / euclidean distance)
 *   out_indices  [n_queries, k] int64 row ids (+ index_offset), -1 = no result
 *   out_keys     NULL or [n_queries, k] fp64 exact ranking keys (cosine: the
 *                similarity; euclidean: minus the squared distance) — what a
 *                multi-GPU merge needs to stay bit-identical to one GPU.
 */
int32_t vdb_index_search(vdb_index* idx, const float* queries, int32_t n_queries, int32_t k,
                         const uint32_t* row_mask, int32_t mem,
                         float* out_scores, int64_t* out_indices, double* out_keys,
                         int64_t index_offset, void* stream);

/* Search explicit row-id lists, one per query or shared between queries: only the listed rows
 * are scored, exactly, so a selective filter costs its own rows and not a pass over the corpus.
 * Replaces: the reference's O(N) metadata scan plus masked argsort
 * (service/optimized_vector_store.py:159-183), for which vdb_index_search's row_mask is the
 * whole-corpus form: one bitmap for the batch, every row streamed.
 *   list_offsets [n_lists + 1] int64, list_rows [n_ids] int64: the candidate sets in CSR form,
 *                list l = list_rows[list_offsets[l] .. list_offsets[l+1]), offsets ascending
 *                from >= 0 to <= n_ids, each list strictly ascending row ids in [0, count).
 *                An empty list is valid (every slot of its queries is "no result").
 *   n_ids        host scalar, the length of list_rows: the launch is sized from it, so a
 *                device-memory call reads nothing back.
 *   query_list   [n_queries] int32, query b searches list query_list[b]; several queries may
 *                share a list.  NULL = query b searches list b (n_lists == n_queries).
 *   queries, k, mem, out_*, index_offset, stream: as vdb_index_search; all pointers of one
 *                memory kind.  n_queries == 0 is VDB_OK.
 * Result: that of vdb_index_search over row_mask = exactly the list's set, bit for bit --
 * ranking by the canonical fp64 key, ties to the lower row, scores the key rounded to fp32, slots
 * past min(k, list length) index -1 / score 0 / key -inf -- for every precision setting: the
 * rows come from the row-major fp32 copy and the candidate copies are not read.
 * One launch per call plus the query norms: grid (workgroups per query, queries), a wave per
 * row, per-wave streaming top-k, and the workgroup that finishes a query last merges its lists.
 * Host-memory calls are validated before anything is launched: offsets that decrease or pass
 * n_ids, an id outside [0, count), a list not strictly ascending, a query_list entry outside
 * [0, n_lists) -> VDB_ERR_INVALID; NaN / Inf in a query -> VDB_ERR_NONFINITE.  A device-memory
 * call cannot be validated without a sync, so the kernel handles such input itself: offsets are
 * clamped to [0, n_ids], a query whose query_list entry is out of range gets an empty result,
 * and an id outside [0, count) or not greater than the entry before it in its list is skipped
 * and counted (stat "subset_bad_ids", once per query that meets it); nothing out of bounds is
 * read.  Takes the index's shared lock, a per-search workspace and its stream as a search does
 * (add / remove / update / clear wait for queued calls).  Stats (cumulative, successful calls):
 * "subset_searches", "subset_queries", "subset_rows" (ids offered), "subset_bad_ids".  Knob
 * "subset_wgs": workgroups per query, 0 = auto from n_ids over the lists (or queries, if fewer)
 * and the CU count; results are identical for every value. */
int32_t vdb_index_search_rows(vdb_index* idx, const float* queries, int32_t n_queries, int32_t k,
                              const int64_t* list_offsets, int32_t n_lists, const int64_t* list_rows, int64_t n_ids,
                              const int32_t* query_list, int32_t mem,
                              float* out_scores, int64_t* out_indices, double* out_keys,
                              int64_t index_offset, void* stream);

/* Range search: every stored row within a score threshold of a query, exactly, with exact counts.
 * Replaces: the "ask for more and cut" the reference's own RAG pipeline does, a k * 2 fetch with
 * the results under min_similarity dropped afterwards (integrations/mlx_lm_pipeline.py:725-736),
 * which silently returns too few whenever more than 2k rows qualify; and it answers what no top-k
 * call can: "is anything within t of this vector" and "how many rows are within t".
 *   thresholds   [n_queries] fp64, in score units.  cosine: a minimum similarity t, kt = t.
 *                euclidean: a radius t >= 0, kt = -(t * t) (one fp64 multiply).  -inf (cosine) or
 *                +inf (euclidean) passes every eligible row.
 *   row_mask     as vdb_index_search.
 *   cap          slots per query, >= 0, with n_queries * cap <= 2^36 (else VDB_ERR_INVALID, for
 *                either memory kind).  0 = count only (the three list pointers may be NULL).
 *   out_counts   [n_queries] int64, required: the exact number of eligible passing rows, also
 *                when it exceeds cap.
 *   out_indices  [n_queries, cap] int64, out_scores [n_queries, cap] fp32 (required when cap > 0),
 *   out_keys     NULL or [n_queries, cap] fp64.
 *   queries, mem, index_offset, stream: as vdb_index_search; all pointers of one memory kind.
 *                n_queries == 0 is VDB_OK.  index_offset is added to the returned ids only.
 * Result: row r passes query b when its canonical fp64 key -- the key vdb_index_search ranks by
 * and returns in out_keys -- satisfies key >= kt[b]; a key equal to kt passes.  The first
 * min(count, cap) passing rows are returned in ASCENDING ROW ID, each with its key rounded to the
 * fp32 score as a search rounds it; the slots after them hold index -1 / score 0 / key -inf, and
 * nothing at or past cap is written.  (Ascending row order needs no sort of unbounded length and
 * never depends on the order atomics land in; best-first for a result that fits is one host sort,
 * and best-first truncated is what vdb_index_search is.)  The result is the same bytes for every
 * precision setting: the rows come from the row-major fp32 copy, the candidate copies are not
 * read and no "searches_*" stat moves.
 * Launches, per block of up to 64 queries (fewer for long rows): a scan that reads every row once
 * for the whole block and writes a hit bitmap per query plus per-workgroup hit counts (no
 * atomics); a prefix over those counts, which also gives the exact totals; and, when cap > 0, an
 * emit that writes the ids of the hits below cap and a scoring pass over the filled slots, so the
 * list work is proportional to min(count, cap).  Blocks run one after another on one stream over
 * the same scratch.
 * Host-memory calls are validated before anything is launched: NaN / Inf in a query ->
 * VDB_ERR_NONFINITE; a NaN threshold, a negative euclidean radius or a cap outside its bounds ->
 * VDB_ERR_INVALID.  A device-memory call cannot be validated without a sync (the cap aside): its kernel gives a
 * query with a NaN threshold or a negative radius a count of 0, and nothing out of bounds is read
 * or written.  Device-memory calls are stream-ordered and read nothing back; host-memory calls
 * take a per-search workspace, its stream and one pinned staging copy each way, as
 * vdb_index_search_rows does.  Takes the index's shared lock (add / remove / update / clear wait
 * for queued calls).  An empty index gives counts 0 and every slot "no result".  Stats
 * (cumulative, successful calls): "range_searches", "range_queries". */
int32_t vdb_index_search_range(vdb_index* idx, const float* queries, int32_t n_queries,
                               const double* thresholds, const uint32_t* row_mask, int32_t mem,
                               int64_t cap, int64_t* out_counts, int64_t* out_indices,
                               float* out_scores, double* out_keys, int64_t index_offset, void* stream);

/* Grouped search: the k best DISTINCT groups of a query, each with its best row (Qdrant's "search
 * groups", Milvus' "group by").
 * Replaces: nothing in the reference's store; its RAG pipeline stores document_id /
 * document_source beside every chunk (integrations/mlx_lm_pipeline.py:656-670, :747-751) and can
 * only ask for the best k chunks.  Without this call: over-fetch with vdb_index_search and
 * de-duplicate on the host, which returns too few documents whenever one long document fills the
 * fetched list.
 *
 * vdb_index_set_groups attaches a group column: groups [n] int32, n == count (else
 * VDB_ERR_INVALID), host or device memory per `mem` (device: read after the work queued on
 * `stream`).  A negative id means the row has no group and is never returned.  The index keeps a
 * device copy, builds the bitmap of the rows with an id >= 0 and notes whether any id is negative.
 * groups == NULL with n == 0 detaches the column.  Takes the exclusive lock, waits for queued
 * searches and returns when done, as an add does.  Every successful add, remove and clear drops
 * the column (its rows no longer line up); vdb_index_update keeps it.  Stats: "group_rows" (rows
 * attached, 0 = none), "group_sets" (cumulative).
 *
 * vdb_index_search_groups:
 *   k            1..128 groups per query
 *   out_groups   [n_queries, k] int32, required: the group id of each slot, -1 = no result
 *   out_scores / out_indices / out_keys: [n_queries, k], slot j = the BEST ROW of the j-th group
 *   queries, row_mask, mem, index_offset, stream: as vdb_index_search; all pointers of one memory
 *                kind.  n_queries == 0 is VDB_OK; at most 65 535 queries per call.
 * Result: a row is eligible when its group id is >= 0 and row_mask (if given) has its bit.  The
 * best row of a group is its eligible row with the best canonical fp64 key, ties to the lower row
 * id (the order vdb_index_search uses); groups rank by (best key desc, best row asc).  The score
 * is the key rounded to fp32 as a search rounds it.  Slots past the number of eligible groups
 * hold index -1 / score 0 / key -inf / group -1.  The result is the same bytes for every
 * precision setting and both memory kinds.
 * How: the ordinary certified search fetches the best k' >= k eligible rows with their keys into
 * scratch (k' <= 200; knob "group_fetch": 0 = auto, 200 rows, or 1 for k = 1; 1..200 sets it, never
 * below k); one select kernel marks each group's first occurrence in that ranked list and writes
 * the first k.  The list settles the query when it holds k groups, when it came back short of k',
 * or when the call's eligible rows (those with a group and their mask bit, counted on the device;
 * mask bits at or past count name no row) number at most k': then every eligible row was seen.
 * Any other query is flagged on the device and answered by an exact scan kept per (key, row,
 * group), launched for the whole batch and gated per query, so a device-memory call never waits.  Results are identical for every
 * group_fetch; knob "group_force_exact" (0/1) sends every query to the exact scan (tests, A/B).
 * Errors: no column attached, k outside [1, 128], n_queries above 65 535, a NULL queries / out_scores / out_indices /
 * out_groups -> VDB_ERR_INVALID; host-memory queries with NaN / Inf -> VDB_ERR_NONFINITE, before
 * anything is launched.  Device-memory calls are stream-ordered and read nothing back.  Takes the
 * index's shared lock and a per-search workspace, as vdb_index_search_rows does.  An empty index
 * (with an empty column attached) gives every slot "no result".  Stats (cumulative, successful
 * calls): "group_searches", "group_queries", "group_fallback_queries" (counted on the device);
 * "searches" / "queries" move once per call and the "searches_*" stats show the inner search's
 * candidate pass. */
int32_t vdb_index_set_groups(vdb_index* idx, const int32_t* groups, int64_t n, int32_t mem, void* stream);
int32_t vdb_index_search_groups(vdb_index* idx, const float* queries, int32_t n_queries, int32_t k,
                                const uint32_t* row_mask, int32_t mem,
                                float* out_scores, int64_t* out_indices, int32_t* out_groups, double* out_keys,
                                int64_t index_offset, void* stream);

/* --- MMR search: k relevant and mutually diverse rows -----------------------------
 * Replaces: nothing the reference has.  Its RAG pipeline cuts documents into chunks that overlap
 * by 50 characters and fills a fixed context with the best chunks
 * (integrations/mlx_lm_pipeline.py:646-756), so near-copies of one paragraph fill the context.
 * Maximal marginal relevance (Carbonell & Goldstein) is the usual answer; without this call a user
 * runs search(fetch_k), pulls the rows to the host one by one and builds a fetch_k x fetch_k
 * similarity matrix in numpy per query, and a device-memory caller cannot do it at all.
 *
 *   k            1..200 rows per query
 *   fetch_k      k..200 candidates per query (the most the certified fast path returns)
 *   lambda       host fp64, finite, in [0, 1]: 1 = relevance only, 0 = diversity only
 *   out_scores / out_indices / out_keys: [n_queries, k] in pick order; out_keys may be NULL
 *   out_mmr      NULL, or [n_queries, k] fp64: the value each pick won with
 *   queries, row_mask, mem, index_offset, stream: as vdb_index_search; all pointers of one memory
 *                kind.  n_queries == 0 is VDB_OK.
 * Candidates: query b's list c_0 .. c_{n-1} is what vdb_index_search(k = fetch_k, row_mask)
 * returns, the best n = min(fetch_k, eligible rows) rows by (canonical key desc, row asc); rel_i is
 * the canonical fp64 key of (q_b, c_i).  Pair similarity: S[i][j] is the canonical fp64 key of the
 * pair (stored row c_i taken as the query, stored row c_j), the same metric and operation order as
 * any key.  Both terms are in KEY units for both metrics: cosine similarity, and MINUS THE SQUARED
 * L2 distance for euclidean.  Euclidean stays in squared units on purpose: the formula then holds
 * no square root whose rounding an oracle would have to match (so lambda weighs squared distances
 * there).  S is bitwise symmetric for finite rows (products and the norm product commute,
 * (x-q)^2 == (q-x)^2), so each pair is computed once.
 * Selection, all fp64 with separate multiply and subtract: slot 0 is position 0 with mmr_0 =
 * lambda * rel_0 and pen_i = S[i][0]; every further slot computes v_i = lambda * rel_i -
 * (1.0 - lambda) * pen_i over the unpicked positions, picks the greatest (a tie goes to the lower
 * position: the better key, then the lower row id), sets mmr_t = v_pick and pen_i = (S[i][pick] >
 * pen_i) ? S[i][pick] : pen_i; it stops after min(k, n) picks.  out_indices = row id +
 * index_offset, out_keys = rel, out_scores = rel rounded as a search rounds it, out_mmr = mmr_t;
 * slots past min(k, n) hold index -1 / score 0 / key -inf / mmr -inf.
 * lambda == 1 returns, byte for byte, the first k slots of vdb_index_search(k).  The result is the
 * same bytes for every precision setting and both memory kinds: the inner search is certified
 * exact, and everything after it reads only the fp32 rows and their canonical norms.
 * How: the inner search fetches the lists into scratch; per block of max(1, 64 MiB / (fetch_k^2 *
 * 8)) queries one kernel scores the pairs i < j of each list (one wave per position i and batch of
 * four positions j) and one kernel selects (one wave per query).
 * Errors: k outside [1, 200], fetch_k outside [k, 200], lambda outside [0, 1] or NaN, n_queries
 * < 0, a NULL queries / out_scores / out_indices -> VDB_ERR_INVALID; host-memory queries with NaN /
 * Inf -> VDB_ERR_NONFINITE, before anything is launched.  Device-memory calls are stream-ordered
 * and read nothing back.  Takes the index's shared lock and a per-search workspace, as
 * vdb_index_search_groups does.  An empty index gives every slot "no result".  Stats (cumulative,
 * successful calls): "mmr_searches", "mmr_queries"; "searches" / "queries" move once per call
 * through the inner search. */
int32_t vdb_index_search_mmr(vdb_index* idx, const float* queries, int32_t n_queries,
                             int32_t k, int32_t fetch_k, double lambda,
                             const uint32_t* row_mask, int32_t mem,
                             float* out_scores, int64_t* out_indices, double* out_keys,
                             double* out_mmr, int64_t index_offset, void* stream);

/* --- recommend search: rows like stored examples ------------------------------------
 * Replaces: nothing the reference has.  Every other read takes a query VECTOR; "more like this
 * stored row", "more like these chunks and not like those" and "more like this document" take
 * stored rows (Qdrant's recommend with positive and negative ids, Pinecone's query by id, Weaviate's
 * nearObject).  Without this call a user copies each example to the host, averages in numpy in
 * whatever order it picks, searches for k + examples rows and drops the examples; the averaged
 * query has near-ties, so a last-bit difference changes the list, and a device-memory caller cannot
 * do it at all.
 *
 *   pos_offsets [n_queries + 1], pos_rows [n_pos]: query b's positive examples are
 *                pos_rows[pos_offsets[b] .. pos_offsets[b + 1]), stored row ids in [0, count) in any
 *                order (the CSR form of vdb_index_search_rows' lists).  A row may repeat and counts
 *                as often as it appears; it may stand in both lists.
 *   neg_offsets, neg_rows, n_neg: the negatives in the same form; neg_offsets == NULL with n_neg
 *                == 0: no query has negatives.
 *   n_pos, n_neg host scalars, the lengths of the id arrays: the launches are sized from them, so a
 *                device-memory call reads nothing back.
 *   A query has at most 64 examples, positives and negatives together; k is in 1..136 (200 - 64:
 *   the inner fetch of k + examples rows never leaves the certified fast path's 200).
 *   out_scores / out_indices / out_keys: [n_queries, k], written as a search writes them; out_keys
 *                may be NULL.
 *   out_queries  NULL, or [n_queries, dim] fp32: the query vectors that were built.
 *   row_mask, mem, index_offset, stream: as vdb_index_search; all pointers of one memory kind.
 *                n_queries == 0 is VDB_OK.
 * The built query, element d of query b, every operation a separate fp64 operation: acc = 0.0; for
 * the positives in list order acc = acc + e, with e = (double)x[d] for euclidean and e =
 * (double)x[d] / max(norm, 1e-8) for cosine (one fp64 divide per element by the row's canonical
 * norm, the clamp a key uses); mp = acc / (double)(number of positives); mn likewise over the
 * negatives; t = mp without negatives, else (mp + mp) - mn (Qdrant's average-vector rule); q[d] =
 * (float)t, round to nearest even.  Elements are independent: nothing depends on how they are dealt
 * to threads.
 * The result is what vdb_index_search ranks for q_b under row_mask (canonical fp64 key desc, then
 * row asc) with every row of the query's positives or negatives left out: the first k of what
 * remains, scores rounded as a search rounds them; slots past the eligible non-example rows hold
 * index -1 / score 0 / key -inf.  Examples need not be eligible under row_mask.  The result is the
 * same bytes for every precision setting and both memory kinds.  For euclidean, one positive p and
 * no negatives give, byte for byte, the first k slots of a search with row p as the query and k + 1
 * results with row p struck out, since (float)((double)x / 1.0) == x.  Cosine has no such identity:
 * its query is the normalised row rounded to fp32, not the row.
 * Queries answered with every slot "no result" (out_queries holds zeros for them): (1) a query
 * without a positive example, which is no error in either memory kind; (2) a query whose built
 * vector has a non-finite element (euclidean rows above about 1.1e38 only); (3) on a device-memory
 * call, which is not validated: a query with an id outside [0, count) or more than 64 examples
 * (offsets are clamped to [0, n_pos] / [0, n_neg] and nothing out of bounds is read).  (2) and (3)
 * are counted on the device in stat "recommend_bad_queries".
 * How: one kernel builds the queries (one workgroup per query, a thread per 256th element, the
 * examples walked in order), the inner search fetches k' = k + E rows (host memory: E = the largest
 * example count of the call; device memory: min(64, n_pos + n_neg)), one kernel drops the examples
 * in order (one wave per query).
 * Errors, host-memory calls, before anything is launched: k outside [1, 136], n_queries < 0, a NULL
 * pos_offsets / out_scores / out_indices with n_queries > 0, neg_offsets NULL with n_neg != 0,
 * offsets that decrease or pass their n_pos / n_neg, an id outside [0, count), a query with more
 * than 64 examples, a bad mem -> VDB_ERR_INVALID (no stat moves).  There are no caller vectors, so
 * no VDB_ERR_NONFINITE.  An empty index with empty lists gives every slot "no result".  Takes the
 * index's shared lock and a per-search workspace, as vdb_index_search_mmr does.  Stats (cumulative,
 * successful calls): "recommend_searches", "recommend_queries", "recommend_bad_queries";
 * "searches" / "queries" move once per call through the inner search. */
int32_t vdb_index_search_recommend(vdb_index* idx, int32_t n_queries, int32_t k,
                                   const int64_t* pos_offsets, const int64_t* pos_rows, int64_t n_pos,
                                   const int64_t* neg_offsets, const int64_t* neg_rows, int64_t n_neg,
                                   const uint32_t* row_mask, int32_t mem,
                                   float* out_scores, int64_t* out_indices, double* out_keys, float* out_queries,
                                   int64_t index_offset, void* stream);

/* --- fused search: one ranked list from several query vectors ----------------------
 * Replaces: nothing the reference has.  Its RAG pipeline retrieves with one embedding of the
 * question (integrations/mlx_lm_pipeline.py); the usual next step is several per question
 * (paraphrases, the question plus a hypothetical answer, a title and a body embedding) answered
 * with one list, as Milvus' hybrid_search with RRFRanker, Qdrant's prefetch + fusion and LangChain's
 * EnsembleRetriever do.  Without this call a user runs a batch search, pulls the lists to the host
 * and adds reciprocal ranks in a dict: the sums tie exactly all the time, so the order depends on
 * an unstated tie rule, and a device-memory caller cannot do it at all.
 *
 *   queries      [n_sub, dim] fp32: the sub-queries of all sets, back to back
 *   set_offsets  [n_sets + 1] int64, CSR as vdb_index_search_rows' lists: set s is sub-queries
 *                [set_offsets[s], set_offsets[s + 1]).  A set has 0..16 sub-queries; one without
 *                any is no error, all its slots are "no result".
 *   n_sub        host scalar: the launches are sized from it, so a device-memory call reads nothing
 *                back
 *   weights      NULL, or [n_sub] fp64, one per sub-query, finite and >= 0.  NULL is 1.0 for RRF; it
 *                must be NULL for VDB_FUSE_MAX.
 *   k, fetch_k   1 <= k <= fetch_k <= 200 (the most the certified fast path returns, as for MMR)
 *   fusion       VDB_FUSE_RRF or VDB_FUSE_MAX
 *   rrf_c        host fp64, finite and >= 0 (customarily 60); ignored for MAX
 *   out_scores / out_indices: [n_sets, k]; out_fused: NULL or [n_sets, k] fp64; out_hits: NULL or
 *                [n_sets, k] int32
 *   row_mask, mem, index_offset, stream: as vdb_index_search; all pointers of one memory kind.
 *                n_sets == 0 is VDB_OK.
 * Lists: list l of a set (l counted within the set, in sub-query order) is what vdb_index_search(k
 * = fetch_k, row_mask) returns for that sub-query: rows c_{l,0} .. c_{l,n_l-1} by (canonical key
 * desc, row asc) with keys kappa_{l,p}, n_l = min(fetch_k, eligible rows).  The candidates of a set
 * are the union of its lists' rows; hits(r) is the number of lists holding r.
 * RRF: fused(r) in fp64, every operation separate: acc = 0.0; for l ascending, if r stands in list l
 * at position p: t = rrf_c + (double)(p + 1); u = w_l / t; acc = acc + u.
 * MAX: fused(r) starts as the kappa of the first list (lowest l) holding r; for every later holding
 * list fused = (kappa > fused) ? kappa : fused (this form and not fmax, so that the sign of a zero
 * cannot differ between device and oracle).
 * Ranking: candidates by (fused desc, row id asc); the first min(k, candidates) are written:
 * out_indices = row id + index_offset, out_fused = fused, out_hits = hits, out_scores = (float)fused
 * (round to nearest even) for RRF and, for MAX, the inner search's fp32 score at the list entry that
 * holds the maximum (equal keys have equal scores, so which entry does not matter).  Slots past that
 * hold index -1 / score 0 / fused -inf / hits 0.
 * MAX is exact over the corpus: with fetch_k >= k the result is the top k of max_l key(q_l, r) over
 * all eligible rows.  Take a row r of that top k and the list l where it attains its maximum: every
 * row ahead of r in list l has a key there not below r's maximum, so its own maximum is not below
 * r's, and at equality its row id is lower; so it is ahead of r in the fused order too.  Fewer than
 * k rows are ahead of r in the fused order, hence fewer than k in that list: r is in the list.
 * Consequences: a set of one sub-query under MAX with fetch_k == k returns, byte for byte,
 * vdb_index_search(k) with out_fused = its out_keys.  The result of a set depends only on its own
 * sub-queries.  The result is the same bytes for every precision setting and both memory kinds: the
 * inner search is certified exact, and the fusion reads only its lists.
 * How: the inner search fetches the lists of all n_sub sub-queries into scratch; one kernel, one
 * workgroup per set, sorts the set's <= 3 200 list entries by (row, list) in LDS, lets the thread at
 * the head of each row's run add that row's terms in list order, and sorts the candidates by (fused
 * desc, row asc).  No sum depends on arrival order.
 * Errors, before anything is launched, both memory kinds: k outside [1, 200], fetch_k outside [k,
 * 200], an unknown fusion, rrf_c NaN / infinite / negative (RRF), a bad mem, n_sub or n_sets < 0, a
 * NULL queries with n_sub > 0, a NULL set_offsets / out_scores / out_indices with n_sets > 0,
 * weights with MAX -> VDB_ERR_INVALID.  Host-memory calls also: offsets that decrease or pass
 * n_sub, a set of more than 16, a weight that is NaN, infinite or negative -> VDB_ERR_INVALID; a NaN
 * or Inf in a query -> VDB_ERR_NONFINITE (no stat moves).  Device-memory calls are stream-ordered
 * and read nothing back, so the kernel handles bad input itself: offsets are clamped to [0, n_sub]
 * and nothing out of bounds is read; a set whose offsets decrease or lie outside [0, n_sub], that is
 * longer than 16 or has a bad weight is answered with all slots "no result" and counted on the
 * device in stat "fused_bad_sets"; the other sets of the call are unaffected.
 * Takes the index's shared lock and a per-search workspace, as vdb_index_search_mmr does.  An empty
 * index gives every slot "no result".  Stats (cumulative, successful calls): "fused_searches",
 * "fused_sets", "fused_bad_sets"; "searches" / "queries" (+ n_sub) move once per call through the
 * inner search. */
enum { VDB_FUSE_RRF = 0, VDB_FUSE_MAX = 1 };
int32_t vdb_index_search_fused(vdb_index* idx, const float* queries, int32_t n_sub,
                               const int64_t* set_offsets, int32_t n_sets, const double* weights,
                               int32_t k, int32_t fetch_k, int32_t fusion, double rrf_c,
                               const uint32_t* row_mask, int32_t mem,
                               float* out_scores, int64_t* out_indices, double* out_fused, int32_t* out_hits,
                               int64_t index_offset, void* stream);

/* --- Hybrid search: a sparse vector per row, exact sparse top-k, RRF with dense ------
 * Replaces: nothing the reference has.  The models of vdb_index_search_fused (Milvus' hybrid_search
 * with RRFRanker, Qdrant's prefetch + fusion, LangChain's EnsembleRetriever) are mostly used to fuse
 * a dense retriever with a sparse, lexical one (BM25, SPLADE or BGE-M3 term weights).  These three
 * calls hold a sparse vector per row, rank by it exactly, and fuse that ranking with the dense one on
 * the device.  Weighting (BM25 itself) is the caller's: the store keeps the weights it is given.
 *
 * vdb_index_set_sparse attaches one sparse vector per stored row, in CSR form: row r's entries are
 * [indptr[r], indptr[r + 1]) of terms (int32) / weights (fp32).  Required, else VDB_ERR_INVALID (a NaN
 * or Inf weight: VDB_ERR_NONFINITE): n == count; indptr ascending from 0 to nnz; term ids in [0,
 * n_terms) and strictly ascending within a row; 1 <= n_terms <= 2^31 - 1.  A row without entries is
 * valid.  indptr == NULL with n == 0 detaches the column.  Validation runs before the column is
 * replaced (a device-memory call: by a kernel, one flag word read back); on any error the column
 * attached before stays exactly as it was.  The call takes the exclusive lock, waits for queued
 * searches, copies the column (the caller's arrays may be reused on return) and returns when done.
 * Every successful add, remove and clear drops the column; vdb_index_update keeps it; it and the group
 * column are independent.  The device copy interleaves (term, weight) as 8-byte pairs.  Stats:
 * "sparse_rows" (rows attached, 0 = none), "sparse_nnz", "sparse_sets" (cumulative).
 *
 * vdb_index_search_sparse: the k best rows of each sparse query.
 *   q_indptr     [n_queries + 1] int64, q_terms / q_weights [q_nnz]: the queries in CSR form.  A query
 *                has at most 1 024 terms, ids strictly ascending in [0, n_terms), weights finite.
 *   q_nnz        host scalar, so a device-memory call reads nothing back
 *   k            1..1024
 *   out_scores   [n_queries, k] fp32; out_indices [n_queries, k] int64; out_keys NULL or fp64
 *   row_mask, mem, index_offset, stream: as vdb_index_search_rows; all pointers of one memory kind.
 * Contract (every operation a separate fp64 operation): qd[t] = the query's weight for term t as a
 * double, 0.0 for a term it does not list.  For row r: acc = 0.0; for the row's entries e in stored
 * order acc = acc + (double)w_e * qd[t_e]; the sum is the key.  Row r matches when some entry has w_e
 * != 0 and qd[t_e] != 0.  Candidates: the matching rows whose mask bit is set (a row that matches
 * nothing is never returned, whatever its key).  Ranking by (key desc, row asc); the first min(k,
 * candidates) are written: out_indices = row + index_offset, out_keys = key, out_scores = (float)key
 * (round to nearest even).  Slots past that hold index -1 / score 0 / key -inf.  The key is a dot
 * product whatever the index's metric; the result is the same bytes for every precision setting and
 * both memory kinds (the dense rows and the candidate copies are not read).
 * Errors, before anything is launched, both memory kinds: no sparse column attached, k outside [1,
 * 1024], n_queries or q_nnz < 0, a NULL q_indptr / out_scores / out_indices with n_queries > 0, a bad
 * mem -> VDB_ERR_INVALID.  Host-memory calls also: offsets that decrease or pass q_nnz, a query of
 * more than 1 024 terms, a term id out of range or not above its predecessor -> VDB_ERR_INVALID; a
 * NaN or Inf weight -> VDB_ERR_NONFINITE (no stat moves).  Device-memory calls are stream-ordered and
 * read nothing back, so the kernel takes any input: offsets are clamped to [0, q_nnz] and nothing out
 * of bounds is read; a query whose offsets the clamp changed or that decrease, that is too long or
 * holds a bad term id or a non-finite weight is answered with all slots "no result" and counted on
 * the device in stat "sparse_bad_queries"; the other queries are unaffected.  n_queries == 0 is
 * VDB_OK; a query without terms is no error (all its slots "no result"); an empty index with an empty
 * column attached gives "no result" everywhere.  Takes the shared lock and a per-search workspace, as
 * vdb_index_search_rows does.  Knob "sparse_wgs": workgroups per query, 0 = auto (results identical).
 * Stats: "sparse_searches", "sparse_queries", "sparse_bad_queries"; "searches" / "queries" and every
 * "searches_*" stat stay still.
 *
 * vdb_index_search_hybrid: query b is the fused-search set whose list 0 is what vdb_index_search
 * returns for queries[b] with k = fetch_k and row_mask, whose list 1 is what vdb_index_search_sparse
 * returns for sparse query b with k = fetch_k and row_mask, whose weights are (w_dense, w_sparse) and
 * whose fusion is VDB_FUSE_RRF with rrf_c; the outputs are as vdb_index_search_fused defines them
 * (out_hits 1 or 2; ties to the lower row).  1 <= k <= fetch_k <= 200; w_dense, w_sparse and rrf_c
 * finite and >= 0; out_fused and out_hits may be NULL.  With w_sparse == 0 the first k rows are those
 * of the dense search, in its order; a query with no sparse terms, or with none matching, ranks by its
 * dense list alone.  Same bytes for every precision setting and both memory kinds.  Errors: those of
 * the two inner calls and those checks, before anything is launched; a device-memory query the sparse
 * kernel finds bad contributes an empty sparse list (counted in "sparse_bad_queries") and its dense
 * list still ranks.  Stats: "hybrid_searches", "hybrid_queries"; "searches" / "queries" move once per
 * call through the inner dense search; "sparse_searches" / "sparse_queries" stay still. */
int32_t vdb_index_set_sparse(vdb_index* idx, const int64_t* indptr, const int32_t* terms, const float* weights,
                             int64_t n, int64_t nnz, int32_t n_terms, int32_t mem, void* stream);
int32_t vdb_index_search_sparse(vdb_index* idx, const int64_t* q_indptr, const int32_t* q_terms, const float* q_weights,
                                int32_t n_queries, int64_t q_nnz, int32_t k,
                                const uint32_t* row_mask, int32_t mem,
                                float* out_scores, int64_t* out_indices, double* out_keys,
                                int64_t index_offset, void* stream);
int32_t vdb_index_search_hybrid(vdb_index* idx, const float* queries,
                                const int64_t* q_indptr, const int32_t* q_terms, const float* q_weights,
                                int32_t n_queries, int64_t q_nnz,
                                int32_t k, int32_t fetch_k, double w_dense, double w_sparse, double rrf_c,
                                const uint32_t* row_mask, int32_t mem,
                                float* out_scores, int64_t* out_indices, double* out_fused, int32_t* out_hits,
                                int64_t index_offset, void* stream);

/* --- Weighted-sum hybrid search: exact top-k of dense plus sparse scores -------------
 * Replaces: nothing the reference has.  Beside reciprocal-rank fusion, the systems
 * vdb_index_search_hybrid was modelled on offer a weighted sum of the two scores (Pinecone's
 * sparse-dense alpha, Milvus' WeightedRanker, Elasticsearch's linear retriever, Weaviate's score
 * fusion).  They add the scores of two fetched lists, where a row missing from one list counts 0
 * there: a row that stands 250th in both rankings can have the best sum and stands in neither list.
 * This call computes the sum for every row of the corpus and returns its exact top k.
 *
 *   queries      [n_queries, dim] fp32: the dense query vectors
 *   q_indptr     [n_queries + 1] int64, q_terms / q_weights [q_nnz]: the sparse queries in CSR form,
 *                as vdb_index_search_sparse takes them; q_nnz a host scalar
 *   k            1..1024; n_queries at most 65 535
 *   w_dense, w_sparse  finite, >= 0 and <= 2^64 (the cap keeps every product finite: |kd| and |ks|
 *                are below 2^280 for any finite fp32 input, so no sum is inf - inf)
 *   out_scores   [n_queries, k] fp32; out_indices [n_queries, k] int64; out_fused, out_dense,
 *                out_sparse NULL or [n_queries, k] fp64
 *   row_mask, mem, index_offset, stream: as vdb_index_search_hybrid; all pointers of one memory kind.
 * Contract (every operation a separate fp64 operation).  For query b and row r: kd = the canonical
 * fp64 key vdb_index_search ranks by (the cosine similarity, or minus the squared L2 distance; it
 * stays in key units, as MMR's and MaxSim's do); ks = the key vdb_index_search_sparse's contract
 * defines (acc = 0.0, then over the row's entries in stored order acc = acc + (double)w_e * qd[t_e]):
 * +0.0 for a row that shares no term with the query, and never -0.0.  t1 = w_dense * kd; t2 =
 * w_sparse * ks; u = t1 + t2; c = u + 0.0 (the last add turns -0.0 into +0.0, as MaxSim's, so equal
 * values have equal bits).  Candidates: EVERY row below count whose mask bit is set, whether it
 * shares a term with the query or not (unlike vdb_index_search_sparse, on purpose: an unmatched row
 * still has its dense score).  Ranking by (c desc, row asc); the first min(k, candidates) slots hold
 * out_indices = row + index_offset, out_fused = c, out_scores = (float)c (round to nearest even),
 * out_dense = kd, out_sparse = ks.  Slots past that hold index -1 / score 0 / fused, dense and sparse
 * -inf.
 * Consequences: with w_dense == 1 and w_sparse == 0 the indices are those of vdb_index_search(k,
 * row_mask) in its order and out_fused has the bits of its out_keys + 0.0.  A query without terms
 * ranks by its dense key alone; that is no error.  With w_dense == 0 and w_sparse == 1 the leading
 * slots whose out_sparse is > 0 are the leading slots of vdb_index_search_sparse(k) with keys > 0:
 * same rows, same order, out_fused == its out_keys.  The result of a query depends only on that
 * query.  The result is the same bytes for every precision setting and both memory kinds: only the
 * fp32 rows, their canonical norms and the sparse column are read.
 * Errors, before anything is launched, both memory kinds, all VDB_ERR_INVALID: those of
 * vdb_index_search_sparse's call checks (no sparse column attached, k outside [1, 1024], n_queries or
 * q_nnz < 0, a NULL q_indptr / out_scores / out_indices with n_queries > 0, a bad mem), a NULL
 * queries with n_queries > 0, a weight outside [0, 2^64] or NaN, n_queries above 65 535.
 * Host-memory calls also: the sparse queries are checked as vdb_index_search_sparse checks them, and
 * a NaN or Inf in a dense query -> VDB_ERR_NONFINITE; no stat moves on an error.  Device-memory calls
 * are stream-ordered and read nothing back: sparse offsets are clamped to [0, q_nnz] as the sparse
 * kernel clamps them; a query it finds bad by vdb_index_search_sparse's rule gets "no result" in
 * every slot and is counted in "sparse_bad_queries", its neighbours unaffected; a non-finite dense
 * query is the caller's error, as for vdb_index_search_rows (nothing out of bounds is read).
 * n_queries == 0 is VDB_OK; an empty index with an empty column attached gives "no result"
 * everywhere.  Takes the shared lock and a per-search workspace, with one pinned staging copy each
 * way for host calls, as vdb_index_search_sparse does.  Knob "hybrid_sum_wgs": workgroups per query,
 * 0 = auto, 1..512 (results identical).  Stats: "hybrid_sum_searches", "hybrid_sum_queries"
 * (cumulative over successful calls); "searches", "queries" and every "searches_*" stat stay still. */
int32_t vdb_index_search_hybrid_sum(vdb_index* idx, const float* queries,
                                    const int64_t* q_indptr, const int32_t* q_terms, const float* q_weights,
                                    int32_t n_queries, int64_t q_nnz, int32_t k,
                                    double w_dense, double w_sparse,
                                    const uint32_t* row_mask, int32_t mem,
                                    float* out_scores, int64_t* out_indices, double* out_fused,
                                    double* out_dense, double* out_sparse,
                                    int64_t index_offset, void* stream);

/* --- filter operators: numeric columns and predicate masks on the device -------------
 * Replaces: nothing the reference has.  Its filter is `meta.get(key) == value` alone
 * (service/optimized_vector_store.py:159-165); range filters ("timestamp >= t", "price between a
 * and b") are what Qdrant, Milvus, Pinecone, Weaviate and Chroma offer beside equality.  A range
 * bound usually differs per request, so a cached bitmap never hits: these two calls build the
 * row_mask of such a filter on the device, from fp64 columns the index holds, for every search call
 * that takes a row_mask.
 *
 * vdb_index_set_column attaches one fp64 value per stored row to `slot` (16 slots, 0..15): values
 * [n], n == count (else VDB_ERR_INVALID).  NaN = the row has no value; +-inf and +-0 are ordinary
 * values, so nothing is validated.  NULL with n == 0 detaches the slot.  It takes the exclusive
 * lock, waits for queued searches, copies and returns when done, as vdb_index_set_groups does;
 * device memory is read after the work queued on `stream`.  Every successful add, remove and clear
 * drops all slots; vdb_index_update keeps them.  The slots are independent of the group and sparse
 * columns.  Stats: "column_slots" (bitmask of the attached slots), "column_sets" (cumulative);
 * "device_bytes" includes the columns.
 *
 * vdb_index_filter_mask evaluates n_preds predicates in one launch.  Predicate p is the AND of the
 * clauses [pred_offsets[p], pred_offsets[p + 1]): 0 <= n_preds <= 256, at most 8 clauses per
 * predicate, offsets ascending from 0.  For a row whose value in the clause's column is v:
 *     has = !(v != v)
 *     t   = has && (LO_INCL ? v >= lo : v > lo) && (HI_INCL ? v <= hi : v < hi)
 *     the clause holds iff  NEGATE ? !t : t
 * so a row without a value fails every plain clause and passes every negated one (MongoDB's $ne).
 * Equality is [x, x] with both bounds inclusive, "exists" [-inf, +inf] with both inclusive; a
 * predicate without clauses passes every row.  All compares are plain IEEE fp64 (-0.0 == +0.0, no
 * rounding): the answer is a set, the same as a numpy restatement bit for bit.
 *
 *   clauses, pred_offsets  HOST memory always, whatever `mem` says (a few KB): fully validated
 *                before anything is launched and copied into the call's workspace staging before
 *                the call returns
 *   mem          the memory kind of base_masks, out_masks and out_counts
 *   base_masks   NULL or [n_preds][W] uint32, W = ceil(count / 32), the row_mask layout
 *   out_masks    [n_preds][W]: bit r of predicate p is set iff r < count, the predicate holds and
 *                the bit of base_masks[p] is set; bits at or past count in the last word are
 *                written as 0; nothing at or past n_preds * W words is written.  Only 4-byte
 *                alignment is required.  May not alias base_masks.
 *   out_counts   NULL or [n_preds] int64: the exact number of bits set
 *
 * Device-memory calls are stream-ordered and read nothing back, so an output mask can be the
 * row_mask of a device search queued behind it on the same stream.  Host-memory calls take a
 * per-search workspace, its stream and pinned staging, as vdb_index_search_range does, and return
 * with the results in host memory.  Takes the shared lock.  An empty index gives W = 0, counts 0
 * and VDB_OK.  Errors, all VDB_ERR_INVALID, no stat moves on any: a slot outside 0..15 or one not
 * attached, unknown flag bits, a NaN bound, more than 8 clauses in a predicate, n_preds outside
 * 0..256, offsets that decrease or do not start at 0, a NULL out_masks with n_preds > 0 and
 * count > 0, a bad mem.  Stats: "filter_calls", "filter_preds" (cumulative over successful calls);
 * "searches", "queries" and every "searches_*" stat stay still. */
enum { VDB_FILTER_LO_INCL = 1, VDB_FILTER_HI_INCL = 2, VDB_FILTER_NEGATE = 4 };
typedef struct { int32_t column; int32_t flags; double lo; double hi; } vdb_filter_clause;
int32_t vdb_index_set_column(vdb_index* idx, int32_t slot, const double* values, int64_t n,
                             int32_t mem, void* stream);
int32_t vdb_index_filter_mask(vdb_index* idx, const vdb_filter_clause* clauses, const int32_t* pred_offsets,
                              int32_t n_preds, const uint32_t* base_masks, int32_t mem,
                              uint32_t* out_masks, int64_t* out_counts, void* stream);

/* --- MaxSim search: groups ranked by the summed best match per query vector ---------
 * Replaces: nothing the reference has.  Multi-vector ("late interaction") retrieval -- ColBERT /
 * ColPali token embeddings, Qdrant's multivector MAX_SIM, Vespa's and Milvus' MaxSim -- scores a
 * document by  sum over the query's vectors t of  max over the document's rows r of sim(q_t, r).
 * A document is a group of the column vdb_index_set_groups attached.  No other call gives this
 * answer: vdb_index_search_groups ranks by one vector's best row, VDB_FUSE_MAX takes the maximum
 * over vectors, and summing over-fetched per-vector lists on the host is wrong (a document that is
 * second best for every vector stands in no list and can still have the best sum).
 *
 *   queries      [n_sub, dim] fp32: the sub-queries of all sets, back to back
 *   set_offsets  [n_sets + 1] int64, CSR as vdb_index_search_fused's: set s is sub-queries
 *                [set_offsets[s], set_offsets[s + 1]).  A set has 0..64 sub-queries; one without
 *                any is no error, all its slots are "no result".
 *   n_sub        host scalar: the launches are sized from it, so a device-memory call reads nothing
 *                back
 *   n_group_slots  host scalar: the caller states that the attached group ids lie in
 *                [0, n_group_slots); the launches and the scratch are sized from it.  1 <=
 *                n_group_slots and n_sub * n_group_slots <= 2^27 (a 1 GiB table).  A row whose id is
 *                at or past it is treated as a row without a group and counted in stat
 *                "maxsim_skipped_rows" (both memory kinds: the column lives on the device).
 *   k            1..128
 *   out_scores   [n_sets, k] fp32; out_groups [n_sets, k] int32; out_sums NULL or [n_sets, k] fp64
 *   row_mask, mem, stream: as vdb_index_search_groups; all pointers of one memory kind.
 *                n_sets == 0 is VDB_OK.
 * Contract: a row r is eligible when 0 <= group[r] < n_group_slots and its mask bit is set.  For
 * sub-query t and group g, m[t][g] = the maximum over g's eligible rows r of (key(q_t, r) + 0.0),
 * key the canonical fp64 key vdb_index_search ranks by; the one fp64 add turns -0.0 (the euclidean
 * key of an exact match) into +0.0, so equal values have equal bits and the maximum of a set of
 * values is one bit pattern in whatever order it is formed.  sum[s][g]: acc = 0.0, then for t
 * ascending within the set acc = acc + m[t][g], separate fp64 adds.  A group without an eligible row
 * is no candidate (eligibility does not depend on t, so a candidate has all its maxima).  Ranking:
 * candidates by (sum desc, group id asc); the first min(k, candidates) are written: out_groups = the
 * id, out_sums = sum, out_scores = (float)sum (round to nearest even), in key units for both
 * metrics (euclidean: minus the summed squared distances, as MMR's stay in key units).  Slots past
 * that hold group -1 / score 0 / sum -inf.
 * Consequences: a set of one sub-query gives, per group, the key vdb_index_search_groups returns
 * for that group (+ 0.0), in the same order.  The result of a set depends only on its own
 * sub-queries.  The result is the same bytes for every precision setting and both memory kinds: the
 * rows come from the fp32 copy and the candidate copies are not read.
 * How: a table T [n_sub][n_group_slots] of order-preserving uint64 encodings, zeroed per call; one
 * scan of the rows per block of up to 64 sub-queries (the shape of the range scan) folds runs of
 * rows of one group in registers and issues one 64-bit atomic maximum per (wave, sub-query, run);
 * one rank kernel sums each set's entries in sub-query order and keeps the best k.  A maximum does
 * not depend on arrival order; no sum is formed by an atomic.
 * Errors, before anything is launched, both memory kinds: no group column attached, k outside [1,
 * 128], n_group_slots < 1 or the table above 2^27 entries, n_sub or n_sets < 0, a NULL queries with
 * n_sub > 0, a NULL set_offsets / out_scores / out_groups with n_sets > 0, a bad mem ->
 * VDB_ERR_INVALID.  Host-memory calls also: offsets that decrease or pass n_sub, a set of more than
 * 64 -> VDB_ERR_INVALID; a NaN or Inf in a query -> VDB_ERR_NONFINITE (no stat moves).
 * Device-memory calls are stream-ordered and read nothing back, so the kernel handles bad input
 * itself: offsets are clamped to [0, n_sub] and nothing out of bounds is read; a set whose offsets
 * decrease or lie outside [0, n_sub] or that is longer than 64 is answered with all slots "no
 * result" and counted on the device in stat "maxsim_bad_sets"; the other sets are unaffected.
 * Takes the index's shared lock and a per-search workspace, as vdb_index_search_groups does.  An
 * empty index with an empty column attached gives every slot "no result".  Stats (cumulative,
 * successful calls): "maxsim_searches", "maxsim_sets", "maxsim_bad_sets", "maxsim_skipped_rows"
 * (rows, masked or not, with an id at or past n_group_slots, counted while the call's first block of
 * sub-queries is scanned: once per call that scans).  "searches" / "queries" and every "searches_*"
 * stat stay still. */
int32_t vdb_index_search_maxsim(vdb_index* idx, const float* queries, int32_t n_sub,
                                const int64_t* set_offsets, int32_t n_sets,
                                int32_t n_group_slots, int32_t k,
                                const uint32_t* row_mask, int32_t mem,
                                float* out_scores, int32_t* out_groups, double* out_sums,
                                void* stream);

/* --- multi-GPU merge -----------------------------------------------------------
 * Merge per-shard top-k lists (all device memory, already all-gathered):
 *   keys [n_lists, n_queries, k_in] fp64 ranking keys (higher first),
 *   idx  [n_lists, n_queries, k_in] int64 global row ids (-1 = empty)
 * into the global top-k_out per query, ordered by (key desc, index asc) —
 * bit-identical to a single-GPU search.  No reference counterpart (the
 * reference is single device); SURVEY.md §8e. */
int32_t vdb_merge_topk(const double* keys, const int64_t* idx, int32_t n_lists, int32_t n_queries,
                       int32_t k_in, int32_t k_out, int32_t metric,
                       float* out_scores, int64_t* out_indices, double* out_keys, void* stream);

/* --- stateless operator slot ---------------------------------------------------
 * The reference's similarity functions themselves, returning every score
 * (no top-k): `_compiled_cosine_similarity` / `_compiled_euclidean_distance`
 * (service/optimized_vector_store.py:31-48) for n_queries = 1,
 * `compute_cosine_similarity_batch` (performance/mlx_optimized.py:59-88) for
 * n_queries > 1, and `compute_dot_product` (mlx_optimized.py:150-156, metric
 * VDB_METRIC_DOT).  All pointers are device memory: corpus [n, dim] row-major
 * fp32, queries [n_queries, dim], out [n_queries, n] fp32.  cosine / dot: an fp32
 * MFMA GEMM over LDS-staged tiles with the norms applied in the epilogue;
 * euclidean: direct differences (the reference's form).  Within 1e-4 of the
 * reference's fp32 arithmetic. */
int32_t vdb_similarity_matrix(const float* corpus, int64_t n, int32_t dim,
                              const float* queries, int32_t n_queries, int32_t metric,
                              float* out, void* stream);
/* `normalize_vectors` (performance/mlx_optimized.py:110-125): out = x / max(|x|, 1e-8)
 * per row; device memory, in == out allowed. */
int32_t vdb_normalize_rows(const float* in, int64_t n, int32_t dim, float* out, void* stream);
/* `fast_top_k_indices` / `mx.argsort(-scores)[:k]` (mlx_optimized.py:90-108,
 * optimized_vector_store.py:176-183) over `rows` score rows of length n (device
 * memory): the k best per row, largest first (largest = 1) or smallest first.  The
 * key is s when largest, otherwise -s, with NaN mapped to -inf; order is key
 * descending, index ascending.  So ties go to the lower index (-0.0 and +0.0 tie),
 * and NaN ties with the worst infinity and is ordered against it by index.
 * out_indices [rows, k] int64; out_values NULL or [rows, k] fp32, the raw scores at
 * the returned indices.  1 <= k <= min(n, 1024). */
int32_t vdb_topk_scores(const float* scores, int32_t rows, int64_t n, int32_t k, int32_t largest,
                        int64_t* out_indices, float* out_values, void* stream);

/* --- graph index (the HNSW path) -------------------------------------------------
 * Replaces ProductionHNSWIndex (performance/hnsw_index.py:23-129: hnswlib
 * build / knn_query / save / load), re-laid out for the GPU: one
 * level of out-degree `degree` (hnswlib's level-0 degree 2M) as a [N][degree]
 * int32 neighbour array, built from the exact kNN of every row (the brute-force
 * path above, `knn` neighbours) as the degree/2 nearest out-edges plus the nearest
 * reverse edges; searches start from the best of `n_entries` spread rows.  The
 * graph refers to the index's rows; adding rows makes it stale (search errors). */
typedef struct vdb_graph vdb_graph;

int32_t vdb_graph_build(vdb_index* idx, int32_t degree, int32_t knn, int32_t n_entries, vdb_graph** out);
/* Persistence: a graph exported by vdb_graph_export (neighbours [n][degree], -1 =
 * none; entry rows) re-attached to an index holding the same rows.  The entry rows must be
 * distinct: a repeated entry row is refused (VDB_ERR_INVALID), as is any id out of range. */
int32_t vdb_graph_import(vdb_index* idx, int32_t degree, int64_t n, const int32_t* nbr, int32_t n_entries,
                         const int32_t* entries, vdb_graph** out);
int32_t vdb_graph_export(const vdb_graph* g, int32_t* nbr_host, int32_t* entries_host);
/* Incremental maintenance (replaces the rebuild per add of
 * service/optimized_vector_store.py:110-112): inserts the rows the index gained since the
 * graph was built or last extended (exact kNN of the new rows, hnswlib's heuristic for their
 * out-edges, re-selection of every list that gains an in-edge).  A graph must be extended
 * before it is searched again after its index grew (vdb_graph_search reports it stale). */
int32_t vdb_graph_add(vdb_graph* g);
int32_t vdb_graph_info(const vdb_graph* g, int64_t* n_rows, int32_t* degree, int32_t* n_entries);
/* hnswlib knn_query semantics (hnsw_index.py:98-101): labels [n_queries, k] int64
 * (-1 = none), distances [n_queries, k] fp32: cosine 1 - cos, euclidean squared L2;
 * best first.  ef = beam width (search depth), k <= ef <= 256. */
int32_t vdb_graph_search(vdb_graph* g, const float* queries, int32_t n_queries, int32_t k, int32_t ef, int32_t mem,
                         int64_t* labels, float* distances, void* stream);
/* stats: "queries", "iterations" (beam iterations, summed over queries and teams),
 * "visited" (rows scored, summed) */
int32_t vdb_graph_stat(const vdb_graph* g, const char* name, int64_t* value);
/* Graph search knobs: "teams" (1..256, at most the entry rows; default 1): workgroups per query, each
 * searching from a disjoint slice of the entry rows (entry rank r -> team r mod
 * teams) with its own beam of `ef`, merged into the top k distinct rows.  At
 * batch 1 it puts several CUs on the query: more of the graph explored (higher
 * recall) in about the same latency.  Replaces: nothing in hnswlib (its search
 * is single-threaded per query). */
int32_t vdb_graph_set_param(vdb_graph* g, const char* name, int64_t value);

int32_t vdb_graph_destroy(vdb_graph* g);

/* --- multi-device corpus (one process, several GPUs) ------------------------------
 * The store's corpus row-sharded over `n_devices` GPUs of this process (SURVEY.md §8e;
 * the reference serves from one process, main.py:395, with the corpus on one device,
 * service/optimized_vector_store.py:59-114).  Rows keep their global ids (insertion
 * order); each add is cut into contiguous pieces that level the shard sizes.  A search
 * runs on every shard at once (one stream each, device-resident top-k with exact fp64
 * keys and global ids), gathers the G lists to devices[0] by peer copies over xGMI and
 * merges them there by (key desc, row asc): results identical to vdb_index_search on
 * one index holding every row.  Host memory in and out.  A device may repeat. */
typedef struct vdb_shards vdb_shards;
int32_t vdb_shards_create(int32_t dim, int32_t metric, const int32_t* devices, int32_t n_devices, vdb_shards** out);
int32_t vdb_shards_destroy(vdb_shards* s);
int32_t vdb_shards_add(vdb_shards* s, const float* vectors_host, int64_t n);
int32_t vdb_shards_count(const vdb_shards* s, int64_t* n);
int32_t vdb_shards_shard_count(const vdb_shards* s, int32_t shard, int64_t* n);
/* row_mask: NULL or ceil(count/32) host words over GLOBAL rows (as vdb_index_search) */
int32_t vdb_shards_search(vdb_shards* s, const float* queries_host, int32_t n_queries, int32_t k,
                          const uint32_t* row_mask, float* out_scores, int64_t* out_indices, double* out_keys);
/* Stream-ordered form (no host wait): queries [n_queries, dim], row_mask (NULL or
 * ceil(count/32) words over GLOBAL rows) and the outputs are device memory on devices[0];
 * the search is ordered after the work queued on `stream` (a stream of devices[0], NULL = its
 * null stream) and the outputs are ready when `stream` reaches the merge, so batches can be
 * queued back to back.  Per shard: peer copies of the queries (and the mask, whose shard-local
 * bitmap is built on the shard's device), the shard's device search, a peer copy of its lists
 * to devices[0]; the merge runs on `stream`.  vdb_shards_search is the host-memory form of
 * the same path.  Reference constraint: one process serving every device (main.py:395). */
int32_t vdb_shards_search_device(vdb_shards* s, const float* queries, int32_t n_queries, int32_t k,
                                 const uint32_t* row_mask, float* out_scores, int64_t* out_indices,
                                 double* out_keys, void* stream);
int32_t vdb_shards_get_vectors(vdb_shards* s, int64_t start, int64_t n, float* out_host);
int32_t vdb_shards_clear(vdb_shards* s);
int32_t vdb_shards_reserve(vdb_shards* s, int64_t rows);
/* applied to every shard's index (vdb_index_set_param names) */
int32_t vdb_shards_set_param(vdb_shards* s, const char* name, int64_t value);
/* "count", "shards", else the vdb_index_get_stat name summed over the shards */
int32_t vdb_shards_get_stat(const vdb_shards* s, const char* name, int64_t* value);

/* --- lifecycle ------------------------------------------------------------------------
 * Waits for every queued search of every live index, releases their idle per-search
 * workspaces and trims the devices' stream-ordered pools back to the driver.  Indexes
 * stay valid; the next search re-allocates what it needs. */
int32_t vdb_shutdown(void);

#ifdef __cplusplus
}
#endif
#endif /* VDB_H */
