// vdb_api.cpp — the C-ABI (include/vdb.h): index object, workspace pool and the
// search driver that sequences the kernels of the vdb_*.hip files (launchers: vdb_internal.h);
// the host arithmetic of each entry point lives in its vdb_*_plan.h.
//
// Host-side restatement of the reference store's operator flow
// (service/optimized_vector_store.py:96-192): ingest appends rows in place and
// computes norms once (instead of re-normalising the corpus on every query,
// :31-41); search = candidate pass + exact rerank instead of a full argsort
// (:176-183).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <set>
#include <unordered_map>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/vdb.h"
#include "vdb_compact_plan.h"
#include "vdb_subset_plan.h"
#include "vdb_range_plan.h"
#include "vdb_group_plan.h"
#include "vdb_filter_plan.h"
#include "vdb_mmr_plan.h"
#include "vdb_fuse_plan.h"
#include "vdb_maxsim_plan.h"
#include "vdb_sparse_plan.h"
#include "vdb_hybsum_plan.h"
#include "vdb_recommend_plan.h"
#include "vdb_search_plan.h"
#include "vdb_internal.h"

using namespace vdb;

namespace {

thread_local std::string g_last_error;

int set_error(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return set_error(_e == hipErrorOutOfMemory ? VDB_ERR_OOM : VDB_ERR_HIP, "%s failed: %s (%s:%d)", \
                             #expr, hipGetErrorString(_e), __FILE__, __LINE__);                        \
    } while (0)

constexpr int64_t kRowAlign = ROW_ALIGN;   // capacity granule, a multiple of every scan step

constexpr size_t kGatedExactBytes = 256u << 20;  // device-gated fallback lists sized for every query of a batch
constexpr int kSubsetBadWord = 12;        // d_xmax word (8 bytes each) counting a row-list search's skipped ids
constexpr int kRecommendBadWord = 13;     // d_xmax word counting the queries a recommend search flagged on the device
constexpr int kFusedBadWord = 14;         // d_xmax word counting the sets a fused search found bad on the device
constexpr int kMaxsimBadWord = 24;        // d_xmax word counting the sets a MaxSim search found bad on the device
constexpr int kMaxsimSkippedWord = 25;    // d_xmax word counting the rows MaxSim searches skipped for an id past the slots
constexpr int kSparseBadWord = 26;        // d_xmax word counting the queries a sparse search found bad on the device
constexpr int kSparseFlagWord = 27;       // d_xmax word a device-memory vdb_index_set_sparse's validation writes its causes to
constexpr size_t kXmaxBytes = 256;        // d_xmax in all (layout: vdb_index_create)

inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline int next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// Bump allocator over one device buffer (256-B aligned carve).
struct Carver {
    char* base;
    size_t off = 0;
    template <typename T>
    T* take(size_t count) {
        off = (off + 255) & ~size_t(255);
        T* p = reinterpret_cast<T*>(base + off);
        off += count * sizeof(T);
        return p;
    }
};

struct Workspace {
    char* dev = nullptr;
    size_t dev_bytes = 0;
    char* exact = nullptr;  // exact-path lists, grown on demand
    size_t exact_cap = 0;
    int* host_flag = nullptr;  // pinned
    // pinned staging of a host-memory search: the queries up, the results down (read with the
    // certificate's flags in one synchronisation; grown on demand)
    char* host_io = nullptr;
    size_t host_io_bytes = 0;
    hipEvent_t done = nullptr;
    // timing (vdb_index_set_param "timing"): a ring of event sets, one per timed search
    // (scan start / scan end / finish end / pilot start), read once complete, so timed
    // device-memory searches can be queued back to back without a host wait
    static constexpr int kTRing = 64;
    hipEvent_t tring[kTRing][4] = {};
    int t_head = 0, t_pending = 0;
    bool busy = false;
    bool used = false;
    hipStream_t last_st = nullptr;  // stream of the last search that used it
    // host-memory searches without a caller stream run on their workspace's own stream, so
    // concurrent host searches (the reference's 4-thread executor, api/routes/vectors.py:43)
    // overlap on the device instead of queueing on one index stream
    hipStream_t own = nullptr;
    // vdb_index_filter_mask: pinned slots for the staged clauses and offsets of a call (one
    // allocation of kFiltRing x kFilterStageBytes, on first use) and the event after each slot's
    // upload: a device-memory call returns with its upload only queued, so the next call takes the
    // next slot, and a slot is rewritten only once its last upload has run
    static constexpr int kFiltRing = 8;
    char* filt_io = nullptr;
    hipEvent_t filt_up[kFiltRing] = {};
    bool filt_used[kFiltRing] = {};
    int filt_head = 0;
};

}  // namespace

struct vdb_index {
    int dim = 0, metric = 0, device = 0;
    int Dp = 0, G = 0;
    int64_t count = 0;
    int64_t cap_rows = 0;  // multiple of kRowAlign
    float* X = nullptr;   // row-major fp32 [cap_rows][Dp] (rerank, exact scan, export, graph)
    float* Xs = nullptr;  // the candidate pass's copy, same bytes: split-bf16 tiles (PREC_BF16X3 / BF16 /
                          // AUTO) or fp32 tiles (PREC_FP32), rebuilt from X when the precision class changes.
                          // AUTO with the int8 copy allocates it lazily, on the first search that runs a
                          // split pass (a hold, a host re-pass or retry): ensure_xs
    float* Xq = nullptr;  // the int8 copy (PREC_I8 / I8X3, AUTO with auto_i8): half the bytes of X
    // its xh plane row-major [cap][Dp] (with Xq): the finish refines I8 candidates' scores with
    // the query's rounding residual, reading each candidate's row whole (vdb_exact.hip)
    int8_t* Xh = nullptr;
    double* nrm64 = nullptr;
    float* inv32 = nullptr;
    float* sq32 = nullptr;
    float* rinit32 = nullptr;  // -|x|^2 / 2: the split pass's L2 accumulator start (vdb_scan2.hip)
    unsigned long long* d_xmax = nullptr;
    int* d_nonfinite = nullptr;
    double xmax = 0.0;
    double xres_rel = 0.0, xres_abs = 0.0;  // max |x - bf16(x)| / |x| and max |x - bf16(x)| (PREC_BF16 bound)
    // PREC_BF16 bound along a direction: dir = the normalised mean of the split
    // copy's rows of the first add (up to kDirRows of them), frozen until clear();
    // xres_dir = max |dir . (y - bf16(y))| over all rows
    float* d_dir = nullptr;  // [Dp], zero padded
    bool dir_set = false;
    double xres_dir = 0.0;
    // The int8 pass (PREC_I8 / PREC_I8X3, vdb_scan8.hip): the candidate copy holds z = y - mu,
    // mu [Dp] the mean of the first add's candidate rows (set with dir, frozen until clear()),
    // quantised with step sx = 1.25 max |z| / 127 (over those rows; later rows past the range
    // clip, which the residual statistics then show); d_i8 [0..6) the running row statistics of
    // quant_rows (fp64 bits), [6] max |z| (float bits) at setup; i8st = their host copies.
    float* d_mu = nullptr;
    float sx = 0.0f;
    int64_t dir_rows = 0;  // rows dir / mu / sx were derived from (re-derived as the index doubles, up to kDirRows)
    unsigned long long* d_i8 = nullptr;
    double i8st[6] = {0, 0, 0, 0, 0, 0};
    // the int8 pass's checksum (vdb_scan8.hip): column sums (mod 2^32) of the int8 copy's xh and
    // xl planes over rows [0, count), [2][Dp]; kept by build_candidate_rows
    uint32_t* d_csum = nullptr;
    int64_t scan_checksum = 1;  // knob: 1 the pass's sums are checked by the finish, 0 off (A/B)
    // VDB_PREC_AUTO's candidate copy: the int8 one (I8 / I8X3) when set, else the split-bf16 one
    bool auto_i8 = true;
    hipStream_t stream = nullptr;
    int n_cu = 256;
    // knobs
    int64_t precision = VDB_PREC_AUTO;
    // VDB_PREC_AUTO: BF16 by default; a BF16 search whose uncertified queries are
    // too many for a re-pass (host memory: more than 1/8 of the batch; device memory: any, seen
    // lagged through h_totals) starts a HOLD of BF16X3 searches, 16 << (fails - 1) of them
    // (exponential backoff up to 2048 while probes keep failing; `fails` resets after 64 BF16
    // searches without a new failure, and hold and fails reset when the rows change).  So one
    // near-duplicate query no longer pins the index to BF16X3, and a corpus that never certifies
    // in BF16 pays a probe only once per 2048 searches.
    std::atomic<int> auto_hold{0}, auto_fails{0}, auto_ok{0};
    // With auto_i8, the one-plane pass is I8 (the int8 copy); an I8 failure too large for a
    // re-pass holds BF16 (the split copy) instead for 16 << (fails8 - 1) searches (up to 2048;
    // fails8 resets after 64 I8 searches without a new failure, both when the rows change), so
    // data where the 8-bit query's wider bound does not certify (1M x 1536) runs BF16 and probes
    // I8 rarely.  last_i8: the last one-plane pass was I8 (device-memory failures arrive late).
    std::atomic<int> auto_hold8{0}, auto_fails8{0}, auto_ok8{0};
    std::atomic<bool> last_i8{false};
    // The device-gated fallback total last seen: pinned mirror of d_totals[0], written by the
    // gated exact kernel of a device-memory search and read by the next search.
    std::atomic<unsigned long long> auto_seen{0};
    unsigned long long* h_totals = nullptr;
    int64_t margin = -1;  // -1 = default
    int64_t force_exact = 0;
    int64_t n_wg_override = 0;
    int64_t timing = 0;  // record HIP events around the candidate pass
    int64_t pilot_tiles = -1;  // row tiles sampled by the pilot bound (0 = off, -1 = by k)
    int64_t graph_fill = 0;     // graph build: top up pruned neighbour lists (hnswlib keepPrunedConnections)
    int64_t scan_variant = 0;     // fp32 candidate pass variant (vdb_scan.hip)
    int64_t scan_variant_b3 = 0;  // bf16x3 candidate pass variant
    int64_t scan_sync = 0;        // scan step end: 0 auto, 1 lockstep barrier, 2 flag-gated rounds
    int64_t no_fallback = 0;      // diagnostics only: skip the exact fallback (results may be wrong)
    int64_t pilot_rank_override = 0;  // tuning: rank of the pilot bound (0 = the Poisson rule)
    bool no_dir_bound = false;    // diagnostics: PREC_BF16 certificate with Cauchy-Schwarz only
    int64_t finish_split = 1;  // workgroups per query in the finish kernel (tuning)
    // the finish's small form (4 waves, 4096-entry buffer) that fits beside a long-row wide scan:
    // -1 auto (with that scan at <= 1024 dims), 0 off, 1 on
    int64_t finish_small = -1;
    int64_t scan_qlds = -1;    // split pass: query block in LDS when it fits (-1 auto), 0 never
    // the finish's I8 refinement (i8_refine): -1 auto = rows of kRefineMinDp dims or more (C3 +6%,
    // C2 neutral, C6 -1%: shorter rows rerank cheaply; profiles/r04_mx1); 0 off; 1 on
    int i8_refine = -1;
    // device-memory searches: uncertified queries of an I8 / BF16 / I8X3 pass re-passed in BF16X3
    // on the device (gated kernels, no host wait) instead of the fp64 exact scan.  -1 auto: armed
    // for kRepassArm searches once a device fallback has been seen; 0 off; 1 always
    int64_t device_repass = -1;
    std::atomic<int> repass_arm{0};
    // auto's I8 pass on indexes of <= kI8NarrowRows rows: KP = 128 instead of 256 (a weak-scaled
    // rank's shard: the k-th to KP-th gap widens as rows thin out) until any search of this index
    // flags a query, then 256 for good (i8_wide).  Knob "i8_narrow": -1 auto, 0 off.
    int64_t i8_narrow = -1;
    std::atomic<bool> i8_wide{false};
    // auto's L2 pass for 16 < k <= 100: PREC_I8Q (the xh plane against the 16-bit query) unless
    // "auto_i8q" = 0, or once a batch flagged more than 1/8 of its queries (i8q_off: I8X3 after)
    std::atomic<bool> auto_i8q{true};
    std::atomic<bool> i8q_off{false};
    // the last auto pass was I8Q, and its batch size: a device-memory search sees its flags a
    // search or more late (h_totals), and turns I8Q off by the same 1/8 rule
    std::atomic<bool> last_i8q{false};
    std::atomic<int> last_i8q_b{0};
    int64_t scan_q4 = -1;      // split pass 128-query shape (D <= 128, KP = 128, B >= 256): -1 auto, 0 off, 1 on
    // the wide int8 pass (vdb_scan8w.hip: rows of 4 groups, B > 256): -1 auto (from kWideMinRows
    // rows), 0 off, 1 at any row count
    int64_t scan_wide = -1;
    // vdb_index_remove: rows per chunk of the gather's scratch (0 = by bytes, vdb_compact_plan.h)
    int64_t remove_chunk = 0;
    // vdb_index_update: rows per staging chunk (0 = by bytes, 256 MiB as an add's staging)
    int64_t update_chunk = 0;
    // bumped whenever rows leave, move or change (remove, clear, update): a graph built before is
    // stale even when the count is (again) what it recorded
    std::atomic<int64_t> gen{0};
    // stats
    std::atomic<int64_t> n_searches{0}, n_queries{0}, n_fallback{0}, n_overflow{0}, n_incons{0}, n_repass{0}, n_q4{0};
    std::atomic<int64_t> n_wide{0};  // searches through the wide int8 pass
    std::atomic<int64_t> n_xs_builds{0};  // lazy builds of the split copy (ensure_xs)
    std::atomic<int64_t> n_rows_removed{0};  // rows removed by vdb_index_remove (cumulative)
    std::atomic<int64_t> n_rows_updated{0};  // rows rewritten by vdb_index_update (cumulative)
    // vdb_index_search_rows: calls, queries and ids offered (successful calls); the ids a
    // device-memory call's kernel skipped are counted on the device (d_xmax + kSubsetBadWord)
    std::atomic<int64_t> n_subset_searches{0}, n_subset_queries{0}, n_subset_rows{0};
    int64_t subset_wgs = 0;  // knob: workgroups per query of a row-list search (0 = auto)
    std::atomic<int64_t> n_range_searches{0}, n_range_queries{0};  // vdb_index_search_range (successful calls)
    // vdb_index_set_groups: the group column [group_n] (a device copy owned by the index), the bitmap
    // of its rows with an id >= 0 (ceil(group_n / 32) words) and whether any id is negative; add,
    // remove and clear drop it (group_set = false), update keeps it
    int32_t* groups = nullptr;
    uint32_t* group_valid = nullptr;
    int64_t group_n = 0, group_cap = 0;
    bool group_set = false, group_any_neg = false;
    int64_t group_valid_rows = 0;  // rows with an id >= 0
    // vdb_index_search_groups: calls and queries (successful calls), and the device's count of the
    // queries that took the exact fallback
    std::atomic<int64_t> n_group_sets{0}, n_group_searches{0}, n_group_queries{0};
    unsigned long long* d_group_fb = nullptr;
    int64_t group_fetch = 0;        // knob: rows the inner search fetches (0 = auto, vdb_group_plan.h)
    int64_t group_force_exact = 0;  // knob: every query takes the exact fallback (tests, A/B)
    // vdb_index_search_mmr: calls and queries (successful calls)
    std::atomic<int64_t> n_mmr_searches{0}, n_mmr_queries{0};
    // vdb_index_search_recommend: calls and queries (successful calls); the queries its build kernel
    // flagged are counted on the device (d_xmax + kRecommendBadWord)
    std::atomic<int64_t> n_rec_searches{0}, n_rec_queries{0};
    // vdb_index_search_fused: calls and sets (successful calls); the sets its kernel found bad are
    // counted on the device (d_xmax + kFusedBadWord)
    std::atomic<int64_t> n_fused_searches{0}, n_fused_sets{0};
    // vdb_index_search_maxsim: calls and sets (successful calls); the sets its rank kernel found bad
    // and the rows its scan skipped are counted on the device (d_xmax + kMaxsimBadWord / SkippedWord)
    std::atomic<int64_t> n_maxsim_searches{0}, n_maxsim_sets{0};
    // vdb_index_set_sparse: the sparse column, one CSR row per stored row (device copies owned by the
    // index): sparse_indptr [sparse_n + 1] and sparse_pairs [sparse_nnz] interleaved (term, weight);
    // add, remove and clear drop it (sparse_set = false), update keeps it; independent of the groups
    int64_t* sparse_indptr = nullptr;
    SparsePair* sparse_pairs = nullptr;
    int64_t sparse_n = 0, sparse_nnz = 0;
    int32_t sparse_terms = 0;
    bool sparse_set = false;
    int64_t sparse_wgs = 0;  // knob: workgroups per query of a sparse search (0 = auto)
    // vdb_index_search_sparse / _hybrid: calls and queries (successful calls); the queries the sparse
    // kernel found bad are counted on the device (d_xmax + kSparseBadWord)
    std::atomic<int64_t> n_sparse_sets{0}, n_sparse_searches{0}, n_sparse_queries{0};
    std::atomic<int64_t> n_hybrid_searches{0}, n_hybrid_queries{0};
    // vdb_index_search_hybrid_sum: calls and queries (successful calls)
    std::atomic<int64_t> n_hybsum_searches{0}, n_hybsum_queries{0};
    // vdb_index_set_column: the numeric columns, slot s = fp64 [count] (a device copy owned by the
    // index, NaN = the row has no value), col_mask bit s = slot s is attached; add, remove and clear
    // drop them all (col_mask = 0), update keeps them; independent of the groups and the sparse column
    double* cols[kFilterSlots] = {};
    int64_t col_cap[kFilterSlots] = {};
    uint32_t col_mask = 0;
    // vdb_index_set_column / vdb_index_filter_mask: successful calls, and the predicates of those
    std::atomic<int64_t> n_column_sets{0}, n_filter_calls{0}, n_filter_preds{0};
    int64_t hybsum_wgs = 0;  // knob: workgroups per query of a weighted-sum hybrid search (0 = auto)
    std::atomic<int64_t> n_by_prec[N_PREC] = {{0}, {0}, {0}, {0}, {0}, {0}};  // candidate passes per PREC_* (VDB_PREC_AUTO's choices)
    std::atomic<int64_t> scan_ns{0}, pipe_ns{0}, n_timed{0};
    unsigned long long* d_totals = nullptr;  // device: flagged / overflowed / flagged-in-bf16 queries of device-gated searches
    std::shared_mutex mu;  // add/clear/reserve exclusive; search shared
    std::mutex xs_mu;      // the lazy split copy's allocation + build (under the shared lock)
    std::mutex ws_mu;
    std::vector<Workspace*> pool;
    // last work queued on each caller stream by searches without a workspace (graph searches):
    // wait_idle() waits for these and the workspaces' events instead of the whole device
    std::unordered_map<hipStream_t, hipEvent_t> uses;
};

namespace {

// Live indexes, for vdb_shutdown().
std::mutex g_reg_mu;
std::set<vdb_index*> g_indices;

void free_workspace_memory(Workspace* w) {
    if (w->dev) (void)hipFree(w->dev);
    if (w->exact) (void)hipFree(w->exact);
    if (w->host_flag) (void)hipHostFree(w->host_flag);
    if (w->host_io) (void)hipHostFree(w->host_io);
    if (w->filt_io) (void)hipHostFree(w->filt_io);
    w->filt_io = nullptr;
    for (int r = 0; r < Workspace::kFiltRing; ++r) w->filt_used[r] = false;
    w->dev = nullptr;
    w->exact = nullptr;
    w->host_flag = nullptr;
    w->host_io = nullptr;
    w->dev_bytes = w->exact_cap = w->host_io_bytes = 0;
}

int wait_idle(vdb_index* ix);

// The candidate copies a precision setting keeps: Xs holds fp32 tiles (FP32), split-bf16 tiles
// (BF16 / BF16X3 / AUTO) or nothing (I8 / I8X3); Xq the int8 copy (I8 / I8X3, AUTO with auto_i8:
// AUTO keeps both and picks per batch, vdb_index_search).
enum XsKind { kXsNone = -1, kXsFp32 = 0, kXsSplit = 1 };
int xs_kind(int64_t precision) {
    if (precision == VDB_PREC_FP32) return kXsFp32;
    if (precision == VDB_PREC_I8 || precision == VDB_PREC_I8X3 || precision == VDB_PREC_I8Q) return kXsNone;
    return kXsSplit;
}
bool needs_i8(int64_t precision, bool auto_i8) {
    return precision == VDB_PREC_I8 || precision == VDB_PREC_I8X3 || precision == VDB_PREC_I8Q ||
           (precision == VDB_PREC_AUTO && auto_i8);
}
// Settings whose candidate pass reads Xs on every search keep it allocated and up to date from the
// start; AUTO with the int8 copy reads it only for holds, host re-passes and retries, so it is
// built on first use (ensure_xs): 7 instead of 11 B per element (fp32 rows 4, int8 planes 2, the
// row-major xh 1) while no search needs it.  I8 / I8X3 never read it.
bool xs_eager(const vdb_index* ix) {
    const int kind = xs_kind(ix->precision);
    return kind == kXsFp32 || (kind == kXsSplit && !(ix->precision == VDB_PREC_AUTO && ix->auto_i8));
}
float* xs_ptr(const vdb_index* ix) { return __atomic_load_n(&ix->Xs, __ATOMIC_ACQUIRE); }

// The candidate copies of rows [row0, row0 + n) from the row-major rows (tiles: whole row tiles;
// the int8 copy row by row, its statistics into d_i8).  xs / xq: which copies to build.
hipError_t build_candidate_rows(const vdb_index* ix, int64_t row0, int64_t n, hipStream_t st, bool xs = true,
                                bool xq = true) {
    const float* inv = ix->metric == VDB_METRIC_COSINE ? ix->inv32 : nullptr;
    hipError_t e = hipSuccess;
    if (xs && ix->Xs && xs_kind(ix->precision) == kXsFp32) e = launch_tile_rows(ix->X, ix->G, row0, n, ix->Xs, st);
    if (xs && ix->Xs && xs_kind(ix->precision) == kXsSplit) e = launch_split_rows(ix->X, ix->G, row0, n, inv, ix->Xs, st);
    if (e == hipSuccess && xq && needs_i8(ix->precision, ix->auto_i8)) {
        // (rows [0, n) rebuild the whole copy: its column sums start again)
        if (row0 == 0) e = hipMemsetAsync(ix->d_csum, 0, (size_t)2 * ix->Dp * sizeof(uint32_t), st);
        if (e == hipSuccess)
            e = launch_quant_rows(ix->X, inv, ix->d_mu, ix->d_dir, ix->sx, row0, n, ix->G, ix->Xq, ix->d_i8, st, ix->Xh);
        if (e == hipSuccess) e = launch_colsum8(ix->Xq, row0, n, ix->G / 4, ix->d_csum, st);
    }
    return e;
}

// Host copies of the int8 copy's row statistics (after the kernels that update them).
hipError_t read_i8_stats(vdb_index* ix, hipStream_t st) {
    unsigned long long b[6];
    hipError_t e = hipMemcpyAsync(b, ix->d_i8, sizeof(b), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) std::memcpy(ix->i8st, b, sizeof(b));
    return e;
}

// Device memory zeroed and the zeroing finished when this returns, so work on ANY stream after it
// sees zeros.  (hipMemset enqueues on the null stream, which the library's and the callers'
// non-blocking streams are not ordered after.)
hipError_t zero_now(void* p, size_t bytes, hipStream_t st) {
    hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

bool debug_knobs_enabled() {
    const char* e = std::getenv("VDB_DEBUG_KNOBS");
    return e && std::strcmp(e, "1") == 0;
}

int ensure_capacity(vdb_index* ix, int64_t rows) {
    if (rows <= ix->cap_rows) return VDB_OK;
    if (ix->X) {  // every search that might read the old buffers is done (callers hold the write lock)
        const int wr = wait_idle(ix);
        if (wr) return wr;
    }
    int64_t cap = std::max<int64_t>(ix->cap_rows * 2, kRowAlign);
    while (cap < rows) cap *= 2;
    cap = round_up(cap, kRowAlign);
    const size_t tile_floats = (size_t)ix->G * BLOCK_FLOATS;
    const size_t x_bytes = (size_t)(cap / 32) * tile_floats * sizeof(float);
    float* X = nullptr;
    float* Xs = nullptr;
    float* Xq = nullptr;
    int8_t* Xh = nullptr;
    double* n64 = nullptr;
    float *i32 = nullptr, *s32 = nullptr, *r32 = nullptr;
    // All new buffers are allocated and filled before the index switches to them; on
    // any failure (typically out of memory while doubling at large N) they are freed
    // and the index keeps its current buffers, so a later retry sees the same HBM.
    auto fail = [&](hipError_t e, const char* what) {
        (void)hipStreamSynchronize(ix->stream);
        for (void* p : {(void*)X, (void*)Xs, (void*)Xq, (void*)Xh, (void*)n64, (void*)i32, (void*)s32, (void*)r32})
            if (p) (void)hipFree(p);
        return set_error(e == hipErrorOutOfMemory ? VDB_ERR_OOM : VDB_ERR_HIP,
                         "growing the index to %lld rows: %s failed: %s", (long long)cap, what, hipGetErrorString(e));
    };
#define CAP_TRY(expr)                          \
    do {                                       \
        hipError_t _e = (expr);                \
        if (_e != hipSuccess) return fail(_e, #expr); \
    } while (0)
    CAP_TRY(hipMalloc(&X, x_bytes));
    if (ix->Xs || xs_eager(ix)) {  // (AUTO with the int8 copy: lazily, ensure_xs)
        CAP_TRY(hipMalloc(&Xs, x_bytes));
        CAP_TRY(hipMemsetAsync(Xs, 0, x_bytes, ix->stream));
    }
    // the int8 copy only where a setting reads it (FP32 / BF16X3 / BF16 / AUTO without
    // auto_int8 never do; set_param allocates it when a setting starts to, ensure_xq)
    const bool with_xq = ix->Xq || needs_i8(ix->precision, ix->auto_i8);
    if (with_xq) {
        CAP_TRY(hipMalloc(&Xq, x_bytes / 2));
        CAP_TRY(hipMemsetAsync(Xq, 0, x_bytes / 2, ix->stream));
        CAP_TRY(hipMalloc(&Xh, x_bytes / 4));
        CAP_TRY(hipMemsetAsync(Xh, 0, x_bytes / 4, ix->stream));
    }
    CAP_TRY(hipMalloc(&n64, cap * sizeof(double)));
    CAP_TRY(hipMalloc(&i32, cap * sizeof(float)));
    CAP_TRY(hipMalloc(&s32, cap * sizeof(float)));
    CAP_TRY(hipMalloc(&r32, cap * sizeof(float)));
    CAP_TRY(hipMemsetAsync(r32, 0, cap * sizeof(float), ix->stream));
    CAP_TRY(hipMemsetAsync(X, 0, x_bytes, ix->stream));
    CAP_TRY(hipMemsetAsync(n64, 0, cap * sizeof(double), ix->stream));
    CAP_TRY(hipMemsetAsync(i32, 0, cap * sizeof(float), ix->stream));
    CAP_TRY(hipMemsetAsync(s32, 0, cap * sizeof(float), ix->stream));
    if (ix->X) {
        const int64_t used_tiles = round_up(ix->count, 128) / 32;  // whole super tiles (prefix of the layout)
        CAP_TRY(hipMemcpyAsync(X, ix->X, (size_t)ix->count * ix->Dp * sizeof(float), hipMemcpyDeviceToDevice,
                               ix->stream));
        if (Xs && ix->Xs)
            CAP_TRY(hipMemcpyAsync(Xs, ix->Xs, (size_t)used_tiles * tile_floats * sizeof(float),
                                   hipMemcpyDeviceToDevice, ix->stream));
        if (Xq && ix->Xq)
            CAP_TRY(hipMemcpyAsync(Xq, ix->Xq, (size_t)used_tiles * tile_floats * sizeof(float) / 2,
                                   hipMemcpyDeviceToDevice, ix->stream));
        if (Xh && ix->Xh)
            CAP_TRY(hipMemcpyAsync(Xh, ix->Xh, (size_t)ix->count * ix->Dp, hipMemcpyDeviceToDevice, ix->stream));
        CAP_TRY(hipMemcpyAsync(n64, ix->nrm64, ix->count * sizeof(double), hipMemcpyDeviceToDevice, ix->stream));
        CAP_TRY(hipMemcpyAsync(i32, ix->inv32, ix->count * sizeof(float), hipMemcpyDeviceToDevice, ix->stream));
        CAP_TRY(hipMemcpyAsync(s32, ix->sq32, ix->count * sizeof(float), hipMemcpyDeviceToDevice, ix->stream));
        CAP_TRY(hipMemcpyAsync(r32, ix->rinit32, ix->count * sizeof(float), hipMemcpyDeviceToDevice, ix->stream));
    }
    CAP_TRY(hipStreamSynchronize(ix->stream));
#undef CAP_TRY
    if (ix->X) {
        (void)hipFree(ix->X);
        if (ix->Xs) (void)hipFree(ix->Xs);
        if (ix->Xq) (void)hipFree(ix->Xq);
        if (ix->Xh) (void)hipFree(ix->Xh);
        (void)hipFree(ix->nrm64);
        (void)hipFree(ix->inv32);
        (void)hipFree(ix->sq32);
        (void)hipFree(ix->rinit32);
    }
    ix->X = X;
    ix->Xs = Xs;
    ix->Xq = Xq;
    ix->Xh = Xh;
    ix->nrm64 = n64;
    ix->inv32 = i32;
    ix->sq32 = s32;
    ix->rinit32 = r32;
    ix->cap_rows = cap;
    return VDB_OK;
}

// The int8 copy for a setting that starts to read it (lazily: ensure_capacity keeps it only
// while a setting does).  Zeroed; the caller rebuilds rows [0, count) (build_candidate_rows).
int ensure_xq(vdb_index* ix) {
    if (ix->Xq || ix->cap_rows == 0) return VDB_OK;
    const size_t bytes = (size_t)(ix->cap_rows / 32) * ix->G * BLOCK_FLOATS * sizeof(float) / 2;
    float* Xq = nullptr;
    int8_t* Xh = nullptr;
    hipError_t e = hipMalloc(&Xq, bytes);
    if (e == hipSuccess) e = hipMalloc(&Xh, bytes / 2);
    if (e == hipSuccess) e = hipMemsetAsync(Xq, 0, bytes, ix->stream);
    if (e == hipSuccess) e = hipMemsetAsync(Xh, 0, bytes / 2, ix->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) {
        if (Xq) (void)hipFree(Xq);
        if (Xh) (void)hipFree(Xh);
        return set_error(e == hipErrorOutOfMemory ? VDB_ERR_OOM : VDB_ERR_HIP, "int8 copy: %s", hipGetErrorString(e));
    }
    ix->Xq = Xq;
    ix->Xh = Xh;
    return VDB_OK;
}

// The candidate copy Xs for a search that runs a split (or fp32) pass while it is not allocated
// (AUTO with the int8 copy: xs_eager).  Called under the index's shared lock (no add, growth or
// clear runs meanwhile); concurrent searches serialise on xs_mu, and the first allocates it, builds
// rows [0, count) on the index's stream and waits, then publishes the pointer.
int ensure_xs(vdb_index* ix) {
    if (xs_ptr(ix) || ix->cap_rows == 0 || xs_kind(ix->precision) == kXsNone) return VDB_OK;
    std::lock_guard<std::mutex> lg(ix->xs_mu);
    if (ix->Xs) return VDB_OK;
    const size_t bytes = (size_t)(ix->cap_rows / 32) * ix->G * BLOCK_FLOATS * sizeof(float);
    float* Xs = nullptr;
    hipError_t e = hipMalloc(&Xs, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(Xs, 0, bytes, ix->stream);
    if (e == hipSuccess && ix->count > 0) {
        const float* inv = ix->metric == VDB_METRIC_COSINE ? ix->inv32 : nullptr;
        e = xs_kind(ix->precision) == kXsFp32 ? launch_tile_rows(ix->X, ix->G, 0, ix->count, Xs, ix->stream)
                                              : launch_split_rows(ix->X, ix->G, 0, ix->count, inv, Xs, ix->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess) {
        if (Xs) (void)hipFree(Xs);
        return set_error(e == hipErrorOutOfMemory ? VDB_ERR_OOM : VDB_ERR_HIP, "split candidate copy: %s",
                         hipGetErrorString(e));
    }
    __atomic_store_n(&ix->Xs, Xs, __ATOMIC_RELEASE);
    ix->n_xs_builds++;
    return VDB_OK;
}

// A free workspace whose last search was queued on the same stream (stream order makes the
// reuse safe without a wait), else one whose last search has finished, else a new one (up to
// kMaxWs; then any free one, its reuse waiting on its last search): searches queued on several
// streams from one host thread (a server's request streams) then run concurrently instead of
// serialising on one workspace.
constexpr size_t kMaxWs = 16;

// own = a host-memory search that runs on the workspace's own stream: any free workspace
// whose last search has finished (or a new one) serves.
Workspace* acquire_ws(vdb_index* ix, hipStream_t st, bool own = false) {
    std::lock_guard<std::mutex> g(ix->ws_mu);
    Workspace* idle = nullptr;
    Workspace* any = nullptr;
    for (Workspace* w : ix->pool) {
        if (w->busy) continue;
        if (!w->used || (!own && w->last_st == st)) {
            w->busy = true;
            return w;
        }
        if (!idle && w->done && hipEventQuery(w->done) == hipSuccess) idle = w;
        if (!any) any = w;
    }
    Workspace* w = idle ? idle : ix->pool.size() >= kMaxWs ? any : nullptr;
    if (!w) {
        w = new Workspace();
        ix->pool.push_back(w);
    }
    w->busy = true;
    return w;
}

// Another search of this index on the device right now (being queued, or queued and not finished):
// the finish's small form pays off only when it can run beside another batch's scan.
bool others_in_flight(vdb_index* ix, const Workspace* self) {
    std::lock_guard<std::mutex> g(ix->ws_mu);
    for (Workspace* w : ix->pool) {
        if (w == self) continue;
        if (w->busy) return true;
        if (w->used && w->done && hipEventQuery(w->done) == hipErrorNotReady) return true;
    }
    return false;
}

void release_ws(vdb_index* ix, Workspace* w, hipStream_t st) {
    if (w->done == nullptr) (void)hipEventCreateWithFlags(&w->done, hipEventDisableTiming);
    (void)hipEventRecord(w->done, st);
    w->used = true;
    w->last_st = st;
    std::lock_guard<std::mutex> g(ix->ws_mu);
    w->busy = false;
}

// Remember the last work a search without a workspace queued on `st` (wait_idle).
int note_use(vdb_index* ix, hipStream_t st) {
    std::lock_guard<std::mutex> g(ix->ws_mu);
    // a server that makes a stream per request would grow this map without bound:
    // past 64 entries, the ones whose last recorded work has completed are dropped
    if (ix->uses.size() >= 64 && !ix->uses.count(st)) {
        for (auto it = ix->uses.begin(); it != ix->uses.end();) {
            if (hipEventQuery(it->second) == hipSuccess) {
                (void)hipEventDestroy(it->second);
                it = ix->uses.erase(it);
            } else {
                ++it;
            }
        }
    }
    hipEvent_t& e = ix->uses[st];
    if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(e, st));
    return VDB_OK;
}

// Every search queued on this index (any stream) and its own stream are done: what a resize,
// a rebuild of the candidate copy or a clear needs before touching the buffers searches read.
// Waits on this index's events only, not on the whole device (other indexes keep running).
int wait_idle(vdb_index* ix) {
    std::vector<hipEvent_t> evs;
    {
        std::lock_guard<std::mutex> g(ix->ws_mu);
        for (Workspace* w : ix->pool)
            if (w->used && w->done) evs.push_back(w->done);
        for (auto& kv : ix->uses) evs.push_back(kv.second);
    }
    for (hipEvent_t e : evs) HIP_TRY(hipEventSynchronize(e));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    return VDB_OK;
}

// Accumulate the timing events of a search whose host side returned without
// waiting for the device (device-gated fallback).
// Read the `n` oldest pending event sets of the ring (waiting for them if needed).
int flush_timing(vdb_index* ix, Workspace* w, int n = Workspace::kTRing) {
    while (w->t_pending > 0 && n-- > 0) {
        hipEvent_t* ev = w->tring[(w->t_head - w->t_pending + Workspace::kTRing) % Workspace::kTRing];
        HIP_TRY(hipEventSynchronize(ev[2]));
        float ms_scan = 0.f, ms_pipe = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms_scan, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms_pipe, ev[3], ev[2]));
        ix->scan_ns += (int64_t)(ms_scan * 1e6);
        ix->pipe_ns += (int64_t)(ms_pipe * 1e6);
        ix->n_timed++;
        w->t_pending--;
    }
    return VDB_OK;
}

int flush_all_timing(vdb_index* ix) {
    std::lock_guard<std::mutex> g(ix->ws_mu);
    for (Workspace* w : ix->pool)
        if (!w->busy) {
            const int rc = flush_timing(ix, w);
            if (rc) return rc;
        }
    return VDB_OK;
}

// Make the workspace at least `bytes` large and stream-ordered after its last use.
int ws_reserve(Workspace* w, size_t bytes, hipStream_t st) {
    if (w->used && w->done) HIP_TRY(hipStreamWaitEvent(st, w->done, 0));
    if (!w->host_flag) HIP_TRY(hipHostMalloc(&w->host_flag, 64 * sizeof(int), hipHostMallocDefault));
    if (bytes > w->dev_bytes) {
        if (w->dev) {
            HIP_TRY(hipStreamSynchronize(st));
            (void)hipFree(w->dev);
            w->dev = nullptr;
        }
        size_t nb = std::max(bytes, w->dev_bytes * 2);
        HIP_TRY(hipMalloc(&w->dev, nb));
        w->dev_bytes = nb;
    }
    return VDB_OK;
}

// The pinned staging of a host-memory search (the previous host search on this workspace
// synchronised before returning, so nothing reads the old buffer).
int ws_host_io(Workspace* w, size_t bytes) {
    if (bytes > w->host_io_bytes) {
        const size_t nb = std::max(bytes, w->host_io_bytes * 2);
        if (w->host_io) (void)hipHostFree(w->host_io);
        w->host_io = nullptr;
        w->host_io_bytes = 0;
        HIP_TRY(hipHostMalloc(&w->host_io, nb, hipHostMallocDefault));
        w->host_io_bytes = nb;
    }
    return VDB_OK;
}

int ws_reserve_exact(Workspace* w, size_t bytes, hipStream_t st) {
    if (bytes > w->exact_cap) {
        if (w->exact) {
            HIP_TRY(hipStreamSynchronize(st));
            (void)hipFree(w->exact);
            w->exact = nullptr;
        }
        HIP_TRY(hipMalloc(&w->exact, bytes));
        w->exact_cap = bytes;
    }
    return VDB_OK;
}

bool all_finite(const float* p, int64_t n) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(p[i])) return false;
    return true;
}

// ---- the call frame the entry points share -------------------------------------------------------
// A search's stream and workspace, for the length of the call.  Device memory: the caller's
// stream, NULL = the null stream (ordered with the caller's default-stream work, e.g. PyTorch's);
// host memory: the caller's stream, or (NULL) the stream of the workspace the call takes, created
// on first use, so concurrent host searches overlap.  rc != 0: no workspace is held and the error
// is set.  The workspace goes back (its event recorded on the stream) when the lease ends.
struct SearchLease {
    vdb_index* ix;
    Workspace* w = nullptr;
    hipStream_t st = nullptr;
    int rc = VDB_OK;
    SearchLease(vdb_index* ix_, int32_t mem, void* stream) : ix(ix_) {
        const bool own_stream = mem == VDB_MEM_HOST && !stream;
        st = own_stream ? nullptr : (hipStream_t)stream;
        w = acquire_ws(ix, st, own_stream);
        if (!own_stream) return;
        if (!w->own) {
            const hipError_t e = hipStreamCreateWithFlags(&w->own, hipStreamNonBlocking);
            if (e != hipSuccess) {
                {
                    std::lock_guard<std::mutex> lg(ix->ws_mu);
                    w->busy = false;
                }
                w = nullptr;
                rc = set_error(VDB_ERR_HIP, "workspace stream: %s", hipGetErrorString(e));
                return;
            }
        }
        st = w->own;
    }
    ~SearchLease() {
        if (w) release_ws(ix, w, st);
    }
    SearchLease(const SearchLease&) = delete;
    SearchLease& operator=(const SearchLease&) = delete;
};

// `st` runs what follows after the work queued so far on the caller's stream (NULL = the null
// stream): device-memory arguments may still be being written there.
hipError_t order_after_caller(hipStream_t st, void* caller_stream) {
    hipEvent_t ready = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ready, hipEventDisableTiming);
    if (e != hipSuccess) return e;
    e = hipEventRecord(ready, (hipStream_t)caller_stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, ready, 0);
    (void)hipEventDestroy(ready);
    return e;
}

// Host-memory staging of the plan-style entry points (row-list, range and grouped search; their
// *_scratch() keeps the arguments in [in0, in0 + in_bytes) of the workspace and the results in
// [out0, out0 + out_bytes)).  Up: pack(h) writes the arguments into the pinned buffer h, which goes
// up in one copy.
template <typename Pack>
int stage_up(Workspace* w, int64_t in0, int64_t in_bytes, int64_t out_bytes, hipStream_t st, Pack&& pack) {
    const int rc = ws_host_io(w, (size_t)(in_bytes + out_bytes));
    if (rc) return rc;
    pack(w->host_io);
    HIP_TRY(hipMemcpyAsync(w->dev + in0, w->host_io, (size_t)in_bytes, hipMemcpyHostToDevice, st));
    return VDB_OK;
}
// Down: the results in one copy, complete on return, at *r (the pinned buffer, out0's bytes first).
int stage_down(Workspace* w, int64_t in_bytes, int64_t out0, int64_t out_bytes, hipStream_t st, const char** r) {
    *r = w->host_io + in_bytes;
    HIP_TRY(hipMemcpyAsync(w->host_io + in_bytes, w->dev + out0, (size_t)out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VDB_OK;
}


// The index's knobs for the main search's plan (i8_narrow: the policy's answer, see search_locked).
SearchKnobs search_knobs(const vdb_index* ix, bool i8_narrow) {
    SearchKnobs kn{};
    kn.force_exact = ix->force_exact != 0;
    kn.margin = ix->margin;
    kn.i8_narrow = i8_narrow;
    kn.scan_q4 = ix->scan_q4;
    kn.scan_wide = ix->scan_wide;
    kn.n_wg_override = ix->n_wg_override;
    kn.scan_variant = ix->scan_variant;
    kn.scan_sync = ix->scan_sync;
    kn.finish_split = ix->finish_split;
    kn.i8_refine = ix->i8_refine;
    kn.scan_checksum = ix->scan_checksum;
    kn.pilot_tiles = ix->pilot_tiles;
    kn.pilot_rank_override = ix->pilot_rank_override;
    kn.has_xh = ix->Xh != nullptr;
    kn.has_csum = ix->d_csum != nullptr;
    return kn;
}

// What the candidate passes' own files say about this call (the plan never calls into them).
SearchKernelFacts kernel_facts(const SearchShape& s, const SearchKnobs& kn, const SearchKP& kp) {
    SearchKernelFacts f{};
    const int Gs = search_groups(s.prec, s.G);
    if (prec_is_i8(s.prec)) {
        f.scan8wl_ok = scan8wl_ok(s.prec, s.metric, Gs, s.B);
        f.scan8w_ok = scan8w_ok(Gs, s.B);
        f.rows_per_step = scan8_rows_per_step(s.prec, s.metric);
    } else if (s.prec == PREC_BF16X3 || s.prec == PREC_BF16) {
        f.rows_per_step = scan2_rows_per_step(false);
        f.rows_per_step_q4 = scan2_rows_per_step(true);
    } else {
        f.scan_variant_ok = scan_variant_ok(s.prec, (int)kn.scan_variant, Gs);
        const int v = f.scan_variant_ok ? (int)kn.scan_variant : 0;
        f.rows_per_step = scan_rows_per_step(s.prec, v);
        f.scan_priv = scan_priv(s.prec, v, kp.KP);
    }
    return f;
}

// Bytes a device-memory batch's gated fallback is judged by (exact_gate_bytes, vdb_search_plan.h).
size_t gated_exact_bytes(const vdb_index* ix, int nq, int k) {
    const ExactPlan ep = exact_plan(ix->count, ix->n_cu, nq, k, true);
    return (size_t)exact_gate_bytes(ep, nq, (int64_t)exact_scan_scratch_bytes(ep.KE, ep.n_wg_gate, ep.slots));
}

// Exact scan of the queries qlist[0..nq) (or 0..nq) -> writes outputs.  Device-gated form
// (qcount_dev): the flagged count is read on the device, nq is the capacity, and nothing runs
// when no query was flagged.  The plan and the lists' layout: vdb_search_plan.h.
int run_exact(vdb_index* ix, Workspace* w, const float* Qd, const double* qn64, const int* qlist_dev, int nq, int k,
              const uint32_t* mask_dev, float* out_s, int64_t* out_i, double* out_k, int64_t index_offset,
              const int64_t* row_ids, hipStream_t st, const int* qcount_dev = nullptr, const int* ovf_dev = nullptr,
              int* done_dev = nullptr, unsigned long long* host_totals = nullptr) {
    const int64_t N = ix->count;
    const bool gated = qcount_dev != nullptr;
    const ExactPlan ep = exact_plan(N, ix->n_cu, nq, k, gated);
    const int KE = ep.KE, n_wg = ep.n_wg, n_lists = ep.n_wg;
    const int64_t rpw = ep.rpw;
    // the device-gated form keeps its top-k buffers in the workspace (no LDS, vdb_exact.hip)
    const ExactLayout el =
        exact_layout(ep, nq, gated && done_dev ? (int64_t)exact_scan_scratch_bytes(KE, n_wg, ep.slots) : 0);
    int rc = ws_reserve_exact(w, (size_t)el.total, st);
    if (rc) return rc;
    double* lk = reinterpret_cast<double*>(w->exact + el.lk);
    uint32_t* li = reinterpret_cast<uint32_t*>(w->exact + el.li);
    double* mk = reinterpret_cast<double*>(w->exact + el.mk);
    uint32_t* mi = reinterpret_cast<uint32_t*>(w->exact + el.mi);
    char* gscr = el.scr >= 0 ? w->exact + el.scr : nullptr;
    if (gated && done_dev) {  // one launch: the last workgroup per query merges and writes (ExactTail)
        const ExactTail tail{done_dev, mk, mi, k, index_offset, out_s, out_i, out_k, row_ids, host_totals};
        HIP_TRY(launch_exact_scan(ix->metric, KE, Qd, qn64, qlist_dev, nq, ix->X, ix->G, ix->dim, ix->nrm64, mask_dev,
                                  N, n_wg, rpw, lk, li, st, qcount_dev, ovf_dev, ix->d_totals, &tail, kGateSlots,
                                  gscr));
        return VDB_OK;
    }
    HIP_TRY(launch_exact_scan(ix->metric, KE, Qd, qn64, qlist_dev, nq, ix->X, ix->G, ix->dim, ix->nrm64, mask_dev, N,
                              n_wg, rpw, lk, li, st, qcount_dev, ovf_dev, gated ? ix->d_totals : nullptr));
    HIP_TRY(launch_merge_f64_u32(KE, lk, li, n_lists, KE, (int64_t)n_lists * KE, KE, nq, mk, mi, st, qcount_dev));
    HIP_TRY(launch_finalize_u32(ix->metric, mk, mi, KE, nq, qlist_dev, k, index_offset, out_s, out_i, out_k, st,
                                qcount_dev, row_ids));
    return VDB_OK;
}

}  // namespace

extern "C" {

const char* vdb_last_error(void) { return g_last_error.c_str(); }

int32_t vdb_version(void) { return 2; }

int32_t vdb_device_count(int32_t* n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) c = 0;
    if (n) *n = c;
    return VDB_OK;
}

int32_t vdb_index_create(int32_t dim, int32_t metric, int32_t device, vdb_index** out) {
    if (!out) return set_error(VDB_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (dim <= 0 || dim > 65536) return set_error(VDB_ERR_INVALID, "dimension must be in [1, 65536], got %d", dim);
    if (metric != VDB_METRIC_COSINE && metric != VDB_METRIC_EUCLIDEAN)
        return set_error(VDB_ERR_UNSUPPORTED, "unsupported metric id %d (cosine=0, euclidean=1)", metric);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return set_error(VDB_ERR_NODEVICE, "no HIP device visible: the vdb core needs an MI355X (gfx950)");
    if (device < 0 || device >= ndev) return set_error(VDB_ERR_INVALID, "device %d out of range [0,%d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_error(VDB_ERR_NODEVICE, "device %d is %s; this build targets gfx950 only", device,
                         prop.gcnArchName);
    vdb_index* ix = new vdb_index();
    ix->dim = dim;
    ix->metric = metric;
    ix->device = device;
    ix->Dp = (int)round_up(dim, 64);  // G = Dp/8 is a multiple of the scan prefetch depth
    ix->G = ix->Dp / GROUP_DIMS;
    ix->n_cu = prop.multiProcessorCount;
    if (const char* q4 = std::getenv("VDB_SCAN_Q4")) ix->scan_q4 = std::min(1, std::max(-1, std::atoi(q4)));
    if (const char* a8 = std::getenv("VDB_AUTO_I8")) ix->auto_i8 = std::atoi(a8) != 0;
    hipError_t e = hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking);
    // d_xmax: [0, 32) the residual maxima, [32, 36) the non-finite count, [64, 96) and
    // [128, 192) an add's snapshot of the maxima and of d_i8 (restored when the add is rejected),
    // [96, 104) the ids row-list searches skipped (kSubsetBadWord; cumulative, a clear keeps it),
    // [104, 112) the queries recommend searches flagged (kRecommendBadWord; likewise),
    // [112, 120) the sets fused searches found bad (kFusedBadWord; likewise),
    // [192, 200) the sets MaxSim searches found bad and [200, 208) the rows they skipped
    // (kMaxsimBadWord, kMaxsimSkippedWord; likewise), [208, 216) the queries sparse searches found
    // bad (kSparseBadWord; likewise), [216, 224) the causes of a device-memory vdb_index_set_sparse
    // (kSparseFlagWord; zeroed by each such call)
    if (e == hipSuccess) e = hipMalloc(&ix->d_xmax, kXmaxBytes);
    if (e == hipSuccess) e = zero_now(ix->d_xmax, kXmaxBytes, ix->stream);
    if (e == hipSuccess) e = hipMalloc(&ix->d_i8, 64);
    if (e == hipSuccess) e = zero_now(ix->d_i8, 64, ix->stream);
    if (e == hipSuccess) e = hipMalloc(&ix->d_csum, (size_t)2 * ix->Dp * sizeof(uint32_t));
    if (e == hipSuccess) e = zero_now(ix->d_csum, (size_t)2 * ix->Dp * sizeof(uint32_t), ix->stream);
    if (e != hipSuccess) {
        delete ix;
        return set_error(VDB_ERR_HIP, "index setup failed: %s", hipGetErrorString(e));
    }
    ix->d_nonfinite = reinterpret_cast<int*>(reinterpret_cast<char*>(ix->d_xmax) + 32);
    {
        std::lock_guard<std::mutex> rg(g_reg_mu);
        g_indices.insert(ix);
    }
    *out = ix;
    return VDB_OK;
}

int32_t vdb_index_destroy(vdb_index* ix) {
    if (!ix) return VDB_OK;
    {
        std::lock_guard<std::mutex> rg(g_reg_mu);
        g_indices.erase(ix);
    }
    (void)hipSetDevice(ix->device);
    (void)wait_idle(ix);
    for (Workspace* w : ix->pool) {
        free_workspace_memory(w);
        if (w->done) (void)hipEventDestroy(w->done);
        if (w->own) (void)hipStreamDestroy(w->own);
        for (int r = 0; r < Workspace::kTRing; ++r)
            for (int e = 0; e < 4; ++e)
                if (w->tring[r][e]) (void)hipEventDestroy(w->tring[r][e]);
        for (int r = 0; r < Workspace::kFiltRing; ++r)
            if (w->filt_up[r]) (void)hipEventDestroy(w->filt_up[r]);
        delete w;
    }
    if (ix->X) (void)hipFree(ix->X);
    if (ix->Xs) (void)hipFree(ix->Xs);
    if (ix->Xq) (void)hipFree(ix->Xq);
    if (ix->Xh) (void)hipFree(ix->Xh);
    if (ix->nrm64) (void)hipFree(ix->nrm64);
    if (ix->inv32) (void)hipFree(ix->inv32);
    if (ix->sq32) (void)hipFree(ix->sq32);
    if (ix->rinit32) (void)hipFree(ix->rinit32);
    if (ix->d_xmax) (void)hipFree(ix->d_xmax);
    if (ix->d_dir) (void)hipFree(ix->d_dir);
    if (ix->d_mu) (void)hipFree(ix->d_mu);
    if (ix->d_i8) (void)hipFree(ix->d_i8);
    if (ix->d_csum) (void)hipFree(ix->d_csum);
    if (ix->d_totals) (void)hipFree(ix->d_totals);
    if (ix->groups) (void)hipFree(ix->groups);
    if (ix->group_valid) (void)hipFree(ix->group_valid);
    if (ix->d_group_fb) (void)hipFree(ix->d_group_fb);
    if (ix->sparse_indptr) (void)hipFree(ix->sparse_indptr);
    if (ix->sparse_pairs) (void)hipFree(ix->sparse_pairs);
    for (int s = 0; s < kFilterSlots; ++s)
        if (ix->cols[s]) (void)hipFree(ix->cols[s]);
    if (ix->h_totals) (void)hipHostFree(ix->h_totals);
    for (auto& kv : ix->uses) (void)hipEventDestroy(kv.second);
    if (ix->stream) (void)hipStreamDestroy(ix->stream);
    delete ix;
    return VDB_OK;
}

int32_t vdb_index_reserve(vdb_index* ix, int64_t rows) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (rows < 0) return set_error(VDB_ERR_INVALID, "rows must be >= 0");
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_lock<std::shared_mutex> g(ix->mu);
    return ensure_capacity(ix, rows);
}

int32_t vdb_index_set_param(vdb_index* ix, const char* name, int64_t value) {
    if (!ix || !name) return set_error(VDB_ERR_INVALID, "NULL argument");
    std::string n(name);
    if (n == "precision") {
        if (value != VDB_PREC_FP32 && value != VDB_PREC_BF16X3 && value != VDB_PREC_BF16 && value != VDB_PREC_AUTO &&
            value != VDB_PREC_I8 && value != VDB_PREC_I8X3 && value != VDB_PREC_I8Q)
            return set_error(VDB_ERR_INVALID,
                             "precision must be %d (fp32), %d (bf16x3), %d (bf16), %d (auto), %d (i8), %d (i8x3) or "
                             "%d (i8q), got %lld",
                             VDB_PREC_FP32, VDB_PREC_BF16X3, VDB_PREC_BF16, VDB_PREC_AUTO, VDB_PREC_I8, VDB_PREC_I8X3,
                             VDB_PREC_I8Q, (long long)value);
        HIP_TRY(hipSetDevice(ix->device));
        std::unique_lock<std::shared_mutex> g(ix->mu);
        if (value == ix->precision) return VDB_OK;
        const int wr = wait_idle(ix);  // queued searches read the candidate copy
        if (wr) return wr;
        // rebuild a copy the new setting reads that the old one did not keep up to date
        const bool xs = xs_kind(value) != kXsNone && xs_kind(value) != xs_kind(ix->precision);
        const bool xq = needs_i8(value, ix->auto_i8) && !needs_i8(ix->precision, ix->auto_i8);
        if (xq) {
            const int xr = ensure_xq(ix);
            if (xr) return xr;
        }
        ix->precision = value;
        bool built = false;
        if (!ix->Xs && xs_eager(ix)) {  // a setting that reads it on every search: allocated + built now
            const int xr = ensure_xs(ix);
            if (xr) return xr;
            built = true;
        }
        if (((xs && !built) || xq) && ix->X && ix->count > 0) {
            HIP_TRY(build_candidate_rows(ix, 0, ix->count, ix->stream, xs && !built, xq));
            HIP_TRY(read_i8_stats(ix, ix->stream));
        }
    } else if (n == "auto_i8q") {
        ix->auto_i8q = value != 0;
    } else if (n == "auto_int8") {  // VDB_PREC_AUTO's candidate copy: 1 int8, 0 split-bf16
        HIP_TRY(hipSetDevice(ix->device));
        std::unique_lock<std::shared_mutex> g(ix->mu);
        const bool v = value != 0;
        if (v == ix->auto_i8) return VDB_OK;
        const int wr = wait_idle(ix);
        if (wr) return wr;
        const bool xq = needs_i8(ix->precision, v) && !needs_i8(ix->precision, ix->auto_i8);
        if (xq) {
            const int xr = ensure_xq(ix);
            if (xr) return xr;
        }
        ix->auto_i8 = v;
        if (!ix->Xs && xs_eager(ix)) {  // AUTO on the split copy alone: reads it on every search
            const int xr = ensure_xs(ix);
            if (xr) return xr;
        }
        if (xq && ix->X && ix->count > 0) {
            HIP_TRY(build_candidate_rows(ix, 0, ix->count, ix->stream, false, true));
            HIP_TRY(read_i8_stats(ix, ix->stream));
        }
    } else if (n == "margin") {
        ix->margin = value;
    } else if (n == "force_exact") {
        ix->force_exact = value != 0;
    } else if (n == "n_wg") {
        ix->n_wg_override = value;
    } else if (n == "scan_sync") {
        if (value < 0 || value > 2) return set_error(VDB_ERR_INVALID, "scan_sync must be 0, 1 or 2");
        ix->scan_sync = value;
    } else if (n == "scan_variant") {
        if (value < 0 || value > 2) return set_error(VDB_ERR_INVALID, "scan_variant must be 0, 1 or 2");
        ix->scan_variant = value;
    } else if (n == "scan_variant_bf16x3") {
        if (value != 0) return set_error(VDB_ERR_INVALID, "the split-bf16 pass has one variant (0)");
        ix->scan_variant_b3 = value;
    } else if (n == "graph_fill") {
        if (value < 0 || value > 1) return set_error(VDB_ERR_INVALID, "graph_fill must be 0 or 1");
        ix->graph_fill = value;
    } else if (n == "pilot_tiles") {
        if (value < -1 || value > 32768) return set_error(VDB_ERR_INVALID, "pilot_tiles must be in [-1, 32768]");
        ix->pilot_tiles = value;
    } else if (n == "timing") {
        ix->timing = value != 0;
    } else if (n == "no_fallback") {
        ix->no_fallback = value != 0;
    } else if (n == "finish_small") {
        if (value < -1 || value > 1) return set_error(VDB_ERR_INVALID, "finish_small must be -1, 0 or 1");
        ix->finish_small = value;
    } else if (n == "finish_split") {
        if (value < 1 || value > 8) return set_error(VDB_ERR_INVALID, "finish_split must be in [1, 8]");
        ix->finish_split = value;
    } else if (n == "scan_qlds") {
        if (value < -1 || value > 2) return set_error(VDB_ERR_INVALID, "scan_qlds must be -1 (auto), 0, 1 or 2");
        ix->scan_qlds = value;
    } else if (n == "scan_wide") {
        if (value < -1 || value > 1) return set_error(VDB_ERR_INVALID, "scan_wide must be -1, 0 or 1");
        ix->scan_wide = value;
    } else if (n == "scan_q4") {
        if (value < -1 || value > 1) return set_error(VDB_ERR_INVALID, "scan_q4 must be -1, 0 or 1");
        ix->scan_q4 = value;
    } else if (n == "dir_bound") {
        ix->no_dir_bound = value == 0;
    } else if (n == "i8_refine") {
        if (value < -1 || value > 1) return set_error(VDB_ERR_INVALID, "i8_refine must be -1, 0 or 1");
        ix->i8_refine = (int)value;
    } else if (n == "i8_narrow") {
        if (value < -1 || value > 0) return set_error(VDB_ERR_INVALID, "i8_narrow must be -1 or 0");
        ix->i8_narrow = value;
    } else if (n == "remove_chunk") {
        if (value < 0) return set_error(VDB_ERR_INVALID, "remove_chunk must be >= 0 (0 = sized by bytes)");
        std::unique_lock<std::shared_mutex> g(ix->mu);
        ix->remove_chunk = value;
    } else if (n == "update_chunk") {
        if (value < 0) return set_error(VDB_ERR_INVALID, "update_chunk must be >= 0 (0 = sized by bytes)");
        std::unique_lock<std::shared_mutex> g(ix->mu);
        ix->update_chunk = value;
    } else if (n == "subset_wgs") {
        if (value < 0 || value > kSubsetMaxSeg)
            return set_error(VDB_ERR_INVALID, "subset_wgs must be in [0, %d] (0 = auto)", kSubsetMaxSeg);
        std::unique_lock<std::shared_mutex> g(ix->mu);
        ix->subset_wgs = value;
    } else if (n == "sparse_wgs") {
        if (value < 0 || value > kSparseMaxSeg)
            return set_error(VDB_ERR_INVALID, "sparse_wgs must be in [0, %d] (0 = auto)", kSparseMaxSeg);
        std::unique_lock<std::shared_mutex> g(ix->mu);
        ix->sparse_wgs = value;
    } else if (n == "hybrid_sum_wgs") {
        if (value < 0 || value > kHybsumMaxSeg)
            return set_error(VDB_ERR_INVALID, "hybrid_sum_wgs must be in [0, %d] (0 = auto)", kHybsumMaxSeg);
        std::unique_lock<std::shared_mutex> g(ix->mu);
        ix->hybsum_wgs = value;
    } else if (n == "group_fetch") {
        if (value < 0 || value > kGroupMaxFetch)
            return set_error(VDB_ERR_INVALID, "group_fetch must be in [0, %d] (0 = auto)", kGroupMaxFetch);
        std::unique_lock<std::shared_mutex> g(ix->mu);
        ix->group_fetch = value;
    } else if (n == "group_force_exact") {
        if (value < 0 || value > 1) return set_error(VDB_ERR_INVALID, "group_force_exact must be 0 or 1");
        std::unique_lock<std::shared_mutex> g(ix->mu);
        ix->group_force_exact = value;
    } else if (n == "device_repass") {
        if (value < -1 || value > 1) return set_error(VDB_ERR_INVALID, "device_repass must be -1, 0 or 1");
        ix->device_repass = value;
    } else if (n.rfind("debug_", 0) == 0 && !debug_knobs_enabled()) {
        // test-only knobs corrupt the index on purpose: only with VDB_DEBUG_KNOBS=1
        return set_error(VDB_ERR_INVALID, "'%s' is a test-only knob (set VDB_DEBUG_KNOBS=1)", name);
    } else if (n == "debug_sink_row8") {
        // TEST ONLY: both int8 planes of row `value` := -127 (the column sums untouched): a corpus
        // operand the int8 pass reads wrong that UNDER-scores the row (for queries with
        // non-negative components) -- the side the finish's approx-vs-exact check cannot see; the
        // pass's checksum flags it
        HIP_TRY(hipSetDevice(ix->device));
        std::unique_lock<std::shared_mutex> g(ix->mu);
        if (value < 0 || value >= ix->count || !ix->Xq)
            return set_error(VDB_ERR_INVALID, "debug_sink_row8: no int8 row %lld", (long long)value);
        const int wr = wait_idle(ix);
        if (wr) return wr;
        HIP_TRY(launch_sink_row8(ix->Xq, value, ix->G / 4, ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    } else if (n == "scan_checksum") {
        if (value < 0 || value > 2) return set_error(VDB_ERR_INVALID, "scan_checksum must be 0, 1 or 2");
        ix->scan_checksum = value;
    } else if (n == "debug_stale_rinit") {
        // TEST ONLY: plants a stale L2 start value, -|x|^2/2 := 0 for row `value` (the operand a
        // scan read before its load landed in VERDICT r3), so the consistency guard of the
        // finish can be seen to flag the query instead of certifying it
        if (value < 0) return set_error(VDB_ERR_INVALID, "debug_stale_rinit: row must be >= 0");
        HIP_TRY(hipSetDevice(ix->device));
        std::unique_lock<std::shared_mutex> g(ix->mu);
        if (value >= ix->count || !ix->rinit32) return set_error(VDB_ERR_INVALID, "debug_stale_rinit: no row %lld", (long long)value);
        const int wr = wait_idle(ix);
        if (wr) return wr;
        const float zero = 0.0f;
        HIP_TRY(hipMemcpyAsync(ix->rinit32 + value, &zero, sizeof(float), hipMemcpyHostToDevice, ix->stream));
        HIP_TRY(hipStreamSynchronize(ix->stream));
    } else if (n == "pilot_rank") {
        if (value < 0 || value > 256) return set_error(VDB_ERR_INVALID, "pilot_rank must be in [0, 256]");
        ix->pilot_rank_override = value;
    } else {
        return set_error(VDB_ERR_INVALID, "unknown parameter '%s'", name);
    }
    return VDB_OK;
}

int32_t vdb_index_get_stat(const vdb_index* cix, const char* name, int64_t* value) {
    if (!cix || !name || !value) return set_error(VDB_ERR_INVALID, "NULL argument");
    vdb_index* ix = const_cast<vdb_index*>(cix);  // pending device-side counts are folded in
    std::string n(name);
    unsigned long long dt[4] = {0, 0, 0, 0};
    if ((n == "fallback_queries" || n == "overflow_queries" || n == "repass_queries") && ix->d_totals) {
        HIP_TRY(hipSetDevice(ix->device));
        const int wr = wait_idle(ix);  // device-memory searches queued on caller streams
        if (wr) return wr;
        HIP_TRY(hipMemcpy(dt, ix->d_totals, sizeof(dt), hipMemcpyDeviceToHost));
    }
    if (n == "scan_ns" || n == "pipeline_ns" || n == "timed_searches") {
        HIP_TRY(hipSetDevice(ix->device));
        const int rc = flush_all_timing(ix);
        if (rc) return rc;
    }
    if (n == "searches") *value = ix->n_searches.load();
    else if (n == "queries") *value = ix->n_queries.load();
    else if (n == "fallback_queries") *value = ix->n_fallback.load() + (int64_t)dt[0];
    else if (n == "repass_queries") *value = ix->n_repass.load() + (int64_t)dt[3];  // + device re-passes
    else if (n == "searches_q4") *value = ix->n_q4.load();
    else if (n == "searches_wide") *value = ix->n_wide.load();
    else if (n == "auto_hold") *value = ix->auto_hold.load();
    else if (n == "auto_hold8") *value = ix->auto_hold8.load();
    else if (n == "overflow_queries") *value = ix->n_overflow.load() + (int64_t)dt[1];
    else if (n == "inconsistent_queries") *value = ix->n_incons.load();  // host-memory searches
    else if (n == "capacity") *value = ix->cap_rows;
    else if (n == "scan_ns") *value = ix->scan_ns.load();
    else if (n == "pipeline_ns") *value = ix->pipe_ns.load();
    else if (n == "timed_searches") *value = ix->n_timed.load();
    else if (n == "count") *value = ix->count;
    else if (n == "precision") *value = ix->precision;
    else if (n == "searches_fp32") *value = ix->n_by_prec[PREC_FP32].load();
    else if (n == "searches_bf16x3") *value = ix->n_by_prec[PREC_BF16X3].load();
    else if (n == "searches_bf16") *value = ix->n_by_prec[PREC_BF16].load();
    else if (n == "searches_i8") *value = ix->n_by_prec[PREC_I8].load();
    else if (n == "searches_i8x3") *value = ix->n_by_prec[PREC_I8X3].load();
    else if (n == "auto_int8") *value = ix->auto_i8 ? 1 : 0;
    else if (n == "auto_i8q") *value = ix->auto_i8q ? 1 : 0;
    else if (n == "i8q_off") *value = ix->i8q_off.load() ? 1 : 0;
    else if (n == "searches_i8q") *value = ix->n_by_prec[PREC_I8Q].load();
    else if (n == "i8_wide") *value = ix->i8_wide ? 1 : 0;
    else if (n == "device_bytes") {  // the row buffers actually allocated
        const int64_t xb = (int64_t)(ix->cap_rows / 32) * ix->G * BLOCK_FLOATS * 4;  // fp32 X: 4 B per element
        int64_t cb = 0;  // the numeric columns (vdb_index_set_column), attached or kept for the next attach
        for (int s = 0; s < kFilterSlots; ++s) cb += ix->cols[s] ? ix->col_cap[s] * 8 : 0;
        *value = xb + (xs_ptr(ix) ? xb : 0) + (ix->Xq ? xb / 2 : 0) + (ix->Xh ? xb / 4 : 0) + ix->cap_rows * 20 + cb;
    } else if (n == "split_copy") *value = xs_ptr(ix) ? 1 : 0;
    else if (n == "split_copy_builds") *value = ix->n_xs_builds.load();
    else if (n == "rows_removed") *value = ix->n_rows_removed.load();
    else if (n == "rows_updated") *value = ix->n_rows_updated.load();
    else if (n == "subset_searches") *value = ix->n_subset_searches.load();
    else if (n == "subset_queries") *value = ix->n_subset_queries.load();
    else if (n == "subset_rows") *value = ix->n_subset_rows.load();
    else if (n == "range_searches") *value = ix->n_range_searches.load();
    else if (n == "range_queries") *value = ix->n_range_queries.load();
    else if (n == "column_slots") *value = ix->col_mask;
    else if (n == "column_sets") *value = ix->n_column_sets.load();
    else if (n == "filter_calls") *value = ix->n_filter_calls.load();
    else if (n == "filter_preds") *value = ix->n_filter_preds.load();
    else if (n == "group_rows") *value = ix->group_set ? ix->group_n : 0;
    else if (n == "group_sets") *value = ix->n_group_sets.load();
    else if (n == "group_searches") *value = ix->n_group_searches.load();
    else if (n == "group_queries") *value = ix->n_group_queries.load();
    else if (n == "mmr_searches") *value = ix->n_mmr_searches.load();
    else if (n == "mmr_queries") *value = ix->n_mmr_queries.load();
    else if (n == "recommend_searches") *value = ix->n_rec_searches.load();
    else if (n == "recommend_queries") *value = ix->n_rec_queries.load();
    else if (n == "recommend_bad_queries") {  // counted by the build kernel: after the searches queued so far
        HIP_TRY(hipSetDevice(ix->device));
        const int wr = wait_idle(ix);
        if (wr) return wr;
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpy(&bad, ix->d_xmax + kRecommendBadWord, sizeof(bad), hipMemcpyDeviceToHost));
        *value = (int64_t)bad;
    }
    else if (n == "fused_searches") *value = ix->n_fused_searches.load();
    else if (n == "fused_sets") *value = ix->n_fused_sets.load();
    else if (n == "fused_bad_sets") {  // counted by the fuse kernel: after the searches queued so far
        HIP_TRY(hipSetDevice(ix->device));
        const int wr = wait_idle(ix);
        if (wr) return wr;
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpy(&bad, ix->d_xmax + kFusedBadWord, sizeof(bad), hipMemcpyDeviceToHost));
        *value = (int64_t)bad;
    }
    else if (n == "maxsim_searches") *value = ix->n_maxsim_searches.load();
    else if (n == "maxsim_sets") *value = ix->n_maxsim_sets.load();
    else if (n == "maxsim_bad_sets" || n == "maxsim_skipped_rows") {  // counted by the kernels: after the searches queued so far
        HIP_TRY(hipSetDevice(ix->device));
        const int wr = wait_idle(ix);
        if (wr) return wr;
        unsigned long long c = 0;
        HIP_TRY(hipMemcpy(&c, ix->d_xmax + (n == "maxsim_bad_sets" ? kMaxsimBadWord : kMaxsimSkippedWord), sizeof(c),
                          hipMemcpyDeviceToHost));
        *value = (int64_t)c;
    }
    else if (n == "sparse_rows") *value = ix->sparse_set ? ix->sparse_n : 0;
    else if (n == "sparse_nnz") *value = ix->sparse_set ? ix->sparse_nnz : 0;
    else if (n == "sparse_sets") *value = ix->n_sparse_sets.load();
    else if (n == "sparse_searches") *value = ix->n_sparse_searches.load();
    else if (n == "sparse_queries") *value = ix->n_sparse_queries.load();
    else if (n == "hybrid_searches") *value = ix->n_hybrid_searches.load();
    else if (n == "hybrid_queries") *value = ix->n_hybrid_queries.load();
    else if (n == "hybrid_sum_searches") *value = ix->n_hybsum_searches.load();
    else if (n == "hybrid_sum_queries") *value = ix->n_hybsum_queries.load();
    else if (n == "sparse_bad_queries") {  // counted by the sparse kernel: after the searches queued so far
        HIP_TRY(hipSetDevice(ix->device));
        const int wr = wait_idle(ix);
        if (wr) return wr;
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpy(&bad, ix->d_xmax + kSparseBadWord, sizeof(bad), hipMemcpyDeviceToHost));
        *value = (int64_t)bad;
    }
    else if (n == "group_fallback_queries") {  // counted by the select kernel: after the searches queued so far
        unsigned long long fb = 0;
        if (ix->d_group_fb) {
            HIP_TRY(hipSetDevice(ix->device));
            const int wr = wait_idle(ix);
            if (wr) return wr;
            HIP_TRY(hipMemcpy(&fb, ix->d_group_fb, sizeof(fb), hipMemcpyDeviceToHost));
        }
        *value = (int64_t)fb;
    }
    else if (n == "subset_bad_ids") {  // counted by the kernel: after the row-list searches queued so far
        HIP_TRY(hipSetDevice(ix->device));
        const int wr = wait_idle(ix);
        if (wr) return wr;
        unsigned long long bad = 0;
        HIP_TRY(hipMemcpy(&bad, ix->d_xmax + kSubsetBadWord, sizeof(bad), hipMemcpyDeviceToHost));
        *value = (int64_t)bad;
    }
    else return set_error(VDB_ERR_INVALID, "unknown stat '%s'", name);
    return VDB_OK;
}

// Rows [row0, row0 + n) were just packed: on the first add, fix the residual direction
// (normalised column sums of up to kDirRows of these rows; a host round trip, once per
// index); then the maximum of |dir . (y - bf16(y))| over these rows (d_xmax[3]).
constexpr int64_t kDirRows = 65536;

// On the first add also the int8 copy's centring row mu (the mean of the same rows) and its
// quantisation step sx = 1.25 max |y - mu| / 127 over them (vdb_scan8.hip): this runs before
// the candidate copy of the first rows is built.
static hipError_t setup_direction(vdb_index* ix, int64_t row0, int64_t n, hipStream_t st) {
    if (ix->dir_set) return hipSuccess;
    const float* inv = ix->metric == VDB_METRIC_COSINE ? ix->inv32 : nullptr;
    const int D = ix->dim;
    const int64_t m = std::min(n, kDirRows);
    hipError_t e = hipSuccess;
    if (!ix->d_dir) e = hipMalloc(&ix->d_dir, (size_t)ix->Dp * sizeof(float));
    if (e == hipSuccess && !ix->d_mu) e = hipMalloc(&ix->d_mu, (size_t)ix->Dp * sizeof(float));
    double* sums = nullptr;
    if (e == hipSuccess) e = hipMalloc(&sums, (size_t)D * sizeof(double));
    if (e == hipSuccess) e = hipMemsetAsync(sums, 0, (size_t)D * sizeof(double), st);
    if (e == hipSuccess) e = launch_dir_sum(ix->X, inv, row0, m, D, ix->G, sums, st);
    std::vector<double> h(D);
    if (e == hipSuccess) e = hipMemcpyAsync(h.data(), sums, (size_t)D * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (sums) (void)hipFree(sums);
    if (e != hipSuccess) return e;
    double nn = 0.0;
    for (double v : h) nn += v * v;
    std::vector<float> dir(ix->Dp, 0.0f), mu(ix->Dp, 0.0f);
    if (nn > 0.0 && std::isfinite(nn))
        for (int d = 0; d < D; ++d) dir[d] = (float)(h[d] / std::sqrt(nn));
    for (int d = 0; d < D; ++d) mu[d] = (float)(h[d] / (double)std::max<int64_t>(m, 1));
    e = hipMemcpyAsync(ix->d_dir, dir.data(), (size_t)ix->Dp * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ix->d_mu, mu.data(), (size_t)ix->Dp * sizeof(float), hipMemcpyHostToDevice, st);
    uint32_t zb = 0;
    uint32_t* dz = reinterpret_cast<uint32_t*>(ix->d_i8 + 6);
    if (e == hipSuccess) e = hipMemsetAsync(dz, 0, sizeof(uint32_t), st);
    if (e == hipSuccess) e = launch_zmax(ix->X, inv, ix->d_mu, row0, m, D, ix->G, dz, st);
    if (e == hipSuccess) e = hipMemcpyAsync(&zb, dz, sizeof(zb), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // dir / mu are stack buffers
    if (e != hipSuccess) return e;
    float zmax = 0.0f;
    std::memcpy(&zmax, &zb, sizeof(zmax));
    ix->sx = zmax > 0.0f && std::isfinite(zmax) ? 1.25f * zmax / 127.0f : 1.0f;
    ix->dir_rows = m;
    ix->dir_set = true;
    return hipSuccess;
}

static hipError_t residual_direction(vdb_index* ix, int64_t row0, int64_t n, hipStream_t st) {
    const float* inv = ix->metric == VDB_METRIC_COSINE ? ix->inv32 : nullptr;
    return launch_resid_dir(ix->X, inv, row0, n, ix->dim, ix->G, ix->d_dir, ix->d_xmax + 3, st);
}

int32_t vdb_index_add(vdb_index* ix, const float* vectors, int64_t n, int32_t mem, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (n < 0) return set_error(VDB_ERR_INVALID, "n must be >= 0");
    if (n == 0) return VDB_OK;
    if (!vectors) return set_error(VDB_ERR_INVALID, "vectors is NULL");
    if (ix->count + n > (int64_t)0xFFFFFFFE) return set_error(VDB_ERR_INVALID, "index is limited to 2^32-2 rows");
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_lock<std::shared_mutex> g(ix->mu);
    hipStream_t st = ix->stream;
    int rc = ensure_capacity(ix, ix->count + n);
    if (rc) return rc;
    // While the direction / centring row / int8 step still come from fewer than kDirRows rows,
    // this add may derive them again and rebuild the int8 copy of rows [0, count) in place
    // (below): device-memory searches still running on caller streams read those buffers
    // together with host-captured scalars (sx, i8st) -- wait for them first.  Past
    // that phase an add only writes rows >= count, which no queued search reads.
    if (ix->count > 0 && ix->dir_rows < kDirRows) {
        const int wr = wait_idle(ix);
        if (wr) return wr;
    }
    HIP_TRY(hipMemsetAsync(ix->d_nonfinite, 0, sizeof(int), st));
    // snapshot of the row statistics the kernels below raise over the new rows: a rejected add
    // puts them back (its rows must leave no trace in any statistic or column sum)
    char* bak = reinterpret_cast<char*>(ix->d_xmax);
    HIP_TRY(hipMemcpyAsync(bak + 64, ix->d_xmax, 32, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(bak + 128, ix->d_i8, 64, hipMemcpyDeviceToDevice, st));
    if (mem == VDB_MEM_DEVICE) {
        // the rows may still be being written on the caller's stream (NULL = the null stream):
        // ingest (on the index's own stream) starts after that work
        HIP_TRY(order_after_caller(st, stream));
    }
    const int D = ix->dim;
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(256ll << 20) / ((int64_t)D * 4));
    float* staging = nullptr;
    if (mem == VDB_MEM_HOST) HIP_TRY(hipMalloc(&staging, (size_t)std::min(chunk, n) * D * sizeof(float)));
    for (int64_t r = 0; r < n; r += chunk) {
        const int64_t m = std::min(chunk, n - r);
        const float* src = vectors + r * D;
        if (mem == VDB_MEM_HOST) {
            hipError_t e = hipMemcpyAsync(staging, src, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice, st);
            if (e == hipSuccess)
                e = launch_pack_rows(staging, m, D, ix->G, ix->X, ix->count + r, ix->nrm64, ix->inv32, ix->sq32,
                                     ix->rinit32, ix->metric == VDB_METRIC_COSINE, ix->d_xmax, ix->d_nonfinite, st);
            if (e == hipSuccess) e = setup_direction(ix, ix->count + r, m, st);
            if (e == hipSuccess) e = build_candidate_rows(ix, ix->count + r, m, st);
            if (e == hipSuccess) e = residual_direction(ix, ix->count + r, m, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);  // staging reuse
            if (e != hipSuccess) {
                (void)hipFree(staging);
                return set_error(VDB_ERR_HIP, "ingest failed: %s", hipGetErrorString(e));
            }
        } else {
            HIP_TRY(launch_pack_rows(src, m, D, ix->G, ix->X, ix->count + r, ix->nrm64, ix->inv32, ix->sq32,
                                     ix->rinit32, ix->metric == VDB_METRIC_COSINE, ix->d_xmax, ix->d_nonfinite, st));
            HIP_TRY(setup_direction(ix, ix->count + r, m, st));
            HIP_TRY(build_candidate_rows(ix, ix->count + r, m, st));
            HIP_TRY(residual_direction(ix, ix->count + r, m, st));
        }
    }
    if (staging) (void)hipFree(staging);  // ingest runs on the index's own stream (serialised with growth)
    int nonfinite = 0;
    unsigned long long xb[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(&nonfinite, ix->d_nonfinite, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(xb, ix->d_xmax, sizeof(xb), hipMemcpyDeviceToHost, st));
    HIP_TRY(read_i8_stats(ix, st));
    if (nonfinite) {
        // rows past `count` are never read; the next add overwrites them.  A rejected first add
        // leaves no direction / centring row behind (they would hold its non-finite values).
        if (ix->count == 0) {
            ix->dir_set = false;
            ix->dir_rows = 0;
            HIP_TRY(hipMemsetAsync(ix->d_xmax, 0, 32, st));
            HIP_TRY(hipMemsetAsync(ix->d_i8, 0, 64, st));
            HIP_TRY(hipStreamSynchronize(st));
            std::memset(ix->i8st, 0, sizeof(ix->i8st));
        } else {
            // the rejected rows' statistics and column sums came in with them: the maxima and the
            // int8 statistics go back to the snapshot, the column sums are rebuilt over [0, count)
            HIP_TRY(hipMemcpyAsync(ix->d_xmax, bak + 64, 32, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipMemcpyAsync(ix->d_i8, bak + 128, 64, hipMemcpyDeviceToDevice, st));
            if (ix->Xq && needs_i8(ix->precision, ix->auto_i8)) {
                HIP_TRY(hipMemsetAsync(ix->d_csum, 0, (size_t)2 * ix->Dp * sizeof(uint32_t), st));
                HIP_TRY(launch_colsum8(ix->Xq, 0, ix->count, ix->G / 4, ix->d_csum, st));
            }
            HIP_TRY(read_i8_stats(ix, st));  // (synchronises)
        }
        return set_error(VDB_ERR_NONFINITE, "%d row(s) contain NaN or Inf; nothing was added", nonfinite);
    }
    // Direction, centring row and quantisation step from a few rows (a store filled one REST add
    // at a time) would stay poor for good: while they came from fewer than kDirRows rows, they
    // are derived again from all rows each time the index doubles, and the int8 copy and the
    // residual maxima along dir are rebuilt (O(kDirRows) work in total).
    if (ix->dir_rows < kDirRows && ix->count + n >= 2 * ix->dir_rows) {
        const int64_t all = ix->count + n;
        ix->dir_set = false;
        HIP_TRY(hipMemsetAsync(ix->d_xmax + 3, 0, 8, st));
        HIP_TRY(hipMemsetAsync(ix->d_i8, 0, 64, st));
        HIP_TRY(setup_direction(ix, 0, all, st));
        if (needs_i8(ix->precision, ix->auto_i8)) HIP_TRY(build_candidate_rows(ix, 0, all, st, false, true));
        HIP_TRY(residual_direction(ix, 0, all, st));
        HIP_TRY(hipMemcpyAsync(xb, ix->d_xmax, sizeof(xb), hipMemcpyDeviceToHost, st));
        HIP_TRY(read_i8_stats(ix, st));
    }
    double xm[4];
    std::memcpy(xm, xb, sizeof(xm));
    ix->xmax = xm[0];
    ix->xres_rel = xm[1];
    ix->xres_abs = xm[2];
    ix->xres_dir = xm[3];
    ix->count += n;
    ix->group_set = false;  // the group column covered the old rows only
    ix->sparse_set = false;  // and so did the sparse column
    ix->col_mask = 0;        // and the numeric columns
    ix->auto_hold = 0;  // new rows: VDB_PREC_AUTO tries the one-plane passes again
    ix->auto_fails = 0;
    ix->auto_hold8 = 0;
    ix->auto_fails8 = 0;
    // device-memory failures already landed belong to the old rows: they start no hold
    if (ix->h_totals) ix->auto_seen = ix->h_totals[0];
    return VDB_OK;
}

int32_t vdb_index_count(const vdb_index* ix, int64_t* n) {
    if (!ix || !n) return set_error(VDB_ERR_INVALID, "NULL argument");
    *n = ix->count;
    return VDB_OK;
}

// vdb_index_clear under the exclusive lock (also the end of a remove that leaves no row).
static int32_t clear_locked(vdb_index* ix) {
    {
        const int wr = wait_idle(ix);
        if (wr) return wr;
    }
    if (ix->X) {
        HIP_TRY(hipMemsetAsync(ix->X, 0, (size_t)(ix->cap_rows / 32) * ix->G * BLOCK_FLOATS * sizeof(float),
                               ix->stream));
        HIP_TRY(hipMemsetAsync(ix->nrm64, 0, ix->cap_rows * sizeof(double), ix->stream));
        if (ix->Xs)
            HIP_TRY(hipMemsetAsync(ix->Xs, 0, (size_t)(ix->cap_rows / 32) * ix->G * BLOCK_FLOATS * sizeof(float),
                                   ix->stream));
        if (ix->Xq)
            HIP_TRY(hipMemsetAsync(ix->Xq, 0, (size_t)(ix->cap_rows / 32) * ix->G * BLOCK_FLOATS * sizeof(float) / 2,
                                   ix->stream));
    }
    HIP_TRY(hipMemsetAsync(ix->d_xmax, 0, 64, ix->stream));
    HIP_TRY(hipMemsetAsync(ix->d_i8, 0, 64, ix->stream));
    HIP_TRY(hipMemsetAsync(ix->d_csum, 0, (size_t)2 * ix->Dp * sizeof(uint32_t), ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    std::memset(ix->i8st, 0, sizeof(ix->i8st));
    ix->count = 0;
    ix->group_set = false;
    ix->sparse_set = false;
    ix->col_mask = 0;
    ix->auto_hold = 0;
    ix->auto_fails = 0;
    ix->auto_hold8 = 0;
    ix->auto_fails8 = 0;
    ix->xmax = 0.0;
    ix->xres_rel = ix->xres_abs = 0.0;
    ix->dir_set = false;  // the next add picks a new direction (xres_dir's bits were cleared above)
    ix->dir_rows = 0;
    ix->xres_dir = 0.0;
    ix->gen++;
    return VDB_OK;
}

int32_t vdb_index_clear(vdb_index* ix) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_lock<std::shared_mutex> g(ix->mu);
    return clear_locked(ix);
}

int32_t vdb_index_remove(vdb_index* ix, const uint32_t* remove_mask, int32_t mem, void* stream, int64_t* n_removed) {
    if (n_removed) *n_removed = 0;
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (!remove_mask) return set_error(VDB_ERR_INVALID, "remove_mask is NULL");
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    if (N == 0) return VDB_OK;
    // queued device-memory searches on caller streams read the buffers the rows move in
    {
        const int wr = wait_idle(ix);
        if (wr) return wr;
    }
    hipStream_t st = ix->stream;
    const int64_t n_words = remove_mask_words(N);
    // one allocation: [the mask's device copy (host masks)] base [n_words + 1], part, info
    const size_t mask_bytes = mem == VDB_MEM_HOST ? ((size_t)n_words * sizeof(uint32_t) + 255) & ~size_t(255) : 0;
    char* scan = nullptr;
    HIP_TRY(hipMalloc(&scan, mask_bytes + remove_scan_bytes(n_words)));
    RemoveScratch scr{nullptr, nullptr, nullptr, nullptr, nullptr};
    auto done = [&](int rc) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(scan);
        if (scr.X) (void)hipFree(scr.X);
        return rc;
    };
#define RM_TRY(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return done(set_error(_e == hipErrorOutOfMemory ? VDB_ERR_OOM : VDB_ERR_HIP, "remove: %s failed: %s", \
                                  #expr, hipGetErrorString(_e)));                                      \
    } while (0)
    const uint32_t* md = remove_mask;
    if (mem == VDB_MEM_HOST) {
        RM_TRY(hipMemcpyAsync(scan, remove_mask, (size_t)n_words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        md = reinterpret_cast<const uint32_t*>(scan);
    } else {
        // the mask may still be being written on the caller's stream (NULL = the null stream)
        RM_TRY(order_after_caller(st, stream));
    }
    Carver c{scan, mask_bytes};
    uint32_t* base = c.take<uint32_t>((size_t)n_words + 1);
    uint32_t* part = c.take<uint32_t>((size_t)((n_words + kScanWgWords - 1) / kScanWgWords));
    uint32_t* info = c.take<uint32_t>(2);
    RM_TRY(launch_remove_scan(md, n_words, N, base, part, info, st));
    uint32_t h_info[2] = {0, 0};
    RM_TRY(hipMemcpyAsync(h_info, info, sizeof(h_info), hipMemcpyDeviceToHost, st));
    RM_TRY(hipStreamSynchronize(st));
    const int64_t kept = (int64_t)h_info[0];
    if (kept > N || (kept < N && (int64_t)h_info[1] >= n_words))
        return done(set_error(VDB_ERR_HIP, "remove: inconsistent scan (kept %lld of %lld)", (long long)kept, (long long)N));
    if (kept == N) return done(VDB_OK);  // no bit set below count: nothing is touched
    if (kept == 0) {                     // every row: the index is left as a clear leaves it
        const int rc = done(clear_locked(ix));
        if (rc == VDB_OK) {
            ix->n_rows_removed += N;
            if (n_removed) *n_removed = N;
        }
        return rc;
    }
    // the gather, chunk by chunk in ascending order from the first word that loses a row
    const int64_t first_word = (int64_t)h_info[1];
    const int64_t cw = std::min(remove_chunk_words(ix->remove_chunk, ix->Dp), n_words - first_word);
    const int64_t crows = cw * 32;
    {
        // (each carve starts 256-B aligned: the rows, then the four scalar arrays)
        const size_t sbytes = (size_t)crows * ((size_t)ix->Dp * sizeof(float) + kRowScalarBytes) + 5 * 256;
        char* sbuf = nullptr;
        RM_TRY(hipMalloc(&sbuf, sbytes));
        Carver s2{sbuf};
        scr.X = s2.take<float>((size_t)crows * ix->Dp);  // (offset 0: done() frees it through scr.X)
        scr.nrm64 = s2.take<double>((size_t)crows);
        scr.inv32 = s2.take<float>((size_t)crows);
        scr.sq32 = s2.take<float>((size_t)crows);
        scr.rinit32 = s2.take<float>((size_t)crows);
    }
    const RemoveRows rows{ix->X, ix->Dp, ix->nrm64, ix->inv32, ix->sq32, ix->rinit32};
    const int64_t n_chunks = remove_n_chunks(first_word, n_words, cw);
    for (int64_t ci = 0; ci < n_chunks; ++ci) {
        const RemoveChunk k = remove_chunk(first_word, n_words, cw, ci);
        RM_TRY(launch_remove_chunk(rows, md, base, N, k.w0, k.w1, scr, st));
    }
    // the vacated tail: zero, as in an index that never held those rows
    const RemoveTail t = remove_tail(first_word, kept, N);
    const size_t Dp = (size_t)ix->Dp;
    RM_TRY(hipMemsetAsync(ix->X + (size_t)kept * Dp, 0, (size_t)(N - kept) * Dp * sizeof(float), st));
    RM_TRY(hipMemsetAsync(ix->nrm64 + kept, 0, (size_t)(N - kept) * sizeof(double), st));
    RM_TRY(hipMemsetAsync(ix->inv32 + kept, 0, (size_t)(N - kept) * sizeof(float), st));
    RM_TRY(hipMemsetAsync(ix->sq32 + kept, 0, (size_t)(N - kept) * sizeof(float), st));
    RM_TRY(hipMemsetAsync(ix->rinit32 + kept, 0, (size_t)(N - kept) * sizeof(float), st));
    // the candidate copies of the moved rows, from the moved rows and the frozen mu / sx / dir.
    // The tiled copy is rebuilt through its last super tile: X is zero past `kept`, so those
    // tiles come out zero; whole super tiles past it are zeroed directly.  A copy the current
    // precision does not read is not rebuilt (set_param rebuilds [0, count) when a setting
    // starts to read it) but its tail is zeroed all the same.
    const size_t st_bytes = (size_t)(t.st_end - t.tiles_end) * Dp;  // per byte of an element
    if (ix->Xs) {
        if (xs_kind(ix->precision) != kXsNone)
            RM_TRY(build_candidate_rows(ix, t.rebuild0, t.tiles_end - t.rebuild0, st, true, false));
        else if (kept % 128)
            RM_TRY(hipMemsetAsync(reinterpret_cast<char*>(ix->Xs) + (size_t)(kept / 128 * 128) * Dp * 4, 0,
                                  (size_t)128 * Dp * 4, st));
        if (st_bytes) RM_TRY(hipMemsetAsync(reinterpret_cast<char*>(ix->Xs) + (size_t)t.tiles_end * Dp * 4, 0, st_bytes * 4, st));
    }
    if (ix->Xq) {
        RM_TRY(launch_zero_rows8(ix->Xq, kept, t.rowz_end - kept, ix->G / 4, st));
        if (st_bytes) RM_TRY(hipMemsetAsync(reinterpret_cast<char*>(ix->Xq) + (size_t)t.tiles_end * Dp * 2, 0, st_bytes * 2, st));
        if (ix->Xh) RM_TRY(hipMemsetAsync(ix->Xh + (size_t)kept * Dp, 0, (size_t)(N - kept) * Dp, st));
        if (needs_i8(ix->precision, ix->auto_i8)) {
            // the column sums start again: rows below the rebuilt range here, the rest as the
            // rebuild adds them (exact integers: they equal the sums over [0, kept))
            RM_TRY(hipMemsetAsync(ix->d_csum, 0, (size_t)2 * Dp * sizeof(uint32_t), st));
            RM_TRY(launch_colsum8(ix->Xq, 0, t.rebuild0, ix->G / 4, ix->d_csum, st));
            if (kept > t.rebuild0) RM_TRY(build_candidate_rows(ix, t.rebuild0, kept - t.rebuild0, st, false, true));
        }
    }
    RM_TRY(hipStreamSynchronize(st));
#undef RM_TRY
    (void)done(VDB_OK);
    ix->count = kept;
    ix->group_set = false;  // the rows moved: the group column no longer lines up
    ix->sparse_set = false;  // nor does the sparse column
    ix->col_mask = 0;        // nor do the numeric columns
    ix->gen++;
    ix->n_rows_removed += N - kept;
    ix->auto_hold = 0;  // the rows changed: VDB_PREC_AUTO tries the one-plane passes again
    ix->auto_fails = 0;
    ix->auto_hold8 = 0;
    ix->auto_fails8 = 0;
    if (ix->h_totals) ix->auto_seen = ix->h_totals[0];
    if (n_removed) *n_removed = N - kept;
    return VDB_OK;
}

int32_t vdb_index_update(vdb_index* ix, const int64_t* rows, const float* vectors, int64_t n, int32_t mem,
                         void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (n < 0) return set_error(VDB_ERR_INVALID, "n must be >= 0");
    if (n == 0) return VDB_OK;
    if (!rows || !vectors) return set_error(VDB_ERR_INVALID, "rows or vectors is NULL");
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    if (n > N) return set_error(VDB_ERR_INVALID, "%lld distinct rows of %lld cannot be updated", (long long)n, (long long)N);
    // queued device-memory searches on caller streams read the rows this call overwrites
    {
        const int wr = wait_idle(ix);
        if (wr) return wr;
    }
    hipStream_t st = ix->stream;
    const int D = ix->dim;
    const int64_t by_bytes = std::max<int64_t>(1, (int64_t)(256ll << 20) / ((int64_t)D * 4));
    const int64_t chunk = std::min(n, ix->update_chunk > 0 ? ix->update_chunk : by_bytes);
    const bool host = mem == VDB_MEM_HOST;
    // one allocation: the repeat bitmap, the flags and (host-memory arguments) one staging chunk
    // of ids and rows
    const size_t n_words = (size_t)((N + 31) / 32);
    const size_t bytes = n_words * sizeof(uint32_t) + 4 * sizeof(uint32_t) +
                         (host ? (size_t)chunk * ((size_t)D * sizeof(float) + sizeof(int64_t)) : 0) + 4 * 256;
    char* buf = nullptr;
    HIP_TRY(hipMalloc(&buf, bytes));
    auto done = [&](int rc) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(buf);
        return rc;
    };
#define UP_TRY(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return done(set_error(_e == hipErrorOutOfMemory ? VDB_ERR_OOM : VDB_ERR_HIP, "update: %s failed: %s", \
                                  #expr, hipGetErrorString(_e)));                                      \
    } while (0)
    Carver c{buf};
    uint32_t* bitmap = c.take<uint32_t>(n_words);
    uint32_t* flags = c.take<uint32_t>(4);
    int64_t* s_ids = host ? c.take<int64_t>((size_t)chunk) : nullptr;
    float* s_rows = host ? c.take<float>((size_t)chunk * D) : nullptr;
    if (!host) {
        // the ids and rows may still be being written on the caller's stream (NULL = the null stream)
        UP_TRY(order_after_caller(st, stream));
    }
    // chunk [r, r + m) of the call on the device: staged (host memory; the staging is free again
    // once the stream has run what read it) or where the caller put it
    const int64_t* d_ids = nullptr;
    const float* d_rows = nullptr;
    auto stage = [&](int64_t r, int64_t m) -> hipError_t {
        if (!host) {
            d_ids = rows + r;
            d_rows = vectors + r * D;
            return hipSuccess;
        }
        hipError_t e = hipMemcpyAsync(s_ids, rows + r, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync(s_rows, vectors + r * D, (size_t)m * D * sizeof(float), hipMemcpyHostToDevice, st);
        d_ids = s_ids;
        d_rows = s_rows;
        return e;
    };
    // 1. validation, before the first write: range, repeats, finiteness
    UP_TRY(hipMemsetAsync(bitmap, 0, n_words * sizeof(uint32_t), st));
    UP_TRY(hipMemsetAsync(flags, 0, 4 * sizeof(uint32_t), st));
    for (int64_t r = 0; r < n; r += chunk) {
        const int64_t m = std::min(chunk, n - r);
        UP_TRY(stage(r, m));
        UP_TRY(launch_update_validate(d_ids, d_rows, m, D, N, bitmap, flags, st));
        if (host && r + m < n) UP_TRY(hipStreamSynchronize(st));  // staging reuse
    }
    uint32_t h_flags[4] = {0, 0, 0, 0};
    UP_TRY(hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, st));
    UP_TRY(hipStreamSynchronize(st));
    if (h_flags[0])
        return done(set_error(VDB_ERR_INVALID, "update: a row id is outside [0, %lld); nothing was updated", (long long)N));
    if (h_flags[1]) return done(set_error(VDB_ERR_INVALID, "update: a row id is given more than once; nothing was updated"));
    if (h_flags[2])
        return done(set_error(VDB_ERR_NONFINITE, "%u row(s) contain NaN or Inf; nothing was updated", h_flags[2]));
    // 2. the apply, for the updated rows only, with mu / sx / dir as they are
    const float* inv = ix->metric == VDB_METRIC_COSINE ? ix->inv32 : nullptr;
    const bool i8 = ix->Xq && needs_i8(ix->precision, ix->auto_i8);
    const int kind = ix->Xs ? xs_kind(ix->precision) : kXsNone;
    const int G8 = ix->G / 4;
    UP_TRY(hipMemsetAsync(ix->d_nonfinite, 0, sizeof(int), st));
    for (int64_t r = 0; r < n; r += chunk) {
        const int64_t m = std::min(chunk, n - r);
        if (n > chunk || !host) UP_TRY(stage(r, m));  // (a single host chunk is still staged)
        // the old bytes leave the column sums before they are overwritten
        if (i8) UP_TRY(launch_update_colsum8(ix->Xq, d_ids, m, N, G8, -1, ix->d_csum, st));
        UP_TRY(launch_update_pack_rows(d_rows, d_ids, m, N, D, ix->G, ix->X, ix->nrm64, ix->inv32, ix->sq32,
                                       ix->rinit32, ix->metric == VDB_METRIC_COSINE, ix->d_xmax, ix->d_nonfinite, st));
        if (kind == kXsFp32) UP_TRY(launch_update_tile_rows(ix->X, ix->G, d_ids, m, N, ix->Xs, st));
        if (kind == kXsSplit) UP_TRY(launch_update_split_rows(ix->X, ix->G, d_ids, m, N, inv, ix->Xs, st));
        if (i8) {
            UP_TRY(launch_update_quant_rows(ix->X, inv, ix->d_mu, ix->d_dir, ix->sx, d_ids, m, N, ix->G, ix->Xq,
                                            ix->d_i8, ix->Xh, st));
            UP_TRY(launch_update_colsum8(ix->Xq, d_ids, m, N, G8, +1, ix->d_csum, st));
        }
        UP_TRY(launch_update_resid_dir(ix->X, inv, d_ids, m, N, D, ix->G, ix->d_dir, ix->d_xmax + 3, st));
        if (host && r + m < n) UP_TRY(hipStreamSynchronize(st));  // staging reuse
    }
    unsigned long long xb[4] = {0, 0, 0, 0};
    UP_TRY(hipMemcpyAsync(xb, ix->d_xmax, sizeof(xb), hipMemcpyDeviceToHost, st));
    UP_TRY(read_i8_stats(ix, st));  // (synchronises)
#undef UP_TRY
    (void)done(VDB_OK);
    double xm[4];
    std::memcpy(xm, xb, sizeof(xm));
    ix->xmax = xm[0];
    ix->xres_rel = xm[1];
    ix->xres_abs = xm[2];
    ix->xres_dir = xm[3];
    ix->gen++;
    ix->n_rows_updated += n;
    ix->auto_hold = 0;  // the rows changed: VDB_PREC_AUTO tries the one-plane passes again
    ix->auto_fails = 0;
    ix->auto_hold8 = 0;
    ix->auto_fails8 = 0;
    if (ix->h_totals) ix->auto_seen = ix->h_totals[0];
    return VDB_OK;
}

int32_t vdb_index_get_vectors(vdb_index* ix, int64_t start, int64_t n, float* out_host) {
    if (!ix || (!out_host && n > 0)) return set_error(VDB_ERR_INVALID, "NULL argument");
    if (start < 0 || n < 0 || start + n > ix->count)
        return set_error(VDB_ERR_INVALID, "rows [%lld, %lld) out of range [0, %lld)", (long long)start,
                         (long long)(start + n), (long long)ix->count);
    if (n == 0) return VDB_OK;
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int D = ix->dim;
    const int64_t chunk = std::max<int64_t>(1, (int64_t)(256ll << 20) / ((int64_t)D * 4));
    float* tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, (size_t)std::min(chunk, n) * D * sizeof(float)));
    for (int64_t r = 0; r < n; r += chunk) {
        const int64_t m = std::min(chunk, n - r);
        hipError_t e = launch_unpack_rows(ix->X, ix->G, D, start + r, m, tmp, ix->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(out_host + r * D, tmp, (size_t)m * D * sizeof(float), hipMemcpyDeviceToHost, ix->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
        if (e != hipSuccess) {
            (void)hipFree(tmp);
            return set_error(VDB_ERR_HIP, "export failed: %s", hipGetErrorString(e));
        }
    }
    (void)hipFree(tmp);
    return VDB_OK;
}

// vdb_index_search with an optional global id per row (row_ids, device memory, read by
// the result write-out): a shard of a multi-device set holds pieces of the global
// insertion order (vdb_shards_*).
// search_impl's answer when VDB_PREC_AUTO's bf16 pass left too many queries uncertified in a
// host-memory search: nothing was written, the caller runs the search again in bf16x3 (two
// candidate passes cost far less than the exact scan of most of the batch)
constexpr int32_t kRetryBf16x3 = 1 << 20;
// A host-memory bf16 search re-passes its uncertified queries in bf16x3 (gathered into one
// device-memory sub-search) when they are at most 1/8 of the batch and at most this many.
constexpr int kRepassMax = 64;
// Device-memory searches (device_repass): up to kRepassDev (vdb_search_plan.h) uncertified queries
// of a batch take a gated sub-search on the device; auto arms the re-pass for this many searches
// after a device fallback was seen.
constexpr int kRepassArm = 256;
// VDB_PREC_AUTO uses the bf16 pass up to this k (its KP = next_pow2(k + 112) stays 128)
constexpr int kAutoBf16MaxK = 16;

// VDB_PREC_AUTO bookkeeping (vdb_index::auto_hold): a bf16 failure too large for a re-pass
// starts a hold of bf16x3 searches, doubling per failed probe (16 .. 2048).
void auto_fail(vdb_index* ix) {
    const int f = std::min(8, ix->auto_fails.load() + 1);
    ix->auto_fails = f;
    ix->auto_ok = 0;
    ix->auto_hold = 16 << (f - 1);
}

// The precision class of the next auto search: bf16x3 while a hold lasts.
bool auto_take_hold(vdb_index* ix) {
    int h = ix->auto_hold.load();
    while (h > 0)
        if (ix->auto_hold.compare_exchange_weak(h, h - 1)) return true;
    if (++ix->auto_ok >= 64) ix->auto_fails = 0;  // probes have been certifying for a while
    return false;
}

// The same pair for the I8 -> BF16 hold (vdb_index::auto_hold8).
void auto_fail8(vdb_index* ix) {
    const int f = std::min(8, ix->auto_fails8.load() + 1);
    ix->auto_fails8 = f;
    ix->auto_ok8 = 0;
    ix->auto_hold8 = 16 << (f - 1);
}
bool auto_take_hold8(vdb_index* ix) {
    int h = ix->auto_hold8.load();
    while (h > 0)
        if (ix->auto_hold8.compare_exchange_weak(h, h - 1)) return true;
    if (++ix->auto_ok8 >= 64) ix->auto_fails8 = 0;
    return false;
}

static int32_t search_locked(vdb_index* ix, const float* queries, int32_t B, int32_t k, const uint32_t* row_mask,
                             int32_t mem, float* out_scores, int64_t* out_indices, double* out_keys,
                             int64_t index_offset, void* stream, const int64_t* row_ids, struct SearchOpts opt);

// The uncertified queries flag_list[0..n) (device) of a bf16 search, gathered into a
// device-memory bf16x3 sub-search on the same stream (its own certificate and gated exact
// fallback), whose result rows are scattered back into the batch's outputs.
static int repass_flagged(vdb_index* ix, const float* Qd, const int* flag_list, int n, int k, const uint32_t* md,
                          float* out_s, int64_t* out_i, double* out_k, int64_t index_offset, const int64_t* row_ids,
                          hipStream_t st);

struct SearchOpts {
    bool force_b3 = false;  // VDB_PREC_AUTO: this search runs bf16x3 (retry / re-pass)
    bool repass = false;    // an internal sub-search of a re-pass (no search / query counts)
    // device re-pass: the sub-search's query count lives on the device (B is its capacity);
    // its candidate pass and finish are gated on it, and it runs without a pilot
    const int* gate = nullptr;
    bool force_i8x3 = false;  // the re-pass in I8X3 (the int8 copy's two planes: half BF16X3's bytes)
};

static int32_t search_locked(vdb_index* ix, const float* queries, int32_t B, int32_t k, const uint32_t* row_mask,
                             int32_t mem, float* out_scores, int64_t* out_indices, double* out_keys,
                             int64_t index_offset, void* stream, const int64_t* row_ids, SearchOpts opt);

static int32_t search_impl(vdb_index* ix, const float* queries, int32_t B, int32_t k, const uint32_t* row_mask,
                           int32_t mem, float* out_scores, int64_t* out_indices, double* out_keys,
                           int64_t index_offset, void* stream, const int64_t* row_ids, bool force_b3 = false) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (B <= 0) return set_error(VDB_ERR_INVALID, "n_queries must be >= 1, got %d", B);
    if (k <= 0 || k > 1024) return set_error(VDB_ERR_INVALID, "k must be in [1, 1024], got %d", k);
    if (!queries || !out_scores || !out_indices) return set_error(VDB_ERR_INVALID, "NULL query/output pointer");
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    if (mem == VDB_MEM_HOST && !all_finite(queries, (int64_t)B * ix->dim))
        return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    SearchOpts opt;
    opt.force_b3 = force_b3;
    return search_locked(ix, queries, B, k, row_mask, mem, out_scores, out_indices, out_keys, index_offset, stream,
                         row_ids, opt);
}

static int repass_flagged(vdb_index* ix, const float* Qd, const int* flag_list, int n, int k, const uint32_t* md,
                          float* out_s, int64_t* out_i, double* out_k, int64_t index_offset, const int64_t* row_ids,
                          hipStream_t st) {
    const int D = ix->dim;
    const size_t qb = round_up((int64_t)n * D * 4, 256), sb = round_up((int64_t)n * k * 4, 256),
                 lb = round_up((int64_t)n * k * 8, 256);
    char* buf = nullptr;
    HIP_TRY(hipMallocAsync((void**)&buf, qb + sb + 2 * lb, st));
    float* Qs = (float*)buf;
    float* ss = (float*)(buf + qb);
    int64_t* si = (int64_t*)(buf + qb + sb);
    double* sk = (double*)(buf + qb + sb + lb);
    hipError_t e = launch_gather_rows(Qd, D, flag_list, n, Qs, st);
    int rc = e == hipSuccess ? VDB_OK : set_error(VDB_ERR_HIP, "re-pass gather: %s", hipGetErrorString(e));
    if (rc == VDB_OK) {
        SearchOpts o;
        o.force_b3 = true;
        o.repass = true;
        rc = search_locked(ix, Qs, n, k, md, VDB_MEM_DEVICE, ss, si, sk, index_offset, st, row_ids, o);
    }
    if (rc == VDB_OK) {
        e = launch_scatter_results(flag_list, n, k, ss, si, sk, out_s, out_i, out_k, st);
        if (e != hipSuccess) rc = set_error(VDB_ERR_HIP, "re-pass scatter: %s", hipGetErrorString(e));
    }
    (void)hipFreeAsync(buf, st);
    ix->n_repass += n;
    return rc;
}

// The search itself (the caller holds the index's shared lock).
static int32_t search_locked(vdb_index* ix, const float* queries, int32_t B, int32_t k, const uint32_t* row_mask,
                             int32_t mem, float* out_scores, int64_t* out_indices, double* out_keys,
                             int64_t index_offset, void* stream, const int64_t* row_ids, SearchOpts opt) {
    const int D = ix->dim;
    const int64_t N = ix->count;
    if (!opt.repass) {
        ix->n_searches++;
        ix->n_queries += B;
    }

    // ---- the precision policy (stateful: VDB_PREC_AUTO's holds and re-pass bookkeeping) ----
    const bool auto_prec = ix->precision == VDB_PREC_AUTO;
    if (auto_prec && ix->h_totals && !opt.repass) {  // fallbacks of earlier device-memory searches (lagged)
        const unsigned long long seen = ix->h_totals[0];
        const unsigned long long prev = ix->auto_seen.exchange(seen);
        if (seen > prev) {
            if (ix->last_i8q && seen - prev > (unsigned long long)std::max(1, ix->last_i8q_b.load() / 8))
                ix->i8q_off = true;
            if (ix->last_i8) {
                auto_fail8(ix);
                ix->i8_wide = true;
            } else {
                auto_fail(ix);
            }
            ix->repass_arm = kRepassArm;  // device_repass auto: re-pass on the device for a while
        }
    }
    const bool approx = N > 0 && !(ix->force_exact || k > kMaxApproxK);
    // AUTO takes bf16x3 directly where bf16's wider certificate needs KP = 256 (k > 16): that
    // pass runs 32-query blocks at twice the query-operand traffic and measured 3x slower than
    // bf16x3 (C4, k = 100: 13 vs 3.9 ms, profiles/r02s_ab/s4_c4_str2.json), and in device memory
    // its uncertified queries cost the exact path
    const bool auto_b16 = k <= kAutoBf16MaxK;
    // AUTO keeps both copies with auto_i8: the one-plane pass is I8 unless an I8 hold is on
    // (then BF16); the k > 16 pass is I8X3 unless an I8 hold is on (then BF16X3) -- with the
    // insertion by pass-bit masks I8X3 runs C4 / C3 / C2 at 2.89 / 1.42 / 0.28 ms against BF16X3's
    // 3.41 / 2.17 / 0.47 (profiles/r03_i8/c4prec, x3prec); holds, re-passes and retries stay
    // BF16X3 (per-element relative precision: no dependence on the rows' range)
    const bool x3_i8 = auto_prec && !opt.force_b3 && !auto_b16 && ix->auto_i8;
    const bool auto_x3 = auto_prec && (opt.force_b3 || !auto_b16 || (approx && auto_take_hold(ix)));
    const bool hold8 = auto_prec && ix->auto_i8 && approx && (x3_i8 || !auto_x3) && auto_take_hold8(ix);
    const bool auto_8 = auto_prec && !auto_x3 && ix->auto_i8 && !hold8;
    const bool auto_8x3 = x3_i8 && !hold8;
    // L2, 16 < k <= 100: the xh plane against the 16-bit query (two MFMAs per group, half the
    // corpus bytes of I8X3; its 8-bit corpus bound certifies at KP = 256)
    const bool auto_8q = auto_8x3 && ix->metric == 1 && k <= 100 && ix->auto_i8q && !ix->i8q_off;
    const bool force_8x3 = auto_prec && opt.force_i8x3 && ix->auto_i8 && ix->Xq;
    const int prec_req = !ix->X ? PREC_FP32
                         : force_8x3 ? PREC_I8X3
                         : ix->precision == VDB_PREC_BF16X3 ? PREC_BF16X3
                         : ix->precision == VDB_PREC_BF16 ? PREC_BF16
                         : ix->precision == VDB_PREC_I8X3 ? PREC_I8X3
                         : ix->precision == VDB_PREC_I8Q ? PREC_I8Q
                         : ix->precision == VDB_PREC_I8 ? PREC_I8
                         : auto_prec ? (auto_x3 ? (auto_8x3 ? (auto_8q ? PREC_I8Q : PREC_I8X3) : PREC_BF16X3)
                                                 : auto_8 ? PREC_I8 : PREC_BF16)
                                     : PREC_FP32;
    if (auto_prec && approx && (!auto_x3 || x3_i8)) {
        ix->last_i8 = auto_8 || auto_8x3;
        ix->last_i8q = prec_req == PREC_I8Q;
        ix->last_i8q_b = (int)B;
    }
    // (a device re-pass's gated sub-search is counted by the device: repass_queries)
    if (approx && !opt.gate) ix->n_by_prec[prec_req]++;
    // the "one plane" precisions (a wide certificate: KP = 128 for small k) and their re-pass
    const bool one_plane = prec_req == PREC_BF16 || prec_req == PREC_I8;

    // ---- the plan (vdb_search_plan.h): pure arithmetic from here to the launches ----
    const int prec = prec_req;
    SearchShape sh{};
    sh.B = B; sh.k = k; sh.D = D; sh.Dp = ix->Dp; sh.G = ix->G; sh.metric = ix->metric; sh.N = N; sh.n_cu = ix->n_cu;
    sh.prec = prec; sh.host = mem == VDB_MEM_HOST; sh.gated = opt.gate != nullptr; sh.repass = opt.repass;
    const SearchKnobs kn = search_knobs(ix, auto_prec && ix->i8_narrow != 0 && !ix->i8_wide);
    const SearchKP kp = search_kp(sh, kn);
    const int KP = kp.KP;
    const bool exact_all = kp.exact_all;
    if (!prec_is_i8(prec) && !exact_all && N > 0 && !xs_ptr(ix)) {  // a split pass under AUTO + int8: the lazy copy
        const int xr = ensure_xs(ix);
        if (xr) return xr;
    }
    const SearchGeometry g = search_geometry(sh, kn, kp, kernel_facts(sh, kn, kp));
    const SearchPilot pilot = search_pilot(sh, kn, kp, g);
    const SearchLayout lay = search_layout(sh, g, pilot);
    const bool i8_pass = g.i8_pass, split_pass = g.split_pass, q4 = g.q4, wide_long = g.wide_long, wide8 = g.wide8;
    const bool priv = g.priv, i8_refine = g.i8_refine, chk = g.chk, chk_l = g.chk_l;
    const int Gs = g.Gs, n_seg8 = g.n_seg8, QB = g.QB, QB_pilot = g.QB_pilot, Bp = g.Bp, n_qblocks = g.n_qblocks;
    const int variant = g.variant, n_wg = g.n_wg, spw = g.spw, lockstep = g.lockstep, n_wg8 = g.n_wg8;
    const int fin_split = g.fin_split, R_rep = g.R_rep, n_pilot = pilot.n_pilot, pilot_rank = pilot.pilot_rank;
    const int64_t n_steps = g.n_steps, mask_words = g.mask_words, gl_cap = g.gl_cap;

    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;
    int rc = ws_reserve(w, (size_t)lay.total, st);
    if (rc) return rc;
    char* const dev = w->dev;
    auto at = [dev](int64_t off) { return off < 0 ? nullptr : dev + off; };  // (-1: no such buffer in this call)
    float* Qraw = (float*)at(lay.Qraw);
    uint32_t* maskd = (uint32_t*)at(lay.maskd);
    float* Qt = (float*)at(lay.Qt);
    double* qn64 = (double*)at(lay.qn64);
    double* qconst = (double*)at(lay.qconst);
    // the finish's centring row and residual direction (the same conditions as its arguments below)
    const float* q_mu = i8_pass ? ix->d_mu : nullptr;
    const float* q_dir = (prec == PREC_BF16 || i8_pass) && ix->dir_set && !ix->no_dir_bound ? ix->d_dir : nullptr;
    float* os = (float*)at(lay.os);
    int64_t* oi = (int64_t*)at(lay.oi);
    double* ok = (double*)at(lay.ok);
    int* flags = (int*)at(lay.flags);
    int* done = (int*)at(lay.done);
    uint32_t* gthr = (uint32_t*)at(lay.gthr);
    uint32_t* gslots = (uint32_t*)at(lay.gslots);
    uint32_t* pslots = gslots + (size_t)Bp * KP_MAX;
    float* gl_s = (float*)at(lay.gl_s);
    uint32_t* gl_i = (uint32_t*)at(lay.gl_i);
    uint32_t* gl_cnt = (uint32_t*)at(lay.gl_cnt);
    double* fx_ek = (double*)at(lay.fx_ek);
    uint32_t* fx_ck = (uint32_t*)at(lay.fx_ck);
    uint32_t* fx_cr = (uint32_t*)at(lay.fx_cr);
    int* fx_n = (int*)at(lay.fx_n);
    float* q8max = (float*)at(lay.q8max);
    float* q8lsl = (float*)at(lay.q8lsl);
    float* q8err = (float*)at(lay.q8err);
    float* q8scal = (float*)at(lay.q8scal);
    float* q8res = (float*)at(lay.q8res);
    float* q8err2 = (float*)at(lay.q8err2);
    uint32_t* chkp = (uint32_t*)at(lay.chkp);
    uint32_t* segc = (uint32_t*)at(lay.segc);
    uint32_t* chkr = (uint32_t*)at(lay.chkr);
    int* rs8 = (int*)at(lay.rs8);
    uint32_t* chke = (uint32_t*)at(lay.chke);
    float* rep_q = (float*)at(lay.rep_q);
    float* rep_s = (float*)at(lay.rep_s);
    int64_t* rep_i = (int64_t*)at(lay.rep_i);
    double* rep_k = (double*)at(lay.rep_k);

    const float* Qd = queries;
    const uint32_t* md = row_mask;
    float* out_s = out_scores;
    int64_t* out_i = out_indices;
    double* out_k = out_keys;
    // host memory: the queries go up and the results come down through the workspace's pinned
    // staging (asynchronous copies; the results are read in the same synchronisation as the
    // certificate's flags, and copied out on the host when nothing was flagged)
    const size_t io_q = mem == VDB_MEM_HOST ? (size_t)B * D * 4 : 0;
    const size_t io_r = (size_t)B * k * (4 + 8 + (out_keys ? 8 : 0));
    bool staged = false;
    if (mem == VDB_MEM_HOST) {
        rc = ws_host_io(w, io_q + io_r);
        if (rc) return rc;
        std::memcpy(w->host_io, queries, io_q);
        HIP_TRY(hipMemcpyAsync(Qraw, w->host_io, io_q, hipMemcpyHostToDevice, st));
        Qd = Qraw;
        if (row_mask && N > 0) {
            HIP_TRY(hipMemcpyAsync(maskd, row_mask, (size_t)mask_words * 4, hipMemcpyHostToDevice, st));
            md = maskd;
        }
        out_s = os;
        out_i = oi;
        out_k = out_keys ? ok : nullptr;
    }

    if (N == 0) {
        // empty store: every slot "no result" (reference returns ([],[],[]), :117), keys -inf
        // like every other invalid entry, so an empty shard's lists rank last in a merge
        HIP_TRY(launch_empty_results((int64_t)B * k, out_s, out_i, out_k, st));
    } else {
        HIP_TRY(launch_prep_queries(Qd, B, Bp, D, ix->G, ix->metric, prec == PREC_FP32 ? Qt : nullptr,
                                    split_pass ? Qt : nullptr, qn64, flags, gthr, gslots, gl_cnt, done, st,
                                    i8_pass ? q8max : nullptr, q_mu, q_dir, qconst));
        if (i8_pass && !exact_all) {
            Int8Consts c8;
            c8.sx = ix->sx;
            c8.zmax_h = ix->i8st[4];
            c8.xl_max = ix->i8st[5];
            c8.rmax_half = 0.5 * ix->xmax * ix->xmax;
            HIP_TRY(launch_prep8(Qd, qn64, q8max, B, Bp, D, Gs, ix->metric, prec, c8, Qt, q8lsl, q8err, q8scal, st,
                                 q8res, q8err2));
            if (rs8) {  // L2: the start values at this batch's scale (+ their sum, the checksum's)
                if (chkr) HIP_TRY(hipMemsetAsync(chkr, 0, sizeof(uint32_t), st));
                HIP_TRY(launch_rstart8(ix->rinit32, N, q8scal, rs8, chkr, st));
            }
        }
        int n_flag = 0;
        if (!exact_all) {
            const bool timed = ix->timing != 0 && !opt.gate;  // a gated sub-search may not run at all
            hipEvent_t* tev = nullptr;
            if (timed) {
                if (w->t_pending == Workspace::kTRing) {  // ring full: read the oldest set
                    const int frc = flush_timing(ix, w, 1);
                    if (frc) return frc;
                }
                tev = w->tring[w->t_head];
                w->t_head = (w->t_head + 1) % Workspace::kTRing;
                w->t_pending++;
                for (int e = 0; e < 4; ++e)
                    if (!tev[e]) HIP_TRY(hipEventCreate(&tev[e]));
                HIP_TRY(hipEventRecord(tev[3], st));
            }
            const float* rowscale = ix->metric == 0 ? ix->inv32 : ix->sq32;
            const float* Xscan = i8_pass ? ix->Xq : xs_ptr(ix);  // the copy this pass reads
            if (n_pilot > 0) {
                if (i8_pass) {
                    HIP_TRY(launch_pilot8(prec, ix->metric, Xscan, ix->rinit32, md, Qt, q8scal, Gs, N, B,
                                          (B + QB_pilot - 1) / QB_pilot, QB_pilot, n_pilot, pslots, st,
                                          chke ? ix->d_csum : nullptr, chke, wide_long));
                    HIP_TRY(launch_pilot_bound(pslots, B, pilot_rank, gthr, st));
                } else if (split_pass) {
                    HIP_TRY(launch_pilot2(prec, ix->metric, pilot_rank, Xscan, ix->rinit32, md, Qt, Gs, N, B,
                                          (B + QB_pilot - 1) / QB_pilot, QB_pilot, n_pilot, pslots, gthr, st));
                    HIP_TRY(launch_pilot_bound(pslots, B, pilot_rank, gthr, st));
                }
                else
                    HIP_TRY(launch_pilot(prec, ix->metric, pilot_rank, Xscan, rowscale, md, Qt, Gs, N, B,
                                         n_qblocks, QB, n_pilot, pslots, gthr, st));
            }
            // scan_ns times the scan kernel alone (the roofline's kernel); pipeline_ns
            // everything from the pilot to the rerank
            if (opt.gate && (q4 || !(split_pass || i8_pass)))  // only these passes are gated
                return set_error(VDB_ERR_INVALID, "device re-pass: the sub-search has no gated candidate pass");
            if (timed) HIP_TRY(hipEventRecord(tev[0], st));
            if (q4) ix->n_q4++;
            if (wide8) ix->n_wide++;
            if (wide_long)
                HIP_TRY(launch_scan8wl(prec, ix->metric, Xscan, md, Qt, q8lsl, q8scal, Gs, N, B, n_seg8, gl_s, gl_i,
                                       gl_cap, segc, gthr, chkp, st));
            else if (wide8)
                HIP_TRY(launch_scan8w(prec, ix->metric, Xscan, rs8, md, Qt, q8lsl, q8scal, Gs, N, B, Bp, n_seg8, gl_s, gl_i,
                                      gl_cap, segc, gthr, chkp, Bp, chk_l ? 1 : 0, st));
            else if (i8_pass)
                HIP_TRY(launch_scan8(prec, ix->metric, KP, Xscan, (const float*)rs8, md, Qt, q8lsl, q8scal, Gs, N, B,
                                     n_qblocks, n_steps, n_wg, spw, gl_s, gl_i, gl_cnt, gl_cap, gthr, lockstep,
                                     (int)ix->scan_qlds, st, opt.gate, chkp, Bp, chk_l ? 1 : 0));
            else if (split_pass)
                HIP_TRY(launch_scan2(prec, ix->metric, KP, Xscan, ix->rinit32, md, Qt, Gs, N, B, n_qblocks, n_steps,
                                     n_wg, spw, gl_s, gl_i, gl_cnt, gl_cap, gthr, lockstep, st, q4,
                                     (int)ix->scan_qlds, opt.gate));
            else if (priv)
                HIP_TRY(launch_scan_topk_priv(prec, ix->metric, KP, Xscan, rowscale, md, Qt, Gs, N, B, n_qblocks,
                                              n_steps, n_wg, spw, gl_s, gl_i, gl_cnt, gl_cap, gthr, gslots, st));
            else
                HIP_TRY(launch_scan_topk(prec, ix->metric, KP, variant, Xscan, rowscale, md, Qt, Gs, N, B, n_qblocks,
                                         n_steps, n_wg, spw, gl_s, gl_i, gl_cnt, gl_cap, gthr, gslots, lockstep, st));
            if (timed) HIP_TRY(hipEventRecord(tev[1], st));
            FinishArgs fa;
            fa.gl_s = gl_s; fa.gl_i = gl_i; fa.gl_cnt = gl_cnt; fa.gl_cap = gl_cap;
            fa.Q = Qd; fa.qn64 = qn64; fa.X = ix->X; fa.G = ix->G; fa.D = D; fa.nrm64 = ix->nrm64; fa.k = k;
            // |approx - exact| <= eps_rel * sum|q_i x_i| (relative to |q||x|):
            //   fp32:   D fp32 MFMA additions + ~8 roundings of the normalisation / scaling
            //   bf16x3: 3D additions (each counted at 2^-23 in case the bf16 MFMA adds
            //           truncate) + the dropped hi*lo-order terms (< 3.1 2^-16) + the same 8
            //   bf16:   2D additions + the query split (2^-16) + the same 8, plus xres: the
            //           corpus rounding |q.(x - bf16(x))| <= |q| |x - bf16(x)|, bounded by the
            //           largest row residual measured at ingest (relative for cosine)
            // int8: exact integer sums; 8 roundings (normalisation, centring, the fp32 combination)
            fa.eps_rel = i8_pass ? 1.01 * 8.0 * std::ldexp(1.0, -24)
                         : prec == PREC_FP32 ? 1.01 * (double)(D + 8) * std::ldexp(1.0, -24)
                         : prec == PREC_BF16X3
                             ? 1.01 * (3.0 * D * std::ldexp(1.0, -23) + 3.1 * std::ldexp(1.0, -16) +
                                       8.0 * std::ldexp(1.0, -24))
                             : 1.01 * (2.0 * D * std::ldexp(1.0, -23) + 1.1 * std::ldexp(1.0, -16) +
                                       8.0 * std::ldexp(1.0, -24));
            fa.xmax = ix->xmax;
            fa.xres = prec != PREC_BF16 ? 0.0 : 1.01 * (ix->metric == 0 ? ix->xres_rel : ix->xres_abs);
            fa.dir = prec == PREC_BF16 && ix->dir_set && !ix->no_dir_bound ? ix->d_dir : nullptr;
            fa.dres = 1.01 * ix->xres_dir;
            if (i8_pass) {  // the int8 copy's rounding of the centred rows (absolute: cosine rows are unit)
                fa.xres = 1.01 * ix->i8st[prec == PREC_I8X3 ? 2 : 0] + 1e-300;  // (I8 / I8Q: the xh plane's)
                fa.dir = ix->dir_set && !ix->no_dir_bound ? ix->d_dir : nullptr;
                fa.dres = 1.01 * ix->i8st[prec == PREC_I8X3 ? 3 : 1];
                fa.qerr = q8err;
                fa.mu = ix->d_mu;
                if (i8_refine) {
                    fa.xh_rm = ix->Xh;
                    fa.qres = q8res;
                    fa.qerr2 = q8err2;
                    fa.qscal = q8scal;
                    fa.sx = ix->sx;
                    fa.Dp = ix->Dp;
                }
            }
            fa.out_s = out_s; fa.out_i = out_i; fa.out_k = out_k; fa.index_offset = index_offset;
            fa.row_ids = row_ids;
            fa.flag_count = flags; fa.flag_list = flags + 1; fa.gthr = gthr; fa.overflow_count = flags + B + 1;
            fa.incons_count = flags + B + 2;
            fa.gate = opt.gate;
            if (chk) {
                fa.chkp = chkp;
                fa.chke = chke;
                fa.chkr = chkr;
                fa.chk_q = Qt;
                fa.chk_csum = ix->d_csum;
                fa.chk_g8 = Gs;
                fa.chk_nw = n_wg8;
                fa.chk_ld = Bp;
                fa.chk_l = chk_l;
            }
            fa.qconst = fa.mu == q_mu && fa.dir == q_dir ? qconst : nullptr;  // (prep_queries' constants)
            fa.seg_cnt = segc;
            fa.seg_n = n_seg8;
            // auto: batches of >= 32 (throughput: C2 under three streams 437 -> 453 K QPS, the finish
            // beside the next batch's scan), not single queries (one batch alone its 4 waves are
            // slower: C2 B = 2 step 0.195 -> 0.217 ms; B = 64 p50 0.213 -> 0.240; profiles/r06_fs)
            // (and with the short-row wide pass, <= 128 dims: beside its small stage for <= 256
            // queries; for C4's 512 three workgroups per CU instead of one, 366 -> 374 K QPS,
            // profiles/r06_c4f);
            // auto also only while another search of the index is in flight: a batch alone keeps the
            // 16-wave form (its latency, the bench's p50)
            fa.small = D <= 1024 && (ix->finish_small == 1 ||
                                     (ix->finish_small < 0 && B >= 32 &&
                                      ((wide_long && Gs <= 32) || (wide8 && !wide_long)) &&
                                      others_in_flight(ix, w))) ? 1 : 0;
            fa.split = fin_split; fa.sx_ek = fx_ek; fa.sx_ck = fx_ck; fa.sx_cr = fx_cr; fa.sx_n = fx_n; fa.done = done;
            HIP_TRY(launch_finish(ix->metric, KP, fa, B, st));
            if (timed) HIP_TRY(hipEventRecord(tev[2], st));
            // Device-memory searches do not wait for the certificate: the exact path is
            // launched gated on the device's flag count (nothing runs when no query was
            // flagged), so the call returns with the whole search queued.
            if (ix->no_fallback && mem == VDB_MEM_DEVICE) return VDB_OK;
            if (!ix->no_fallback && mem == VDB_MEM_DEVICE && gated_exact_bytes(ix, B, k) <= kGatedExactBytes) {
                {
                    std::lock_guard<std::mutex> lg(ix->ws_mu);  // lazily, once (concurrent searches)
                    if (!ix->d_totals) {
                        HIP_TRY(hipHostMalloc(&ix->h_totals, 2 * sizeof(unsigned long long), hipHostMallocDefault));
                        ix->h_totals[0] = ix->h_totals[1] = 0;
                        unsigned long long* d = nullptr;
                        // flagged, overflowed, flagged in a one-plane pass, re-passed on the device
                        HIP_TRY(hipMalloc(&d, 4 * sizeof(unsigned long long)));
                        // zeroed and COMPLETE before any search stream can use it: a plain hipMemset
                        // runs on the null stream, which a non-blocking caller stream does not order
                        // after -- the first search's device re-pass count could land before the
                        // zeroing and be wiped (GPUTEST_r04: repass_queries 2 of 3 on a side stream)
                        HIP_TRY(zero_now(d, 4 * sizeof(unsigned long long), ix->stream));
                        ix->d_totals = d;
                    }
                }
                unsigned long long* htot =
                    auto_prec && (one_plane || prec == PREC_I8X3 || prec == PREC_I8Q) ? ix->h_totals : nullptr;
                // The device re-pass: up to kRepassDev uncertified queries gathered on the
                // device into a BF16X3 sub-search on this stream, gated on their count (its candidate
                // pass and finish exit at once when nothing was flagged), its rows scattered back;
                // the rest, if any, take the gated exact path.  Like the host re-pass (repass_flagged)
                // for auto's one-plane / I8X3 passes, with the split copy kept beside the int8 one.
                const bool can_rep = !opt.repass && auto_prec && (one_plane || prec == PREC_I8X3 || prec == PREC_I8Q) &&
                                     xs_kind(VDB_PREC_BF16X3) == xs_kind(ix->precision) && rep_q &&
                                     k <= kMaxApproxK;
                bool rep = can_rep && ix->device_repass == 1;
                if (can_rep && ix->device_repass < 0) {
                    int a = ix->repass_arm.load();
                    while (a > 0 && !ix->repass_arm.compare_exchange_weak(a, a - 1)) {}
                    rep = a > 0;
                }
                if (rep) {
                    int* counts = flags + B + 3;  // [0] gathered (the sub-search's gate), [1] left over
                    HIP_TRY(launch_repass_gather(Qd, D, flags, R_rep, rep_q, counts, ix->d_totals + 3, st));
                    SearchOpts o;
                    o.force_b3 = true;
                    o.force_i8x3 = true;  // (I8X3 where the int8 copy is kept, else BF16X3)
                    o.repass = true;
                    o.gate = counts;
                    rc = search_locked(ix, rep_q, R_rep, k, md, VDB_MEM_DEVICE, rep_s, rep_i, rep_k, index_offset, st,
                                       row_ids, o);
                    if (rc) return rc;
                    HIP_TRY(launch_scatter_results(flags + 1, R_rep, k, rep_s, rep_i, rep_k, out_s, out_i, out_k, st,
                                                   counts));
                    if (B > R_rep)
                        rc = run_exact(ix, w, Qd, qn64, flags + 1 + R_rep, B - R_rep, k, md, out_s, out_i, out_k,
                                       index_offset, row_ids, st, counts + 1, flags + B + 1, done + R_rep, htot);
                    return rc;
                }
                rc = run_exact(ix, w, Qd, qn64, flags + 1, B, k, md, out_s, out_i, out_k, index_offset, row_ids, st,
                               flags, flags + B + 1, done, htot);
                return rc;
            }
            HIP_TRY(hipMemcpyAsync(w->host_flag, flags, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(w->host_flag + 1, flags + B + 1, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
            if (mem == VDB_MEM_HOST) {  // (valid when nothing was flagged: nothing rewrites them then)
                char* r = w->host_io + io_q;
                HIP_TRY(hipMemcpyAsync(r, out_s, (size_t)B * k * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(r + (size_t)B * k * 4, out_i, (size_t)B * k * 8, hipMemcpyDeviceToHost, st));
                if (out_keys)
                    HIP_TRY(hipMemcpyAsync(r + (size_t)B * k * 12, out_k, (size_t)B * k * 8, hipMemcpyDeviceToHost, st));
            }
            HIP_TRY(hipStreamSynchronize(st));
            n_flag = w->host_flag[0];
            staged = mem == VDB_MEM_HOST && n_flag == 0;
            if (prec == PREC_I8 && n_flag > 0) ix->i8_wide = true;
            ix->n_overflow += w->host_flag[1];
            ix->n_incons += w->host_flag[2];
            if (auto_prec && one_plane && n_flag > 0 && !ix->no_fallback) {
                if (n_flag <= std::max(1, B / 8) && n_flag <= kRepassMax) {
                    // a few uncertified queries: re-pass just those in bf16x3 (the index stays bf16)
                    if (timed) {
                        const int frc = flush_timing(ix, w);
                        if (frc) return frc;
                    }
                    rc = repass_flagged(ix, Qd, flags + 1, n_flag, k, md, out_s, out_i, out_k, index_offset,
                                        row_ids, st);
                    if (rc) return rc;
                    n_flag = 0;
                } else {
                    if (prec == PREC_I8) auto_fail8(ix);
                    else auto_fail(ix);
                    ix->n_searches--;  // the retry counts this search (no double count)
                    ix->n_queries -= B;
                    return kRetryBf16x3;
                }
            }
            // auto's I8X3 pass: a failure the size of the one-plane passes' retries holds BF16X3
            // for the next searches (this batch's uncertified queries take the exact path below)
            if (auto_prec && prec == PREC_I8X3 && n_flag > std::max(1, B / 8) && !ix->no_fallback) auto_fail8(ix);
            // auto's I8Q pass: such a failure turns it off for this index (I8X3 from then on)
            if (auto_prec && prec == PREC_I8Q && n_flag > std::max(1, B / 8) && !ix->no_fallback) ix->i8q_off = true;
            if (timed) {
                const int frc = flush_timing(ix, w);
                if (frc) return frc;
            }
            if (n_flag > 0 && !ix->no_fallback) {
                ix->n_fallback += n_flag;
                rc = run_exact(ix, w, Qd, qn64, flags + 1, n_flag, k, md, out_s, out_i, out_k, index_offset, row_ids,
                               st);
                if (rc) return rc;
            }
        } else {
            ix->n_fallback += B;
            rc = run_exact(ix, w, Qd, qn64, nullptr, B, k, md, out_s, out_i, out_k, index_offset, row_ids, st);
            if (rc) return rc;
        }
    }
    if (mem == VDB_MEM_HOST && staged) {
        const char* r = w->host_io + io_q;
        std::memcpy(out_scores, r, (size_t)B * k * 4);
        std::memcpy(out_indices, r + (size_t)B * k * 4, (size_t)B * k * 8);
        if (out_keys) std::memcpy(out_keys, r + (size_t)B * k * 12, (size_t)B * k * 8);
    } else if (mem == VDB_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out_scores, out_s, (size_t)B * k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_indices, out_i, (size_t)B * k * 8, hipMemcpyDeviceToHost, st));
        if (out_keys) HIP_TRY(hipMemcpyAsync(out_keys, out_k, (size_t)B * k * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return VDB_OK;
}

int32_t vdb_shutdown(void) {
    std::vector<vdb_index*> live;
    {
        std::lock_guard<std::mutex> rg(g_reg_mu);
        live.assign(g_indices.begin(), g_indices.end());
    }
    std::set<int> devices;
    for (vdb_index* ix : live) {
        HIP_TRY(hipSetDevice(ix->device));
        devices.insert(ix->device);
        {
            const int wr = wait_idle(ix);  // every queued search of this index is done
            if (wr) return wr;
        }
        const int frc = flush_all_timing(ix);
        if (frc) return frc;
        std::lock_guard<std::mutex> g(ix->ws_mu);
        for (Workspace* w : ix->pool)
            if (!w->busy) free_workspace_memory(w);
    }
    for (int d : devices) {  // stream-ordered allocations (merge / graph scratch) back to the driver
        HIP_TRY(hipSetDevice(d));
        hipMemPool_t pool = nullptr;
        if (hipDeviceGetDefaultMemPool(&pool, d) == hipSuccess && pool) (void)hipMemPoolTrimTo(pool, 0);
    }
    return VDB_OK;
}

int32_t vdb_index_search_rows(vdb_index* ix, const float* queries, int32_t B, int32_t k, const int64_t* list_offsets,
                              int32_t n_lists, const int64_t* list_rows, int64_t n_ids, const int32_t* query_list,
                              int32_t mem, float* out_scores, int64_t* out_indices, double* out_keys,
                              int64_t index_offset, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (B == 0) return VDB_OK;
    if (B < 0) return set_error(VDB_ERR_INVALID, "n_queries must be >= 0, got %d", B);
    if (k <= 0 || k > 1024) return set_error(VDB_ERR_INVALID, "k must be in [1, 1024], got %d", k);
    if (!queries || !out_scores || !out_indices) return set_error(VDB_ERR_INVALID, "NULL query/output pointer");
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    if (n_lists < 0 || n_ids < 0) return set_error(VDB_ERR_INVALID, "n_lists and n_ids must be >= 0");
    if (!list_offsets || (n_ids > 0 && !list_rows)) return set_error(VDB_ERR_INVALID, "NULL list pointer");
    if (!query_list && n_lists != B)
        return set_error(VDB_ERR_INVALID, "without a query_list n_lists (%d) must equal n_queries (%d)", n_lists, B);
    const int D = ix->dim;
    if (mem == VDB_MEM_HOST && !all_finite(queries, (int64_t)B * D))
        return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    if (mem == VDB_MEM_HOST) {  // everything checked before any launch
        int64_t at = 0;
        switch (subset_validate(list_offsets, n_lists, list_rows, n_ids, query_list, B, N, &at)) {
            case kSubsetOk: break;
            case kSubsetBadOffsets:
                return set_error(VDB_ERR_INVALID, "list_offsets[%lld] = %lld: offsets must ascend from >= 0 to <= n_ids (%lld)",
                                 (long long)at, (long long)list_offsets[at], (long long)n_ids);
            case kSubsetBadId:
                return set_error(VDB_ERR_INVALID, "list_rows[%lld] = %lld is outside [0, %lld)", (long long)at,
                                 (long long)list_rows[at], (long long)N);
            case kSubsetUnsorted:
                return set_error(VDB_ERR_INVALID, "list_rows[%lld] = %lld: a list must be strictly ascending", (long long)at,
                                 (long long)list_rows[at]);
            case kSubsetBadQueryList:
                return set_error(VDB_ERR_INVALID, "query_list[%lld] = %d is outside [0, %d)", (long long)at,
                                 query_list[at], n_lists);
            default:
                return set_error(VDB_ERR_INVALID, "without a query_list n_lists must equal n_queries");
        }
    }
    // as a search: the caller's stream (device memory: NULL = the null stream), or for a
    // host-memory call without one the stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool host = mem == VDB_MEM_HOST;
    const int KE = subset_ke(k);
    const int n_seg = N > 0 ? subset_n_seg(ix->subset_wgs, n_ids, B, n_lists, ix->n_cu) : 1;
    const SubsetScratch sc = subset_scratch(B, D, k, n_seg, n_lists, n_ids, host, query_list != nullptr, out_keys != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    SubsetArgs a{};
    a.Q = queries;
    a.offs = list_offsets;
    a.rows = list_rows;
    a.qlist = query_list;
    a.out_s = out_scores;
    a.out_i = out_indices;
    a.out_k = out_keys;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            std::memcpy(h + (sc.q - sc.in0), queries, (size_t)B * D * 4);
            std::memcpy(h + (sc.offs - sc.in0), list_offsets, ((size_t)n_lists + 1) * 8);
            if (n_ids > 0) std::memcpy(h + (sc.rows - sc.in0), list_rows, (size_t)n_ids * 8);
            if (query_list) std::memcpy(h + (sc.qlist - sc.in0), query_list, (size_t)B * 4);
        });
        if (rc) return rc;
        a.Q = reinterpret_cast<const float*>(dev + sc.q);
        a.offs = reinterpret_cast<const int64_t*>(dev + sc.offs);
        a.rows = reinterpret_cast<const int64_t*>(dev + sc.rows);
        a.qlist = query_list ? reinterpret_cast<const int32_t*>(dev + sc.qlist) : nullptr;
        a.out_s = reinterpret_cast<float*>(dev + sc.out_s);
        a.out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        a.out_k = out_keys ? reinterpret_cast<double*>(dev + sc.out_k) : nullptr;
    }
    if (N == 0) {  // an empty index: every slot "no result", as a search
        HIP_TRY(launch_empty_results((int64_t)B * k, a.out_s, a.out_i, a.out_k, st));
    } else {
        double* qn64 = reinterpret_cast<double*>(dev + sc.qn64);
        int* done = reinterpret_cast<int*>(dev + sc.done);
        // the canonical query norms and the zeroed per-query counters, nothing else: no query tiles
        HIP_TRY(launch_prep_queries(a.Q, B, B, D, ix->G, ix->metric, nullptr, nullptr, qn64, nullptr, nullptr, nullptr,
                                    nullptr, done, st));
        a.qn64 = qn64;
        a.X = ix->X;
        a.G = ix->G;
        a.D = D;
        a.nrm64 = ix->nrm64;
        a.count = N;
        a.n_lists = n_lists;
        a.n_ids = n_ids;
        a.k = k;
        a.KE = KE;
        a.lk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.lk) : nullptr;
        a.li = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.li) : nullptr;
        a.mk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.mk) : nullptr;
        a.mi = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.mi) : nullptr;
        a.done = done;
        a.bad = ix->d_xmax + kSubsetBadWord;
        a.index_offset = index_offset;
        HIP_TRY(launch_subset_search(ix->metric, a, B, n_seg, st));
    }
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)B * k * 4);
        std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)B * k * 8);
        if (out_keys) std::memcpy(out_keys, r + (sc.out_k - sc.out0), (size_t)B * k * 8);
    }
    ix->n_subset_searches++;
    ix->n_subset_queries += B;
    ix->n_subset_rows += n_ids;
    return VDB_OK;
}

int32_t vdb_index_search_range(vdb_index* ix, const float* queries, int32_t B, const double* thresholds,
                               const uint32_t* row_mask, int32_t mem, int64_t cap, int64_t* out_counts,
                               int64_t* out_indices, float* out_scores, double* out_keys, int64_t index_offset,
                               void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (B == 0) return VDB_OK;
    if (B < 0) return set_error(VDB_ERR_INVALID, "n_queries must be >= 0, got %d", B);
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    if (range_validate_cap(B, cap))
        return set_error(VDB_ERR_INVALID, "cap must be >= 0 and n_queries * cap <= %lld, got cap %lld for %d queries",
                         (long long)kRangeMaxSlots, (long long)cap, B);
    if (!queries || !thresholds || !out_counts) return set_error(VDB_ERR_INVALID, "NULL query/threshold/count pointer");
    if (cap > 0 && (!out_indices || !out_scores))
        return set_error(VDB_ERR_INVALID, "out_indices and out_scores are required when cap > 0");
    const int D = ix->dim;
    const bool host = mem == VDB_MEM_HOST;
    if (host) {  // everything checked before any launch
        if (!all_finite(queries, (int64_t)B * D)) return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
        int64_t at = 0;
        switch (range_validate(ix->metric, thresholds, B, &at)) {
            case kRangeNanThreshold: return set_error(VDB_ERR_INVALID, "thresholds[%lld] is NaN", (long long)at);
            case kRangeNegRadius:
                return set_error(VDB_ERR_INVALID, "thresholds[%lld] = %g: a euclidean radius must be >= 0", (long long)at,
                                 thresholds[at]);
            default: break;
        }
    }
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    // as vdb_index_search_rows: the caller's stream (device memory: NULL = the null stream), or for
    // a host-memory call without one the stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const RangeScratch sc = range_scratch(B, D, ix->Dp, N, cap, host, masked, out_keys != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    RangeArgs a{};
    a.Q = queries;
    a.thr = thresholds;
    a.mask = masked ? row_mask : nullptr;
    a.out_c = out_counts;
    a.out_i = out_indices;
    a.out_s = out_scores;
    a.out_k = out_keys;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            std::memcpy(h + (sc.q - sc.in0), queries, (size_t)B * D * 4);
            std::memcpy(h + (sc.thr - sc.in0), thresholds, (size_t)B * 8);
            if (masked) std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.n_words * 4);
        });
        if (rc) return rc;
        a.Q = reinterpret_cast<const float*>(dev + sc.q);
        a.thr = reinterpret_cast<const double*>(dev + sc.thr);
        a.mask = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        a.out_c = reinterpret_cast<int64_t*>(dev + sc.out_c);
        a.out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        a.out_s = reinterpret_cast<float*>(dev + sc.out_s);
        a.out_k = out_keys ? reinterpret_cast<double*>(dev + sc.out_k) : nullptr;
    }
    if (cap == 0) a.out_i = nullptr, a.out_s = nullptr, a.out_k = nullptr;
    if (N == 0) {  // an empty index: counts 0 and every slot "no result"
        HIP_TRY(hipMemsetAsync(a.out_c, 0, (size_t)B * 8, st));
        if (cap > 0) HIP_TRY(launch_empty_results((int64_t)B * cap, a.out_s, a.out_i, a.out_k, st));
    } else {
        double* qn64 = reinterpret_cast<double*>(dev + sc.qn64);
        // the canonical query norms, nothing else: no query tiles
        HIP_TRY(launch_prep_queries(a.Q, B, B, D, ix->G, ix->metric, nullptr, nullptr, qn64, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, st));
        a.qn64 = qn64;
        a.X = ix->X;
        a.G = ix->G;
        a.D = D;
        a.nrm64 = ix->nrm64;
        a.N = N;
        a.H = reinterpret_cast<uint32_t*>(dev + sc.H);
        a.part = reinterpret_cast<uint32_t*>(dev + sc.part);
        a.cnt = reinterpret_cast<int64_t*>(dev + sc.cnt);
        a.cap = cap;
        a.index_offset = index_offset;
        // block after block on this stream over the same scratch
        for (int b0 = 0; b0 < B; b0 += sc.block)
            HIP_TRY(launch_range_block(ix->metric, a, b0, std::min(sc.block, B - b0), st));
    }
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_counts, r + (sc.out_c - sc.out0), (size_t)B * 8);
        if (cap > 0) {
            std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)B * cap * 8);
            std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)B * cap * 4);
            if (out_keys) std::memcpy(out_keys, r + (sc.out_k - sc.out0), (size_t)B * cap * 8);
        }
    }
    ix->n_range_searches++;
    ix->n_range_queries += B;
    return VDB_OK;
}

int32_t vdb_index_set_groups(vdb_index* ix, const int32_t* groups, int64_t n, int32_t mem, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_lock<std::shared_mutex> g(ix->mu);
    if (!group_set_ok(groups != nullptr, n, ix->count))
        return set_error(VDB_ERR_INVALID, groups ? "the group column has %lld rows, the index %lld"
                                                 : "a NULL group column detaches: n must be 0 (got %lld)",
                         (long long)n, (long long)ix->count);
    // queued device-memory searches on caller streams read the column this call replaces
    {
        const int wr = wait_idle(ix);
        if (wr) return wr;
    }
    if (!groups) {  // detach
        ix->group_set = false;
        return VDB_OK;
    }
    hipStream_t st = ix->stream;
    const int64_t n_words = (n + 31) / 32;
    if (n > ix->group_cap || !ix->groups) {  // (+ 64 words: the candidate passes read whole mask tiles)
        const int64_t cap = round_up(std::max<int64_t>(n, 1), kRowAlign);
        int32_t* gnew = nullptr;
        uint32_t* vnew = nullptr;
        HIP_TRY(hipMalloc(&gnew, (size_t)cap * sizeof(int32_t)));
        const hipError_t e = hipMalloc(&vnew, (size_t)(cap / 32 + 64) * sizeof(uint32_t));
        if (e != hipSuccess) {
            (void)hipFree(gnew);
            HIP_TRY(e);
        }
        if (ix->groups) (void)hipFree(ix->groups);
        if (ix->group_valid) (void)hipFree(ix->group_valid);
        ix->groups = gnew;
        ix->group_valid = vnew;
        ix->group_cap = cap;
        ix->group_set = false;
    }
    if (!ix->d_group_fb) {
        HIP_TRY(hipMalloc(&ix->d_group_fb, 2 * sizeof(unsigned long long)));
        HIP_TRY(zero_now(ix->d_group_fb, 2 * sizeof(unsigned long long), st));
    }
    ix->group_set = false;  // until the new column and its bitmap are whole
    unsigned long long* n_valid = ix->d_group_fb + 1;
    if (n > 0) {
        if (mem == VDB_MEM_DEVICE) {
            // the ids may still be being written on the caller's stream: the copy starts after that work
            HIP_TRY(order_after_caller(st, stream));
        }
        HIP_TRY(hipMemcpyAsync(ix->groups, groups, (size_t)n * sizeof(int32_t),
                               mem == VDB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipMemsetAsync(ix->group_valid, 0, (size_t)(ix->group_cap / 32 + 64) * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(n_valid, 0, sizeof(unsigned long long), st));
    HIP_TRY(launch_group_valid(ix->groups, n, ix->group_valid, n_words, n_valid, st));
    unsigned long long nv = 0;
    HIP_TRY(hipMemcpyAsync(&nv, n_valid, sizeof(nv), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    ix->group_valid_rows = (int64_t)nv;
    ix->group_any_neg = (int64_t)nv < n;
    ix->group_n = n;
    ix->group_set = true;
    ix->n_group_sets++;
    return VDB_OK;
}

static_assert(sizeof(vdb_filter_clause) == sizeof(FilterClause) && sizeof(FilterClause) == 24 &&
                  offsetof(vdb_filter_clause, column) == offsetof(FilterClause, column) &&
                  offsetof(vdb_filter_clause, flags) == offsetof(FilterClause, flags) &&
                  offsetof(vdb_filter_clause, lo) == offsetof(FilterClause, lo) &&
                  offsetof(vdb_filter_clause, hi) == offsetof(FilterClause, hi),
              "vdb_filter_clause and FilterClause share one layout");
static_assert(VDB_FILTER_LO_INCL == kFilterLoIncl && VDB_FILTER_HI_INCL == kFilterHiIncl &&
                  VDB_FILTER_NEGATE == kFilterNegate,
              "the flag values of vdb.h and vdb_filter_plan.h agree");

int32_t vdb_index_set_column(vdb_index* ix, int32_t slot, const double* values, int64_t n, int32_t mem, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    if (slot < 0 || slot >= kFilterSlots)
        return set_error(VDB_ERR_INVALID, "slot must be in [0, %d), got %d", kFilterSlots, slot);
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_lock<std::shared_mutex> g(ix->mu);
    if (!filter_column_ok(slot, values != nullptr, n, ix->count))
        return set_error(VDB_ERR_INVALID, values ? "the column has %lld rows, the index %lld"
                                                 : "a NULL column detaches: n must be 0 (got %lld)",
                         (long long)n, (long long)ix->count);
    // queued device-memory calls on caller streams read the column this call replaces
    {
        const int wr = wait_idle(ix);
        if (wr) return wr;
    }
    const uint32_t bit = 1u << slot;
    if (!values) {  // detach
        ix->col_mask &= ~bit;
        return VDB_OK;
    }
    hipStream_t st = ix->stream;
    if (n > ix->col_cap[slot] || !ix->cols[slot]) {
        const int64_t cap = round_up(std::max<int64_t>(n, 1), kRowAlign);
        double* cnew = nullptr;
        HIP_TRY(hipMalloc(&cnew, (size_t)cap * sizeof(double)));
        if (ix->cols[slot]) (void)hipFree(ix->cols[slot]);
        ix->cols[slot] = cnew;
        ix->col_cap[slot] = cap;
    }
    ix->col_mask &= ~bit;  // until the new column is whole
    if (n > 0) {
        if (mem == VDB_MEM_DEVICE) {
            // the values may still be being written on the caller's stream: the copy starts after that work
            HIP_TRY(order_after_caller(st, stream));
        }
        HIP_TRY(hipMemcpyAsync(ix->cols[slot], values, (size_t)n * sizeof(double),
                               mem == VDB_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    ix->col_mask |= bit;
    ix->n_column_sets++;
    return VDB_OK;
}

int32_t vdb_index_filter_mask(vdb_index* ix, const vdb_filter_clause* clauses, const int32_t* pred_offsets,
                              int32_t n_preds, const uint32_t* base_masks, int32_t mem, uint32_t* out_masks,
                              int64_t* out_counts, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    // the clauses and offsets are host memory whatever `mem` says: everything checked before any launch
    const FilterClause* cl = reinterpret_cast<const FilterClause*>(clauses);
    int64_t at = 0;
    uint32_t used = 0;
    switch (filter_validate(cl, pred_offsets, n_preds, ix->col_mask, &at, &used)) {
        case kFilterBadPreds:
            return set_error(VDB_ERR_INVALID, "n_preds must be in [0, %d], got %d", kFilterMaxPreds, n_preds);
        case kFilterNullArgs: return set_error(VDB_ERR_INVALID, "NULL clauses / pred_offsets pointer");
        case kFilterBadOffsets:
            return set_error(VDB_ERR_INVALID, "pred_offsets must start at 0 and ascend (predicate %lld)", (long long)at);
        case kFilterTooMany:
            return set_error(VDB_ERR_INVALID, "predicate %lld has more than %d clauses", (long long)at, kFilterMaxClauses);
        case kFilterBadSlot:
            return set_error(VDB_ERR_INVALID, "clause %lld: column %d is outside [0, %d)", (long long)at, cl[at].column,
                             kFilterSlots);
        case kFilterNotAttached:
            return set_error(VDB_ERR_INVALID,
                             "clause %lld: no column is attached to slot %d (vdb_index_set_column; add, remove and "
                             "clear drop the columns)",
                             (long long)at, cl[at].column);
        case kFilterBadFlags:
            return set_error(VDB_ERR_INVALID, "clause %lld: unknown flag bits 0x%x", (long long)at, (unsigned)cl[at].flags);
        case kFilterNanBound: return set_error(VDB_ERR_INVALID, "clause %lld: a bound is NaN", (long long)at);
        default: break;
    }
    const int64_t N = ix->count;
    if (n_preds > 0 && N > 0 && !out_masks) return set_error(VDB_ERR_INVALID, "out_masks is NULL");
    if (out_masks && base_masks && N > 0 && (const uint32_t*)out_masks == base_masks)
        return set_error(VDB_ERR_INVALID, "out_masks may not alias base_masks");
    if (n_preds == 0) {
        ix->n_filter_calls++;
        return VDB_OK;
    }
    const bool host = mem == VDB_MEM_HOST;
    const int32_t n_clauses = pred_offsets[n_preds];
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;
    const bool based = base_masks != nullptr && N > 0;
    const FilterScratch sc = filter_scratch(n_preds, N, host, based);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    const size_t mask_bytes = (size_t)n_preds * (size_t)sc.n_words * 4;
    FilterArgs a{};
    a.base = based ? base_masks : nullptr;
    a.out = out_masks;
    a.counts = reinterpret_cast<unsigned long long*>(out_counts);
    if (host) {  // the base masks go up in one copy through the pinned staging, the results come down in one
        if (based) {
            rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st,
                          [&](char* h) { std::memcpy(h + (sc.base - sc.in0), base_masks, mask_bytes); });
            if (rc) return rc;
            a.base = reinterpret_cast<const uint32_t*>(dev + sc.base);
        } else {
            rc = ws_host_io(w, (size_t)(sc.in_bytes + sc.out_bytes));
            if (rc) return rc;
        }
        a.out = reinterpret_cast<uint32_t*>(dev + sc.out_m);
        a.counts = out_counts ? reinterpret_cast<unsigned long long*>(dev + sc.out_c) : nullptr;
    }
    if (a.counts) HIP_TRY(hipMemsetAsync(a.counts, 0, (size_t)n_preds * 8, st));  // (an empty index: all there is)
    if (N > 0) {
        // the clauses and offsets: into a pinned slot of the workspace's ring now, up on the stream
        if (!w->filt_io)
            HIP_TRY(hipHostMalloc(&w->filt_io, (size_t)Workspace::kFiltRing * kFilterStageBytes, hipHostMallocDefault));
        const int slot = w->filt_head;
        w->filt_head = (slot + 1) % Workspace::kFiltRing;
        if (!w->filt_up[slot]) HIP_TRY(hipEventCreateWithFlags(&w->filt_up[slot], hipEventDisableTiming));
        if (w->filt_used[slot]) HIP_TRY(hipEventSynchronize(w->filt_up[slot]));
        char* h = w->filt_io + (size_t)slot * kFilterStageBytes;
        const FilterStage fs = filter_stage(n_clauses, n_preds);
        if (n_clauses > 0) std::memcpy(h + fs.clauses, cl, (size_t)n_clauses * sizeof(FilterClause));
        std::memcpy(h + fs.offsets, pred_offsets, (size_t)(n_preds + 1) * 4);
        HIP_TRY(hipMemcpyAsync(dev + sc.stage, h, (size_t)fs.bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(w->filt_up[slot], st));
        w->filt_used[slot] = true;
        for (int s = 0; s < kFilterSlots; ++s) a.cols[s] = ((used >> s) & 1u) ? ix->cols[s] : nullptr;
        a.used = used;
        a.N = N;
        a.n_words = sc.n_words;
        a.n_preds = n_preds;
        a.n_clauses = n_clauses;
        a.clauses = reinterpret_cast<const FilterClause*>(dev + sc.stage + fs.clauses);
        a.offsets = reinterpret_cast<const int32_t*>(dev + sc.stage + fs.offsets);
        HIP_TRY(launch_filter_mask(a, ix->n_cu, st));
    }
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        if (out_masks && mask_bytes) std::memcpy(out_masks, r + (sc.out_m - sc.out0), mask_bytes);
        if (out_counts) std::memcpy(out_counts, r + (sc.out_c - sc.out0), (size_t)n_preds * 8);
    }
    ix->n_filter_calls++;
    ix->n_filter_preds += n_preds;
    return VDB_OK;
}

int32_t vdb_index_search_groups(vdb_index* ix, const float* queries, int32_t B, int32_t k, const uint32_t* row_mask,
                                int32_t mem, float* out_scores, int64_t* out_indices, int32_t* out_groups,
                                double* out_keys, int64_t index_offset, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (B == 0) return VDB_OK;
    const int D = ix->dim;
    const bool host = mem == VDB_MEM_HOST;
    // everything checked before any launch (the column itself under the lock, below)
    switch (group_validate(B, k, queries != nullptr, out_scores != nullptr, out_indices != nullptr,
                           out_groups != nullptr, mem, true, 0, 0)) {
        case kGroupBadQueries:
            return set_error(VDB_ERR_INVALID, "n_queries must be in [0, %d], got %d", kGroupMaxQueries, B);
        case kGroupBadK: return set_error(VDB_ERR_INVALID, "k must be in [1, %d], got %d", kGroupMaxK, k);
        case kGroupNullPointer:
            return set_error(VDB_ERR_INVALID, "NULL query/output pointer (out_groups is required)");
        case kGroupBadMem: return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
        default: break;
    }
    if (host && !all_finite(queries, (int64_t)B * D)) return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    if (group_validate(B, k, true, true, true, true, mem, ix->group_set, ix->group_n, N) == kGroupNoColumn)
        return set_error(VDB_ERR_INVALID, "no group column is attached (vdb_index_set_groups; add, remove and clear drop it)");
    // as vdb_index_search_rows: the caller's stream (device memory: NULL = the null stream), or for
    // a host-memory call without one the stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const bool force = ix->group_force_exact != 0;
    const int kf = group_fetch_k(ix->group_fetch, k);
    const int n_seg = N > 0 ? group_n_seg(N, B, k) : 1;
    const GroupScratch sc = group_scratch(B, D, k, kf, n_seg, N, host, masked, out_keys != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    const float* Qd = queries;
    const uint32_t* cm = masked ? row_mask : nullptr;  // the caller's mask, on the device
    float* out_s = out_scores;
    int64_t* out_i = out_indices;
    int32_t* out_g = out_groups;
    double* out_k = out_keys;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            std::memcpy(h + (sc.q - sc.in0), queries, (size_t)B * D * 4);
            if (masked) std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.mask_words * 4);
        });
        if (rc) return rc;
        Qd = reinterpret_cast<const float*>(dev + sc.q);
        cm = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        out_s = reinterpret_cast<float*>(dev + sc.out_s);
        out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        out_g = reinterpret_cast<int32_t*>(dev + sc.out_g);
        out_k = out_keys ? reinterpret_cast<double*>(dev + sc.out_k) : nullptr;
    }
    if (N == 0) {  // an empty index: every slot "no result", as a search
        HIP_TRY(launch_empty_results((int64_t)B * k, out_s, out_i, out_k, st));
        HIP_TRY(hipMemsetAsync(out_g, 0xFF, (size_t)B * k * sizeof(int32_t), st));
    } else {
        // the mask of this call: the rows with a group AND the caller's rows
        const uint32_t* fm = nullptr;
        unsigned long long* elig_dev = nullptr;  // a masked call's eligible rows, counted on the device
        if (cm) {
            uint32_t* both = reinterpret_cast<uint32_t*>(dev + sc.fmask);
            elig_dev = reinterpret_cast<unsigned long long*>(dev + sc.elig);
            HIP_TRY(hipMemsetAsync(elig_dev, 0, sizeof(unsigned long long), st));
            HIP_TRY(launch_group_and(cm, ix->group_valid, both, sc.mask_words, elig_dev, st));
            fm = both;
        } else if (ix->group_any_neg) {
            fm = ix->group_valid;
        }
        double* qn64 = reinterpret_cast<double*>(dev + sc.qn64);
        int* done = reinterpret_cast<int*>(dev + sc.done);
        int* need = reinterpret_cast<int*>(dev + sc.need);
        float* fs = reinterpret_cast<float*>(dev + sc.fs);
        int64_t* fi = reinterpret_cast<int64_t*>(dev + sc.fi);
        double* fk = reinterpret_cast<double*>(dev + sc.fk);
        if (!force) {
            // step 1: the best kf eligible rows with their keys, by the ordinary search in device
            // memory on this stream (its own workspace, certificate and gated fallback; it counts
            // the call in "searches" / "queries")
            SearchOpts o;
            rc = search_locked(ix, Qd, B, kf, fm, VDB_MEM_DEVICE, fs, fi, fk, 0, st, nullptr, o);
            if (rc == kRetryBf16x3) {
                o.force_b3 = true;
                rc = search_locked(ix, Qd, B, kf, fm, VDB_MEM_DEVICE, fs, fi, fk, 0, st, nullptr, o);
            }
            if (rc) return rc;
        } else {
            ix->n_searches++;
            ix->n_queries += B;
        }
        // the canonical query norms and the zeroed per-query counters of the fallback
        HIP_TRY(launch_prep_queries(Qd, B, B, D, ix->G, ix->metric, nullptr, nullptr, qn64, nullptr, nullptr, nullptr,
                                    nullptr, done, st));
        GroupSelectArgs sa{};
        sa.fs = fs; sa.fi = fi; sa.fk = fk; sa.k_fetch = kf;
        sa.groups = ix->groups; sa.count = N; sa.k = k; sa.force = force ? 1 : 0;
        sa.eligible = ix->group_valid_rows; sa.eligible_dev = elig_dev;
        sa.need = need; sa.fallback_total = ix->d_group_fb;
        sa.out_s = out_s; sa.out_i = out_i; sa.out_g = out_g; sa.out_k = out_k; sa.index_offset = index_offset;
        HIP_TRY(launch_group_select(sa, B, st));
        // step 3, gated per query on the device: nothing to wait for
        GroupExactArgs ea{};
        ea.Q = Qd; ea.qn64 = qn64; ea.X = ix->X; ea.G = ix->G; ea.D = D; ea.nrm64 = ix->nrm64; ea.N = N;
        ea.mask = fm; ea.groups = ix->groups; ea.need = need; ea.k = k;
        ea.lk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.lk) : nullptr;
        ea.lr = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.lr) : nullptr;
        ea.lg = n_seg > 1 ? reinterpret_cast<int32_t*>(dev + sc.lg) : nullptr;
        ea.done = done;
        ea.out_s = out_s; ea.out_i = out_i; ea.out_g = out_g; ea.out_k = out_k; ea.index_offset = index_offset;
        HIP_TRY(launch_group_exact(ix->metric, ea, B, n_seg, st));
    }
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)B * k * 4);
        std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)B * k * 8);
        std::memcpy(out_groups, r + (sc.out_g - sc.out0), (size_t)B * k * 4);
        if (out_keys) std::memcpy(out_keys, r + (sc.out_k - sc.out0), (size_t)B * k * 8);
    }
    if (N == 0) {  // (a non-empty index's call was counted by its inner search)
        ix->n_searches++;
        ix->n_queries += B;
    }
    ix->n_group_searches++;
    ix->n_group_queries += B;
    return VDB_OK;
}

int32_t vdb_index_search_mmr(vdb_index* ix, const float* queries, int32_t B, int32_t k, int32_t fetch_k, double lambda,
                             const uint32_t* row_mask, int32_t mem, float* out_scores, int64_t* out_indices,
                             double* out_keys, double* out_mmr, int64_t index_offset, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    // everything checked before any launch
    switch (mmr_validate(B, k, fetch_k, lambda, queries != nullptr || B == 0, out_scores != nullptr || B == 0,
                         out_indices != nullptr || B == 0, mem)) {
        case kMmrBadQueries: return set_error(VDB_ERR_INVALID, "n_queries must be >= 0, got %d", B);
        case kMmrBadK: return set_error(VDB_ERR_INVALID, "k must be in [1, %d], got %d", kMmrMaxK, k);
        case kMmrBadFetch:
            return set_error(VDB_ERR_INVALID, "fetch_k must be in [k, %d], got fetch_k=%d k=%d", kMmrMaxFetch, fetch_k, k);
        case kMmrBadLambda: return set_error(VDB_ERR_INVALID, "lambda must be in [0, 1], got %g", lambda);
        case kMmrNullPointer: return set_error(VDB_ERR_INVALID, "NULL query/output pointer");
        case kMmrBadMem: return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
        default: break;
    }
    if (B == 0) return VDB_OK;
    const int D = ix->dim;
    const bool host = mem == VDB_MEM_HOST;
    if (host && !all_finite(queries, (int64_t)B * D)) return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    // as vdb_index_search_groups: the caller's stream, or for a host-memory call without one the
    // stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const MmrScratch sc = mmr_scratch(B, D, k, fetch_k, N, host, masked, out_keys != nullptr, out_mmr != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    const float* Qd = queries;
    const uint32_t* md = masked ? row_mask : nullptr;
    float* out_s = out_scores;
    int64_t* out_i = out_indices;
    double* out_k = out_keys;
    double* out_m = out_mmr;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            std::memcpy(h + (sc.q - sc.in0), queries, (size_t)B * D * 4);
            if (masked) {
                std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.mask_words * 4);
                std::memset(h + (sc.mask - sc.in0) + sc.mask_words * 4, 0, 64 * 4);
            }
        });
        if (rc) return rc;
        Qd = reinterpret_cast<const float*>(dev + sc.q);
        md = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        out_s = reinterpret_cast<float*>(dev + sc.out_s);
        out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        out_k = out_keys ? reinterpret_cast<double*>(dev + sc.out_k) : nullptr;
        out_m = out_mmr ? reinterpret_cast<double*>(dev + sc.out_m) : nullptr;
    }
    if (N == 0) {  // an empty index: every slot "no result", as a search
        HIP_TRY(launch_empty_results((int64_t)B * k, out_s, out_i, out_k, st));
        // (out_mmr is -inf as the keys are: the same fill once more, with it in the keys' place)
        if (out_m) HIP_TRY(launch_empty_results((int64_t)B * k, out_s, out_i, out_m, st));
    } else {
        float* fs = reinterpret_cast<float*>(dev + sc.fs);
        int64_t* fi = reinterpret_cast<int64_t*>(dev + sc.fi);
        double* fk = reinterpret_cast<double*>(dev + sc.fk);
        // step 1: the candidate lists, the best fetch_k eligible rows with their keys, by the
        // ordinary search in device memory on this stream (its own workspace, certificate and
        // gated fallback; it counts the call in "searches" / "queries")
        SearchOpts o;
        rc = search_locked(ix, Qd, B, fetch_k, md, VDB_MEM_DEVICE, fs, fi, fk, 0, st, nullptr, o);
        if (rc == kRetryBf16x3) {
            o.force_b3 = true;
            rc = search_locked(ix, Qd, B, fetch_k, md, VDB_MEM_DEVICE, fs, fi, fk, 0, st, nullptr, o);
        }
        if (rc) return rc;
        // steps 2 and 3, block after block of queries over the same pair scratch
        MmrArgs a{};
        a.fi = fi; a.fk = fk; a.k_fetch = fetch_k; a.k = k; a.lambda = lambda;
        a.X = ix->X; a.G = ix->G; a.D = D; a.nrm64 = ix->nrm64; a.count = N;
        a.S = reinterpret_cast<double*>(dev + sc.S);
        a.out_s = out_s; a.out_i = out_i; a.out_k = out_k; a.out_m = out_m; a.index_offset = index_offset;
        const int qblock = mmr_query_block(fetch_k);
        for (int b0 = 0; b0 < B; b0 += qblock) {
            const int qb = std::min(qblock, B - b0);
            HIP_TRY(launch_mmr_pairs(ix->metric, a, b0, qb, st));
            HIP_TRY(launch_mmr_select(ix->metric, a, b0, qb, st));
        }
    }
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)B * k * 4);
        std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)B * k * 8);
        if (out_keys) std::memcpy(out_keys, r + (sc.out_k - sc.out0), (size_t)B * k * 8);
        if (out_mmr) std::memcpy(out_mmr, r + (sc.out_m - sc.out0), (size_t)B * k * 8);
    }
    if (N == 0) {  // (a non-empty index's call was counted by its inner search)
        ix->n_searches++;
        ix->n_queries += B;
    }
    ix->n_mmr_searches++;
    ix->n_mmr_queries += B;
    return VDB_OK;
}

int32_t vdb_index_search_recommend(vdb_index* ix, int32_t B, int32_t k, const int64_t* pos_offsets,
                                   const int64_t* pos_rows, int64_t n_pos, const int64_t* neg_offsets,
                                   const int64_t* neg_rows, int64_t n_neg, const uint32_t* row_mask, int32_t mem,
                                   float* out_scores, int64_t* out_indices, double* out_keys, float* out_queries,
                                   int64_t index_offset, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    // everything checked before any launch (a host-memory call's lists under the lock, below)
    switch (rec_validate(B, k, n_pos, n_neg, pos_offsets != nullptr, pos_rows != nullptr, neg_offsets != nullptr,
                         neg_rows != nullptr, out_scores != nullptr, out_indices != nullptr, mem)) {
        case kRecBadQueries: return set_error(VDB_ERR_INVALID, "n_queries must be >= 0, got %d", B);
        case kRecBadK: return set_error(VDB_ERR_INVALID, "k must be in [1, %d], got %d", kRecMaxK, k);
        case kRecBadMem: return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
        case kRecBadCounts:
            return set_error(VDB_ERR_INVALID, "n_pos and n_neg must be >= 0, and n_neg 0 without neg_offsets (got %lld, %lld)",
                             (long long)n_pos, (long long)n_neg);
        case kRecNullPointer: return set_error(VDB_ERR_INVALID, "NULL list/output pointer");
        default: break;
    }
    if (B == 0) return VDB_OK;
    const int D = ix->dim;
    const bool host = mem == VDB_MEM_HOST;
    const bool has_neg = neg_offsets != nullptr;
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    int examples = rec_fetch_examples_device(n_pos, n_neg);
    if (host) {
        int64_t at = 0;
        int which = 0;
        const int vr = rec_validate_lists(pos_offsets, pos_rows, n_pos, neg_offsets, neg_rows, n_neg, B, N, &at, &which,
                                          &examples);
        const char* name = which ? "neg" : "pos";
        const int64_t* offs = which ? neg_offsets : pos_offsets;
        const int64_t* rows = which ? neg_rows : pos_rows;
        switch (vr) {
            case kRecOk: break;
            case kRecBadOffsets:
                return set_error(VDB_ERR_INVALID, "%s_offsets[%lld] = %lld: offsets must ascend from >= 0 to <= n_%s (%lld)",
                                 name, (long long)at, (long long)offs[at], name, (long long)(which ? n_neg : n_pos));
            case kRecBadId:
                return set_error(VDB_ERR_INVALID, "%s_rows[%lld] = %lld is outside [0, %lld)", name, (long long)at,
                                 (long long)rows[at], (long long)N);
            default:
                return set_error(VDB_ERR_INVALID, "query %lld has more than %d examples", (long long)at, kRecMaxExamples);
        }
    }
    // as vdb_index_search_mmr: the caller's stream, or for a host-memory call without one the
    // stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const int fetch_k = rec_fetch_k(k, examples);
    const RecScratch sc = rec_scratch(B, D, k, fetch_k, N, n_pos, n_neg, host, has_neg, masked, out_keys != nullptr,
                                      out_queries != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    RecommendArgs a{};
    a.pos_offs = pos_offsets; a.pos_rows = pos_rows; a.n_pos = n_pos;
    a.neg_offs = neg_offsets; a.neg_rows = neg_rows; a.n_neg = n_neg;
    const uint32_t* md = masked ? row_mask : nullptr;
    a.out_s = out_scores; a.out_i = out_indices; a.out_k = out_keys;
    if (host) {  // the lists and the mask go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            std::memcpy(h + (sc.pos_offs - sc.in0), pos_offsets, ((size_t)B + 1) * 8);
            if (n_pos > 0) std::memcpy(h + (sc.pos_rows - sc.in0), pos_rows, (size_t)n_pos * 8);
            if (has_neg) {
                std::memcpy(h + (sc.neg_offs - sc.in0), neg_offsets, ((size_t)B + 1) * 8);
                if (n_neg > 0) std::memcpy(h + (sc.neg_rows - sc.in0), neg_rows, (size_t)n_neg * 8);
            }
            if (masked) {
                std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.mask_words * 4);
                std::memset(h + (sc.mask - sc.in0) + sc.mask_words * 4, 0, 64 * 4);
            }
        });
        if (rc) return rc;
        a.pos_offs = reinterpret_cast<const int64_t*>(dev + sc.pos_offs);
        a.pos_rows = reinterpret_cast<const int64_t*>(dev + sc.pos_rows);
        a.neg_offs = has_neg ? reinterpret_cast<const int64_t*>(dev + sc.neg_offs) : nullptr;
        a.neg_rows = has_neg ? reinterpret_cast<const int64_t*>(dev + sc.neg_rows) : nullptr;
        md = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        a.out_s = reinterpret_cast<float*>(dev + sc.out_s);
        a.out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        a.out_k = out_keys ? reinterpret_cast<double*>(dev + sc.out_k) : nullptr;
    }
    a.X = ix->X; a.G = ix->G; a.D = D; a.nrm64 = ix->nrm64; a.count = N;
    a.Q = reinterpret_cast<float*>(dev + sc.q);
    a.flag = reinterpret_cast<int*>(dev + sc.flag);
    a.bad = ix->d_xmax + kRecommendBadWord;
    a.k = k; a.k_fetch = fetch_k; a.index_offset = index_offset;
    // step 1: the built queries and their flags (an empty index: every query is flagged or empty)
    HIP_TRY(launch_recommend_build(ix->metric, a, B, st));
    if (N == 0) {  // every slot "no result", as a search
        HIP_TRY(launch_empty_results((int64_t)B * k, a.out_s, a.out_i, a.out_k, st));
    } else {
        float* fs = reinterpret_cast<float*>(dev + sc.fs);
        int64_t* fi = reinterpret_cast<int64_t*>(dev + sc.fi);
        double* fk = reinterpret_cast<double*>(dev + sc.fk);
        // step 2: the best fetch_k eligible rows of every built query with their keys, by the
        // ordinary search in device memory on this stream (its own workspace, certificate and
        // gated fallback; it counts the call in "searches" / "queries")
        SearchOpts o;
        rc = search_locked(ix, a.Q, B, fetch_k, md, VDB_MEM_DEVICE, fs, fi, fk, 0, st, nullptr, o);
        if (rc == kRetryBf16x3) {
            o.force_b3 = true;
            rc = search_locked(ix, a.Q, B, fetch_k, md, VDB_MEM_DEVICE, fs, fi, fk, 0, st, nullptr, o);
        }
        if (rc) return rc;
        // step 3: the examples dropped, the first k kept
        a.fi = fi; a.fk = fk;
        HIP_TRY(launch_recommend_select(ix->metric, a, B, st));
    }
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)B * k * 4);
        std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)B * k * 8);
        if (out_keys) std::memcpy(out_keys, r + (sc.out_k - sc.out0), (size_t)B * k * 8);
        if (out_queries) std::memcpy(out_queries, r + (sc.q - sc.out0), (size_t)B * D * 4);
    } else if (out_queries) {
        HIP_TRY(hipMemcpyAsync(out_queries, a.Q, (size_t)B * D * 4, hipMemcpyDeviceToDevice, st));
    }
    if (N == 0) {  // (a non-empty index's call was counted by its inner search)
        ix->n_searches++;
        ix->n_queries += B;
    }
    ix->n_rec_searches++;
    ix->n_rec_queries += B;
    return VDB_OK;
}

int32_t vdb_index_search_fused(vdb_index* ix, const float* queries, int32_t n_sub, const int64_t* set_offsets,
                               int32_t n_sets, const double* weights, int32_t k, int32_t fetch_k, int32_t fusion,
                               double rrf_c, const uint32_t* row_mask, int32_t mem, float* out_scores,
                               int64_t* out_indices, double* out_fused, int32_t* out_hits, int64_t index_offset,
                               void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    // everything checked before any launch (a device-memory call's offsets and weights: by the kernel)
    switch (fuse_validate(n_sub, n_sets, k, fetch_k, fusion, rrf_c, queries != nullptr, set_offsets != nullptr,
                          weights != nullptr, out_scores != nullptr, out_indices != nullptr, mem)) {
        case kFuseBadCounts:
            return set_error(VDB_ERR_INVALID, "n_sub and n_sets must be >= 0, got %d and %d", n_sub, n_sets);
        case kFuseBadK: return set_error(VDB_ERR_INVALID, "k must be in [1, %d], got %d", kFuseMaxK, k);
        case kFuseBadFetch:
            return set_error(VDB_ERR_INVALID, "fetch_k must be in [k, %d], got fetch_k=%d k=%d", kFuseMaxFetch, fetch_k, k);
        case kFuseBadFusion: return set_error(VDB_ERR_INVALID, "fusion must be VDB_FUSE_RRF or VDB_FUSE_MAX, got %d", fusion);
        case kFuseBadC: return set_error(VDB_ERR_INVALID, "rrf_c must be finite and >= 0, got %g", rrf_c);
        case kFuseNullPointer: return set_error(VDB_ERR_INVALID, "NULL query/offset/output pointer");
        case kFuseBadMem: return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
        case kFuseWeightsWithMax: return set_error(VDB_ERR_INVALID, "weights must be NULL for VDB_FUSE_MAX");
        default: break;
    }
    if (n_sets == 0) return VDB_OK;
    const int D = ix->dim;
    const bool host = mem == VDB_MEM_HOST;
    if (host) {
        int64_t at = 0;
        switch (fuse_validate_lists(set_offsets, n_sets, n_sub, weights, &at)) {
            case kFuseBadOffsets:
                return set_error(VDB_ERR_INVALID, "set_offsets[%lld] = %lld: offsets must ascend from >= 0 to <= n_sub (%d)",
                                 (long long)at, (long long)set_offsets[at], n_sub);
            case kFuseSetTooLong:
                return set_error(VDB_ERR_INVALID, "set %lld has more than %d sub-queries", (long long)at, kFuseMaxLists);
            case kFuseBadWeight:
                return set_error(VDB_ERR_INVALID, "weights[%lld] = %g: a weight must be finite and >= 0", (long long)at,
                                 weights[at]);
            default: break;
        }
        if (!all_finite(queries, (int64_t)n_sub * D)) return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    }
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    // as vdb_index_search_mmr: the caller's stream, or for a host-memory call without one the
    // stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const FuseScratch sc = fuse_scratch(n_sub, n_sets, D, k, fetch_k, N, host, weights != nullptr, masked,
                                        out_fused != nullptr, out_hits != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    const float* Qd = queries;
    const uint32_t* md = masked ? row_mask : nullptr;
    FuseArgs a{};
    a.offs = set_offsets; a.weights = weights;
    a.out_s = out_scores; a.out_i = out_indices; a.out_f = out_fused; a.out_h = out_hits;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            if (n_sub > 0) std::memcpy(h + (sc.q - sc.in0), queries, (size_t)n_sub * D * 4);
            std::memcpy(h + (sc.offs - sc.in0), set_offsets, ((size_t)n_sets + 1) * 8);
            if (weights && n_sub > 0) std::memcpy(h + (sc.w - sc.in0), weights, (size_t)n_sub * 8);
            if (masked) {
                std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.mask_words * 4);
                std::memset(h + (sc.mask - sc.in0) + sc.mask_words * 4, 0, 64 * 4);
            }
        });
        if (rc) return rc;
        Qd = reinterpret_cast<const float*>(dev + sc.q);
        md = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        a.offs = reinterpret_cast<const int64_t*>(dev + sc.offs);
        a.weights = weights ? reinterpret_cast<const double*>(dev + sc.w) : nullptr;
        a.out_s = reinterpret_cast<float*>(dev + sc.out_s);
        a.out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        a.out_f = out_fused ? reinterpret_cast<double*>(dev + sc.out_f) : nullptr;
        a.out_h = out_hits ? reinterpret_cast<int32_t*>(dev + sc.out_h) : nullptr;
    }
    float* fs = reinterpret_cast<float*>(dev + sc.fs);
    int64_t* fi = reinterpret_cast<int64_t*>(dev + sc.fi);
    double* fk = reinterpret_cast<double*>(dev + sc.fk);
    a.fs = fs; a.fi = fi; a.fk = fk;
    a.k_fetch = fetch_k; a.k = k; a.n_sub = n_sub; a.rrf_c = rrf_c; a.count = N;
    a.bad = ix->d_xmax + kFusedBadWord;
    a.index_offset = index_offset;
    const bool inner = N > 0 && n_sub > 0;
    if (inner) {
        // step 1: the lists, the best fetch_k eligible rows of every sub-query with their scores and
        // keys, by the ordinary search in device memory on this stream (its own workspace,
        // certificate and gated fallback; it counts the call in "searches" / "queries")
        SearchOpts o;
        rc = search_locked(ix, Qd, n_sub, fetch_k, md, VDB_MEM_DEVICE, fs, fi, fk, 0, st, nullptr, o);
        if (rc == kRetryBf16x3) {
            o.force_b3 = true;
            rc = search_locked(ix, Qd, n_sub, fetch_k, md, VDB_MEM_DEVICE, fs, fi, fk, 0, st, nullptr, o);
        }
        if (rc) return rc;
    }
    // step 2: one workgroup per set (an empty index or a call without sub-queries: it reads no list
    // and every slot is "no result"; a device-memory call's bad sets are still counted)
    HIP_TRY(launch_fuse(fusion, a, n_sets, st));
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)n_sets * k * 4);
        std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)n_sets * k * 8);
        if (out_fused) std::memcpy(out_fused, r + (sc.out_f - sc.out0), (size_t)n_sets * k * 8);
        if (out_hits) std::memcpy(out_hits, r + (sc.out_h - sc.out0), (size_t)n_sets * k * 4);
    }
    if (!inner) {  // (otherwise the call was counted by its inner search)
        ix->n_searches++;
        ix->n_queries += n_sub;
    }
    ix->n_fused_searches++;
    ix->n_fused_sets += n_sets;
    return VDB_OK;
}

int32_t vdb_index_set_sparse(vdb_index* ix, const int64_t* indptr, const int32_t* terms, const float* weights, int64_t n,
                             int64_t nnz, int32_t n_terms, int32_t mem, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    HIP_TRY(hipSetDevice(ix->device));
    std::unique_lock<std::shared_mutex> g(ix->mu);
    switch (sparse_column_args(indptr != nullptr, terms != nullptr, weights != nullptr, n, nnz, n_terms, ix->count)) {
        case kSparseColBadCounts:
            return set_error(VDB_ERR_INVALID,
                             indptr ? "the sparse column has %lld rows, the index %lld (nnz %lld >= 0 and n_terms %d >= 1 required)"
                                    : "a NULL indptr detaches: n must be 0 (got %lld)",
                             (long long)n, (long long)ix->count, (long long)nnz, n_terms);
        case kSparseColNullPointer: return set_error(VDB_ERR_INVALID, "NULL terms / weights with nnz %lld", (long long)nnz);
        default: break;
    }
    const bool host = mem == VDB_MEM_HOST;
    const auto cause_error = [&](int cause, int64_t row, bool have_row) {
        const char* what = cause == kSparseColBadIndptr  ? "indptr must ascend from 0 to nnz"
                           : cause == kSparseColBadTerm  ? "a term id outside [0, n_terms)"
                           : cause == kSparseColUnsorted ? "term ids must be strictly ascending within a row"
                                                         : "a NaN or Inf weight";
        const int code = cause == kSparseColNonFinite ? VDB_ERR_NONFINITE : VDB_ERR_INVALID;
        return have_row ? set_error(code, "sparse column, row %lld: %s", (long long)row, what)
                        : set_error(code, "sparse column: %s", what);
    };
    if (indptr && host) {  // everything checked before the column is replaced
        int64_t at = 0;
        const int cause = sparse_validate_column(indptr, terms, weights, n, nnz, n_terms, &at);
        if (cause != kSparseColOk) return cause_error(cause, at, true);
    }
    // queued device-memory searches on caller streams read the column this call replaces
    {
        const int wr = wait_idle(ix);
        if (wr) return wr;
    }
    if (!indptr) {  // detach
        ix->sparse_set = false;
        return VDB_OK;
    }
    // the new column is built beside the old one, which stays as it was on any error
    hipStream_t st = ix->stream;
    int64_t* ind_new = nullptr;
    SparsePair* pairs_new = nullptr;
    HIP_TRY(hipMalloc(&ind_new, (size_t)(n + 1) * sizeof(int64_t)));
    {
        const hipError_t e = hipMalloc(&pairs_new, (size_t)std::max<int64_t>(nnz, 1) * sizeof(SparsePair));
        if (e != hipSuccess) {
            (void)hipFree(ind_new);
            HIP_TRY(e);
        }
    }
    const auto build = [&]() -> int {
        if (host) {
            std::vector<SparsePair> pairs((size_t)nnz);
            for (int64_t e = 0; e < nnz; ++e) pairs[(size_t)e] = SparsePair{terms[e], weights[e]};
            HIP_TRY(hipMemcpyAsync(ind_new, indptr, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
            if (nnz > 0)
                HIP_TRY(hipMemcpyAsync(pairs_new, pairs.data(), (size_t)nnz * sizeof(SparsePair), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
            return VDB_OK;
        }
        // device memory: the arrays may still be being written on the caller's stream; a kernel
        // validates them and one flag word comes back, as vdb_index_update's does
        HIP_TRY(order_after_caller(st, stream));
        uint32_t* flags = reinterpret_cast<uint32_t*>(ix->d_xmax + kSparseFlagWord);
        HIP_TRY(hipMemsetAsync(flags, 0, sizeof(unsigned long long), st));
        HIP_TRY(hipMemcpyAsync(ind_new, indptr, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        HIP_TRY(launch_sparse_validate(ind_new, terms, weights, n, nnz, n_terms, flags, st));
        uint32_t hflags[2] = {0, 0};
        int64_t first = 0;
        HIP_TRY(hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, st));
        if (n == 0) HIP_TRY(hipMemcpyAsync(&first, ind_new, sizeof(first), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n == 0 && (first != 0 || nnz != 0)) return cause_error(kSparseColBadIndptr, 0, false);
        const int cause = sparse_column_cause(hflags[0]);
        if (cause != kSparseColOk) return cause_error(cause, 0, false);
        HIP_TRY(launch_sparse_pack(terms, weights, nnz, pairs_new, st));
        HIP_TRY(hipStreamSynchronize(st));
        return VDB_OK;
    };
    const int rc = build();
    if (rc) {
        (void)hipFree(ind_new);
        (void)hipFree(pairs_new);
        return rc;
    }
    if (ix->sparse_indptr) (void)hipFree(ix->sparse_indptr);
    if (ix->sparse_pairs) (void)hipFree(ix->sparse_pairs);
    ix->sparse_indptr = ind_new;
    ix->sparse_pairs = pairs_new;
    ix->sparse_n = n;
    ix->sparse_nnz = nnz;
    ix->sparse_terms = n_terms;
    ix->sparse_set = true;
    ix->n_sparse_sets++;
    return VDB_OK;
}

namespace {
// What a sparse or hybrid call's validation found, as the error the call returns.
int sparse_call_error(int cause, int k, int fetch_k, int64_t at) {
    switch (cause) {
        case kSparseBadCounts: return set_error(VDB_ERR_INVALID, "n_queries and q_nnz must be >= 0");
        case kSparseBadK: return set_error(VDB_ERR_INVALID, "k must be in [1, %d], got %d", fetch_k ? kFuseMaxK : kSparseMaxK, k);
        case kSparseNullPointer: return set_error(VDB_ERR_INVALID, "NULL query/output pointer");
        case kSparseBadMem: return set_error(VDB_ERR_INVALID, "bad mem kind");
        case kSparseNoColumn: return set_error(VDB_ERR_INVALID, "no sparse column is attached (vdb_index_set_sparse)");
        case kSparseBadOffsets:
            return set_error(VDB_ERR_INVALID, "q_indptr[%lld]: offsets must ascend from >= 0 to <= q_nnz", (long long)at);
        case kSparseTooLong:
            return set_error(VDB_ERR_INVALID, "query %lld has more than %d terms", (long long)at, kSparseMaxQueryTerms);
        case kSparseBadTerm: return set_error(VDB_ERR_INVALID, "q_terms[%lld] is outside [0, n_terms)", (long long)at);
        case kSparseUnsorted:
            return set_error(VDB_ERR_INVALID, "q_terms[%lld]: a query's term ids must be strictly ascending", (long long)at);
        case kSparseNonFinite: return set_error(VDB_ERR_NONFINITE, "q_weights[%lld] is NaN or Inf", (long long)at);
        case kHybridBadFetch:
            return set_error(VDB_ERR_INVALID, "fetch_k must be in [k, %d], got fetch_k=%d k=%d", kFuseMaxFetch, fetch_k, k);
        case kHybridBadWeight: return set_error(VDB_ERR_INVALID, "w_dense and w_sparse must be finite and >= 0");
        case kHybridBadC: return set_error(VDB_ERR_INVALID, "rrf_c must be finite and >= 0");
        default: return VDB_OK;
    }
}
}  // namespace

int32_t vdb_index_search_sparse(vdb_index* ix, const int64_t* q_indptr, const int32_t* q_terms, const float* q_weights,
                                int32_t B, int64_t q_nnz, int32_t k, const uint32_t* row_mask, int32_t mem,
                                float* out_scores, int64_t* out_indices, double* out_keys, int64_t index_offset,
                                void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    // everything checked before any launch (a device-memory call's queries: by the kernel)
    const bool column = ix->sparse_set && ix->sparse_n == N;
    int cause = sparse_validate_call(B, q_nnz, k, q_indptr != nullptr, q_terms != nullptr, q_weights != nullptr,
                                     out_scores != nullptr, out_indices != nullptr, mem, column);
    if (cause) return sparse_call_error(cause, k, 0, 0);
    if (B == 0) return VDB_OK;
    const bool host = mem == VDB_MEM_HOST;
    if (host) {
        int64_t at = 0;
        cause = sparse_validate_queries(q_indptr, q_terms, q_weights, B, q_nnz, ix->sparse_terms, &at);
        if (cause) return sparse_call_error(cause, k, 0, at);
    }
    // as vdb_index_search_rows: the caller's stream (device memory: NULL = the null stream), or for
    // a host-memory call without one the stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const int KE = sparse_ke(k);
    const int n_seg = N > 0 ? sparse_n_seg(ix->sparse_wgs, N, B, ix->n_cu) : 1;
    const SparseScratch sc = sparse_scratch(B, k, n_seg, q_nnz, N, host, masked, out_keys != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    SparseArgs a{};
    a.q_indptr = q_indptr;
    a.q_terms = q_terms;
    a.q_weights = q_weights;
    a.mask = masked ? row_mask : nullptr;
    a.out_s = out_scores;
    a.out_i = out_indices;
    a.out_k = out_keys;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            std::memcpy(h + (sc.indptr - sc.in0), q_indptr, ((size_t)B + 1) * 8);
            if (q_nnz > 0) {
                std::memcpy(h + (sc.terms - sc.in0), q_terms, (size_t)q_nnz * 4);
                std::memcpy(h + (sc.weights - sc.in0), q_weights, (size_t)q_nnz * 4);
            }
            if (masked) std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.mask_words * 4);
        });
        if (rc) return rc;
        a.q_indptr = reinterpret_cast<const int64_t*>(dev + sc.indptr);
        a.q_terms = reinterpret_cast<const int32_t*>(dev + sc.terms);
        a.q_weights = reinterpret_cast<const float*>(dev + sc.weights);
        a.mask = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        a.out_s = reinterpret_cast<float*>(dev + sc.out_s);
        a.out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        a.out_k = out_keys ? reinterpret_cast<double*>(dev + sc.out_k) : nullptr;
    }
    a.indptr = ix->sparse_indptr;
    a.pairs = ix->sparse_pairs;
    a.N = N;
    a.n_terms = ix->sparse_terms;
    a.q_nnz = q_nnz;
    a.k = k;
    a.KE = KE;
    a.out_ld = k;
    a.done = reinterpret_cast<int*>(dev + sc.done);
    a.lk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.lk) : nullptr;
    a.li = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.li) : nullptr;
    a.mk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.mk) : nullptr;
    a.mi = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.mi) : nullptr;
    a.bad = ix->d_xmax + kSparseBadWord;
    a.index_offset = index_offset;
    // the per-query counters start at zero (the kernel leaves them so; a grown workspace is fresh)
    if (n_seg > 1) HIP_TRY(hipMemsetAsync(a.done, 0, (size_t)B * sizeof(int), st));
    // (an empty index: no row is read, every slot "no result"; a device call's bad queries still count)
    HIP_TRY(launch_sparse_search(a, B, n_seg, st));
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)B * k * 4);
        std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)B * k * 8);
        if (out_keys) std::memcpy(out_keys, r + (sc.out_k - sc.out0), (size_t)B * k * 8);
    }
    ix->n_sparse_searches++;
    ix->n_sparse_queries += B;
    return VDB_OK;
}

int32_t vdb_index_search_hybrid(vdb_index* ix, const float* queries, const int64_t* q_indptr, const int32_t* q_terms,
                                const float* q_weights, int32_t B, int64_t q_nnz, int32_t k, int32_t fetch_k,
                                double w_dense, double w_sparse, double rrf_c, const uint32_t* row_mask, int32_t mem,
                                float* out_scores, int64_t* out_indices, double* out_fused, int32_t* out_hits,
                                int64_t index_offset, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    // everything checked before any launch: the checks of the two inner calls and the fuse call's
    const bool column = ix->sparse_set && ix->sparse_n == N;
    int cause = hybrid_validate_call(B, q_nnz, k, fetch_k, w_dense, w_sparse, rrf_c, queries != nullptr, q_indptr != nullptr,
                                     q_terms != nullptr, q_weights != nullptr, out_scores != nullptr,
                                     out_indices != nullptr, mem, column);
    if (cause) return sparse_call_error(cause, k, fetch_k, 0);
    if (B == 0) return VDB_OK;
    const int D = ix->dim;
    const bool host = mem == VDB_MEM_HOST;
    if (host) {
        int64_t at = 0;
        cause = sparse_validate_queries(q_indptr, q_terms, q_weights, B, q_nnz, ix->sparse_terms, &at);
        if (cause) return sparse_call_error(cause, k, fetch_k, at);
        if (!all_finite(queries, (int64_t)B * D)) return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    }
    // as vdb_index_search_fused: the caller's stream, or for a host-memory call without one the
    // stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const int F = fetch_k;
    const int KE = sparse_ke(F);
    const int n_seg = N > 0 ? sparse_n_seg(ix->sparse_wgs, N, B, ix->n_cu) : 1;
    const HybridScratch sc = hybrid_scratch(B, D, k, F, n_seg, q_nnz, N, host, masked, out_fused != nullptr,
                                            out_hits != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    const float* Qd = queries;
    const uint32_t* md = masked ? row_mask : nullptr;
    SparseArgs sa{};
    sa.q_indptr = q_indptr;
    sa.q_terms = q_terms;
    sa.q_weights = q_weights;
    FuseArgs a{};
    a.out_s = out_scores; a.out_i = out_indices; a.out_f = out_fused; a.out_h = out_hits;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            std::memcpy(h + (sc.q - sc.in0), queries, (size_t)B * D * 4);
            std::memcpy(h + (sc.indptr - sc.in0), q_indptr, ((size_t)B + 1) * 8);
            if (q_nnz > 0) {
                std::memcpy(h + (sc.terms - sc.in0), q_terms, (size_t)q_nnz * 4);
                std::memcpy(h + (sc.weights - sc.in0), q_weights, (size_t)q_nnz * 4);
            }
            if (masked) {
                std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.mask_words * 4);
                std::memset(h + (sc.mask - sc.in0) + sc.mask_words * 4, 0, 64 * 4);
            }
        });
        if (rc) return rc;
        Qd = reinterpret_cast<const float*>(dev + sc.q);
        md = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        sa.q_indptr = reinterpret_cast<const int64_t*>(dev + sc.indptr);
        sa.q_terms = reinterpret_cast<const int32_t*>(dev + sc.terms);
        sa.q_weights = reinterpret_cast<const float*>(dev + sc.weights);
        a.out_s = reinterpret_cast<float*>(dev + sc.out_s);
        a.out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        a.out_f = out_fused ? reinterpret_cast<double*>(dev + sc.out_f) : nullptr;
        a.out_h = out_hits ? reinterpret_cast<int32_t*>(dev + sc.out_h) : nullptr;
    }
    float* ds = reinterpret_cast<float*>(dev + sc.ds);
    int64_t* di = reinterpret_cast<int64_t*>(dev + sc.di);
    double* dk = reinterpret_cast<double*>(dev + sc.dk);
    float* fs = reinterpret_cast<float*>(dev + sc.fs);
    int64_t* fi = reinterpret_cast<int64_t*>(dev + sc.fi);
    double* fk = reinterpret_cast<double*>(dev + sc.fk);
    int64_t* offs = reinterpret_cast<int64_t*>(dev + sc.offs);
    double* wts = reinterpret_cast<double*>(dev + sc.w);
    const bool inner = N > 0;
    if (inner) {
        // step 1: the dense lists, the best fetch_k eligible rows of every query with their scores and
        // keys, by the ordinary search in device memory on this stream (its own workspace,
        // certificate and gated fallback; it counts the call in "searches" / "queries")
        SearchOpts o;
        rc = search_locked(ix, Qd, B, F, md, VDB_MEM_DEVICE, ds, di, dk, 0, st, nullptr, o);
        if (rc == kRetryBf16x3) {
            o.force_b3 = true;
            rc = search_locked(ix, Qd, B, F, md, VDB_MEM_DEVICE, ds, di, dk, 0, st, nullptr, o);
        }
        if (rc) return rc;
        // step 2: into the even lists of the sets (list 2 b of [2 B][F]): three strided copies
        HIP_TRY(hipMemcpy2DAsync(fs, (size_t)2 * F * 4, ds, (size_t)F * 4, (size_t)F * 4, B, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpy2DAsync(fi, (size_t)2 * F * 8, di, (size_t)F * 8, (size_t)F * 8, B, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpy2DAsync(fk, (size_t)2 * F * 8, dk, (size_t)F * 8, (size_t)F * 8, B, hipMemcpyDeviceToDevice, st));
    }
    // step 3: the sparse lists straight into the odd ones (an empty index: "no result" lists the fuse
    // kernel does not read; a device-memory call's bad queries are still counted)
    sa.indptr = ix->sparse_indptr;
    sa.pairs = ix->sparse_pairs;
    sa.N = N;
    sa.n_terms = ix->sparse_terms;
    sa.q_nnz = q_nnz;
    sa.mask = md;
    sa.k = F;
    sa.KE = KE;
    sa.out_s = fs + F;
    sa.out_i = fi + F;
    sa.out_k = fk + F;
    sa.out_ld = 2 * (int64_t)F;
    sa.done = reinterpret_cast<int*>(dev + sc.done);
    sa.lk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.lk) : nullptr;
    sa.li = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.li) : nullptr;
    sa.mk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.mk) : nullptr;
    sa.mi = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.mi) : nullptr;
    sa.bad = ix->d_xmax + kSparseBadWord;
    sa.index_offset = 0;
    if (n_seg > 1) HIP_TRY(hipMemsetAsync(sa.done, 0, (size_t)B * sizeof(int), st));
    HIP_TRY(launch_sparse_search(sa, B, n_seg, st));
    // step 4: one workgroup per query fuses its two lists by weighted reciprocal rank
    HIP_TRY(launch_hybrid_sets(offs, wts, B, w_dense, w_sparse, st));
    a.fs = fs; a.fi = fi; a.fk = fk;
    a.k_fetch = F; a.k = k; a.n_sub = 2 * (int64_t)B; a.rrf_c = rrf_c; a.count = N;
    a.offs = offs; a.weights = wts;
    a.bad = ix->d_xmax + kFusedBadWord;  // (never moved: the sets are built here)
    a.index_offset = index_offset;
    HIP_TRY(launch_fuse(kFuseRrf, a, B, st));
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)B * k * 4);
        std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)B * k * 8);
        if (out_fused) std::memcpy(out_fused, r + (sc.out_f - sc.out0), (size_t)B * k * 8);
        if (out_hits) std::memcpy(out_hits, r + (sc.out_h - sc.out0), (size_t)B * k * 4);
    }
    if (!inner) {  // (otherwise the call was counted by its inner search)
        ix->n_searches++;
        ix->n_queries += B;
    }
    ix->n_hybrid_searches++;
    ix->n_hybrid_queries += B;
    return VDB_OK;
}

int32_t vdb_index_search_hybrid_sum(vdb_index* ix, const float* queries, const int64_t* q_indptr, const int32_t* q_terms,
                                    const float* q_weights, int32_t B, int64_t q_nnz, int32_t k, double w_dense,
                                    double w_sparse, const uint32_t* row_mask, int32_t mem, float* out_scores,
                                    int64_t* out_indices, double* out_fused, double* out_dense, double* out_sparse,
                                    int64_t index_offset, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    // everything checked before any launch (a device-memory call's queries: by the kernel)
    const bool column = ix->sparse_set && ix->sparse_n == N;
    switch (hybsum_validate_call(B, q_nnz, k, w_dense, w_sparse, queries != nullptr, q_indptr != nullptr,
                                 q_terms != nullptr, q_weights != nullptr, out_scores != nullptr, out_indices != nullptr,
                                 mem, column)) {
        case kHybsumOk: break;
        case kHybsumBadCounts: return set_error(VDB_ERR_INVALID, "n_queries and q_nnz must be >= 0");
        case kHybsumBadK: return set_error(VDB_ERR_INVALID, "k must be in [1, %d], got %d", kHybsumMaxK, k);
        case kHybsumBadMem: return set_error(VDB_ERR_INVALID, "bad mem kind");
        case kHybsumNullPointer: return set_error(VDB_ERR_INVALID, "NULL query/output pointer");
        case kHybsumNoColumn: return set_error(VDB_ERR_INVALID, "no sparse column is attached (vdb_index_set_sparse)");
        case kHybsumTooManyQueries:
            return set_error(VDB_ERR_INVALID, "n_queries must be at most %d, got %d", kHybsumMaxQueries, B);
        default: return set_error(VDB_ERR_INVALID, "w_dense and w_sparse must be in [0, 2^64]");
    }
    if (B == 0) return VDB_OK;
    const int D = ix->dim;
    const bool host = mem == VDB_MEM_HOST;
    if (host) {
        int64_t at = 0;
        const int cause = sparse_validate_queries(q_indptr, q_terms, q_weights, B, q_nnz, ix->sparse_terms, &at);
        if (cause) return sparse_call_error(cause, k, 0, at);
        if (!all_finite(queries, (int64_t)B * D)) return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    }
    // as vdb_index_search_sparse: the caller's stream (device memory: NULL = the null stream), or for
    // a host-memory call without one the stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const bool parts = out_dense != nullptr || out_sparse != nullptr;
    const int KE = sparse_ke(k);
    const int n_seg = N > 0 ? hybsum_n_seg(ix->hybsum_wgs, N, B, ix->n_cu) : 1;
    const HybsumScratch sc = hybsum_scratch(B, D, k, n_seg, q_nnz, N, host, masked, out_fused != nullptr,
                                            out_dense != nullptr, out_sparse != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    HybsumArgs a{};
    a.Q = queries;
    a.q_indptr = q_indptr;
    a.q_terms = q_terms;
    a.q_weights = q_weights;
    a.mask = masked ? row_mask : nullptr;
    a.out_s = out_scores;
    a.out_i = out_indices;
    a.out_f = out_fused;
    a.out_d = out_dense;
    a.out_p = out_sparse;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            std::memcpy(h + (sc.q - sc.in0), queries, (size_t)B * D * 4);
            std::memcpy(h + (sc.indptr - sc.in0), q_indptr, ((size_t)B + 1) * 8);
            if (q_nnz > 0) {
                std::memcpy(h + (sc.terms - sc.in0), q_terms, (size_t)q_nnz * 4);
                std::memcpy(h + (sc.weights - sc.in0), q_weights, (size_t)q_nnz * 4);
            }
            if (masked) std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.mask_words * 4);
        });
        if (rc) return rc;
        a.Q = reinterpret_cast<const float*>(dev + sc.q);
        a.q_indptr = reinterpret_cast<const int64_t*>(dev + sc.indptr);
        a.q_terms = reinterpret_cast<const int32_t*>(dev + sc.terms);
        a.q_weights = reinterpret_cast<const float*>(dev + sc.weights);
        a.mask = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        a.out_s = reinterpret_cast<float*>(dev + sc.out_s);
        a.out_i = reinterpret_cast<int64_t*>(dev + sc.out_i);
        a.out_f = out_fused ? reinterpret_cast<double*>(dev + sc.out_f) : nullptr;
        a.out_d = out_dense ? reinterpret_cast<double*>(dev + sc.out_d) : nullptr;
        a.out_p = out_sparse ? reinterpret_cast<double*>(dev + sc.out_p) : nullptr;
    }
    a.out_r = parts ? reinterpret_cast<uint32_t*>(dev + sc.rows) : nullptr;
    a.done = reinterpret_cast<int*>(dev + sc.done);
    double* qn64 = reinterpret_cast<double*>(dev + sc.qn64);
    if (N > 0) {
        // the canonical query norms and the zeroed per-query counters, nothing else: no query tiles
        // (the launch the row-list search uses)
        HIP_TRY(launch_prep_queries(a.Q, B, B, D, ix->G, ix->metric, nullptr, nullptr, qn64, nullptr, nullptr, nullptr,
                                    nullptr, a.done, st));
    }
    a.qn64 = qn64;
    a.X = ix->X;
    a.G = ix->G;
    a.D = D;
    a.nrm64 = ix->nrm64;
    a.indptr = ix->sparse_indptr;
    a.pairs = ix->sparse_pairs;
    a.N = N;
    a.n_terms = ix->sparse_terms;
    a.q_nnz = q_nnz;
    a.w_dense = w_dense;
    a.w_sparse = w_sparse;
    a.k = k;
    a.KE = KE;
    a.lk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.lk) : nullptr;
    a.li = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.li) : nullptr;
    a.mk = n_seg > 1 ? reinterpret_cast<double*>(dev + sc.mk) : nullptr;
    a.mi = n_seg > 1 ? reinterpret_cast<uint32_t*>(dev + sc.mi) : nullptr;
    a.bad = ix->d_xmax + kSparseBadWord;
    a.index_offset = index_offset;
    // (an empty index: no row is read, every slot "no result"; a device call's bad queries still count)
    HIP_TRY(launch_hybsum_search(ix->metric, a, B, n_seg, st));
    if (parts) HIP_TRY(launch_hybsum_parts(ix->metric, a, B, st));
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)B * k * 4);
        std::memcpy(out_indices, r + (sc.out_i - sc.out0), (size_t)B * k * 8);
        if (out_fused) std::memcpy(out_fused, r + (sc.out_f - sc.out0), (size_t)B * k * 8);
        if (out_dense) std::memcpy(out_dense, r + (sc.out_d - sc.out0), (size_t)B * k * 8);
        if (out_sparse) std::memcpy(out_sparse, r + (sc.out_p - sc.out0), (size_t)B * k * 8);
    }
    ix->n_hybsum_searches++;
    ix->n_hybsum_queries += B;
    return VDB_OK;
}

int32_t vdb_index_search_maxsim(vdb_index* ix, const float* queries, int32_t n_sub, const int64_t* set_offsets,
                                int32_t n_sets, int32_t n_group_slots, int32_t k, const uint32_t* row_mask, int32_t mem,
                                float* out_scores, int32_t* out_groups, double* out_sums, void* stream) {
    if (!ix) return set_error(VDB_ERR_INVALID, "index is NULL");
    // everything checked before any launch (a device-memory call's offsets: by the rank kernel; the
    // column itself under the lock, below)
    switch (maxsim_validate(n_sub, n_sets, n_group_slots, k, queries != nullptr, set_offsets != nullptr,
                            out_scores != nullptr, out_groups != nullptr, mem)) {
        case kMaxsimBadCounts:
            return set_error(VDB_ERR_INVALID, "n_sub and n_sets must be >= 0, got %d and %d", n_sub, n_sets);
        case kMaxsimBadK: return set_error(VDB_ERR_INVALID, "k must be in [1, %d], got %d", kMaxsimMaxK, k);
        case kMaxsimBadSlots:
            return set_error(VDB_ERR_INVALID,
                             "n_group_slots must be >= 1 and n_sub * n_group_slots <= %lld, got %d slots for %d sub-queries",
                             (long long)kMaxsimMaxCells, n_group_slots, n_sub);
        case kMaxsimNullPointer: return set_error(VDB_ERR_INVALID, "NULL query/offset/output pointer");
        case kMaxsimBadMem: return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
        default: break;
    }
    if (n_sets == 0) return VDB_OK;
    const int D = ix->dim;
    const bool host = mem == VDB_MEM_HOST;
    if (host) {
        int64_t at = 0;
        switch (maxsim_validate_sets(set_offsets, n_sets, n_sub, &at)) {
            case kMaxsimBadOffsets:
                return set_error(VDB_ERR_INVALID, "set_offsets[%lld] = %lld: offsets must ascend from >= 0 to <= n_sub (%d)",
                                 (long long)at, (long long)set_offsets[at], n_sub);
            case kMaxsimSetTooLong:
                return set_error(VDB_ERR_INVALID, "set %lld has more than %d sub-queries", (long long)at, kMaxsimMaxVectors);
            default: break;
        }
        if (!all_finite(queries, (int64_t)n_sub * D)) return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    }
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> g(ix->mu);
    const int64_t N = ix->count;
    if (!ix->group_set || ix->group_n != N)
        return set_error(VDB_ERR_INVALID, "no group column is attached (vdb_index_set_groups; add, remove and clear drop it)");
    // as vdb_index_search_groups: the caller's stream (device memory: NULL = the null stream), or for
    // a host-memory call without one the stream of the workspace it takes
    SearchLease lease(ix, mem, stream);
    if (lease.rc) return lease.rc;
    Workspace* const w = lease.w;
    const hipStream_t st = lease.st;

    const bool masked = row_mask != nullptr && N > 0;
    const bool scan = N > 0 && n_sub > 0;
    const MaxsimScratch sc = maxsim_scratch(n_sub, n_sets, scan ? n_group_slots : 1, D, range_query_block(ix->Dp), k, N,
                                            host, masked, out_sums != nullptr);
    int rc = ws_reserve(w, (size_t)sc.total, st);
    if (rc) return rc;
    char* dev = w->dev;
    MaxsimScanArgs a{};
    MaxsimRankArgs ra{};
    a.Q = queries;
    a.mask = masked ? row_mask : nullptr;
    ra.offs = set_offsets;
    ra.out_s = out_scores; ra.out_g = out_groups; ra.out_sum = out_sums;
    if (host) {  // the arguments go up in one copy through the pinned staging, the results come down in one
        rc = stage_up(w, sc.in0, sc.in_bytes, sc.out_bytes, st, [&](char* h) {
            if (n_sub > 0) std::memcpy(h + (sc.q - sc.in0), queries, (size_t)n_sub * D * 4);
            std::memcpy(h + (sc.offs - sc.in0), set_offsets, ((size_t)n_sets + 1) * 8);
            if (masked) std::memcpy(h + (sc.mask - sc.in0), row_mask, (size_t)sc.mask_words * 4);
        });
        if (rc) return rc;
        a.Q = reinterpret_cast<const float*>(dev + sc.q);
        a.mask = masked ? reinterpret_cast<const uint32_t*>(dev + sc.mask) : nullptr;
        ra.offs = reinterpret_cast<const int64_t*>(dev + sc.offs);
        ra.out_s = reinterpret_cast<float*>(dev + sc.out_s);
        ra.out_g = reinterpret_cast<int32_t*>(dev + sc.out_g);
        ra.out_sum = out_sums ? reinterpret_cast<double*>(dev + sc.out_sum) : nullptr;
    }
    unsigned long long* T = reinterpret_cast<unsigned long long*>(dev + sc.T);
    // the table and the rank kernel's per-set counters, zeroed together
    HIP_TRY(hipMemsetAsync(T, 0, (size_t)sc.zero_bytes, st));
    if (scan) {
        double* qn64 = reinterpret_cast<double*>(dev + sc.qn64);
        // the canonical query norms, nothing else: no query tiles
        HIP_TRY(launch_prep_queries(a.Q, n_sub, n_sub, D, ix->G, ix->metric, nullptr, nullptr, qn64, nullptr, nullptr,
                                    nullptr, nullptr, nullptr, st));
        a.qn64 = qn64;
        a.X = ix->X; a.G = ix->G; a.D = D; a.nrm64 = ix->nrm64; a.N = N;
        a.groups = ix->groups; a.n_slots = n_group_slots; a.T = T;
        // block after block on this stream into the one table; the first counts the rows it skips
        for (int b0 = 0; b0 < n_sub; b0 += sc.block) {
            a.skipped = b0 == 0 ? ix->d_xmax + kMaxsimSkippedWord : nullptr;
            HIP_TRY(launch_maxsim_scan(ix->metric, a, b0, std::min(sc.block, n_sub - b0), st));
        }
    }
    // one rank launch for all sets (an empty index or a call without sub-queries: it reads no table
    // and every slot is "no result"; a device-memory call's bad sets are still counted)
    ra.T = T; ra.n_slots = scan ? n_group_slots : 1; ra.scanned = scan ? 1 : 0;
    ra.n_sub = n_sub; ra.k = k; ra.KE = sc.KE;
    ra.lk = reinterpret_cast<double*>(dev + sc.lk); ra.li = reinterpret_cast<uint32_t*>(dev + sc.li);
    ra.mk = reinterpret_cast<double*>(dev + sc.mk); ra.mi = reinterpret_cast<uint32_t*>(dev + sc.mi);
    ra.done = reinterpret_cast<int*>(dev + sc.done);
    ra.bad = ix->d_xmax + kMaxsimBadWord;
    HIP_TRY(launch_maxsim_rank(ra, n_sets, sc.n_seg, st));
    if (host) {
        const char* r = nullptr;
        rc = stage_down(w, sc.in_bytes, sc.out0, sc.out_bytes, st, &r);
        if (rc) return rc;
        std::memcpy(out_scores, r + (sc.out_s - sc.out0), (size_t)n_sets * k * 4);
        std::memcpy(out_groups, r + (sc.out_g - sc.out0), (size_t)n_sets * k * 4);
        if (out_sums) std::memcpy(out_sums, r + (sc.out_sum - sc.out0), (size_t)n_sets * k * 8);
    }
    ix->n_maxsim_searches++;
    ix->n_maxsim_sets += n_sets;
    return VDB_OK;
}

int32_t vdb_index_search(vdb_index* ix, const float* queries, int32_t B, int32_t k, const uint32_t* row_mask,
                         int32_t mem, float* out_scores, int64_t* out_indices, double* out_keys,
                         int64_t index_offset, void* stream) {
    int32_t rc = search_impl(ix, queries, B, k, row_mask, mem, out_scores, out_indices, out_keys, index_offset, stream,
                             nullptr);
    if (rc == kRetryBf16x3)
        rc = search_impl(ix, queries, B, k, row_mask, mem, out_scores, out_indices, out_keys, index_offset, stream,
                         nullptr, true);
    return rc;
}

}  // extern "C"

// ---- internal hooks for the multi-device set (vdb_shards.cpp) ----------------------------
namespace vdb {
int32_t index_search_rows(vdb_index* ix, const float* queries, int32_t B, int32_t k, const uint32_t* row_mask,
                          float* out_scores, int64_t* out_indices, double* out_keys, void* stream,
                          const int64_t* row_ids) {
    int32_t rc = search_impl(ix, queries, B, k, row_mask, VDB_MEM_DEVICE, out_scores, out_indices, out_keys, 0,
                             stream, row_ids);
    if (rc == kRetryBf16x3)  // a batch too large for the device-gated fallback: rerun in bf16x3
        rc = search_impl(ix, queries, B, k, row_mask, VDB_MEM_DEVICE, out_scores, out_indices, out_keys, 0, stream,
                         row_ids, true);
    return rc;
}
// Drop rows past `rows` (undo of a partial multi-shard add; rows past count are never read).
int32_t index_truncate(vdb_index* ix, int64_t rows) {
    std::unique_lock<std::shared_mutex> g(ix->mu);
    if (rows < ix->count) ix->count = rows;
    return VDB_OK;
}
int index_device(const vdb_index* ix) { return ix->device; }
int32_t set_error_msg(int code, const char* msg) { return set_error(code, "%s", msg); }
}  // namespace vdb

extern "C" {

int32_t vdb_merge_topk(const double* keys, const int64_t* idx, int32_t n_lists, int32_t nq, int32_t k_in,
                       int32_t k_out, int32_t metric, float* out_scores, int64_t* out_indices, double* out_keys,
                       void* stream) {
    if (!keys || !idx || !out_scores || !out_indices) return set_error(VDB_ERR_INVALID, "NULL argument");
    if (n_lists <= 0 || nq <= 0 || k_in <= 0 || k_out <= 0 || k_out > 1024 || k_in > 1024)
        return set_error(VDB_ERR_INVALID, "bad sizes n_lists=%d nq=%d k_in=%d k_out=%d", n_lists, nq, k_in, k_out);
    if (metric != 0 && metric != 1) return set_error(VDB_ERR_UNSUPPORTED, "metric %d", metric);
    hipStream_t st = (hipStream_t)stream;
    const int KP = std::max(32, next_pow2(std::max(k_in, k_out)));
    double* mk = nullptr;
    int64_t* mi = nullptr;
    HIP_TRY(hipMallocAsync((void**)&mk, (size_t)nq * KP * 8, st));
    HIP_TRY(hipMallocAsync((void**)&mi, (size_t)nq * KP * 8, st));
    // input [n_lists][nq][k_in]: list j of query q at j*nq*k_in + q*k_in
    HIP_TRY(launch_merge_f64_i64(KP, keys, idx, n_lists, k_in, k_in, (int64_t)nq * k_in, nq, mk, mi, st));
    HIP_TRY(launch_finalize_i64(metric, mk, mi, KP, nq, nullptr, k_out, out_scores, out_indices, out_keys, st));
    HIP_TRY(hipFreeAsync(mk, st));
    HIP_TRY(hipFreeAsync(mi, st));
    return VDB_OK;
}

int32_t vdb_similarity_matrix(const float* corpus, int64_t n, int32_t dim, const float* queries, int32_t nq,
                              int32_t metric, float* out, void* stream) {
    if (!corpus || !queries || !out) return set_error(VDB_ERR_INVALID, "NULL argument");
    if (n < 0 || dim <= 0 || nq <= 0) return set_error(VDB_ERR_INVALID, "bad sizes");
    if (metric < 0 || metric > 2) return set_error(VDB_ERR_UNSUPPORTED, "metric %d", metric);
    HIP_TRY(launch_similarity_matrix(corpus, n, dim, queries, nq, metric, out, (hipStream_t)stream));
    return VDB_OK;
}

int32_t vdb_normalize_rows(const float* in, int64_t n, int32_t dim, float* out, void* stream) {
    if ((!in || !out) && n > 0) return set_error(VDB_ERR_INVALID, "NULL argument");
    if (n < 0 || dim <= 0) return set_error(VDB_ERR_INVALID, "bad sizes");
    HIP_TRY(launch_normalize_rows(in, n, dim, out, (hipStream_t)stream));
    return VDB_OK;
}

int32_t vdb_topk_scores(const float* scores, int32_t rows, int64_t n, int32_t k, int32_t largest, int64_t* out_indices,
                        float* out_values, void* stream) {
    if (!scores || !out_indices) return set_error(VDB_ERR_INVALID, "NULL argument");
    if (rows <= 0 || n <= 0 || n > 0xFFFFFFFEll) return set_error(VDB_ERR_INVALID, "bad sizes rows=%d n=%lld", rows,
                                                                   (long long)n);
    if (k <= 0 || k > 1024 || k > n) return set_error(VDB_ERR_INVALID, "k must be in [1, min(n, 1024)], got %d", k);
    hipStream_t st = (hipStream_t)stream;
    void* ws = nullptr;
    HIP_TRY(hipMallocAsync(&ws, topk_workspace_bytes(n, rows, k), st));
    const hipError_t e = launch_topk_scores(scores, rows, n, k, largest, out_indices, out_values, ws, st);
    HIP_TRY(hipFreeAsync(ws, st));
    HIP_TRY(e);
    return VDB_OK;
}

}  // extern "C"

// =============================================================================
// Graph index (HNSW replacement, performance/hnsw_index.py:23-129)
// =============================================================================
struct vdb_graph {
    vdb_index* ix = nullptr;
    int R = 0;
    int knn = 0;                 // kNN candidates per row of the build (vdb_graph_add reuses it)
    int64_t n = 0;
    int64_t gen = 0;             // the index's generation at build / import / add (rows removed since: stale)
    int64_t cap = 0;             // rows the device neighbour array holds
    int n_entries = 0;
    int32_t* nbr = nullptr;      // device [cap][R]
    int32_t* entries = nullptr;  // device [n_entries]
    std::vector<int32_t> h_nbr;  // host mirror [n][R] (incremental updates re-prune from it)
    int teams = 1;               // workgroups per query (vdb_graph_set_param "teams")
    unsigned long long* d_stats = nullptr;
    std::atomic<int64_t> n_queries{0};
    int device = 0;  // the index's device (the graph may outlive an explicitly closed index)
    // last search queued on each stream (device memory): vdb_graph_destroy waits for these only
    std::mutex use_mu;
    std::unordered_map<hipStream_t, hipEvent_t> uses;
};

namespace {

int graph_upload(vdb_index* ix, int R, int64_t n, const int32_t* nbr_host, const int32_t* ent_host, int n_ent,
                 vdb_graph** out) {
    vdb_graph* g = new vdb_graph();
    g->ix = ix;
    g->device = ix->device;
    g->R = R;
    g->knn = R;
    g->n = n;
    g->gen = ix->gen.load();
    g->cap = std::max<int64_t>(n, 1);
    g->n_entries = n_ent;
    hipError_t e = hipMalloc(&g->nbr, (size_t)g->cap * R * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&g->entries, (size_t)std::max(n_ent, 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&g->d_stats, 64);
    if (e == hipSuccess) e = zero_now(g->d_stats, 64, ix->stream);
    if (e == hipSuccess && n > 0) e = hipMemcpy(g->nbr, nbr_host, (size_t)n * R * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_ent > 0)
        e = hipMemcpy(g->entries, ent_host, (size_t)n_ent * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(g->nbr);
        (void)hipFree(g->entries);
        (void)hipFree(g->d_stats);
        delete g;
        return set_error(e == hipErrorOutOfMemory ? VDB_ERR_OOM : VDB_ERR_HIP, "graph upload failed: %s",
                         hipGetErrorString(e));
    }
    g->h_nbr.assign(nbr_host, nbr_host + (size_t)n * R);
    *out = g;
    return VDB_OK;
}

// Exact kNN (kk incl. the row itself) of rows [r0, r1) over the whole index: the brute-force
// path with the rows as queries, 512 per launch.  kid [(r1 - r0) * kk] on the host.
int graph_knn(vdb_index* ix, int64_t r0, int64_t r1, int kk, std::vector<int64_t>& kid) {
    const int Bq = 512;
    const int D = ix->dim;
    kid.assign((size_t)(r1 - r0) * kk, -1);
    float* qbuf = nullptr;
    float* dsc = nullptr;
    int64_t* did = nullptr;
    hipStream_t st = ix->stream;
    hipError_t e = hipMalloc(&qbuf, (size_t)Bq * D * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&dsc, (size_t)Bq * kk * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&did, (size_t)Bq * kk * sizeof(int64_t));
    int rc = e == hipSuccess ? VDB_OK : set_error(VDB_ERR_OOM, "graph build buffers: %s", hipGetErrorString(e));
    for (int64_t q0 = r0; rc == VDB_OK && q0 < r1; q0 += Bq) {
        const int m = (int)std::min<int64_t>(Bq, r1 - q0);
        {
            std::shared_lock<std::shared_mutex> g(ix->mu);
            e = launch_unpack_rows(ix->X, ix->G, D, q0, m, qbuf, st);
        }
        if (e != hipSuccess) {
            rc = set_error(VDB_ERR_HIP, "graph build: %s", hipGetErrorString(e));
            break;
        }
        rc = vdb_index_search(ix, qbuf, m, kk, nullptr, VDB_MEM_DEVICE, dsc, did, nullptr, 0, st);
        if (rc) break;
        e = hipMemcpyAsync(kid.data() + (size_t)(q0 - r0) * kk, did, (size_t)m * kk * sizeof(int64_t),
                           hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = set_error(VDB_ERR_HIP, "graph build: %s", hipGetErrorString(e));
    }
    (void)hipFree(qbuf);
    (void)hipFree(dsc);
    (void)hipFree(did);
    return rc;
}

// graph_prune over n work items: candidate rows cv [n][cw] (-1 padded), optional node ids
// (else items 0..n), results hn [n][limit] (and distances hd).
int graph_prune_host(vdb_index* ix, const std::vector<int32_t>& cv, int cw, const std::vector<int32_t>* nodes,
                     int64_t n, int limit, int fill, int sort, int32_t* hn, float* hd) {
    if (n <= 0) return VDB_OK;
    hipStream_t st = ix->stream;
    int32_t *dcand = nullptr, *dnbr = nullptr, *dnodes = nullptr;
    float* ddist = nullptr;
    hipError_t e = hipMalloc(&dcand, (size_t)n * cw * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&dnbr, (size_t)n * limit * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&ddist, (size_t)n * limit * sizeof(float));
    if (e == hipSuccess && nodes) e = hipMalloc(&dnodes, (size_t)n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpyAsync(dcand, cv.data(), (size_t)n * cw * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && nodes)
        e = hipMemcpyAsync(dnodes, nodes->data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        GraphPruneArgs pa;
        std::shared_lock<std::shared_mutex> g(ix->mu);
        pa.X = ix->X; pa.G = ix->G;
        pa.rowscale = ix->metric == VDB_METRIC_COSINE ? ix->inv32 : ix->sq32;
        pa.cand = dcand; pa.cw = cw; pa.n_nodes = n; pa.limit = limit; pa.rw = limit; pa.fill = fill;
        pa.out_nbr = dnbr; pa.out_dist = ddist; pa.nodes = dnodes; pa.sort = sort;
        e = launch_graph_prune(ix->metric, pa, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(hn, dnbr, (size_t)n * limit * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && hd) e = hipMemcpyAsync(hd, ddist, (size_t)n * limit * sizeof(float), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dcand);
    (void)hipFree(dnbr);
    (void)hipFree(ddist);
    (void)hipFree(dnodes);
    return e == hipSuccess ? VDB_OK : set_error(VDB_ERR_HIP, "graph prune: %s", hipGetErrorString(e));
}

// Candidate rows of rows [r0, r1) from their kNN lists (self and -1 dropped), cw per row.
std::vector<int32_t> knn_candidates(const std::vector<int64_t>& kid, int64_t r0, int64_t r1, int kk, int cw) {
    std::vector<int32_t> cand((size_t)(r1 - r0) * cw, -1);
    for (int64_t i = r0; i < r1; ++i) {
        int c = 0;
        for (int j = 0; j < kk && c < cw; ++j) {
            const int64_t v = kid[(size_t)(i - r0) * kk + j];
            if (v < 0 || v == i) continue;
            cand[(size_t)(i - r0) * cw + c++] = (int32_t)v;
        }
    }
    return cand;
}

}  // namespace

extern "C" {

// entry rows of a graph: up to 256 every search team scores all of them; more (up to this many)
// are split into one spread slice of <= 256 per team (vdb_graph.hip)
constexpr int kGraphEntriesMax = 1 << 20;

int32_t vdb_graph_build(vdb_index* ix, int32_t degree, int32_t knn, int32_t n_entries, vdb_graph** out) {
    if (!ix || !out) return set_error(VDB_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (degree < 2 || degree > 64 || (degree & 1)) return set_error(VDB_ERR_INVALID, "degree must be even in [2, 64]");
    if (knn < degree / 2 || knn > 200) return set_error(VDB_ERR_INVALID, "knn must be in [degree/2, 200]");
    if (n_entries < 1 || n_entries > kGraphEntriesMax)
        return set_error(VDB_ERR_INVALID, "n_entries must be in [1, %d]", kGraphEntriesMax);
    HIP_TRY(hipSetDevice(ix->device));
    const int64_t N = ix->count;
    if (N > 0x7FFFFFFF) return set_error(VDB_ERR_INVALID, "graph rows are int32");
    const int R = degree, F = degree / 2;
    const int kk = (int)std::min<int64_t>(knn + 1, std::max<int64_t>(N, 1));  // + the row itself
    std::vector<int32_t> nbr((size_t)N * R, -1);
    if (N > 1) {
        // 1. exact kNN of every row (the brute-force path, rows as queries)
        std::vector<int64_t> kid;
        int rc = graph_knn(ix, 0, N, kk, kid);
        if (rc) return rc;
        // 2. hnswlib-style selection: pass 1 keeps <= M = R/2 diverse
        //    out-edges from the kNN; pass 2 re-selects <= R from out- plus in-edges
        //    (hnswlib's level-0 lists: the node's own links plus the links of later
        //    insertions that chose it, re-pruned when they exceed 2M).
        const int CW = std::min(knn, 63);
        std::vector<int32_t> cand = knn_candidates(kid, 0, N, kk, CW);
        kid.clear(); kid.shrink_to_fit();
        std::vector<int32_t> fwd((size_t)N * F);
        std::vector<float> fdist((size_t)N * F);
        rc = graph_prune_host(ix, cand, CW, nullptr, N, F, 0, 0, fwd.data(), fdist.data());
        if (rc) return rc;
        cand.clear(); cand.shrink_to_fit();
        // pool of v: out-edges of v and in-edges u -> v, nearest first, <= 63
        std::vector<int64_t> roff(N + 1, 0);
        for (size_t t = 0; t < fwd.size(); ++t)
            if (fwd[t] >= 0) roff[fwd[t] + 1]++;
        for (int64_t i = 0; i < N; ++i) roff[i + 1] += roff[i];
        std::vector<std::pair<float, int32_t>> rev(roff[N]);
        std::vector<int64_t> rpos(roff.begin(), roff.end() - 1);
        for (int64_t u = 0; u < N; ++u)
            for (int j = 0; j < F; ++j) {
                const int32_t w = fwd[(size_t)u * F + j];
                if (w >= 0) rev[rpos[w]++] = {fdist[(size_t)u * F + j], (int32_t)u};
            }
        std::vector<int32_t> cand2((size_t)N * 63, -1);
        std::vector<std::pair<float, int32_t>> pool;
        for (int64_t v = 0; v < N; ++v) {
            pool.clear();
            for (int j = 0; j < F; ++j)
                if (fwd[(size_t)v * F + j] >= 0) pool.push_back({fdist[(size_t)v * F + j], fwd[(size_t)v * F + j]});
            pool.insert(pool.end(), rev.begin() + roff[v], rev.begin() + roff[v + 1]);
            std::sort(pool.begin(), pool.end(), [](const std::pair<float, int32_t>& x, const std::pair<float, int32_t>& y) {
                return x.first < y.first || (x.first == y.first && x.second < y.second);
            });
            int c = 0;
            int32_t* row = cand2.data() + (size_t)v * 63;
            for (size_t t = 0; t < pool.size() && c < 63; ++t) {
                bool dup = false;
                for (int q = c - 1; q >= 0 && !dup; --q) dup = row[q] == pool[t].second;
                if (!dup) row[c++] = pool[t].second;
            }
        }
        rc = graph_prune_host(ix, cand2, 63, nullptr, N, R, (int)ix->graph_fill, 0, nbr.data(), nullptr);
        if (rc) return rc;
    }
    // 3. entry rows: evenly spread
    const int E = (int)std::min<int64_t>(n_entries, std::max<int64_t>(N, 1));
    std::vector<int32_t> ent(E);
    for (int i = 0; i < E; ++i) ent[i] = (int32_t)((int64_t)i * N / E);
    const int rc = graph_upload(ix, R, N, nbr.data(), ent.data(), N > 0 ? E : 0, out);
    if (rc == VDB_OK) (*out)->knn = knn;
    return rc;
}

// Incremental insertion of the rows the index gained since the graph was built (hnswlib
// inserts one row at a time; here a whole batch): exact kNN of the new rows over all rows,
// pass-1 selection of their out-edges, then every node that gains an in-edge (old or new)
// re-selects <= R from its current list plus the new in-edges (pass 2 with the candidates
// ordered by distance in the kernel).  Old rows' other links are kept.
int32_t vdb_graph_add(vdb_graph* g) {
    if (!g) return set_error(VDB_ERR_INVALID, "graph is NULL");
    vdb_index* ix = g->ix;
    HIP_TRY(hipSetDevice(ix->device));
    const int64_t n0 = g->n, N = ix->count;
    if (g->gen != ix->gen.load())
        return set_error(VDB_ERR_INVALID, "graph is stale: rows were removed from or updated in the index since it was built");
    if (N < n0) return set_error(VDB_ERR_INVALID, "index has fewer rows (%lld) than the graph (%lld)", (long long)N,
                                 (long long)n0);
    if (N == n0) return VDB_OK;
    if (N > 0x7FFFFFFF) return set_error(VDB_ERR_INVALID, "graph rows are int32");
    const int R = g->R, F = std::max(1, R / 2);
    const int knn = std::max(g->knn, F);
    const int kk = (int)std::min<int64_t>(knn + 1, N);
    const int64_t nn = N - n0;
    // 1. new rows' out-edges
    std::vector<int64_t> kid;
    int rc = graph_knn(ix, n0, N, kk, kid);
    if (rc) return rc;
    const int CW = std::min(knn, 63);
    std::vector<int32_t> cand = knn_candidates(kid, n0, N, kk, CW);
    kid.clear(); kid.shrink_to_fit();
    std::vector<int32_t> nodes(nn);
    for (int64_t i = 0; i < nn; ++i) nodes[i] = (int32_t)(n0 + i);
    std::vector<int32_t> fwd((size_t)nn * F);
    rc = graph_prune_host(ix, cand, CW, &nodes, nn, F, 0, 0, fwd.data(), nullptr);
    if (rc) return rc;
    // 2. pools: affected node v -> its current list (new rows: their out-edges) + in-edges
    std::unordered_map<int32_t, std::vector<int32_t>> in;
    for (int64_t i = 0; i < nn; ++i)
        for (int j = 0; j < F; ++j) {
            const int32_t w = fwd[(size_t)i * F + j];
            if (w >= 0) in[w].push_back((int32_t)(n0 + i));
        }
    std::vector<int32_t> aff(nodes);
    for (const auto& kv : in)
        if (kv.first < n0) aff.push_back(kv.first);
    std::vector<int32_t> cand2(aff.size() * 63, -1);
    for (size_t a = 0; a < aff.size(); ++a) {
        const int32_t v = aff[a];
        int32_t* row = cand2.data() + a * 63;
        int c = 0;
        auto push = [&](int32_t u) {
            if (u < 0 || u == v || c >= 63) return;
            for (int q = 0; q < c; ++q)
                if (row[q] == u) return;
            row[c++] = u;
        };
        if (v >= n0) {
            for (int j = 0; j < F; ++j) push(fwd[(size_t)(v - n0) * F + j]);
        } else {
            for (int j = 0; j < R; ++j) push(g->h_nbr[(size_t)v * R + j]);
        }
        auto it = in.find(v);
        if (it != in.end())
            for (int32_t u : it->second) push(u);
    }
    std::vector<int32_t> upd(aff.size() * R);
    rc = graph_prune_host(ix, cand2, 63, &aff, (int64_t)aff.size(), R, (int)ix->graph_fill, 1, upd.data(), nullptr);
    if (rc) return rc;
    // 3. device array: grow (doubling) and scatter the updated lists
    hipStream_t st = ix->stream;
    if (N > g->cap) {
        int64_t cap = std::max<int64_t>(g->cap * 2, 1024);
        while (cap < N) cap *= 2;
        int32_t* nb = nullptr;
        HIP_TRY(hipMalloc(&nb, (size_t)cap * R * sizeof(int32_t)));
        hipError_t e = hipMemcpyAsync(nb, g->nbr, (size_t)n0 * R * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFree(nb);
            return set_error(VDB_ERR_HIP, "graph grow: %s", hipGetErrorString(e));
        }
        {
            const int wr = wait_idle(ix);  // graph searches that read the old array are done
            if (wr) return wr;
        }
        (void)hipFree(g->nbr);
        g->nbr = nb;
        g->cap = cap;
    }
    g->h_nbr.resize((size_t)N * R, -1);
    for (size_t a = 0; a < aff.size(); ++a)
        std::memcpy(g->h_nbr.data() + (size_t)aff[a] * R, upd.data() + a * R, R * sizeof(int32_t));
    int32_t *dids = nullptr, *drows = nullptr;
    hipError_t e = hipMalloc(&dids, aff.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&drows, upd.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpyAsync(dids, aff.data(), aff.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(drows, upd.data(), upd.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_graph_scatter(g->nbr, R, dids, drows, (int64_t)aff.size(), st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dids);
    (void)hipFree(drows);
    if (e != hipSuccess) return set_error(VDB_ERR_HIP, "graph update: %s", hipGetErrorString(e));
    g->n = N;
    return VDB_OK;
}

int32_t vdb_graph_import(vdb_index* ix, int32_t degree, int64_t n, const int32_t* nbr, int32_t n_entries,
                         const int32_t* entries, vdb_graph** out) {
    if (!ix || !out || (n > 0 && !nbr) || (n_entries > 0 && !entries)) return set_error(VDB_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (degree < 1 || degree > 64) return set_error(VDB_ERR_INVALID, "degree must be in [1, 64]");
    if (n != ix->count) return set_error(VDB_ERR_INVALID, "graph has %lld rows, index %lld", (long long)n, (long long)ix->count);
    if (n_entries < 0 || n_entries > kGraphEntriesMax)
        return set_error(VDB_ERR_INVALID, "n_entries must be in [0, %d]", kGraphEntriesMax);
    for (int64_t i = 0; i < n * degree; ++i)
        if (nbr[i] < -1 || nbr[i] >= n) return set_error(VDB_ERR_INVALID, "neighbour id out of range at %lld", (long long)i);
    for (int i = 0; i < n_entries; ++i)
        if (entries[i] < 0 || entries[i] >= n) return set_error(VDB_ERR_INVALID, "entry id out of range");
    // The search kernel ranks the entries by counting the better ones: a repeated row would share
    // its rank with its copy and leave a beam slot that is counted but never written.
    std::vector<int32_t> sorted_ent(entries, entries + n_entries);
    std::sort(sorted_ent.begin(), sorted_ent.end());
    const auto rep = std::adjacent_find(sorted_ent.begin(), sorted_ent.end());
    if (rep != sorted_ent.end()) return set_error(VDB_ERR_INVALID, "entry row %d is repeated", (int)*rep);
    HIP_TRY(hipSetDevice(ix->device));
    return graph_upload(ix, degree, n, nbr, entries, n_entries, out);
}

int32_t vdb_graph_info(const vdb_graph* g, int64_t* n_rows, int32_t* degree, int32_t* n_entries) {
    if (!g) return set_error(VDB_ERR_INVALID, "graph is NULL");
    if (n_rows) *n_rows = g->n;
    if (degree) *degree = g->R;
    if (n_entries) *n_entries = g->n_entries;
    return VDB_OK;
}

int32_t vdb_graph_export(const vdb_graph* g, int32_t* nbr_host, int32_t* entries_host) {
    if (!g) return set_error(VDB_ERR_INVALID, "graph is NULL");
    HIP_TRY(hipSetDevice(g->ix->device));
    if (nbr_host && g->n > 0)
        HIP_TRY(hipMemcpy(nbr_host, g->nbr, (size_t)g->n * g->R * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (entries_host && g->n_entries > 0)
        HIP_TRY(hipMemcpy(entries_host, g->entries, (size_t)g->n_entries * sizeof(int32_t), hipMemcpyDeviceToHost));
    return VDB_OK;
}

int32_t vdb_graph_search(vdb_graph* g, const float* queries, int32_t nq, int32_t k, int32_t ef, int32_t mem,
                         int64_t* labels, float* distances, void* stream) {
    if (!g || !queries || !labels || !distances) return set_error(VDB_ERR_INVALID, "NULL argument");
    if (nq <= 0) return set_error(VDB_ERR_INVALID, "n_queries must be >= 1");
    if (ef < 1 || ef > 256) return set_error(VDB_ERR_INVALID, "ef must be in [1, 256], got %d", ef);
    if (k < 1 || k > ef) return set_error(VDB_ERR_INVALID, "k must be in [1, ef], got k=%d ef=%d", k, ef);
    if (mem != VDB_MEM_HOST && mem != VDB_MEM_DEVICE) return set_error(VDB_ERR_INVALID, "bad mem kind %d", mem);
    vdb_index* ix = g->ix;
    const int D = ix->dim;
    if (mem == VDB_MEM_HOST && !all_finite(queries, (int64_t)nq * D))
        return set_error(VDB_ERR_NONFINITE, "query contains NaN or Inf");
    HIP_TRY(hipSetDevice(ix->device));
    std::shared_lock<std::shared_mutex> lk(ix->mu);
    if (ix->count != g->n) return set_error(VDB_ERR_INVALID, "graph is stale: %lld rows, index %lld", (long long)g->n,
                                            (long long)ix->count);
    if (ix->gen.load() != g->gen)
        return set_error(VDB_ERR_INVALID, "graph is stale: rows were removed from or updated in the index since it was built");
    // device memory: the caller's stream, NULL = the null stream (ordered with the caller's
    // default-stream work, e.g. PyTorch's); host memory: NULL = the index's own stream
    hipStream_t st = (stream || mem == VDB_MEM_DEVICE) ? (hipStream_t)stream : ix->stream;
    const float* Qd = queries;
    int64_t* ol = labels;
    float* od = distances;
    void* tmp = nullptr;
    const int T = (int)std::min<int64_t>(g->teams, std::max(g->n_entries, 1));
    const size_t qb = mem == VDB_MEM_HOST ? (size_t)nq * D * 4 : 0, lb = (size_t)nq * k * 8, db = (size_t)nq * k * 4;
    const size_t tb = T > 1 ? (size_t)nq * T * k * 12 + 512 : 0;
    if (mem == VDB_MEM_HOST || T > 1) {
        HIP_TRY(hipMallocAsync(&tmp, qb + lb + db + tb + 1024, st));
        char* base = (char*)tmp;
        if (mem == VDB_MEM_HOST) {
            HIP_TRY(hipMemcpyAsync(base, queries, qb, hipMemcpyHostToDevice, st));
            Qd = (const float*)base;
            ol = (int64_t*)(base + ((qb + 255) & ~size_t(255)));
            od = (float*)((char*)ol + ((lb + 255) & ~size_t(255)));
        }
    }
    GraphSearchArgs a;
    a.rows = ix->X; a.Dp = ix->Dp; a.D = D; a.rowscale = ix->metric == 0 ? ix->inv32 : ix->sq32; a.n_rows = g->n;
    a.nbr = g->nbr; a.R = g->R; a.entries = g->entries; a.n_entries = g->n_entries;
    a.Q = Qd; a.k = k; a.ef = ef; a.out_lab = ol; a.out_dist = od; a.stats = g->d_stats;
    a.teams = T;
    if (T > 1) {
        char* tbase = (char*)tmp + ((qb + 255) & ~size_t(255)) + ((lb + 255) & ~size_t(255)) + ((db + 255) & ~size_t(255));
        a.tmp_lab = (int64_t*)tbase;
        a.tmp_dist = (float*)(tbase + (((size_t)nq * T * k * 8 + 255) & ~size_t(255)));
    }
    if (g->n == 0) {
        HIP_TRY(hipMemsetAsync(ol, 0xFF, (size_t)nq * k * 8, st));
    } else {
        HIP_TRY(launch_graph_search(ix->metric, a, nq, st));
    }
    g->n_queries += nq;
    if (mem == VDB_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(labels, ol, (size_t)nq * k * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(distances, od, (size_t)nq * k * 4, hipMemcpyDeviceToHost, st));
    }
    if (tmp) HIP_TRY(hipFreeAsync(tmp, st));
    if (mem == VDB_MEM_HOST) HIP_TRY(hipStreamSynchronize(st));
    else {
        const int nr = note_use(ix, st);  // a later resize of the index waits for this search
        if (nr) return nr;
        std::lock_guard<std::mutex> lg(g->use_mu);  // and so does the graph's destroy
        hipEvent_t& ev = g->uses[st];
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ev, st));
    }
    return VDB_OK;
}

int32_t vdb_graph_set_param(vdb_graph* g, const char* name, int64_t value) {
    if (!g || !name) return set_error(VDB_ERR_INVALID, "NULL argument");
    const std::string n(name);
    if (n == "teams") {
        if (value < 1 || value > 256) return set_error(VDB_ERR_INVALID, "teams must be in [1, 256]");
        g->teams = (int)value;
    } else {
        return set_error(VDB_ERR_INVALID, "unknown graph parameter '%s'", name);
    }
    return VDB_OK;
}

int32_t vdb_graph_stat(const vdb_graph* g, const char* name, int64_t* value) {
    if (!g || !name || !value) return set_error(VDB_ERR_INVALID, "NULL argument");
    std::string n(name);
    if (n == "queries") {
        *value = g->n_queries.load();
    } else if (n == "iterations" || n == "visited") {
        unsigned long long v[2] = {0, 0};
        HIP_TRY(hipMemcpy(v, g->d_stats, sizeof(v), hipMemcpyDeviceToHost));
        *value = (int64_t)v[n == "visited" ? 1 : 0];
    } else {
        return set_error(VDB_ERR_INVALID, "unknown graph stat '%s'", name);
    }
    return VDB_OK;
}

int32_t vdb_graph_destroy(vdb_graph* g) {
    if (!g) return VDB_OK;
    (void)hipSetDevice(g->device);
    for (auto& kv : g->uses) {  // its own searches only: the index may already be closed
        (void)hipEventSynchronize(kv.second);
        (void)hipEventDestroy(kv.second);
    }
    (void)hipFree(g->nbr);
    (void)hipFree(g->entries);
    (void)hipFree(g->d_stats);
    delete g;
    return VDB_OK;
}

}  // extern "C"
