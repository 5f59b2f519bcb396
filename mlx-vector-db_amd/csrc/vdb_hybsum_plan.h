// vdb_hybsum_plan.h — the host arithmetic of vdb_index_search_hybrid_sum (vdb_api.cpp) and the
// decisions its kernels share with it (vdb_hybsum.hip): the limits, the combination of a row's two
// keys, how the rows are dealt to workgroups (the sparse search's deal, vdb_sparse_plan.h), the
// workgroups per query, the LDS size, the per-call scratch and the validation of a call (one enum
// value per cause).  Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a
// sanitizer (tools/hybsum_plan_check.cpp).
#pragma once
#include <stdint.h>

#include "vdb_sparse_plan.h"

namespace vdb {

constexpr int kHybsumMaxK = kSparseMaxK;       // 1024, as the sparse search
constexpr int kHybsumMaxQueries = 65535;       // the grid's second dimension
constexpr int kHybsumMaxSeg = kSparseMaxSeg;   // most workgroups per query (the tail merge's list heads)
constexpr int kHybsumNB = 4;                   // rows whose dense keys a wave forms together
// The greatest weight: 2^64.  |dense key| and |sparse key| are below 2^280 for any finite fp32 input,
// so every product is finite and no sum is inf - inf.
constexpr double kHybsumMaxWeight = 18446744073709551616.0;

// finite, >= 0 and <= 2^64 (a NaN fails both comparisons)
VDB_SPARSE_HD inline bool hybsum_weight_ok(double w) { return w >= 0.0 && w <= kHybsumMaxWeight; }

// The value a row is ranked by: four separate fp64 operations.  The last add turns -0.0 into +0.0,
// so equal values have equal bits.
VDB_SPARSE_HD inline double hybsum_combine(double w_dense, double kd, double w_sparse, double ks) {
    const double t1 = w_dense * kd;
    const double t2 = w_sparse * ks;
    const double u = t1 + t2;
    return u + 0.0;
}

// ---- the deal of rows ---------------------------------------------------------------------------
// As the sparse search: chunks of kSparseChunk rows (sparse_n_chunks), segment s walks chunks s, s +
// n_seg, ... (sparse_live_segs of them have any), lane `lane` of wave `wv` takes sparse_row_of(c, wv,
// lane).  The dense keys of a wave's 64 rows are formed kHybsumNB at a time: batch t holds the rows
// of lanes [kHybsumNB t, kHybsumNB t + kHybsumNB), and lane kHybsumNB t + u keeps row u's key.
VDB_SPARSE_HD inline int hybsum_batch_of(int lane) { return lane / kHybsumNB; }
VDB_SPARSE_HD inline int hybsum_slot_of(int lane) { return lane % kHybsumNB; }
// Workgroups per query.  knob ("hybrid_sum_wgs") > 0 forces it; 0 = auto, as sparse_n_seg.
inline int hybsum_n_seg(int64_t knob, int64_t N, int n_queries, int n_cu) { return sparse_n_seg(knob, N, n_queries, n_cu); }
// The dense key's form: rows of up to 1024 dims hold 4 pieces per lane in registers, up to 2048 dims
// 8; 0 = any length, one piece per row in flight per trip (as the row-list search chooses).
inline int hybsum_mp(int dim) { return dim <= 1024 ? 4 : dim <= 2048 ? 8 : 0; }

// ---- scratch --------------------------------------------------------------------------------------
// LDS of one workgroup: the query's terms and weights, then the four WaveTopK buffers (or the tail
// merge's buffer, which takes their place), as sparse_lds_bytes.
inline int64_t hybsum_lds_bytes(int64_t cap, int64_t merge_lds) { return sparse_lds_bytes(cap, merge_lds); }
struct HybsumScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t done, qn64, lk, li, mk, mi, rows;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, indptr, terms, weights, mask, in_bytes, out0, out_s, out_i, out_f, out_d, out_p, out_bytes;
    int64_t mask_words, total;
};
// rows: the local row id of every slot, kept for the parts kernel (parts: out_dense or out_sparse given)
inline HybsumScratch hybsum_scratch(int n_queries, int dim, int k, int n_seg, int64_t q_nnz, int64_t rows, bool host,
                                    bool masked, bool fused, bool dense, bool sparse) {
    HybsumScratch s{};
    const int64_t B = n_queries, KE = sparse_ke(k);
    s.mask_words = (rows + 31) / 32;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += sparse_align(bytes);
        return at;
    };
    s.done = take(B * 4);
    s.qn64 = take(B * 8);
    s.lk = take(n_seg > 1 ? B * n_seg * KE * 8 : 0);
    s.li = take(n_seg > 1 ? B * n_seg * KE * 4 : 0);
    s.mk = take(n_seg > 1 ? B * KE * 8 : 0);
    s.mi = take(n_seg > 1 ? B * KE * 4 : 0);
    s.rows = take(dense || sparse ? B * k * 4 : 0);
    s.in0 = o;
    if (host) {
        s.q = take(B * dim * 4);
        s.indptr = take((B + 1) * 8);
        s.terms = take(q_nnz * 4);
        s.weights = take(q_nnz * 4);
        s.mask = take(masked ? s.mask_words * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_s = take(B * k * 4);
        s.out_i = take(B * k * 8);
        s.out_f = take(fused ? B * k * 8 : 0);
        s.out_d = take(dense ? B * k * 8 : 0);
        s.out_p = take(sparse ? B * k * 8 : 0);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation of a call -------------------------------------------------------------------------
// Both memory kinds, before anything is launched.  (A host-memory call's sparse queries:
// sparse_validate_queries; its dense queries: finite.)
enum {
    kHybsumOk = 0,
    kHybsumBadCounts = 1,       // n_queries or q_nnz < 0
    kHybsumBadK = 2,            // k outside [1, kHybsumMaxK]
    kHybsumBadMem = 3,          // a memory kind that is neither host (0) nor device (1)
    kHybsumNullPointer = 4,     // queries / q_indptr / out_scores / out_indices with n_queries > 0, or terms / weights with q_nnz > 0
    kHybsumNoColumn = 5,        // no sparse column attached (or one that does not cover the rows)
    kHybsumTooManyQueries = 6,  // n_queries above kHybsumMaxQueries
    kHybsumBadWeight = 7        // w_dense or w_sparse NaN, negative or above 2^64
};
inline int hybsum_validate_call(int64_t n_queries, int64_t q_nnz, int k, double w_dense, double w_sparse, bool has_queries,
                                bool has_indptr, bool has_terms, bool has_weights, bool has_scores, bool has_indices,
                                int mem, bool column) {
    if (n_queries > kHybsumMaxQueries) return kHybsumTooManyQueries;
    if (!hybsum_weight_ok(w_dense) || !hybsum_weight_ok(w_sparse)) return kHybsumBadWeight;
    if (n_queries > 0 && !has_queries) return kHybsumNullPointer;
    switch (sparse_validate_call(n_queries, q_nnz, k, has_indptr, has_terms, has_weights, has_scores, has_indices, mem,
                                 column)) {
        case kSparseOk: return kHybsumOk;
        case kSparseBadCounts: return kHybsumBadCounts;
        case kSparseBadK: return kHybsumBadK;
        case kSparseBadMem: return kHybsumBadMem;
        case kSparseNullPointer: return kHybsumNullPointer;
        default: return kHybsumNoColumn;
    }
}

}  // namespace vdb
