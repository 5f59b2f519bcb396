// vdb_sparse_plan.h — the host arithmetic of vdb_index_set_sparse, vdb_index_search_sparse and
// vdb_index_search_hybrid (vdb_api.cpp) and the decisions their kernels share with it
// (vdb_sparse.hip): the limits, how the rows are cut into chunks and dealt to workgroups, the clamp
// of a device call's query offsets and what makes a query bad, the term search, one step of a row's
// key, the per-call scratch, and the validation of the column and of the queries (one enum value per
// cause).  Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/sparse_plan_check.cpp).
#pragma once
#include <stdint.h>

#include "vdb_fuse_plan.h"

#ifdef __HIPCC__
#define VDB_SPARSE_HD __host__ __device__
#else
#define VDB_SPARSE_HD
#endif

namespace vdb {

// A workgroup is 4 waves; one lane takes one row, so a wave scores 64 rows per trip and a chunk, the
// rows one workgroup handles per trip, is 256 rows: wave w takes [64 w, 64 w + 64) of it.
constexpr int kSparseWaves = 4;
constexpr int kSparseWaveRows = 64;
constexpr int kSparseChunk = kSparseWaves * kSparseWaveRows;  // 256 rows
// Most workgroups per query (the tail merge's list heads, vdb_merge_block.h MERGE_HEADS).
constexpr int kSparseMaxSeg = 512;
// Workgroups the grid aims for per CU (a workgroup at k = 1024 holds 104 KiB of LDS: one per CU; at
// small k several fit and hide each other's gather latency).
constexpr int kSparseWgPerCu = 4;
constexpr int kSparseMaxK = 1024;
constexpr int kSparseMaxQueryTerms = 1024;  // a query's terms and weights in LDS: 8 KiB
constexpr int64_t kSparseQueryLds = (int64_t)kSparseMaxQueryTerms * 8;

// One stored entry: the term id and its weight side by side, so one 8-byte load brings both.
struct SparsePair {
    int32_t term;
    float weight;
};

inline int sparse_ke(int k) {  // the top-k width: max(32, next_pow2(k)), as the exact scan's
    int p = 32;
    while (p < k) p <<= 1;
    return p;
}

// ---- the deal of rows ---------------------------------------------------------------------------
// Chunks of N rows, and the workgroups of a query that have any: segment s walks chunks s, s + n_seg,
// ..., so segments at or past the chunk count have nothing to do.
VDB_SPARSE_HD inline int64_t sparse_n_chunks(int64_t N) { return N <= 0 ? 0 : (N + kSparseChunk - 1) / kSparseChunk; }
VDB_SPARSE_HD inline int sparse_live_segs(int64_t N, int n_seg) {
    const int64_t c = sparse_n_chunks(N);
    return c < n_seg ? (int)c : n_seg;
}
// The row lane `lane` of wave `wv` takes in chunk c (at or past N: none).
VDB_SPARSE_HD inline int64_t sparse_row_of(int64_t c, int wv, int lane) {
    return c * kSparseChunk + (int64_t)wv * kSparseWaveRows + lane;
}
// Workgroups per query.  knob ("sparse_wgs") > 0 forces it; 0 = auto: one per chunk, capped so that
// the grid is about kSparseWgPerCu workgroups per CU.
inline int sparse_n_seg(int64_t knob, int64_t N, int n_queries, int n_cu) {
    if (knob > 0) return (int)(knob < kSparseMaxSeg ? knob : kSparseMaxSeg);
    int64_t chunks = sparse_n_chunks(N);
    int64_t cap = ((int64_t)n_cu * kSparseWgPerCu) / (n_queries > 0 ? n_queries : 1);
    if (cap < 1) cap = 1;
    if (chunks > cap) chunks = cap;
    if (chunks > kSparseMaxSeg) chunks = kSparseMaxSeg;
    return chunks < 1 ? 1 : (int)chunks;
}

// ---- a query's entries --------------------------------------------------------------------------
// Query b is entries [q_indptr[b], q_indptr[b + 1]).  A device-memory call is not validated: the
// range is clamped to [0, q_nnz] so that nothing out of bounds is read, and the query is bad (every
// slot "no result", counted in "sparse_bad_queries") when the clamp changed an offset, the offsets
// decrease or it has more than kSparseMaxQueryTerms entries.  len is the number of entries read: 0
// for a bad range.
struct SparseQRange {
    int64_t o0;
    int len;
    bool bad;
};
VDB_SPARSE_HD inline SparseQRange sparse_query_range(int64_t off_lo, int64_t off_hi, int64_t q_nnz) {
    SparseQRange r;
    r.o0 = off_lo < 0 ? 0 : off_lo > q_nnz ? q_nnz : off_lo;
    const int64_t o1 = off_hi < r.o0 ? r.o0 : off_hi > q_nnz ? q_nnz : off_hi;
    r.bad = off_lo < 0 || off_lo > q_nnz || off_hi > q_nnz || off_hi < off_lo || o1 - r.o0 > kSparseMaxQueryTerms;
    r.len = r.bad ? 0 : (int)(o1 - r.o0);
    return r;
}
// A term id is eligible when it names a term and is greater than the entry before it (prev = -1 for
// the first): a strictly ascending run of terms passes whole.
VDB_SPARSE_HD inline bool sparse_term_ok(int32_t term, int32_t prev, int32_t n_terms) {
    return term >= 0 && term < n_terms && term > prev;
}
// finite (a NaN fails both comparisons)
VDB_SPARSE_HD inline bool sparse_weight_ok(float w) { return w >= -3.4028234663852886e38f && w <= 3.4028234663852886e38f; }

// The position of term t among the query's len strictly ascending terms, -1 when it is not listed.
VDB_SPARSE_HD inline int sparse_find(const int32_t* qt, int len, int32_t t) {
    int lo = 0, hi = len;  // the answer, if any, lies in [lo, hi)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int32_t v = qt[mid];
        if (v == t) return mid;
        if (v < t)
            lo = mid + 1;
        else
            hi = mid;
    }
    return -1;
}
// One step of a row's key: every operation a separate fp64 operation.
VDB_SPARSE_HD inline double sparse_step(double acc, float w, double qd) {
    const double p = (double)w * qd;
    return acc + p;
}
VDB_SPARSE_HD inline bool sparse_entry_matches(float w, double qd) { return w != 0.0f && qd != 0.0; }

// The key of one row over plain arrays, as the kernel's lane forms it: the row's entries in stored
// order against the query's len terms qt / weights qw; *matched: some entry has w != 0 and qd != 0.
inline double sparse_row_key(const SparsePair* row, int64_t n_entries, const int32_t* qt, const float* qw, int len,
                             bool* matched) {
    double acc = 0.0;
    bool m = false;
    for (int64_t e = 0; e < n_entries; ++e) {
        const int j = sparse_find(qt, len, row[e].term);
        if (j < 0) continue;
        const double qd = (double)qw[j];
        acc = sparse_step(acc, row[e].weight, qd);
        m = m || sparse_entry_matches(row[e].weight, qd);
    }
    *matched = m;
    return acc;
}

// ---- scratch --------------------------------------------------------------------------------------
inline int64_t sparse_align(int64_t b) { return (b + 255) / 256 * 256; }
// LDS of one workgroup: the query, then the four WaveTopK buffers (or the tail merge's buffer, which
// takes their place): cap = WaveTopK capacity(KE), merge_lds = merge_block_lds(KE) when n_seg > 1.
inline int64_t sparse_lds_bytes(int64_t cap, int64_t merge_lds) {
    const int64_t tk = (int64_t)kSparseWaves * cap * 12;
    return kSparseQueryLds + (tk > merge_lds ? tk : merge_lds);
}
struct SparseScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t done, lk, li, mk, mi;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, indptr, terms, weights, mask, in_bytes, out0, out_s, out_i, out_k, out_bytes;
    int64_t mask_words, total;
};
inline SparseScratch sparse_scratch(int n_queries, int k, int n_seg, int64_t q_nnz, int64_t rows, bool host, bool masked,
                                    bool keys) {
    SparseScratch s{};
    const int64_t B = n_queries, KE = sparse_ke(k);
    s.mask_words = (rows + 31) / 32;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += sparse_align(bytes);
        return at;
    };
    s.done = take(B * 4);
    s.lk = take(n_seg > 1 ? B * n_seg * KE * 8 : 0);
    s.li = take(n_seg > 1 ? B * n_seg * KE * 4 : 0);
    s.mk = take(n_seg > 1 ? B * KE * 8 : 0);
    s.mi = take(n_seg > 1 ? B * KE * 4 : 0);
    s.in0 = o;
    if (host) {
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
        s.out_k = take(keys ? B * k * 8 : 0);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}
// The hybrid call: the dense lists ds / di / dk [B][F] as the inner search writes them, the set lists
// fs / fi / fk [2 B][F] as the fuse kernel reads them (list 2 b: query b's dense list, list 2 b + 1
// its sparse list), the sets' offsets [B + 1] and weights [2 B], and the sparse kernel's own scratch.
struct HybridScratch {
    int64_t ds, di, dk, fs, fi, fk, offs, w, done, lk, li, mk, mi;
    int64_t in0, q, indptr, terms, weights, mask, in_bytes, out0, out_s, out_i, out_f, out_h, out_bytes;
    int64_t mask_words, total;
};
inline HybridScratch hybrid_scratch(int n_queries, int dim, int k, int fetch_k, int n_seg, int64_t q_nnz, int64_t rows,
                                    bool host, bool masked, bool fused, bool hits) {
    HybridScratch s{};
    const int64_t B = n_queries, F = fetch_k, KE = sparse_ke(fetch_k);
    s.mask_words = (rows + 31) / 32;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += sparse_align(bytes);
        return at;
    };
    s.ds = take(B * F * 4);
    s.di = take(B * F * 8);
    s.dk = take(B * F * 8);
    s.fs = take(2 * B * F * 4);
    s.fi = take(2 * B * F * 8);
    s.fk = take(2 * B * F * 8);
    s.offs = take((B + 1) * 8);
    s.w = take(2 * B * 8);
    s.done = take(B * 4);
    s.lk = take(n_seg > 1 ? B * n_seg * KE * 8 : 0);
    s.li = take(n_seg > 1 ? B * n_seg * KE * 4 : 0);
    s.mk = take(n_seg > 1 ? B * KE * 8 : 0);
    s.mi = take(n_seg > 1 ? B * KE * 4 : 0);
    s.in0 = o;
    if (host) {
        s.q = take(B * dim * 4);
        s.indptr = take((B + 1) * 8);
        s.terms = take(q_nnz * 4);
        s.weights = take(q_nnz * 4);
        // (+ 64 zero words, as a host search's staged mask: the candidate passes read whole mask tiles)
        s.mask = take(masked ? (s.mask_words + 64) * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_s = take(B * k * 4);
        s.out_i = take(B * k * 8);
        s.out_f = take(fused ? B * k * 8 : 0);
        s.out_h = take(hits ? B * k * 4 : 0);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation of the column ---------------------------------------------------------------------
enum {
    kSparseColOk = 0,
    kSparseColBadCounts = 1,   // n != count, nnz < 0, n_terms < 1, or a NULL indptr with n != 0
    kSparseColNullPointer = 2, // terms / weights NULL with nnz > 0
    kSparseColBadIndptr = 3,   // indptr not ascending from 0 to nnz
    kSparseColBadTerm = 4,     // a term id outside [0, n_terms)
    kSparseColUnsorted = 5,    // a row whose term ids are not strictly ascending
    kSparseColNonFinite = 6    // a NaN or Inf weight
};
// What the scalars and the pointers' presence say, for both memory kinds.
inline int sparse_column_args(bool has_indptr, bool has_terms, bool has_weights, int64_t n, int64_t nnz, int32_t n_terms,
                              int64_t count) {
    if (!has_indptr) return n == 0 ? kSparseColOk : kSparseColBadCounts;  // detach
    if (n != count || nnz < 0 || n_terms < 1) return kSparseColBadCounts;
    if (nnz > 0 && (!has_terms || !has_weights)) return kSparseColNullPointer;
    return kSparseColOk;
}
// The column is checked in two passes, as the device-memory call's two kernels do it (one thread per
// row each).  First the offsets: row r's lie in [0, nnz] and ascend, the first row starts at 0 and the
// last ends at nnz.  When that holds for every row the rows' ranges tile [0, nnz): the second pass,
// which runs only then, reads each entry once and nothing outside [0, nnz).
VDB_SPARSE_HD inline bool sparse_column_offsets_ok(const int64_t* indptr, int64_t r, int64_t n, int64_t nnz) {
    const int64_t o0 = indptr[r], o1 = indptr[r + 1];
    return !(o0 < 0 || o1 < o0 || o1 > nnz || (r == 0 && o0 != 0) || (r == n - 1 && o1 != nnz));
}
// The entries of row r (its offsets passed the first pass): the cause with the lowest enum value
// found in this row.
VDB_SPARSE_HD inline int sparse_column_row(const int64_t* indptr, const int32_t* terms, const float* weights, int64_t r,
                                           int32_t n_terms) {
    const int64_t o0 = indptr[r], o1 = indptr[r + 1];
    int worst = kSparseColOk;
    int32_t prev = -1;
    for (int64_t e = o0; e < o1; ++e) {
        const int32_t t = terms[e];
        int c = kSparseColOk;
        if (t < 0 || t >= n_terms)
            c = kSparseColBadTerm;
        else if (t <= prev)
            c = kSparseColUnsorted;
        else if (!sparse_weight_ok(weights[e]))
            c = kSparseColNonFinite;
        if (c != kSparseColOk && (worst == kSparseColOk || c < worst)) worst = c;
        prev = t;
    }
    return worst;
}
// A host-memory call's column: the first row with bad offsets, else the first offending row's cause.
// *where: that row.
inline int sparse_validate_column(const int64_t* indptr, const int32_t* terms, const float* weights, int64_t n,
                                  int64_t nnz, int32_t n_terms, int64_t* where) {
    *where = 0;
    if (n == 0) return indptr[0] == 0 && nnz == 0 ? kSparseColOk : kSparseColBadIndptr;
    for (int64_t r = 0; r < n; ++r)
        if (!sparse_column_offsets_ok(indptr, r, n, nnz)) {
            *where = r;
            return kSparseColBadIndptr;
        }
    for (int64_t r = 0; r < n; ++r) {
        const int c = sparse_column_row(indptr, terms, weights, r, n_terms);
        if (c != kSparseColOk) {
            *where = r;
            return c;
        }
    }
    return kSparseColOk;
}
// The flag word of the device-memory call: bit c set for every cause c some row showed.  The call
// reports the lowest.
VDB_SPARSE_HD inline uint32_t sparse_column_flag(int cause) { return cause == kSparseColOk ? 0u : 1u << cause; }
inline int sparse_column_cause(uint32_t flags) {
    for (int c = kSparseColBadIndptr; c <= kSparseColNonFinite; ++c)
        if (flags & (1u << c)) return c;
    return kSparseColOk;
}

// ---- validation of a search -----------------------------------------------------------------------
enum {
    kSparseOk = 0,
    kSparseBadCounts = 1,    // n_queries or q_nnz < 0
    kSparseBadK = 2,         // k outside [1, kSparseMaxK]
    kSparseNullPointer = 3,  // q_indptr / out_scores / out_indices with n_queries > 0, or terms / weights with q_nnz > 0
    kSparseBadMem = 4,       // a memory kind that is neither host (0) nor device (1)
    kSparseNoColumn = 5,     // no sparse column attached (or one that does not cover the rows)
    kSparseBadOffsets = 6,   // host: offsets negative, decreasing or past q_nnz
    kSparseTooLong = 7,      // host: a query of more than kSparseMaxQueryTerms terms
    kSparseBadTerm = 8,      // host: a term id outside [0, n_terms)
    kSparseUnsorted = 9,     // host: a query whose term ids are not strictly ascending
    kSparseNonFinite = 10,   // host: a NaN or Inf weight
    // the hybrid call's own
    kHybridBadFetch = 11,    // fetch_k outside [k, kFuseMaxFetch] (k itself outside [1, kFuseMaxK]: kSparseBadK)
    kHybridBadWeight = 12,   // w_dense or w_sparse NaN, infinite or negative
    kHybridBadC = 13         // rrf_c NaN, infinite or negative
};
inline int sparse_validate_call(int64_t n_queries, int64_t q_nnz, int k, bool has_indptr, bool has_terms,
                                bool has_weights, bool has_scores, bool has_indices, int mem, bool column) {
    if (n_queries < 0 || q_nnz < 0) return kSparseBadCounts;
    if (k < 1 || k > kSparseMaxK) return kSparseBadK;
    if (mem != 0 && mem != 1) return kSparseBadMem;
    if (n_queries > 0 && (!has_indptr || !has_scores || !has_indices)) return kSparseNullPointer;
    if (n_queries > 0 && q_nnz > 0 && (!has_terms || !has_weights)) return kSparseNullPointer;
    if (!column) return kSparseNoColumn;
    return kSparseOk;
}
inline int hybrid_validate_call(int64_t n_queries, int64_t q_nnz, int k, int fetch_k, double w_dense, double w_sparse,
                                double rrf_c, bool has_queries, bool has_indptr, bool has_terms, bool has_weights,
                                bool has_scores, bool has_indices, int mem, bool column) {
    if (n_queries < 0 || q_nnz < 0) return kSparseBadCounts;
    if (k < 1 || k > kFuseMaxK) return kSparseBadK;
    if (fetch_k < k || fetch_k > kFuseMaxFetch) return kHybridBadFetch;
    if (!fuse_weight_ok(w_dense) || !fuse_weight_ok(w_sparse)) return kHybridBadWeight;
    if (!fuse_weight_ok(rrf_c)) return kHybridBadC;
    if (n_queries > 0 && !has_queries) return kSparseNullPointer;
    return sparse_validate_call(n_queries, q_nnz, fetch_k, has_indptr, has_terms, has_weights, has_scores, has_indices, mem,
                                column);
}
// A host-memory call's queries.  *at: the offending offset index / entry.
inline int sparse_validate_queries(const int64_t* q_indptr, const int32_t* q_terms, const float* q_weights,
                                   int64_t n_queries, int64_t q_nnz, int32_t n_terms, int64_t* at) {
    *at = 0;
    for (int64_t b = 0; b <= n_queries && n_queries > 0; ++b) {
        const int64_t o = q_indptr[b];
        if (o < 0 || o > q_nnz || (b > 0 && o < q_indptr[b - 1])) {
            *at = b;
            return kSparseBadOffsets;
        }
        if (b > 0 && o - q_indptr[b - 1] > kSparseMaxQueryTerms) {
            *at = b - 1;
            return kSparseTooLong;
        }
    }
    for (int64_t b = 0; b < n_queries; ++b) {
        int32_t prev = -1;
        for (int64_t e = q_indptr[b]; e < q_indptr[b + 1]; ++e) {
            *at = e;
            const int32_t t = q_terms[e];
            if (t < 0 || t >= n_terms) return kSparseBadTerm;
            if (t <= prev) return kSparseUnsorted;
            if (!sparse_weight_ok(q_weights[e])) return kSparseNonFinite;
            prev = t;
        }
    }
    *at = 0;
    return kSparseOk;
}
// Whether the kernel answers a query with "no result" in every slot and counts it: its range is bad
// or one of its entries is.
inline bool sparse_query_bad(const int64_t* q_indptr, const int32_t* q_terms, const float* q_weights, int64_t b,
                             int64_t q_nnz, int32_t n_terms) {
    const SparseQRange r = sparse_query_range(q_indptr[b], q_indptr[b + 1], q_nnz);
    if (r.bad) return true;
    int32_t prev = -1;
    for (int e = 0; e < r.len; ++e) {
        const int32_t t = q_terms[r.o0 + e];
        if (!sparse_term_ok(t, prev, n_terms) || !sparse_weight_ok(q_weights[r.o0 + e])) return true;
        prev = t;
    }
    return false;
}

}  // namespace vdb
