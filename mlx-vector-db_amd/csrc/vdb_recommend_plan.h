// vdb_recommend_plan.h — the host arithmetic of vdb_index_search_recommend (vdb_api.cpp) and the
// decisions its kernels share with it (vdb_recommend.hip): the limits and the argument validation,
// the clamp of a device-memory call's offsets, the state of a query's example lists, the
// per-element step of the built query (term, combine, finite test), the membership test and the
// in-order compaction of the select, the inner fetch size and the per-call scratch.  Plain C++ with
// no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/recommend_plan_check.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_REC_HD __host__ __device__
#else
#define VDB_REC_HD
#endif

namespace vdb {

constexpr int kRecMaxExamples = 64;  // positives and negatives of one query together
constexpr int kRecMaxFetch = 200;    // the most the certified fast path returns (kMaxApproxK)
constexpr int kRecMaxK = kRecMaxFetch - kRecMaxExamples;  // 136: k + examples never leaves the fast path
// The build kernel: one workgroup per query, thread t owns dims t, t + kRecBuildThreads, ...
constexpr int kRecBuildThreads = 256;
// The select kernel: one wave per query, kRecSelectWaves waves per workgroup; lane l holds fetched
// positions l, l + 64, ...
constexpr int kRecSelectWaves = 4;
constexpr int kRecLanePos = (kRecMaxFetch + 63) / 64;

// ---- a query's lists ------------------------------------------------------------------------------
// Offsets as a device-memory call may hold them, clamped into [0, n] and made to ascend: nothing
// outside the id array is read whatever they are.
struct RecRange {
    int64_t o0, o1;
};
VDB_REC_HD inline RecRange rec_range(int64_t off_lo, int64_t off_hi, int64_t n) {
    RecRange r;
    r.o0 = off_lo < 0 ? 0 : off_lo > n ? n : off_lo;
    r.o1 = off_hi < r.o0 ? r.o0 : off_hi > n ? n : off_hi;
    return r;
}
// What the list lengths alone say of a query (np positives, nn negatives, after the clamp):
// kRecListEmpty = no positive example, every slot "no result", not an error and not counted;
// kRecListBad = more than kRecMaxExamples examples (device-memory calls: counted in
// "recommend_bad_queries").  The empty test comes first.
enum { kRecListOk = 0, kRecListEmpty = 1, kRecListBad = 2 };
VDB_REC_HD inline int rec_list_state(int64_t np, int64_t nn) {
    if (np <= 0) return kRecListEmpty;
    if (np > kRecMaxExamples || nn > kRecMaxExamples || np + nn > kRecMaxExamples) return kRecListBad;
    return kRecListOk;
}
VDB_REC_HD inline bool rec_id_ok(int64_t id, int64_t count) { return id >= 0 && id < count; }

// ---- the built query, one element -----------------------------------------------------------------
// All fp64, every operation apart (the library is built without contraction): acc = acc + term over
// a list in list order, mp = acc / (double)n, then rec_combine.  The cosine term is one fp64 divide
// per element by the row's canonical norm under the clamp a key uses.
VDB_REC_HD inline double rec_term(float x, double norm, int metric) {
    return metric == 0 ? (double)x / (norm > 1e-8 ? norm : 1e-8) : (double)x;
}
VDB_REC_HD inline double rec_mean(double acc, int64_t n) { return acc / (double)n; }
// Qdrant's average-vector rule, rounded to fp32 to nearest even (beyond fp32's range: +-inf).
VDB_REC_HD inline float rec_combine(double mp, double mn, bool has_neg) {
    double t = mp;
    if (has_neg) {
        const double two = mp + mp;
        t = two - mn;
    }
    return (float)t;
}
VDB_REC_HD inline bool rec_finite(float q) { return (q < 0.0f ? -q : q) <= 3.40282346638528859812e+38f; }

// ---- the select -----------------------------------------------------------------------------------
// Row `id` stands in the query's examples (pos[0 .. np), neg[0 .. nn)).
VDB_REC_HD inline bool rec_is_example(int64_t id, const int64_t* pos, int np, const int64_t* neg, int nn) {
    for (int e = 0; e < np; ++e)
        if (pos[e] == id) return true;
    for (int e = 0; e < nn; ++e)
        if (neg[e] == id) return true;
    return false;
}
// A fetched entry is kept when it names a row that is no example.
VDB_REC_HD inline bool rec_keep(int64_t id, int64_t count, const int64_t* pos, int np, const int64_t* neg, int nn) {
    return rec_id_ok(id, count) && !rec_is_example(id, pos, np, neg, nn);
}
// The compaction over plain arrays: the fetched list fi[0 .. F) in order, the first k kept
// positions to out_pos; returns their number (at most k).
inline int rec_compact(const int64_t* fi, int F, int k, int64_t count, const int64_t* pos, int np, const int64_t* neg,
                       int nn, int* out_pos) {
    int m = 0;
    for (int p = 0; p < F && m < k; ++p)
        if (rec_keep(fi[p], count, pos, np, neg, nn)) out_pos[m++] = p;
    return m;
}

// ---- the inner fetch ------------------------------------------------------------------------------
// k' = k + E rows per query: a query's examples can take at most that many of its best rows.  Host
// memory: E = the largest example count of any query (the lists are read anyway); device memory: E =
// min(kRecMaxExamples, n_pos + n_neg), from the host scalars alone.  The result is the same for
// every k' >= k + (the query's examples); only the cost moves.
inline int rec_fetch_examples_device(int64_t n_pos, int64_t n_neg) {
    const int64_t e = (n_pos > 0 ? n_pos : 0) + (n_neg > 0 ? n_neg : 0);
    return (int)(e < kRecMaxExamples ? e : kRecMaxExamples);
}
inline int rec_fetch_k(int k, int examples) { return k + examples; }

// ---- scratch --------------------------------------------------------------------------------------
inline int64_t rec_align(int64_t b) { return (b + 255) / 256 * 256; }
struct RecScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t q, flag, fs, fi, fk;
    // host-memory calls: the staged arguments (one upload) and the results (one download; the built
    // queries lie in it when the caller asks for them)
    int64_t in0, pos_offs, pos_rows, neg_offs, neg_rows, mask, in_bytes, out0, out_s, out_i, out_k, out_bytes;
    int64_t mask_words, total;
};
inline RecScratch rec_scratch(int n_queries, int dim, int k, int fetch_k, int64_t rows, int64_t n_pos, int64_t n_neg,
                              bool host, bool has_neg, bool masked, bool keys, bool queries) {
    RecScratch s{};
    const int64_t B = n_queries, F = fetch_k;
    s.mask_words = (rows + 31) / 32;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += rec_align(bytes);
        return at;
    };
    const bool q_down = host && queries;
    if (!q_down) s.q = take(B * dim * 4);
    s.flag = take(B * 4);
    s.fs = take(B * F * 4);
    s.fi = take(B * F * 8);
    s.fk = take(B * F * 8);
    s.in0 = o;
    if (host) {
        s.pos_offs = take((B + 1) * 8);
        s.pos_rows = take(n_pos * 8);
        s.neg_offs = take(has_neg ? (B + 1) * 8 : 0);
        s.neg_rows = take(has_neg ? n_neg * 8 : 0);
        // (+ 64 zero words, as a host search's staged mask: the candidate passes read whole mask tiles)
        s.mask = take(masked ? (s.mask_words + 64) * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_s = take(B * k * 4);
        s.out_i = take(B * k * 8);
        s.out_k = take(keys ? B * k * 8 : 0);
        if (q_down) s.q = take(B * dim * 4);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -----------------------------------------------------------------------------------
enum {
    kRecOk = 0,
    kRecBadQueries = 1,   // n_queries < 0
    kRecBadK = 2,         // k outside [1, kRecMaxK]
    kRecNullPointer = 3,  // pos_offsets, an id array with entries, or a required output missing
    kRecBadMem = 4,       // a memory kind that is neither host (0) nor device (1)
    kRecBadCounts = 5,    // n_pos or n_neg < 0, or negatives without neg_offsets
    kRecBadOffsets = 6,   // offsets that decrease, start below 0 or pass their n
    kRecBadId = 7,        // an id outside [0, count)
    kRecTooMany = 8       // a query with more than kRecMaxExamples examples
};
// The scalars and pointers (both memory kinds).  The has_* of a call without queries are not looked at.
inline int rec_validate(int n_queries, int k, int64_t n_pos, int64_t n_neg, bool has_pos_offs, bool has_pos_rows,
                        bool has_neg_offs, bool has_neg_rows, bool has_scores, bool has_indices, int mem) {
    if (n_queries < 0) return kRecBadQueries;
    if (k < 1 || k > kRecMaxK) return kRecBadK;
    if (mem != 0 && mem != 1) return kRecBadMem;
    if (n_pos < 0 || n_neg < 0) return kRecBadCounts;
    if (!has_neg_offs && n_neg != 0) return kRecBadCounts;
    if (n_queries == 0) return kRecOk;
    if (!has_pos_offs || !has_scores || !has_indices) return kRecNullPointer;
    if ((n_pos > 0 && !has_pos_rows) || (has_neg_offs && n_neg > 0 && !has_neg_rows)) return kRecNullPointer;
    return kRecOk;
}
// One CSR pair of a host-memory call: offs[0 .. B] ascend from >= 0 to <= n, every id names a row.
// *where = the offending offset or id position.
inline int rec_validate_csr(const int64_t* offs, const int64_t* rows, int64_t n, int n_queries, int64_t count,
                            int64_t* where) {
    int64_t prev = 0;
    for (int b = 0; b <= n_queries; ++b) {
        if (offs[b] < prev || offs[b] > n) {
            *where = b;
            return kRecBadOffsets;
        }
        prev = offs[b];
    }
    for (int64_t i = offs[0]; i < offs[n_queries]; ++i)
        if (!rec_id_ok(rows[i], count)) {
            *where = i;
            return kRecBadId;
        }
    return kRecOk;
}
// Both pairs of a host-memory call (neg_offs may be NULL: no negatives), then the example counts;
// *max_examples = the largest count of any query.  *which = 0 / 1: the positives / negatives failed.
inline int rec_validate_lists(const int64_t* pos_offs, const int64_t* pos_rows, int64_t n_pos, const int64_t* neg_offs,
                              const int64_t* neg_rows, int64_t n_neg, int n_queries, int64_t count, int64_t* where,
                              int* which, int* max_examples) {
    int64_t w = 0;
    int dummy_which = 0, dummy_max = 0;
    if (!where) where = &w;
    if (!which) which = &dummy_which;
    if (!max_examples) max_examples = &dummy_max;
    *where = 0;
    *which = 0;
    *max_examples = 0;
    int rc = rec_validate_csr(pos_offs, pos_rows, n_pos, n_queries, count, where);
    if (rc) return rc;
    if (neg_offs) {
        *which = 1;
        rc = rec_validate_csr(neg_offs, neg_rows, n_neg, n_queries, count, where);
        if (rc) return rc;
    }
    *which = 0;
    for (int b = 0; b < n_queries; ++b) {
        const int64_t np = pos_offs[b + 1] - pos_offs[b];
        const int64_t nn = neg_offs ? neg_offs[b + 1] - neg_offs[b] : 0;
        if (np > kRecMaxExamples || nn > kRecMaxExamples || np + nn > kRecMaxExamples) {
            *where = b;
            return kRecTooMany;
        }
        if (np + nn > *max_examples) *max_examples = (int)(np + nn);
    }
    return kRecOk;
}

}  // namespace vdb
