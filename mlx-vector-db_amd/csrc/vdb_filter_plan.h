// vdb_filter_plan.h — the host arithmetic of vdb_index_set_column / vdb_index_filter_mask
// (vdb_api.cpp) and what their kernel shares with it (vdb_filter.hip): the clause test itself, the
// validation of a call with its causes, the mask width, the deal of word pairs to waves and
// workgroups, the last-word rule and the layout of the staged arguments and of a host-memory call's
// scratch.  Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/filter_plan_check.cpp).  There is no arithmetic on the values: only IEEE fp64 compares.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_FILTER_HD __host__ __device__
#else
#define VDB_FILTER_HD
#endif

namespace vdb {

constexpr int kFilterSlots = 16;      // numeric columns an index holds at most (slots 0..15)
constexpr int kFilterMaxPreds = 256;  // predicates per call
constexpr int kFilterMaxClauses = 8;  // clauses per predicate
constexpr int kFilterMaxTotal = kFilterMaxPreds * kFilterMaxClauses;  // clauses per call: 2048
// flags of a clause (include/vdb.h VDB_FILTER_*)
constexpr int32_t kFilterLoIncl = 1, kFilterHiIncl = 2, kFilterNegate = 4;
constexpr int32_t kFilterAllFlags = kFilterLoIncl | kFilterHiIncl | kFilterNegate;

// The layout of include/vdb.h vdb_filter_clause (24 bytes; vdb_api.cpp asserts the two agree).
struct FilterClause {
    int32_t column;
    int32_t flags;
    double lo;
    double hi;
};

// ---- shared with the kernel ---------------------------------------------------------------------
// One clause against a row's value v (NaN = the row has no value): a row without a value fails
// every plain clause and passes every negated one.
VDB_FILTER_HD inline bool clause_passes(double v, const FilterClause& c) {
    const bool has = !(v != v);
    const bool lo_ok = (c.flags & kFilterLoIncl) ? v >= c.lo : v > c.lo;
    const bool hi_ok = (c.flags & kFilterHiIncl) ? v <= c.hi : v < c.hi;
    const bool t = has && lo_ok && hi_ok;
    return (c.flags & kFilterNegate) ? !t : t;
}

// A workgroup is 4 waves; a wave owns one pair of mask words (64 rows, a lane per row) per trip and
// the workgroups walk the pairs round robin, so the clauses a workgroup stages in LDS serve every
// trip: pair = (trip * n_wgs + wg) * 4 + wave.
constexpr int kFilterWaves = 4;
constexpr int kFilterWgRows = 64 * kFilterWaves;
// workgroups per compute unit the grid is capped at; a call of a few clauses fits them all at once,
// the largest call (filter_lds_bytes = 52 228 B of a CU's 160 KB) runs 3 at a time and the rest after
constexpr int kFilterWgsPerCu = 4;
// The workgroup's LDS: the clauses [n_clauses] (24 B each), then the per-predicate counts [n_preds]
// (8 B), then the offsets [n_preds + 1] (4 B); every part starts 8-byte aligned.
VDB_FILTER_HD inline int64_t filter_lds_counts(int n_clauses) { return (int64_t)n_clauses * 24; }
VDB_FILTER_HD inline int64_t filter_lds_offsets(int n_clauses, int n_preds) {
    return filter_lds_counts(n_clauses) + (int64_t)n_preds * 8;
}
VDB_FILTER_HD inline int64_t filter_lds_bytes(int n_clauses, int n_preds) {
    return filter_lds_offsets(n_clauses, n_preds) + (int64_t)(n_preds + 1) * 4;
}

VDB_FILTER_HD inline int64_t filter_n_words(int64_t N) { return N > 0 ? (N + 31) / 32 : 0; }
VDB_FILTER_HD inline int64_t filter_n_pairs(int64_t n_words) { return (n_words + 1) / 2; }
// Workgroups of the launch: one per 4 pairs, at most kFilterWgsPerCu per compute unit, at least 1.
VDB_FILTER_HD inline int64_t filter_n_wgs(int64_t n_pairs, int n_cu) {
    const int64_t want = (n_pairs + kFilterWaves - 1) / kFilterWaves;
    const int64_t most = (int64_t)(n_cu > 0 ? n_cu : 1) * kFilterWgsPerCu;
    return want < 1 ? 1 : want > most ? most : want;
}
VDB_FILTER_HD inline int64_t filter_trips(int64_t n_pairs, int64_t n_wgs) {
    const int64_t per = n_wgs * kFilterWaves;
    return (n_pairs + per - 1) / per;
}
VDB_FILTER_HD inline int64_t filter_wave_pair(int64_t trip, int64_t n_wgs, int64_t wg, int wave) {
    return (trip * n_wgs + wg) * kFilterWaves + wave;
}
// The last-word rule: pair p holds words 2p and 2p + 1; with an odd word count the last pair's high
// word does not exist and is never written.
VDB_FILTER_HD inline bool filter_has_high(int64_t pair, int64_t n_words) { return pair * 2 + 1 < n_words; }
// Row of lane `lane` of pair `pair`, and whether it is a stored row (a tail row is never loaded and
// its bit is 0).
VDB_FILTER_HD inline int64_t filter_lane_row(int64_t pair, int lane) { return pair * 64 + lane; }
VDB_FILTER_HD inline bool filter_row_live(int64_t row, int64_t N) { return row < N; }

// ---- validation (host memory, both memory kinds of the masks) -----------------------------------
enum {
    kFilterOk = 0,
    kFilterBadPreds = 1,     // n_preds outside [0, 256]
    kFilterNullArgs = 2,     // n_preds > 0 without pred_offsets, or clauses missing while some are named
    kFilterBadOffsets = 3,   // offsets that do not start at 0 or that decrease
    kFilterTooMany = 4,      // more than 8 clauses in a predicate
    kFilterBadSlot = 5,      // a column outside 0..15
    kFilterNotAttached = 6,  // a column with nothing attached
    kFilterBadFlags = 7,     // unknown flag bits
    kFilterNanBound = 8      // a NaN bound
};
// attached: bit s = slot s holds a column.  *where: the offending predicate (offset causes) or
// clause (clause causes).  *used: the slots the call reads (set on success).
inline int filter_validate(const FilterClause* clauses, const int32_t* pred_offsets, int32_t n_preds, uint32_t attached,
                           int64_t* where, uint32_t* used) {
    int64_t dummy;
    uint32_t dummy_u;
    if (!where) where = &dummy;
    if (!used) used = &dummy_u;
    *where = 0;
    *used = 0;
    if (n_preds < 0 || n_preds > kFilterMaxPreds) return kFilterBadPreds;
    if (n_preds == 0) return kFilterOk;
    if (!pred_offsets) return kFilterNullArgs;
    if (pred_offsets[0] != 0) return kFilterBadOffsets;
    for (int32_t p = 0; p < n_preds; ++p) {
        *where = p;
        const int64_t len = (int64_t)pred_offsets[p + 1] - (int64_t)pred_offsets[p];
        if (len < 0) return kFilterBadOffsets;
        if (len > kFilterMaxClauses) return kFilterTooMany;
    }
    const int32_t total = pred_offsets[n_preds];  // <= 2048 by the two checks above
    if (total > 0 && !clauses) {
        *where = 0;
        return kFilterNullArgs;
    }
    uint32_t u = 0;
    for (int32_t c = 0; c < total; ++c) {
        *where = c;
        const FilterClause& cl = clauses[c];
        if (cl.column < 0 || cl.column >= kFilterSlots) return kFilterBadSlot;
        if (!((attached >> cl.column) & 1u)) return kFilterNotAttached;
        if (cl.flags & ~kFilterAllFlags) return kFilterBadFlags;
        if (cl.lo != cl.lo || cl.hi != cl.hi) return kFilterNanBound;
        u |= 1u << cl.column;
    }
    *where = 0;
    *used = u;
    return kFilterOk;
}

// ---- layout -------------------------------------------------------------------------------------
inline int64_t filter_align(int64_t b) { return (b + 255) / 256 * 256; }
// The staged arguments of one call, one pinned slot and one device block of the same layout: the
// clauses, then the n_preds + 1 offsets.  kFilterStageBytes holds the largest call.
struct FilterStage {
    int64_t clauses, offsets, bytes;
};
inline FilterStage filter_stage(int32_t n_clauses, int32_t n_preds) {
    FilterStage s{};
    s.clauses = 0;
    s.offsets = filter_align((int64_t)n_clauses * (int64_t)sizeof(FilterClause));
    s.bytes = s.offsets + filter_align((int64_t)(n_preds + 1) * 4);
    return s;
}
constexpr int64_t kFilterStageBytes =
    ((int64_t)kFilterMaxTotal * 24 + 255) / 256 * 256 + ((int64_t)(kFilterMaxPreds + 1) * 4 + 255) / 256 * 256;

// The workspace of a call: the staged arguments, and for a host-memory call the base masks (one
// upload) and the results (one download).
struct FilterScratch {
    int64_t n_words;
    int64_t stage;  // kFilterStageBytes
    int64_t in0, base, in_bytes, out0, out_m, out_c, out_bytes;
    int64_t total;
};
inline FilterScratch filter_scratch(int32_t n_preds, int64_t N, bool host, bool has_base) {
    FilterScratch s{};
    s.n_words = filter_n_words(N);
    const int64_t P = n_preds > 0 ? n_preds : 0;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += filter_align(bytes);
        return at;
    };
    s.stage = take(kFilterStageBytes);
    s.in0 = o;
    if (host) s.base = take(has_base ? P * s.n_words * 4 : 0);
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_m = take(P * s.n_words * 4);
        s.out_c = take(P * 8);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// vdb_index_set_column: n must be the index's count (n == 0 with no pointer detaches).
inline bool filter_column_ok(int32_t slot, bool has_values, int64_t n, int64_t count) {
    if (slot < 0 || slot >= kFilterSlots) return false;
    return has_values ? n == count : n == 0;
}

}  // namespace vdb
