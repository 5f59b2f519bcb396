// vdb_group_plan.h — the host arithmetic of vdb_index_search_groups (vdb_api.cpp) and the decisions
// its kernels share with it (vdb_group.hip): how many rows the inner search fetches, which entries
// of a ranked list are the first of their group and when such a list settles a query, how the exact
// fallback's rows are dealt to workgroups, the per-call scratch, and the argument validation.
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/group_plan_check.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_GROUP_HD __host__ __device__
#else
#define VDB_GROUP_HD
#endif

namespace vdb {

constexpr int kGroupMaxK = 128;      // groups a query can ask for
constexpr int kGroupMaxQueries = 65535;  // queries per call: one per grid row of the fallback's launch
constexpr int kGroupMaxFetch = 200;  // rows the inner search returns at most (its certified fast path)
// The exact fallback: a workgroup is 4 waves, a wave scores kGroupNB rows at a time; a segment is a
// contiguous row range, a multiple of kGroupSegAlign rows (whole mask words, whole wave trips).
constexpr int kGroupWaves = 4;
constexpr int kGroupNB = 4;
constexpr int kGroupSegAlign = 32;
constexpr int kGroupMaxSeg = 256;                   // most segments per query
constexpr int64_t kGroupMinSegRows = 1024;          // fewest rows worth a segment of their own
constexpr int64_t kGroupListBytes = 64ll << 20;     // bound on the segments' partial lists of one call
constexpr int64_t kGroupEntryBytes = 16;            // fp64 key + uint32 row + int32 group

// ---- the fetch rule -------------------------------------------------------------------------------
// Rows the inner search is asked for.  knob ("group_fetch") 1..200 sets it, never below k; 0 = auto:
// 1 for k = 1 (the best row's group is the best group), else 200, the most the certified fast path
// returns: measured, a query that one 64-row group fills costs a whole exact scan at
// a smaller fetch, far more than the larger fetch costs every query.  Every value gives the same
// results (only the share of queries that need the exact fallback moves).
VDB_GROUP_HD inline int group_fetch_k(int64_t knob, int k) {
    int64_t f = knob > 0 ? knob : (k <= 1 ? 1 : kGroupMaxFetch);
    if (f > kGroupMaxFetch) f = kGroupMaxFetch;
    if (f < k) f = k;
    return (int)f;
}

// ---- shared with the kernels ----------------------------------------------------------------------
// Entry j of a list ranked by (key desc, row asc) is the first of its group when it is valid (g[j] >=
// 0) and no earlier entry has its group: then it is that group's best row among the list's rows.
VDB_GROUP_HD inline bool group_first_occurrence(const int32_t* g, int j) {
    const int32_t gj = g[j];
    if (gj < 0) return false;
    for (int i = 0; i < j; ++i)
        if (g[i] == gj) return false;
    return true;
}
// A fetched list (the true best k_fetch eligible rows, n_valid of its slots filled, n_first distinct
// groups among them) settles the query when it holds k groups, or when every eligible row was seen:
// the list is short, or the call's `eligible` rows (those with a group and their mask bit) are no
// more than were fetched.
VDB_GROUP_HD inline bool group_complete(int n_first, int n_valid, int k, int k_fetch, int64_t eligible) {
    return n_first >= k || n_valid < k_fetch || eligible <= (int64_t)k_fetch;
}

// Segments per query of the exact fallback: about kGroupMinSegRows rows each, at most kGroupMaxSeg,
// and few enough for the partial lists [n_queries][n_seg][k] to stay inside kGroupListBytes.
inline int group_n_seg(int64_t rows, int n_queries, int k) {
    int64_t s = (rows + kGroupMinSegRows - 1) / kGroupMinSegRows;
    if (s > kGroupMaxSeg) s = kGroupMaxSeg;
    const int64_t per_seg = (int64_t)(n_queries > 0 ? n_queries : 1) * (k > 0 ? k : 1) * kGroupEntryBytes;
    const int64_t fit = kGroupListBytes / per_seg;
    if (s > fit) s = fit;
    return s < 1 ? 1 : (int)s;
}
// Rows per segment (a multiple of kGroupSegAlign) and segment s's range [r0, r1) of [0, rows).
VDB_GROUP_HD inline int64_t group_seg_rows(int64_t rows, int n_seg) {
    const int64_t per = (rows + n_seg - 1) / n_seg;
    return (per + kGroupSegAlign - 1) / kGroupSegAlign * kGroupSegAlign;
}
struct GroupRange {
    int64_t r0, r1;
};
VDB_GROUP_HD inline GroupRange group_seg_range(int64_t rows, int n_seg, int s) {
    const int64_t per = group_seg_rows(rows, n_seg);
    GroupRange r;
    r.r0 = (int64_t)s * per;
    if (r.r0 > rows) r.r0 = rows;
    r.r1 = r.r0 + per;
    if (r.r1 > rows) r.r1 = rows;
    return r;
}
// Segments that hold any row: the ones the per-query counter waits for.
VDB_GROUP_HD inline int group_live_segs(int64_t rows, int n_seg) {
    const int64_t per = group_seg_rows(rows, n_seg);
    const int64_t live = per > 0 ? (rows + per - 1) / per : 0;
    return live < n_seg ? (int)live : n_seg;
}
// Entries of a GroupTopK buffer for k groups: a power of two >= max(2 k, k + 64).
VDB_GROUP_HD inline int group_topk_cap(int k) {
    const int need = 2 * k > k + 64 ? 2 * k : k + 64;
    int p = 1;
    while (p < need) p <<= 1;
    return p;
}

// ---- scratch --------------------------------------------------------------------------------------
inline int64_t group_align(int64_t b) { return (b + 255) / 256 * 256; }
struct GroupScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t qn64, done, need, elig, fmask, fs, fi, fk, lk, lr, lg;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, mask, in_bytes, out0, out_s, out_i, out_g, out_k, out_bytes;
    int64_t mask_words, total;
};
inline GroupScratch group_scratch(int n_queries, int dim, int k, int k_fetch, int n_seg, int64_t rows, bool host,
                                  bool masked, bool keys) {
    GroupScratch s{};
    const int64_t B = n_queries;
    s.mask_words = (rows + 31) / 32;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += group_align(bytes);
        return at;
    };
    s.qn64 = take(B * 8);
    s.done = take(B * 4);
    s.need = take(B * 4);
    s.elig = take(8);  // the eligible rows of a masked call, counted by the AND kernel
    // the caller's mask AND the rows with a group (+ 64 words, as a host search's staged mask)
    s.fmask = take(masked ? (s.mask_words + 64) * 4 : 0);
    s.fs = take(B * k_fetch * 4);
    s.fi = take(B * k_fetch * 8);
    s.fk = take(B * k_fetch * 8);
    s.lk = take(n_seg > 1 ? B * n_seg * k * 8 : 0);
    s.lr = take(n_seg > 1 ? B * n_seg * k * 4 : 0);
    s.lg = take(n_seg > 1 ? B * n_seg * k * 4 : 0);
    s.in0 = o;
    if (host) {
        s.q = take(B * dim * 4);
        s.mask = take(masked ? s.mask_words * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_s = take(B * k * 4);
        s.out_i = take(B * k * 8);
        s.out_g = take(B * k * 4);
        s.out_k = take(keys ? B * k * 8 : 0);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -----------------------------------------------------------------------------------
enum {
    kGroupOk = 0,
    kGroupBadQueries = 1,  // n_queries < 0 or above kGroupMaxQueries
    kGroupBadK = 2,        // k outside [1, kGroupMaxK]
    kGroupNullPointer = 3, // queries or a required output missing
    kGroupBadMem = 4,      // a memory kind that is neither host (0) nor device (1)
    kGroupNoColumn = 5     // no group column attached (or its length is not the index's count)
};
inline int group_validate(int n_queries, int k, bool has_queries, bool has_scores, bool has_indices, bool has_groups,
                          int mem, bool has_column, int64_t group_rows, int64_t count) {
    if (n_queries < 0 || n_queries > kGroupMaxQueries) return kGroupBadQueries;
    if (k < 1 || k > kGroupMaxK) return kGroupBadK;
    if (!has_queries || !has_scores || !has_indices || !has_groups) return kGroupNullPointer;
    if (mem != 0 && mem != 1) return kGroupBadMem;
    if (!has_column || group_rows != count) return kGroupNoColumn;
    return kGroupOk;
}
// vdb_index_set_groups: n must be the index's count (n == 0 with no pointer detaches).
inline bool group_set_ok(bool has_groups, int64_t n, int64_t count) {
    if (!has_groups) return n == 0;
    return n == count && n >= 0;
}

}  // namespace vdb
