// vdb_subset_plan.h — the host arithmetic of vdb_index_search_rows (vdb_api.cpp) and the index
// arithmetic its kernel shares with it (vdb_subset.hip): how a query's row-id list is cut into
// chunks and dealt to workgroups, the per-call scratch, and the validation of the CSR arguments.
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/subset_plan_check.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_SUBSET_HD __host__ __device__
#else
#define VDB_SUBSET_HD
#endif

namespace vdb {

// A workgroup is 4 waves; a wave scores kSubsetNB rows at a time (their pieces in flight together)
// and reads the ids of kSubsetWaveRows consecutive list positions with one load.  A chunk is the
// positions one workgroup handles per trip: wave w takes [16 w, 16 w + 16) of it.
constexpr int kSubsetWaves = 4;
constexpr int kSubsetNB = 4;
constexpr int kSubsetWaveRows = 16;
constexpr int kSubsetChunk = kSubsetWaves * kSubsetWaveRows;  // 64 list positions
// Most workgroups per query: the tail merge selects over at most this many list heads
// (vdb_merge_block.h MERGE_HEADS) before it falls back to streaming every entry.
constexpr int kSubsetMaxSeg = 512;
// Workgroups the grid aims for per CU (short rows, small k: several fit a CU and hide each other's
// gather latency).
constexpr int kSubsetWgPerCu = 4;

// fp64 keys + uint32 rows of one top-k entry
constexpr int64_t kSubsetEntryBytes = 12;

inline int subset_ke(int k) {  // the top-k width: max(32, next_pow2(k)), as the exact scan's
    int p = 32;
    while (p < k) p <<= 1;
    return p;
}

// Workgroups per query.  knob ("subset_wgs") > 0 forces it; 0 = auto: one per chunk of the average
// list (n_ids over the lists or queries, whichever are fewer), capped so that the grid is about
// kSubsetWgPerCu workgroups per CU.
inline int subset_n_seg(int64_t knob, int64_t n_ids, int n_queries, int n_lists, int n_cu) {
    if (knob > 0) return (int)(knob < kSubsetMaxSeg ? knob : kSubsetMaxSeg);
    const int64_t users = n_lists < n_queries ? (n_lists > 0 ? n_lists : 1) : (n_queries > 0 ? n_queries : 1);
    const int64_t avg = n_ids / users;
    int64_t chunks = (avg + kSubsetChunk - 1) / kSubsetChunk;
    int64_t cap = ((int64_t)n_cu * kSubsetWgPerCu) / (n_queries > 0 ? n_queries : 1);
    if (cap < 1) cap = 1;
    if (chunks > cap) chunks = cap;
    if (chunks > kSubsetMaxSeg) chunks = kSubsetMaxSeg;
    return chunks < 1 ? 1 : (int)chunks;
}

// ---- shared with the kernel ---------------------------------------------------------------------
// List l's positions in list_rows, with the offsets clamped so that nothing outside [0, n_ids) is
// ever addressed: [o0, o1), o0 <= o1 (a decreasing or negative pair gives an empty range).
struct SubsetRange {
    int64_t o0, o1;
};
VDB_SUBSET_HD inline SubsetRange subset_range(int64_t off_lo, int64_t off_hi, int64_t n_ids) {
    SubsetRange r;
    r.o0 = off_lo < 0 ? 0 : off_lo > n_ids ? n_ids : off_lo;
    r.o1 = off_hi < r.o0 ? r.o0 : off_hi > n_ids ? n_ids : off_hi;
    return r;
}
// Chunks of a list of `len` positions, and the workgroups of a query that have any: segment s
// walks chunks s, s + n_seg, ..., so segments at or past the chunk count have nothing to do.
VDB_SUBSET_HD inline int64_t subset_n_chunks(int64_t len) { return (len + kSubsetChunk - 1) / kSubsetChunk; }
VDB_SUBSET_HD inline int subset_live_segs(int64_t len, int n_seg) {
    const int64_t c = subset_n_chunks(len);
    return c < n_seg ? (int)c : n_seg;
}
// An id is eligible when it names a row and is greater than the entry before it in its list
// (prev = -1 for the first): a strictly ascending list of rows passes whole.
VDB_SUBSET_HD inline bool subset_id_ok(int64_t id, int64_t prev, int64_t count) {
    return id >= 0 && id < count && id > prev;
}

// ---- scratch ------------------------------------------------------------------------------------
inline int64_t subset_align(int64_t b) { return (b + 255) / 256 * 256; }
struct SubsetScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t qn64, done, lk, li, mk, mi;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, offs, rows, qlist, in_bytes, out0, out_s, out_i, out_k, out_bytes;
    int64_t total;
};
inline SubsetScratch subset_scratch(int n_queries, int dim, int k, int n_seg, int n_lists, int64_t n_ids, bool host,
                                    bool has_qlist, bool keys) {
    SubsetScratch s{};
    const int64_t B = n_queries, KE = subset_ke(k);
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += subset_align(bytes);
        return at;
    };
    s.qn64 = take(B * 8);
    s.done = take(B * 4);
    s.lk = take(n_seg > 1 ? B * n_seg * KE * 8 : 0);
    s.li = take(n_seg > 1 ? B * n_seg * KE * 4 : 0);
    s.mk = take(n_seg > 1 ? B * KE * 8 : 0);
    s.mi = take(n_seg > 1 ? B * KE * 4 : 0);
    s.in0 = o;
    if (host) {
        s.q = take(B * dim * 4);
        s.offs = take(((int64_t)n_lists + 1) * 8);
        s.rows = take(n_ids * 8);
        s.qlist = take(has_qlist ? B * 4 : 0);
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

// ---- validation of a host-memory call -----------------------------------------------------------
enum {
    kSubsetOk = 0,
    kSubsetBadOffsets = 1,    // offsets negative, decreasing or past n_ids
    kSubsetBadId = 2,         // an id outside [0, count)
    kSubsetUnsorted = 3,      // a list that is not strictly ascending
    kSubsetBadQueryList = 4,  // a query_list entry outside [0, n_lists)
    kSubsetBadCounts = 5      // no query_list and n_lists != n_queries
};
// *where: the offending offset index / position in list_rows / query.
inline int subset_validate(const int64_t* offs, int n_lists, const int64_t* rows, int64_t n_ids, const int32_t* qlist,
                           int n_queries, int64_t count, int64_t* where) {
    int64_t dummy;
    if (!where) where = &dummy;
    *where = 0;
    if (!qlist && n_lists != n_queries) return kSubsetBadCounts;
    int64_t prev = 0;
    for (int l = 0; l <= n_lists; ++l) {
        if (offs[l] < prev || offs[l] > n_ids) {
            *where = l;
            return kSubsetBadOffsets;
        }
        prev = offs[l];
    }
    for (int l = 0; l < n_lists; ++l) {
        int64_t last = -1;
        for (int64_t p = offs[l]; p < offs[l + 1]; ++p) {
            const int64_t id = rows[p];
            *where = p;
            if (id < 0 || id >= count) return kSubsetBadId;
            if (id <= last) return kSubsetUnsorted;
            last = id;
        }
    }
    if (qlist)
        for (int b = 0; b < n_queries; ++b)
            if (qlist[b] < 0 || qlist[b] >= n_lists) {
                *where = b;
                return kSubsetBadQueryList;
            }
    *where = 0;
    return kSubsetOk;
}

}  // namespace vdb
