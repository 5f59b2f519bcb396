// vdb_maxsim_plan.h — the host arithmetic of vdb_index_search_maxsim (vdb_api.cpp) and the decisions
// its kernels share with it (vdb_maxsim.hip): the limits and the argument validation (one enum value
// per cause), the table size check, the order-preserving encoding of a maximum, the clamp of a
// device call's offsets and what makes a set bad, the deal of group slots to the rank kernel's
// segments, the per-call scratch, and the score of one set (`maxsim_select`) as a plain function
// over plain arrays.  Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a
// sanitizer (tools/maxsim_plan_check.cpp).  The deal of rows to the scan kernel's workgroups and
// waves and its query blocks are vdb_range_plan.h's.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define VDB_MAXSIM_HD __host__ __device__
#else
#define VDB_MAXSIM_HD
#endif

namespace vdb {

constexpr int kMaxsimMaxK = 128;          // groups a set can ask for (kGroupMaxK)
constexpr int kMaxsimMaxVectors = 64;     // sub-queries per set
constexpr int64_t kMaxsimMaxCells = (int64_t)1 << 27;  // n_sub x n_group_slots: a 1 GiB table
constexpr int kMaxsimThreads = 256;       // the rank kernel's workgroup, 4 waves
constexpr int kMaxsimSegSlots = 1024;     // slots a rank segment takes at least: 4 per thread
constexpr int kMaxsimMaxSeg = 256;        // segments per set at most (one merge of <= 512 lists)
constexpr int kMaxsimCallWgs = 2048;      // ... and about this many rank workgroups per call
constexpr int kMaxsimRankSets = 32768;    // sets per rank launch (the grid's second dimension)

// ---- the table ------------------------------------------------------------------------------------
// T [n_sub][n_group_slots] of uint64: the order-preserving encoding of the fp64 maximum of (sub-query,
// group), 0 = no eligible row.  u > v as unsigned integers iff the doubles compare so (with -0.0
// below +0.0, which the + 0.0 of the contract removes before encoding); -inf encodes to
// 0x000FFFFFFFFFFFFF, so 0 is below every value a key can take.
VDB_MAXSIM_HD inline uint64_t maxsim_bits(double f) {
    uint64_t b;
    memcpy(&b, &f, 8);
    return b;
}
VDB_MAXSIM_HD inline double maxsim_from_bits(uint64_t b) {
    double f;
    memcpy(&f, &b, 8);
    return f;
}
VDB_MAXSIM_HD inline uint64_t maxsim_encode(double f) {
    const uint64_t b = maxsim_bits(f);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
VDB_MAXSIM_HD inline double maxsim_decode(uint64_t u) {
    return maxsim_from_bits(u ^ ((u >> 63) ? (1ull << 63) : ~0ull));
}
// The table entry of one key: one fp64 add first, which turns -0.0 into +0.0 and changes nothing else.
VDB_MAXSIM_HD inline uint64_t maxsim_entry(double key) { return maxsim_encode(key + 0.0); }
// 1 <= n_group_slots and n_sub * n_group_slots <= kMaxsimMaxCells, tested by division so that the
// product is never formed.
VDB_MAXSIM_HD inline bool maxsim_table_ok(int64_t n_sub, int64_t n_slots) {
    if (n_slots < 1 || n_sub < 0) return false;
    return n_sub == 0 || n_slots <= kMaxsimMaxCells / n_sub;
}
// A row's slot: its group id when that lies in [0, n_slots), else -1 (a row without a usable group).
VDB_MAXSIM_HD inline int32_t maxsim_slot(int32_t group, int32_t n_slots) {
    return (group >= 0 && group < n_slots) ? group : -1;
}

// ---- the sets of a call ---------------------------------------------------------------------------
// Set s is sub-queries [offsets[s], offsets[s + 1]).  A device-memory call is not validated: the
// range is clamped to [0, n_sub] so that nothing out of bounds is read, and the set is bad (every
// slot "no result", counted in "maxsim_bad_sets") when the clamp changed an offset, the offsets
// decrease or it has more than kMaxsimMaxVectors sub-queries.  m is the number of sub-queries
// summed: 0 for a bad set.
struct MaxsimRange {
    int64_t o0;
    int m;
    bool bad;
};
VDB_MAXSIM_HD inline MaxsimRange maxsim_range(int64_t off_lo, int64_t off_hi, int64_t n_sub) {
    MaxsimRange r;
    r.o0 = off_lo < 0 ? 0 : off_lo > n_sub ? n_sub : off_lo;
    const int64_t o1 = off_hi < r.o0 ? r.o0 : off_hi > n_sub ? n_sub : off_hi;
    r.bad = off_lo < 0 || off_lo > n_sub || off_hi > n_sub || off_hi < off_lo || o1 - r.o0 > kMaxsimMaxVectors;
    r.m = r.bad ? 0 : (int)(o1 - r.o0);
    return r;
}

// ---- the rank kernel's deal -----------------------------------------------------------------------
// The top-k buffers hold KE = the power of two at or above k entries.
VDB_MAXSIM_HD inline int maxsim_ke(int k) {
    int p = 1;
    while (p < k) p <<= 1;
    return p;
}
// Segments per set: one per kMaxsimSegSlots slots, at most kMaxsimMaxSeg, and fewer when the call
// has so many sets that they fill the device by themselves.
VDB_MAXSIM_HD inline int maxsim_n_seg(int64_t n_slots, int64_t n_sets) {
    int64_t g = (n_slots + kMaxsimSegSlots - 1) / kMaxsimSegSlots;
    const int64_t per_call = kMaxsimCallWgs / (n_sets > 0 ? n_sets : 1);
    if (g > per_call) g = per_call;
    if (g > kMaxsimMaxSeg) g = kMaxsimMaxSeg;
    return g < 1 ? 1 : (int)g;
}
// Trip i of wave `wave` of segment `seg` starts at this slot and its lane j takes the slot j after
// it: consecutive lanes read consecutive table entries.  The caller stops at the first start at or
// past n_slots.
VDB_MAXSIM_HD inline int64_t maxsim_trip_slot(int seg, int n_seg, int wave, int64_t i) {
    return ((i * n_seg + seg) * (kMaxsimThreads / 64) + wave) * 64;
}

// ---- the score of one set -------------------------------------------------------------------------
// One candidate's sum: acc = 0.0, then the set's entries of slot g added in sub-query order, each a
// separate fp64 add.  col points at T[o0][g]; consecutive sub-queries are n_slots entries apart.
VDB_MAXSIM_HD inline double maxsim_sum(const uint64_t* col, int m, int64_t n_slots) {
    double acc = 0.0;
    for (int t = 0; t < m; ++t) acc = acc + maxsim_decode(col[(int64_t)t * n_slots]);
    return acc;
}
// The whole ranking of one set over a plain table: sub-queries [o0, o0 + m), slots [0, n_slots).
// Writes the first min(k, candidates) by (sum desc, slot asc) and returns their number.  O(slots x k),
// for checking.
inline int maxsim_select(const uint64_t* T, int64_t n_slots, int64_t o0, int m, int k, int32_t* out_group,
                         double* out_sum) {
    int n = 0;
    if (m <= 0) return 0;
    for (int64_t g = 0; g < n_slots; ++g) {
        const uint64_t* col = T + o0 * n_slots + g;
        if (col[0] == 0) continue;
        const double sum = maxsim_sum(col, m, n_slots);
        int at = n < k ? n : k;
        while (at > 0 && sum > out_sum[at - 1]) --at;  // (slots ascend: an equal sum stays behind)
        if (at >= k) continue;
        const int last = n < k ? n : k - 1;
        for (int s = last; s > at; --s) {
            out_group[s] = out_group[s - 1];
            out_sum[s] = out_sum[s - 1];
        }
        out_group[at] = (int32_t)g;
        out_sum[at] = sum;
        if (n < k) ++n;
    }
    return n;
}

// ---- scratch --------------------------------------------------------------------------------------
inline int64_t maxsim_align(int64_t b) { return (b + 255) / 256 * 256; }
struct MaxsimScratch {
    int block;  // sub-queries per scan block (range_query_block of the padded row length)
    int n_seg, KE;
    // byte offsets into the workspace (each 256-byte aligned): the sub-queries' norms; the table and,
    // right behind it, the per-set counters of the rank kernel (zeroed together: zero_bytes from T);
    // the segments' lists lk / li [n_sets][n_seg][KE] and the merged mk / mi [n_sets][KE]
    int64_t qn64, T, done, zero_bytes, lk, li, mk, mi;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, offs, mask, in_bytes, out0, out_s, out_g, out_sum, out_bytes;
    int64_t mask_words, total;
};
inline MaxsimScratch maxsim_scratch(int64_t n_sub, int64_t n_sets, int64_t n_slots, int dim, int block, int k,
                                    int64_t rows, bool host, bool masked, bool sums) {
    MaxsimScratch s{};
    s.block = block < 1 ? 1 : block;
    s.KE = maxsim_ke(k);
    s.n_seg = maxsim_n_seg(n_slots, n_sets);
    s.mask_words = (rows + 31) / 32;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += maxsim_align(bytes);
        return at;
    };
    s.qn64 = take(n_sub * 8);
    s.T = take(n_sub * n_slots * 8);
    s.done = take(n_sets * 4);
    s.zero_bytes = o - s.T;
    const int64_t lists = s.n_seg > 1 ? n_sets * s.n_seg * s.KE : 0;
    s.lk = take(lists * 8);
    s.li = take(lists * 4);
    s.mk = take(s.n_seg > 1 ? n_sets * s.KE * 8 : 0);
    s.mi = take(s.n_seg > 1 ? n_sets * s.KE * 4 : 0);
    s.in0 = o;
    if (host) {
        s.q = take(n_sub * dim * 4);
        s.offs = take((n_sets + 1) * 8);
        s.mask = take(masked ? s.mask_words * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_s = take(n_sets * k * 4);
        s.out_g = take(n_sets * k * 4);
        s.out_sum = take(sums ? n_sets * k * 8 : 0);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -----------------------------------------------------------------------------------
enum {
    kMaxsimOk = 0,
    kMaxsimBadCounts = 1,    // n_sub or n_sets < 0
    kMaxsimBadK = 2,         // k outside [1, kMaxsimMaxK]
    kMaxsimBadSlots = 3,     // n_group_slots < 1, or n_sub * n_group_slots above kMaxsimMaxCells
    kMaxsimNullPointer = 4,  // queries with n_sub > 0, or set_offsets / out_scores / out_groups with n_sets > 0
    kMaxsimBadMem = 5        // a memory kind that is neither host (0) nor device (1)
};
// What the scalars and the pointers' presence say, for both memory kinds.
inline int maxsim_validate(int64_t n_sub, int64_t n_sets, int64_t n_slots, int k, bool has_queries, bool has_offsets,
                           bool has_scores, bool has_groups, int mem) {
    if (n_sub < 0 || n_sets < 0) return kMaxsimBadCounts;
    if (k < 1 || k > kMaxsimMaxK) return kMaxsimBadK;
    if (!maxsim_table_ok(n_sub, n_slots) || n_slots > 0x7FFFFFFF) return kMaxsimBadSlots;
    if (mem != 0 && mem != 1) return kMaxsimBadMem;
    if (n_sub > 0 && !has_queries) return kMaxsimNullPointer;
    if (n_sets > 0 && (!has_offsets || !has_scores || !has_groups)) return kMaxsimNullPointer;
    return kMaxsimOk;
}
// A host-memory call's offsets.  *at: the offending offset index / set.
enum { kMaxsimSetsOk = 0, kMaxsimBadOffsets = 1, kMaxsimSetTooLong = 2 };
inline int maxsim_validate_sets(const int64_t* offsets, int64_t n_sets, int64_t n_sub, int64_t* at) {
    for (int64_t s = 0; s <= n_sets && n_sets > 0; ++s) {
        const int64_t o = offsets[s];
        if (o < 0 || o > n_sub || (s > 0 && o < offsets[s - 1])) {
            *at = s;
            return kMaxsimBadOffsets;
        }
        if (s > 0 && o - offsets[s - 1] > kMaxsimMaxVectors) {
            *at = s - 1;
            return kMaxsimSetTooLong;
        }
    }
    return kMaxsimSetsOk;
}

}  // namespace vdb
