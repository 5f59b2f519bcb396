// vdb_fuse_plan.h — the host arithmetic of vdb_index_search_fused (vdb_api.cpp) and the decisions its
// kernel shares with it (vdb_fuse.hip): the limits and the argument validation (one enum value per
// cause), the clamp of a device call's offsets and what makes a set bad, the two packed sort words
// and the padded sort length, the workgroup size and its LDS, the per-call scratch, and the fusion
// of one set (`fuse_select`) as a plain function over plain arrays.  Plain C++ with no HIP in it, so
// a stand-alone CPU program can sweep it under a sanitizer (tools/fuse_plan_check.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define VDB_FUSE_HD __host__ __device__
#else
#define VDB_FUSE_HD
#endif

namespace vdb {

constexpr int kFuseRrf = 0;          // VDB_FUSE_RRF
constexpr int kFuseMaxFusion = 1;    // VDB_FUSE_MAX
constexpr int kFuseMaxK = 200;       // rows a set can ask for
constexpr int kFuseMaxFetch = 200;   // entries per list: the most the certified fast path returns
constexpr int kFuseMaxLists = 16;    // sub-queries per set
constexpr int kFuseMaxEntries = kFuseMaxLists * kFuseMaxFetch;  // 3 200 list entries per set
constexpr int kFuseMaxSort = 4096;   // their padded sort length
constexpr int kFuseMinThreads = 64;
constexpr int kFuseMaxThreads = 1024;
constexpr int kFusePosPerThread = 4;  // sort positions a thread owns in the walk (registers)
constexpr uint64_t kFusePad = ~0ull;  // a sort word that names no entry / no candidate: sorts last

// ---- the sets of a call ---------------------------------------------------------------------------
// Set s is sub-queries [offsets[s], offsets[s + 1]).  A device-memory call is not validated: the
// range is clamped to [0, n_sub] so that nothing out of bounds is read, and the set is bad (every
// slot "no result", counted in "fused_bad_sets") when the clamp changed an offset, the offsets
// decrease or it has more than kFuseMaxLists sub-queries.  m is the number of lists fused: 0 for a
// bad set.
struct FuseRange {
    int64_t o0;
    int m;
    bool bad;
};
VDB_FUSE_HD inline FuseRange fuse_range(int64_t off_lo, int64_t off_hi, int64_t n_sub) {
    FuseRange r;
    r.o0 = off_lo < 0 ? 0 : off_lo > n_sub ? n_sub : off_lo;
    int64_t o1 = off_hi < r.o0 ? r.o0 : off_hi > n_sub ? n_sub : off_hi;
    r.bad = off_lo < 0 || off_lo > n_sub || off_hi > n_sub || off_hi < off_lo || o1 - r.o0 > kFuseMaxLists;
    r.m = r.bad ? 0 : (int)(o1 - r.o0);
    return r;
}
// finite and >= 0 (a NaN fails the first comparison)
VDB_FUSE_HD inline bool fuse_weight_ok(double w) { return w >= 0.0 && w <= 1.7976931348623157e308; }

// ---- the sort words -------------------------------------------------------------------------------
// First sort, ascending: entry p of list l holding row r is (r << 12) | (l << 8) | p, so the entries
// of one row end up adjacent and in list order.  p < 256, l < 16, r < 2^52.
VDB_FUSE_HD inline uint64_t fuse_pack_entry(uint64_t row, int l, int p) {
    return (row << 12) | ((uint64_t)l << 8) | (uint64_t)p;
}
VDB_FUSE_HD inline uint64_t fuse_entry_row(uint64_t w) { return w >> 12; }
VDB_FUSE_HD inline int fuse_entry_list(uint64_t w) { return (int)((w >> 8) & 15u); }
VDB_FUSE_HD inline int fuse_entry_pos(uint64_t w) { return (int)(w & 255u); }
// Second sort: a candidate is (key, pay).  key orders fused values as unsigned integers (greater
// value = greater key; both zeros share one key, as they compare equal); pay is (row << 20) | (l <<
// 16) | (p << 8) | hits with (l, p) the entry that holds the maximum (MAX; zero for RRF), so that
// among equal keys the lower pay is the lower row.  r < 2^44.
VDB_FUSE_HD inline uint64_t fuse_bits(double f) {
    uint64_t b;
    memcpy(&b, &f, 8);
    return b;
}
VDB_FUSE_HD inline double fuse_from_bits(uint64_t b) {
    double f;
    memcpy(&f, &b, 8);
    return f;
}
VDB_FUSE_HD inline uint64_t fuse_order_key(double f) {
    const uint64_t b = f == 0.0 ? 0ull : fuse_bits(f);
    return (b >> 63) ? ~b : (b | (1ull << 63));
}
// The value of a key (a zero comes back as +0.0: an RRF sum is never -0.0).
VDB_FUSE_HD inline double fuse_key_value(uint64_t key) {
    return fuse_from_bits((key >> 63) ? (key & ~(1ull << 63)) : ~key);
}
VDB_FUSE_HD inline uint64_t fuse_pack_cand(uint64_t row, int l, int p, int hits) {
    return (row << 20) | ((uint64_t)l << 16) | ((uint64_t)p << 8) | (uint64_t)hits;
}
VDB_FUSE_HD inline uint64_t fuse_cand_row(uint64_t pay) { return pay >> 20; }
VDB_FUSE_HD inline int fuse_cand_list(uint64_t pay) { return (int)((pay >> 16) & 15u); }
VDB_FUSE_HD inline int fuse_cand_pos(uint64_t pay) { return (int)((pay >> 8) & 255u); }
VDB_FUSE_HD inline int fuse_cand_hits(uint64_t pay) { return (int)(pay & 255u); }
// (fused desc, row asc); a pad (key 0, pay kFusePad) comes after every candidate
VDB_FUSE_HD inline bool fuse_cand_before(uint64_t ka, uint64_t pa, uint64_t kb, uint64_t pb) {
    return ka > kb || (ka == kb && pa < pb);
}

// ---- the sort length, the workgroup and its LDS ---------------------------------------------------
// A set of m lists sorts fuse_sort_len(m * fetch_k) words: the power of two at or above its
// entries, at least 64.  0 entries sort nothing.
VDB_FUSE_HD inline int fuse_sort_len(int entries) {
    if (entries <= 0) return 0;
    int L = 64;
    while (L < entries) L <<= 1;
    return L;
}
// The launch is sized for the largest set the call can hold, min(n_sub, 16) lists: a thread owns
// kFusePosPerThread sort positions at most.
VDB_FUSE_HD inline int fuse_call_sort_len(int64_t n_sub, int fetch_k) {
    const int m = n_sub < kFuseMaxLists ? (int)n_sub : kFuseMaxLists;
    return fuse_sort_len(m * fetch_k);
}
VDB_FUSE_HD inline int fuse_threads(int sort_len) {
    int t = sort_len / kFusePosPerThread;
    if (t < kFuseMinThreads) t = kFuseMinThreads;
    return t > kFuseMaxThreads ? kFuseMaxThreads : t;
}
// One array of sort words for the entries; the candidates' keys take its place and their payloads
// the second half: 16 bytes per position, 64 KiB for the largest set.
VDB_FUSE_HD inline int64_t fuse_lds_bytes(int sort_len) { return (int64_t)sort_len * 16; }
// Compare-exchange e of a bitonic step with this stride: the lower index of its pair.
VDB_FUSE_HD inline int fuse_pair_lo(int e, int stride) { return 2 * stride * (e / stride) + (e % stride); }
// Below 32 positions the two halves of 32 lanes would read positions 32 apart, the same LDS banks:
// the pairs of every second block of 32 positions touch their upper element first.
VDB_FUSE_HD inline int fuse_pair_first(int lo, int stride) { return (stride < 32 && ((lo >> 5) & 1)) ? lo + stride : lo; }

// ---- the fusion of one set ------------------------------------------------------------------------
// RRF, one term: every operation a separate fp64 operation.
VDB_FUSE_HD inline double fuse_rrf_add(double acc, double w, double rrf_c, int p) {
    const double t = rrf_c + (double)(p + 1);
    const double u = w / t;
    return acc + u;
}
// MAX: exactly this form (not fmax), so that the sign of a zero cannot differ from the oracle's.
VDB_FUSE_HD inline bool fuse_max_takes(double kappa, double fused) { return kappa > fused; }

// The whole fusion of one set over plain arrays: m lists of F entries each, rows[l * F + p] (-1 or
// >= count: no entry), keys[l * F + p], weights w[l] (nullptr: 1.0).  Writes the first min(k,
// candidates) candidates by (fused desc, row asc): out_row, out_fused, out_hits and out_at (the l *
// F + p of the entry that holds the maximum; MAX only, else -1); returns their number.  O(entries^2),
// for checking.
inline int fuse_select(int m, int F, int k, int fusion, double rrf_c, const int64_t* rows, const double* keys,
                       const double* w, int64_t count, int64_t* out_row, double* out_fused, int* out_hits, int* out_at) {
    int n = 0;
    const int E = m * F;
    for (int e = 0; e < E; ++e) {
        const int64_t r = rows[e];
        if (r < 0 || r >= count) continue;
        bool first = true;
        for (int e2 = 0; e2 < e && first; ++e2) first = rows[e2] != r;
        if (!first) continue;
        double fused = 0.0;
        int hits = 0, at = -1;
        for (int l = e / F; l < m; ++l)
            for (int p = 0; p < F; ++p) {
                if (rows[l * F + p] != r) continue;
                if (fusion == kFuseRrf) {
                    fused = fuse_rrf_add(fused, w ? w[l] : 1.0, rrf_c, p);
                } else if (hits == 0 || fuse_max_takes(keys[l * F + p], fused)) {
                    fused = keys[l * F + p];
                    at = l * F + p;
                }
                ++hits;
                break;  // a list holds a row once
            }
        // insert by (fused desc, row asc) among the first k
        int at_slot = n < k ? n : k;
        while (at_slot > 0 && (fused > out_fused[at_slot - 1] || (fused == out_fused[at_slot - 1] && r < out_row[at_slot - 1])))
            --at_slot;
        if (at_slot >= k) continue;
        const int last = n < k ? n : k - 1;
        for (int s = last; s > at_slot; --s) {
            out_row[s] = out_row[s - 1];
            out_fused[s] = out_fused[s - 1];
            out_hits[s] = out_hits[s - 1];
            out_at[s] = out_at[s - 1];
        }
        out_row[at_slot] = r;
        out_fused[at_slot] = fused;
        out_hits[at_slot] = hits;
        out_at[at_slot] = at;
        if (n < k) ++n;
    }
    return n;
}

// ---- scratch --------------------------------------------------------------------------------------
inline int64_t fuse_align(int64_t b) { return (b + 255) / 256 * 256; }
struct FuseScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t fs, fi, fk;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, offs, w, mask, in_bytes, out0, out_s, out_i, out_f, out_h, out_bytes;
    int64_t mask_words, total;
};
inline FuseScratch fuse_scratch(int64_t n_sub, int64_t n_sets, int dim, int k, int fetch_k, int64_t rows, bool host,
                                bool weighted, bool masked, bool fused, bool hits) {
    FuseScratch s{};
    const int64_t F = fetch_k;
    s.mask_words = (rows + 31) / 32;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += fuse_align(bytes);
        return at;
    };
    s.fs = take(n_sub * F * 4);
    s.fi = take(n_sub * F * 8);
    s.fk = take(n_sub * F * 8);
    s.in0 = o;
    if (host) {
        s.q = take(n_sub * dim * 4);
        s.offs = take((n_sets + 1) * 8);
        s.w = take(weighted ? n_sub * 8 : 0);
        // (+ 64 zero words, as a host search's staged mask: the candidate passes read whole mask tiles)
        s.mask = take(masked ? (s.mask_words + 64) * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_s = take(n_sets * k * 4);
        s.out_i = take(n_sets * k * 8);
        s.out_f = take(fused ? n_sets * k * 8 : 0);
        s.out_h = take(hits ? n_sets * k * 4 : 0);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -----------------------------------------------------------------------------------
enum {
    kFuseOk = 0,
    kFuseBadCounts = 1,      // n_sub or n_sets < 0
    kFuseBadK = 2,           // k outside [1, kFuseMaxK]
    kFuseBadFetch = 3,       // fetch_k outside [k, kFuseMaxFetch]
    kFuseBadFusion = 4,      // neither VDB_FUSE_RRF nor VDB_FUSE_MAX
    kFuseBadC = 5,           // rrf_c NaN, infinite or negative (RRF; MAX ignores it)
    kFuseNullPointer = 6,    // queries with n_sub > 0, or set_offsets / out_scores / out_indices with n_sets > 0
    kFuseBadMem = 7,         // a memory kind that is neither host (0) nor device (1)
    kFuseWeightsWithMax = 8  // weights given for VDB_FUSE_MAX
};
// What the scalars and the pointers' presence say, for both memory kinds.
inline int fuse_validate(int64_t n_sub, int64_t n_sets, int k, int fetch_k, int fusion, double rrf_c, bool has_queries,
                         bool has_offsets, bool has_weights, bool has_scores, bool has_indices, int mem) {
    if (n_sub < 0 || n_sets < 0) return kFuseBadCounts;
    if (k < 1 || k > kFuseMaxK) return kFuseBadK;
    if (fetch_k < k || fetch_k > kFuseMaxFetch) return kFuseBadFetch;
    if (fusion != kFuseRrf && fusion != kFuseMaxFusion) return kFuseBadFusion;
    if (fusion == kFuseRrf && !fuse_weight_ok(rrf_c)) return kFuseBadC;
    if (mem != 0 && mem != 1) return kFuseBadMem;
    if (n_sub > 0 && !has_queries) return kFuseNullPointer;
    if (n_sets > 0 && (!has_offsets || !has_scores || !has_indices)) return kFuseNullPointer;
    if (fusion == kFuseMaxFusion && has_weights) return kFuseWeightsWithMax;
    return kFuseOk;
}
// A host-memory call's offsets and weights.  *at: the offending offset index / set / weight index.
enum { kFuseListsOk = 0, kFuseBadOffsets = 1, kFuseSetTooLong = 2, kFuseBadWeight = 3 };
inline int fuse_validate_lists(const int64_t* offsets, int64_t n_sets, int64_t n_sub, const double* weights, int64_t* at) {
    for (int64_t s = 0; s <= n_sets && n_sets > 0; ++s) {
        const int64_t o = offsets[s];
        if (o < 0 || o > n_sub || (s > 0 && o < offsets[s - 1])) {
            *at = s;
            return kFuseBadOffsets;
        }
        if (s > 0 && o - offsets[s - 1] > kFuseMaxLists) {
            *at = s - 1;
            return kFuseSetTooLong;
        }
    }
    if (weights)
        for (int64_t i = 0; i < n_sub; ++i)
            if (!fuse_weight_ok(weights[i])) {
                *at = i;
                return kFuseBadWeight;
            }
    return kFuseListsOk;
}

}  // namespace vdb
