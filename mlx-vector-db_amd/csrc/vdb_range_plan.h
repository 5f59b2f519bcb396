// vdb_range_plan.h — the host arithmetic of vdb_index_search_range (vdb_api.cpp) and the index
// arithmetic its kernels share with it (vdb_range.hip): the query-block size, how the rows are
// dealt to workgroups and waves, the hit bitmap and its prefix, the per-call scratch, the
// threshold-to-key conversion and the validation of a host-memory call.
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/range_plan_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_RANGE_HD __host__ __device__
#else
#define VDB_RANGE_HD
#endif

namespace vdb {

// Phase 1 (scan).  A workgroup is 4 waves and owns one chunk of kRangeWgWords bitmap words
// (kRangeWgRows rows); wave w owns words [4 w, 4 w + 4) of the chunk, one whole 32-row word at a
// time, kRangeNB rows of it in registers per trip.  Lane j of a wave accumulates the word of query
// j of the block, so a block is at most 64 queries.
constexpr int kRangeWaves = 4;
constexpr int kRangeNB = 4;
constexpr int kRangeWaveWords = 4;
constexpr int kRangeWgWords = kRangeWaves * kRangeWaveWords;  // 16 words
constexpr int kRangeWgRows = 32 * kRangeWgWords;              // 512 rows
constexpr int kRangeMaxBlock = 64;
// The queries of a block are read through L1 / L2 once per kRangeNB rows: a block's queries are
// kept to this many bytes so that they stay cache-resident beside the streaming corpus rows.
constexpr int64_t kRangeQueryBytes = 128 * 1024;
// Phase 2 (emit): a workgroup of 256 threads takes one word per thread, i.e. 16 chunks.
constexpr int kRangeEmitWords = 256;
// ... and the scoring of the emitted slots: one wave per slot, at most this many workgroups.
constexpr int kRangeScoreWgs = 4096;
// Most result slots of one call, n_queries x cap: the scratch of a host-memory call holds 20 bytes
// per slot, so every byte count stays below 2^41 and far inside int64 whatever the batch size.
constexpr int64_t kRangeMaxSlots = (int64_t)1 << 36;

// Queries per block for rows of Dp padded dims: 64, fewer once 64 queries pass the byte budget.
VDB_RANGE_HD inline int range_query_block(int Dp) {
    const int64_t row = (int64_t)(Dp > 0 ? Dp : 1) * 4;
    const int64_t qb = kRangeQueryBytes / row;
    return qb < 1 ? 1 : qb > kRangeMaxBlock ? kRangeMaxBlock : (int)qb;
}

// ---- shared with the kernels --------------------------------------------------------------------
VDB_RANGE_HD inline int64_t range_n_words(int64_t N) { return (N + 31) / 32; }
VDB_RANGE_HD inline int64_t range_n_chunks(int64_t n_words) { return (n_words + kRangeWgWords - 1) / kRangeWgWords; }
// Word i of wave `wave` of chunk `chunk` (may be at or past n_words: the caller stops there).
VDB_RANGE_HD inline int64_t range_wave_word(int64_t chunk, int wave, int i) {
    return chunk * kRangeWgWords + (int64_t)wave * kRangeWaveWords + i;
}
// The bits of word w that name a row below N.
VDB_RANGE_HD inline uint32_t range_valid_bits(int64_t w, int64_t N) {
    const int64_t left = N - w * 32;
    return left >= 32 ? 0xFFFFFFFFu : left <= 0 ? 0u : ((1u << (int)left) - 1u);
}
// Threshold (score units) -> the key bound kt: a row passes iff key >= kt.  cosine: the similarity
// itself; euclidean: a radius t, kt = -(t * t) with one multiply.  A NaN threshold or a negative
// radius gives NaN, which no key is at or above (a device-memory call's count is then 0).
VDB_RANGE_HD inline double range_kt(int metric, double t) {
    if (metric == 0) return t;
    if (!(t >= 0.0)) return (double)NAN;
    return -(t * t);
}
// Slots of a query that hold a row: the first min(count, cap) hits.
VDB_RANGE_HD inline int64_t range_filled(int64_t count, int64_t cap) { return count < cap ? count : cap; }
// Workgroups of the emit kernel per query, and whether the one that starts at exclusive prefix
// `base` (hits below its first word) has anything to write.
VDB_RANGE_HD inline int64_t range_emit_wgs(int64_t n_words) { return (n_words + kRangeEmitWords - 1) / kRangeEmitWords; }
VDB_RANGE_HD inline bool range_emit_live(int64_t base, int64_t cap) { return base < cap; }
// Workgroups of the score kernel per query (4 slots per workgroup trip).
VDB_RANGE_HD inline int range_score_wgs(int64_t cap) {
    const int64_t g = (cap + kRangeWaves - 1) / kRangeWaves;
    return g < 1 ? 1 : g > kRangeScoreWgs ? kRangeScoreWgs : (int)g;
}

// ---- scratch ------------------------------------------------------------------------------------
inline int64_t range_align(int64_t b) { return (b + 255) / 256 * 256; }
struct RangeScratch {
    int block;  // queries per block (range_query_block)
    int64_t n_words, n_chunks;
    // byte offsets into the workspace (each 256-byte aligned): the batch's query norms; one
    // block's hit bitmap H [block][n_words], chunk counts / prefixes part [block][n_chunks] and
    // totals cnt [block], reused block after block
    int64_t qn64, H, part, cnt;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, thr, mask, in_bytes, out0, out_c, out_i, out_s, out_k, out_bytes;
    int64_t total;
};
inline RangeScratch range_scratch(int n_queries, int dim, int Dp, int64_t N, int64_t cap, bool host, bool has_mask,
                                  bool keys) {
    RangeScratch s{};
    const int64_t B = n_queries;
    s.block = range_query_block(Dp);
    if (s.block > n_queries) s.block = n_queries > 0 ? n_queries : 1;
    s.n_words = range_n_words(N);
    s.n_chunks = range_n_chunks(s.n_words);
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += range_align(bytes);
        return at;
    };
    s.qn64 = take(B * 8);
    s.H = take((int64_t)s.block * s.n_words * 4);
    s.part = take((int64_t)s.block * s.n_chunks * 4);
    s.cnt = take((int64_t)s.block * 8);
    s.in0 = o;
    if (host) {
        s.q = take(B * dim * 4);
        s.thr = take(B * 8);
        s.mask = take(has_mask ? s.n_words * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_c = take(B * 8);
        s.out_i = take(B * cap * 8);
        s.out_s = take(B * cap * 4);
        s.out_k = take(keys ? B * cap * 8 : 0);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation of a host-memory call -----------------------------------------------------------
enum {
    kRangeOk = 0,
    kRangeBadCap = 1,        // cap negative, or n_queries * cap above kRangeMaxSlots
    kRangeNanThreshold = 2,  // a NaN threshold
    kRangeNegRadius = 3      // euclidean: a negative radius
};
// The cap against the batch size (all a device-memory call can be checked for): 0 <= cap and
// n_queries * cap <= kRangeMaxSlots, tested by division so that the product is never formed.
inline int range_validate_cap(int n_queries, int64_t cap) {
    if (cap < 0) return kRangeBadCap;
    const int64_t B = n_queries > 0 ? n_queries : 1;
    return cap > kRangeMaxSlots / B ? kRangeBadCap : kRangeOk;
}
// The thresholds of a host-memory call.  *where: the offending query.
inline int range_validate(int metric, const double* thresholds, int n_queries, int64_t* where) {
    int64_t dummy;
    if (!where) where = &dummy;
    *where = 0;
    for (int b = 0; b < n_queries; ++b) {
        const double t = thresholds[b];
        *where = b;
        if (t != t) return kRangeNanThreshold;
        if (metric != 0 && t < 0.0) return kRangeNegRadius;
    }
    *where = 0;
    return kRangeOk;
}

}  // namespace vdb
