// vdb_sparse_inv_plan.h — the host arithmetic of the inverted (term-major) sparse search
// (vdb_sparse_inv.hip) and the decisions its kernels share with vdb_api.cpp: when postings are built
// and when they serve a call, the row-block size R(KE), the deal of row blocks to a query's
// workgroups, the rows a wave owns in a block, the lower bound by row inside a term's postings, the
// LDS layout with its 160 KiB check, and a CPU restatement of "key of row r by postings".  Plain C++
// with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/sparse_inv_plan_check.cpp).
//
// The postings are the column again in (term ascending, row ascending) order: inv_tptr [n_terms + 1]
// and inv_posts [nnz] of (row, weight).  That order defines the arrays completely.
#pragma once
#include <stdint.h>

#include "vdb_sparse_plan.h"

namespace vdb {

// Most terms a column may name and still get postings: inv_tptr is 8 (n_terms + 1) bytes, 32 MiB here.
constexpr int32_t kSparseInvMaxTerms = 1 << 22;
// Rows of a row block at most, and the LDS a workgroup may take.
constexpr int kSparseInvMaxBlockRows = 8192;
constexpr int64_t kSparseInvLdsLimit = 160 * 1024;
// Knob "sparse_inverted" = 0 (auto): the inverted kernel serves an index of at least this many rows
// (the smallest measured size at which it wins at every measured query length and
// batch).  By rows alone: a device-memory call may read nothing back.
constexpr int64_t kSparseInvAutoRows = 1000000;

// One posting: the row and the stored weight side by side, so one 8-byte load brings both (the row in
// the low word).
struct SparsePost {
    uint32_t row;
    float weight;
};

// ---- which kernel ---------------------------------------------------------------------------------
inline bool sparse_inv_knob_ok(int64_t knob) { return knob >= 0 && knob <= 2; }
// Whether vdb_index_set_sparse builds postings: not under knob 2, and not for a vocabulary above the cap.
inline bool sparse_inv_builds(int64_t knob, int32_t n_terms) { return knob != 2 && n_terms <= kSparseInvMaxTerms; }
// Whether a call over N rows goes to the inverted kernel (built: postings exist for the attached column).
inline bool sparse_inv_serves(int64_t knob, bool built, int64_t N) {
    if (!built || knob == 2) return false;
    return knob == 1 || N >= kSparseInvAutoRows;
}
// Bits of a term id that the build's radix sort has to look at: enough for n_terms - 1, at least 1.
inline int sparse_inv_term_bits(int32_t n_terms) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) < (int64_t)n_terms) ++b;
    return b;
}

// ---- LDS ------------------------------------------------------------------------------------------
// What vdb_common.h's WaveTopK<double, uint32_t>::capacity and vdb_merge_block.h's merge_block_lds
// give (restated here without HIP; the launch compares them and refuses to run on a difference).
VDB_SPARSE_HD inline int64_t sparse_inv_topk_cap(int KE) {
    const int64_t want = 2 * (int64_t)KE > (int64_t)KE + 64 ? 2 * (int64_t)KE : (int64_t)KE + 64;
    int64_t p = 1;
    while (p < want) p <<= 1;
    return p;
}
VDB_SPARSE_HD inline int64_t sparse_inv_merge_lds(int KE) {
    const int64_t cap = sparse_inv_topk_cap(KE);
    return (cap > 1024 ? cap : 1024) * 12;
}
// One workgroup: the query's terms and weights (8 KiB), R fp64 accumulators, R matched flags (one bit
// each, 32 rows a word), then the four WaveTopK buffers (the tail merge's buffer takes their place).
struct SparseInvLds {
    int64_t acc, flags, tk, total;
};
VDB_SPARSE_HD inline SparseInvLds sparse_inv_lds(int R, int KE, bool merge) {
    SparseInvLds l{};
    l.acc = kSparseQueryLds;
    l.flags = l.acc + (int64_t)R * 8;
    l.tk = (l.flags + (int64_t)R / 8 + 15) / 16 * 16;
    const int64_t tk = (int64_t)kSparseWaves * sparse_inv_topk_cap(KE) * 12;
    const int64_t mg = merge ? sparse_inv_merge_lds(KE) : 0;
    l.total = l.tk + (tk > mg ? tk : mg);
    return l;
}
// R(KE): the largest power of two up to kSparseInvMaxBlockRows whose layout (with the merge buffer)
// fits the LDS limit; a multiple of 4 * 64 so that every wave owns whole groups of 64 rows.  0: none
// fits (no KE the call accepts gets there).
inline int sparse_inv_block_rows(int KE) {
    for (int R = kSparseInvMaxBlockRows; R >= kSparseWaves * 64; R >>= 1)
        if (sparse_inv_lds(R, KE, true).total <= kSparseInvLdsLimit) return R;
    return 0;
}

// ---- the deal of row blocks ---------------------------------------------------------------------
// Blocks of R rows; segment s of n_seg walks blocks s, s + n_seg, ..., so segments at or past the
// block count have nothing to do (and are not counted by the merge tail).
VDB_SPARSE_HD inline int64_t sparse_inv_n_blocks(int64_t N, int R) { return N <= 0 ? 0 : (N + R - 1) / R; }
VDB_SPARSE_HD inline int sparse_inv_live_segs(int64_t N, int R, int n_seg) {
    const int64_t c = sparse_inv_n_blocks(N, R);
    return c < n_seg ? (int)c : n_seg;
}
// Wave wv of 4 owns rows [lo, hi) of block c: a quarter of the block, cut at N.  (lo >= hi: none.)
struct SparseInvRows {
    int64_t lo, hi;
};
VDB_SPARSE_HD inline SparseInvRows sparse_inv_wave_rows(int64_t c, int wv, int R, int64_t N) {
    SparseInvRows r;
    r.lo = c * R + (int64_t)wv * (R / kSparseWaves);
    r.hi = r.lo + R / kSparseWaves;
    if (r.hi > N) r.hi = N;
    if (r.lo > N) r.lo = N;
    return r;
}

// ---- a term's postings ----------------------------------------------------------------------------
// The first position p in [lo, hi) whose row is >= row, hi when there is none (rows ascend in [lo, hi)).
VDB_SPARSE_HD inline int64_t sparse_inv_lower_bound(const SparsePost* posts, int64_t lo, int64_t hi, int64_t row) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)posts[mid].row < row)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// The postings of term t that fall in rows [rows.lo, rows.hi): [*p0, *p1).  The second search looks no
// further than the rows' count past the first (a row appears once in a term's postings).
VDB_SPARSE_HD inline void sparse_inv_range(const int64_t* tptr, const SparsePost* posts, int32_t t, SparseInvRows rows,
                                           int64_t* p0, int64_t* p1) {
    const int64_t b = tptr[t], e = tptr[t + 1];
    const int64_t lo = sparse_inv_lower_bound(posts, b, e, rows.lo);
    const int64_t span = rows.hi - rows.lo;
    *p0 = lo;
    *p1 = sparse_inv_lower_bound(posts, lo, e - lo > span ? lo + span : e, rows.hi);
}

// The key of row r by the postings, as the unit that owns r forms it: the query's terms in ascending
// order, each adding its posting for r (if any) into one accumulator.  Equal in every bit to
// sparse_row_key over the row's stored entries: the same adds in the same order, since term ids
// ascend within a row and within a query and a row appears at most once per term.
inline double sparse_inv_row_key(const int64_t* tptr, const SparsePost* posts, int64_t r, const int32_t* qt,
                                 const float* qw, int len, bool* matched) {
    double acc = 0.0;
    bool m = false;
    for (int j = 0; j < len; ++j) {
        const int64_t b = tptr[qt[j]], e = tptr[qt[j] + 1];
        const int64_t p = sparse_inv_lower_bound(posts, b, e, r);
        if (p == e || (int64_t)posts[p].row != r) continue;
        const double qd = (double)qw[j];
        acc = sparse_step(acc, posts[p].weight, qd);
        m = m || sparse_entry_matches(posts[p].weight, qd);
    }
    *matched = m;
    return acc;
}

}  // namespace vdb
