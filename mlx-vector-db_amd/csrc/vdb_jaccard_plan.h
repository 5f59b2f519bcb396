// vdb_jaccard_plan.h — the host arithmetic of vdb_index_search_jaccard (vdb_api.cpp) and the decisions
// its two kernels share with it (vdb_jaccard.hip, the popcount form; vdb_jaccard_mfma.hip, the int8-MFMA
// form): the exact keys of a similarity that is a ratio, the query-block size and LDS layout of the
// popcount form, the LDS layout of the MFMA form, the per-call scratch, the validation (one enum value
// per cause) and the choice between the forms.  The column, its tiles, the deal of tiles to segments
// and waves, the mask words and the MFMA bit mapping are the Hamming search's (vdb_hamming_plan.h).
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/jaccard_plan_check.cpp).
//
// The keys.  s = i / u with 0 <= i <= u <= 8 192 (u == 0: both sets empty, s = 1).  Two distinct
// similarities differ by at least 1 / (8192 * 8191) > 2^-26, which fp32 cannot separate.
//  - The popcount form ranks by the IEEE fp64 quotient (double)i / (double)u, higher is better.  The
//    quotient is the correctly rounded value of the rational, so equal ratios (1/2, 2/4) give the same
//    double; rounding is monotone and moves a value by at most 2^-53 relative, far less than the 2^-26
//    gap, so distinct ratios stay distinct and in order.
//  - The MFMA form ranks by the 32-bit integer jac_key_hi = floor((u - i) * 2^27 / u), lower is better.
//    It is a function of the ratio alone; distinct values of 1 - s are more than 2 / 2^27 apart, so their
//    floors differ and keep the order.  It is formed only for entries that pass the threshold; the test
//    itself (jac_pass) is one 64-bit multiply and two compares, the cross-multiplication of (u - i) / u
//    against the threshold key T / 2^27: floor(x) < T <=> x < T for an integer T.
// Neither key gives back i and u: the kernels' tails recount them for the k winners (vdb_jaccard_tail.h).
#pragma once
#include <stdint.h>

#include "vdb_hamming_plan.h"

#define VDB_JAC_HD VDB_HAM_HD

namespace vdb {

// ---- the exact keys -----------------------------------------------------------------------------------
// The definition of the order: is i1 / u1 greater than i2 / u2 (u == 0 counts as 1 / 1)?  Products are
// at most 2^26.
VDB_JAC_HD inline bool jac_greater(int i1, int u1, int i2, int u2) {
    if (u1 == 0) i1 = u1 = 1;
    if (u2 == 0) i2 = u2 = 1;
    return (int64_t)i1 * u2 > (int64_t)i2 * u1;
}
// The popcount form's key: higher is better.
VDB_JAC_HD inline double jac_key(int i, int u) { return u == 0 ? 1.0 : (double)i / (double)u; }
// The MFMA form's key: lower is better, 0 (s = 1) .. 2^27 (s = 0).  The fp64 quotient of the two exact
// integers is within 2^-25 of the rational (the quotient is below 2^28), and a rational that is not an
// integer is at least 1 / u >= 2^-13 from the next one, so the truncation is the exact floor.
constexpr int kJacKeyShift = 27;
VDB_JAC_HD inline uint32_t jac_key_hi(int i, int u) {
    const int u1 = u == 0 ? 1 : u;
    return (uint32_t)((double)((int64_t)(u - i) << kJacKeyShift) / (double)u1);
}
VDB_JAC_HD inline uint64_t jac_key64(int i, int u, uint32_t row) { return ((uint64_t)jac_key_hi(i, u) << 32) | row; }
// jac_key64(i, u, row) < thr, without the division.  thr = T << 32 | row_t: the key is below it when
// (u - i) * 2^27 < T * u, or when it lies in [T * u, (T + 1) * u) (the same T) and the row is lower.
// T * u < 2^45 for every 32-bit T.
VDB_JAC_HD inline bool jac_pass(int i, int u, uint32_t row, uint64_t thr) {
    const uint64_t u1 = u == 0 ? 1u : (uint64_t)u;
    const uint64_t lhs = (uint64_t)(u - i) << kJacKeyShift;
    const uint64_t tu = (thr >> 32) * u1;
    return lhs < tu + u1 && (lhs < tu || row < (uint32_t)thr);
}

// ---- the popcount form (vdb_jaccard.hip) ----------------------------------------------------------------
// As the Hamming search: 4 waves, a lane per row, a wave per tile, a block of QB queries in LDS.  What
// differs is the width of a top-k entry: an fp64 key and a uint32 row, 12 bytes against 8, and |q| of
// every query of the block beside the query words.
constexpr int kJacMaxQB = 8;      // (16 queries of the shortest k do not fit twice: checked by the sweep)
constexpr int kJacEntryBytes = 12;
constexpr int kJacQpopBytes = 64;  // |q| of up to kJacMaxQB queries as int32, padded so that the fp64 keys stay aligned
static_assert(kJacMaxQB * 4 <= kJacQpopBytes && kJacQpopBytes % 8 == 0, "the |q| words fit their pad");
// The tail merge's buffer (merge_block_lds<double, uint32_t>(KE)).
VDB_JAC_HD inline int64_t jac_merge_lds(int KE) {
    const int c = ham_cap(KE) > kHamMergeBuf ? ham_cap(KE) : kHamMergeBuf;
    return (int64_t)c * kJacEntryBytes;
}
// LDS of one workgroup: qb queries of W words, their |q|, then per (wave, query) one WaveTopK buffer:
// keys [waves][qb][cap] fp64, then rows [waves][qb][cap] uint32; the tail merge's buffer takes the
// top-k buffers' place.
VDB_JAC_HD inline int64_t jac_query_lds(int qb, int W) { return ham_query_lds(qb, W) + kJacQpopBytes; }
VDB_JAC_HD inline int64_t jac_qpop_off(int qb, int W) { return ham_query_lds(qb, W); }
VDB_JAC_HD inline int64_t jac_topk_lds(int qb, int KE) { return (int64_t)kHamWaves * qb * ham_cap(KE) * kJacEntryBytes; }
VDB_JAC_HD inline int64_t jac_lds_bytes(int qb, int W, int KE, bool merge) {
    const int64_t tk = jac_topk_lds(qb, KE), mg = merge ? jac_merge_lds(KE) : 0;
    return jac_query_lds(qb, W) + (tk > mg ? tk : mg);
}
VDB_JAC_HD inline int64_t jac_lds_key_off(int wv, int q, int qb, int W, int KE) {
    return jac_query_lds(qb, W) + ((int64_t)wv * qb + q) * ham_cap(KE) * 8;
}
VDB_JAC_HD inline int64_t jac_lds_row_off(int wv, int q, int qb, int W, int KE) {
    return jac_query_lds(qb, W) + (int64_t)kHamWaves * qb * ham_cap(KE) * 8 + ((int64_t)wv * qb + q) * ham_cap(KE) * 4;
}
// QB: the largest power of two <= kJacMaxQB for which kHamWgPerCuLds workgroups of the longest code fit
// the LDS limit, the merge buffer included: 8 up to k = 64, 4 to 128, 2 to 256, 1 above.  Above k = 512
// one query's buffers are 97 KiB: a single workgroup per CU, still inside the limit.
VDB_JAC_HD inline int jac_qb(int k) {
    const int KE = ham_ke(k);
    int qb = kJacMaxQB;
    while (qb > 1 && kHamWgPerCuLds * jac_lds_bytes(qb, kHamMaxWords, KE, true) > kHamLdsLimit) qb >>= 1;
    return qb;
}
// The block a launch uses: QB, or the power of two that covers a smaller batch.
VDB_JAC_HD inline int jac_block(int k, int n_queries) {
    const int qb = jac_qb(k);
    int p = 1;
    while (p < n_queries && p < qb) p <<= 1;
    return p;
}

// ---- the int8-MFMA form (vdb_jaccard_mfma.hip) ----------------------------------------------------------
// Stored bits and query bits both become the int8 0 / 1 (ham_mfma_row4), so an accumulator holds i.
// Blocks of kHamMfmaQB queries, k <= kHamMfmaMaxK and the candidate buffers of vdb_mfma_topk.h, as the
// Hamming search's MFMA form.  LDS: that form's regions (query words, candidate buffers, thresholds,
// counts), then |q| of the block's queries [QB] int32 and the row popcounts of every wave's tile
// [waves][64] int32.  The longest code's query block is 64 KiB and fits beside the 64 KiB of candidate
// buffers: K needs no chunking.
VDB_JAC_HD inline int64_t jac_mfma_qpop_off(int W) { return ham_mfma_lds_bytes(W); }
VDB_JAC_HD inline int64_t jac_mfma_xpop_off(int W) { return jac_mfma_qpop_off(W) + (int64_t)kHamMfmaQB * 4; }
VDB_JAC_HD inline int64_t jac_mfma_lds_bytes(int W) { return jac_mfma_xpop_off(W) + (int64_t)kHamWaves * kHamTileRows * 4; }
VDB_JAC_HD inline int jac_mfma_qb(int k) {
    if (k < 1 || k > kHamMfmaMaxK) return 0;
    return jac_mfma_lds_bytes(kHamMaxWords) + kHamMfmaStaticLds <= kHamLdsLimit ? kHamMfmaQB : 0;
}
// Which form a call takes.  knob ("jaccard_mfma"): 0 = by the batch size, 1 = the MFMA form whenever
// the call is eligible (k <= kHamMfmaMaxK; every width is), 2 = never.  The smallest batch that takes
// the MFMA form by itself is a measurement (at k = 10 it wins from 16 queries on 1M rows
// of 1 024 and 2 048 bits but loses there on 10M rows of 256 bits, and wins from 64 on all three); 0
// would mean "not measured": auto never takes it.
constexpr int kJacMfmaMinQueries = 64;
VDB_JAC_HD inline bool jaccard_knob_ok(int64_t v) { return v >= 0 && v <= 2; }
VDB_JAC_HD inline bool jaccard_use_mfma(int64_t knob, int n_queries, int k, int n_bytes) {
    if (knob == 2 || jac_mfma_qb(k) == 0 || n_bytes < 1 || n_bytes > kHamMaxBytes || n_queries < 1) return false;
    return knob == 1 || (kJacMfmaMinQueries > 0 && n_queries >= kJacMfmaMinQueries);
}

// ---- scratch --------------------------------------------------------------------------------------------
struct JaccardScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t done, lk, li, mk, mi;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, mask, in_bytes, out0, out_n, out_u, out_i, out_bytes;
    int64_t mask_words, total;
};
inline JaccardScratch jaccard_scratch(int n_queries, int n_bytes, int k, int qb, int n_seg, int64_t rows, bool host,
                                      bool masked) {
    JaccardScratch s{};
    const int64_t B = n_queries, KE = ham_ke(k);
    s.mask_words = ham_mask_words(rows);
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += ham_align(bytes);
        return at;
    };
    s.done = take((int64_t)ham_n_blocks(n_queries, qb) * 4);
    s.lk = take(n_seg > 1 ? B * n_seg * KE * 8 : 0);
    s.li = take(n_seg > 1 ? B * n_seg * KE * 4 : 0);
    s.mk = take(n_seg > 1 ? B * KE * 8 : 0);
    s.mi = take(n_seg > 1 ? B * KE * 4 : 0);
    s.in0 = o;
    if (host) {
        s.q = take(B * n_bytes);
        s.mask = take(masked ? s.mask_words * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_n = take(B * k * 4);
        s.out_u = take(B * k * 4);
        s.out_i = take(B * k * 8);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -----------------------------------------------------------------------------------------
enum {
    kJacOk = 0,
    kJacBadCount = 1,     // n_queries outside [0, kHamMaxQueries]
    kJacBadK = 2,         // k outside [1, kHamMaxK]
    kJacBadMem = 3,       // a memory kind that is neither host (0) nor device (1)
    kJacNullPointer = 4,  // queries / out_inter / out_union / out_indices NULL with n_queries > 0
    kJacNoColumn = 5      // no code column attached (or one that does not cover the rows)
};
inline int jaccard_validate_call(int64_t n_queries, int k, bool has_queries, bool has_inter, bool has_union, bool has_idx,
                                 int mem, bool column) {
    if (n_queries < 0 || n_queries > kHamMaxQueries) return kJacBadCount;
    if (k < 1 || k > kHamMaxK) return kJacBadK;
    if (mem != 0 && mem != 1) return kJacBadMem;
    if (n_queries > 0 && (!has_queries || !has_inter || !has_union || !has_idx)) return kJacNullPointer;
    if (!column) return kJacNoColumn;
    return kJacOk;
}

}  // namespace vdb
