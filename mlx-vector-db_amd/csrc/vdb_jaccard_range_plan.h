// vdb_jaccard_range_plan.h — the host arithmetic of vdb_index_search_jaccard_range (vdb_api.cpp) and the
// decisions its kernels share with it (vdb_jaccard_range.hip): the exact test of a ratio against a
// rational threshold, what makes a threshold bad, the query-block size of the two scans, their LDS
// layouts, which scan serves a call, the per-call scratch and the validation (one enum value per cause).
// The chunk / tile / word geometry, the eligible rows of a word, the accumulator-row mapping, the stage
// stride and the fill's deal of lanes are the Hamming range search's (vdb_hamming_range_plan.h).
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/jaccard_range_plan_check.cpp).
#pragma once
#include <stdint.h>

#include "vdb_hamming_range_plan.h"
#include "vdb_jaccard_plan.h"

namespace vdb {

// ---- the test ---------------------------------------------------------------------------------------
// The threshold of a query is the exact rational num / den, 1 <= den <= 2^18, 0 <= num <= den.  With
// i <= u <= 8 192 = 2^13 both products of the cross-multiplication are at most 2^31: they fit an
// unsigned 32-bit register, so the test is two 32-bit multiplies and one compare, with no division and
// no rounding.  u == 0 (query and row both empty) counts as 1 / 1, vdb_index_search_jaccard's rule.
constexpr int kJacRangeMaxDen = 1 << 18;
static_assert((int64_t)kHamMaxBytes * 8 * kJacRangeMaxDen <= ((int64_t)1 << 31), "a product fits 32 unsigned bits");
VDB_JAC_HD inline bool jac_range_bad_threshold(int num, int den) {
    return den < 1 || den > kJacRangeMaxDen || num < 0 || num > den;
}
VDB_JAC_HD inline bool jac_range_pass(int i, int u, int num, int den) {
    if (u == 0) i = u = 1;
    return (uint32_t)i * (uint32_t)den >= (uint32_t)num * (uint32_t)u;
}
// What a kernel holds for an absent query or a bad device-memory threshold: i * 0 >= 1 * u is false
// for every u >= 1 (and u == 0 is tested as 1), so nothing passes.
constexpr int kJacRangeNoneNum = 1;
constexpr int kJacRangeNoneDen = 0;

// ---- the popcount scan ------------------------------------------------------------------------------
// The Hamming range scan's shape: one lane per row, a pass of kHamPassWords words of the row in
// registers (32), blocks of up to 16 queries.  On top of it a lane keeps |x| of its row (one register,
// running across the passes of a long code) and, for a long code, one running i per query (16).  LDS:
// the block's queries as whole passes of words, then |q|, num and den, [qb] int32 each.
constexpr int kJacRangeMaxQB = kHamRangeMaxQB;  // 16
static_assert(kHamPassWords * 2 + kJacRangeMaxQB + 1 <= 64, "a pass, the running i and |x| are half the register budget");
VDB_JAC_HD inline int64_t jac_range_pop_qpop_off(int qb, int W) { return ham_query_lds(qb, W); }
VDB_JAC_HD inline int64_t jac_range_pop_num_off(int qb, int W) { return jac_range_pop_qpop_off(qb, W) + (int64_t)qb * 4; }
VDB_JAC_HD inline int64_t jac_range_pop_den_off(int qb, int W) { return jac_range_pop_num_off(qb, W) + (int64_t)qb * 4; }
VDB_JAC_HD inline int64_t jac_range_pop_lds(int qb, int W) { return jac_range_pop_den_off(qb, W) + (int64_t)qb * 4; }
// The block a launch uses: the power of two that covers the batch, at most kJacRangeMaxQB, and no more
// than kHamWgPerCuLds workgroups' LDS allows (it allows all of them).
VDB_JAC_HD inline int jac_range_pop_block(int n_queries, int W) {
    int qb = kJacRangeMaxQB;
    while (qb > 1 && kHamWgPerCuLds * jac_range_pop_lds(qb, W) > kHamLdsLimit) qb >>= 1;
    int p = 1;
    while (p < n_queries && p < qb) p <<= 1;
    return p;
}

// ---- the MFMA scan ----------------------------------------------------------------------------------
// Blocks of 64 queries, both sides as the int8 0 / 1 (ham_mfma_row4): an accumulator register holds i.
// LDS: the query words word-major [ham_mfma_words(W)][64], the staged bitmap words of the chunk
// [64][kHamRangeStageStride] uint32, then |q|, num and den [64] int32 each, then the row popcounts of
// every wave's tile [waves][64] int32.
constexpr int kJacRangeMfmaQB = kHamMfmaQB;
VDB_JAC_HD inline int64_t jac_range_mfma_stage_off(int W) { return ham_mfma_query_lds(W); }
VDB_JAC_HD inline int64_t jac_range_mfma_qpop_off(int W) {
    return jac_range_mfma_stage_off(W) + (int64_t)kJacRangeMfmaQB * kHamRangeStageStride * 4;
}
VDB_JAC_HD inline int64_t jac_range_mfma_num_off(int W) { return jac_range_mfma_qpop_off(W) + (int64_t)kJacRangeMfmaQB * 4; }
VDB_JAC_HD inline int64_t jac_range_mfma_den_off(int W) { return jac_range_mfma_num_off(W) + (int64_t)kJacRangeMfmaQB * 4; }
VDB_JAC_HD inline int64_t jac_range_mfma_xpop_off(int W) { return jac_range_mfma_den_off(W) + (int64_t)kJacRangeMfmaQB * 4; }
VDB_JAC_HD inline int64_t jac_range_mfma_lds(int W) {
    return jac_range_mfma_xpop_off(W) + (int64_t)kHamRangeWaves * kHamTileRows * 4;
}
// Two workgroups per CU at the longest code: 64 KiB of queries + 4.25 KiB of staging + 768 bytes of
// query scalars + 1 KiB of row popcounts each.
static_assert(kHamWgPerCuLds * ((int64_t)(kHamMaxWords + 1) / 2 * 2 * kHamMfmaQB * 8 + kHamMfmaQB * (kHamRangeStageStride + 3) * 4 +
                                kHamRangeWaves * kHamTileRows * 4) <= kHamLdsLimit,
              "two workgroups of the MFMA Jaccard range scan fit a CU's LDS");

// The smallest batch that takes the MFMA scan by itself (knob "jaccard_range_mfma" = 0).  Measured for
// this call (tools/jaccard_range_bench.py): of the batches 1, 16, 64, 256 and 1 024 the
// MFMA scan loses at 16 and below (2x to 4x) and wins from 64 up, 1.5x to 1.8x, on 1M x 1 024 bits, 1M x
// 2 048 bits and 10M x 256 bits, counting only and with about 100 hits per query.  (0 would mean "not
// measured": auto never takes the MFMA scan, the convention of vdb_jaccard_plan.h.)
constexpr int kJacRangeMfmaMinQueries = 64;
// knob: 0 = by the batch size, 1 = the MFMA scan for every call, 2 = never.
VDB_JAC_HD inline bool jaccard_range_knob_ok(int64_t v) { return v >= 0 && v <= 2; }
VDB_JAC_HD inline bool jaccard_range_use_mfma(int64_t knob, int n_queries) {
    if (knob == 2 || n_queries < 1) return false;
    return knob == 1 || (kJacRangeMfmaMinQueries > 0 && n_queries >= kJacRangeMfmaMinQueries);
}
VDB_JAC_HD inline int jac_range_block(bool mfma, int n_queries, int W) {
    return mfma ? kJacRangeMfmaQB : jac_range_pop_block(n_queries, W);
}

// ---- scratch ----------------------------------------------------------------------------------------
struct JacRangeScratch {
    int block;  // queries per block of the scan that will run
    int64_t n_words, n_chunks;
    // byte offsets into the workspace (each 256-byte aligned): one block's hit bitmap H [block][n_words],
    // chunk counts / prefixes part [block][n_chunks] and totals cnt [block], reused block after block
    int64_t H, part, cnt;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, num, den, mask, in_bytes, out0, out_c, out_i, out_n, out_u, out_bytes;
    int64_t total;
};
inline JacRangeScratch jaccard_range_scratch(int n_queries, int n_bytes, int block, int64_t N, int64_t cap, bool host,
                                             bool has_mask) {
    JacRangeScratch s{};
    const int64_t B = n_queries;
    s.block = block < 1 ? 1 : block;
    if (s.block > n_queries) s.block = n_queries > 0 ? n_queries : 1;
    s.n_words = range_n_words(N);
    s.n_chunks = range_n_chunks(s.n_words);
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += ham_align(bytes);
        return at;
    };
    s.H = take((int64_t)s.block * s.n_words * 4);
    s.part = take((int64_t)s.block * s.n_chunks * 4);
    s.cnt = take((int64_t)s.block * 8);
    s.in0 = o;
    if (host) {
        s.q = take(B * n_bytes);
        s.num = take(B * 4);
        s.den = take(B * 4);
        s.mask = take(has_mask ? s.n_words * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_c = take(B * 8);
        s.out_i = take(B * cap * 8);
        s.out_n = take(B * cap * 4);
        s.out_u = take(B * cap * 4);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -------------------------------------------------------------------------------------
enum {
    kJacRangeOk = 0,
    kJacRangeNoColumn = 1,      // no code column attached (or one that does not cover the rows)
    kJacRangeBadCount = 2,      // n_queries outside [0, kHamMaxQueries]
    kJacRangeBadCap = 3,        // range_validate_cap
    kJacRangeBadMem = 4,        // a memory kind that is neither host (0) nor device (1)
    kJacRangeNullPointer = 5,   // queries / thr_num / thr_den / out_counts NULL with n_queries > 0
    kJacRangeNullLists = 6,     // out_indices / out_inter / out_union NULL with n_queries > 0 and cap > 0
    kJacRangeBadThreshold = 7   // host memory: jac_range_bad_threshold (*where: the query)
};
// (num / den: read only for a host-memory call that has passed every other check)
inline int jaccard_range_validate(bool column, int64_t n_queries, int64_t cap, int mem, bool has_queries, bool has_num,
                                  bool has_den, bool has_counts, bool has_idx, bool has_inter, bool has_union,
                                  const int32_t* num, const int32_t* den, int64_t* where) {
    int64_t dummy;
    if (!where) where = &dummy;
    *where = 0;
    if (!column) return kJacRangeNoColumn;
    if (n_queries < 0 || n_queries > kHamMaxQueries) return kJacRangeBadCount;
    if (range_validate_cap((int)n_queries, cap)) return kJacRangeBadCap;
    if (mem != 0 && mem != 1) return kJacRangeBadMem;
    if (n_queries == 0) return kJacRangeOk;
    if (!has_queries || !has_num || !has_den || !has_counts) return kJacRangeNullPointer;
    if (cap > 0 && (!has_idx || !has_inter || !has_union)) return kJacRangeNullLists;
    if (mem == 0)
        for (int64_t b = 0; b < n_queries; ++b)
            if (jac_range_bad_threshold(num[b], den[b])) {
                *where = b;
                return kJacRangeBadThreshold;
            }
    return kJacRangeOk;
}

}  // namespace vdb
