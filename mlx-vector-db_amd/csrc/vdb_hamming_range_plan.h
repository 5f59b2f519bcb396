// vdb_hamming_range_plan.h — the host arithmetic of vdb_index_search_hamming_range (vdb_api.cpp) and
// the decisions its kernels share with it (vdb_hamming_range.hip): how the code tiles of
// vdb_hamming_plan.h map onto the hit-bitmap words and chunks of vdb_range_plan.h, the query-block
// size of the two scans, their LDS layouts, which scan serves a call, the per-call scratch and the
// validation (one enum value per cause).
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/hamming_range_plan_check.cpp).
#pragma once
#include <stdint.h>

#include "vdb_hamming_plan.h"
#include "vdb_range_plan.h"

namespace vdb {

// ---- geometry -----------------------------------------------------------------------------------
// The hit bitmap is the dense range search's: 32-row words, chunks of kRangeWgWords words
// (kRangeWgRows rows), one workgroup of 4 waves per chunk.  A code tile is 64 rows, i.e. the two
// words 2 t and 2 t + 1, so a chunk is 8 tiles and wave w takes tiles 2 w and 2 w + 1 of it: the
// chunk's words 4 w .. 4 w + 3, as the dense scan deals them.
constexpr int kHamRangeWaves = kRangeWaves;
constexpr int kHamRangeChunkTiles = kRangeWgRows / kHamTileRows;            // 8
constexpr int kHamRangeWaveTiles = kHamRangeChunkTiles / kHamRangeWaves;    // 2
constexpr int kHamRangeTileWords = kHamTileRows / 32;                       // 2
static_assert(kHamRangeWaves == kHamWaves, "both parents use workgroups of 4 waves");
static_assert(kHamRangeChunkTiles * kHamTileRows == kRangeWgRows, "a chunk is whole tiles");
static_assert(kHamRangeWaveTiles * kHamRangeTileWords == kRangeWaveWords, "a wave's tiles are its words of the chunk");

// Tile i (0 or 1) of wave wv in chunk c; at or past ham_n_tiles(N) it is not loaded.
VDB_HAM_HD inline int64_t ham_range_tile(int64_t c, int wv, int i) {
    return c * kHamRangeChunkTiles + (int64_t)wv * kHamRangeWaveTiles + i;
}
// Bitmap word h (0 or 1) of tile t; at or past range_n_words(N) it is not written and counts zero.
VDB_HAM_HD inline int64_t ham_range_word(int64_t t, int h) { return t * kHamRangeTileWords + h; }
// The position of that word inside its chunk (0..15): where the MFMA scan stages it.
VDB_HAM_HD inline int ham_range_chunk_word(int wv, int i, int h) {
    return (wv * kHamRangeWaveTiles + i) * kHamRangeTileWords + h;
}
// The rows of word w a query may hit: below N, and the mask's bits (mask_word: 0xFFFFFFFF without one).
VDB_HAM_HD inline uint32_t ham_range_eligible(int64_t w, int64_t N, uint32_t mask_word) {
    return range_valid_bits(w, N) & mask_word;
}
// Row `row` of a 32 x 32 MFMA accumulator held in register v (0..15) of lane half `half`.
VDB_HAM_HD inline int ham_range_acc_row(int v, int half) { return 8 * (v >> 2) + 4 * half + (v & 3); }

// ---- the popcount scan ----------------------------------------------------------------------------
// One lane per row; a lane holds kHamPassWords words of its row (32 registers) at once.  Codes of up
// to kHamPassWords words are read once and decided query after query, with no state per query; longer
// codes carry one running distance per query across the passes: 16 more registers at a block of 16,
// which keeps the kernel far below the 128 registers at which a SIMD still holds 4 waves.  LDS: the
// block's queries as whole passes of words and its radii, 16.1 KiB at the longest code.
constexpr int kHamRangeMaxQB = kHamMaxQB;  // 16
VDB_HAM_HD inline bool ham_range_long(int W) { return W > kHamPassWords; }
VDB_HAM_HD inline int64_t ham_range_pop_radius_off(int qb, int W) { return ham_query_lds(qb, W); }
VDB_HAM_HD inline int64_t ham_range_pop_lds(int qb, int W) { return ham_range_pop_radius_off(qb, W) + (int64_t)qb * 4; }
static_assert(kHamPassWords * 2 + kHamRangeMaxQB <= 64, "a pass and the running distances are half the register budget");
// The block a launch uses: the power of two that covers the batch, at most kHamRangeMaxQB, and no more
// than kHamWgPerCuLds workgroups' LDS allows (it allows all of them).
VDB_HAM_HD inline int ham_range_pop_block(int n_queries, int W) {
    int qb = kHamRangeMaxQB;
    while (qb > 1 && kHamWgPerCuLds * ham_range_pop_lds(qb, W) > kHamLdsLimit) qb >>= 1;
    int p = 1;
    while (p < n_queries && p < qb) p <<= 1;
    return p;
}

// ---- the MFMA scan --------------------------------------------------------------------------------
// Blocks of kHamMfmaQB (64) queries, the operand mapping of vdb_hamming_plan.h.  LDS: the query words
// word-major [ham_mfma_words(W)][64], the staged bitmap words of the chunk [64][stride] uint32 (the
// stride is odd so that the 32 lanes of a half wave, one query each, write one word position into 32
// banks), the radii [64] and the query popcounts [64].
constexpr int kHamRangeMfmaQB = kHamMfmaQB;
constexpr int kHamRangeStageStride = kRangeWgWords + 1;  // 17
VDB_HAM_HD inline int64_t ham_range_mfma_stage_off(int W) { return ham_mfma_query_lds(W); }
VDB_HAM_HD inline int64_t ham_range_mfma_radius_off(int W) {
    return ham_range_mfma_stage_off(W) + (int64_t)kHamRangeMfmaQB * kHamRangeStageStride * 4;
}
VDB_HAM_HD inline int64_t ham_range_mfma_pop_off(int W) { return ham_range_mfma_radius_off(W) + (int64_t)kHamRangeMfmaQB * 4; }
VDB_HAM_HD inline int64_t ham_range_mfma_lds(int W) { return ham_range_mfma_pop_off(W) + (int64_t)kHamRangeMfmaQB * 4; }
// Two workgroups per CU at the longest code: 64 KiB of queries + 4.25 KiB of staging + 512 bytes each.
static_assert(kHamWgPerCuLds * ((int64_t)(kHamMaxWords + 1) / 2 * 2 * kHamMfmaQB * 8 + kHamMfmaQB * (kHamRangeStageStride + 2) * 4) <=
                  kHamLdsLimit,
              "two workgroups of the MFMA range scan fit a CU's LDS");

// The smallest batch that takes the MFMA scan by itself (knob "hamming_range_mfma" = 0).  Measured for
// this call (tools/hamming_range_bench.py): of the batches 1, 16, 64, 256 and 1 024 the
// MFMA scan loses at 16 and below and wins from 64 up, about 2x, on 1M x 1 024 bits and on 10M x 256
// bits, counting only and with about 100 hits per query.
constexpr int kHamRangeMfmaMinQueries = 64;
// knob: 0 = by the batch size, 1 = the MFMA scan for every call, 2 = never.
VDB_HAM_HD inline bool ham_range_use_mfma(int64_t knob, int n_queries) {
    if (knob == 2 || n_queries < 1) return false;
    return knob == 1 || n_queries >= kHamRangeMfmaMinQueries;
}
VDB_HAM_HD inline int ham_range_block(bool mfma, int n_queries, int W) {
    return mfma ? kHamRangeMfmaQB : ham_range_pop_block(n_queries, W);
}

// ---- the distance fill ----------------------------------------------------------------------------
// 16 lanes per filled slot (lane j adds words j, j + 16, ...), 16 slots per workgroup trip; at most
// this many workgroups per query.
constexpr int kHamRangeFillLanes = 16;
constexpr int kHamRangeFillSlots = 256 / kHamRangeFillLanes;
constexpr int kHamRangeFillWgs = 4096;
VDB_HAM_HD inline int ham_range_fill_wgs(int64_t cap) {
    const int64_t g = (cap + kHamRangeFillSlots - 1) / kHamRangeFillSlots;
    return g < 1 ? 1 : g > kHamRangeFillWgs ? kHamRangeFillWgs : (int)g;
}

// ---- scratch --------------------------------------------------------------------------------------
struct HamRangeScratch {
    int block;  // queries per block of the scan that will run
    int64_t n_words, n_chunks;
    // byte offsets into the workspace (each 256-byte aligned): one block's hit bitmap H [block][n_words],
    // chunk counts / prefixes part [block][n_chunks] and totals cnt [block], reused block after block
    int64_t H, part, cnt;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, radii, mask, in_bytes, out0, out_c, out_i, out_d, out_bytes;
    int64_t total;
};
inline HamRangeScratch hamming_range_scratch(int n_queries, int n_bytes, int block, int64_t N, int64_t cap, bool host,
                                             bool has_mask) {
    HamRangeScratch s{};
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
        s.radii = take(B * 4);
        s.mask = take(has_mask ? s.n_words * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_c = take(B * 8);
        s.out_i = take(B * cap * 8);
        s.out_d = take(B * cap * 4);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -----------------------------------------------------------------------------------
enum {
    kHamRangeOk = 0,
    kHamRangeNoColumn = 1,     // no code column attached (or one that does not cover the rows)
    kHamRangeBadCount = 2,     // n_queries outside [0, kHamMaxQueries]
    kHamRangeBadCap = 3,       // range_validate_cap
    kHamRangeBadMem = 4,       // a memory kind that is neither host (0) nor device (1)
    kHamRangeNullPointer = 5,  // queries / radii / out_counts NULL with n_queries > 0
    kHamRangeNullLists = 6,    // out_indices / out_distances NULL with n_queries > 0 and cap > 0
    kHamRangeNegRadius = 7     // host memory: a negative radius (*where: the query)
};
// (radii: read only for a host-memory call that has passed every other check)
inline int hamming_range_validate(bool column, int64_t n_queries, int64_t cap, int mem, bool has_queries, bool has_radii,
                                  bool has_counts, bool has_idx, bool has_dist, const int32_t* radii, int64_t* where) {
    int64_t dummy;
    if (!where) where = &dummy;
    *where = 0;
    if (!column) return kHamRangeNoColumn;
    if (n_queries < 0 || n_queries > kHamMaxQueries) return kHamRangeBadCount;
    if (range_validate_cap((int)n_queries, cap)) return kHamRangeBadCap;
    if (mem != 0 && mem != 1) return kHamRangeBadMem;
    if (n_queries == 0) return kHamRangeOk;
    if (!has_queries || !has_radii || !has_counts) return kHamRangeNullPointer;
    if (cap > 0 && (!has_idx || !has_dist)) return kHamRangeNullLists;
    if (mem == 0)
        for (int64_t b = 0; b < n_queries; ++b)
            if (radii[b] < 0) {
                *where = b;
                return kHamRangeNegRadius;
            }
    return kHamRangeOk;
}

}  // namespace vdb
