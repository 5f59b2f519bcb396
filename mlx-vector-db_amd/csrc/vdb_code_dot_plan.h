// vdb_code_dot_plan.h — the host arithmetic of vdb_index_search_code_dot (vdb_api.cpp) and the decisions
// its two kernels share with it: int8 queries against the bit codes of the column vdb_index_set_codes
// attached, s(b, r) = sum_j q[b][j] * bit_j(code r), ranked by (s descending, row ascending).
//   the bit-plane form (vdb_code_dot.hip): the plane count rule, the plane layout in LDS, the block size;
//   the int8-MFMA form (vdb_code_dot_mfma.hip): the piece mapping of the query operand, the K chunk,
//   the LDS layout and the key encoding;
// and the limits, the validation (one enum value per cause), the scratch and the choice of form.
// The column's layout, the deal of tiles and the row side of the MFMA are vdb_hamming_plan.h's.
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/code_dot_plan_check.cpp).
#pragma once
#include <stdint.h>

#include "vdb_hamming_plan.h"

namespace vdb {

constexpr int kCdMaxPlanes = 8;               // bit planes of an int8 value
constexpr int32_t kCdBias = 1 << 20;          // |s| <= 8 192 * 128 = 2^20
constexpr int32_t kCdNoScore = INT32_MIN;     // the score of a slot past the candidates (-1 is a real score)
static_assert(kHamMaxBytes * 8 * 128 == kCdBias, "the largest |s| is the bias of the key");

// ---- the bit-plane form -----------------------------------------------------------------------------
// Two's complement: v = -2^(m-1) v_(m-1) + sum_{p < m-1} 2^p v_p for every v that fits m bits, so with
// P_p the plane of bit p of a query over all dimensions, s = sum_{p < m-1} 2^p popcount(x & P_p) -
// 2^(m-1) popcount(x & P_(m-1)).  (The planes above m - 1 equal the sign plane and telescope away.)
// The fewest bits that hold v: 1 for 0 and -1, 4 for [-8, 7], 8 for -128.
VDB_HAM_HD inline int cd_bits_needed(int8_t v) {
    uint32_t u = (uint32_t)(uint8_t)(v < 0 ? ~v : v);  // the magnitude bits below the sign
    int n = 1;
    while (u) {
        ++n;
        u >>= 1;
    }
    return n;
}
// The same for eight values at once (byte i of v8): a fold of each byte by its sign, one OR.
VDB_HAM_HD inline int cd_bits_needed8(uint64_t v8) {
    const uint64_t sign = (v8 >> 7) & 0x0101010101010101ull;
    uint64_t f = v8 ^ (sign * 0xFFull);
    f |= f >> 32;
    f |= f >> 16;
    f |= f >> 8;
    uint32_t u = (uint32_t)(f & 0x7Full);
    int n = 1;
    while (u) {
        ++n;
        u >>= 1;
    }
    return n;
}
// Bit p of each of eight values (byte i of v8) as one byte, value i to bit i: the byte of plane p
// that pairs with one code byte.
VDB_HAM_HD inline uint32_t cd_plane_byte(uint64_t v8, int p) {
    uint32_t b = 0;
    for (int i = 0; i < 8; ++i) b |= (uint32_t)((v8 >> (8 * i + p)) & 1ull) << i;
    return b;
}
// The weight of plane p of m.
VDB_HAM_HD inline int32_t cd_plane_weight(int p, int m) { return p == m - 1 ? -(1 << p) : (1 << p); }
// A block's planes in LDS: [query][kCdMaxPlanes][WS] 64-bit words, WS = ham_query_stride(W) (whole
// register passes, the pad zero).  A wave reads "word w of plane p of query q": one address for all
// its lanes, a broadcast.  Then, as the popcount search, one WaveTopK buffer per (wave, query), whose
// place the tail merge's buffer takes.
constexpr int64_t kCdStaticLds = 64;  // the kernel's static words (the plane count, the last-workgroup flag)
VDB_HAM_HD inline int64_t cd_plane_lds(int qb, int W) { return (int64_t)qb * kCdMaxPlanes * ham_query_stride(W) * 8; }
VDB_HAM_HD inline int64_t cd_plane_byte_off(int q, int p, int W) {
    return ((int64_t)q * kCdMaxPlanes + p) * ham_query_stride(W) * 8;
}
VDB_HAM_HD inline int64_t cd_lds_bytes(int qb, int W, int KE, bool merge) {
    const int64_t tk = ham_topk_lds(qb, KE), mg = merge ? ham_merge_lds(KE) : 0;
    return cd_plane_lds(qb, W) + (tk > mg ? tk : mg);
}
VDB_HAM_HD inline int64_t cd_lds_key_off(int wv, int q, int qb, int W, int KE) {
    return cd_plane_lds(qb, W) + ((int64_t)wv * qb + q) * ham_cap(KE) * 4;
}
VDB_HAM_HD inline int64_t cd_lds_row_off(int wv, int q, int qb, int W, int KE) {
    return cd_plane_lds(qb, W) + (int64_t)kHamWaves * qb * ham_cap(KE) * 4 + ((int64_t)wv * qb + q) * ham_cap(KE) * 4;
}
// QB: the largest power of two <= kCdMaxQB for which kHamWgPerCuLds workgroups of this width fit the
// LDS limit, the merge buffer and the static words included.  A query is eight planes, so up to k = 64
// it is 8 for codes of at most 80 words and 4 at the longest; 1 from k = 257 at the longest.  (16 never
// fits: its top-k buffers alone are half the limit.)
constexpr int kCdMaxQB = 8;
VDB_HAM_HD inline int cd_qb(int k, int W) {
    const int KE = ham_ke(k);
    int qb = kCdMaxQB;
    while (qb > 1 && kHamWgPerCuLds * (cd_lds_bytes(qb, W, KE, true) + kCdStaticLds) > kHamLdsLimit) qb >>= 1;
    return qb;
}
VDB_HAM_HD inline int cd_block(int k, int W, int n_queries) {
    const int qb = cd_qb(k, W);
    int p = 1;
    while (p < n_queries && p < qb) p <<= 1;
    return p;
}

// ---- the int8-MFMA form -----------------------------------------------------------------------------
// Rows go in as vdb_hamming_plan.h maps them (ham_mfma_slot: code bit b to MFMA step, lane half, byte).
// Lane l of step s then needs, of query l % 32, the int8 values of the 16 dimensions from 64 *
// ham_mfma_word(s, l / 32) + ham_mfma_shift(s) up: piece cd_mfma_piece(s, l / 32) of the row-major
// query, 16 aligned bytes that go into the operand as they are.
constexpr int kCdPieceBytes = 16;
constexpr int kCdPiecesPerPair = 8;  // a word pair is 128 dimensions
VDB_HAM_HD inline int cd_mfma_piece(int step, int half) { return 4 * ham_mfma_word(step, half) + step % 4; }
VDB_HAM_HD inline int cd_mfma_pairs(int W) { return ham_mfma_words(W) / 2; }
// LDS: the pieces of a K chunk piece-major, [piece][kHamMfmaQB queries][16 B] (the 32 lanes of a half
// read 512 consecutive bytes), then the candidate buffers, thresholds and counts of the Hamming form.
constexpr int64_t kCdPairLds = (int64_t)kCdPiecesPerPair * kHamMfmaQB * kCdPieceBytes;
constexpr int64_t kCdMfmaTopkLds = (int64_t)kHamMfmaQB * kHamMfmaCap * 8 + (int64_t)kHamMfmaQB * 8 + (int64_t)kHamMfmaQB * 4;
// The K chunk: the most word pairs whose pieces fit beside them.  A code of at most that many pairs is
// staged once per workgroup; a longer one chunk by chunk, every trip.
constexpr int kCdMfmaChunkPairs = (int)((kHamLdsLimit - kHamMfmaStaticLds - kCdMfmaTopkLds) / kCdPairLds);
static_assert(kCdMfmaChunkPairs >= 1, "a word pair fits");
constexpr int kCdMfmaChunkBytes = kCdMfmaChunkPairs * 16;  // the widest code of one chunk
VDB_HAM_HD inline int cd_mfma_lds_pairs(int W) {
    const int p = cd_mfma_pairs(W);
    return p < kCdMfmaChunkPairs ? p : kCdMfmaChunkPairs;
}
VDB_HAM_HD inline int cd_mfma_k_chunks(int W) { return (cd_mfma_pairs(W) + kCdMfmaChunkPairs - 1) / kCdMfmaChunkPairs; }
VDB_HAM_HD inline int64_t cd_mfma_piece_off(int local_piece, int q) {
    return ((int64_t)local_piece * kHamMfmaQB + q) * kCdPieceBytes;
}
VDB_HAM_HD inline int64_t cd_mfma_cand_off(int W) { return (int64_t)cd_mfma_lds_pairs(W) * kCdPairLds; }
VDB_HAM_HD inline int64_t cd_mfma_thr_off(int W) { return cd_mfma_cand_off(W) + (int64_t)kHamMfmaQB * kHamMfmaCap * 8; }
VDB_HAM_HD inline int64_t cd_mfma_cnt_off(int W) { return cd_mfma_thr_off(W) + (int64_t)kHamMfmaQB * 8; }
VDB_HAM_HD inline int64_t cd_mfma_lds_bytes(int W) { return cd_mfma_cnt_off(W) + (int64_t)kHamMfmaQB * 4; }
// The key of a candidate: one unsigned compare ranks (s descending, row ascending).
VDB_HAM_HD inline uint32_t cd_key_hi(int32_t s) { return (uint32_t)(kCdBias - s); }
VDB_HAM_HD inline int32_t cd_score_of_key_hi(uint32_t hi) { return kCdBias - (int32_t)hi; }
VDB_HAM_HD inline uint64_t cd_key(int32_t s, uint32_t row) { return ((uint64_t)cd_key_hi(s) << 32) | row; }

// ---- the form ---------------------------------------------------------------------------------------
// knob ("code_dot_mfma"): 0 = by the batch size, 1 = the MFMA form whenever the call is eligible (k <=
// kHamMfmaMaxK), 2 = never.  The auto threshold is measured: at 16 queries the MFMA
// form was 2.9 to 4 times the faster at every code width measured, at one query the plane form 1.7 to 2.2
// times; batches of 2 to 15 were not measured and stay with the plane form.
constexpr int kCdMfmaMinQueries = 16;
VDB_HAM_HD inline bool code_dot_knob_ok(int64_t knob) { return knob >= 0 && knob <= 2; }
VDB_HAM_HD inline bool code_dot_use_mfma(int64_t knob, int n_queries, int k, int n_bytes) {
    if (knob == 2 || k < 1 || k > kHamMfmaMaxK || n_bytes < 1 || n_bytes > kHamMaxBytes || n_queries < 1) return false;
    return knob == 1 || n_queries >= kCdMfmaMinQueries;
}

// ---- scratch and validation -------------------------------------------------------------------------
// The Hamming search's layout with queries of 8 * n_bytes bytes: block counters, the segments' lists
// as fp32 keys and uint32 rows, the merged lists, and a host call's staged arguments and results.
inline HammingScratch code_dot_scratch(int n_queries, int n_bytes, int k, int qb, int n_seg, int64_t rows, bool host,
                                       bool masked) {
    return hamming_scratch(n_queries, 8 * n_bytes, k, qb, n_seg, rows, host, masked);
}
enum {
    kCdOk = 0,
    kCdBadCount = 1,     // n_queries outside [0, kHamMaxQueries]
    kCdBadK = 2,         // k outside [1, kHamMaxK]
    kCdBadMem = 3,       // a memory kind that is neither host (0) nor device (1)
    kCdNullPointer = 4,  // queries / out_scores / out_indices NULL with n_queries > 0
    kCdNoColumn = 5      // no code column attached (or one that does not cover the rows)
};
inline int code_dot_validate_call(int64_t n_queries, int k, bool has_queries, bool has_scores, bool has_idx, int mem,
                                  bool column) {
    if (n_queries < 0 || n_queries > kHamMaxQueries) return kCdBadCount;
    if (k < 1 || k > kHamMaxK) return kCdBadK;
    if (mem != 0 && mem != 1) return kCdBadMem;
    if (n_queries > 0 && (!has_queries || !has_scores || !has_idx)) return kCdNullPointer;
    if (!column) return kCdNoColumn;
    return kCdOk;
}

}  // namespace vdb
