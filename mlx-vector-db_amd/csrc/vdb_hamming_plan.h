// vdb_hamming_plan.h — the host arithmetic of vdb_index_set_codes and vdb_index_search_hamming
// (vdb_api.cpp) and the decisions their kernels share with it (vdb_hamming.hip): the limits, the
// tiled layout of the code column, the query-block size QB, how the tiles are dealt to workgroups
// and waves, the LDS layout, the per-call scratch and the validation (one enum value per cause); and
// for the integer-MFMA form of the search (vdb_hamming_mfma.hip): its bit-to-operand mapping, block
// size, k limit, LDS layout and the choice between the two forms (ham_use_mfma).
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/hamming_plan_check.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_HAM_HD __host__ __device__
#else
#define VDB_HAM_HD
#endif

namespace vdb {

// A workgroup is 4 waves; one lane takes one row, so a wave scores one tile of 64 rows per trip and
// a chunk, the rows one workgroup handles per trip, is 4 tiles: wave w takes tile 4 c + w.
constexpr int kHamWaves = 4;
constexpr int kHamTileRows = 64;
constexpr int kHamChunkTiles = kHamWaves;
constexpr int kHamMaxBytes = 1024;               // a code: 1..1024 bytes (8..8192 bits)
constexpr int kHamMaxWords = kHamMaxBytes / 8;   // 64-bit words of the longest code
constexpr int kHamPassWords = 16;                // words of its row a lane holds in registers at once
constexpr int kHamMaxK = 1024;
constexpr int kHamMaxQueries = 65535;            // the grid's y extent, in queries
constexpr int kHamMaxQB = 16;                    // most queries a workgroup scores per code read
// Most workgroups per query block (the tail merge's list heads, vdb_merge_block.h MERGE_HEADS).
constexpr int kHamMaxSeg = 512;
// LDS of a CU, and the workgroups QB leaves room for on one (two: a workgroup is one wave per SIMD,
// and a second one covers the first's load latency and its top-k compactions).
constexpr int64_t kHamLdsLimit = 160 * 1024;
constexpr int kHamWgPerCuLds = 2;
// Workgroups the auto grid aims for per CU: what is resident at once.  Measured: with
// 4 blocks of 16 queries, 128 segments per block (2 per CU in all) took 1.81 ms on 1M x 1 024 bits,
// 256 segments 2.95 ms.
constexpr int kHamWgPerCu = 2;
constexpr int kHamMergeBuf = 1024;               // vdb_merge_block.h MERGE_BUF (checked at the launch)

// ---- the column's layout --------------------------------------------------------------------------
// Row-major bytes [n][n_bytes] are repacked into tiles of 64 rows, word-major inside a tile:
// [n_tiles][W][64] 64-bit words, W = ceil(n_bytes / 8); byte j of a row is bits [8 (j % 8), 8 (j % 8)
// + 8) of its word j / 8.  Pad bytes of the last word and pad rows of the last tile are zero.
VDB_HAM_HD inline int ham_words(int n_bytes) { return (n_bytes + 7) / 8; }
VDB_HAM_HD inline int64_t ham_n_tiles(int64_t N) { return N <= 0 ? 0 : (N + kHamTileRows - 1) / kHamTileRows; }
VDB_HAM_HD inline int64_t ham_packed_words(int64_t N, int W) { return ham_n_tiles(N) * W * kHamTileRows; }
// The packed word that holds word w of row r.
VDB_HAM_HD inline int64_t ham_word_index(int64_t r, int w, int W) {
    return ((r / kHamTileRows) * W + w) * kHamTileRows + (r % kHamTileRows);
}
// Word w of a row given as bytes (the pack kernel's and the query load's rule).
VDB_HAM_HD inline uint64_t ham_word_of(const uint8_t* row, int n_bytes, int w) {
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) {
        const int j = 8 * w + i;
        if (j < n_bytes) v |= (uint64_t)row[j] << (8 * i);
    }
    return v;
}

// ---- top-k widths and LDS -------------------------------------------------------------------------
VDB_HAM_HD inline int ham_ke(int k) {  // the top-k width: max(32, next_pow2(k)), as the exact scan's
    int p = 32;
    while (p < k) p <<= 1;
    return p;
}
VDB_HAM_HD inline int ham_cap(int KE) {  // WaveTopK<>::capacity(KE) (checked at the launch)
    const int need = 2 * KE > KE + 64 ? 2 * KE : KE + 64;
    int p = 1;
    while (p < need) p <<= 1;
    return p;
}
// A query's words in LDS: W rounded up to whole register passes, the pad words zero, so the inner
// loop reads a full pass without a guard.
VDB_HAM_HD inline int ham_query_stride(int W) { return (W + kHamPassWords - 1) / kHamPassWords * kHamPassWords; }
// The tail merge's buffer (merge_block_lds<float, uint32_t>(KE)).
VDB_HAM_HD inline int64_t ham_merge_lds(int KE) {
    const int c = ham_cap(KE) > kHamMergeBuf ? ham_cap(KE) : kHamMergeBuf;
    return (int64_t)c * 8;
}
// LDS of one workgroup: qb queries of W words, then per (wave, query) one WaveTopK buffer of fp32
// keys and uint32 rows; the tail merge's buffer takes the top-k buffers' place.
VDB_HAM_HD inline int64_t ham_query_lds(int qb, int W) { return (int64_t)qb * ham_query_stride(W) * 8; }
VDB_HAM_HD inline int64_t ham_topk_lds(int qb, int KE) { return (int64_t)kHamWaves * qb * ham_cap(KE) * 8; }
VDB_HAM_HD inline int64_t ham_lds_bytes(int qb, int W, int KE, bool merge) {
    const int64_t tk = ham_topk_lds(qb, KE), mg = merge ? ham_merge_lds(KE) : 0;
    return ham_query_lds(qb, W) + (tk > mg ? tk : mg);
}
// QB: the largest power of two <= kHamMaxQB for which kHamWgPerCuLds workgroups of the longest code
// fit the LDS limit, the merge buffer included.  16 up to k = 64, 8 to 128, 4 to 256, 2 to 512, 1 above.
VDB_HAM_HD inline int ham_qb(int k) {
    const int KE = ham_ke(k);
    int qb = kHamMaxQB;
    while (qb > 1 && kHamWgPerCuLds * ham_lds_bytes(qb, kHamMaxWords, KE, true) > kHamLdsLimit) qb >>= 1;
    return qb;
}
// The block a launch uses: QB, or the power of two that covers a smaller batch (a batch of one does
// not pay for sixteen).
VDB_HAM_HD inline int ham_block(int k, int n_queries) {
    const int qb = ham_qb(k);
    int p = 1;
    while (p < n_queries && p < qb) p <<= 1;
    return p;
}
VDB_HAM_HD inline int ham_n_blocks(int n_queries, int qb) { return (n_queries + qb - 1) / qb; }
// LDS offsets of the launch (bytes): the query words of block query q, and the key / row buffers of
// (wave, q): keys [waves][qb][cap] fp32 then rows [waves][qb][cap] uint32, both after the queries.
VDB_HAM_HD inline int64_t ham_lds_query_off(int q, int W) { return (int64_t)q * ham_query_stride(W) * 8; }
VDB_HAM_HD inline int64_t ham_lds_key_off(int wv, int q, int qb, int W, int KE) {
    return ham_query_lds(qb, W) + ((int64_t)wv * qb + q) * ham_cap(KE) * 4;
}
VDB_HAM_HD inline int64_t ham_lds_row_off(int wv, int q, int qb, int W, int KE) {
    return ham_query_lds(qb, W) + (int64_t)kHamWaves * qb * ham_cap(KE) * 4 + ((int64_t)wv * qb + q) * ham_cap(KE) * 4;
}

// ---- the deal of tiles ------------------------------------------------------------------------------
// Chunks of N rows, and the segments of a query block that have any: segment s walks chunks s, s +
// n_seg, ..., so segments at or past the chunk count have nothing to do.
VDB_HAM_HD inline int64_t ham_n_chunks(int64_t N) { return (ham_n_tiles(N) + kHamChunkTiles - 1) / kHamChunkTiles; }
VDB_HAM_HD inline int ham_live_segs(int64_t N, int n_seg) {
    const int64_t c = ham_n_chunks(N);
    return c < n_seg ? (int)c : n_seg;
}
// The tile wave wv takes in chunk c (at or past ham_n_tiles(N): none).
VDB_HAM_HD inline int64_t ham_tile_of(int64_t c, int wv) { return c * kHamChunkTiles + wv; }
// Workgroups per query block.  knob ("hamming_wgs") > 0 forces it; 0 = auto: one per chunk, capped so
// that the grid is about kHamWgPerCu workgroups per CU.
inline int ham_n_seg(int64_t knob, int64_t N, int n_blocks, int n_cu) {
    if (knob > 0) return (int)(knob < kHamMaxSeg ? knob : kHamMaxSeg);
    int64_t chunks = ham_n_chunks(N);
    int64_t cap = ((int64_t)n_cu * kHamWgPerCu) / (n_blocks > 0 ? n_blocks : 1);
    if (cap < 1) cap = 1;
    if (chunks > cap) chunks = cap;
    if (chunks > kHamMaxSeg) chunks = kHamMaxSeg;
    return chunks < 1 ? 1 : (int)chunks;
}
// The mask words of a tile: rows [64 t, 64 t + 64) are bits of words 2 t and 2 t + 1; the second may
// lie past the mask's ceil(N / 32) words (it then counts as zero: its rows are past N).
VDB_HAM_HD inline int64_t ham_mask_words(int64_t N) { return (N + 31) / 32; }

// ---- the integer-MFMA form (vdb_hamming_mfma.hip) ---------------------------------------------------
// The same call, column and result through v_mfma_i32_32x32x32_i8: a stored bit x becomes the int8
// 0 / 1, a query bit q becomes -1 / +1, and dot = 2 (q.x) - |x|, so the distance is |q| - dot.  A
// workgroup (4 waves) takes a block of kHamMfmaQB queries (two MFMA query tiles); per trip wave w
// takes tile 4 c + w as two 32-row sub-tiles, as the popcount form deals them.
constexpr int kHamMfmaQT = 2;                        // query tiles of 32 per workgroup
constexpr int kHamMfmaQB = 32 * kHamMfmaQT;
constexpr int kHamMfmaMaxK = 64;
// A query's candidate buffer, shared by the four waves: kHamMfmaCap (distance, row) entries.  A wave
// offers at most 64 rows per query and trip, so after a compaction to k <= kHamMfmaMaxK entries one
// wave's offers always fit; above kHamMfmaHigh entries a buffer is compacted at the trip's end.
constexpr int kHamMfmaCap = 128;
constexpr int kHamMfmaHigh = 96;
static_assert(kHamMfmaMaxK + kHamTileRows <= kHamMfmaCap, "one wave's offers fit a compacted buffer");
// The smallest batch that takes this form by itself (knob "hamming_mfma" = 0).  Measured, DESIGN.md §24.
constexpr int kHamMfmaMinQueries = 64;

// The bit mapping.  One MFMA multiplies 32 code bits: lane half h supplies 16 bytes.  Code bit b (bit
// b % 64 of word b / 64) goes to MFMA step 4 (word / 2) + (b % 64) / 16, lane half word % 2, byte b % 16:
// lane l of step s reads word ham_mfma_word(s, l / 32) and expands its 16 bits from ham_mfma_shift(s)
// up, bit i to byte i.  The same function serves rows and queries; a dot product needs no more.
struct HamMfmaSlot { int step, half, byte; };
VDB_HAM_HD inline HamMfmaSlot ham_mfma_slot(int bit) {
    const int w = bit / 64, c = bit % 64;
    return HamMfmaSlot{4 * (w / 2) + c / 16, w % 2, c % 16};
}
VDB_HAM_HD inline int ham_mfma_word(int step, int half) { return 2 * (step / 4) + half; }
VDB_HAM_HD inline int ham_mfma_shift(int step) { return 16 * (step % 4); }
VDB_HAM_HD inline int ham_mfma_words(int W) { return (W + 1) / 2 * 2; }   // W up to a whole word pair (the odd one: zero)
VDB_HAM_HD inline int ham_mfma_steps(int W) { return 2 * ham_mfma_words(W); }
// Four bits to the four bytes of an operand register: a row's 0 / 1 (the products of the multiply do
// not overlap: bit i lands on bit 8 i) and a query's -1 / +1.
VDB_HAM_HD inline uint32_t ham_mfma_row4(uint32_t nib) { return ((nib & 15u) * 0x00204081u) & 0x01010101u; }
VDB_HAM_HD inline uint32_t ham_mfma_query4(uint32_t nib) {
    const uint32_t e = ham_mfma_row4(nib);
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0x000001FFu, 0x000001FFu, e);  // selector byte 0 -> 0xFF, 1 -> 0x01
#else
    const uint32_t ne = e ^ 0x01010101u;
    return e | ((ne << 8) - ne);
#endif
}
// LDS of a workgroup (bytes): the block's query words word-major [ham_mfma_words(W)][QB] (a lane's
// read of "word w of query l % 32" is conflict free), the candidate buffers [QB][cap] of 64-bit keys
// (distance << 32 | row), the thresholds [QB] and the counts [QB].  (The segments' lists are merged
// by a launch of its own, one workgroup per query, with the merge's buffer as its only LDS.)
VDB_HAM_HD inline int64_t ham_mfma_query_lds(int W) { return (int64_t)ham_mfma_words(W) * kHamMfmaQB * 8; }
VDB_HAM_HD inline int64_t ham_mfma_cand_off(int W) { return ham_mfma_query_lds(W); }
VDB_HAM_HD inline int64_t ham_mfma_thr_off(int W) { return ham_mfma_cand_off(W) + (int64_t)kHamMfmaQB * kHamMfmaCap * 8; }
VDB_HAM_HD inline int64_t ham_mfma_cnt_off(int W) { return ham_mfma_thr_off(W) + (int64_t)kHamMfmaQB * 8; }
VDB_HAM_HD inline int64_t ham_mfma_lds_bytes(int W) { return ham_mfma_cnt_off(W) + (int64_t)kHamMfmaQB * 4; }
// The kernel's static LDS (its flag words) on top of that: room kept under the limit.
constexpr int64_t kHamMfmaStaticLds = 256;
// The query block of this form for k, 0 = k is not served.  Every width fits with kHamMfmaQB:
// 64 KiB of queries at the longest code and 64 KiB of candidates.
VDB_HAM_HD inline int ham_mfma_qb(int k) {
    if (k < 1 || k > kHamMfmaMaxK) return 0;
    return ham_mfma_lds_bytes(kHamMaxWords) + kHamMfmaStaticLds <= kHamLdsLimit ? kHamMfmaQB : 0;
}
// Which form a call takes.  knob ("hamming_mfma"): 0 = by the batch size, 1 = this form whenever the
// call is eligible, 2 = never.  Every code width is eligible.
VDB_HAM_HD inline bool ham_use_mfma(int64_t knob, int n_queries, int k, int n_bytes) {
    if (knob == 2 || ham_mfma_qb(k) == 0 || n_bytes < 1 || n_bytes > kHamMaxBytes || n_queries < 1) return false;
    return knob == 1 || n_queries >= kHamMfmaMinQueries;
}

// ---- scratch ------------------------------------------------------------------------------------------
inline int64_t ham_align(int64_t b) { return (b + 255) / 256 * 256; }
struct HammingScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t done, lk, li, mk, mi;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, mask, in_bytes, out0, out_d, out_i, out_bytes;
    int64_t mask_words, total;
};
inline HammingScratch hamming_scratch(int n_queries, int n_bytes, int k, int qb, int n_seg, int64_t rows, bool host,
                                      bool masked) {
    HammingScratch s{};
    const int64_t B = n_queries, KE = ham_ke(k);
    s.mask_words = ham_mask_words(rows);
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += ham_align(bytes);
        return at;
    };
    s.done = take((int64_t)ham_n_blocks(n_queries, qb) * 4);
    s.lk = take(n_seg > 1 ? B * n_seg * KE * 4 : 0);
    s.li = take(n_seg > 1 ? B * n_seg * KE * 4 : 0);
    s.mk = take(n_seg > 1 ? B * KE * 4 : 0);
    s.mi = take(n_seg > 1 ? B * KE * 4 : 0);
    s.in0 = o;
    if (host) {
        s.q = take(B * n_bytes);
        s.mask = take(masked ? s.mask_words * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_d = take(B * k * 4);
        s.out_i = take(B * k * 8);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -----------------------------------------------------------------------------------------
enum {
    kHamColOk = 0,
    kHamColBadRows = 1,   // n != count, or a NULL column with n != 0
    kHamColBadWidth = 2   // n_bytes outside [1, kHamMaxBytes]
};
inline int hamming_column_args(bool has_codes, int64_t n, int n_bytes, int64_t count) {
    if (!has_codes) return n == 0 ? kHamColOk : kHamColBadRows;  // detach
    if (n != count) return kHamColBadRows;
    if (n_bytes < 1 || n_bytes > kHamMaxBytes) return kHamColBadWidth;
    return kHamColOk;
}
enum {
    kHamOk = 0,
    kHamBadCount = 1,     // n_queries outside [0, kHamMaxQueries]
    kHamBadK = 2,         // k outside [1, kHamMaxK]
    kHamBadMem = 3,       // a memory kind that is neither host (0) nor device (1)
    kHamNullPointer = 4,  // queries / out_distances / out_indices NULL with n_queries > 0
    kHamNoColumn = 5      // no code column attached (or one that does not cover the rows)
};
inline int hamming_validate_call(int64_t n_queries, int k, bool has_queries, bool has_dist, bool has_idx, int mem,
                                 bool column) {
    if (n_queries < 0 || n_queries > kHamMaxQueries) return kHamBadCount;
    if (k < 1 || k > kHamMaxK) return kHamBadK;
    if (mem != 0 && mem != 1) return kHamBadMem;
    if (n_queries > 0 && (!has_queries || !has_dist || !has_idx)) return kHamNullPointer;
    if (!column) return kHamNoColumn;
    return kHamOk;
}

}  // namespace vdb
