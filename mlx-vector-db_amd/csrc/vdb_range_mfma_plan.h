// vdb_range_mfma_plan.h — the arithmetic the fp32-MFMA form of the range scan (vdb_range_mfma.hip)
// shares with the host (vdb_api.cpp): tile sizes, the query block, the LDS layout, which form serves
// a call, and the decision of one (row, query) pair with its margin.  The margin is derived in
// DESIGN.md §14.1; the constants here are that derivation's.
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/range_mfma_plan_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>

#include "vdb_range_plan.h"

namespace vdb {

// ---- tiling ---------------------------------------------------------------------------------------
// A workgroup is 4 waves and owns the same chunk of kRangeWgWords bitmap words as the fp64 scan, so
// part [query][chunk] means the same to the prefix kernel.  Wave w owns words [4 w, 4 w + 4) and
// takes them in kRangeMfmaPasses passes of kRangeMfmaPassTiles 32-row tiles; a tile against 32
// queries is one 32x32 accumulator of v_mfma_f32_32x32x2_f32, rows on M and queries on N.  K runs in
// chunks of kRangeMfmaKC dims: a chunk of the wave's rows (one 128-byte line per row) and of the
// block's queries goes through LDS with rows padded to kRangeMfmaLdsStride floats, which makes the
// 16-byte operand reads of 16 lanes hit 64 distinct banks.
constexpr int kRangeMfmaWaves = kRangeWaves;
constexpr int kRangeMfmaTileRows = 32;
constexpr int kRangeMfmaPassTiles = 2;
constexpr int kRangeMfmaPasses = kRangeWaveWords / kRangeMfmaPassTiles;
constexpr int kRangeMfmaPassRows = kRangeMfmaTileRows * kRangeMfmaPassTiles;  // 64 rows per wave and pass
constexpr int kRangeMfmaQB = 64;       // queries per block at every dim: K is tiled
constexpr int kRangeMfmaKC = 32;       // dims per K chunk
constexpr int kRangeMfmaLdsStride = kRangeMfmaKC + 4;
constexpr int kRangeMfmaMaxDim = 65536;  // the margin's 1.01 covers gamma_n up to here (n u <= 0.0099)
static_assert(kRangeMfmaQB == kRangeMaxBlock, "one bitmap row per query of a block, as the fp64 scan");
static_assert(kRangeMfmaPasses * kRangeMfmaPassTiles == kRangeWaveWords, "a wave's words split into whole passes");
static_assert(kRangeMfmaLdsStride % 4 == 0, "16-byte operand reads stay aligned");

// LDS of a workgroup (float offsets / bytes): the waves' row chunks, the block's query chunk, the
// rows' norms per wave and the waves' per-query counts.
VDB_RANGE_HD inline int range_mfma_lds_x_floats() { return kRangeMfmaPassRows * kRangeMfmaLdsStride; }  // per wave
VDB_RANGE_HD inline int range_mfma_lds_q_floats() { return kRangeMfmaQB * kRangeMfmaLdsStride; }
VDB_RANGE_HD inline int64_t range_mfma_lds_bytes() {
    return (int64_t)kRangeMfmaWaves * range_mfma_lds_x_floats() * 4 + (int64_t)range_mfma_lds_q_floats() * 4 +
           (int64_t)kRangeMfmaWaves * kRangeMfmaPassRows * 8 + (int64_t)kRangeMfmaWaves * kRangeMfmaQB * 4;
}
constexpr int64_t kRangeMfmaLdsLimit = 64 * 1024;  // static LDS of one workgroup

// The load of a K chunk: instruction i of lane l brings 16 bytes of row i * 8 + l / 8 of the pass,
// floats [4 (l % 8), +4) of the chunk, so 8 lanes read one row's 128 contiguous bytes.
constexpr int kRangeMfmaXLoads = kRangeMfmaPassRows * kRangeMfmaKC / (64 * 4);  // 8 per lane and chunk
VDB_RANGE_HD inline int range_mfma_xload_row(int i, int lane) { return i * 8 + lane / 8; }
VDB_RANGE_HD inline int range_mfma_xload_col(int lane) { return (lane % 8) * 4; }
// ... and of the queries: element i * 256 + t of [kRangeMfmaQB][kRangeMfmaKC] to thread t.
constexpr int kRangeMfmaQLoads = kRangeMfmaQB * kRangeMfmaKC / 256;  // 8 per thread and chunk
// K steps of a chunk: lane half h of step s supplies floats [8 s + 4 h, +4) of its row / query to four
// MFMAs, one float each (both operands use the same map, so the K order they imply is shared).
constexpr int kRangeMfmaSteps = kRangeMfmaKC / 8;
VDB_RANGE_HD inline int range_mfma_operand_col(int step, int half) { return 8 * step + 4 * half; }
// Accumulator v (0..15) of lane half h of a 32x32 tile is row 8 (v / 4) + 4 h + v % 4 of the query
// lane % 32; the other 16 rows sit in lane ^ 32.
VDB_RANGE_HD inline int range_mfma_acc_row(int v, int half) { return 8 * (v / 4) + 4 * half + v % 4; }
VDB_RANGE_HD inline int range_mfma_k_chunks(int Dp) { return (Dp + kRangeMfmaKC - 1) / kRangeMfmaKC; }
// The first word of pass p of wave w of a chunk.
VDB_RANGE_HD inline int64_t range_mfma_pass_word(int64_t chunk, int wave, int pass) {
    return range_wave_word(chunk, wave, pass * kRangeMfmaPassTiles);
}

// ---- which form serves a call ---------------------------------------------------------------------
// knob ("range_mfma"): 0 = by the batch size, 1 = the MFMA form for every call, 2 = never.  Auto takes
// the MFMA form from kRangeMfmaMinQueries queries (0 = never by itself): the smallest measured batch
// at which it is not slower at either benchmark shape (tools/range_bench.py).
// Measured: it is not slower at any batch, 1 included (0.65 against 0.76 ms at 1M x 768, 0.19 against
// 0.32 ms at 1M x 128), so every eligible call takes it.
constexpr int kRangeMfmaMinQueries = 1;
VDB_RANGE_HD inline bool range_mfma_knob_ok(int64_t knob) { return knob >= 0 && knob <= 2; }
VDB_RANGE_HD inline bool range_use_mfma(int64_t knob, int n_queries, int dim) {
    if (knob == 2 || n_queries < 1 || dim < 1 || dim > kRangeMfmaMaxDim) return false;
    return knob == 1 || (kRangeMfmaMinQueries > 0 && n_queries >= kRangeMfmaMinQueries);
}
VDB_RANGE_HD inline int range_mfma_block(int n_queries) {
    return n_queries < 1 ? 1 : n_queries > kRangeMfmaQB ? kRangeMfmaQB : n_queries;
}

// ---- the decision of one pair ---------------------------------------------------------------------
// a: the fp32 MFMA dot product of row and query (any summation order).  With S the real dot product
// and qn, xn the canonical fp64 norms,  |a - S| <= crel qn xn + cabs (1 + qn + xn)  whenever a is
// finite and qn xn <= 2^126: crel = 2.02 (D + 8) 2^-24 is twice the round-to-nearest bound (so it also holds for an
// accumulator that truncates) plus (D + 8) 2^-50 for the canonical fp64 sum against S; cabs =
// (D + 8) 2^-124 covers operands, products and partial sums that are flushed to zero or rounded as
// denormals.  kRangeMfmaSlack64 covers the fp64 roundings of bound x norm product and of the
// division; c64 those of the norms, their squares and the canonical sum of squares.
constexpr double kRangeMfmaSlack64 = 0x1p-48;
VDB_RANGE_HD inline double range_mfma_crel(int D) { return 2.02 * (double)(D + 8) * 0x1p-24 + (double)(D + 8) * 0x1p-50; }
VDB_RANGE_HD inline double range_mfma_cabs(int D) { return (double)(D + 8) * 0x1p-124; }
VDB_RANGE_HD inline double range_mfma_c64(int D) { return (double)(D + 8) * 0x1p-48; }
enum { kRangeMfmaMiss = 0, kRangeMfmaHit = 1, kRangeMfmaExact = 2 };
// kt: the key bound (range_kt).  Hit and miss are certain for the canonical key; everything else,
// a NaN or an infinity among it (either test is false for a NaN), takes the exact path.
VDB_RANGE_HD inline int range_mfma_decide(int metric, float af, double kt, double qn, double xn, int D) {
    if (kt != kt) return kRangeMfmaMiss;  // a NaN bound: no key is at or above it
    const double a = (double)af;
    // fp32 overflow: nothing is known.  No partial sum passes qn xn in magnitude, so below 2^126 none
    // overflowed, whether an overflow would have shown as an infinity or as a saturated finite value.
    if (!(fabs(a) <= 3.4028234663852886e38) || !(qn * xn <= 0x1p126)) return kRangeMfmaExact;
    const double dot = range_mfma_crel(D) * qn * xn + range_mfma_cabs(D) * (1.0 + qn + xn);
    double have, want, e;
    if (metric == 0) {  // key = acc / (qn' xn') >= kt  <=>  acc >= kt qn' xn' up to the roundings
        have = a;
        want = kt * (fmax(qn, 1e-8) * fmax(xn, 1e-8));
        e = dot + fabs(want) * kRangeMfmaSlack64;
    } else {  // key = -sum (x - q)^2 >= kt  <=>  -kt >= sum, the sum about xn^2 + qn^2 - 2 a
        const double nn = xn * xn + qn * qn;
        have = -kt;
        want = nn - 2.0 * a;
        e = 2.0 * dot + range_mfma_c64(D) * nn;
    }
    if (have - want >= e) return kRangeMfmaHit;
    if (want - have >= e) return kRangeMfmaMiss;
    return kRangeMfmaExact;
}

// ---- scratch ------------------------------------------------------------------------------------
// The layout of range_scratch with this form's own block: H, part and cnt hold range_mfma_block
// queries whatever the dim.
inline RangeScratch range_mfma_scratch(int n_queries, int dim, int64_t N, int64_t cap, bool host, bool has_mask,
                                       bool keys) {
    return range_scratch_block(n_queries, dim, range_mfma_block(n_queries), N, cap, host, has_mask, keys);
}

}  // namespace vdb
