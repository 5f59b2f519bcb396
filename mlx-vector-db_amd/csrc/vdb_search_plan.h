// vdb_search_plan.h — the host arithmetic of the main search (search_locked / run_exact in
// vdb_api.cpp): the candidate count KP and its margin rules, which candidate pass a batch takes and
// its launch geometry, the pilot's sample and rank, and the workspace layouts (the only place a
// buffer's size and offset are written down).  The stateful precision policy (VDB_PREC_AUTO's holds
// and re-pass bookkeeping) stays in the driver and yields a PREC_*; from there on everything here is
// a pure function of plain values.  What the kernels decide themselves (which shapes a pass is
// built for, rows per step) the driver evaluates and hands in as SearchKernelFacts: this header
// never calls into a .hip file.
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/search_plan_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace vdb {

// Candidate-pass arithmetic (vdb.h VDB_PREC_*):
//   PREC_FP32   fp32 corpus tiles, v_mfma_f32_32x32x2_f32 (8-dim groups, 4 KiB per super-tile group)
//   PREC_BF16X3 split-bf16 corpus (x = hi + lo + O(2^-16 x)), three v_mfma_f32_32x32x16_bf16 per
//               16-dim group: hi*hi + hi*lo + lo*hi (8 KiB per super-tile group: [plane][sub tile])
constexpr int PREC_FP32 = 0;
constexpr int PREC_BF16X3 = 1;
//   PREC_BF16   the hi plane of the split copy only (x ~ bf16(x), half the bytes), query split:
//               x.q ~ xh.qh + xh.ql, two v_mfma_f32_32x32x16_bf16 per 16-dim group; bounded by the
//               index's largest row residual |x - bf16(x)| (pack_rows)
constexpr int PREC_BF16 = 2;
//   PREC_I8     int8 copy of the centred rows (vdb_scan8_kernel.h): x ~ s_x xh (1 byte per element),
//               query s_q qh (8 bits): one v_mfma_i32_32x32x32_i8 per 32-dim group
//   PREC_I8X3   both planes of the int8 copy, x ~ s_x (xh + xl/256), query 16 bits: three per group
//   PREC_I8Q    the xh plane (8 bits, 1 byte per element) against the 16-bit query: xh.qh + xh.ql /
//               256, two per group (L2, 16 < k <= 100: C4)
constexpr int PREC_I8 = 3;
constexpr int PREC_I8X3 = 4;
constexpr int PREC_I8Q = 5;
constexpr int N_PREC = 6;
inline bool prec_is_i8(int p) { return p == PREC_I8 || p == PREC_I8X3 || p == PREC_I8Q; }

constexpr int QG_EXTRA = 8;        // duplicated leading dim-groups at the end of each query tile
// the wide int8 pass (vdb_scan8w.hip): W8_CH slots per (workgroup, query) segment of the candidate lists
constexpr int W8_CH = 32;
// gthr[B]: per-query shared threshold (order-preserving score key, 0 = none) and
// gslots[B][KP_MAX]: per-query slots of published workgroup bests; both zeroed by
// prep_queries (see the publish step of scan_topk_kernel).
constexpr int KP_MAX = 256;
constexpr int PILOT_SLOTS = 256;  // pilot bound slots per query
constexpr int kMaxApproxK = 200;  // k above this uses the exact path
// Device-memory searches (device_repass): up to this many uncertified queries of a batch are
// gathered into a gated BF16X3 sub-search on the device (more go to the exact path)
constexpr int kRepassDev = 16;
// auto's I8 pass: KP = 128 up to this many rows (i8_narrow)
constexpr int64_t kI8NarrowRows = 512 * 1024;
constexpr int64_t kI8NarrowRowsShort = 4 * 1024 * 1024;  // rows of <= 128 dims
// the wide int8 pass under scan_wide auto: from this many rows (smaller indexes: the 64-query shape)
constexpr int64_t kWideMinRows = 65536;
// ... and, for batches of <= 256 (a 64-query block's stage tiles split over 2..8 waves), up to this
// many rows: the c6 shard of an 8-way run (1.25M x 128, B = 64) 1.03 -> 1.25 M QPS per rank, scan
// 60 -> 40 us; at 10M rows the scan is faster (0.218 -> 0.206 ms) but the three-stream step slower
// (0.235 -> 0.245: its 134 KiB of LDS leave no room for the other streams' side kernels),
// profiles/r06_c6w2
constexpr int64_t kWideSplitMaxRows = 2500000;
// the finish holds every segment's entries: at most FIN_CAP (16 K) / W8_CH segments
constexpr int FIN_SEG_MAX = 512;
// i8_refine auto: the finish refines I8 candidates' scores for padded rows of this many dims or more
constexpr int64_t kRefineMinDp = 512;
// query slots of the device-gated exact scan (each loops over the flagged queries)
constexpr int kGateSlots = 4;

inline int64_t plan_round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
inline int plan_next_pow2(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline int64_t plan_align(int64_t b) { return (b + 255) / 256 * 256; }

// ---- inputs ---------------------------------------------------------------------------------------
// One search call, after the precision policy: the batch, the index's shape and the pass it runs.
struct SearchShape {
    int B, k;            // queries, results per query
    int D, Dp, G;        // dims, padded dims, 8-dim groups (Dp / 8)
    int metric;          // 0 cosine, 1 euclidean
    int64_t N;           // rows
    int n_cu;
    int prec;            // PREC_*
    bool host;           // a host-memory call (the queries, mask and results staged in the workspace)
    bool gated;          // a device re-pass's sub-search: its query count lives on the device
    bool repass;         // a re-pass sub-search (host or device)
};
// The index's knobs as vdb_index_set_param leaves them, and which optional copies it keeps.
struct SearchKnobs {
    bool force_exact;
    int64_t margin;               // < 0: the default rules
    bool i8_narrow;               // the policy allows KP = 128 for auto's I8 pass (not yet widened)
    int64_t scan_q4, scan_wide;   // -1 auto, 0 off, 1 on
    int64_t n_wg_override;        // > 0: workgroups of the candidate pass
    int64_t scan_variant;         // fp32 pass
    int64_t scan_sync;            // 0 auto, 1 lockstep, 2 flag-gated
    int64_t finish_split;
    int64_t i8_refine;            // -1 auto, 0 off, 1 on
    int64_t scan_checksum;        // 0 off, 1 H sums, 2 L sums too
    int64_t pilot_tiles;          // < 0: by k
    int64_t pilot_rank_override;  // > 0: the pilot bound's rank
    bool has_xh;                  // the row-major xh plane is kept (the finish's I8 refinement)
    bool has_csum;                // the int8 copy's column sums are kept (the checksum)
};
// What the kernels' translation units answer for this call (the driver asks them).
struct SearchKernelFacts {
    bool scan8wl_ok;       // scan8wl_ok(prec, metric, Gs, B)
    bool scan8w_ok;        // scan8w_ok(Gs, B)
    bool scan_variant_ok;  // scan_variant_ok(prec, scan_variant, Gs)
    int rows_per_step;     // the pass's own: scan8_ / scan2_ / scan_rows_per_step (the fp32 pass: of the
                           // variant it runs, variant 0 where scan_variant_ok is false)
    int rows_per_step_q4;  // scan2_rows_per_step(true)
    bool scan_priv;        // scan_priv(prec, variant, KP), the variant as above
};

// scan groups of a pass: 8 (fp32), 32 (int8) or 16 (split) dims each
inline int search_groups(int prec, int G) { return prec == PREC_FP32 ? G : prec_is_i8(prec) ? G / 4 : G / 2; }

// ---- KP -------------------------------------------------------------------------------------------
struct SearchKP {
    int KP;
    bool exact_all;  // the whole batch takes the exact path
};
// candidates beyond k: the certificate needs a gap of 2 eps between the k-th and the
// KP-th approximate score; bf16x3's bound grows with D (3D additions), so large D
// gets a wider margin (1M x 1536 uniform: KP = 32 left ~1.5% of queries uncertified)
inline SearchKP search_kp(const SearchShape& s, const SearchKnobs& kn) {
    const int k = s.k, prec = s.prec;
    // the "one plane" precisions (a wide certificate: KP = 128 for small k) and their re-pass
    const bool one_plane = prec == PREC_BF16 || prec == PREC_I8;
    int margin_def = std::max(16, k / 4);
    if ((prec == PREC_BF16X3 || prec == PREC_I8X3) && s.D >= 1024) margin_def = std::max(margin_def, 48);
    // bf16 (hi plane only): eps ~ the rows' bf16 residual (~1.5e-3 relative on uniform data),
    // ~30x bf16x3's: 1M x 768 uniform needs KP = 128 for k = 10 (KP = 64 left 26% of the
    // queries uncertified; KP = 128: none of 2560)
    if (one_plane) margin_def = std::max(16, std::min(std::max(112, k / 2), 256 - k));
    // I8 (the 8-bit query's wider bound): KP = 256.  1M x 768 uniform, B = 64: KP = 128 left one
    // query per batch uncertified; 256 none (profiles/r03_i8/c2_i8_kp*)
    // -- except auto on small indexes (i8_narrow): at <= 512 K rows KP = 128 (one rank of an 8-way
    // weak-scaled C2, 125 K rows x 512 queries: step 0.248 -> 0.207 ms, 0 fallbacks; 250 K: 0.181 ->
    // 0.157; KP = 64 failed thousands of queries, profiles/r04_ab/rank*), widened for good at the
    // first flagged query
    // Rows of <= 128 dims (C6's 10M x 128): 0 fallbacks at KP = 128 even at 10 M rows, faster up to
    // the 4-way shard (8-way 1.25 M x 512: 1.38 -> 1.56 M QPS; 4-way 2.5 M x 256: +4%) and slower
    // at 10 M (262 -> 248 K: the KP = 128 scan's 106 KiB of LDS leaves no room beside it for the
    // next batch's pilot, profiles/r04_ab/rank6m, c6m), hence 4 M
    const bool i8_narrow = kn.i8_narrow && (s.N <= kI8NarrowRows || (s.Dp <= 128 && s.N <= kI8NarrowRowsShort));
    if (prec == PREC_I8) margin_def = std::max(16, (i8_narrow ? 128 : 256) - k);
    // I8Q (the 8-bit corpus's bound, as I8's): KP = 256
    if (prec == PREC_I8Q) margin_def = std::max(16, 256 - k);
    // a re-pass sub-search (host or device) takes KP = 128: its few queries are the ones whose
    // rows sit closer together than the one-plane pass could separate, so they need the wider
    // gap between the k-th and the KP-th candidate (C2 with 300 rows in a 3e-3 cosine band:
    // BF16X3 at KP = 32 left every such query to the exact scan)
    if (s.repass) margin_def = std::max(margin_def, 128 - k);
    const int margin = kn.margin >= 0 ? (int)kn.margin : margin_def;
    SearchKP r;
    r.KP = std::max(32, plan_next_pow2(k + margin));
    r.exact_all = kn.force_exact || k > kMaxApproxK || r.KP > 256;
    if (r.KP > 256) r.KP = 256;
    return r;
}

// ---- geometry -------------------------------------------------------------------------------------
struct SearchGeometry {
    int Gs;             // scan groups (search_groups)
    bool i8_pass, split_pass;
    bool q4;            // the split pass's 128-query shape
    bool wide_long;     // the wide int8 pass's long-row form
    bool wide8;         // the wide int8 pass (either form)
    int n_seg8;         // its row segments (workgroups)
    int QB, QB_pilot;   // query rows per block of the candidate pass / the pilot
    int Bp;             // B in whole query super tiles
    int n_qblocks;
    int variant;        // fp32 pass
    int64_t step_rows, n_steps;
    int n_wg, spw;      // workgroups per query block, steps per workgroup
    int64_t mask_words;
    int lockstep;
    int n_wg8;          // checksum partials per query
    int64_t gl_cap;     // entries per query of the global candidate lists
    bool priv;          // the fp32 pass's wave-private form
    bool rs8_on;        // int8 L2 pass: per-batch integer start values
    bool i8_refine;     // the finish's I8 refinement
    bool chk, chk_l;    // the int8 pass's checksum; its L sums too
    int fin_split;
    int R_rep;          // device re-pass: gathered queries at most
};
inline SearchGeometry search_geometry(const SearchShape& s, const SearchKnobs& kn, const SearchKP& kp,
                                      const SearchKernelFacts& f) {
    SearchGeometry g{};
    const int B = s.B, KP = kp.KP, prec = s.prec;
    const int64_t N = s.N;
    const bool exact_all = kp.exact_all;
    g.i8_pass = prec_is_i8(prec);  // vdb_scan8.hip
    g.Gs = search_groups(prec, s.G);
    // fp32: vdb_scan.hip (variants); split-bf16 (bf16x3, bf16): vdb_scan2.hip
    g.split_pass = prec == PREC_BF16X3 || prec == PREC_BF16;
    // The split pass's 128-query shape (vdb_scan2_kernel.h, q4): short rows whose query block
    // fits LDS at 128 queries (D <= 128), KP = 128, batches of >= 256: half the query blocks, so
    // each row range is re-read from L2 by half as many workgroups (C4: 8 -> 4 blocks)
    g.q4 = g.split_pass && !exact_all && !s.gated && KP == 128 && B >= 256 && g.Gs <= 8 &&
           (kn.scan_q4 == 1 || (kn.scan_q4 < 0));
    // The wide int8 pass (vdb_scan8w.hip): rows of 4 groups (D <= 128) and batches of more than 256
    // (C4, and each rank of its row-sharded run): all queries of a 512-query block in one
    // workgroup, the corpus staged once through LDS; one workgroup per CU, tiles dealt round-robin
    const int64_t n_tiles_all = plan_round_up(N, 32) / 32;
    // ... and its long-row form (vdb_scan8wl.hip): the I8 cosine pass for 16..48 groups and up to
    // 256 queries, all of them in one workgroup's registers, two waves per query tile for batches
    // of <= 128 with rows of <= 1024 dims.  Auto (profiles/r06_wl3, r06_rl4): every batch for rows
    // of <= 1024 dims (C2, B = 64: scan 0.142 -> 0.117 ms, 410 -> 432 K QPS; B = 2 / 32 / 128
    // faster too); at 1536 dims batches of <= 16 and > 96 (C3: 420 -> 494 K; B = 32 even, 64
    // slower).
    g.wide_long = g.i8_pass && !exact_all && !s.gated && f.scan8wl_ok && N > 0 &&
                  (kn.scan_wide == 1 || (kn.scan_wide < 0 && N >= kWideMinRows && (g.Gs <= 32 || B <= 16 || B > 96)));
    g.wide8 = g.wide_long ||
              (g.i8_pass && !exact_all && !s.gated && f.scan8w_ok && N > 0 &&
               (kn.scan_wide == 1 || (kn.scan_wide < 0 && N >= kWideMinRows && (B > 256 || N <= kWideSplitMaxRows))));
    g.n_seg8 = !g.wide8 ? 0
               : kn.n_wg_override > 0
                   ? (int)std::min<int64_t>(FIN_SEG_MAX, std::min<int64_t>(kn.n_wg_override, n_tiles_all))
                   : (int)std::min<int64_t>(FIN_SEG_MAX, plan_round_up(std::min<int64_t>(s.n_cu, n_tiles_all), 8));
    // query rows per candidate-pass block: the int8 pass keeps 64 at KP = 256 (KW = 64 kept per
    // workgroup, vdb_scan8_kernel.h), the split pass 32 there
    g.QB = g.q4 ? 128 : g.i8_pass ? 64 : KP == 256 ? 32 : 64;
    g.QB_pilot = g.i8_pass ? 64 : KP == 256 ? 32 : 64;  // the pilot's own query blocks (instantiations)
    g.Bp = (int)plan_round_up(B, 128);                 // whole query super tiles (tiled layout)
    g.n_qblocks = (B + g.QB - 1) / g.QB;
    g.variant = g.split_pass || g.i8_pass ? 0 : (int)kn.scan_variant;
    if (!g.split_pass && !g.i8_pass && !f.scan_variant_ok) g.variant = 0;  // e.g. PX=8 needs Dp % 128 == 0
    g.step_rows = g.q4 ? f.rows_per_step_q4 : f.rows_per_step;
    g.n_steps = std::max<int64_t>(1, plan_round_up(N, g.step_rows) / g.step_rows);
    // one 4-wave workgroup per CU (1 wave per SIMD, all of its 512 registers):
    // measured faster than two per CU, whose top-k epilogues then overlap (profiles/)
    const int target = kn.n_wg_override > 0 ? (int)kn.n_wg_override : std::max(1, s.n_cu / g.n_qblocks);
    g.spw = (int)std::max<int64_t>(1, (g.n_steps + target - 1) / target);
    g.n_wg = (int)((g.n_steps + g.spw - 1) / g.spw);
    g.mask_words = plan_round_up(N, 32) / 32;
    // Step end of the scan (vdb_scan.hip): short steps (Dp <= 128: C4's 10M x 128 runs 8 split
    // groups per step, the epilogue ~half of it) gain from dropping the per-step workgroup barrier
    // (C4 scan 7.58 -> 6.22 ms); long steps lose (C2 0.57 -> 0.65 ms, C3 2.62 -> 2.90 ms), measured.
    // The int8 pass drops it at every length: a per-step barrier lines up the 4 waves' epilogues,
    // so the CU's stream idles through all of them at once; flag-gated, one wave's epilogue runs
    // under the others' loads (C2 366 -> 384 K QPS, C3 365 -> 401 K with its scan 0.576 -> 0.487 ms,
    // profiles/r04_ab/sync, same box).
    g.lockstep = kn.scan_sync == 0 ? (!g.i8_pass && s.Dp > 128) : kn.scan_sync == 1;
    // finish: optionally several workgroups per query share the exact rerank (tuning knob
    // "finish_split"; measured at C2 bf16, B = 64: split 4 took the finish 24.5 -> 45.9 us,
    // profiles/r02_ab, so the default is 1)
    g.fin_split = (int)kn.finish_split;
    // int8 L2 pass: the batch's integer accumulator start values (vdb_scan8.hip rstart8)
    g.rs8_on = g.i8_pass && !exact_all && s.metric == 1;
    g.i8_refine = prec == PREC_I8 && kn.has_xh &&  // the finish's I8 refinement
                  (kn.i8_refine == 1 || (kn.i8_refine == -1 && s.Dp >= kRefineMinDp));
    g.R_rep = std::min(B, kRepassDev);  // device re-pass: gathered queries + results
    // the int8 pass's checksum: partial sums [2][n_wg8][Bp], expected values [Bp][2], L2 start sum
    g.chk = g.i8_pass && !exact_all && kn.scan_checksum && kn.has_csum && N > 0;
    // the L sums of I8X3 too (scan_checksum 2): +5% on C4's scan over H alone (the xh plane, the
    // query's hi plane and the start values; an L operand moves a score by at most the slack lsl)
    g.chk_l = g.chk && prec == PREC_I8X3 && kn.scan_checksum == 2;
    g.n_wg8 = g.wide8 ? g.n_seg8 : (g.n_wg + 7) / 8 * 8;
    g.priv = !exact_all && !g.split_pass && !g.i8_pass && f.scan_priv;
    // global per-query candidate lists: at most 512 entries per workgroup and query
    // (the largest LDS buffer of any variant; 4 x 64 for the wave-private one)
    g.gl_cap = exact_all ? 0 : g.wide8 ? (int64_t)g.n_seg8 * W8_CH : (int64_t)((g.n_wg + 7) / 8 * 8) * 512;
    return g;
}

// ---- pilot ----------------------------------------------------------------------------------------
struct SearchPilot {
    int n_pilot;     // row tiles sampled (0: no pilot)
    int pilot_rank;  // rank of the bound among the sampled scores, in [1, KP]
};
inline SearchPilot search_pilot(const SearchShape& s, const SearchKnobs& kn, const SearchKP& kp,
                                const SearchGeometry& g) {
    const int k = s.k, KP = kp.KP;
    const int64_t N = s.N;
    // Pilot sample: 512 row tiles, more for large k (its bound then saves more insert work than
    // the sample costs: C4, k = 100, 512 -> 4096 tiles: 89.5 K -> 96.4 K QPS, profiles/r02_ab),
    // and at least 1/160 of the rows: the bound's global rank ~ r N / S sets how many entries
    // each workgroup inserts (C6, 10 M rows, int8 pass: 512 -> 2048 tiles, scan 0.329 -> 0.259 ms,
    // 200 K -> 250 K QPS; C2 / C3, 1 M rows: larger samples only add pilot time,
    // profiles/r03_i8/pilot).
    // Rows of 4 groups (D <= 128: the int8 pass's register-resident pilot, vdb_scan8.hip
    // pilot8_g4) take twice the k-based sample, up to 8192 tiles where the rows are many (at most
    // ~2.5% of them): C4 (k = 100) 4096 -> 8192, scan 2.32 -> 2.19 ms, 213 K -> 220 K QPS with
    // the pilot at ~50 -> ~90 us (profiles/r05_ab/ab20)
    const bool cheap_pilot = g.i8_pass && g.Gs == 4;
    const int64_t pilot_cap = cheap_pilot ? std::max<int64_t>(4096, std::min<int64_t>(8192, N / (32 * 40))) : 4096;
    const int64_t pilot_def = std::min<int64_t>(
        pilot_cap, std::max<int64_t>((cheap_pilot ? 1024 : 512) * std::max(1, k / 12), N / (32 * 160)));
    SearchPilot p;
    p.n_pilot = s.gated ? 0  // a gated re-pass sub-search: no pilot (few queries; its launches stay light)
                        : (int)std::min<int64_t>(kn.pilot_tiles >= 0 ? kn.pilot_tiles : pilot_def,
                                                 plan_round_up(N, 32) / 32);
    // Rank of the pilot's bound among its sampled scores.  The KP-th best sample is a
    // guaranteed lower bound of the global KP-th best but sits at global rank ~KP N / S (C2:
    // ~2000), so the candidate pass inserts every score above that until its own buffers
    // tighten (the warm-up: 140 us of a 680 us C2 scan without a pilot, ~65 us with one).
    // Instead: the r-th best sample, r the smallest rank such that (1) the sample holds r of
    // the global top k with probability < 1e-6 (Poisson(k S / N) tail; rows in no particular
    // order), so T stays below a_k, and (2) T's expected global rank r N / S is >= 2 KP, so T
    // mostly stays below a_KP too and the certificate's cut max(a_KP, T) is what it would be
    // without a pilot (T near a_k failed bf16's wide certificate: C2 with 2048 tiles and rule
    // (1) alone; the KP-based Poisson rule instead cost C2 bf16 7%, profiles/r02_ab).  C2: r = 5,
    // T at rank ~300 instead of ~2000.  Exactness does not depend on it: rows dropped below the
    // bound are covered by the certificate (acut >= T), which sends a query whose bound was too
    // high to the exact path.
    p.pilot_rank = KP;
    if (p.n_pilot > 0) {
        const double S = (double)std::min<int64_t>((int64_t)p.n_pilot * 32, N);
        const double x = (double)k * S / (double)N;
        double term = std::exp(-x), cdf = term;
        int r = 1;
        while (1.0 - cdf >= 1e-6 && r < KP) {
            term *= x / r;
            cdf += term;
            ++r;
        }
        const int r_min = (int)std::ceil(2.0 * KP * S / (double)N);
        p.pilot_rank = std::min(std::max(r, r_min), KP);
    }
    if (kn.pilot_rank_override > 0) p.pilot_rank = (int)std::min<int64_t>(kn.pilot_rank_override, KP);
    return p;
}

// ---- workspace layout -----------------------------------------------------------------------------
// Byte offsets into the workspace (each 256-byte aligned; -1: the call has no such buffer), and
// the total to reserve.
constexpr int kFlagInts = 64;  // beyond the flag list [B]: its count, overflow, inconsistent, two re-pass counts
struct SearchLayout {
    int64_t Qraw, maskd;               // host mode: the staged queries [B][D] and mask (+ 64 words)
    int64_t Qt;                        // query tiles [Bp][Dp + 16 QG_EXTRA] (fp32, split or int8)
    int64_t qn64, qconst;              // canonical norms [Bp]; the finish's per-query constants [Bp][3]
    int64_t os, oi, ok;                // host mode: the results [B][k]
    int64_t flags;                     // [1 + B + 4]: flag count, list, overflow, inconsistent, re-pass counts
    int64_t done;                      // gated fallback: workgroups done per query [Bp]
    int64_t gthr, gslots;              // shared thresholds [Bp]; threshold slots, then pilot slots [Bp] each
    int64_t gl_s, gl_i, gl_cnt;        // candidate lists [B][gl_cap] and their counts [Bp]
    int64_t fx_ek, fx_ck, fx_cr, fx_n; // finish_split > 1: the workgroups' partial reranks
    int64_t q8max, q8lsl, q8err, q8scal;  // int8 pass: per query [Bp]; per batch [64]
    int64_t q8res, q8err2;             // I8 refinement: query residuals [Bp][Dp], their bound [Bp]
    int64_t chkp, segc, chkr;          // checksum partials [2][n_wg8][Bp]; wide segment counts; L2 start sum
    int64_t rs8;                       // int8 L2 start values, one per row of the whole steps
    int64_t chke;                      // checksum expectations [Bp][2] (written by the pilot)
    int64_t rep_q, rep_s, rep_i, rep_k;  // device re-pass: gathered queries and their results [R_rep]
    int64_t total;
};
inline SearchLayout search_layout(const SearchShape& s, const SearchGeometry& g, const SearchPilot& p) {
    SearchLayout l;
    const int64_t B = s.B, Bp = g.Bp, k = s.k, D = s.D, Dp = s.Dp;
    int64_t o = 0;
    auto take = [&](bool on, int64_t bytes) {
        if (!on) return (int64_t)-1;
        const int64_t at = o;
        o += plan_align(bytes);
        return at;
    };
    const bool fx = g.fin_split > 1, dev = !s.host;
    l.Qraw = take(true, B * D * 4);
    l.maskd = take(true, (g.mask_words + 64) * 4);
    l.Qt = take(true, Bp * (Dp + 16 * QG_EXTRA) * 4);
    l.qn64 = take(true, Bp * 8);
    l.qconst = take(true, Bp * 3 * 8);
    l.os = take(true, B * k * 4);
    l.oi = take(true, B * k * 8);
    l.ok = take(true, B * k * 8);
    l.flags = take(true, (B + kFlagInts) * 4);
    l.done = take(true, Bp * 4);
    l.gthr = take(true, Bp * 4);
    l.gslots = take(true, Bp * (KP_MAX + PILOT_SLOTS) * 4);
    l.gl_s = take(true, B * g.gl_cap * 4);
    l.gl_i = take(true, B * g.gl_cap * 4);
    l.gl_cnt = take(true, Bp * 4);
    l.fx_ek = take(fx, B * g.fin_split * KP_MAX * 8);
    l.fx_ck = take(fx, B * g.fin_split * KP_MAX * 4);
    l.fx_cr = take(fx, B * g.fin_split * KP_MAX * 4);
    l.fx_n = take(fx, B * g.fin_split * 4);
    l.q8max = take(true, Bp * 4);
    l.q8lsl = take(true, Bp * 4);
    l.q8err = take(true, Bp * 4);
    l.q8scal = take(true, 64 * 4);
    l.q8res = take(g.i8_refine, Bp * Dp * 4);
    l.q8err2 = take(g.i8_refine, Bp * 4);
    l.chkp = take(g.chk, 2 * (int64_t)g.n_wg8 * Bp * 4);
    l.segc = take(g.wide8, Bp * g.n_seg8 * 4);
    l.chkr = take(g.chk && s.metric == 1, 64 * 4);
    // (rstart8 writes the rows of whole 32-row tiles; the 64-query int8 pass loads the start values
    // of every row tile of a step, so the buffer covers the last step whole)
    l.rs8 = take(g.rs8_on, plan_round_up(s.N, std::max<int64_t>(32, g.step_rows)) * 4);
    // (the pilot writes the checksum's expectations when it runs; else the finish computes them)
    l.chke = take(g.chk && p.n_pilot > 0, 2 * Bp * 4);
    l.rep_q = take(dev, (int64_t)g.R_rep * D * 4);
    l.rep_s = take(dev, (int64_t)g.R_rep * k * 4);
    l.rep_i = take(dev, (int64_t)g.R_rep * k * 8);
    l.rep_k = take(dev, (int64_t)g.R_rep * k * 8);
    l.total = o;
    return l;
}

// ---- the exact path -------------------------------------------------------------------------------
// The exact scan of nq queries (run_exact): KE entries per list, n_wg row ranges of rpw rows, one
// list per (query, range), merged per query.  gated: the device-gated form (the flagged count is
// read on the device), one workgroup per CU instead of two since an empty gated launch still has to
// find free CUs beside the next batch's scan; at least 256 rows per workgroup.
struct ExactPlan {
    int KE, n_wg;
    int64_t rpw;
    int slots;       // gated: query slots of the launch
    int n_wg_gate;   // the range count before rebalancing: what the kGatedExactBytes test counts
};
inline ExactPlan exact_plan(int64_t N, int n_cu, int nq, int k, bool gated) {
    ExactPlan e;
    e.KE = std::max(32, plan_next_pow2(k));
    const int64_t wg_target = gated ? std::max<int64_t>(1, n_cu) : std::max<int64_t>(1, 2 * (int64_t)n_cu);
    e.n_wg_gate = (int)std::min<int64_t>(wg_target, std::max<int64_t>(1, N / 256));
    e.rpw = std::max<int64_t>(1, (N + e.n_wg_gate - 1) / e.n_wg_gate);
    // whole ranges only: fewer workgroups than n_wg_gate when the rows do not fill them
    e.n_wg = (int)std::max<int64_t>(1, (N + e.rpw - 1) / e.rpw);
    e.slots = std::min(nq, kGateSlots);
    return e;
}
// Its lists in the workspace's exact buffer.  scratch_bytes: the device-gated single-launch form's
// top-k buffers (exact_scan_scratch_bytes(KE, n_wg, slots), vdb_exact.hip), 0 for the other forms.
struct ExactLayout {
    int64_t lk, li;  // per (query, range) lists [nq][n_wg][KE]: fp64 keys, rows
    int64_t mk, mi;  // merged [nq][KE]
    int64_t scr;     // -1: none
    int64_t total;
};
// Bytes of the lists for n_wg ranges: their sum and a page for the five buffers' alignment.
inline int64_t exact_list_bytes(int nq, int n_wg, int KE, int64_t scratch_bytes) {
    return (int64_t)nq * n_wg * KE * 12 + (int64_t)nq * KE * 12 + 4096 + scratch_bytes;
}
inline ExactLayout exact_layout(const ExactPlan& e, int nq, int64_t scratch_bytes) {
    ExactLayout l;
    const int64_t list_elems = (int64_t)nq * e.n_wg * e.KE;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += plan_align(bytes);
        return at;
    };
    l.lk = take(list_elems * 8);
    l.li = take(list_elems * 4);
    l.mk = take((int64_t)nq * e.KE * 8);
    l.mi = take((int64_t)nq * e.KE * 4);
    l.scr = scratch_bytes > 0 ? take(scratch_bytes) : -1;
    l.total = exact_list_bytes(nq, e.n_wg, e.KE, scratch_bytes);  // (>= o: the page covers the alignment)
    return l;
}
// The size a device-memory batch's gated fallback is judged by (against kGatedExactBytes: it decides
// whether the batch's fallback is gated on the device).  It counts n_wg_gate ranges, the count
// before rebalancing, as it always has: the rebalanced layout is never larger, and counting that
// instead would move batches across the threshold.  scratch_bytes_gate: exact_scan_scratch_bytes(KE,
// n_wg_gate, slots).
inline int64_t exact_gate_bytes(const ExactPlan& e, int nq, int64_t scratch_bytes_gate) {
    return exact_list_bytes(nq, e.n_wg_gate, e.KE, scratch_bytes_gate);
}

}  // namespace vdb
