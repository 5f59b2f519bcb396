// search_plan_check.cpp — the host arithmetic of the main search (csrc/vdb_search_plan.h) swept on
// the CPU: KP and its margins, the choice of candidate pass and its launch geometry, the pilot's
// sample and rank, the workspace layout (every buffer against what its consumers index) and the
// exact path's plan and layout; and the plans of the benchmark's own shapes pinned to their values.
// A stand-alone host program (its own main, no GPU, nothing loaded into another process);
// `make search-plan-check` builds it with -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../csrc/vdb_search_plan.h"

using namespace vdb;

static long g_checks = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        ++g_checks;                           \
        if (!(cond)) {                        \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");       \
            std::exit(1);                     \
        }                                     \
    } while (0)

// ---- the kernels' facts, restated ------------------------------------------------------------------
// vdb_scan8wl.hip:411 scan8wl_ok: the I8 cosine pass, up to W8L_QB = 256 queries, 16 / 24 / 32 / 48 groups
static bool host_scan8wl_ok(int prec, int metric, int G8, int B) {
    return prec == PREC_I8 && metric == 0 && B >= 1 && B <= 256 && (G8 == 16 || G8 == 24 || G8 == 32 || G8 == 48);
}
// vdb_scan8w.hip:431 scan8w_ok: rows of W8_G = 4 groups
static bool host_scan8w_ok(int G8, int B) { return G8 == 4 && B >= 1; }
// vdb_scan.hip:1026 scan_variant_ok: the fp32 pass, variants 0..2, G a multiple of the prefetch depth (8 for variant 2, else 4)
static bool host_scan_variant_ok(int prec, int variant, int G) {
    return prec == PREC_FP32 && variant >= 0 && variant <= 2 && G % (variant == 2 ? 8 : 4) == 0;
}
// vdb_scan.hip:1024 scan_rows_per_step: 4 waves x 32 rows x (2 row tiles for variant 0, else 4)
static int host_scan_rows_per_step(int, int variant) { return 4 * 32 * (variant == 0 ? 2 : 4); }
// vdb_scan2.hip:127 scan2_rows_per_step: S2_ROWS = 4 tiles x 4 waves x 32; the 128-query shape 2 x 4 x 32
static int host_scan2_rows_per_step(bool q4) { return q4 ? 256 : 512; }
// vdb_scan8.hip:580 scan8_rows_per_step = scan8_rows (vdb_scan8_kernel.h:100): I8 cosine 4 tiles x 4
// waves x 32; the L-plane passes and L2 2 x 4 x 32, their L2 form 1 x 8 x 32
static int host_scan8_rows_per_step(int prec, int metric) { return prec == PREC_I8 && metric == 0 ? 512 : 256; }
// vdb_scan.hip:843 scan_priv: the fp32 pass's variant 0 at KP = 32
static bool host_scan_priv(int prec, int variant, int KP) { return KP == 32 && prec == PREC_FP32 && variant == 0; }

// as the driver's kernel_facts (vdb_api.cpp)
static SearchKernelFacts facts_of(const SearchShape& s, const SearchKnobs& kn, const SearchKP& kp) {
    SearchKernelFacts f{};
    const int Gs = search_groups(s.prec, s.G);
    if (prec_is_i8(s.prec)) {
        f.scan8wl_ok = host_scan8wl_ok(s.prec, s.metric, Gs, s.B);
        f.scan8w_ok = host_scan8w_ok(Gs, s.B);
        f.rows_per_step = host_scan8_rows_per_step(s.prec, s.metric);
    } else if (s.prec == PREC_BF16X3 || s.prec == PREC_BF16) {
        f.rows_per_step = host_scan2_rows_per_step(false);
        f.rows_per_step_q4 = host_scan2_rows_per_step(true);
    } else {
        f.scan_variant_ok = host_scan_variant_ok(s.prec, (int)kn.scan_variant, Gs);
        const int v = f.scan_variant_ok ? (int)kn.scan_variant : 0;
        f.rows_per_step = host_scan_rows_per_step(s.prec, v);
        f.scan_priv = host_scan_priv(s.prec, v, kp.KP);
    }
    return f;
}

static SearchKnobs default_knobs() {
    SearchKnobs kn{};
    kn.margin = -1;
    kn.scan_q4 = kn.scan_wide = -1;
    kn.finish_split = 1;
    kn.i8_refine = -1;
    kn.scan_checksum = 1;
    kn.pilot_tiles = -1;
    kn.has_xh = kn.has_csum = true;
    return kn;
}

static long g_shapes = 0;

static const char* where(const SearchShape& s, const SearchKnobs& kn) {
    static char buf[512];
    std::snprintf(buf, sizeof(buf),
                  "B %d k %d D %d N %lld prec %d metric %d host %d gated %d repass %d n_cu %d | margin %lld q4 %lld wide %lld n_wg %lld "
                  "variant %lld split %lld checksum %lld pilot_tiles %lld pilot_rank %lld narrow %d refine %lld",
                  s.B, s.k, s.D, (long long)s.N, s.prec, s.metric, (int)s.host, (int)s.gated, (int)s.repass, s.n_cu,
                  (long long)kn.margin, (long long)kn.scan_q4, (long long)kn.scan_wide, (long long)kn.n_wg_override,
                  (long long)kn.scan_variant, (long long)kn.finish_split, (long long)kn.scan_checksum, (long long)kn.pilot_tiles,
                  (long long)kn.pilot_rank_override, (int)kn.i8_narrow, (long long)kn.i8_refine);
    return buf;
}

static void check_one(const SearchShape& s, const SearchKnobs& kn) {
    ++g_shapes;
    const SearchKP kp = search_kp(s, kn);
    const SearchKernelFacts f = facts_of(s, kn, kp);
    const SearchGeometry g = search_geometry(s, kn, kp, f);
    const SearchPilot p = search_pilot(s, kn, kp, g);
    const SearchLayout l = search_layout(s, g, p);
    const int64_t B = s.B, N = s.N, k = s.k;
#define WHERE "%s", where(s, kn)
    // ---- geometry
    CHECK(kp.KP == 32 || kp.KP == 64 || kp.KP == 128 || kp.KP == 256, WHERE);
    CHECK(kp.exact_all || (kp.KP <= 256 && kp.KP >= k), WHERE);
    CHECK(g.n_wg >= 1 && g.spw >= 1 && g.n_steps >= 1, WHERE);
    CHECK((int64_t)g.n_wg * g.spw >= g.n_steps, WHERE);
    CHECK(g.n_steps * g.step_rows >= N && (g.n_steps - 1) * g.step_rows < std::max<int64_t>(N, 1), WHERE);
    CHECK(g.n_seg8 <= FIN_SEG_MAX && (g.n_seg8 > 0) == g.wide8, WHERE);
    CHECK(!g.wide_long || g.wide8, WHERE);
    CHECK(!g.wide8 || (g.i8_pass && !kp.exact_all && !s.gated && N > 0 && g.gl_cap == (int64_t)g.n_seg8 * W8_CH), WHERE);
    CHECK(!g.q4 || (g.split_pass && kp.KP == 128 && B >= 256 && g.Gs <= 8 && !s.gated), WHERE);
    CHECK(g.QB == (g.q4 ? 128 : g.i8_pass ? 64 : kp.KP == 256 ? 32 : 64), WHERE);  // the instantiations
    CHECK(g.QB_pilot == (g.i8_pass ? 64 : kp.KP == 256 ? 32 : 64), WHERE);
    CHECK(g.n_qblocks >= 1 && (int64_t)g.n_qblocks * g.QB >= B && (int64_t)(g.n_qblocks - 1) * g.QB < B, WHERE);
    CHECK(g.Bp % 128 == 0 && g.Bp >= B && g.Bp - B < 128, WHERE);
    CHECK(g.mask_words * 32 >= N && (g.mask_words == 0 || (g.mask_words - 1) * 32 < N), WHERE);
    CHECK(g.variant >= 0 && g.variant <= 2 && (g.variant == 0 || s.prec == PREC_FP32), WHERE);
    CHECK(g.n_wg8 % 8 == 0 || g.wide8, WHERE);
    CHECK(g.n_wg8 >= (g.wide8 ? g.n_seg8 : g.n_wg), WHERE);
    CHECK(kp.exact_all ? g.gl_cap == 0 : g.gl_cap >= (g.wide8 ? 32 : 512), WHERE);
    CHECK(g.R_rep >= 1 && g.R_rep <= kRepassDev && g.R_rep <= B, WHERE);
    // ---- pilot
    CHECK(p.pilot_rank >= 1 && p.pilot_rank <= kp.KP, WHERE);
    CHECK(p.n_pilot >= 0 && p.n_pilot <= (N + 31) / 32, WHERE);
    CHECK(!s.gated || p.n_pilot == 0, WHERE);
    // ---- layout: every buffer against what the driver's launches index
    struct Region { const char* name; int64_t at, need; bool present; };
    const int64_t Bp = g.Bp, fs = g.fin_split;
    const bool fx = fs > 1, dev = !s.host;
    const Region rs[] = {
        {"Qraw", l.Qraw, B * s.D * 4, true},
        {"maskd", l.maskd, (g.mask_words + 64) * 4, true},  // (the passes read whole mask tiles)
        // G + QG_EXTRA groups of 8 fp32 dims per query, the widest tile form
        {"Qt", l.Qt, std::max<int64_t>(Bp * ((int64_t)s.G + QG_EXTRA) * 8 * 4, Bp * ((int64_t)s.Dp + 16 * QG_EXTRA) * 4), true},
        {"qn64", l.qn64, Bp * 8, true},
        {"qconst", l.qconst, Bp * 24, true},
        {"os", l.os, B * k * 4, true},
        {"oi", l.oi, B * k * 8, true},
        {"ok", l.ok, B * k * 8, true},
        // flag count, list [B], overflow, inconsistent, two re-pass counts
        {"flags", l.flags, (B + 5) * 4, true},
        {"done", l.done, Bp * 4, true},
        {"gthr", l.gthr, Bp * 4, true},
        {"gslots", l.gslots, Bp * (KP_MAX + PILOT_SLOTS) * 4, true},
        {"gl_s", l.gl_s, B * g.gl_cap * 4, true},
        {"gl_i", l.gl_i, B * g.gl_cap * 4, true},
        {"gl_cnt", l.gl_cnt, Bp * 4, true},
        {"fx_ek", l.fx_ek, B * fs * KP_MAX * 8, fx},
        {"fx_ck", l.fx_ck, B * fs * KP_MAX * 4, fx},
        {"fx_cr", l.fx_cr, B * fs * KP_MAX * 4, fx},
        {"fx_n", l.fx_n, B * fs * 4, fx},
        {"q8max", l.q8max, Bp * 4, true},
        {"q8lsl", l.q8lsl, Bp * 4, true},
        {"q8err", l.q8err, Bp * 4, true},
        {"q8scal", l.q8scal, 3 * 4, true},
        {"q8res", l.q8res, Bp * s.Dp * 4, g.i8_refine},
        {"q8err2", l.q8err2, Bp * 4, g.i8_refine},
        {"chkp", l.chkp, 2 * (int64_t)g.n_wg8 * Bp * 4, g.chk},
        {"segc", l.segc, Bp * g.n_seg8 * 4, g.wide8},
        {"chkr", l.chkr, 4, g.chk && s.metric == 1},
        // the 64-query pass loads a start value for every row of its steps; the wide pass per row tile
        // (an empty index runs no pass)
        {"rs8", l.rs8, (N == 0 ? 0 : g.wide8 ? (N + 31) / 32 * 32 : g.n_steps * g.step_rows) * 4, g.rs8_on},
        {"chke", l.chke, 2 * Bp * 4, g.chk && p.n_pilot > 0},  // only with a pilot
        {"rep_q", l.rep_q, (int64_t)g.R_rep * s.D * 4, dev},
        {"rep_s", l.rep_s, (int64_t)g.R_rep * k * 4, dev},
        {"rep_i", l.rep_i, (int64_t)g.R_rep * k * 8, dev},
        {"rep_k", l.rep_k, (int64_t)g.R_rep * k * 8, dev},
    };
    int64_t end = 0;
    for (const Region& r : rs) {
        if (!r.present) {
            CHECK(r.at == -1, "%s is laid out without a consumer (%s)", r.name, where(s, kn));
            continue;
        }
        CHECK(r.at >= 0 && r.at % 256 == 0 && r.at >= end && r.at + r.need <= l.total,
              "%s at %lld + %lld (previous end %lld, total %lld; %s)", r.name, (long long)r.at, (long long)r.need,
              (long long)end, (long long)l.total, where(s, kn));
        end = r.at + r.need;
    }
    CHECK(l.total >= end && l.total % 256 == 0, WHERE);
    CHECK(g.chk || l.chke == -1, WHERE);
#undef WHERE
}

// The sweep: every (B, k, D, N, precision, metric, memory kind) with the default knobs, with each
// knob alone at its other values, and with a few mixed settings.
template <typename F>
static void sweep(F&& fn) {
    const int Bs[] = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 512, 1100};
    const int ks[] = {1, 16, 17, 100, 200, 201, 1024};
    const int Ds[] = {1, 8, 65, 128, 129, 768, 1024, 1536};
    const int64_t Ns[] = {0, 1, 31, 32, 33, 1000, 65535, 65536, 2500001, 10000000};
    const int64_t kSplits[] = {1, 2, 8}, kWgs[] = {0, 1, 7, 300}, kTiles[] = {-1, 0, 32768}, kMargins[] = {-1, 0, 1000},
                  kRanks[] = {0, 1, 256};
    uint32_t lcg = 20261020u;
    auto rnd = [&](uint32_t n) {
        lcg = lcg * 1664525u + 1013904223u;
        return (lcg >> 8) % n;
    };
    for (int B : Bs)
        for (int k : ks)
            for (int D : Ds)
                for (int64_t N : Ns)
                    for (int prec = 0; prec < N_PREC; ++prec)
                        for (int metric = 0; metric < 2; ++metric)
                            for (int host = 0; host < 2; ++host) {
                                SearchShape s{};
                                s.B = B; s.k = k; s.D = D; s.Dp = (D + 63) / 64 * 64; s.G = s.Dp / 8;
                                s.metric = metric; s.N = N; s.n_cu = 256; s.prec = prec; s.host = host != 0;
                                const SearchKnobs d = default_knobs();
                                fn(s, d);
                                SearchShape t = s;
                                SearchKnobs kn = d;
                                t.gated = t.repass = true; t.host = false; fn(t, d);  // a device re-pass's sub-search
                                t = s; t.repass = true; fn(t, d);                     // a host re-pass's
                                t = s; t.n_cu = 8; fn(t, d);
                                for (int64_t v : {2, 8}) { kn = d; kn.finish_split = v; fn(s, kn); }
                                for (int64_t v : {0, 2}) { kn = d; kn.scan_checksum = v; fn(s, kn); }
                                for (int64_t v : {1, 7, 300}) { kn = d; kn.n_wg_override = v; fn(s, kn); }
                                for (int64_t v : {0, 1}) { kn = d; kn.scan_wide = v; fn(s, kn); }
                                for (int64_t v : {0, 1}) { kn = d; kn.scan_q4 = v; fn(s, kn); }
                                for (int64_t v : {0, 32768}) { kn = d; kn.pilot_tiles = v; fn(s, kn); }
                                for (int64_t v : {0, 1000}) { kn = d; kn.margin = v; fn(s, kn); }
                                for (int64_t v : {1, 256}) { kn = d; kn.pilot_rank_override = v; fn(s, kn); }
                                for (int64_t v : {0, 1}) { kn = d; kn.i8_refine = v; fn(s, kn); }
                                for (int64_t v : {1, 2}) { kn = d; kn.scan_variant = v; fn(s, kn); }
                                for (int64_t v : {1, 2}) { kn = d; kn.scan_sync = v; fn(s, kn); }
                                kn = d; kn.i8_narrow = true; fn(s, kn);
                                kn = d; kn.force_exact = true; fn(s, kn);
                                kn = d; kn.has_xh = kn.has_csum = false; fn(s, kn);
                                for (int mix = 0; mix < 3; ++mix) {
                                    kn = d; t = s;
                                    t.gated = rnd(4) == 0; t.repass = t.gated || rnd(3) == 0;
                                    if (t.gated) t.host = false;
                                    kn.finish_split = kSplits[rnd(3)];
                                    kn.scan_checksum = rnd(3);
                                    kn.n_wg_override = kWgs[rnd(4)];
                                    kn.scan_wide = (int64_t)rnd(3) - 1;
                                    kn.scan_q4 = (int64_t)rnd(3) - 1;
                                    kn.pilot_tiles = kTiles[rnd(3)];
                                    kn.margin = kMargins[rnd(3)];
                                    kn.pilot_rank_override = kRanks[rnd(3)];
                                    kn.i8_narrow = rnd(2) != 0;
                                    kn.i8_refine = (int64_t)rnd(3) - 1;
                                    kn.scan_variant = rnd(3);
                                    fn(t, kn);
                                }
                            }
}

// ---- the exact path ----------------------------------------------------------------------------------
static void check_exact() {
    for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)1000, (int64_t)65536, (int64_t)65793,
                      (int64_t)2500001, (int64_t)10000000})
        for (int n_cu : {1, 8, 256, 304})
            for (int nq : {1, 3, 4, 5, 130, 1100})
                for (int k : {1, 32, 33, 200, 201, 1024})
                    for (int gated = 0; gated < 2; ++gated) {
                        const ExactPlan e = exact_plan(N, n_cu, nq, k, gated != 0);
                        CHECK(e.KE >= 32 && e.KE >= k && e.KE < 2 * std::max(k, 32) && (e.KE & (e.KE - 1)) == 0, "KE %d for k %d", e.KE, k);
                        CHECK(e.n_wg >= 1 && e.n_wg <= e.n_wg_gate && e.n_wg_gate <= (gated ? n_cu : 2 * n_cu), "n_wg %d of %d", e.n_wg, e.n_wg_gate);
                        CHECK(e.rpw >= 1 && (int64_t)e.n_wg * e.rpw >= N, "ranges of %lld rows x %d cover %lld", (long long)e.rpw, e.n_wg, (long long)N);
                        CHECK(N == 0 || (int64_t)(e.n_wg - 1) * e.rpw < N, "an empty last range");
                        CHECK(N < 256 || e.rpw >= 256 || e.n_wg_gate == 1, "ranges of %lld rows", (long long)e.rpw);
                        CHECK(e.slots >= 1 && e.slots <= kGateSlots && e.slots <= nq, "slots %d", e.slots);
                        for (int64_t scr : {(int64_t)0, (int64_t)1, (int64_t)123456}) {
                            const ExactLayout l = exact_layout(e, nq, scr);
                            const int64_t elems = (int64_t)nq * e.n_wg * e.KE;
                            const int64_t at[] = {l.lk, l.li, l.mk, l.mi, l.scr};
                            const int64_t need[] = {elems * 8, elems * 4, (int64_t)nq * e.KE * 8, (int64_t)nq * e.KE * 4, scr};
                            int64_t end = 0;
                            for (int i = 0; i < 5; ++i) {
                                if (i == 4 && scr == 0) {
                                    CHECK(l.scr == -1, "scratch laid out for a form without one");
                                    continue;
                                }
                                CHECK(at[i] % 256 == 0 && at[i] >= end && at[i] + need[i] <= l.total, "exact buffer %d at %lld + %lld of %lld", i,
                                      (long long)at[i], (long long)need[i], (long long)l.total);
                                end = at[i] + need[i];
                            }
                            // the threshold's figure counts the ranges before rebalancing: never below the layout
                            CHECK(exact_gate_bytes(e, nq, scr) >= l.total, "gate bytes below the layout");
                        }
                    }
}

// ---- the benchmark's shapes (bench.py CONFIGS), device memory, default knobs, 256 CUs, the pass
// VDB_PREC_AUTO takes on them -------------------------------------------------------------------------
struct Pinned {
    const char* name;
    int64_t N; int D, B, k, metric, prec; bool narrow;
    int KP, QB, n_qblocks; int64_t n_steps; int n_wg, spw, n_seg8; int64_t gl_cap; int n_pilot, pilot_rank;
};
static const Pinned kPinned[] = {
    {"c1 (single query)", 10000, 384, 1, 10, 0, PREC_I8, true, 128, 64, 1, 20, 20, 1, 0, 12288, 313, 128},
    {"c2", 1000000, 768, 64, 10, 0, PREC_I8, true, 256, 64, 1, 1954, 245, 8, 256, 8192, 512, 9},
    {"c3", 1000000, 1536, 256, 10, 0, PREC_I8, true, 256, 64, 4, 1954, 64, 31, 256, 8192, 512, 9},
    {"c4", 10000000, 128, 512, 100, 1, PREC_I8Q, true, 256, 64, 8, 39063, 32, 1221, 256, 8192, 7812, 14},
    {"c6", 10000000, 128, 64, 10, 0, PREC_I8, true, 256, 64, 1, 19532, 254, 77, 0, 131072, 1953, 4},
};

static void check_pinned() {
    for (const Pinned& c : kPinned) {
        SearchShape s{};
        s.B = c.B; s.k = c.k; s.D = c.D; s.Dp = (c.D + 63) / 64 * 64; s.G = s.Dp / 8;
        s.metric = c.metric; s.N = c.N; s.n_cu = 256; s.prec = c.prec;
        SearchKnobs kn = default_knobs();
        kn.i8_narrow = c.narrow;
        const SearchKP kp = search_kp(s, kn);
        const SearchGeometry g = search_geometry(s, kn, kp, facts_of(s, kn, kp));
        const SearchPilot p = search_pilot(s, kn, kp, g);
        CHECK(kp.KP == c.KP && !kp.exact_all, "%s: KP %d", c.name, kp.KP);
        CHECK(g.QB == c.QB && g.n_qblocks == c.n_qblocks, "%s: QB %d, %d blocks", c.name, g.QB, g.n_qblocks);
        CHECK(g.n_steps == c.n_steps && g.n_wg == c.n_wg && g.spw == c.spw, "%s: %lld steps, %d x %d", c.name, (long long)g.n_steps, g.n_wg, g.spw);
        CHECK(g.n_seg8 == c.n_seg8 && g.gl_cap == c.gl_cap, "%s: %d segments, gl_cap %lld", c.name, g.n_seg8, (long long)g.gl_cap);
        CHECK(p.n_pilot == c.n_pilot && p.pilot_rank == c.pilot_rank, "%s: pilot %d tiles, rank %d", c.name, p.n_pilot, p.pilot_rank);
    }
}

int main() {
    sweep(check_one);
    check_exact();
    check_pinned();
    std::printf("search plan ok: %ld plans, %ld checks\n", g_shapes, g_checks);
    return 0;
}
