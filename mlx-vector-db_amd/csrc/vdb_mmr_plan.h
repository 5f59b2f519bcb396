// vdb_mmr_plan.h — the host arithmetic of vdb_index_search_mmr (vdb_api.cpp) and the decisions its
// kernels share with it (vdb_mmr.hip): the limits and the argument validation, how many queries
// share one pair-similarity scratch, how the (i < j) position pairs of a candidate list are dealt to
// workgroups and waves, the per-call scratch, and the selection step itself (value, tie rule,
// penalty update) as plain functions over plain arrays.  Plain C++ with no HIP in it, so a
// stand-alone CPU program can sweep it under a sanitizer (tools/mmr_plan_check.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_MMR_HD __host__ __device__
#else
#define VDB_MMR_HD
#endif

namespace vdb {

constexpr int kMmrMaxK = 200;      // rows a query can ask for
constexpr int kMmrMaxFetch = 200;  // candidates per query: the most the certified fast path returns
// The pairs kernel: a workgroup is kMmrWaves waves; it takes kMmrWaves consecutive positions i (one
// per wave) and one aligned batch of kMmrNB positions j, of which a wave scores those above its i.
constexpr int kMmrWaves = 4;
constexpr int kMmrNB = 4;
// The select kernel: one wave per query, lane l holds positions l, l + 64, ...
constexpr int kMmrLanePos = (kMmrMaxFetch + 63) / 64;
constexpr int64_t kMmrPairBytes = 64ll << 20;  // bound on the pair similarities of one query block
constexpr int kMmrMaxBlock = 32768;            // queries per block at most (a grid dimension)

// ---- the query block ------------------------------------------------------------------------------
// S takes fetch_k^2 fp64 per query; a call runs in blocks of this many queries, one after another on
// the stream over the same scratch (209 queries at fetch_k = 200).
VDB_MMR_HD inline int mmr_query_block(int fetch_k) {
    const int64_t per = (int64_t)fetch_k * fetch_k * 8;
    int64_t qb = per > 0 ? kMmrPairBytes / per : kMmrMaxBlock;
    if (qb > kMmrMaxBlock) qb = kMmrMaxBlock;
    return qb < 1 ? 1 : (int)qb;
}

// ---- the deal of pair tasks -----------------------------------------------------------------------
// Positions 0 .. F-1 (F = fetch_k).  Row group g holds positions i in [g W, g W + W) (W = kMmrWaves),
// batch jb positions j in [jb NB, jb NB + NB).  Group g needs the batches that can hold a j above its
// lowest i: jb >= (g W + 1) / NB.  Workgroups are numbered group by group, batches ascending.
VDB_MMR_HD inline int mmr_batches(int F) { return (F + kMmrNB - 1) / kMmrNB; }
VDB_MMR_HD inline int mmr_row_groups(int F) { return (F + kMmrWaves - 1) / kMmrWaves; }
VDB_MMR_HD inline int mmr_first_batch(int g) { return (g * kMmrWaves + 1) / kMmrNB; }
VDB_MMR_HD inline int mmr_group_wgs(int F, int g) {
    const int c = mmr_batches(F) - mmr_first_batch(g);
    return c > 0 ? c : 0;
}
// Workgroups of one query's pairs.
VDB_MMR_HD inline int mmr_pair_wgs(int F) {
    int t = 0;
    for (int g = 0; g < mmr_row_groups(F); ++g) t += mmr_group_wgs(F, g);
    return t;
}
// Wave `wave` of workgroup `wg`: position i and the positions [j0, j1) it scores against i (all
// above i and below F; empty when j0 >= j1).
struct MmrPairTask {
    int i, j0, j1;
};
VDB_MMR_HD inline MmrPairTask mmr_pair_task(int F, int wg, int wave) {
    MmrPairTask t;
    t.i = 0; t.j0 = 0; t.j1 = 0;
    int g = 0;
    const int ng = mmr_row_groups(F);
    while (g < ng && wg >= mmr_group_wgs(F, g)) {
        wg -= mmr_group_wgs(F, g);
        ++g;
    }
    if (g >= ng) return t;  // past the last workgroup: nothing
    const int jb = mmr_first_batch(g) + wg;
    t.i = g * kMmrWaves + wave;
    if (t.i >= F) {
        t.i = 0;
        return t;
    }
    t.j0 = jb * kMmrNB > t.i + 1 ? jb * kMmrNB : t.i + 1;
    t.j1 = jb * kMmrNB + kMmrNB < F ? jb * kMmrNB + kMmrNB : F;
    if (t.j0 >= t.j1) t.j0 = t.j1 = 0;
    return t;
}

// ---- the selection step ---------------------------------------------------------------------------
// All fp64, multiply and subtract apart (the library is built without contraction).
VDB_MMR_HD inline double mmr_value(double lambda, double one_minus_lambda, double rel, double pen) {
    const double a = lambda * rel;
    const double b = one_minus_lambda * pen;
    return a - b;
}
// (value desc, position asc): a tie goes to the lower position, the better key and then the lower row.
VDB_MMR_HD inline bool mmr_better(double va, int pa, double vb, int pb) { return va > vb || (va == vb && pa < pb); }
// The greatest similarity to a picked row so far; exactly this form (not fmax) so that the sign of a
// zero cannot differ between device and oracle.
VDB_MMR_HD inline double mmr_pen_update(double s, double pen) { return (s > pen) ? s : pen; }

// The whole selection of one query over plain arrays: n candidates with relevance rel[i] and pair
// similarities S[i * ld + j]; writes the min(k, n) picked positions and their values in pick order,
// returns their number.  pen and picked are scratch of n entries.
inline int mmr_select(int n, int k, double lambda, const double* rel, const double* S, int ld, int* out_pos,
                      double* out_mmr, double* pen, unsigned char* picked) {
    const int m = k < n ? k : n;
    if (m <= 0) return 0;
    const double oml = 1.0 - lambda;
    for (int i = 0; i < n; ++i) picked[i] = 0;
    int pick = 0;
    double v_pick = lambda * rel[0];
    for (int s = 0; s < m; ++s) {
        if (s > 0) {
            pick = -1;
            v_pick = 0.0;
            for (int i = 0; i < n; ++i) {
                if (picked[i]) continue;
                const double v = mmr_value(lambda, oml, rel[i], pen[i]);
                if (pick < 0 || mmr_better(v, i, v_pick, pick)) {
                    pick = i;
                    v_pick = v;
                }
            }
        }
        out_pos[s] = pick;
        out_mmr[s] = v_pick;
        picked[pick] = 1;
        for (int i = 0; i < n; ++i) {
            if (picked[i]) continue;
            const double sv = S[(int64_t)i * ld + pick];
            pen[i] = s == 0 ? sv : mmr_pen_update(sv, pen[i]);
        }
    }
    return m;
}

// ---- scratch --------------------------------------------------------------------------------------
inline int64_t mmr_align(int64_t b) { return (b + 255) / 256 * 256; }
struct MmrScratch {
    // byte offsets into the workspace (each 256-byte aligned), and the total
    int64_t fs, fi, fk, S;
    // host-memory calls: the staged arguments (one upload) and the results (one download)
    int64_t in0, q, mask, in_bytes, out0, out_s, out_i, out_k, out_m, out_bytes;
    int64_t mask_words, total;
};
inline MmrScratch mmr_scratch(int n_queries, int dim, int k, int fetch_k, int64_t rows, bool host, bool masked,
                              bool keys, bool mmr) {
    MmrScratch s{};
    const int64_t B = n_queries, F = fetch_k;
    s.mask_words = (rows + 31) / 32;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += mmr_align(bytes);
        return at;
    };
    const int64_t qb = B < mmr_query_block(fetch_k) ? B : mmr_query_block(fetch_k);
    s.fs = take(B * F * 4);
    s.fi = take(B * F * 8);
    s.fk = take(B * F * 8);
    s.S = take(qb * F * F * 8);
    s.in0 = o;
    if (host) {
        s.q = take(B * dim * 4);
        // (+ 64 zero words, as a host search's staged mask: the candidate passes read whole mask tiles)
        s.mask = take(masked ? (s.mask_words + 64) * 4 : 0);
    }
    s.in_bytes = o - s.in0;
    s.out0 = o;
    if (host) {
        s.out_s = take(B * k * 4);
        s.out_i = take(B * k * 8);
        s.out_k = take(keys ? B * k * 8 : 0);
        s.out_m = take(mmr ? B * k * 8 : 0);
    }
    s.out_bytes = o - s.out0;
    s.total = o;
    return s;
}

// ---- validation -----------------------------------------------------------------------------------
enum {
    kMmrOk = 0,
    kMmrBadQueries = 1,   // n_queries < 0
    kMmrBadK = 2,         // k outside [1, kMmrMaxK]
    kMmrBadFetch = 3,     // fetch_k outside [k, kMmrMaxFetch]
    kMmrBadLambda = 4,    // lambda NaN, infinite or outside [0, 1]
    kMmrNullPointer = 5,  // queries or a required output missing
    kMmrBadMem = 6        // a memory kind that is neither host (0) nor device (1)
};
inline int mmr_validate(int n_queries, int k, int fetch_k, double lambda, bool has_queries, bool has_scores,
                        bool has_indices, int mem) {
    if (n_queries < 0) return kMmrBadQueries;
    if (k < 1 || k > kMmrMaxK) return kMmrBadK;
    if (fetch_k < k || fetch_k > kMmrMaxFetch) return kMmrBadFetch;
    if (!(lambda >= 0.0 && lambda <= 1.0)) return kMmrBadLambda;  // (a NaN fails both comparisons)
    if (!has_queries || !has_scores || !has_indices) return kMmrNullPointer;
    if (mem != 0 && mem != 1) return kMmrBadMem;
    return kMmrOk;
}

}  // namespace vdb
