// vdb_mmr.hip: MMR search (vdb_index_search_mmr), part of the gfx950 kernels of the brute-force
// distance + top-k path (pipeline overview: vdb_scan.hip).  Built with -ffp-contract=off.
//
// A query gets k rows that are relevant and unlike each other: of its best k' = fetch_k rows (the
// candidate list, positions 0 .. n-1 by (key desc, row asc)) it picks greedily, each time the
// unpicked position i with the greatest lambda * rel_i - (1 - lambda) * max over picked p of
// S[i][p], where rel_i is the canonical fp64 key of (query, row c_i) and S[i][j] the canonical key
// of (row c_i taken as the query, row c_j) (vdb_exact_keys.h).  Three steps per call, all queued on
// one stream:
//   1. the ordinary certified search fetches the candidate lists with their keys;
//   2. mmr_pairs_kernel, per block of queries, scores every pair i < j of a list, one wave per
//      (i, batch of 4 positions j), and writes S[i][j] and S[j][i] (the key is bitwise symmetric);
//   3. mmr_select_kernel, one wave per query, keeps rel, the penalty and the picked bit of up to 4
//      positions per lane in registers; a pick is a wave reduction on (value desc, position asc)
//      and one coalesced read of row S[pick][.].
// No atomics, no LDS; the value, the tie rule and the penalty update are vdb_mmr_plan.h's.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_exact_keys.h"
#include "vdb_mmr_plan.h"

namespace vdb {

// ---- step 2: the pair similarities ----------------------------------------------------------------------
// MP: 4 / 8 = rows of up to 256 MP dims with every piece of a batch in flight; 0 = any length.
// Grid (mmr_pair_wgs(k_fetch), queries of the block).  Positions whose candidate is -1 (at or past
// the list's valid count) are neither read nor written.
template <int METRIC, int MP>
__global__ void __launch_bounds__(256) mmr_pairs_kernel(MmrArgs a, int b0) {
    constexpr int NB = kMmrNB;
    const int F = a.k_fetch;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const MmrPairTask t = mmr_pair_task(F, (int)blockIdx.x, wv);
    if (t.j0 >= t.j1) return;
    const int bq = blockIdx.y;
    const int64_t* c = a.fi + (size_t)(b0 + bq) * F;
    const int64_t ci = c[t.i];
    if (ci < 0 || ci >= a.count) return;
    // the valid positions of a list are a prefix of it: so are this batch's
    uint32_t rows[NB];
    double xn[NB];
    int nb = 0;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int j = t.j0 + u;
        const int64_t r = j < t.j1 ? c[j] : (int64_t)-1;
        const bool ok = nb == u && r >= 0 && r < a.count;
        rows[u] = ok ? (uint32_t)r : 0u;
        xn[u] = (METRIC == 0 && ok) ? a.nrm64[r] : 1.0;
        nb += ok ? 1 : 0;
    }
    if (nb == 0) return;
    // row c_i as the query: a contiguous fp32 vector of the row-major copy, its canonical norm kept
    const float* q = a.X + row_piece_offset((uint64_t)ci, 0, a.G);
    const double qn = METRIC == 0 ? a.nrm64[ci] : 1.0;
    double keys[NB];
    if constexpr (MP > 0) {
        exact_keys_rows<METRIC, NB, MP>(q, a.D, qn, a.X, a.G, (a.D + 255) / 256, rows, xn, nb, keys);
    } else {
        exact_keys_batch<METRIC, NB>(q, qn, a.X, a.G, a.D, rows, xn, nb, keys);
    }
    double* S = a.S + (size_t)bq * F * F;
#pragma unroll
    for (int u = 0; u < NB; ++u)
        if (u < nb && lane == u) {
            const int j = t.j0 + u;
            S[(size_t)t.i * F + j] = keys[u];
            S[(size_t)j * F + t.i] = keys[u];
        }
}

hipError_t launch_mmr_pairs(int metric, const MmrArgs& a, int b0, int qb, hipStream_t st) {
    if (qb <= 0) return hipSuccess;
    if (a.k_fetch < 1 || a.k_fetch > kMmrMaxFetch || qb > mmr_query_block(a.k_fetch) || !a.S || !a.fi)
        return hipErrorInvalidValue;
    const int wgs = mmr_pair_wgs(a.k_fetch);
    if (wgs == 0) return hipSuccess;  // a list of one position has no pair
    const dim3 grid(wgs, qb);
    const int mp = a.D <= 1024 ? 4 : a.D <= 2048 ? 8 : 0;
#define VDB_MMR(M, MPV)                                                                       \
    if (metric == M && mp == MPV) {                                                           \
        hipLaunchKernelGGL((mmr_pairs_kernel<M, MPV>), grid, dim3(256), 0, st, a, b0);        \
        return hipGetLastError();                                                             \
    }
    VDB_MMR(0, 4) VDB_MMR(0, 8) VDB_MMR(0, 0)
    VDB_MMR(1, 4) VDB_MMR(1, 8) VDB_MMR(1, 0)
#undef VDB_MMR
    return hipErrorInvalidValue;
}

// ---- step 3: the selection --------------------------------------------------------------------------------
// One wave per query (grid = the block's queries, 64 threads).  Writes out_* [b][k] in pick order,
// "no result" past min(k, valid positions).
template <int METRIC>
__global__ void __launch_bounds__(64) mmr_select_kernel(MmrArgs a, int b0) {
    constexpr int T = kMmrLanePos;
    const int lane = threadIdx.x;
    const int bq = blockIdx.x;
    const size_t b = (size_t)b0 + bq;
    const int F = a.k_fetch;
    const int K = a.k;
    const int64_t* c = a.fi + b * F;
    const double* fk = a.fk + b * F;
    const double* S = a.S + (size_t)bq * F * F;
    float* os = a.out_s + b * K;
    int64_t* oi = a.out_i + b * K;
    double* ok = a.out_k ? a.out_k + b * K : nullptr;
    double* om = a.out_m ? a.out_m + b * K : nullptr;

    double rel[T], pen[T];
    int64_t row[T];
    bool live[T];  // a valid position not picked yet
    int n = 0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int p = lane + 64 * t;
        const int64_t r = p < F ? c[p] : (int64_t)-1;
        live[t] = r >= 0 && r < a.count;
        row[t] = r;
        rel[t] = live[t] ? fk[p] : -INFINITY;
        pen[t] = 0.0;
        n += __popcll(__ballot(live[t]));
    }
    const int m = K < n ? K : n;
    const double lam = a.lambda;
    const double oml = 1.0 - lam;
    for (int s = 0; s < m; ++s) {
        // this lane's best unpicked position, then the wave's
        double bv = -INFINITY;
        int bp = -1;
        if (s == 0) {  // slot 0 is position 0, mmr = lambda * rel
            if (lane == 0) {
                bv = lam * rel[0];
                bp = 0;
            }
        } else {
#pragma unroll
            for (int t = 0; t < T; ++t)
                if (live[t]) {
                    const double v = mmr_value(lam, oml, rel[t], pen[t]);
                    const int p = lane + 64 * t;
                    if (bp < 0 || mmr_better(v, p, bv, bp)) {
                        bv = v;
                        bp = p;
                    }
                }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_xor(bv, off, 64);
            const int op = __shfl_xor(bp, off, 64);
            if (op >= 0 && (bp < 0 || mmr_better(ov, op, bv, bp))) {
                bv = ov;
                bp = op;
            }
        }
        const int pick = bp;  // the same in every lane; >= 0: s < n unpicked positions remain
        if (pick < 0) break;
        const double* Sp = S + (size_t)pick * F;  // row S[pick][.] = column pick (bitwise symmetric)
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int p = lane + 64 * t;
            if (p == pick) {
                write_result(METRIC, rel[t], (uint64_t)row[t] + (uint64_t)a.index_offset, true, os + s, oi + s,
                             ok ? ok + s : nullptr);
                if (om) om[s] = bv;
                live[t] = false;
            }
            if (live[t] && s + 1 < m) {
                const double sv = Sp[p];
                pen[t] = s == 0 ? sv : mmr_pen_update(sv, pen[t]);
            }
        }
    }
    for (int e = m + lane; e < K; e += 64) {
        write_result(METRIC, -INFINITY, 0, false, os + e, oi + e, ok ? ok + e : nullptr);
        if (om) om[e] = -INFINITY;
    }
}

hipError_t launch_mmr_select(int metric, const MmrArgs& a, int b0, int qb, hipStream_t st) {
    if (qb <= 0) return hipSuccess;
    if (a.k < 1 || a.k > kMmrMaxK || a.k_fetch < a.k || a.k_fetch > kMmrMaxFetch || qb > mmr_query_block(a.k_fetch) ||
        !a.S || !a.fi || !a.fk || !a.out_s || !a.out_i)
        return hipErrorInvalidValue;
    if (metric == 0)
        hipLaunchKernelGGL((mmr_select_kernel<0>), dim3(qb), dim3(64), 0, st, a, b0);
    else
        hipLaunchKernelGGL((mmr_select_kernel<1>), dim3(qb), dim3(64), 0, st, a, b0);
    return hipGetLastError();
}

}  // namespace vdb
