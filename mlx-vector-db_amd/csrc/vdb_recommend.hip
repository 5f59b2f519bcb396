// vdb_recommend.hip: recommend search (vdb_index_search_recommend), part of the gfx950 kernels of the
// brute-force distance + top-k path (pipeline overview: vdb_scan.hip).  Built with -ffp-contract=off.
//
// A query is given as stored rows: positive examples and, optionally, negative ones.  Its vector is
// built on the device, q = (float)(mean of the positives), or (float)((mp + mp) - mn) with negatives,
// element by element in fp64 in list order (cosine: each row divided by its canonical norm), and the
// answer is what a search for q ranks, the examples left out.  Three steps per call, all queued on
// one stream:
//   1. recommend_build_kernel, one workgroup per query, builds q and the query's flag;
//   2. the ordinary certified search fetches the best k' = k + E rows of every q with their keys;
//   3. recommend_select_kernel, one wave per query, drops the examples from the fetched list in
//      order (a ballot and a prefix popcount give the output slot) and writes the first k.
// One atomic per flagged query; the only LDS is what the workgroup-wide OR of the build needs.  The
// element step, the list state, the membership test and the keep rule are vdb_recommend_plan.h's.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_recommend_plan.h"

namespace vdb {

// The clamped lists of query b: pointers to its ids and their numbers.
struct RecLists {
    const int64_t* pos;
    const int64_t* neg;
    int64_t np, nn;
};
__device__ __forceinline__ RecLists rec_lists(const RecommendArgs& a, size_t b) {
    RecLists l;
    const RecRange p = rec_range(a.pos_offs[b], a.pos_offs[b + 1], a.n_pos);
    l.pos = a.pos_rows + p.o0;
    l.np = p.o1 - p.o0;
    l.neg = a.neg_rows;
    l.nn = 0;
    if (a.neg_offs) {
        const RecRange n = rec_range(a.neg_offs[b], a.neg_offs[b + 1], a.n_neg);
        l.neg = a.neg_rows + n.o0;
        l.nn = n.o1 - n.o0;
    }
    return l;
}

// ---- step 1: the built queries ----------------------------------------------------------------------------
// Grid (queries), kRecBuildThreads threads.  Writes Q[b][0 .. D) and flag[b]: 0, or the reason every
// slot of the query is "no result" (kRecListEmpty; kRecListBad for a bad list or a non-finite
// element, which also adds one to *bad).  A flagged query's vector is zeros.  Ids are checked before
// a row is read; count == 0 reads no row at all.
template <int METRIC>
__global__ void __launch_bounds__(kRecBuildThreads) recommend_build_kernel(RecommendArgs a) {
    const int t = threadIdx.x;
    const size_t b = blockIdx.x;
    const int D = a.D;
    float* q = a.Q + b * (size_t)D;
    const RecLists l = rec_lists(a, b);
    const int state = rec_list_state(l.np, l.nn);  // the same in every thread
    // thread e checks example e (a list that passed the state test has at most kRecMaxExamples)
    bool bad_id = false;
    if (state == kRecListOk && t < l.np + l.nn) {
        const int64_t id = t < l.np ? l.pos[t] : l.neg[t - l.np];
        bad_id = !rec_id_ok(id, a.count);
    }
    const bool bad_list = __syncthreads_or(bad_id ? 1 : 0) != 0;
    const bool build = state == kRecListOk && !bad_list;
    bool nonfinite = false;
    if (build) {
        const int np = (int)l.np, nn = (int)l.nn;
        for (int d = t; d < D; d += kRecBuildThreads) {
            double acc = 0.0;
            for (int e = 0; e < np; ++e) {
                const uint64_t r = (uint64_t)l.pos[e];
                acc = acc + rec_term(a.X[row_piece_offset(r, 0, a.G) + d], METRIC == 0 ? a.nrm64[r] : 1.0, METRIC);
            }
            const double mp = rec_mean(acc, np);
            double mn = 0.0;
            if (nn > 0) {
                double accn = 0.0;
                for (int e = 0; e < nn; ++e) {
                    const uint64_t r = (uint64_t)l.neg[e];
                    accn = accn + rec_term(a.X[row_piece_offset(r, 0, a.G) + d], METRIC == 0 ? a.nrm64[r] : 1.0, METRIC);
                }
                mn = rec_mean(accn, nn);
            }
            const float v = rec_combine(mp, mn, nn > 0);
            nonfinite = nonfinite || !rec_finite(v);
            q[d] = v;
        }
    }
    const bool any_nonfinite = __syncthreads_or(nonfinite ? 1 : 0) != 0;
    const bool flagged = !build || any_nonfinite;
    if (flagged)  // (each thread rewrites the elements it wrote itself)
        for (int d = t; d < D; d += kRecBuildThreads) q[d] = 0.0f;
    if (t == 0) {
        const int f = !flagged ? 0 : state == kRecListEmpty ? kRecListEmpty : kRecListBad;
        a.flag[b] = f;
        if (f == kRecListBad) atomicAdd(a.bad, 1ull);
    }
}

hipError_t launch_recommend_build(int metric, const RecommendArgs& a, int n_queries, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (!a.pos_offs || !a.Q || !a.flag || !a.bad || a.D < 1 || a.n_pos < 0 || a.n_neg < 0 || a.count < 0 ||
        (a.n_pos > 0 && !a.pos_rows) || (a.neg_offs && a.n_neg > 0 && !a.neg_rows) ||
        (a.count > 0 && (!a.X || (metric == 0 && !a.nrm64))))
        return hipErrorInvalidValue;
    if (metric == 0)
        hipLaunchKernelGGL((recommend_build_kernel<0>), dim3(n_queries), dim3(kRecBuildThreads), 0, st, a);
    else
        hipLaunchKernelGGL((recommend_build_kernel<1>), dim3(n_queries), dim3(kRecBuildThreads), 0, st, a);
    return hipGetLastError();
}

// ---- step 3: the select -----------------------------------------------------------------------------------
// One wave per query, kRecSelectWaves waves per workgroup.  Query b's fetched list fi / fk [b][k_fetch]
// (local rows, -1 = none, ranked by (key desc, row asc)) -> out_* [b][k]: its first k entries that
// are no example, "no result" after them; a flagged query is "no result" throughout.
template <int METRIC>
__global__ void __launch_bounds__(64 * kRecSelectWaves) recommend_select_kernel(RecommendArgs a, int n_queries) {
    const int lane = threadIdx.x & 63;
    const size_t b = (size_t)blockIdx.x * kRecSelectWaves + (threadIdx.x >> 6);
    if (b >= (size_t)n_queries) return;  // (whole waves; no workgroup barrier below)
    const int F = a.k_fetch;
    const int K = a.k;
    float* os = a.out_s + b * K;
    int64_t* oi = a.out_i + b * K;
    double* ok = a.out_k ? a.out_k + b * K : nullptr;
    int kept = 0;
    if (a.flag[b] == 0) {  // an unflagged query has 1 .. kRecMaxExamples examples
        const RecLists l = rec_lists(a, b);
        const int np = (int)l.np, nn = (int)l.nn;
        const int64_t* c = a.fi + b * F;
        const double* fk = a.fk + b * F;
#pragma unroll
        for (int t = 0; t < kRecLanePos; ++t) {
            const int p = lane + 64 * t;
            const int64_t r = p < F ? c[p] : (int64_t)-1;
            const bool keep = rec_keep(r, a.count, l.pos, np, l.neg, nn);
            const unsigned long long m = __ballot(keep);
            const int slot = kept + __popcll(m & ((1ull << lane) - 1ull));
            if (keep && slot < K)
                write_result(METRIC, fk[p], (uint64_t)r + (uint64_t)a.index_offset, true, os + slot, oi + slot,
                             ok ? ok + slot : nullptr);
            kept += __popcll(m);
        }
    }
    for (int e = (kept < K ? kept : K) + lane; e < K; e += 64)
        write_result(METRIC, -INFINITY, 0, false, os + e, oi + e, ok ? ok + e : nullptr);
}

hipError_t launch_recommend_select(int metric, const RecommendArgs& a, int n_queries, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (a.k < 1 || a.k > kRecMaxK || a.k_fetch < a.k || a.k_fetch > kRecMaxFetch || !a.pos_offs || !a.flag || !a.fi ||
        !a.fk || !a.out_s || !a.out_i || a.n_pos < 0 || a.n_neg < 0 || (a.n_pos > 0 && !a.pos_rows) ||
        (a.neg_offs && a.n_neg > 0 && !a.neg_rows))
        return hipErrorInvalidValue;
    const dim3 grid((n_queries + kRecSelectWaves - 1) / kRecSelectWaves);
    if (metric == 0)
        hipLaunchKernelGGL((recommend_select_kernel<0>), grid, dim3(64 * kRecSelectWaves), 0, st, a, n_queries);
    else
        hipLaunchKernelGGL((recommend_select_kernel<1>), grid, dim3(64 * kRecSelectWaves), 0, st, a, n_queries);
    return hipGetLastError();
}

}  // namespace vdb
