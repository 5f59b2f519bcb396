// vdb_hybsum.hip: the weighted-sum hybrid search (vdb_index_search_hybrid_sum), part of the gfx950
// kernels of the brute-force distance + top-k path (pipeline overview: vdb_scan.hip).  Built with
// -ffp-contract=off.
//
// A row is ranked by c = (w_dense * kd + w_sparse * ks) + 0.0 (vdb_hybsum_plan.h hybsum_combine): kd
// the canonical fp64 dense key (vdb_exact_keys.h), ks the sparse key (vdb_sparse_plan.h).  Every row
// below count whose mask bit is set is a candidate, whether it shares a term with the query or not.
//
// hybsum_kernel has the shape of sparse_kernel (vdb_sparse.hip): grid (n_seg, n_queries), 4 waves;
// segment s walks chunks s, s + n_seg, ... of 256 rows and wave w takes 64 consecutive rows of the
// chunk.  Per trip a wave forms both keys of its 64 rows.  First every lane walks its own row's
// entries in stored order against the query's terms in LDS, as the sparse search does.  Then the wave
// forms the dense keys of the same rows four at a time, all lanes on each row (one coalesced read of
// the fp32 rows), and lane 4 t + u keeps the key of row u of batch t, which is its own row.  Every
// lane combines its two keys and the wave makes one offer to its WaveTopK.  The tail is the sparse
// search's: wave 0 folds the four lists, and the workgroup that finishes a query last merges the
// segments' lists and writes the results (a per-query counter, release / acquire fences around it,
// left zero on exit).
//
// hybsum_parts_kernel runs only when the caller wants the two keys of the returned rows: one wave per
// output slot recomputes them with the same device functions.
//
// Device-memory calls are not validated on the host: the sparse query is clamped and judged as the
// sparse kernel does it (a bad query: "no result" in every slot, counted in *bad); a query without
// terms is good and ranks by its dense key.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_exact_keys.h"
#include "vdb_merge_block.h"
#include "vdb_hybsum_plan.h"

namespace vdb {

__device__ __forceinline__ void hybsum_write(const HybsumArgs& a, int b, int e, double key, uint32_t r) {
    const bool valid = r != 0xFFFFFFFFu;
    const size_t o = (size_t)b * a.k + e;
    // (metric 0 of write_result: the score is (float)key, round to nearest even)
    write_result(0, key, valid ? (uint64_t)r + (uint64_t)a.index_offset : 0, valid, a.out_s + o, a.out_i + o,
                 a.out_f ? a.out_f + o : nullptr);
    if (a.out_r) a.out_r[o] = r;
}

// The sparse key of one row: its entries in stored order against the query's len ascending terms.
__device__ __forceinline__ double hybsum_sparse_key(const int64_t* __restrict__ indptr, const SparsePair* __restrict__ pairs,
                                                    int64_t row, const int32_t* qt, const float* qw, int len) {
    double acc = 0.0;
    const int64_t e0 = indptr[row], e1 = indptr[row + 1];
    for (int64_t e = e0; e < e1; ++e) {
        const SparsePair p = pairs[e];
        const int j = sparse_find(qt, len, p.term);
        if (j >= 0) acc = sparse_step(acc, p.weight, (double)qw[j]);
    }
    return acc;
}

// MP: 4 / 8 = rows of up to 256 MP dims with every piece of a batch in flight; 0 = any length, one
// piece per row in flight per trip.
template <int METRIC, int MP>
__global__ void __launch_bounds__(256) hybsum_kernel(HybsumArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NB = kHybsumNB;
    const int KE = a.KE;
    const int cap = WaveTopK<double, uint32_t>::capacity(KE);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int s = blockIdx.x;
    const int n_seg = (int)gridDim.x;
    // LDS: the query's terms and weights, then the top-k buffers (the tail merge reuses those)
    int32_t* qt = reinterpret_cast<int32_t*>(smem);
    float* qw = reinterpret_cast<float*>(smem + (size_t)kSparseMaxQueryTerms * sizeof(int32_t));
    char* tkmem = smem + kSparseQueryLds;
    double* kbase = reinterpret_cast<double*>(tkmem);
    uint32_t* ibase = reinterpret_cast<uint32_t*>(tkmem + (size_t)kSparseWaves * cap * sizeof(double));
    double* bk = kbase + (size_t)wv * cap;
    uint32_t* bi = ibase + (size_t)wv * cap;

    // this query's sparse entries (every workgroup of the query reads and judges them alike)
    const SparseQRange rg = sparse_query_range(a.q_indptr[b], a.q_indptr[b + 1], a.q_nnz);
    const int len = rg.len;
    bool bad_e = false;
    for (int e = threadIdx.x; e < len; e += 256) {
        const int32_t t = a.q_terms[rg.o0 + e];
        const int32_t prev = e > 0 ? a.q_terms[rg.o0 + e - 1] : -1;
        const float w = a.q_weights[rg.o0 + e];
        bad_e = bad_e || !sparse_term_ok(t, prev, a.n_terms) || !sparse_weight_ok(w);
        qt[e] = t;
        qw[e] = w;
    }
    const bool bad = __syncthreads_or(bad_e ? 1 : 0) != 0 || rg.bad;  // (also: the query is in LDS)
    if (bad && s == 0 && threadIdx.x == 0 && a.bad) atomicAdd(a.bad, 1ull);
    const int live = bad ? 0 : sparse_live_segs(a.N, n_seg);  // (a query without terms is live)
    if (live == 0) {  // a bad query, or no rows: "no result" in every slot
        if (s == 0)
            for (int e = threadIdx.x; e < a.k; e += 256) hybsum_write(a, b, e, -INFINITY, 0xFFFFFFFFu);
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do, and not counted below

    const float* q = a.Q + (int64_t)b * a.D;
    const double qn = a.qn64[b];
    const int np = (a.D + 255) / 256;
    WaveTopK<double, uint32_t> tk;
    tk.init(bk, bi, KE);
    const int64_t n_chunks = sparse_n_chunks(a.N);
    for (int64_t c = s; c < n_chunks; c += n_seg) {
        const int64_t row = sparse_row_of(c, wv, lane);
        bool elig = row < a.N;
        if (elig && a.mask) elig = (a.mask[row >> 5] >> (row & 31)) & 1u;
        // the sparse key: a row out of range or masked out walks nothing
        const double ks = (elig && len > 0) ? hybsum_sparse_key(a.indptr, a.pairs, row, qt, qw, len) : 0.0;
        // the dense keys of the wave's 64 rows, NB at a time (em: the eligible lanes, wave-uniform)
        const unsigned long long em = __ballot(elig);
        const int64_t w0 = sparse_row_of(c, wv, 0);
        double kd = 0.0;
        for (int t = 0; t < kSparseWaveRows / NB; ++t) {
            const unsigned g = (unsigned)(em >> (t * NB)) & ((1u << NB) - 1u);
            if (g == 0) continue;  // no eligible row in this batch: nothing is read
            const int first = __builtin_ctz(g);
            uint32_t rws[NB];
            double xn[NB];
            bool ok[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                ok[u] = (g >> u) & 1u;
                // (an ineligible row is not read: the held form skips it; the any-length form reads an
                // eligible row of the batch in its place and its key is dropped)
                rws[u] = (uint32_t)(w0 + t * NB + (ok[u] ? u : first));
                xn[u] = METRIC == 0 ? a.nrm64[rws[u]] : 1.0;
            }
            double keys[NB];
            if constexpr (MP > 0) {
                // exact_keys_rows' arithmetic in its two halves, which take ok[]
                f32x4 xv[MP][NB];
                rows_pieces_load<NB, MP>(a.X, a.G, np, rws, ok, xv);
                exact_keys_held<METRIC, NB, MP>(q, a.D, qn, np, xv, xn, keys);
            } else {
                exact_keys_batch<METRIC, NB>(q, qn, a.X, a.G, a.D, rws, xn, NB, keys);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u)
                if (lane == t * NB + u) kd = keys[u];
        }
        const double cv = hybsum_combine(a.w_dense, kd, a.w_sparse, ks);
        tk.offer(elig, cv, elig ? (uint32_t)row : 0xFFFFFFFFu);
    }
    tk.finish();
    __syncthreads();
    if (wv == 0) {
        for (int w = 1; w < kSparseWaves; ++w) {
            const double* ok = kbase + (size_t)w * cap;
            const uint32_t* oi = ibase + (size_t)w * cap;
            for (int e0 = 0; e0 < KE; e0 += 64) {
                const int e = e0 + lane;
                const bool inb = e < KE && oi[e] != 0xFFFFFFFFu;
                tk.offer(inb, inb ? ok[e] : -INFINITY, inb ? oi[e] : 0xFFFFFFFFu);
            }
        }
        tk.finish();
        if (live == 1) {  // the only list of this query: straight to the results
            for (int e = lane; e < a.k; e += 64) hybsum_write(a, b, e, e < KE ? bk[e] : -INFINITY, e < KE ? bi[e] : 0xFFFFFFFFu);
        } else {
            const size_t base = ((size_t)b * n_seg + s) * KE;
            for (int e = lane; e < KE; e += 64) {
                a.lk[base + e] = bk[e];
                a.li[base + e] = bi[e];
            }
        }
    }
    if (live == 1) return;
    __syncthreads();  // wave 0's list stores are issued; the LDS buffers are free for the merge
    // the last workgroup of this query merges its `live` lists (release: wave 0's list stores
    // before the count; acquire: the other lists after it)
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = atomicAdd(a.done + b, 1) == live - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    const size_t q0 = (size_t)b * n_seg * KE;
    merge_block<double, uint32_t>(a.lk + q0, a.li + q0, live, KE, KE, KE, a.mk + (size_t)b * KE, a.mi + (size_t)b * KE,
                                  tkmem);
    __syncthreads();
    for (int e = threadIdx.x; e < a.k; e += 256) hybsum_write(a, b, e, a.mk[(size_t)b * KE + e], a.mi[(size_t)b * KE + e]);
    if (threadIdx.x == 0) a.done[b] = 0;  // left zero for the next call on this workspace
}

// One wave per output slot: the two keys of the row the slot holds (out_r, written by hybsum_kernel on
// the same stream), -inf for an empty slot.  A slot that holds a row belongs to a query the kernel
// judged good, so its range is in bounds and its terms ascend; the range is clamped all the same.
template <int METRIC>
__global__ void __launch_bounds__(256) hybsum_parts_kernel(HybsumArgs a, int64_t n_slots) {
    const int lane = threadIdx.x & 63;
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= n_slots) return;
    const int b = (int)(slot / a.k);
    const uint32_t r = a.out_r[slot];
    double kd = -INFINITY, ks = -INFINITY;
    if (r != 0xFFFFFFFFu && (int64_t)r < a.N) {
        const SparseQRange rg = sparse_query_range(a.q_indptr[b], a.q_indptr[b + 1], a.q_nnz);
        ks = rg.len > 0 ? hybsum_sparse_key(a.indptr, a.pairs, (int64_t)r, a.q_terms + rg.o0, a.q_weights + rg.o0, rg.len) : 0.0;
        kd = exact_key<METRIC>(a.Q + (int64_t)b * a.D, a.qn64[b], a.X, a.G, a.D, (uint64_t)r,
                               METRIC == 0 ? a.nrm64[r] : 1.0);
    }
    if (lane == 0) {
        if (a.out_d) a.out_d[slot] = kd;
        if (a.out_p) a.out_p[slot] = ks;
    }
}

size_t hybsum_search_lds_bytes(int KE, int n_seg) {
    return (size_t)hybsum_lds_bytes(WaveTopK<double, uint32_t>::capacity(KE),
                                    n_seg > 1 ? (int64_t)merge_block_lds<double, uint32_t>(KE) : 0);
}

hipError_t launch_hybsum_search(int metric, const HybsumArgs& a, int n_queries, int n_seg, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (n_queries > kHybsumMaxQueries || n_seg < 1 || n_seg > kHybsumMaxSeg || a.k < 1 || a.k > a.KE ||
        a.KE > kHybsumMaxK || a.N < 0 || a.D < 1 || a.q_nnz < 0 || a.n_terms < 1 || !a.q_indptr ||
        (a.q_nnz > 0 && (!a.q_terms || !a.q_weights)) ||
        (a.N > 0 && (!a.indptr || !a.pairs || !a.Q || !a.qn64 || !a.X || (metric == 0 && !a.nrm64))) || !a.out_s ||
        !a.out_i || (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi || !a.done)) || ((a.out_d || a.out_p) && !a.out_r))
        return hipErrorInvalidValue;
    const size_t lds = hybsum_search_lds_bytes(a.KE, n_seg);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const dim3 grid(n_seg, n_queries);
    const int mp = hybsum_mp(a.D);
#define VDB_HYBSUM(M, MPV)                                                                                          \
    if (metric == M && mp == MPV) {                                                                                 \
        if (lds > 65536) { /* (k above 256: set per launch, for the device that is current) */                     \
            const hipError_t e = hipFuncSetAttribute((const void*)hybsum_kernel<M, MPV>,                            \
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);         \
            if (e != hipSuccess) return e;                                                                          \
        }                                                                                                           \
        hipLaunchKernelGGL((hybsum_kernel<M, MPV>), grid, dim3(256), lds, st, a);                                   \
        return hipGetLastError();                                                                                   \
    }
    VDB_HYBSUM(0, 4) VDB_HYBSUM(0, 8) VDB_HYBSUM(0, 0)
    VDB_HYBSUM(1, 4) VDB_HYBSUM(1, 8) VDB_HYBSUM(1, 0)
#undef VDB_HYBSUM
    return hipErrorInvalidValue;
}

hipError_t launch_hybsum_parts(int metric, const HybsumArgs& a, int n_queries, hipStream_t st) {
    if (n_queries <= 0 || (!a.out_d && !a.out_p)) return hipSuccess;
    if (!a.out_r || a.k < 1 || !a.q_indptr || (a.N > 0 && (!a.indptr || !a.pairs || !a.Q || !a.qn64 || !a.X)))
        return hipErrorInvalidValue;
    const int64_t n_slots = (int64_t)n_queries * a.k;
    const dim3 grid((unsigned)((n_slots + 3) / 4));
    if (metric == 0)
        hipLaunchKernelGGL(hybsum_parts_kernel<0>, grid, dim3(256), 0, st, a, n_slots);
    else
        hipLaunchKernelGGL(hybsum_parts_kernel<1>, grid, dim3(256), 0, st, a, n_slots);
    return hipGetLastError();
}

}  // namespace vdb
