// vdb_sparse.hip: the sparse column and the exact sparse search (vdb_index_set_sparse,
// vdb_index_search_sparse, and the sparse list of vdb_index_search_hybrid), part of the gfx950
// kernels of the brute-force distance + top-k path (pipeline overview: vdb_scan.hip).  Built with
// -ffp-contract=off.
//
// Every stored row carries a sparse vector in CSR form: indptr [n + 1] and interleaved (term, weight)
// pairs, 8 bytes each, ascending term ids within a row.  A query is up to 1 024 such pairs.  The key
// of row r is the fp64 dot product of the two, summed over the row's entries in stored order.
//
// sparse_kernel has the shape of the row-list scan (vdb_subset.hip): grid (n_seg, n_queries), 4
// waves; segment s walks chunks s, s + n_seg, ... of the rows (vdb_sparse_plan.h).  What differs is
// the key: one lane takes one row and walks its entries in order, so the sum has one order by
// construction and needs no cross-lane reduction.  The query's terms and weights sit in LDS and a
// lane finds a stored term among them by binary search.  The lane offers (matched and mask bit, key,
// row) to its wave's WaveTopK; wave 0 folds the four, and the workgroup that finishes a query last
// merges the segments' lists and writes the results (a per-query counter, release / acquire fences
// around it, left zero on exit).
//
// Device-memory calls are not validated on the host, so the kernel takes any query: offsets are
// clamped to [0, q_nnz], and a query whose range is bad or that holds a term id out of range or not
// above its predecessor, or a non-finite weight, gives "no result" in every slot and is counted in
// *bad.  The column itself was validated when it was attached.  Query handling and the tail are in
// vdb_sparse_query.h, shared with the inverted (term-major) form of this search (vdb_sparse_inv.hip),
// which gives the same result in every byte.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_sparse_plan.h"
#include "vdb_sparse_query.h"

namespace vdb {

// ---- the column -------------------------------------------------------------------------------
// Two passes, one thread per row each; flags |= the causes found.  The first checks the offsets
// alone.  The second walks the rows' entries and does so only when the first found every offset good
// (the flag word is still zero: the launches are ordered on one stream), so that the rows tile [0,
// nnz): nothing outside [0, nnz) of terms / weights is read, and no entry twice, whatever indptr holds.
__global__ void __launch_bounds__(256) sparse_validate_offsets_kernel(const int64_t* indptr, int64_t n, int64_t nnz,
                                                                      uint32_t* flags) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    if (!sparse_column_offsets_ok(indptr, r, n, nnz)) atomicOr(flags, sparse_column_flag(kSparseColBadIndptr));
}
__global__ void __launch_bounds__(256) sparse_validate_entries_kernel(const int64_t* indptr, const int32_t* terms,
                                                                      const float* weights, int64_t n, int32_t n_terms,
                                                                      uint32_t* flags) {
    if (*flags & sparse_column_flag(kSparseColBadIndptr)) return;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int c = sparse_column_row(indptr, terms, weights, r, n_terms);
    if (c != kSparseColOk) atomicOr(flags, sparse_column_flag(c));
}

__global__ void __launch_bounds__(256) sparse_pack_kernel(const int32_t* terms, const float* weights, int64_t nnz,
                                                          SparsePair* pairs) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    SparsePair p;
    p.term = terms[e];
    p.weight = weights[e];
    pairs[e] = p;
}

hipError_t launch_sparse_validate(const int64_t* indptr, const int32_t* terms, const float* weights, int64_t n,
                                  int64_t nnz, int32_t n_terms, uint32_t* flags, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(sparse_validate_offsets_kernel, grid, dim3(256), 0, st, indptr, n, nnz, flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || nnz <= 0) return e;
    hipLaunchKernelGGL(sparse_validate_entries_kernel, grid, dim3(256), 0, st, indptr, terms, weights, n, n_terms, flags);
    return hipGetLastError();
}

hipError_t launch_sparse_pack(const int32_t* terms, const float* weights, int64_t nnz, SparsePair* pairs,
                              hipStream_t st) {
    if (nnz <= 0) return hipSuccess;
    hipLaunchKernelGGL(sparse_pack_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, terms, weights, nnz,
                       pairs);
    return hipGetLastError();
}

// ---- the search -------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sparse_kernel(SparseArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
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

    // this query's entries, loaded and judged (vdb_sparse_query.h)
    bool bad;
    const int len = sparse_load_query(a, b, s, qt, qw, &bad);
    const int live = (bad || len == 0) ? 0 : sparse_live_segs(a.N, n_seg);
    if (live == 0) {  // a bad query, one without terms, or no rows: "no result" in every slot
        if (s == 0) sparse_fill_none(a, b);
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do, and not counted below

    WaveTopK<double, uint32_t> tk;
    tk.init(kbase + (size_t)wv * cap, ibase + (size_t)wv * cap, KE);
    const int64_t n_chunks = sparse_n_chunks(a.N);
    for (int64_t c = s; c < n_chunks; c += n_seg) {
        const int64_t row = sparse_row_of(c, wv, lane);
        const bool in = row < a.N;
        double acc = 0.0;
        bool matched = false;
        if (in) {
            const int64_t e0 = a.indptr[row], e1 = a.indptr[row + 1];
            for (int64_t e = e0; e < e1; ++e) {
                const SparsePair p = a.pairs[e];
                const int j = sparse_find(qt, len, p.term);
                if (j >= 0) {
                    const double qd = (double)qw[j];
                    acc = sparse_step(acc, p.weight, qd);
                    matched = matched || sparse_entry_matches(p.weight, qd);
                }
            }
            if (a.mask) matched = matched && ((a.mask[row >> 5] >> (row & 31)) & 1u);
        }
        tk.offer(in && matched, acc, in ? (uint32_t)row : 0xFFFFFFFFu);
    }
    // fold, per-segment lists, the last workgroup's merge (vdb_sparse_query.h)
    sparse_finish(a, tk, kbase, ibase, cap, b, s, n_seg, live, tkmem);
}

size_t sparse_search_lds_bytes(int KE, int n_seg) {
    return (size_t)sparse_lds_bytes(WaveTopK<double, uint32_t>::capacity(KE),
                                    n_seg > 1 ? (int64_t)merge_block_lds<double, uint32_t>(KE) : 0);
}

hipError_t launch_sparse_search(const SparseArgs& a, int n_queries, int n_seg, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (n_seg < 1 || n_seg > kSparseMaxSeg || a.k < 1 || a.k > a.KE || a.KE > kSparseMaxK || a.N < 0 || a.out_ld < a.k ||
        a.q_nnz < 0 || a.n_terms < 1 || !a.q_indptr || (a.q_nnz > 0 && (!a.q_terms || !a.q_weights)) ||
        (a.N > 0 && (!a.indptr || !a.pairs)) || !a.out_s || !a.out_i ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi || !a.done)))
        return hipErrorInvalidValue;
    const size_t lds = sparse_search_lds_bytes(a.KE, n_seg);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    if (lds > 65536) {  // (k above 256: set per launch, for the device that is current)
        const hipError_t e = hipFuncSetAttribute((const void*)sparse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sparse_kernel, dim3(n_seg, n_queries), dim3(256), lds, st, a);
    return hipGetLastError();
}

// ---- the hybrid call's sets ---------------------------------------------------------------------
// Set b of the fuse kernel is lists 2 b (dense) and 2 b + 1 (sparse): offs [B + 1] = 0, 2, 4, ...,
// weights [2 B] = (w_dense, w_sparse) per set.
__global__ void __launch_bounds__(256) hybrid_sets_kernel(int64_t* offs, double* weights, int n_queries, double w_dense,
                                                          double w_sparse) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b > n_queries) return;
    offs[b] = 2 * (int64_t)b;
    if (b < n_queries) {
        weights[2 * (size_t)b] = w_dense;
        weights[2 * (size_t)b + 1] = w_sparse;
    }
}

hipError_t launch_hybrid_sets(int64_t* offs, double* weights, int n_queries, double w_dense, double w_sparse,
                              hipStream_t st) {
    if (n_queries < 0 || !offs || !weights) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hybrid_sets_kernel, dim3((unsigned)(n_queries / 256 + 1)), dim3(256), 0, st, offs, weights, n_queries,
                       w_dense, w_sparse);
    return hipGetLastError();
}

}  // namespace vdb
