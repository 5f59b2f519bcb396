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
// *bad.  The column itself was validated when it was attached.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_sparse_plan.h"

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
__device__ __forceinline__ void sparse_write(const SparseArgs& a, int b, int e, double key, uint32_t r) {
    const bool valid = r != 0xFFFFFFFFu;
    const size_t o = (size_t)b * a.out_ld + e;
    // (metric 0 of write_result: the score is (float)key, round to nearest even)
    write_result(0, key, valid ? (uint64_t)r + (uint64_t)a.index_offset : 0, valid, a.out_s + o, a.out_i + o,
                 a.out_k ? a.out_k + o : nullptr);
}

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
    double* bk = kbase + (size_t)wv * cap;
    uint32_t* bi = ibase + (size_t)wv * cap;

    // this query's entries (every workgroup of the query reads and judges them alike)
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
    const int live = (bad || len == 0) ? 0 : sparse_live_segs(a.N, n_seg);
    if (live == 0) {  // a bad query, one without terms, or no rows: "no result" in every slot
        if (s == 0)
            for (int e = threadIdx.x; e < a.k; e += 256) sparse_write(a, b, e, -INFINITY, 0xFFFFFFFFu);
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do, and not counted below

    WaveTopK<double, uint32_t> tk;
    tk.init(bk, bi, KE);
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
            for (int e = lane; e < a.k; e += 64) sparse_write(a, b, e, e < KE ? bk[e] : -INFINITY, e < KE ? bi[e] : 0xFFFFFFFFu);
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
    for (int e = threadIdx.x; e < a.k; e += 256) sparse_write(a, b, e, a.mk[(size_t)b * KE + e], a.mi[(size_t)b * KE + e]);
    if (threadIdx.x == 0) a.done[b] = 0;  // left zero for the next call on this workspace
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
