// vdb_sparse_query.h: what the two sparse search kernels (vdb_sparse.hip sparse_kernel, row-major;
// vdb_sparse_inv.hip sparse_inv_kernel, term-major) do alike: loading and judging a query, the "no
// result" fill, writing a result slot, and the tail from the four waves' top-k lists to the results
// (wave 0's fold, the per-segment lists, the per-query counter, the last workgroup's merge).
#pragma once
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_sparse_plan.h"

namespace vdb {

__device__ __forceinline__ void sparse_write(const SparseArgs& a, int b, int e, double key, uint32_t r) {
    const bool valid = r != 0xFFFFFFFFu;
    const size_t o = (size_t)b * a.out_ld + e;
    // (metric 0 of write_result: the score is (float)key, round to nearest even)
    write_result(0, key, valid ? (uint64_t)r + (uint64_t)a.index_offset : 0, valid, a.out_s + o, a.out_i + o,
                 a.out_k ? a.out_k + o : nullptr);
}

// Query b's entries into LDS (qt / qw, kSparseMaxQueryTerms each); every workgroup of the query reads
// and judges them alike, segment s == 0 counts a bad one in *a.bad.  All 256 threads call it; it ends
// in a workgroup barrier, after which the query is in LDS.  -> the entries read (0 for a bad range);
// *bad: the query is answered with "no result".
__device__ __forceinline__ int sparse_load_query(const SparseArgs& a, int b, int s, int32_t* qt, float* qw, bool* bad_out) {
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
    *bad_out = bad;
    return len;
}

// "no result" in every slot of query b (a bad query, one without terms, or no rows).
__device__ __forceinline__ void sparse_fill_none(const SparseArgs& a, int b) {
    for (int e = threadIdx.x; e < a.k; e += 256) sparse_write(a, b, e, -INFINITY, 0xFFFFFFFFu);
}

// The tail of segment s of query b, `live` segments of n_seg having rows: every wave's tk is finished
// here; wave 0 (its tk, over buffers kbase / ibase of `cap` entries a wave) folds the four lists; the
// only list of a query goes straight to the results, otherwise to the segment's slot of a.lk / a.li,
// and the workgroup that finishes the query last merges the `live` lists and writes the results
// (release: wave 0's list stores before the count; acquire: the other lists after it; the counter is
// left zero).  All 256 threads call it; tkmem: the top-k buffers, reused by the merge.
__device__ __forceinline__ void sparse_finish(const SparseArgs& a, WaveTopK<double, uint32_t>& tk, double* kbase,
                                              uint32_t* ibase, int cap, int b, int s, int n_seg, int live, char* tkmem) {
    const int KE = a.KE;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    double* bk = kbase + (size_t)wv * cap;
    uint32_t* bi = ibase + (size_t)wv * cap;
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

}  // namespace vdb
