// vdb_sparse_inv.hip: the inverted (term-major) form of the exact sparse search, a second kernel
// behind vdb_index_search_sparse and the sparse list of vdb_index_search_hybrid, and the build of the
// postings it reads (vdb_index_set_sparse).  Part of the gfx950 kernels of the brute-force distance +
// top-k path (pipeline overview: vdb_scan.hip; the row-major form: vdb_sparse.hip).  Built with
// -ffp-contract=off.  Every result is equal in every byte to sparse_kernel's.
//
// The postings are the column again in (term ascending, row ascending) order: tptr [n_terms + 1]
// and posts [nnz] of (row, weight), 8 bytes each.  A query of 32 terms can only score the postings of
// its 32 terms, so the kernel walks those and nothing else.
//
// Why the bytes are the same.  The contract's key of row r is acc = 0.0; acc = acc + (double)w_e *
// qd[t_e] over the row's entries in stored order, restricted to the terms the query lists.  Term ids
// ascend within a stored row and within a query, and a row appears at most once in a term's
// postings.  So a unit that alone owns r, walks the query's terms in ascending order and adds each
// term's posting for r into one accumulator performs exactly those adds in that order.  Here the
// unit is a WAVE: it owns a quarter of a row block, the accumulators and matched flags of those rows
// sit in LDS and no other wave touches them, and a wave's LDS operations complete in program order.
// No atomic add is needed, and two postings of one term never meet in one accumulator (within one
// term every address is distinct).
//
// sparse_inv_kernel: grid (n_seg, n_queries), 4 waves, as sparse_kernel.  The rows are cut into
// blocks of R rows (R = sparse_inv_block_rows(KE), vdb_sparse_inv_plan.h: 8192, at KE = 1024 4096);
// segment s takes blocks s, s + n_seg, ... and keeps its four WaveTopK across them, so the lists per
// query and the merge tail are sparse_kernel's at any N.  Per block, wave w with rows [lo, hi):
//   1. ranges.  64 of the query's terms at a time, one a lane: two lower bounds by row inside the
//      term's postings give the part that falls in [lo, hi).  The 64 searches are independent loads in
//      flight at once; their results stay in registers (no LDS).
//   2. adds.  The non-empty ranges in ascending term order (a ballot, then lane broadcasts): the
//      lanes stride over a range with 8-byte loads, each posting does acc[row] = sparse_step(acc[row],
//      w, qd) as a plain LDS read-modify-write and, if it matches, an LDS OR into the row's flag bit.
//      The next non-empty term's first load is issued before the current term's adds.
//   3. offers.  The wave's rows 64 at a time to its WaveTopK as (matched and mask bit, acc, row); a
//      group with no flag is skipped whole; accumulators and flags are cleared on the way.  (A row that
//      was added to but never matched holds +0.0: every product was +-0 and 0.0 + -0.0 = +0.0.)
// No workgroup barrier between the query load and the tail.  Query handling and the tail are
// sparse_kernel's (vdb_sparse_query.h).
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_sparse_inv_plan.h"
#include "vdb_sparse_query.h"

namespace vdb {

// ---- the build ------------------------------------------------------------------------------------
// One thread per stored entry e: its row is the last r with indptr[r] <= e; key = the term, value =
// the posting (row in the low word, the weight's bits in the high one).
__global__ void __launch_bounds__(256) sparse_inv_entries_kernel(const int64_t* indptr, const SparsePair* pairs, int64_t n,
                                                                 int64_t nnz, uint32_t* keys, unsigned long long* vals) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nnz) return;
    int64_t lo = 0, hi = n;  // the first r in [0, n] with indptr[r] > e, minus one
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (indptr[mid + 1] <= e)
            lo = mid + 1;
        else
            hi = mid;
    }
    const SparsePair p = pairs[e];
    keys[e] = (uint32_t)p.term;
    vals[e] = (unsigned long long)(uint32_t)lo | ((unsigned long long)__float_as_uint(p.weight) << 32);
}
// One thread per t in [0, n_terms]: tptr[t] = the first sorted entry whose term is >= t.
__global__ void __launch_bounds__(256) sparse_inv_tptr_kernel(const uint32_t* sorted, int64_t nnz, int32_t n_terms,
                                                              int64_t* tptr) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > n_terms) return;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)sorted[mid] < t)
            lo = mid + 1;
        else
            hi = mid;
    }
    tptr[t] = lo;
}

hipError_t launch_sparse_inv_build(const int64_t* indptr, const SparsePair* pairs, int64_t n, int64_t nnz, int32_t n_terms,
                                   int64_t* tptr, SparsePost* posts, hipStream_t st) {
    if (n < 0 || nnz < 0 || n_terms < 1 || n_terms > kSparseInvMaxTerms || !tptr || (nnz > 0 && (!indptr || !pairs || !posts)))
        return hipErrorInvalidValue;
    uint32_t *keys = nullptr, *sorted = nullptr;
    unsigned long long* vals = nullptr;
    void* temp = nullptr;
    const auto run = [&]() -> hipError_t {
        hipError_t e = hipSuccess;
        if (nnz > 0) {
            const size_t cnt = (size_t)nnz;
            if ((e = hipMalloc(&keys, cnt * 4)) != hipSuccess) return e;
            if ((e = hipMalloc(&sorted, cnt * 4)) != hipSuccess) return e;
            if ((e = hipMalloc(&vals, cnt * 8)) != hipSuccess) return e;
            hipLaunchKernelGGL(sparse_inv_entries_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, indptr, pairs,
                               n, nnz, keys, vals);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            // a stable sort by term of entries in row order: (term, row) order
            unsigned long long* out = reinterpret_cast<unsigned long long*>(posts);
            const unsigned bits = (unsigned)sparse_inv_term_bits(n_terms);
            size_t temp_bytes = 0;
            if ((e = rocprim::radix_sort_pairs(nullptr, temp_bytes, keys, sorted, vals, out, cnt, 0u, bits, st)) != hipSuccess)
                return e;
            if ((e = hipMalloc(&temp, temp_bytes > 0 ? temp_bytes : 1)) != hipSuccess) return e;
            if ((e = rocprim::radix_sort_pairs(temp, temp_bytes, keys, sorted, vals, out, cnt, 0u, bits, st)) != hipSuccess)
                return e;
        }
        hipLaunchKernelGGL(sparse_inv_tptr_kernel, dim3((unsigned)(n_terms / 256 + 1)), dim3(256), 0, st, sorted, nnz, n_terms,
                           tptr);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        return hipStreamSynchronize(st);
    };
    const hipError_t rc = run();
    if (rc != hipSuccess) (void)hipStreamSynchronize(st);  // nothing queued still reads what is freed below
    if (keys) (void)hipFree(keys);
    if (sorted) (void)hipFree(sorted);
    if (vals) (void)hipFree(vals);
    if (temp) (void)hipFree(temp);
    return rc;
}

// ---- the search -------------------------------------------------------------------------------
// One posting into its row's accumulator and flag (base: the block's first row).
__device__ __forceinline__ void sparse_inv_add(unsigned long long v, double qd, int64_t base, double* acc, uint32_t* flags) {
    const uint32_t li = (uint32_t)((int64_t)(uint32_t)v - base);
    const float w = __uint_as_float((uint32_t)(v >> 32));
    acc[li] = sparse_step(acc[li], w, qd);
    if (sparse_entry_matches(w, qd)) atomicOr(flags + (li >> 5), 1u << (li & 31));
}

__global__ void __launch_bounds__(256) sparse_inv_kernel(SparseArgs a, const int64_t* __restrict__ tptr,
                                                         const SparsePost* __restrict__ posts, int R) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int KE = a.KE;
    const int cap = WaveTopK<double, uint32_t>::capacity(KE);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int s = blockIdx.x;
    const int n_seg = (int)gridDim.x;
    // LDS (sparse_inv_lds): the query, the accumulators, the flags, the top-k buffers / merge buffer
    const SparseInvLds L = sparse_inv_lds(R, KE, n_seg > 1);
    int32_t* qt = reinterpret_cast<int32_t*>(smem);
    float* qw = reinterpret_cast<float*>(smem + (size_t)kSparseMaxQueryTerms * sizeof(int32_t));
    double* acc = reinterpret_cast<double*>(smem + L.acc);
    uint32_t* flags = reinterpret_cast<uint32_t*>(smem + L.flags);
    char* tkmem = smem + L.tk;
    double* kbase = reinterpret_cast<double*>(tkmem);
    uint32_t* ibase = reinterpret_cast<uint32_t*>(tkmem + (size_t)kSparseWaves * cap * sizeof(double));
    const unsigned long long* pv = reinterpret_cast<const unsigned long long*>(posts);

    bool bad;
    const int len = sparse_load_query(a, b, s, qt, qw, &bad);
    const int live = (bad || len == 0) ? 0 : sparse_inv_live_segs(a.N, R, n_seg);
    if (live == 0) {
        if (s == 0) sparse_fill_none(a, b);
        return;
    }
    if (s >= live) return;

    // the wave's own quarter of the accumulators and flags starts clean (and is left so per block)
    const int QR = R / kSparseWaves;
    for (int i = lane; i < QR; i += 64) acc[wv * QR + i] = 0.0;
    for (int i = lane; i < QR / 32; i += 64) flags[wv * (QR / 32) + i] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

    WaveTopK<double, uint32_t> tk;
    tk.init(kbase + (size_t)wv * cap, ibase + (size_t)wv * cap, KE);
    const int64_t n_blocks = sparse_inv_n_blocks(a.N, R);
    for (int64_t c = s; c < n_blocks; c += n_seg) {
        const SparseInvRows rows = sparse_inv_wave_rows(c, wv, R, a.N);
        if (rows.lo >= rows.hi) continue;  // (the last block: a quarter past N)
        const int64_t base = c * R;
        for (int t0 = 0; t0 < len; t0 += 64) {
            // 1. the ranges of 64 terms, one a lane
            int64_t p0 = 0, p1 = 0;
            if (t0 + lane < len) sparse_inv_range(tptr, posts, qt[t0 + lane], rows, &p0, &p1);
            unsigned long long m = __ballot(p0 < p1);
            // 2. the adds, term by term in ascending order; `n`: the next non-empty term, its first load issued
            int jn = -1;
            int64_t n0 = 0, n1 = 0;
            unsigned long long vn = 0;
            if (m) {
                jn = __ffsll((long long)m) - 1;
                m &= m - 1;
                n0 = __shfl(p0, jn);
                n1 = __shfl(p1, jn);
                if (n0 + lane < n1) vn = pv[n0 + lane];
            }
            while (jn >= 0) {
                const int j = jn;
                const int64_t c0 = n0, c1 = n1;
                const unsigned long long vc = vn;
                jn = -1;
                if (m) {
                    jn = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    n0 = __shfl(p0, jn);
                    n1 = __shfl(p1, jn);
                    if (n0 + lane < n1) vn = pv[n0 + lane];
                }
                const double qd = (double)qw[t0 + j];
                if (c0 + lane < c1) sparse_inv_add(vc, qd, base, acc, flags);
                for (int64_t p = c0 + 64 + lane; p < c1; p += 64) sparse_inv_add(pv[p], qd, base, acc, flags);
                // (one term's LDS operations before the next term's: program order, kept so for the compiler)
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        // 3. the offers, 64 rows at a time
        const int groups = (int)((rows.hi - rows.lo + 63) / 64);
        for (int g = 0; g < groups; ++g) {
            const int li = wv * QR + g * 64 + lane;
            const uint32_t word = flags[li >> 5];
            const bool matched = (word >> (li & 31)) & 1u;
            if (__ballot(matched) == 0) continue;
            const int64_t row = base + li;
            const bool in = row < a.N;
            const double key = acc[li];
            acc[li] = 0.0;
            if ((lane & 31) == 0) flags[li >> 5] = 0u;
            bool ok = in && matched;
            if (ok && a.mask) ok = (a.mask[row >> 5] >> (row & 31)) & 1u;
            tk.offer(ok, key, in ? (uint32_t)row : 0xFFFFFFFFu);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
    }
    sparse_finish(a, tk, kbase, ibase, cap, b, s, n_seg, live, tkmem);
}

size_t sparse_inv_search_lds_bytes(int KE, int n_seg) {
    const int R = sparse_inv_block_rows(KE);
    return R > 0 ? (size_t)sparse_inv_lds(R, KE, n_seg > 1).total : 0;
}

hipError_t launch_sparse_inv_search(const SparseArgs& a, const int64_t* tptr, const SparsePost* posts, int n_queries,
                                    int n_seg, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (n_seg < 1 || n_seg > kSparseMaxSeg || a.k < 1 || a.k > a.KE || a.KE > kSparseMaxK || a.N < 0 || a.out_ld < a.k ||
        a.q_nnz < 0 || a.n_terms < 1 || a.n_terms > kSparseInvMaxTerms || !a.q_indptr ||
        (a.q_nnz > 0 && (!a.q_terms || !a.q_weights)) || !tptr || (a.N > 0 && !posts) || !a.out_s || !a.out_i ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi || !a.done)))
        return hipErrorInvalidValue;
    const int R = sparse_inv_block_rows(a.KE);
    // the plan header's restatement of the top-k and merge buffer sizes must be the kernels' own
    if (R <= 0 || sparse_inv_topk_cap(a.KE) != WaveTopK<double, uint32_t>::capacity(a.KE) ||
        sparse_inv_merge_lds(a.KE) != (int64_t)merge_block_lds<double, uint32_t>(a.KE))
        return hipErrorInvalidValue;
    const size_t lds = (size_t)sparse_inv_lds(R, a.KE, n_seg > 1).total;
    if (lds > (size_t)kSparseInvLdsLimit) return hipErrorInvalidValue;
    if (lds > 65536) {  // (set per launch, for the device that is current)
        const hipError_t e = hipFuncSetAttribute((const void*)sparse_inv_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(sparse_inv_kernel, dim3(n_seg, n_queries), dim3(256), lds, st, a, tptr, posts, R);
    return hipGetLastError();
}

}  // namespace vdb
