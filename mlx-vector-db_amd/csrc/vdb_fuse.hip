// vdb_fuse.hip: fused search (vdb_index_search_fused), part of the gfx950 kernels of the brute-force
// distance + top-k path (pipeline overview: vdb_scan.hip).  Built with -ffp-contract=off.
//
// A set of up to 16 sub-queries gets one ranked list: every sub-query's best fetch_k rows (list l,
// positions 0 .. n_l - 1 by (key desc, row asc)) are fused per row, by weighted reciprocal rank
// (RRF) or by the greatest key (MAX), and the candidates ranked by (fused desc, row asc).  Two steps
// per call on one stream:
//   1. the ordinary certified search fetches the lists of all sub-queries with their keys;
//   2. fuse_kernel, one workgroup per set:
//        a. the set's entries go into LDS as words (row << 12) | (l << 8) | p, pads for the rest;
//        b. a bitonic sort, ascending: the entries of one row are adjacent, in list order;
//        c. the thread at the head of a run walks its <= 16 entries in that order (the fp64 sum has
//           one order) and keeps (fused, row, hits) in registers;
//        d. the candidates, as (order key of fused, row | (l, p) | hits), overwrite the entries and
//           are sorted by (key desc, row asc);
//        e. the first k are written, the rest padded.
// Nothing depends on arrival order; the only atomic is the one that counts a bad set of a
// device-memory call.  The words, the sort length, the walk's arithmetic and the order are
// vdb_fuse_plan.h's.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_fuse_plan.h"

namespace vdb {

// The two bitonic sorts: L (a power of two >= 64) positions in LDS, every thread of the workgroup
// calls them.  Strides below 32 touch a pair in the order fuse_pair_first gives, so that the
// positions one 32-lane half of a wave reads at once are 32 consecutive ones, every bank once.
__device__ __forceinline__ void fuse_sort_words(uint64_t* w, int L) {
    for (int size = 2; size <= L; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = threadIdx.x; e < (L >> 1); e += blockDim.x) {
                const int lo = fuse_pair_lo(e, stride);
                const int i0 = fuse_pair_first(lo, stride);
                const int i1 = i0 == lo ? lo + stride : lo;
                const uint64_t v0 = w[i0], v1 = w[i1];
                const uint64_t vl = i0 == lo ? v0 : v1, vh = i0 == lo ? v1 : v0;  // at the lower / higher index
                const bool asc = (lo & size) == 0;
                if (asc ? vl > vh : vl < vh) {
                    w[i0] = v1;
                    w[i1] = v0;
                }
            }
            __syncthreads();
        }
}
__device__ __forceinline__ void fuse_sort_cands(uint64_t* key, uint64_t* pay, int L) {
    for (int size = 2; size <= L; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = threadIdx.x; e < (L >> 1); e += blockDim.x) {
                const int lo = fuse_pair_lo(e, stride);
                const int i0 = fuse_pair_first(lo, stride);
                const int i1 = i0 == lo ? lo + stride : lo;
                const uint64_t k0 = key[i0], k1 = key[i1];
                const uint64_t p0 = pay[i0], p1 = pay[i1];
                const bool fwd = (lo & size) == 0;
                const bool lo_first = i0 == lo;
                // the element at the higher index comes before the one at the lower index
                const bool hi_before = lo_first ? fuse_cand_before(k1, p1, k0, p0) : fuse_cand_before(k0, p0, k1, p1);
                const bool lo_before = lo_first ? fuse_cand_before(k0, p0, k1, p1) : fuse_cand_before(k1, p1, k0, p0);
                if (fwd ? hi_before : lo_before) {
                    key[i0] = k1;
                    key[i1] = k0;
                    pay[i0] = p1;
                    pay[i1] = p0;
                }
            }
            __syncthreads();
        }
}

// Grid (sets), fuse_threads(fuse_call_sort_len(n_sub, k_fetch)) threads, fuse_lds_bytes of that
// length of dynamic LDS.  Writes out_* [set][k].
template <int FUSION>
__global__ void __launch_bounds__(kFuseMaxThreads) fuse_kernel(FuseArgs a) {
    extern __shared__ __align__(16) uint64_t fuse_lds[];
    const int tid = threadIdx.x;
    const int T = blockDim.x;
    const size_t s = blockIdx.x;
    const int F = a.k_fetch;
    const int K = a.k;
    float* os = a.out_s + s * K;
    int64_t* oi = a.out_i + s * K;
    double* of = a.out_f ? a.out_f + s * K : nullptr;
    int32_t* oh = a.out_h ? a.out_h + s * K : nullptr;

    // the set's lists (the same in every thread), its weights checked by the first m threads
    const FuseRange rg = fuse_range(a.offs[s], a.offs[s + 1], a.n_sub);
    bool bad_w = false;
    if (FUSION == kFuseRrf && a.weights && tid < rg.m) bad_w = !fuse_weight_ok(a.weights[rg.o0 + tid]);
    const bool bad = __syncthreads_or(bad_w ? 1 : 0) != 0 || rg.bad;
    if (bad && tid == 0) atomicAdd(a.bad, 1ull);
    const int m = (bad || a.count <= 0) ? 0 : rg.m;
    const int L = fuse_sort_len(m * F);  // <= kFusePosPerThread * T by the launch
    const int64_t* fi = a.fi + (size_t)rg.o0 * F;
    const double* fk = a.fk + (size_t)rg.o0 * F;
    const float* fs = a.fs + (size_t)rg.o0 * F;

    uint64_t* w = fuse_lds;        // the entries, then the candidates' keys
    uint64_t* pay = fuse_lds + L;  // the candidates' payloads
    if (L > 0) {
        // a. the entries
        const int E = m * F;
        for (int e = tid; e < L; e += T) {
            uint64_t v = kFusePad;
            if (e < E) {
                const int64_t r = fi[e];
                if (r >= 0 && r < a.count) v = fuse_pack_entry((uint64_t)r, e / F, e % F);
            }
            w[e] = v;
        }
        __syncthreads();
        // b. rows together, lists ascending
        fuse_sort_words(w, L);
        // c. the head of each run fuses it
        uint64_t ck[kFusePosPerThread], cp[kFusePosPerThread];
#pragma unroll
        for (int j = 0; j < kFusePosPerThread; ++j) {
            const int i = tid + j * T;
            ck[j] = 0;
            cp[j] = kFusePad;
            if (i >= L) continue;
            const uint64_t v = w[i];
            if (v == kFusePad) continue;
            const uint64_t row = fuse_entry_row(v);
            if (i > 0 && fuse_entry_row(w[i - 1]) == row) continue;
            double fused = 0.0;
            int hits = 0, bl = 0, bp = 0;
            for (int e = i; e < L && hits < kFuseMaxLists; ++e) {
                const uint64_t x = e == i ? v : w[e];
                if (fuse_entry_row(x) != row) break;  // (a pad's row field names no row)
                const int l = fuse_entry_list(x), p = fuse_entry_pos(x);
                if (FUSION == kFuseRrf) {
                    fused = fuse_rrf_add(fused, a.weights ? a.weights[rg.o0 + l] : 1.0, a.rrf_c, p);
                } else {
                    const double kappa = fk[l * F + p];
                    if (hits == 0 || fuse_max_takes(kappa, fused)) {
                        fused = kappa;
                        bl = l;
                        bp = p;
                    }
                }
                ++hits;
            }
            ck[j] = fuse_order_key(fused);
            cp[j] = fuse_pack_cand(row, bl, bp, hits);
        }
        __syncthreads();
        // d. the candidates over the entries, ranked
#pragma unroll
        for (int j = 0; j < kFusePosPerThread; ++j) {
            const int i = tid + j * T;
            if (i < L) {
                w[i] = ck[j];
                pay[i] = cp[j];
            }
        }
        __syncthreads();
        fuse_sort_cands(w, pay, L);
    }
    // e. the slots
    for (int j = tid; j < K; j += T) {
        const uint64_t p = j < L ? pay[j] : kFusePad;
        if (p != kFusePad) {
            const int at = fuse_cand_list(p) * F + fuse_cand_pos(p);
            const double fused = FUSION == kFuseRrf ? fuse_key_value(w[j]) : fk[at];
            os[j] = FUSION == kFuseRrf ? (float)fused : fs[at];
            oi[j] = (int64_t)(fuse_cand_row(p) + (uint64_t)a.index_offset);
            if (of) of[j] = fused;
            if (oh) oh[j] = fuse_cand_hits(p);
        } else {
            os[j] = 0.0f;
            oi[j] = -1;
            if (of) of[j] = -INFINITY;
            if (oh) oh[j] = 0;
        }
    }
}

hipError_t launch_fuse(int fusion, const FuseArgs& a, int n_sets, hipStream_t st) {
    if (n_sets <= 0) return hipSuccess;
    if (a.k < 1 || a.k > kFuseMaxK || a.k_fetch < a.k || a.k_fetch > kFuseMaxFetch || a.n_sub < 0 || a.count < 0 ||
        !a.offs || !a.bad || !a.out_s || !a.out_i || (a.count > 0 && a.n_sub > 0 && (!a.fi || !a.fk || !a.fs)) ||
        (fusion != kFuseRrf && fusion != kFuseMaxFusion))
        return hipErrorInvalidValue;
    const int L = fuse_call_sort_len(a.n_sub, a.k_fetch);
    const dim3 block(fuse_threads(L));
    const size_t lds = (size_t)fuse_lds_bytes(L);
    // (a large set's dynamic LDS, up to 64 KiB, comes on top of the barrier's few static bytes; set per
    // launch, for the device that is current, and only for the rare large call)
    if (lds > 32768) {
        const void* k = fusion == kFuseRrf ? (const void*)fuse_kernel<kFuseRrf> : (const void*)fuse_kernel<kFuseMaxFusion>;
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fuse_lds_bytes(kFuseMaxSort));
        if (e != hipSuccess) return e;
    }
    if (fusion == kFuseRrf)
        hipLaunchKernelGGL((fuse_kernel<kFuseRrf>), dim3(n_sets), block, lds, st, a);
    else
        hipLaunchKernelGGL((fuse_kernel<kFuseMaxFusion>), dim3(n_sets), block, lds, st, a);
    return hipGetLastError();
}

}  // namespace vdb
