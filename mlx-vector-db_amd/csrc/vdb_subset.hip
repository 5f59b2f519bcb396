// vdb_subset.hip: exact search over explicit row-id lists (vdb_index_search_rows), part of the
// gfx950 kernels of the brute-force distance + top-k path (pipeline overview: vdb_scan.hip).
// Built with -ffp-contract=off.
//
// The shape of the exact scan (vdb_exact.hip exact_scan_kernel) driven by a list instead of a row
// range: grid (n_seg, n_queries), 4 waves; one wave per row, the row-major fp32 copy and the
// canonical fp64 key (vdb_exact_keys.h), so the candidate copies are never read and the result is
// that of a masked search whatever the index's precision.  Segment s of query b walks chunks
// s, s + n_seg, ... of b's list (vdb_subset_plan.h); each wave reads the ids of its 16 positions
// of a chunk with one load and scores them 4 rows at a time, all of their pieces in flight
// together; keys stream through a per-wave WaveTopK, wave 0 folds the four, and the workgroup that
// finishes a query last merges the segments' lists and writes the results (the fused tail of the
// exact scan: a per-query counter, release / acquire fences around it).
//
// Device-memory calls are not validated on the host, so the kernel takes any input: offsets are
// clamped to [0, n_ids], a query_list entry outside [0, n_lists) gives an empty result, and an id
// outside [0, count) or not above its predecessor is skipped and counted in *bad.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_exact_keys.h"
#include "vdb_merge_block.h"
#include "vdb_subset_plan.h"

namespace vdb {

// MP: 4 / 8 = rows of up to 256 MP dims with every piece of a batch in flight; 0 = any length, one
// piece per row in flight per trip.
template <int METRIC, int MP>
__global__ void __launch_bounds__(256) subset_kernel(SubsetArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NB = kSubsetNB;
    const int KE = a.KE;
    const int cap = WaveTopK<double, uint32_t>::capacity(KE);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int s = blockIdx.x;
    const int n_seg = (int)gridDim.x;
    double* kbase = reinterpret_cast<double*>(smem);
    uint32_t* ibase = reinterpret_cast<uint32_t*>(smem + (size_t)kSubsetWaves * cap * sizeof(double));
    double* bk = kbase + (size_t)wv * cap;
    uint32_t* bi = ibase + (size_t)wv * cap;

    // this query's list (every workgroup of the query computes the same range)
    const int64_t l = a.qlist ? (int64_t)a.qlist[b] : (int64_t)b;
    SubsetRange rg{0, 0};
    if (l >= 0 && l < a.n_lists) rg = subset_range(a.offs[l], a.offs[l + 1], a.n_ids);
    const int64_t len = rg.o1 - rg.o0;
    const int live = subset_live_segs(len, n_seg);
    if (live == 0) {  // an empty list (or no list): "no result" in every slot
        if (s == 0)
            for (int e = threadIdx.x; e < a.k; e += 256) {
                const size_t o = (size_t)b * a.k + e;
                write_result(METRIC, -INFINITY, 0, false, a.out_s + o, a.out_i + o, a.out_k ? a.out_k + o : nullptr);
            }
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do, and not counted below

    const float* q = a.Q + (int64_t)b * a.D;
    const double qn = a.qn64[b];
    const int np = (a.D + 255) / 256;
    const int64_t* ids = a.rows + rg.o0;
    WaveTopK<double, uint32_t> tk;
    tk.init(bk, bi, KE);
    unsigned n_bad = 0;
    const int64_t n_chunks = subset_n_chunks(len);
    for (int64_t c = s; c < n_chunks; c += n_seg) {
        // wave wv: positions [w0, w1) of the list; lane i holds the id at w0 - 1 + i (i <= 16):
        // the ids and each one's predecessor in one load
        const int64_t w0 = c * kSubsetChunk + (int64_t)wv * kSubsetWaveRows;
        const int64_t w1 = w0 + kSubsetWaveRows < len ? w0 + kSubsetWaveRows : len;
        if (w0 >= w1) continue;
        const int64_t pp = w0 - 1 + lane;
        const int64_t idv = (lane <= kSubsetWaveRows && pp >= 0 && pp < w1) ? ids[pp] : (int64_t)-1;
#pragma unroll
        for (int t = 0; t < kSubsetWaveRows / NB; ++t) {
            const int64_t j0 = w0 + t * NB;
            if (j0 >= w1) break;
            const int nb = (int)(w1 - j0 < NB ? w1 - j0 : NB);
            uint32_t rws[NB];
            double xn[NB];
            bool ok[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int64_t id = __shfl(idv, 1 + t * NB + u, 64);
                const int64_t prev = __shfl(idv, t * NB + u, 64);
                ok[u] = u < nb && subset_id_ok(id, prev, a.count);
                if (u < nb && !ok[u]) ++n_bad;
                rws[u] = ok[u] ? (uint32_t)id : 0u;  // (an ineligible id: row 0 is read, its key dropped)
                xn[u] = METRIC == 0 ? a.nrm64[rws[u]] : 1.0;
            }
            double keys[NB];
            if constexpr (MP > 0)
                exact_keys_rows<METRIC, NB, MP>(q, a.D, qn, a.X, a.G, np, rws, xn, nb, keys);
            else
                exact_keys_batch<METRIC, NB>(q, qn, a.X, a.G, a.D, rws, xn, nb, keys);
            // lane u < NB offers row u of the batch
            double key = -INFINITY;
            uint32_t row = 0xFFFFFFFFu;
            bool valid = false;
#pragma unroll
            for (int u = 0; u < NB; ++u)
                if (lane == u) {
                    valid = ok[u];
                    key = ok[u] ? keys[u] : -INFINITY;
                    row = rws[u];
                }
            tk.offer(valid, key, row);
        }
    }
    if (n_bad && lane == 0 && a.bad) atomicAdd(a.bad, (unsigned long long)n_bad);
    tk.finish();
    __syncthreads();
    if (wv == 0) {
        for (int w = 1; w < kSubsetWaves; ++w) {
            const double* ok = kbase + (size_t)w * cap;
            const uint32_t* oi = ibase + (size_t)w * cap;
            for (int e0 = 0; e0 < KE; e0 += 64) {
                const int e = e0 + lane;
                const bool in = e < KE && oi[e] != 0xFFFFFFFFu;
                tk.offer(in, in ? ok[e] : -INFINITY, in ? oi[e] : 0xFFFFFFFFu);
            }
        }
        tk.finish();
        if (live == 1) {  // the only list of this query: straight to the results
            for (int e = lane; e < a.k; e += 64) {
                const double key = e < KE ? bk[e] : -INFINITY;
                const uint32_t r = e < KE ? bi[e] : 0xFFFFFFFFu;
                const bool valid = r != 0xFFFFFFFFu;
                const size_t o = (size_t)b * a.k + e;
                write_result(METRIC, key, valid ? (uint64_t)r + (uint64_t)a.index_offset : 0, valid && key != -INFINITY,
                             a.out_s + o, a.out_i + o, a.out_k ? a.out_k + o : nullptr);
            }
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
                                  smem);
    __syncthreads();
    for (int e = threadIdx.x; e < a.k; e += 256) {
        const double key = a.mk[(size_t)b * KE + e];
        const uint32_t r = a.mi[(size_t)b * KE + e];
        const bool valid = r != 0xFFFFFFFFu;
        const size_t o = (size_t)b * a.k + e;
        write_result(METRIC, key, valid ? (uint64_t)r + (uint64_t)a.index_offset : 0, valid && key != -INFINITY,
                     a.out_s + o, a.out_i + o, a.out_k ? a.out_k + o : nullptr);
    }
    if (threadIdx.x == 0) a.done[b] = 0;  // left zero for the next call on this workspace
}

size_t subset_lds_bytes(int KE, int n_seg) {
    size_t lds = (size_t)kSubsetWaves * WaveTopK<double, uint32_t>::capacity(KE) * (sizeof(double) + sizeof(uint32_t));
    if (n_seg > 1) lds = std::max(lds, merge_block_lds<double, uint32_t>(KE));
    return lds;
}

hipError_t launch_subset_search(int metric, const SubsetArgs& a, int n_queries, int n_seg, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (n_seg < 1 || n_seg > kSubsetMaxSeg || a.k < 1 || a.k > a.KE || a.KE > 1024 || a.count <= 0 ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi || !a.done)))
        return hipErrorInvalidValue;
    const size_t lds = subset_lds_bytes(a.KE, n_seg);
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    const dim3 grid(n_seg, n_queries);
    const int mp = a.D <= 1024 ? 4 : a.D <= 2048 ? 8 : 0;
#define VDB_SUB(M, MPV)                                                                        \
    if (metric == M && mp == MPV) {                                                            \
        hipLaunchKernelGGL((subset_kernel<M, MPV>), grid, dim3(256), lds, st, a);              \
        return hipGetLastError();                                                              \
    }
    VDB_SUB(0, 4) VDB_SUB(0, 8) VDB_SUB(0, 0)
    VDB_SUB(1, 4) VDB_SUB(1, 8) VDB_SUB(1, 0)
#undef VDB_SUB
    return hipErrorInvalidValue;
}

}  // namespace vdb
