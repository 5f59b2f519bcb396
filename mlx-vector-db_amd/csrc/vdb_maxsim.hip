// vdb_maxsim.hip: MaxSim search (vdb_index_search_maxsim) — groups ranked by the sum, over a set's
// query vectors, of each vector's best canonical fp64 key among the group's rows; part of the gfx950
// kernels of the brute-force path (pipeline overview: vdb_scan.hip).  Built with -ffp-contract=off.
//
// The rows come from the row-major fp32 copy and the keys from the canonical helpers of
// vdb_exact_keys.h, so the candidate copies are never read and the result is the oracle's whatever
// the index's precision.  One call:
//
//   scan    once per block of up to 64 sub-queries (vdb_range_plan.h range_query_block), the shape
//           of the range scan: grid = chunks of 512 rows, 4 waves, a wave owns whole 32-row words in
//           ascending order, holds the pieces of 4 rows in registers and scores them against every
//           sub-query of the block, so the corpus is read once per block.  Lane j serves sub-query j:
//           it keeps the running maximum of the slot (group id) the wave is in, as the
//           order-preserving uint64 of vdb_maxsim_plan.h, and the wave issues one 64-bit atomic
//           maximum into T [sub-query][slot] when the slot changes and after its last row.  The
//           slot is a property of the row, the same in every lane, so the flush is one instruction
//           for the block's lanes.  The maximum of a set of bit patterns does not depend on the
//           order or the grouping of its operands: neither this combining nor the arrival order of
//           the atomics can change a bit of T.
//   rank    grid (segments of slots, sets), 4 waves: lane-consecutive slots, so the reads of
//           T [t][g] coalesce; a slot whose first entry is 0 has no eligible row; the others' entries
//           are decoded and added in sub-query order and (sum, slot) is offered to a per-wave
//           streaming top-k by (sum desc, slot asc).  Wave 0 folds the four; with several segments
//           the workgroup that finishes a set last merges their lists (a per-set counter, release /
//           acquire fences around it, left at zero) and writes the slots.
//
// Device-memory calls are not validated on the host, so the rank kernel takes any offsets: they are
// clamped to [0, n_sub], and a bad set writes "no result" everywhere and is counted in *bad.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_exact_keys.h"
#include "vdb_merge_block.h"
#include "vdb_range_plan.h"
#include "vdb_maxsim_plan.h"

namespace vdb {

namespace {

// MP: 4 / 8 = rows of up to 256 MP dims, the pieces of kRangeNB rows held in registers across the
// block's sub-queries; 0 = any length (as range_scan_kernel).
template <int METRIC, int MP>
__global__ void __launch_bounds__(256) maxsim_scan_kernel(MaxsimScanArgs a, int b0, int qb) {
    constexpr int NB = kRangeNB;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int64_t n_words = range_n_words(a.N);
    const int np = (a.D + 255) / 256;
    const float* Q = a.Q + (int64_t)b0 * a.D;
    const double* qn64 = a.qn64 + b0;
    // lane j: the table row of sub-query j of the block (a lane past the block issues nothing)
    unsigned long long* Tq = a.T + (size_t)(b0 + (lane < qb ? lane : 0)) * (size_t)a.n_slots;
    int32_t cur_slot = -1;       // the slot the wave is in (the same in every lane), -1 = none yet
    unsigned long long cur = 0;  // lane j: the greatest entry of sub-query j in that slot so far
    uint32_t skipped = 0;
    for (int i = 0; i < kRangeWaveWords; ++i) {
        const int64_t w = range_wave_word(chunk, wv, i);
        if (w >= n_words) break;
        // lanes 0 .. 31: the group ids of the word's rows, one load
        const uint32_t valid = range_valid_bits(w, a.N);
        const bool mine = lane < 32 && ((valid >> (lane & 31)) & 1u);
        const int32_t gid = mine ? a.groups[w * 32 + lane] : -1;
        const int32_t sl = maxsim_slot(gid, a.n_slots);
        const uint32_t usable = (uint32_t)__ballot(sl >= 0);
        if (a.skipped) skipped += (uint32_t)__popcll(__ballot(gid >= a.n_slots));
        const uint32_t elig = valid & usable & (a.mask ? a.mask[w] : 0xFFFFFFFFu);
        for (int t = 0; t < 32 / NB; ++t) {
            const uint32_t e = (elig >> (t * NB)) & ((1u << NB) - 1u);
            if (e == 0) continue;  // no eligible row among these: nothing is read
            uint32_t rws[NB];
            double xn[NB];
            bool ok[NB];
            int32_t gs[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                ok[u] = (e >> u) & 1u;
                rws[u] = ok[u] ? (uint32_t)(w * 32 + t * NB + u) : 0u;  // (an ineligible row is not scored)
                xn[u] = (METRIC == 0 && ok[u]) ? a.nrm64[rws[u]] : 1.0;
                gs[u] = __shfl(sl, t * NB + u, 64);
            }
            f32x4 xv[MP > 0 ? MP : 1][NB];
            if constexpr (MP > 0) rows_pieces_load<NB, MP>(a.X, a.G, np, rws, ok, xv);
            double kk[NB];  // lane j: the keys of these rows for sub-query j
#pragma unroll
            for (int u = 0; u < NB; ++u) kk[u] = 0.0;
            for (int j = 0; j < qb; ++j) {
                const float* q = Q + (int64_t)j * a.D;
                const double qn = qn64[j];
                double keys[NB];
                if constexpr (MP > 0)
                    exact_keys_held<METRIC, NB, MP>(q, a.D, qn, np, xv, xn, keys);
                else
                    exact_keys_batch<METRIC, NB>(q, qn, a.X, a.G, a.D, rws, xn, NB, keys);
#pragma unroll
                for (int u = 0; u < NB; ++u)
                    if (lane == j) kk[u] = keys[u];
            }
            // the rows in ascending order; ok and gs are the same in every lane
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                if (!ok[u]) continue;
                if (gs[u] != cur_slot) {
                    if (cur_slot >= 0 && lane < qb) atomicMax(Tq + cur_slot, cur);
                    cur_slot = gs[u];
                    cur = 0;
                }
                const unsigned long long en = maxsim_entry(kk[u]);
                cur = en > cur ? en : cur;
            }
        }
    }
    if (cur_slot >= 0 && lane < qb) atomicMax(Tq + cur_slot, cur);
    if (skipped && lane == 0) atomicAdd(a.skipped, (unsigned long long)skipped);
}

// Grid (n_seg, sets of this launch), 256 threads, maxsim_rank_lds_bytes of dynamic LDS.  Writes
// out_* [set][k].
__global__ void __launch_bounds__(kMaxsimThreads) maxsim_rank_kernel(MaxsimRankArgs a, int set0) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int kWaves = kMaxsimThreads / 64;
    const int KE = a.KE;
    const int cap = WaveTopK<double, uint32_t>::capacity(KE);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int seg = blockIdx.x;
    const int n_seg = (int)gridDim.x;
    const size_t s = (size_t)set0 + blockIdx.y;
    double* kbase = reinterpret_cast<double*>(smem);
    uint32_t* ibase = reinterpret_cast<uint32_t*>(smem + (size_t)kWaves * cap * sizeof(double));
    double* bk = kbase + (size_t)wv * cap;
    uint32_t* bi = ibase + (size_t)wv * cap;

    // the set's sub-queries (every workgroup of the set computes the same range)
    const MaxsimRange rg = maxsim_range(a.offs[s], a.offs[s + 1], a.n_sub);
    if (rg.bad && seg == 0 && threadIdx.x == 0) atomicAdd(a.bad, 1ull);
    const int m = a.scanned ? rg.m : 0;  // (an empty index: no table, no candidate)
    const int64_t n_slots = a.n_slots;

    WaveTopK<double, uint32_t> tk;
    tk.init(bk, bi, KE);
    if (m > 0) {
        const unsigned long long* T0 = a.T + (size_t)rg.o0 * (size_t)n_slots;
        for (int64_t i = 0;; ++i) {
            const int64_t g0 = maxsim_trip_slot(seg, n_seg, wv, i);
            if (g0 >= n_slots) break;
            const int64_t g = g0 + lane;
            // a slot without an eligible row is no candidate (eligibility does not depend on the
            // sub-query: the first entry speaks for all)
            const bool valid = g < n_slots && T0[g] != 0ull;
            double sum = 0.0;
            if (valid) {
                const unsigned long long* col = T0 + g;
                for (int t0 = 0; t0 < m; t0 += 8) {  // eight loads in flight, the adds in order
                    unsigned long long v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = t0 + u < m ? col[(size_t)(t0 + u) * (size_t)n_slots] : 0ull;
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (t0 + u < m) sum = sum + maxsim_decode(v[u]);
                }
            }
            tk.offer(valid, valid ? sum : -INFINITY, valid ? (uint32_t)g : 0xFFFFFFFFu);
        }
    }
    tk.finish();
    __syncthreads();
    float* os = a.out_s + s * a.k;
    int32_t* og = a.out_g + s * a.k;
    double* osum = a.out_sum ? a.out_sum + s * a.k : nullptr;
    if (wv == 0) {
        for (int w = 1; w < kWaves; ++w) {
            const double* ok = kbase + (size_t)w * cap;
            const uint32_t* oi = ibase + (size_t)w * cap;
            for (int e0 = 0; e0 < KE; e0 += 64) {
                const int e = e0 + lane;
                const bool in = e < KE && oi[e] != 0xFFFFFFFFu;
                tk.offer(in, in ? ok[e] : -INFINITY, in ? oi[e] : 0xFFFFFFFFu);
            }
        }
        tk.finish();
        if (n_seg == 1) {  // the only list of this set: straight to the results
            for (int e = lane; e < a.k; e += 64) {
                const uint32_t g = bi[e];
                const bool valid = g != 0xFFFFFFFFu;
                os[e] = valid ? (float)bk[e] : 0.0f;
                og[e] = valid ? (int32_t)g : -1;
                if (osum) osum[e] = valid ? bk[e] : -INFINITY;
            }
        } else {
            const size_t base = (s * n_seg + seg) * KE;
            for (int e = lane; e < KE; e += 64) {
                a.lk[base + e] = bk[e];
                a.li[base + e] = bi[e];
            }
        }
    }
    if (n_seg == 1) return;
    __syncthreads();  // wave 0's list stores are issued; the LDS buffers are free for the merge
    // the last workgroup of this set merges its n_seg lists (release: wave 0's list stores before
    // the count; acquire: the other lists after it)
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = atomicAdd(a.done + s, 1) == n_seg - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    const size_t q0 = s * n_seg * KE;
    merge_block<double, uint32_t>(a.lk + q0, a.li + q0, n_seg, KE, KE, KE, a.mk + s * KE, a.mi + s * KE, smem);
    __syncthreads();
    for (int e = threadIdx.x; e < a.k; e += kMaxsimThreads) {
        const double sum = a.mk[s * KE + e];
        const uint32_t g = a.mi[s * KE + e];
        const bool valid = g != 0xFFFFFFFFu;
        os[e] = valid ? (float)sum : 0.0f;
        og[e] = valid ? (int32_t)g : -1;
        if (osum) osum[e] = valid ? sum : -INFINITY;
    }
    if (threadIdx.x == 0) a.done[s] = 0;  // left zero for the next call on this workspace
}

}  // namespace

hipError_t launch_maxsim_scan(int metric, const MaxsimScanArgs& a, int b0, int qb, hipStream_t st) {
    if (qb <= 0) return hipSuccess;
    if (qb > kRangeMaxBlock || b0 < 0 || a.N <= 0 || a.n_slots < 1 || (metric != 0 && metric != 1) || !a.T || !a.groups ||
        !a.Q || !a.qn64)
        return hipErrorInvalidValue;
    const int64_t n_chunks = range_n_chunks(range_n_words(a.N));
    const int mp = a.D <= 1024 ? 4 : a.D <= 2048 ? 8 : 0;
#define VDB_MAXSIM_SCAN(M, MPV)                                                                                    \
    if (metric == M && mp == MPV) {                                                                                \
        hipLaunchKernelGGL((maxsim_scan_kernel<M, MPV>), dim3((unsigned)n_chunks), dim3(256), 0, st, a, b0, qb);   \
        return hipGetLastError();                                                                                  \
    }
    VDB_MAXSIM_SCAN(0, 4) VDB_MAXSIM_SCAN(0, 8) VDB_MAXSIM_SCAN(0, 0)
    VDB_MAXSIM_SCAN(1, 4) VDB_MAXSIM_SCAN(1, 8) VDB_MAXSIM_SCAN(1, 0)
#undef VDB_MAXSIM_SCAN
    return hipErrorInvalidValue;
}

size_t maxsim_rank_lds_bytes(int KE, int n_seg) {
    size_t lds = (size_t)(kMaxsimThreads / 64) * WaveTopK<double, uint32_t>::capacity(KE) * (sizeof(double) + sizeof(uint32_t));
    if (n_seg > 1) lds = std::max(lds, merge_block_lds<double, uint32_t>(KE));
    return lds;
}

hipError_t launch_maxsim_rank(const MaxsimRankArgs& a, int n_sets, int n_seg, hipStream_t st) {
    if (n_sets <= 0) return hipSuccess;
    if (n_seg < 1 || n_seg > kMaxsimMaxSeg || a.k < 1 || a.k > a.KE || a.KE > kMaxsimMaxK || a.n_slots < 1 || a.n_sub < 0 ||
        !a.offs || !a.bad || !a.out_s || !a.out_g || (a.scanned && !a.T) ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi || !a.done)))
        return hipErrorInvalidValue;
    const size_t lds = maxsim_rank_lds_bytes(a.KE, n_seg);
    for (int s0 = 0; s0 < n_sets; s0 += kMaxsimRankSets) {
        const int ns = n_sets - s0 < kMaxsimRankSets ? n_sets - s0 : kMaxsimRankSets;
        hipLaunchKernelGGL(maxsim_rank_kernel, dim3(n_seg, ns), dim3(kMaxsimThreads), lds, st, a, s0);
    }
    return hipGetLastError();
}

}  // namespace vdb
