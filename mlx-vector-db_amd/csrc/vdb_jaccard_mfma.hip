// vdb_jaccard_mfma.hip: the int8-MFMA form of the exact Jaccard / Tanimoto search (vdb_index_search_jaccard
// at k <= 64; the popcount form and the contract: vdb_jaccard.hip; the column: vdb_hamming.hip).
//
// Scoring.  Stored bits and query bits both become the int8 0 / 1, so v_mfma_i32_32x32x32_i8 leaves i =
// |q AND x| in the accumulators as it stands (i <= 8 192: exact), and u = |q| + |x| - i.  Zero pad bits,
// pad rows and absent queries add nothing to either.
//
// jaccard_mfma_kernel: grid (n_seg, blocks of 64 queries), 4 waves; the walk of chunks and tiles, the bit
// mapping, the row loads with the next word pair in flight and the four 32 x 32 accumulators per wave
// are hamming_mfma_kernel's.  Both operands are expanded the same way (bit field, one 24-bit multiply,
// one AND): a row expansion serves both query tiles, a query expansion both sub-tiles.
//
// Row popcounts.  Lane l holds the words of parity l / 32 of row l % 32 of each sub-tile and counts
// their bits as they pass, before the expansion.  The two sub-tiles' counts (each at most 8 192) share
// one register, 16 bits each, so one exchange with lane l ^ 32 completes both; lane l then parks |x| of
// the tile's row l in the wave's 64 words of LDS.  An accumulator register holds another row than the
// lane loaded, so the lane reads |x| of its 16 rows per sub-tile back by accumulator row (two
// addresses per wave and register: broadcasts) and keeps them in registers for the offer and for the
// repeated offers of a refill round.  |q| of every query lies beside the thresholds in LDS.
//
// Order.  A key is jac_key_hi << 32 | row, jac_key_hi = floor((u - i) 2^27 / u): a function of the ratio,
// distinct and ordered for distinct ratios (vdb_jaccard_plan.h), so one unsigned compare ranks (s
// descending, row ascending).  The offer does not form it: jac_pass tests (i, u, row) against the
// threshold key by one 64-bit multiply, and only an entry that passes pays the fp64 division.  The
// candidate buffers, the compaction and the end of a trip are vdb_mfma_topk.h's, which hands the rank
// object the sub-tile and the accumulator register besides the value.
//
// Segments' lists go out as (-(double)jac_key_hi, row) -- fp64 holds every 28-bit integer -- and a second
// launch merges them with merge_block<double, uint32_t>, one workgroup per query.  i and u of the
// winners are counted again at the write (vdb_jaccard_tail.h).
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_jaccard_plan.h"
#include "vdb_jaccard_tail.h"
#include "vdb_mfma_topk.h"

namespace vdb {

// The rank object of vdb_mfma_topk.h: |q| of the lane's query per query tile, |x| of the lane's
// accumulator rows per sub-tile.
struct JaccardRank {
    int qpop[QT];
    int xpop[RT][16];
    __device__ __forceinline__ bool pass(int qt, int rt, int v, int i, uint32_t row, uint64_t th) const {
        return jac_pass(i, qpop[qt] + xpop[rt][v] - i, row, th);
    }
    __device__ __forceinline__ uint32_t hi(int qt, int rt, int v, int i) const {
        return jac_key_hi(i, qpop[qt] + xpop[rt][v] - i);
    }
};

__global__ void __launch_bounds__(256) jaccard_mfma_kernel(JaccardArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_flag[2];
    const int KE = a.KE, k = a.k;
    const int W = a.W, Wp = ham_mfma_words(W);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int s = blockIdx.x;
    const int n_seg = (int)gridDim.x;
    const int b0 = blockIdx.y * QB;
    const int nq = a.n_queries - b0 < QB ? a.n_queries - b0 : QB;
    uint64_t* qs = reinterpret_cast<uint64_t*>(smem);
    uint64_t* cand = reinterpret_cast<uint64_t*>(smem + ham_mfma_cand_off(W));
    uint64_t* thr = reinterpret_cast<uint64_t*>(smem + ham_mfma_thr_off(W));
    int* cnt = reinterpret_cast<int*>(smem + ham_mfma_cnt_off(W));
    int* s_qpop = reinterpret_cast<int*>(smem + jac_mfma_qpop_off(W));
    int* s_xpop = reinterpret_cast<int*>(smem + jac_mfma_xpop_off(W)) + wv * kHamTileRows;  // this wave's

    const int live = ham_live_segs(a.N, n_seg);
    if (live == 0) {  // no rows: "no result" in every slot
        if (s == 0)
            for (int q = 0; q < nq; ++q)
                for (int e = threadIdx.x; e < k; e += 256) jaccard_write(a, b0 + q, e, 0xFFFFFFFFu);
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do

    // the block's queries as words [Wp][QB], zero where there is no query or no byte
    for (int i = threadIdx.x; i < QB * Wp; i += 256) {
        const int q = i / Wp, w = i - q * Wp;
        qs[(size_t)w * QB + q] = (q < nq && w < W) ? ham_word_of(a.queries + (size_t)(b0 + q) * a.n_bytes, a.n_bytes, w) : 0ull;
    }
    if (threadIdx.x < QB) {
        thr[threadIdx.x] = kNoKey;
        cnt[threadIdx.x] = 0;
    }
    if (threadIdx.x < 2) s_flag[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x < QB) {  // |q|, once per query
        int p = 0;
        for (int w = 0; w < Wp; ++w) p += __popcll(qs[(size_t)w * QB + threadIdx.x]);
        s_qpop[threadIdx.x] = p;
    }
    __syncthreads();
    JaccardRank rank{};
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) rank.qpop[qt] = s_qpop[32 * qt + col];
    int cnt0 = 0;  // thread q < QB: query q's count at the trip's start

    const int64_t n_tiles = ham_n_tiles(a.N);
    const int64_t n_chunks = ham_n_chunks(a.N);
    const int n_pairs = Wp / 2;
    int trip = 0;
    for (int64_t c = s; c < n_chunks; c += n_seg, ++trip) {
        const int64_t t = ham_tile_of(c, wv);
        // the candidate rows of the two sub-tiles: below N, and the mask's word if there is one (the
        // word of a sub-tile with a row below N lies inside the mask's ceil(N / 32) words)
        uint32_t vm[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int64_t base = t * kHamTileRows + 32 * rt;
            uint32_t m = 0;
            if (t < n_tiles && base < a.N) {
                m = a.N - base < 32 ? (1u << (int)(a.N - base)) - 1u : 0xFFFFFFFFu;
                if (a.mask) m &= a.mask[2 * t + rt];
            }
            vm[rt] = __builtin_amdgcn_readfirstlane(m);
        }
        ham_i32x16 acc[RT][QT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[rt][qt][v] = 0;
        if ((vm[0] | vm[1]) != 0u) {  // (a tile the mask rules out whole is not read)
            const uint64_t* xt = a.codes + (size_t)t * W * kHamTileRows + col;
            uint64_t xn[RT];
            int xp[RT];  // bits of the lane's words of row col of each sub-tile
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                xn[rt] = (vm[rt] != 0u && half < W) ? xt[(size_t)half * kHamTileRows + 32 * rt] : 0ull;
                xp[rt] = 0;
            }
            for (int j = 0; j < n_pairs; ++j) {
                uint64_t x[RT], qw[QT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) x[rt] = xn[rt];
                const int wn = ham_mfma_word(4 * (j + 1), half);  // the next pair's word of this lane half
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    xn[rt] = (j + 1 < n_pairs && vm[rt] != 0u && wn < W) ? xt[(size_t)wn * kHamTileRows + 32 * rt] : 0ull;
                const int w = ham_mfma_word(4 * j, half);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) qw[qt] = qs[(size_t)w * QB + 32 * qt + col];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) xp[rt] += __popcll(x[rt]);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int sh = ham_mfma_shift(m);
                    ham_i32x4 xa[RT], qa[QT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) xa[rt] = expand_row16(x[rt], sh);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) qa[qt] = expand_row16(qw[qt], sh);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int qt = 0; qt < QT; ++qt)
                            acc[rt][qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa[rt], qa[qt], acc[rt][qt], 0, 0, 0);
                }
            }
            // |x| of the tile's 64 rows: the two halves of a row joined by one exchange, both
            // sub-tiles in one register; lane l parks row l's (sub-tile l / 32, row l % 32)
            static_assert(RT == 2 && kHamMaxBytes * 8 < (1 << 16), "two counts of 16 bits share the exchange");
            int p = xp[0] | (xp[1] << 16);
            p += __shfl_xor(p, 32, 64);
            s_xpop[lane] = half ? (p >> 16) : (p & 0xFFFF);
            // the stores are complete before the reads below (LDS accesses of a wave complete in order)
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int v = 0; v < 16; ++v) rank.xpop[rt][v] = s_xpop[32 * rt + mfma_acc_row(v)];
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
        mfma_rank_trip(acc, vm, t, rank, nq, k, trip, s_flag, cnt0, cand, thr, cnt);
    }
    // what is kept, sorted
    mfma_compact_all(0, nq, k, cand, thr, cnt);
    __syncthreads();
    for (int q = wv; q < nq; q += kHamWaves) {
        const int c = cnt[q];
        const uint64_t* b = cand + (size_t)q * CAP;
        if (live == 1) {  // the only list of this query: straight to the results
            for (int e = lane; e < k; e += 64) jaccard_write(a, b0 + q, e, e < c ? (uint32_t)b[e] : 0xFFFFFFFFu);
        } else {
            const size_t base = ((size_t)(b0 + q) * n_seg + s) * KE;
            for (int e = lane; e < KE; e += 64) {
                const uint64_t key = e < c ? b[e] : kNoKey;
                a.lk[base + e] = e < c ? -(double)(uint32_t)(key >> 32) : (double)-INFINITY;
                a.li[base + e] = e < c ? (uint32_t)key : 0xFFFFFFFFu;
            }
        }
    }
}

// The segments' lists of query b, merged: one workgroup per query (as hamming_mfma_merge_kernel).
__global__ void __launch_bounds__(256) jaccard_mfma_merge_kernel(JaccardArgs a, int n_seg, int live) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x;
    const int KE = a.KE;
    const size_t l0 = (size_t)b * n_seg * KE;
    merge_block<double, uint32_t>(a.lk + l0, a.li + l0, live, KE, KE, KE, a.mk + (size_t)b * KE, a.mi + (size_t)b * KE, smem);
    __syncthreads();
    for (int e = threadIdx.x; e < a.k; e += 256) jaccard_write(a, b, e, a.mi[(size_t)b * KE + e]);
}

size_t jaccard_mfma_lds_bytes(int W) { return (size_t)jac_mfma_lds_bytes(W); }

hipError_t launch_jaccard_mfma(const JaccardArgs& a, int n_seg, hipStream_t st) {
    if (a.n_queries <= 0) return hipSuccess;
    const int W = ham_words(a.n_bytes);
    if (a.n_queries > kHamMaxQueries || n_seg < 1 || n_seg > kHamMaxSeg || a.k < 1 || jac_mfma_qb(a.k) != QB ||
        a.KE != ham_ke(a.k) || a.N < 0 || a.N > 0xFFFFFFFEll || a.n_bytes < 1 || a.n_bytes > kHamMaxBytes || a.W != W ||
        !a.queries || (a.N > 0 && !a.codes) || !a.out_n || !a.out_u || !a.out_i ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi)))
        return hipErrorInvalidValue;
    // the plan header restates the merge buffer without HIP
    if ((size_t)jac_merge_lds(a.KE) != merge_block_lds<double, uint32_t>(a.KE)) return hipErrorInvalidValue;
    const size_t lds = jaccard_mfma_lds_bytes(W);
    if (lds + (size_t)kHamMfmaStaticLds > (size_t)kHamLdsLimit) return hipErrorInvalidValue;
    if (lds > 65536) {  // (set per launch, for the device that is current)
        const hipError_t e =
            hipFuncSetAttribute((const void*)jaccard_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(jaccard_mfma_kernel, dim3(n_seg, ham_n_blocks(a.n_queries, QB)), dim3(256), lds, st, a);
    hipError_t e = hipGetLastError();
    const int live = ham_live_segs(a.N, n_seg);
    if (e != hipSuccess || live <= 1) return e;  // (one list: the scan wrote the results itself)
    hipLaunchKernelGGL(jaccard_mfma_merge_kernel, dim3(a.n_queries), dim3(256), (size_t)jac_merge_lds(a.KE), st, a, n_seg, live);
    return hipGetLastError();
}

}  // namespace vdb
