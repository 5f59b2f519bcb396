// vdb_hamming_mfma.hip: the integer-MFMA form of the exact Hamming search (vdb_index_search_hamming at
// large batches; the popcount form, the column and its layout: vdb_hamming.hip).
//
// The identity.  A stored bit x becomes the int8 0 / 1, a query bit q the int8 -1 / +1 (2 q - 1).
// Then dot = sum x (2 q - 1) = 2 (q.x) - |x| and the distance |q| + |x| - 2 (q.x) = |q| - dot: the
// only side value is the query's own popcount, the column stays bits in HBM, and zero pad bits and pad
// rows of the column add nothing whatever the query's operand holds there.  |dot| <= 8 192, so the
// i32 accumulators are exact and the distance is the integer the popcount form gives.
//
// hamming_mfma_kernel: grid (n_seg, blocks of 64 queries), 4 waves.  The block's queries lie in LDS as
// bits, word-major.  The workgroup walks chunks s, s + n_seg, ... of 4 tiles; per trip wave w takes
// tile 4 c + w as two 32-row sub-tiles against the two query tiles: four 32 x 32 accumulators.  One
// v_mfma_i32_32x32x32_i8 multiplies 32 bits of the code: lane l supplies 16 bits of row (or query)
// l % 32.  By the mapping of vdb_hamming_plan.h lane l reads word 2 j + l / 32 of its row -- in the
// [tile][W][64] layout two contiguous 256-byte runs per sub-tile -- and that 64-bit word feeds four
// MFMA steps.  Both sides are expanded in registers, four bits to a register: bit field, one 24-bit
// multiply, one AND for a row (0 / 1), and a byte permute on top for a query (-1 / +1).  A row
// expansion is used by both query tiles and a query expansion by both sub-tiles, so a step of four
// MFMAs costs two expansions of each kind.  The next word pair is loaded before the current one is
// expanded.
//
// Top-k.  A key is distance << 32 | row, so "distance ascending, row ascending" is one unsigned compare;
// the per-query candidate buffers in LDS, the threshold test, the compaction and the end of a trip are
// vdb_mfma_topk.h's, shared with the code-dot search, with the distance |q| - dot as the key's upper half.
//
// Segments' lists are written as the popcount form writes them (negated distance as fp32, row) into
// the same scratch and merged by the same merge_block, but in a second launch with one workgroup per
// query (hamming_mfma_merge_kernel): the `done` counters are not used and stay zero.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_hamming_plan.h"
#include "vdb_hamming_tail.h"
#include "vdb_mfma_topk.h"

namespace vdb {

__device__ __forceinline__ ham_i32x4 expand_query16(uint64_t x, int sh) {
    ham_i32x4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d) r[d] = (int)ham_mfma_query4((uint32_t)(x >> (sh + 4 * d)));
    return r;
}

__global__ void __launch_bounds__(256) hamming_mfma_kernel(HammingArgs a) {
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

    const int live = ham_live_segs(a.N, n_seg);
    if (live == 0) {  // no rows: "no result" in every slot
        if (s == 0)
            for (int q = 0; q < nq; ++q)
                for (int e = threadIdx.x; e < k; e += 256) hamming_write(a, b0 + q, e, -INFINITY, 0xFFFFFFFFu);
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do, and not counted below

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
    int qpop[QT];  // |q| of the lane's query in each tile
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        int p = 0;
        for (int w = 0; w < Wp; ++w) p += __popcll(qs[(size_t)w * QB + 32 * qt + col]);
        qpop[qt] = p;
    }
    const auto dist = [&qpop](int qt, int dot) { return (uint32_t)(qpop[qt] - dot); };
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
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) xn[rt] = (vm[rt] != 0u && half < W) ? xt[(size_t)half * kHamTileRows + 32 * rt] : 0ull;
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
                for (int m = 0; m < 4; ++m) {
                    const int sh = ham_mfma_shift(m);
                    ham_i32x4 xa[RT], qa[QT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) xa[rt] = expand_row16(x[rt], sh);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) qa[qt] = expand_query16(qw[qt], sh);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int qt = 0; qt < QT; ++qt)
                            acc[rt][qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa[rt], qa[qt], acc[rt][qt], 0, 0, 0);
                }
            }
        }
        mfma_rank_trip(acc, vm, t, mfma_value_key(dist), nq, k, trip, s_flag, cnt0, cand, thr, cnt);
    }
    // what is kept, sorted
    mfma_compact_all(0, nq, k, cand, thr, cnt);
    __syncthreads();
    for (int q = wv; q < nq; q += kHamWaves) {
        const int c = cnt[q];
        const uint64_t* b = cand + (size_t)q * CAP;
        if (live == 1) {  // the only list of this query: straight to the results
            for (int e = lane; e < k; e += 64) {
                const uint64_t key = e < c ? b[e] : kNoKey;
                hamming_write(a, b0 + q, e, -(float)(uint32_t)(key >> 32), e < c ? (uint32_t)key : 0xFFFFFFFFu);
            }
        } else {
            const size_t base = ((size_t)(b0 + q) * n_seg + s) * KE;
            for (int e = lane; e < KE; e += 64) {
                const uint64_t key = e < c ? b[e] : kNoKey;
                a.lk[base + e] = e < c ? -(float)(uint32_t)(key >> 32) : -INFINITY;
                a.li[base + e] = e < c ? (uint32_t)key : 0xFFFFFFFFu;
            }
        }
    }
}

// The segments' lists of query b, merged: one workgroup per query.  (The popcount form merges in the
// workgroup that finishes a block last; with 64 queries a block and up to 512 lists a query that one
// workgroup's 64 merges in a row took longer than the whole scan: DESIGN.md §24.)
__global__ void __launch_bounds__(256) hamming_mfma_merge_kernel(HammingArgs a, int n_seg, int live) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x;
    const int KE = a.KE;
    const size_t l0 = (size_t)b * n_seg * KE;
    merge_block<float, uint32_t>(a.lk + l0, a.li + l0, live, KE, KE, KE, a.mk + (size_t)b * KE, a.mi + (size_t)b * KE, smem);
    __syncthreads();
    for (int e = threadIdx.x; e < a.k; e += 256) hamming_write(a, b, e, a.mk[(size_t)b * KE + e], a.mi[(size_t)b * KE + e]);
}

size_t hamming_mfma_lds_bytes(int W) { return (size_t)ham_mfma_lds_bytes(W); }

hipError_t launch_hamming_mfma(const HammingArgs& a, int n_seg, hipStream_t st) {
    if (a.n_queries <= 0) return hipSuccess;
    const int W = ham_words(a.n_bytes);
    if (a.n_queries > kHamMaxQueries || n_seg < 1 || n_seg > kHamMaxSeg || a.k < 1 || ham_mfma_qb(a.k) != QB ||
        a.KE != ham_ke(a.k) || a.N < 0 || a.N > 0xFFFFFFFEll || a.n_bytes < 1 || a.n_bytes > kHamMaxBytes || a.W != W ||
        !a.queries || (a.N > 0 && !a.codes) || !a.out_d || !a.out_i ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi)))
        return hipErrorInvalidValue;
    // the plan header restates the merge buffer without HIP
    if ((size_t)ham_merge_lds(a.KE) != merge_block_lds<float, uint32_t>(a.KE)) return hipErrorInvalidValue;
    const size_t lds = hamming_mfma_lds_bytes(W);
    if (lds + (size_t)kHamMfmaStaticLds > (size_t)kHamLdsLimit) return hipErrorInvalidValue;
    if (lds > 65536) {  // (set per launch, for the device that is current)
        const hipError_t e =
            hipFuncSetAttribute((const void*)hamming_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(hamming_mfma_kernel, dim3(n_seg, ham_n_blocks(a.n_queries, QB)), dim3(256), lds, st, a);
    hipError_t e = hipGetLastError();
    const int live = ham_live_segs(a.N, n_seg);
    if (e != hipSuccess || live <= 1) return e;  // (one list: the scan wrote the results itself)
    hipLaunchKernelGGL(hamming_mfma_merge_kernel, dim3(a.n_queries), dim3(256), (size_t)ham_merge_lds(a.KE), st, a, n_seg, live);
    return hipGetLastError();
}

}  // namespace vdb
