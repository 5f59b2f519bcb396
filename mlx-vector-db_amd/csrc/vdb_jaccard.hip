// vdb_jaccard.hip: the popcount form of the exact Jaccard / Tanimoto search over the binary code column
// (vdb_index_search_jaccard; the column, its tiles and the pack kernel: vdb_hamming.hip; the int8-MFMA
// form of this search: vdb_jaccard_mfma.hip).
//
// s(b, r) = |q_b AND x_r| / |q_b OR x_r|, 1 when both are empty; rows rank by (s descending as an exact
// rational, row ascending).  With i = popcount(q AND x) the union is |q| + |x| - i, so a pair costs one
// AND and one popcount per word, as a Hamming pair costs one XOR and one popcount: |x| is counted once
// per row word, not once per pair, and |q| once per query when the block is staged.
//
// jaccard_kernel<QB>: grid (n_seg, query blocks), 4 waves; the layout, the deal of tiles to segments and
// waves and the mask are hamming_kernel's.  A workgroup puts its block's queries into LDS as 64-bit
// words with their popcounts behind them and walks chunks s, s + n_seg, ... of 4 tiles; wave w takes
// tile 4 c + w, a lane one row.  A lane holds up to 16 words of its row in registers per pass and for
// each query of the block adds popcount(x_w & q_w) into one of QB integer accumulators (the query words
// are wave-uniform LDS broadcasts).
//
// Top-k.  Per (wave, query of the block) one WaveTopK<double, uint32_t> keyed by the fp64 quotient i / u
// (vdb_jaccard_plan.h: exact as an order on the ratios; fp32 is not).  An entry is 12 bytes, not the
// Hamming search's 8, so the query block per k is this search's own (jac_qb).  Wave 0 folds the four
// waves' lists per query; the workgroup that finishes a block last merges the segments' lists with
// merge_block<double, uint32_t> and writes the outputs, recounting i and u of the winners
// (vdb_jaccard_tail.h).
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_jaccard_plan.h"
#include "vdb_jaccard_tail.h"

namespace vdb {

static_assert(kHamMergeBuf == MERGE_BUF, "jac_merge_lds restates merge_block_lds");
static_assert(kHamMaxSeg <= MERGE_HEADS, "the tail merge's select path takes at most MERGE_HEADS lists");

template <int QB>
__global__ void __launch_bounds__(256) jaccard_kernel(JaccardArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef WaveTopK<double, uint32_t> TopK;
    const int KE = a.KE;
    const int W = a.W;
    const int WS = ham_query_stride(W);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int s = blockIdx.x;
    const int n_seg = (int)gridDim.x;
    const int b0 = blockIdx.y * QB;                                   // the block's first query
    const int nq = a.n_queries - b0 < QB ? a.n_queries - b0 : QB;     // and how many it has
    const uint64_t* qs = reinterpret_cast<const uint64_t*>(smem);
    int* qpop = reinterpret_cast<int*>(smem + jac_qpop_off(QB, W));
    char* tkmem = smem + jac_query_lds(QB, W);

    const int live = ham_live_segs(a.N, n_seg);
    if (live == 0) {  // no rows: "no result" in every slot
        if (s == 0)
            for (int q = 0; q < nq; ++q)
                for (int e = threadIdx.x; e < a.k; e += 256) jaccard_write(a, b0 + q, e, 0xFFFFFFFFu);
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do, and not counted below

    // the block's queries as words, zero where there is no query or no byte
    {
        uint64_t* qw = reinterpret_cast<uint64_t*>(smem);
        for (int i = threadIdx.x; i < QB * WS; i += 256) {
            const int q = i / WS, w = i - q * WS;
            qw[i] = (q < nq && w < W) ? ham_word_of(a.queries + (size_t)(b0 + q) * a.n_bytes, a.n_bytes, w) : 0ull;
        }
    }
    TopK tk[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q)
        tk[q].init(reinterpret_cast<double*>(smem + jac_lds_key_off(wv, q, QB, W, KE)),
                   reinterpret_cast<uint32_t*>(smem + jac_lds_row_off(wv, q, QB, W, KE)), KE);
    __syncthreads();
    // |q|, once per query: wave w counts queries w, w + 4, ...
    for (int q = wv; q < QB; q += kHamWaves) {
        int p = 0;
        for (int w = lane; w < WS; w += 64) p += __popcll(qs[q * WS + w]);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) p += __shfl_xor(p, m, 64);
        if (lane == 0) qpop[q] = p;
    }
    __syncthreads();

    const int64_t n_tiles = ham_n_tiles(a.N);
    const int64_t n_chunks = ham_n_chunks(a.N);
    const int64_t mask_words = ham_mask_words(a.N);
    for (int64_t c = s; c < n_chunks; c += n_seg) {
        const int64_t t = ham_tile_of(c, wv);
        if (t >= n_tiles) continue;  // (wave-uniform: the last chunk's missing tiles)
        const int64_t row = t * kHamTileRows + lane;
        // the tile's two mask words, read once each
        bool in = row < a.N;
        if (a.mask) {
            uint32_t mw = 0;
            if (lane < 2 && 2 * t + lane < mask_words) mw = a.mask[2 * t + lane];
            mw = __shfl(mw, lane >> 5, 64);
            in = in && ((mw >> (lane & 31)) & 1u);
        }
        if (__ballot(in) == 0ull) continue;  // a tile the mask rules out whole
        int acc[QB];
#pragma unroll
        for (int q = 0; q < QB; ++q) acc[q] = 0;
        int xp = 0;  // |x| of the lane's row
        const uint64_t* xt = a.codes + (size_t)t * W * kHamTileRows + lane;
        for (int w0 = 0; w0 < W; w0 += kHamPassWords) {
            uint64_t x[kHamPassWords];
#pragma unroll
            for (int j = 0; j < kHamPassWords; ++j) x[j] = w0 + j < W ? xt[(size_t)(w0 + j) * kHamTileRows] : 0ull;
#pragma unroll
            for (int j = 0; j < kHamPassWords; ++j) xp += __popcll(x[j]);
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                const uint64_t* qq = qs + q * WS + w0;  // wave-uniform: an LDS broadcast
                int d = acc[q];
#pragma unroll
                for (int j = 0; j < kHamPassWords; ++j) d += __popcll(x[j] & qq[j]);
                acc[q] = d;
            }
        }
#pragma unroll
        for (int q = 0; q < QB; ++q)
            if (q < nq) tk[q].offer(in, jac_key(acc[q], qpop[q] + xp - acc[q]), in ? (uint32_t)row : 0xFFFFFFFFu);
    }
#pragma unroll
    for (int q = 0; q < QB; ++q)
        if (q < nq) tk[q].finish();
    __syncthreads();
    if (wv == 0) {
#pragma unroll
        for (int q = 0; q < QB; ++q) {
            if (q >= nq) continue;
            for (int w = 1; w < kHamWaves; ++w) {
                const double* ok = reinterpret_cast<const double*>(smem + jac_lds_key_off(w, q, QB, W, KE));
                const uint32_t* oi = reinterpret_cast<const uint32_t*>(smem + jac_lds_row_off(w, q, QB, W, KE));
                for (int e0 = 0; e0 < KE; e0 += 64) {
                    const int e = e0 + lane;
                    const bool inb = e < KE && oi[e] != 0xFFFFFFFFu;
                    tk[q].offer(inb, inb ? ok[e] : (double)-INFINITY, inb ? oi[e] : 0xFFFFFFFFu);
                }
            }
            tk[q].finish();
            const double* bk = tk[q].bk;
            const uint32_t* bi = tk[q].bi;
            if (live == 1) {  // the only list of this query: straight to the results
                for (int e = lane; e < a.k; e += 64) jaccard_write(a, b0 + q, e, e < KE ? bi[e] : 0xFFFFFFFFu);
            } else {
                const size_t base = ((size_t)(b0 + q) * n_seg + s) * KE;
                for (int e = lane; e < KE; e += 64) {
                    a.lk[base + e] = bk[e];
                    a.li[base + e] = bi[e];
                }
            }
        }
    }
    if (live == 1) return;
    __syncthreads();  // wave 0's list stores are issued; the LDS buffers are free for the merge
    // the last workgroup of this block merges the `live` lists of each of its queries (release: wave
    // 0's list stores before the count; acquire: the other lists after it)
    __shared__ int s_last;
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = atomicAdd(a.done + blockIdx.y, 1) == live - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    for (int q = 0; q < nq; ++q) {
        const int b = b0 + q;
        const size_t l0 = (size_t)b * n_seg * KE;
        merge_block<double, uint32_t>(a.lk + l0, a.li + l0, live, KE, KE, KE, a.mk + (size_t)b * KE, a.mi + (size_t)b * KE,
                                      tkmem);
        __syncthreads();
        for (int e = threadIdx.x; e < a.k; e += 256) jaccard_write(a, b, e, a.mi[(size_t)b * KE + e]);
    }
    if (threadIdx.x == 0) a.done[blockIdx.y] = 0;  // left zero for the next call on this workspace
}

size_t jaccard_search_lds_bytes(int qb, int W, int KE, int n_seg) { return (size_t)jac_lds_bytes(qb, W, KE, n_seg > 1); }

template <int QB>
static hipError_t launch_jaccard_qb(const JaccardArgs& a, int n_seg, size_t lds, hipStream_t st) {
    if (lds > 65536) {  // (set per launch, for the device that is current)
        const hipError_t e =
            hipFuncSetAttribute((const void*)jaccard_kernel<QB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(jaccard_kernel<QB>, dim3(n_seg, ham_n_blocks(a.n_queries, QB)), dim3(256), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_jaccard_search(const JaccardArgs& a, int qb, int n_seg, hipStream_t st) {
    if (a.n_queries <= 0) return hipSuccess;
    const int W = ham_words(a.n_bytes);
    if (a.n_queries > kHamMaxQueries || n_seg < 1 || n_seg > kHamMaxSeg || a.k < 1 || a.k > a.KE || a.KE != ham_ke(a.k) ||
        a.KE > kHamMaxK || a.N < 0 || a.N > 0xFFFFFFFEll || a.n_bytes < 1 || a.n_bytes > kHamMaxBytes || a.W != W ||
        qb != jac_block(a.k, a.n_queries) || !a.queries || (a.N > 0 && !a.codes) || !a.out_n || !a.out_u || !a.out_i ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi || !a.done)))
        return hipErrorInvalidValue;
    // the plan header restates these two without HIP
    if (ham_cap(a.KE) != WaveTopK<double, uint32_t>::capacity(a.KE) ||
        (size_t)jac_merge_lds(a.KE) != merge_block_lds<double, uint32_t>(a.KE))
        return hipErrorInvalidValue;
    const size_t lds = jaccard_search_lds_bytes(qb, W, a.KE, n_seg);
    if (lds > (size_t)kHamLdsLimit) return hipErrorInvalidValue;
    switch (qb) {
        case 1: return launch_jaccard_qb<1>(a, n_seg, lds, st);
        case 2: return launch_jaccard_qb<2>(a, n_seg, lds, st);
        case 4: return launch_jaccard_qb<4>(a, n_seg, lds, st);
        case 8: return launch_jaccard_qb<8>(a, n_seg, lds, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vdb
