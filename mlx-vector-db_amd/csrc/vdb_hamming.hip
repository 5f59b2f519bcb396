// vdb_hamming.hip: the binary code column and the exact Hamming search (vdb_index_set_codes,
// vdb_index_search_hamming), part of the gfx950 kernels of the brute-force distance + top-k path
// (pipeline overview: vdb_scan.hip).
//
// Every stored row carries a code of n_bytes bytes.  The distance of a query to a row is the number
// of bits in which the two differ; rows rank by (distance ascending, row ascending).  Distances are
// integers, so there is no summation order and no certificate: the result is what a numpy
// restatement gives, bit for bit.
//
// Layout.  A lane takes a row, and rows of the caller's row-major array lie n_bytes apart: a wave
// reading "byte group w of its 64 rows" would gather.  hamming_pack_kernel therefore repacks the
// column once, when it is attached, into tiles of 64 rows that are word-major inside:
// [n_tiles][W][64] 64-bit words (vdb_hamming_plan.h), pad bytes and pad rows zero.  Word w of a
// wave's 64 rows is then one coalesced 512-byte load, and zero padding on both sides of the XOR adds
// nothing to a popcount.
//
// hamming_kernel<QB>: grid (n_seg, query blocks), 4 waves.  The codes are small and a popcount is
// cheap, so the kernel is shaped to read the column once per block of QB queries instead of once
// per query.  A workgroup puts its block's queries into LDS as 64-bit words (zero padded to whole
// passes, absent queries zero) and walks chunks s, s + n_seg, ... of 4 tiles; wave w takes tile 4 c
// + w.  A lane loads up to 16 words of its row into registers (one pass; longer codes take several)
// and for each query of the block adds popcount(x_w ^ q_w) into one of QB integer accumulators.  The
// query words are wave-uniform: every lane reads the same LDS address, which the LDS serves as a
// broadcast, so they cost no per-lane registers and no memory traffic.  The tile's two mask words
// are loaded by two lanes and shared by a shuffle.
//
// Top-k.  Per (wave, query of the block) one WaveTopK<float, uint32_t> in LDS, keyed by the negated
// distance: fp32 holds every integer up to 8 192 exactly, and "higher is better, ties to the lower
// row" becomes (distance asc, row asc).  Wave 0 folds the four waves' lists per query; the
// workgroup that finishes a block last merges the segments' lists per query with merge_block and
// writes the outputs (a per-block counter, release / acquire fences around it, left zero on exit).
// A query needs no validation: any bytes are a query.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_hamming_plan.h"
#include "vdb_hamming_tail.h"

namespace vdb {

static_assert(kHamMergeBuf == MERGE_BUF, "ham_merge_lds restates merge_block_lds");
static_assert(kHamMaxSeg <= MERGE_HEADS, "the tail merge's select path takes at most MERGE_HEADS lists");

// ---- the column -------------------------------------------------------------------------------
// One thread per packed word: (tile, w, lane) <- bytes [8 w, 8 w + 8) of row 64 tile + lane, zero
// past n_bytes and past n.  The strided byte reads happen once per attach; the stores are coalesced.
__global__ void __launch_bounds__(256) hamming_pack_kernel(const uint8_t* __restrict__ codes, int64_t n, int n_bytes, int W,
                                                           uint64_t* __restrict__ packed, int64_t n_words) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n_words) return;
    const int lane = (int)(o & 63);
    const int64_t tw = o >> 6;
    const int w = (int)(tw % W);
    const int64_t r = (tw / W) * kHamTileRows + lane;
    packed[o] = r < n ? ham_word_of(codes + r * n_bytes, n_bytes, w) : 0ull;
}

hipError_t launch_hamming_pack(const uint8_t* codes, int64_t n, int n_bytes, uint64_t* packed, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!codes || !packed || n_bytes < 1 || n_bytes > kHamMaxBytes) return hipErrorInvalidValue;
    const int W = ham_words(n_bytes);
    const int64_t n_words = ham_packed_words(n, W);
    const int64_t blocks = (n_words + 255) / 256;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hamming_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, codes, n, n_bytes, W, packed, n_words);
    return hipGetLastError();
}

// ---- the search -------------------------------------------------------------------------------
template <int QB>
__global__ void __launch_bounds__(256) hamming_kernel(HammingArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef WaveTopK<float, uint32_t> TopK;
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
    char* tkmem = smem + ham_query_lds(QB, W);

    const int live = ham_live_segs(a.N, n_seg);
    if (live == 0) {  // no rows: "no result" in every slot
        if (s == 0)
            for (int q = 0; q < nq; ++q)
                for (int e = threadIdx.x; e < a.k; e += 256) hamming_write(a, b0 + q, e, -INFINITY, 0xFFFFFFFFu);
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
        tk[q].init(reinterpret_cast<float*>(smem + ham_lds_key_off(wv, q, QB, W, KE)),
                   reinterpret_cast<uint32_t*>(smem + ham_lds_row_off(wv, q, QB, W, KE)), KE);
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
        const uint64_t* xt = a.codes + (size_t)t * W * kHamTileRows + lane;
        for (int w0 = 0; w0 < W; w0 += kHamPassWords) {
            uint64_t x[kHamPassWords];
#pragma unroll
            for (int j = 0; j < kHamPassWords; ++j) x[j] = w0 + j < W ? xt[(size_t)(w0 + j) * kHamTileRows] : 0ull;
#pragma unroll
            for (int q = 0; q < QB; ++q) {
                const uint64_t* qq = qs + q * WS + w0;  // wave-uniform: an LDS broadcast
                int d = acc[q];
#pragma unroll
                for (int j = 0; j < kHamPassWords; ++j) d += __popcll(x[j] ^ qq[j]);
                acc[q] = d;
            }
        }
#pragma unroll
        for (int q = 0; q < QB; ++q)
            if (q < nq) tk[q].offer(in, -(float)acc[q], in ? (uint32_t)row : 0xFFFFFFFFu);
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
                const float* ok = reinterpret_cast<const float*>(smem + ham_lds_key_off(w, q, QB, W, KE));
                const uint32_t* oi = reinterpret_cast<const uint32_t*>(smem + ham_lds_row_off(w, q, QB, W, KE));
                for (int e0 = 0; e0 < KE; e0 += 64) {
                    const int e = e0 + lane;
                    const bool inb = e < KE && oi[e] != 0xFFFFFFFFu;
                    tk[q].offer(inb, inb ? ok[e] : -INFINITY, inb ? oi[e] : 0xFFFFFFFFu);
                }
            }
            tk[q].finish();
            const float* bk = tk[q].bk;
            const uint32_t* bi = tk[q].bi;
            if (live == 1) {  // the only list of this query: straight to the results
                for (int e = lane; e < a.k; e += 64)
                    hamming_write(a, b0 + q, e, e < KE ? bk[e] : -INFINITY, e < KE ? bi[e] : 0xFFFFFFFFu);
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
        merge_block<float, uint32_t>(a.lk + l0, a.li + l0, live, KE, KE, KE, a.mk + (size_t)b * KE, a.mi + (size_t)b * KE,
                                     tkmem);
        __syncthreads();
        for (int e = threadIdx.x; e < a.k; e += 256) hamming_write(a, b, e, a.mk[(size_t)b * KE + e], a.mi[(size_t)b * KE + e]);
    }
    if (threadIdx.x == 0) a.done[blockIdx.y] = 0;  // left zero for the next call on this workspace
}

size_t hamming_search_lds_bytes(int qb, int W, int KE, int n_seg) { return (size_t)ham_lds_bytes(qb, W, KE, n_seg > 1); }

template <int QB>
static hipError_t launch_hamming_qb(const HammingArgs& a, int n_seg, size_t lds, hipStream_t st) {
    if (lds > 65536) {  // (set per launch, for the device that is current)
        const hipError_t e =
            hipFuncSetAttribute((const void*)hamming_kernel<QB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(hamming_kernel<QB>, dim3(n_seg, ham_n_blocks(a.n_queries, QB)), dim3(256), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_hamming_search(const HammingArgs& a, int qb, int n_seg, hipStream_t st) {
    if (a.n_queries <= 0) return hipSuccess;
    const int W = ham_words(a.n_bytes);
    if (a.n_queries > kHamMaxQueries || n_seg < 1 || n_seg > kHamMaxSeg || a.k < 1 || a.k > a.KE || a.KE != ham_ke(a.k) ||
        a.KE > kHamMaxK || a.N < 0 || a.N > 0xFFFFFFFEll || a.n_bytes < 1 || a.n_bytes > kHamMaxBytes || a.W != W ||
        qb != ham_block(a.k, a.n_queries) || !a.queries || (a.N > 0 && !a.codes) || !a.out_d || !a.out_i ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi || !a.done)))
        return hipErrorInvalidValue;
    // the plan header restates these two without HIP
    if (ham_cap(a.KE) != WaveTopK<float, uint32_t>::capacity(a.KE) ||
        (size_t)ham_merge_lds(a.KE) != merge_block_lds<float, uint32_t>(a.KE))
        return hipErrorInvalidValue;
    const size_t lds = hamming_search_lds_bytes(qb, W, a.KE, n_seg);
    if (lds > (size_t)kHamLdsLimit) return hipErrorInvalidValue;
    switch (qb) {
        case 1: return launch_hamming_qb<1>(a, n_seg, lds, st);
        case 2: return launch_hamming_qb<2>(a, n_seg, lds, st);
        case 4: return launch_hamming_qb<4>(a, n_seg, lds, st);
        case 8: return launch_hamming_qb<8>(a, n_seg, lds, st);
        case 16: return launch_hamming_qb<16>(a, n_seg, lds, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vdb
