// vdb_code_dot.hip: the bit-plane form of the code-dot search (vdb_index_search_code_dot), every k and
// every batch: int8 queries against the 1-bit code column of vdb_hamming.hip, s(b, r) = sum_j q[b][j] *
// bit_j(code r), ranked by (s descending, row ascending).  (The int8-MFMA form: vdb_code_dot_mfma.hip.)
//
// The identity.  In two's complement an m-bit value is -2^(m-1) v_(m-1) + sum_{p < m-1} 2^p v_p.  With
// P_p the bits p of a query over all dimensions -- a bit vector as wide as a code --
//     s = sum_{p < m-1} 2^p popcount(x & P_p) - 2^(m-1) popcount(x & P_(m-1)),
// integers throughout.  The column stays bits in HBM and is read once per block of queries.
//
// code_dot_kernel<QB>: grid (n_seg, query blocks), 4 waves; the popcount search's work split: the
// workgroup walks chunks s, s + n_seg, ... of 4 tiles, wave w takes tile 4 c + w, a lane takes a row and
// holds kHamPassWords words of it in registers per pass.
//
// Staging.  The block's queries are transposed into planes once: a thread takes the eight values that
// pair with one code byte (one 8-byte load) and writes that byte of each of the eight planes.  LDS
// holds [query][plane][word] (vdb_code_dot_plan.h), so the inner loop's read of "word w of plane p of
// query q" is one address for the whole wave, which LDS serves as a broadcast.  While staging, the
// block finds m, the fewest bits that hold every value of every one of its queries (an LDS max); the
// inner loop then runs m planes, the top one weighted -2^(m-1).  A block of int4 queries costs four
// AND + popcount per word and query, a block of 0 / -1 queries one.  m is uniform over the workgroup
// and only a loop bound.  Pad bytes, pad words and absent queries are zero planes.
//
// Top-k, lists and merge are the popcount search's: per (wave, query) a WaveTopK<float, uint32_t> keyed
// by the score (|s| <= 2^20, exact in fp32; higher is better, ties to the lower row), wave 0 folds the
// four waves' lists, and the workgroup that finishes a block last merges the segments' lists.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_code_dot_plan.h"
#include "vdb_code_dot_tail.h"

namespace vdb {

template <int QB>
__global__ void __launch_bounds__(256) code_dot_kernel(CodeDotArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_m, s_last;
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
    const uint64_t* planes = reinterpret_cast<const uint64_t*>(smem);
    char* tkmem = smem + cd_plane_lds(QB, W);

    const int live = ham_live_segs(a.N, n_seg);
    if (live == 0) {  // no rows: "no result" in every slot
        if (s == 0)
            for (int q = 0; q < nq; ++q)
                for (int e = threadIdx.x; e < a.k; e += 256) code_dot_write(a, b0 + q, e, 0.f, 0, 0xFFFFFFFFu);
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do, and not counted below

    if (threadIdx.x == 0) s_m = 1;
    __syncthreads();
    {
        // byte g of a code pairs with values [8 g, 8 g + 8) of a query: byte g of each of its planes
        const bool aligned = (reinterpret_cast<uintptr_t>(a.queries) & 7u) == 0;
        const int n_bits = 8 * a.n_bytes, SB = WS * 8;
        int need = 1;
        for (int i = threadIdx.x; i < QB * SB; i += 256) {
            const int q = i / SB, g = i - q * SB;
            uint64_t v = 0;
            if (q < nq && g < a.n_bytes) {
                v = cd_load8(a.queries + (size_t)(b0 + q) * n_bits + 8 * g, aligned);
                const int nb = cd_bits_needed8(v);
                need = nb > need ? nb : need;
            }
#pragma unroll
            for (int p = 0; p < kCdMaxPlanes; ++p) smem[cd_plane_byte_off(q, p, W) + g] = (char)cd_plane_byte(v, p);
        }
        if (need > 1) atomicMax(&s_m, need);
    }
    TopK tk[QB];
#pragma unroll
    for (int q = 0; q < QB; ++q)
        tk[q].init(reinterpret_cast<float*>(smem + cd_lds_key_off(wv, q, QB, W, KE)),
                   reinterpret_cast<uint32_t*>(smem + cd_lds_row_off(wv, q, QB, W, KE)), KE);
    __syncthreads();
    const int m = s_m;  // the block's plane count

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
                const uint64_t* pq = planes + (size_t)q * kCdMaxPlanes * WS + w0;  // wave-uniform: LDS broadcasts
                int d = acc[q];
                for (int p = 0; p < m; ++p) {
                    const uint64_t* pp = pq + (size_t)p * WS;
                    int cbits = 0;
#pragma unroll
                    for (int j = 0; j < kHamPassWords; ++j) cbits += __popcll(x[j] & pp[j]);
                    d += cbits * cd_plane_weight(p, m);
                }
                acc[q] = d;
            }
        }
#pragma unroll
        for (int q = 0; q < QB; ++q)
            if (q < nq) tk[q].offer(in, in ? (float)acc[q] : -INFINITY, in ? (uint32_t)row : 0xFFFFFFFFu);
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
                const float* ok = reinterpret_cast<const float*>(smem + cd_lds_key_off(w, q, QB, W, KE));
                const uint32_t* oi = reinterpret_cast<const uint32_t*>(smem + cd_lds_row_off(w, q, QB, W, KE));
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
                    code_dot_write(a, b0 + q, e, e < KE ? bk[e] : 0.f, 0, e < KE ? bi[e] : 0xFFFFFFFFu);
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
        for (int e = threadIdx.x; e < a.k; e += 256) code_dot_write(a, b, e, a.mk[(size_t)b * KE + e], 0, a.mi[(size_t)b * KE + e]);
    }
    if (threadIdx.x == 0) a.done[blockIdx.y] = 0;  // left zero for the next call on this workspace
}

size_t code_dot_lds_bytes(int qb, int W, int KE, int n_seg) { return (size_t)cd_lds_bytes(qb, W, KE, n_seg > 1); }

template <int QB>
static hipError_t launch_code_dot_qb(const CodeDotArgs& a, int n_seg, size_t lds, hipStream_t st) {
    if (lds > 65536) {  // (set per launch, for the device that is current)
        const hipError_t e =
            hipFuncSetAttribute((const void*)code_dot_kernel<QB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(code_dot_kernel<QB>, dim3(n_seg, ham_n_blocks(a.n_queries, QB)), dim3(256), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_code_dot(const CodeDotArgs& a, int qb, int n_seg, hipStream_t st) {
    if (a.n_queries <= 0) return hipSuccess;
    const int W = ham_words(a.n_bytes);
    if (a.n_queries > kHamMaxQueries || n_seg < 1 || n_seg > kHamMaxSeg || a.k < 1 || a.k > a.KE || a.KE != ham_ke(a.k) ||
        a.KE > kHamMaxK || a.N < 0 || a.N > 0xFFFFFFFEll || a.n_bytes < 1 || a.n_bytes > kHamMaxBytes || a.W != W ||
        qb != cd_block(a.k, W, a.n_queries) || !a.queries || (a.N > 0 && !a.codes) || !a.out_s || !a.out_i ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi || !a.done)))
        return hipErrorInvalidValue;
    // the plan header restates these two without HIP
    if (ham_cap(a.KE) != WaveTopK<float, uint32_t>::capacity(a.KE) ||
        (size_t)ham_merge_lds(a.KE) != merge_block_lds<float, uint32_t>(a.KE))
        return hipErrorInvalidValue;
    const size_t lds = code_dot_lds_bytes(qb, W, a.KE, n_seg);
    if (lds + (size_t)kCdStaticLds > (size_t)kHamLdsLimit) return hipErrorInvalidValue;
    switch (qb) {
        case 1: return launch_code_dot_qb<1>(a, n_seg, lds, st);
        case 2: return launch_code_dot_qb<2>(a, n_seg, lds, st);
        case 4: return launch_code_dot_qb<4>(a, n_seg, lds, st);
        case 8: return launch_code_dot_qb<8>(a, n_seg, lds, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vdb
