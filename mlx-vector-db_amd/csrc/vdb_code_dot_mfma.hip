// vdb_code_dot_mfma.hip: the int8-MFMA form of the code-dot search (vdb_index_search_code_dot at large
// batches and k <= 64; the bit-plane form: vdb_code_dot.hip; the column: vdb_hamming.hip).
//
// A stored bit is the int8 0 / 1 and the query is int8 already, so v_mfma_i32_32x32x32_i8 forms s(b, r)
// = sum_j q[b][j] * bit_j(code r) as it stands; |s| <= 2^20, the i32 accumulators are exact, and zero
// pad bits and pad rows of the column add nothing whatever the query holds there.
//
// code_dot_mfma_kernel: grid (n_seg, blocks of 64 queries), 4 waves.  The workgroup walks chunks s, s +
// n_seg, ... of 4 tiles; per trip wave w takes tile 4 c + w as two 32-row sub-tiles against the two
// query tiles: four 32 x 32 accumulators, as the Hamming form.  The row side is that form's: lane l
// reads word 2 j + l / 32 of row l % 32, which feeds four MFMA steps, 16 bits each expanded to 0 / 1
// bytes in registers; the next word pair is loaded before the current one is expanded.
//
// The query side is what differs.  Under the row mapping the operand of lane l at step s is 16
// consecutive int8 values of query l % 32: piece cd_mfma_piece(s, l / 32) of the row-major query, used
// without any expansion.  The block's queries lie in LDS piece-major, [piece][64 queries][16 B], so the
// 32 lanes of a half read 512 consecutive bytes: one conflict-free ds_read_b128 per query tile and
// step, used by both sub-tiles.  Pad pieces, the upper half of a half piece (an odd n_bytes) and
// absent queries are zero.
//
// K chunks.  64 queries of 8 * n_bytes values are up to 512 KiB, so K goes through LDS in chunks of
// kCdMfmaChunkPairs word pairs (vdb_code_dot_plan.h: what fits beside the candidate buffers).  A code
// of one chunk is staged once per workgroup.  A longer one is staged chunk by chunk in every trip, by
// all 256 threads between two barriers, with the waves' accumulators live across the chunks; a wave
// whose tile the mask rules out still stages and keeps the barriers.
//
// Top-k is vdb_mfma_topk.h's with the key (2^20 - s) << 32 | row: one unsigned compare ranks (s
// descending, row ascending).  Segments' lists go to the Hamming search's scratch as -(float)(2^20 - s)
// and are merged by a second launch, one workgroup per query; the scores are written from the key.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_code_dot_plan.h"
#include "vdb_code_dot_tail.h"
#include "vdb_mfma_topk.h"

namespace vdb {

// Pairs [p0, p1) of the block's queries into LDS, piece-major; a thread moves 8 bytes.  Adjacent
// threads take adjacent queries of one piece: the LDS stores are conflict free, and the 16-byte runs
// of the global reads come from lines the block reads whole within the chunk.
__device__ __forceinline__ void cd_stage_pairs(const CodeDotArgs& a, int b0, int nq, int p0, int p1, bool aligned, char* smem) {
    const int n_bits = 8 * a.n_bytes;
    const int units = (p1 - p0) * kCdPiecesPerPair * QB * 2;
    for (int i = threadIdx.x; i < units; i += 256) {
        const int h8 = i & 1, q = (i >> 1) & (QB - 1), lp = i >> 7;
        const int d0 = kCdPieceBytes * (kCdPiecesPerPair * p0 + lp) + 8 * h8;  // the first dimension of these 8 bytes
        uint64_t v = 0;
        if (q < nq && d0 < n_bits) v = cd_load8(a.queries + (size_t)(b0 + q) * n_bits + d0, aligned);
        *reinterpret_cast<uint64_t*>(smem + cd_mfma_piece_off(lp, q) + 8 * h8) = v;
    }
}
static_assert(QB * 2 == 128, "cd_stage_pairs splits a unit's index by shifts");

// (two waves per SIMD: a code of one chunk leaves LDS for a second workgroup)
__global__ void __launch_bounds__(256, 2) code_dot_mfma_kernel(CodeDotArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_flag[2];
    const int KE = a.KE, k = a.k;
    const int W = a.W;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int s = blockIdx.x;
    const int n_seg = (int)gridDim.x;
    const int b0 = blockIdx.y * QB;
    const int nq = a.n_queries - b0 < QB ? a.n_queries - b0 : QB;
    uint64_t* cand = reinterpret_cast<uint64_t*>(smem + cd_mfma_cand_off(W));
    uint64_t* thr = reinterpret_cast<uint64_t*>(smem + cd_mfma_thr_off(W));
    int* cnt = reinterpret_cast<int*>(smem + cd_mfma_cnt_off(W));

    const int live = ham_live_segs(a.N, n_seg);
    if (live == 0) {  // no rows: "no result" in every slot
        if (s == 0)
            for (int q = 0; q < nq; ++q)
                for (int e = threadIdx.x; e < k; e += 256) code_dot_write(a, b0 + q, e, 0.f, 0, 0xFFFFFFFFu);
        return;
    }
    if (s >= live) return;  // more segments than chunks: nothing to do

    const bool aligned = (reinterpret_cast<uintptr_t>(a.queries) & 7u) == 0;
    const int n_pairs = cd_mfma_pairs(W);
    const int n_kch = cd_mfma_k_chunks(W);
    if (n_kch == 1) cd_stage_pairs(a, b0, nq, 0, n_pairs, aligned, smem);  // the whole code, once
    if (threadIdx.x < QB) {
        thr[threadIdx.x] = kNoKey;
        cnt[threadIdx.x] = 0;
    }
    if (threadIdx.x < 2) s_flag[threadIdx.x] = 0;
    __syncthreads();
    const auto key_hi = [](int, int dot) { return cd_key_hi(dot); };
    int cnt0 = 0;  // thread q < QB: query q's count at the trip's start

    const int64_t n_tiles = ham_n_tiles(a.N);
    const int64_t n_chunks = ham_n_chunks(a.N);
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
        const bool has_tile = (vm[0] | vm[1]) != 0u;  // (wave-uniform; a tile the mask rules out whole is not read)
        const uint64_t* xt = a.codes + (size_t)(has_tile ? t : 0) * W * kHamTileRows + col;
        uint64_t xn[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) xn[rt] = (vm[rt] != 0u && half < W) ? xt[(size_t)half * kHamTileRows + 32 * rt] : 0ull;
        for (int ch = 0; ch < n_kch; ++ch) {
            const int p0 = ch * kCdMfmaChunkPairs;
            const int p1 = p0 + kCdMfmaChunkPairs < n_pairs ? p0 + kCdMfmaChunkPairs : n_pairs;
            if (n_kch > 1) {
                if (ch > 0) __syncthreads();  // the last chunk's pieces are read (chunk 0: the trip before ended in a barrier)
                cd_stage_pairs(a, b0, nq, p0, p1, aligned, smem);
                __syncthreads();
            }
            if (!has_tile) continue;
            for (int j = p0; j < p1; ++j) {
                uint64_t x[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) x[rt] = xn[rt];
                const int wn = ham_mfma_word(4 * (j + 1), half);  // the next pair's word of this lane half
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    xn[rt] = (j + 1 < n_pairs && vm[rt] != 0u && wn < W) ? xt[(size_t)wn * kHamTileRows + 32 * rt] : 0ull;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int sh = ham_mfma_shift(m);
                    const int lp = cd_mfma_piece(4 * j + m, half) - kCdPiecesPerPair * p0;
                    ham_i32x4 xa[RT], qa[QT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) xa[rt] = expand_row16(x[rt], sh);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt)
                        qa[qt] = *reinterpret_cast<const ham_i32x4*>(smem + cd_mfma_piece_off(lp, 32 * qt + col));
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int qt = 0; qt < QT; ++qt)
                            acc[rt][qt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(xa[rt], qa[qt], acc[rt][qt], 0, 0, 0);
                }
            }
        }
        mfma_rank_trip(acc, vm, t, mfma_value_key(key_hi), nq, k, trip, s_flag, cnt0, cand, thr, cnt);
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
                code_dot_write(a, b0 + q, e, -(float)(uint32_t)(key >> 32), kCdBias, e < c ? (uint32_t)key : 0xFFFFFFFFu);
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

// The segments' lists of query b, merged: one workgroup per query (as hamming_mfma_merge_kernel).
__global__ void __launch_bounds__(256) code_dot_mfma_merge_kernel(CodeDotArgs a, int n_seg, int live) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x;
    const int KE = a.KE;
    const size_t l0 = (size_t)b * n_seg * KE;
    merge_block<float, uint32_t>(a.lk + l0, a.li + l0, live, KE, KE, KE, a.mk + (size_t)b * KE, a.mi + (size_t)b * KE, smem);
    __syncthreads();
    for (int e = threadIdx.x; e < a.k; e += 256) code_dot_write(a, b, e, a.mk[(size_t)b * KE + e], kCdBias, a.mi[(size_t)b * KE + e]);
}

size_t code_dot_mfma_lds_bytes(int W) { return (size_t)cd_mfma_lds_bytes(W); }

hipError_t launch_code_dot_mfma(const CodeDotArgs& a, int n_seg, hipStream_t st) {
    if (a.n_queries <= 0) return hipSuccess;
    const int W = ham_words(a.n_bytes);
    if (a.n_queries > kHamMaxQueries || n_seg < 1 || n_seg > kHamMaxSeg || a.k < 1 || a.k > kHamMfmaMaxK ||
        a.KE != ham_ke(a.k) || a.N < 0 || a.N > 0xFFFFFFFEll || a.n_bytes < 1 || a.n_bytes > kHamMaxBytes || a.W != W ||
        !a.queries || (a.N > 0 && !a.codes) || !a.out_s || !a.out_i ||
        (n_seg > 1 && (!a.lk || !a.li || !a.mk || !a.mi)))
        return hipErrorInvalidValue;
    // the plan header restates the merge buffer without HIP
    if ((size_t)ham_merge_lds(a.KE) != merge_block_lds<float, uint32_t>(a.KE)) return hipErrorInvalidValue;
    const size_t lds = code_dot_mfma_lds_bytes(W);
    if (lds + (size_t)kHamMfmaStaticLds > (size_t)kHamLdsLimit) return hipErrorInvalidValue;
    if (lds > 65536) {  // (set per launch, for the device that is current)
        const hipError_t e =
            hipFuncSetAttribute((const void*)code_dot_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(code_dot_mfma_kernel, dim3(n_seg, ham_n_blocks(a.n_queries, QB)), dim3(256), lds, st, a);
    hipError_t e = hipGetLastError();
    const int live = ham_live_segs(a.N, n_seg);
    if (e != hipSuccess || live <= 1) return e;  // (one list: the scan wrote the results itself)
    hipLaunchKernelGGL(code_dot_mfma_merge_kernel, dim3(a.n_queries), dim3(256), (size_t)ham_merge_lds(a.KE), st, a, n_seg, live);
    return hipGetLastError();
}

}  // namespace vdb
