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
// Top-k.  A lane holds one query and 16 rows of an accumulator.  Each query has, in LDS, its
// threshold (the k-th best key so far; a key is distance << 32 | row, so "distance ascending, row
// ascending" is one unsigned compare) and one candidate buffer shared by the four waves.  A lane
// tests an accumulator register against its query's threshold; one ballot skips the register when
// nothing passes; a passing entry takes its place in the buffer by an LDS atomic add on the query's
// count.  The order of the appends therefore varies from run to run.  The result does not: the keys
// of a query are distinct (a row appears once), the ranking is a total order, a compaction keeps
// exactly the k smallest keys of what the buffer holds, and an entry is only ever dropped by a test
// against the k-th smallest key of some subset of the rows -- which no row of the final k fails.
// Compaction (one wave per query): every lane ranks its two entries against the whole buffer and
// stores those of rank < k at their rank, which also sorts them.
//
// A buffer cannot be compacted by one wave while the others append, so the trips are uniform across
// the workgroup (a wave without a tile only keeps the barriers) and each ends with a barrier and a
// flag word.  Bit 1: some buffer passed kHamMfmaHigh entries; the buffers above it are compacted.
// Bit 0: an append found its buffer full.  Then the counts go back to their values at the trip's
// start, every buffer is compacted to k, and the four waves offer their accumulators again one after
// the other with a compaction between them; one wave's offers always fit (vdb_hamming_plan.h).  That
// happens in the first trips, while the thresholds are loose, and costs no MFMA work.
//
// Segments' lists are written as the popcount form writes them (negated distance as fp32, row) into
// the same scratch and merged by the same merge_block, but in a second launch with one workgroup per
// query (hamming_mfma_merge_kernel): the `done` counters are not used and stay zero.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_merge_block.h"
#include "vdb_hamming_plan.h"
#include "vdb_hamming_tail.h"

namespace vdb {

typedef int ham_i32x4 __attribute__((ext_vector_type(4)));
typedef int ham_i32x16 __attribute__((ext_vector_type(16)));

constexpr int QT = kHamMfmaQT;
constexpr int QB = kHamMfmaQB;
constexpr int RT = kHamTileRows / 32;  // sub-tiles of a tile
constexpr int CAP = kHamMfmaCap;
static_assert(CAP == 128, "a lane ranks two entries of a buffer");
constexpr uint64_t kNoKey = ~0ull;

// 16 bits of a word from bit `sh` up as one MFMA operand: bit i to byte i.
__device__ __forceinline__ ham_i32x4 expand_row16(uint64_t x, int sh) {
    ham_i32x4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d) r[d] = (int)ham_mfma_row4((uint32_t)(x >> (sh + 4 * d)));
    return r;
}
__device__ __forceinline__ ham_i32x4 expand_query16(uint64_t x, int sh) {
    ham_i32x4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d) r[d] = (int)ham_mfma_query4((uint32_t)(x >> (sh + 4 * d)));
    return r;
}

// A wave offers its tile's accumulators.  vm[rt]: the candidate rows of sub-tile rt as bits.  Returns
// the flag bits of the header comment.
__device__ __forceinline__ int mfma_offer(const ham_i32x16 (&acc)[RT][QT], const uint32_t (&vm)[RT], int64_t t,
                                          const int (&qpop)[QT], int nq, int k_high, uint64_t* cand, const uint64_t* thr,
                                          int* cnt) {
    const int lane = threadIdx.x & 63;
    const int col = lane & 31, half = lane >> 5;
    int flag = 0;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        if (vm[rt] == 0) continue;  // (wave-uniform) a sub-tile with no candidate row
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            if (32 * qt >= nq) continue;  // (uniform) a query tile with no query
            const int q = 32 * qt + col;
            const uint64_t th = q < nq ? thr[q] : 0ull;  // an absent query passes nothing
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int rl = 8 * (v >> 2) + 4 * half + (v & 3);  // the accumulator layout: row of register v
                const uint32_t row = (uint32_t)(t * kHamTileRows + 32 * rt + rl);
                const uint32_t d = (uint32_t)(qpop[qt] - acc[rt][qt][v]);
                const uint64_t key = ((uint64_t)d << 32) | row;
                const bool pass = ((vm[rt] >> rl) & 1u) && key < th;
                if (__ballot(pass) == 0ull) continue;
                if (pass) {
                    const int pos = atomicAdd(&cnt[q], 1);
                    if (pos < CAP) {
                        cand[(size_t)q * CAP + pos] = key;
                        if (pos >= k_high) flag |= 2;
                    } else {
                        flag |= 1;
                    }
                }
            }
        }
    }
    return flag;
}

__device__ __forceinline__ uint64_t lane_key(uint64_t v, int src /* wave-uniform */) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// One wave compacts query q's buffer: the k smallest keys, sorted, and the threshold once there are k.
__device__ __forceinline__ void mfma_compact(int q, int k, uint64_t* cand, uint64_t* thr, int* cnt) {
    const int lane = threadIdx.x & 63;
    uint64_t* b = cand + (size_t)q * CAP;
    const int c = __builtin_amdgcn_readfirstlane(cnt[q]);
    const uint64_t m0 = lane < c ? b[lane] : kNoKey;
    const uint64_t m1 = lane + 64 < c ? b[lane + 64] : kNoKey;
    // entry j comes out of lane j % 64's register (a lane read with a uniform index): no LDS round
    // trip per entry
    int r0 = 0, r1 = 0;
    for (int j = 0; j < (c < 64 ? c : 64); ++j) {
        const uint64_t kj = lane_key(m0, j);
        r0 += kj < m0;
        r1 += kj < m1;
    }
    for (int j = 64; j < c; ++j) {
        const uint64_t kj = lane_key(m1, j - 64);
        r0 += kj < m0;
        r1 += kj < m1;
    }
    // every read above is complete before the stores below (LDS accesses of a wave complete in order)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < c && r0 < k) b[r0] = m0;
    if (lane + 64 < c && r1 < k) b[r1] = m1;
    if (c >= k) {
        if (lane < c && r0 == k - 1) thr[q] = m0;
        if (lane + 64 < c && r1 == k - 1) thr[q] = m1;
    }
    if (lane == 0) cnt[q] = c < k ? c : k;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// Wave wv compacts queries wv, wv + 4, ... whose buffers hold more than `above` entries.
__device__ __forceinline__ void mfma_compact_all(int above, int nq, int k, uint64_t* cand, uint64_t* thr, int* cnt) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int q = wv; q < nq; q += kHamWaves)
        if (cnt[q] > above) mfma_compact(q, k, cand, thr, cnt);
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
        // round 0: every wave offers its tile; rounds 1..4, after a full buffer only: wave r - 1 alone.
        // (The first trip starts at round 1: without thresholds every row passes and round 0 would
        // only find the buffers full.)
        const bool has_tile = (vm[0] | vm[1]) != 0u;
        for (int r = trip == 0 ? 1 : 0; r <= kHamWaves; ++r) {
            if (has_tile && (r == 0 || wv == r - 1)) {
                const int flag = mfma_offer(acc, vm, t, qpop, nq, kHamMfmaHigh, cand, thr, cnt);
                if (r == 0 && flag) atomicOr(&s_flag[trip & 1], flag);
            }
            __syncthreads();  // the round's appends are made
            if (r == 0) {
                const int f = s_flag[trip & 1];
                if (threadIdx.x == 0) s_flag[(trip + 1) & 1] = 0;  // (last read a trip ago, next set after this trip's last barrier)
                if (!(f & 1)) {
                    if (f & 2) {
                        mfma_compact_all(kHamMfmaHigh, nq, k, cand, thr, cnt);
                        __syncthreads();
                    }
                    break;
                }
                // a full buffer: back to the trip's start and compact, then one wave's offers at a time
                if (threadIdx.x < QB) cnt[threadIdx.x] = cnt0;
                __syncthreads();
            }
            mfma_compact_all(k, nq, k, cand, thr, cnt);
            __syncthreads();
        }
        if (threadIdx.x < QB) cnt0 = cnt[threadIdx.x];
        __syncthreads();  // the counts are read before the next trip's appends
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
