// vdb_jaccard_range.hip: the Jaccard range search (vdb_index_search_jaccard_range) -- every row of the
// binary code column whose Jaccard / Tanimoto similarity with a query is at or above that query's
// rational threshold, with exact counts; part of the gfx950 kernels of the brute-force path (the column
// and its layout: vdb_hamming.hip; the hit bitmap, its prefix and the id emit: vdb_range.hip; the
// geometry of chunks, tiles and words: vdb_hamming_range_plan.h).
//
// The decision.  i = |q AND x|, u = |q| + |x| - i, threshold num / den: the row passes when i * den >=
// num * u (jac_range_pass: two unsigned 32-bit multiplies and a compare, exact, u == 0 as 1 / 1).  A
// threshold the call's contract rules out (jac_range_bad_threshold; only a device-memory call can carry
// one this far) and an absent query of a block are replaced once, when the block is loaded, by the pair
// (1, 0), which no row passes: the per-pair test knows nothing of either.
//
// Two scans fill the hit bitmap H [block][n_words] and the chunk counts part [block][n_chunks],
// identical in every byte; the grid of both is one workgroup of 4 waves per 512-row chunk, and wave w
// takes the chunk's tiles 2 w and 2 w + 1, its words 4 w .. 4 w + 3.
//
//   popcount  blocks of up to 16 queries.  One lane per row; the block's query words (whole passes,
//             zero padded), |q|, num and den are in LDS, read wave-uniformly as broadcasts.  A lane
//             holds a pass of its row's words in registers and counts |x| from them once per pass, for
//             every query of the block.  A code of one pass is decided query after query with nothing
//             kept per query; a longer code carries a running i per query and a running |x|.
//             __ballot(eligible && pass) is the tile's two bitmap words of that query as they are.
//   MFMA      blocks of 64 queries through v_mfma_i32_32x32x32_i8, both operands as the int8 0 / 1: the
//             accumulators hold i.  A lane counts the bits of the row words it loads as they pass; one
//             exchange with lane ^ 32 completes |x| of the tile's 64 rows (both sub-tiles in one
//             register), parked in the wave's 64 words of LDS.  In the epilogue a lane reads |x| of its
//             16 accumulator rows back (two addresses per wave and register: broadcasts), forms u, tests
//             and packs 16 bits that already sit at their row positions; the OR with lane ^ 32's bits is
//             the finished bitmap word of (query, sub-tile).  Eligibility is one AND with the
//             wave-uniform word.  The words are staged in LDS as [64 queries][17], written to H as
//             64-byte runs per query and summed into part.
//
// Then range_prefix_kernel / range_emit_kernel (launch_range_prefix_emit), and with cap > 0
// jaccard_range_fill_kernel: for each filled slot it reads the id back, recounts i and |x| from the
// packed column and writes i and u (the raw popcounts: 0 / 0 for two empty sets); the slots from
// min(count, cap) to cap get -1 / -1 / -1.  That is work proportional to the answer.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_jaccard_range_plan.h"

namespace vdb {

namespace {

typedef int jr_i32x4 __attribute__((ext_vector_type(4)));
typedef int jr_i32x16 __attribute__((ext_vector_type(16)));

constexpr int QT = kHamMfmaQT;
constexpr int MQB = kJacRangeMfmaQB;
constexpr int RT = kHamRangeTileWords;  // 32-row sub-tiles of a tile = its bitmap words
static_assert(MQB == 64 && QT == 2 && RT == 2, "the MFMA scan's staging and store loops assume 64 queries, 2 x 2 accumulators");

// The eligible rows of bitmap word w as bits, in a scalar register (every lane reads the same word).
__device__ __forceinline__ uint32_t eligible_word(const JacRangeArgs& a, int64_t w, int64_t n_words) {
    uint32_t m = 0;
    if (w < n_words) m = ham_range_eligible(w, a.N, a.mask ? a.mask[w] : 0xFFFFFFFFu);
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
}

// The threshold of block query q as the kernels hold it: the caller's pair, or "nothing passes" for an
// absent query and for a pair outside the contract.
__device__ __forceinline__ void load_threshold(const JacRangeArgs& a, int b0, int q, int nq, int* num, int* den) {
    int n = kJacRangeNoneNum, d = kJacRangeNoneDen;
    if (q < nq) {
        const int tn = a.thr_num[b0 + q], td = a.thr_den[b0 + q];
        if (!jac_range_bad_threshold(tn, td)) n = tn, d = td;
    }
    num[q] = n;
    den[q] = d;
}

// ---- the popcount scan ----------------------------------------------------------------------------
// QB: the block (a power of two); PW: words of a row a lane holds at once; LONG: more than one pass.
template <int QB, int PW, bool LONG>
__global__ void __launch_bounds__(256) jaccard_range_pop_kernel(JacRangeArgs a, int b0, int nq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint32_t s_cnt[kHamRangeWaves][QB];
    const int W = a.W;
    const int WS = ham_query_stride(W);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int64_t n_words = range_n_words(a.N);
    const int64_t n_chunks = range_n_chunks(n_words);
    const int64_t n_tiles = ham_n_tiles(a.N);
    uint64_t* qs = reinterpret_cast<uint64_t*>(smem);
    int* qpl = reinterpret_cast<int*>(smem + jac_range_pop_qpop_off(QB, W));
    int* num = reinterpret_cast<int*>(smem + jac_range_pop_num_off(QB, W));
    int* den = reinterpret_cast<int*>(smem + jac_range_pop_den_off(QB, W));

    // the block's queries as words, zero where there is no query or no byte
    for (int i = threadIdx.x; i < QB * WS; i += 256) {
        const int q = i / WS, w = i - q * WS;
        qs[i] = (q < nq && w < W) ? ham_word_of(a.queries + (size_t)(b0 + q) * a.n_bytes, a.n_bytes, w) : 0ull;
    }
    if (threadIdx.x < QB) load_threshold(a, b0, threadIdx.x, nq, num, den);
    __syncthreads();
    if (threadIdx.x < QB) {  // |q|, once per query
        int p = 0;
        for (int w = 0; w < W; ++w) p += __popcll(qs[threadIdx.x * WS + w]);
        qpl[threadIdx.x] = p;
    }
    __syncthreads();

    uint32_t total = 0;  // lane q: the wave's hits of query q
    for (int i = 0; i < kHamRangeWaveTiles; ++i) {
        const int64_t t = ham_range_tile(chunk, wv, i);
        if (t >= n_tiles) break;  // (wave-uniform) past the last tile: no word below n_words either
        const int64_t w0 = ham_range_word(t, 0), w1 = ham_range_word(t, 1);
        const uint32_t e0 = eligible_word(a, w0, n_words), e1 = eligible_word(a, w1, n_words);
        const bool in = (((lane < 32 ? e0 : e1) >> (lane & 31)) & 1u) != 0u;
        uint32_t h0 = 0, h1 = 0;  // lane q: query q's two words of this tile
        if ((e0 | e1) != 0u) {    // (a tile the mask rules out whole is not read)
            const uint64_t* xt = a.codes + (size_t)t * W * kHamTileRows + lane;
            if constexpr (!LONG) {
                // the whole code in registers: |x| once, then query after query, nothing kept per query
                // (the loop is not unrolled: unrolled, the compiler hoists every query's LDS reads)
                uint64_t x[PW];
                int xp = 0;
#pragma unroll
                for (int j = 0; j < PW; ++j) {
                    x[j] = j < W ? xt[(size_t)j * kHamTileRows] : 0ull;
                    xp += __popcll(x[j]);
                }
#pragma nounroll
                for (int q = 0; q < nq; ++q) {
                    const uint64_t* qq = qs + q * WS;  // wave-uniform: an LDS broadcast
                    int n = 0;
#pragma unroll
                    for (int j = 0; j < PW; ++j) n += __popcll(x[j] & qq[j]);
                    const uint64_t hit = __ballot(in && jac_range_pass(n, qpl[q] + xp - n, num[q], den[q]));
                    if (lane == q) {
                        h0 = (uint32_t)hit;
                        h1 = (uint32_t)(hit >> 32);
                    }
                }
            } else {
                int acc[QB];  // one running i per query across the passes
                int xp = 0;   // the running |x|
#pragma unroll
                for (int q = 0; q < QB; ++q) acc[q] = 0;
#pragma nounroll
                for (int p0 = 0; p0 < W; p0 += PW) {
                    uint64_t x[PW];
#pragma unroll
                    for (int j = 0; j < PW; ++j) {
                        x[j] = p0 + j < W ? xt[(size_t)(p0 + j) * kHamTileRows] : 0ull;
                        xp += __popcll(x[j]);
                    }
#pragma unroll
                    for (int q = 0; q < QB; ++q) {
                        const uint64_t* qq = qs + q * WS + p0;  // wave-uniform: an LDS broadcast
                        int n = acc[q];
#pragma unroll
                        for (int j = 0; j < PW; ++j) n += __popcll(x[j] & qq[j]);
                        acc[q] = n;
                    }
                }
                // (a slot at or past nq holds a zero query and the pair nothing passes: its ballot is zero)
#pragma unroll
                for (int q = 0; q < QB; ++q) {
                    const uint64_t hit = __ballot(in && jac_range_pass(acc[q], qpl[q] + xp - acc[q], num[q], den[q]));
                    if (lane == q) {
                        h0 = (uint32_t)hit;
                        h1 = (uint32_t)(hit >> 32);
                    }
                }
            }
        }
        if (lane < nq) {
            a.H[(size_t)lane * (size_t)n_words + (size_t)w0] = h0;
            if (w1 < n_words) a.H[(size_t)lane * (size_t)n_words + (size_t)w1] = h1;  // (else e1 == 0: h1 is zero)
        }
        total += (uint32_t)(__popc(h0) + __popc(h1));
    }
    if (lane < QB) s_cnt[wv][lane] = total;
    __syncthreads();
    if (wv == 0 && lane < nq) {
        uint32_t c = 0;
#pragma unroll
        for (int x = 0; x < kHamRangeWaves; ++x) c += s_cnt[x][lane];
        a.part[(size_t)lane * (size_t)n_chunks + (size_t)chunk] = c;
    }
}

// ---- the MFMA scan --------------------------------------------------------------------------------
// 16 bits of a word from bit `sh` up as one MFMA operand: bit i to byte i, 0 / 1 (rows and queries).
__device__ __forceinline__ jr_i32x4 expand16(uint64_t x, int sh) {
    jr_i32x4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d) r[d] = (int)ham_mfma_row4((uint32_t)(x >> (sh + 4 * d)));
    return r;
}

__global__ void __launch_bounds__(256) jaccard_range_mfma_kernel(JacRangeArgs a, int b0, int nq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int W = a.W, Wp = ham_mfma_words(W);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    const int64_t chunk = blockIdx.x;
    const int64_t n_words = range_n_words(a.N);
    const int64_t n_chunks = range_n_chunks(n_words);
    const int64_t n_tiles = ham_n_tiles(a.N);
    uint64_t* qs = reinterpret_cast<uint64_t*>(smem);
    uint32_t* stage = reinterpret_cast<uint32_t*>(smem + jac_range_mfma_stage_off(W));
    int* qpl = reinterpret_cast<int*>(smem + jac_range_mfma_qpop_off(W));
    int* num = reinterpret_cast<int*>(smem + jac_range_mfma_num_off(W));
    int* den = reinterpret_cast<int*>(smem + jac_range_mfma_den_off(W));
    int* s_xpop = reinterpret_cast<int*>(smem + jac_range_mfma_xpop_off(W)) + wv * kHamTileRows;  // this wave's

    // the block's queries as words [Wp][64], zero where there is no query or no byte
    for (int i = threadIdx.x; i < MQB * Wp; i += 256) {
        const int q = i / Wp, w = i - q * Wp;
        qs[(size_t)w * MQB + q] = (q < nq && w < W) ? ham_word_of(a.queries + (size_t)(b0 + q) * a.n_bytes, a.n_bytes, w) : 0ull;
    }
    if (threadIdx.x < MQB) load_threshold(a, b0, threadIdx.x, nq, num, den);
    __syncthreads();
    if (threadIdx.x < MQB) {  // |q|, once per query
        int p = 0;
        for (int w = 0; w < Wp; ++w) p += __popcll(qs[(size_t)w * MQB + threadIdx.x]);
        qpl[threadIdx.x] = p;
    }
    __syncthreads();
    int qpop[QT], qnum[QT], qden[QT];  // of the lane's query in each tile
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        qpop[qt] = qpl[32 * qt + col];
        qnum[qt] = num[32 * qt + col];
        qden[qt] = den[32 * qt + col];
    }

    const int n_pairs = Wp / 2;
    for (int i = 0; i < kHamRangeWaveTiles; ++i) {
        const int64_t t = ham_range_tile(chunk, wv, i);
        // the eligible rows of the two sub-tiles (zero for a tile at or past n_tiles: its words are at
        // or past n_words)
        uint32_t el[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) el[rt] = t < n_tiles ? eligible_word(a, ham_range_word(t, rt), n_words) : 0u;
        const bool read = (el[0] | el[1]) != 0u;  // (a tile past the end or one the mask rules out whole is not read)
        jr_i32x16 acc[RT][QT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[rt][qt][v] = 0;
        if (read) {
            const uint64_t* xt = a.codes + (size_t)t * W * kHamTileRows + col;
            uint64_t xn[RT];
            int xp[RT];  // bits of the lane's words of row col of each sub-tile
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                xn[rt] = (el[rt] != 0u && half < W) ? xt[(size_t)half * kHamTileRows + 32 * rt] : 0ull;
                xp[rt] = 0;
            }
            for (int j = 0; j < n_pairs; ++j) {
                uint64_t x[RT], qw[QT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) x[rt] = xn[rt];
                const int wn = ham_mfma_word(4 * (j + 1), half);  // the next pair's word of this lane half
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
                    xn[rt] = (j + 1 < n_pairs && el[rt] != 0u && wn < W) ? xt[(size_t)wn * kHamTileRows + 32 * rt] : 0ull;
                const int w = ham_mfma_word(4 * j, half);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) qw[qt] = qs[(size_t)w * MQB + 32 * qt + col];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) xp[rt] += __popcll(x[rt]);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int sh = ham_mfma_shift(m);
                    jr_i32x4 xa[RT], qa[QT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) xa[rt] = expand16(x[rt], sh);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) qa[qt] = expand16(qw[qt], sh);
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
        }
        // per sub-tile: |x| of the lane's 16 accumulator rows, then per query tile 16 tests to 16 bits at
        // their row positions, one exchange, one AND: the word of (query, sub-tile).  Lane half rt stages
        // sub-tile rt's words, so each word is stored once.  A tile that was not read stages zeros.
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            int xr[16];
#pragma unroll
            for (int v = 0; v < 16; ++v) xr[v] = read ? s_xpop[32 * rt + ham_range_acc_row(v, half)] : 0;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                uint32_t bits = 0;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int n = acc[rt][qt][v];
                    if (jac_range_pass(n, qpop[qt] + xr[v] - n, qnum[qt], qden[qt])) bits |= 1u << ham_range_acc_row(v, half);
                }
                bits |= (uint32_t)__shfl_xor((int)bits, 32, 64);
                bits &= el[rt];
                if (half == rt) stage[(32 * qt + col) * kHamRangeStageStride + ham_range_chunk_word(wv, i, rt)] = bits;
            }
        }
        // the next tile's park does not overtake these reads
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // thread e: word e % 16 of query e / 16 -- 64-byte runs of H per query, and the chunk's count as
    // the sum over the 16 lanes of a run
    for (int e = threadIdx.x; e < MQB * kRangeWgWords; e += 256) {
        const int q = e / kRangeWgWords, cw = e % kRangeWgWords;
        const uint32_t word = stage[q * kHamRangeStageStride + cw];
        const int64_t w = chunk * kRangeWgWords + cw;
        if (q < nq && w < n_words) a.H[(size_t)q * (size_t)n_words + (size_t)w] = word;
        int c = __popc(word);
#pragma unroll
        for (int off = kRangeWgWords / 2; off > 0; off >>= 1) c += __shfl_xor(c, off, kRangeWgWords);
        if (cw == 0 && q < nq) a.part[(size_t)q * (size_t)n_chunks + (size_t)chunk] = (uint32_t)c;
    }
}

// ---- i and u of the emitted slots -----------------------------------------------------------------
// grid (ham_range_fill_wgs, qb): slots [0, n) of query blockIdx.y (n = min(count, cap)) by groups of 16
// lanes, the row id read back from the slot; slots [n, cap) one thread each.
__global__ void __launch_bounds__(256) jaccard_range_fill_kernel(JacRangeArgs a, int b0) {
    const int q = blockIdx.y;
    const int b = b0 + q;
    const int W = a.W;
    const int64_t n = range_filled(a.cnt[q], a.cap);
    int64_t* oi = a.out_i + (int64_t)b * a.cap;
    int32_t* on = a.out_n + (int64_t)b * a.cap;
    int32_t* ou = a.out_u + (int64_t)b * a.cap;
    const uint8_t* qv = a.queries + (size_t)b * a.n_bytes;
    const int sub = threadIdx.x & (kHamRangeFillLanes - 1), grp = threadIdx.x / kHamRangeFillLanes;
    const int64_t step = (int64_t)gridDim.x * kHamRangeFillSlots;
    for (int64_t p0 = (int64_t)blockIdx.x * kHamRangeFillSlots; p0 < n; p0 += step) {  // (uniform: the shuffles below)
        const int64_t p = p0 + grp;
        const bool live = p < n;
        const int64_t r = live ? oi[p] - a.index_offset : 0;
        int ix = 0, qp = 0;  // i and |x| share a register, 16 bits each (both at most 8 192)
        if (live)
            for (int w = sub; w < W; w += kHamRangeFillLanes) {
                const uint64_t xw = a.codes[ham_word_index(r, w, W)];
                const uint64_t qw = ham_word_of(qv, a.n_bytes, w);
                ix += __popcll(xw & qw) | (__popcll(xw) << 16);
                qp += __popcll(qw);
            }
#pragma unroll
        for (int off = kHamRangeFillLanes / 2; off > 0; off >>= 1) {
            ix += __shfl_xor(ix, off, kHamRangeFillLanes);
            qp += __shfl_xor(qp, off, kHamRangeFillLanes);
        }
        if (live && sub == 0) {
            const int i = ix & 0xFFFF;
            on[p] = i;
            ou[p] = qp + (ix >> 16) - i;
        }
    }
    const int64_t n_thr = (int64_t)gridDim.x * 256;
    for (int64_t p = n + (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.cap; p += n_thr) {
        oi[p] = -1;
        on[p] = -1;
        ou[p] = -1;
    }
}

// An empty index: counts 0 and every slot -1 / -1 / -1.
__global__ void __launch_bounds__(256) jaccard_range_empty_kernel(int64_t* out_c, int n_queries, int64_t* out_i,
                                                                  int32_t* out_n, int32_t* out_u, int64_t slots) {
    const int64_t n_thr = (int64_t)gridDim.x * 256;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_queries; p += n_thr) out_c[p] = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < slots; p += n_thr) {
        out_i[p] = -1;
        out_n[p] = -1;
        out_u[p] = -1;
    }
}

template <int QB>
hipError_t launch_pop(const JacRangeArgs& a, int b0, int nq, unsigned grid, hipStream_t st) {
    const size_t lds = (size_t)jac_range_pop_lds(QB, a.W);
    if (ham_range_long(a.W))
        hipLaunchKernelGGL((jaccard_range_pop_kernel<QB, kHamPassWords, true>), dim3(grid), dim3(256), lds, st, a, b0, nq);
    else if (a.W <= 4)
        hipLaunchKernelGGL((jaccard_range_pop_kernel<QB, 4, false>), dim3(grid), dim3(256), lds, st, a, b0, nq);
    else
        hipLaunchKernelGGL((jaccard_range_pop_kernel<QB, kHamPassWords, false>), dim3(grid), dim3(256), lds, st, a, b0, nq);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_jaccard_range_empty(int64_t* out_c, int n_queries, int64_t* out_i, int32_t* out_n, int32_t* out_u,
                                      int64_t cap, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (!out_c || cap < 0 || (cap > 0 && (!out_i || !out_n || !out_u))) return hipErrorInvalidValue;
    const int64_t slots = (int64_t)n_queries * cap;
    const int64_t most = slots > n_queries ? slots : n_queries;
    const int64_t g = (most + 255) / 256;
    hipLaunchKernelGGL(jaccard_range_empty_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, st, out_c, n_queries,
                       out_i, out_n, out_u, slots);
    return hipGetLastError();
}

hipError_t launch_jaccard_range_block(const JacRangeArgs& a, bool mfma, int block, int b0, int qb, hipStream_t st) {
    if (qb <= 0) return hipSuccess;
    const int W = ham_words(a.n_bytes);
    if (qb > block || b0 < 0 || a.N <= 0 || a.N > 0xFFFFFFFEll || a.n_bytes < 1 || a.n_bytes > kHamMaxBytes || a.W != W ||
        a.cap < 0 || !a.codes || !a.queries || !a.thr_num || !a.thr_den || !a.H || !a.part || !a.cnt || !a.out_c ||
        (a.cap > 0 && (!a.out_i || !a.out_n || !a.out_u)))
        return hipErrorInvalidValue;
    const int64_t n_words = range_n_words(a.N);
    const int64_t n_chunks = range_n_chunks(n_words);
    // (one workgroup per chunk: 2^32 rows are 2^23 chunks)
    const unsigned grid = (unsigned)n_chunks;
    hipError_t e = hipErrorInvalidValue;
    if (mfma) {
        if (block != kJacRangeMfmaQB) return hipErrorInvalidValue;
        const size_t lds = (size_t)jac_range_mfma_lds(W);
        if (kHamWgPerCuLds * lds > (size_t)kHamLdsLimit) return hipErrorInvalidValue;
        if (lds > 65536) {  // (set per launch, for the device that is current)
            e = hipFuncSetAttribute((const void*)jaccard_range_mfma_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(jaccard_range_mfma_kernel, dim3(grid), dim3(256), lds, st, a, b0, qb);
        e = hipGetLastError();
    } else {
        switch (block) {
            case 1: e = launch_pop<1>(a, b0, qb, grid, st); break;
            case 2: e = launch_pop<2>(a, b0, qb, grid, st); break;
            case 4: e = launch_pop<4>(a, b0, qb, grid, st); break;
            case 8: e = launch_pop<8>(a, b0, qb, grid, st); break;
            case 16: e = launch_pop<16>(a, b0, qb, grid, st); break;
            default: return hipErrorInvalidValue;
        }
    }
    if (e != hipSuccess) return e;
    // counts and ascending ids: the dense range search's prefix and emit over the same H and part
    RangeArgs ra{};
    ra.N = a.N;
    ra.H = a.H;
    ra.part = a.part;
    ra.cnt = a.cnt;
    ra.cap = a.cap;
    ra.out_c = a.out_c;
    ra.out_i = a.out_i;
    ra.index_offset = a.index_offset;
    e = launch_range_prefix_emit(ra, b0, qb, st);
    if (e != hipSuccess || a.cap == 0) return e;
    hipLaunchKernelGGL(jaccard_range_fill_kernel, dim3(ham_range_fill_wgs(a.cap), qb), dim3(256), 0, st, a, b0);
    return hipGetLastError();
}

}  // namespace vdb
