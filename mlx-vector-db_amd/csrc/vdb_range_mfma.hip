// vdb_range_mfma.hip: the fp32-MFMA form of the range search's scan (vdb_range.hip has the fp64 form
// and the launches behind either: prefix, emit, score).  It writes the same hit bitmap H and the same
// per-chunk counts part, bit for bit: a pair is decided in fp32 only where a rigorous margin says the
// canonical fp64 key is on the same side of the bound (vdb_range_mfma_plan.h range_mfma_decide; the
// derivation is DESIGN.md §14.1), and every other pair gets its canonical key from exact_key.
// Built with -ffp-contract=off and without the packed fp32 instructions.
//
// A skinny GEMM with a threshold epilogue.  grid = chunks of 512 rows, 4 waves; wave w owns bitmap
// words [4 w, 4 w + 4) of the chunk and takes them two 32-row tiles at a time against the block's up
// to 64 queries: four 32x32 fp32 accumulators of v_mfma_f32_32x32x2_f32, rows on M, queries on N.
//
//   K loop   chunks of 32 dims.  A wave reads its 64 rows' 128-byte segments with 16-byte loads, 8
//            lanes per row (coalesced; rows at or past the count and tiles without an eligible row
//            are not read), the workgroup reads the queries' chunk element-wise (a query row has no
//            alignment: its stride is D), both into registers one chunk ahead and from there into
//            LDS rows padded to 36 floats.  Lane (c, h) of step s reads floats [8 s + 4 h, +4) of
//            row c and of query c, one 16-byte LDS read each per tile, and feeds four MFMAs per
//            accumulator from them: the K order this implies is the same for both operands.
//   epilogue lane (c, h) holds rows 8 b + 4 h + r of query c of the tile: 16 decisions, the undecided
//            ones collected in a bit mask.  The wave then drains the masks one pair at a time, all
//            64 lanes on one canonical key (exact_key, the score kernel's), so a batch in which
//            every pair is undecided is slow and needs no list that could overflow.  The two halves
//            of a bitmap word meet by one exchange with lane ^ 32; no ballots, no atomics on H.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_exact_keys.h"
#include "vdb_range_mfma_plan.h"

namespace vdb {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// The canonical key of one undecided pair on the whole wave; kept out of line so that the scan's
// unrolled epilogue holds one copy of it and not one per accumulator.
template <int METRIC>
__device__ __noinline__ double range_mfma_exact_key(const float* q, double qn, const float* X, int G, int D, uint64_t r,
                                                    const double* nrm64) {
    return exact_key<METRIC>(q, qn, X, G, D, r, METRIC == 0 ? nrm64[r] : 1.0);
}

template <int METRIC>
__global__ void __launch_bounds__(256, 2) range_mfma_scan_kernel(RangeArgs a, int b0, int qb,
                                                              unsigned long long* __restrict__ exact_pairs) {
    constexpr int PT = kRangeMfmaPassTiles, ST = kRangeMfmaLdsStride, KC = kRangeMfmaKC;
    __shared__ __attribute__((aligned(16))) float s_x[kRangeMfmaWaves][kRangeMfmaPassRows * ST];
    __shared__ __attribute__((aligned(16))) float s_q[kRangeMfmaQB * ST];
    __shared__ double s_xn[kRangeMfmaWaves][kRangeMfmaPassRows];
    __shared__ uint32_t s_cnt[kRangeMfmaWaves][kRangeMfmaQB];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const int64_t chunk = blockIdx.x;
    const int64_t n_words = range_n_words(a.N);
    const int64_t n_chunks = range_n_chunks(n_words);
    const int Dp = a.G * GROUP_DIMS;
    const int nkc = range_mfma_k_chunks(Dp);
    const int nnt = qb > 32 ? 2 : 1;  // 32-query N tiles in use
    const float* Q = a.Q + (int64_t)b0 * a.D;
    // lane (c, h): the bound and norm of queries c and 32 + c
    double kt[2], qn[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int j = nt * 32 + c;
        kt[nt] = j < qb ? range_kt(METRIC, a.thr[b0 + j]) : (double)NAN;
        qn[nt] = j < qb ? a.qn64[b0 + j] : 0.0;
    }
    uint32_t cnt[2] = {0u, 0u};
    uint32_t n_exact = 0;  // (wave-uniform)
    for (int pass = 0; pass < kRangeMfmaPasses; ++pass) {
        const int64_t w0 = range_mfma_pass_word(chunk, wv, pass);
        uint32_t elig[PT];
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            const int64_t w = w0 + t;
            elig[t] = w < n_words ? range_valid_bits(w, a.N) & (a.mask ? a.mask[w] : 0xFFFFFFFFu) : 0u;
        }
        // the pass runs its K loop (and its barriers) when any wave of the workgroup has a live tile
        bool pass_live = false;
        for (int x = 0; x < kRangeMfmaWaves; ++x)
            for (int t = 0; t < PT; ++t) {
                const int64_t w = range_mfma_pass_word(chunk, x, pass) + t;
                if (w < n_words) pass_live |= (range_valid_bits(w, a.N) & (a.mask ? a.mask[w] : 0xFFFFFFFFu)) != 0u;
            }
        {
            const int64_t r = w0 * 32 + lane;
            s_xn[wv][lane] = (elig[h] != 0u && r < a.N) ? a.nrm64[r] : 0.0;
        }
        f32x16 acc[PT][2];
#pragma unroll
        for (int t = 0; t < PT; ++t)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[t][nt][v] = 0.0f;
        if (pass_live) {
            f32x4 xr[kRangeMfmaXLoads];
            float qr[kRangeMfmaQLoads];
            auto load_chunk = [&](int kc) {
                const int col = kc * KC + range_mfma_xload_col(lane);
#pragma unroll
                for (int i = 0; i < kRangeMfmaXLoads; ++i) {
                    const int rl = range_mfma_xload_row(i, lane);
                    const int64_t r = w0 * 32 + rl;
                    const bool in = elig[i / (kRangeMfmaXLoads / PT)] != 0u && r < a.N && col < Dp;
                    xr[i] = in ? *(const f32x4*)(a.X + (size_t)r * (size_t)Dp + (size_t)col) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int i = 0; i < kRangeMfmaQLoads; ++i) {
                    const int idx = i * 256 + (int)threadIdx.x;
                    const int j = idx / KC, d = kc * KC + idx % KC;
                    qr[i] = (j < qb && d < a.D) ? Q[(int64_t)j * a.D + d] : 0.0f;
                }
            };
            load_chunk(0);
            for (int kc = 0; kc < nkc; ++kc) {
                __syncthreads();  // the previous chunk's operand reads are done
#pragma unroll
                for (int i = 0; i < kRangeMfmaXLoads; ++i)
                    *(f32x4*)&s_x[wv][range_mfma_xload_row(i, lane) * ST + range_mfma_xload_col(lane)] = xr[i];
#pragma unroll
                for (int i = 0; i < kRangeMfmaQLoads; ++i) {
                    const int idx = i * 256 + (int)threadIdx.x;
                    s_q[(idx / KC) * ST + idx % KC] = qr[i];
                }
                __syncthreads();
                if (kc + 1 < nkc) load_chunk(kc + 1);
#pragma unroll
                for (int s = 0; s < kRangeMfmaSteps; ++s) {
                    const int col = range_mfma_operand_col(s, h);
                    f32x4 av[PT], bv[2];
#pragma unroll
                    for (int t = 0; t < PT; ++t) av[t] = *(const f32x4*)&s_x[wv][(t * 32 + c) * ST + col];
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) bv[nt] = *(const f32x4*)&s_q[(nt * 32 + c) * ST + col];
                    // (a tile without an eligible row holds zeros: its products are not worth a branch)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int t = 0; t < PT; ++t)
                            acc[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][e], bv[0][e], acc[t][0], 0, 0, 0);
                    if (nnt == 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int t = 0; t < PT; ++t)
                                acc[t][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t][e], bv[1][e], acc[t][1], 0, 0, 0);
                    }
                }
            }
        }
        // epilogue
#pragma unroll
        for (int t = 0; t < PT; ++t) {
            const int64_t w = w0 + t;
            if (w >= n_words) break;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                if (nt >= nnt) break;
                const int j = nt * 32 + c;
                uint32_t hit = 0, und = 0;
                if (elig[t] != 0u && j < qb) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int i = range_mfma_acc_row(v, h);
                        if ((elig[t] >> i) & 1u) {
                            const int d = range_mfma_decide(METRIC, acc[t][nt][v], kt[nt], qn[nt], s_xn[wv][t * 32 + i], a.D);
                            hit |= (uint32_t)(d == kRangeMfmaHit) << i;
                            und |= (uint32_t)(d == kRangeMfmaExact) << i;
                        }
                    }
                }
                // the undecided pairs, one at a time on the whole wave (wave-uniform loop)
                for (;;) {
                    const unsigned long long bal = __ballot(und != 0u);
                    if (bal == 0ull) break;
                    const int src = __ffsll((long long)bal) - 1;
                    const uint32_t su = (uint32_t)__shfl((int)und, src, 64);
                    const int i = __ffs((int)su) - 1;
                    const int jj = nt * 32 + (src & 31);
                    const uint64_t r = (uint64_t)(w * 32 + i);
                    const double key = range_mfma_exact_key<METRIC>(Q + (int64_t)jj * a.D, a.qn64[b0 + jj], a.X, a.G, a.D, r,
                                                                    a.nrm64);
                    if (lane == src) {
                        und &= ~(1u << i);
                        if (key >= kt[nt]) hit |= 1u << i;
                    }
                    ++n_exact;
                }
                const uint32_t word = hit | (uint32_t)__shfl_xor((int)hit, 32, 64);
                if (h == 0 && j < qb) {
                    a.H[(size_t)j * (size_t)n_words + (size_t)w] = word;
                    cnt[nt] += (uint32_t)__popc(word);
                }
            }
        }
    }
    if (h == 0) {
        s_cnt[wv][c] = cnt[0];
        s_cnt[wv][32 + c] = cnt[1];
    }
    __syncthreads();
    if (wv == 0 && lane < qb) {
        uint32_t t = 0;
#pragma unroll
        for (int x = 0; x < kRangeMfmaWaves; ++x) t += s_cnt[x][lane];
        a.part[(size_t)lane * (size_t)n_chunks + (size_t)chunk] = t;
    }
    if (lane == 0 && n_exact) atomicAdd(exact_pairs, (unsigned long long)n_exact);
}

}  // namespace

hipError_t launch_range_mfma_block(int metric, const RangeArgs& a, int b0, int qb, unsigned long long* exact_pairs,
                                   hipStream_t st) {
    if (qb <= 0) return hipSuccess;
    if (qb > kRangeMfmaQB || b0 < 0 || a.N <= 0 || a.cap < 0 || (metric != 0 && metric != 1) || !a.H || !a.part ||
        !a.cnt || !a.out_c || (a.cap > 0 && (!a.out_i || !a.out_s)) || !exact_pairs || a.D < 1 ||
        a.D > kRangeMfmaMaxDim || a.D > a.G * GROUP_DIMS)
        return hipErrorInvalidValue;
    static_assert(sizeof(float) * (kRangeMfmaWaves * kRangeMfmaPassRows * kRangeMfmaLdsStride +
                                   kRangeMfmaQB * kRangeMfmaLdsStride) +
                          sizeof(double) * kRangeMfmaWaves * kRangeMfmaPassRows +
                          sizeof(uint32_t) * kRangeMfmaWaves * kRangeMfmaQB <= kRangeMfmaLdsLimit,
                  "the workgroup's static LDS");
    const int64_t n_chunks = range_n_chunks(range_n_words(a.N));
    if (metric == 0)
        hipLaunchKernelGGL((range_mfma_scan_kernel<0>), dim3((unsigned)n_chunks), dim3(256), 0, st, a, b0, qb, exact_pairs);
    else
        hipLaunchKernelGGL((range_mfma_scan_kernel<1>), dim3((unsigned)n_chunks), dim3(256), 0, st, a, b0, qb, exact_pairs);
    return launch_range_finish(metric, a, b0, qb, st);
}

}  // namespace vdb
