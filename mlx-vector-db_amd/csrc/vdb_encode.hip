// vdb_encode.hip: binary codes from fp32 vectors on the device (vdb_index_encode_codes,
// vdb_index_encode).  Bit j of a vector x is 1 iff s_j > t_j, s_j the canonical fp64 dot product
// (vdb_common.h) of projection row j and x: a GEMM with a 1-bit epilogue.  The bytes are defined by
// the fp64 sums; an fp32-MFMA kernel decides every pair a rigorous margin allows
// (vdb_encode_plan.h encode_decide) and a second kernel pays fp64 for the rest, so the bytes do not
// depend on which of them decided a bit.  Built with -ffp-contract=off and without the packed fp32
// instructions.
//
//   prep    one wave per row: a row-major [n][D] source is copied into [n_pad][Dp] rows, zero padded
//           (Dp a multiple of 64: no K chunk of either operand is ragged), with each row's canonical
//           fp64 norm.  Serves the projection and, for vdb_index_encode, the vectors.
//   gemm    grid = (chunk of 128 vectors) x (block of 128 bits), the bit block fastest so that the
//           workgroups sharing a chunk of vectors run side by side and share it in L2.  4 waves as
//           2 x 2, each 64 vectors x 64 bits: 2 x 2 accumulators of v_mfma_f32_32x32x2_f32, vectors on
//           M, bits on N.  K in chunks of 32 dims: each thread brings four 16-byte pieces of either
//           operand (8 threads per row: 128 contiguous bytes) into registers one chunk ahead and from
//           there into LDS rows padded to 36 floats; lane (c, h) of step s reads floats [8 s + 4 h, +4)
//           of vector c and of bit c, one 16-byte LDS read per tile, and feeds four MFMAs per
//           accumulator from them.
//           Epilogue: lane (c, h) holds bit c of vectors 8 b + 4 h + r.  Per accumulator register one
//           decision in fp64 and two ballots (certain ones, undecided): lanes 0-31 of a ballot are 32
//           bits of one vector's code, lanes 32-63 of another's.  The words meet in LDS and leave as
//           one 16-byte store per vector and buffer: no atomics, no score matrix in memory.
//   drain   walks the word buffers, a wave 64 words at a time.  For each undecided bit all 64 lanes
//           compute the canonical sum and the owner sets the bit; then every lane writes its word's
//           bytes to the row-major code bytes.  A wave owns whole words, so no atomics; nothing can
//           overflow, a call in which every pair is undecided is merely slow.  With `all` the word
//           buffers are not read and every bit is decided here (knob encode_mfma = 2).
//   sign    the identity projection: one wave per vector reads 64 dims per load, coalesced; one ballot
//           of (double)x > t is one 64-bit code word.  Exact as it stands, no margin.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_encode_plan.h"

namespace vdb {

namespace {

// ---- prep ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) encode_prep_kernel(const float* __restrict__ src, int64_t n, int64_t n_pad, int D,
                                                          int Dp, float* __restrict__ dst, double* __restrict__ nrm) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_pad) return;
    const int np = (Dp + 255) / 256;
    double acc = 0.0;
    for (int m = 0; m < np; ++m) {
        const int p = m * 64 + lane;
        if (4 * p < Dp) {
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = 4 * p + j;
                v[j] = (r < n && d < D) ? src[r * (int64_t)D + d] : 0.0f;
                acc = acc + (double)v[j] * (double)v[j];
            }
            *(f32x4*)(dst + r * (int64_t)Dp + 4 * p) = v;
        }
    }
    acc = wave_sum_butterfly(acc);
    if (lane == 0) nrm[r] = sqrt(acc);
}

// ---- the GEMM -----------------------------------------------------------------------------------
__global__ void __launch_bounds__(256, 2) encode_gemm_kernel(EncodeArgs a, int n_bb) {
    constexpr int ST = kEncLdsStride, KC = kEncKC;
    __shared__ __attribute__((aligned(16))) float s_x[kEncBM * ST];
    __shared__ __attribute__((aligned(16))) float s_p[kEncBN * ST];
    __shared__ double s_xn[kEncBM];
    __shared__ __attribute__((aligned(16))) uint32_t s_w[2][kEncBM][kEncBlockWords];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int c = lane & 31, h = lane >> 5;
    const int bb = (int)(blockIdx.x % (unsigned)n_bb);
    const int64_t r0 = (int64_t)(blockIdx.x / (unsigned)n_bb) * kEncBM;
    const int j0 = bb * kEncBN;
    const int Dp = a.Dp;
    const int nkc = enc_k_chunks(Dp);
    if (tid < kEncBM) s_xn[tid] = r0 + tid < a.n ? a.xn[r0 + tid] : 0.0;

    f32x16 acc[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[tm][tn][v] = 0.0f;

    f32x4 xr[kEncLoads], pr[kEncLoads];
    auto load_chunk = [&](int kc) {
        const int col = kc * KC + enc_load_col(tid);
#pragma unroll
        for (int i = 0; i < kEncLoads; ++i) {
            const int row = enc_load_row(i, tid);
            const int64_t r = r0 + row;
            const int j = j0 + row;
            const bool cin = col < Dp;  // (Dp is a multiple of 64: always)
            xr[i] = (cin && r < a.n) ? *(const f32x4*)(a.V + (size_t)r * (size_t)a.ldv + (size_t)col) : f32x4{0.f, 0.f, 0.f, 0.f};
            pr[i] = (cin && j < a.n_bits) ? *(const f32x4*)(a.P + (size_t)j * (size_t)Dp + (size_t)col) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    load_chunk(0);
    for (int kc = 0; kc < nkc; ++kc) {
        __syncthreads();  // the previous chunk's operand reads are done
#pragma unroll
        for (int i = 0; i < kEncLoads; ++i) {
            const int at = enc_load_row(i, tid) * ST + enc_load_col(tid);
            *(f32x4*)&s_x[at] = xr[i];
            *(f32x4*)&s_p[at] = pr[i];
        }
        __syncthreads();
        if (kc + 1 < nkc) load_chunk(kc + 1);
#pragma unroll
        for (int s = 0; s < kEncSteps; ++s) {
            const int col = enc_operand_col(s, h);
            f32x4 av[2], bv[2];
#pragma unroll
            for (int tm = 0; tm < 2; ++tm) av[tm] = *(const f32x4*)&s_x[(wm * kEncWaveM + tm * 32 + c) * ST + col];
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) bv[tn] = *(const f32x4*)&s_p[(wn * kEncWaveN + tn * 32 + c) * ST + col];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn)
                        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[tm][e], bv[tn][e], acc[tm][tn], 0, 0, 0);
        }
    }

    // epilogue: accumulators to code words
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int j = j0 + wn * kEncWaveN + tn * 32 + c;
        const bool live = j < a.n_bits;
        const double t = (live && a.thr) ? a.thr[j] : 0.0;
        const double pn = live ? a.pn[j] : 0.0;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
            const int rl = wm * kEncWaveM + tm * 32;
            uint32_t one = 0, und = 0;  // lane i < 32: the words of vector rl + i
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const double xn = s_xn[rl + enc_acc_row(v, h)];
                const int d = live ? encode_decide(acc[tm][tn][v], t, pn, xn, a.D) : (int)kEncZero;
                const unsigned long long b1 = __ballot(d == kEncOne);
                const unsigned long long bu = __ballot(d == kEncUndecided);
                const int i0 = enc_acc_row(v, 0), i1 = enc_acc_row(v, 1);
                if (lane == i0) {
                    one = (uint32_t)b1;
                    und = (uint32_t)bu;
                }
                if (lane == i1) {
                    one = (uint32_t)(b1 >> 32);
                    und = (uint32_t)(bu >> 32);
                }
            }
            if (lane < 32) {
                s_w[0][rl + lane][wn * 2 + tn] = one;
                s_w[1][rl + lane][wn * 2 + tn] = und;
            }
        }
    }
    __syncthreads();
    {
        const int which = tid >> 7, row = tid & (kEncBM - 1);
        const int64_t r = r0 + row;
        if (r < a.n) {
            uint32_t* dst = (which ? a.uw : a.cw) + (size_t)r * (size_t)a.stride + (size_t)bb * kEncBlockWords;
            *(uint4*)dst = *(const uint4*)&s_w[which][row][0];
        }
    }
}

// ---- the undecided pairs --------------------------------------------------------------------------
// The canonical fp64 dot product of two Dp-padded rows on the whole wave (exact_key<0>'s sum: pieces
// 64 m + lane in (m, j) order, separate multiply and add, then the butterfly); up to four pieces of
// either row in flight per lane.
__device__ __noinline__ double encode_canonical_dot(const float* __restrict__ p, const float* __restrict__ x, int D, int Dp) {
    const int lane = threadIdx.x & 63;
    const int np = (D + 255) / 256;
    double acc = 0.0;
    for (int m0 = 0; m0 < np; m0 += 4) {
        f32x4 pv[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int pc = (m0 + u) * 64 + lane;
            const bool in = (m0 + u) < np && 4 * pc < Dp;
            pv[u] = in ? *(const f32x4*)(p + 4 * pc) : f32x4{0.f, 0.f, 0.f, 0.f};
            xv[u] = in ? *(const f32x4*)(x + 4 * pc) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((m0 + u) < np) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = acc + (double)pv[u][j] * (double)xv[u][j];
            }
        }
    }
    return wave_sum_butterfly(acc);
}

__global__ void __launch_bounds__(256) encode_drain_kernel(EncodeArgs a, int all) {
    const int lane = threadIdx.x & 63;
    const int W = enc_words(a.n_bits);
    const int64_t total = a.n * W;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    unsigned long long n_exact = 0;  // (wave-uniform; a wave may own more than 2^32 pairs)
    for (int64_t base = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64; base < total; base += n_waves * 64) {
        const int64_t o = base + lane;
        const bool mine = o < total;
        const int64_t r = mine ? o / W : 0;
        const int w = mine ? (int)(o % W) : 0;
        uint32_t code = 0, und = 0;
        if (mine) {
            const uint32_t valid = enc_valid_bits(w, a.n_bits);
            if (all) {
                und = valid;
            } else {
                code = a.cw[(size_t)r * (size_t)a.stride + (size_t)w] & valid;
                und = a.uw[(size_t)r * (size_t)a.stride + (size_t)w] & valid;
            }
        }
        for (;;) {  // one pair at a time on the whole wave (wave-uniform loop)
            const unsigned long long bal = __ballot(und != 0u);
            if (bal == 0ull) break;
            const int src = __ffsll((long long)bal) - 1;
            const uint32_t su = (uint32_t)__shfl((int)und, src, 64);
            const int i = __ffs((int)su) - 1;
            const int64_t os = base + src;
            const int64_t rs = os / W;
            const int j = (int)(os % W) * 32 + i;
            const double s = encode_canonical_dot(a.P + (size_t)j * (size_t)a.Dp, a.V + (size_t)rs * (size_t)a.ldv, a.D, a.Dp);
            const double t = a.thr ? a.thr[j] : 0.0;
            if (lane == src) {
                und &= ~(1u << i);
                if (s > t) code |= 1u << i;
            }
            ++n_exact;
        }
        if (mine) {
            const int nb = enc_word_bytes(w, a.n_bytes);
            uint8_t* dst = a.out + (size_t)r * (size_t)a.n_bytes + (size_t)4 * w;
            if (nb == 4 && ((uintptr_t)dst & 3u) == 0) {
                *(uint32_t*)dst = code;
            } else {
                for (int b = 0; b < nb; ++b) dst[b] = (uint8_t)(code >> (8 * b));
            }
        }
    }
    if (lane == 0 && n_exact) atomicAdd(a.exact_pairs, n_exact);
}

// ---- the identity projection ----------------------------------------------------------------------
__global__ void __launch_bounds__(256) encode_sign_kernel(EncodeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.n) return;
    const int W64 = (a.D + 63) / 64;
    const float* x = a.V + (size_t)r * (size_t)a.ldv;
    uint8_t* out = a.out + (size_t)r * (size_t)a.n_bytes;
    for (int w0 = 0; w0 < W64; w0 += 4) {
        float xv[4];
        double tv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = (w0 + u) * 64 + lane;
            const bool in = d < a.D;
            xv[u] = in ? x[d] : 0.0f;
            tv[u] = (in && a.thr) ? a.thr[d] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (w0 + u < W64) {
                const int d = (w0 + u) * 64 + lane;
                const unsigned long long bal = __ballot(d < a.D && (double)xv[u] > tv[u]);
                const int byte = 8 * (w0 + u) + lane;
                if (lane < 8 && byte < a.n_bytes) out[byte] = (uint8_t)(bal >> (8 * lane));
            }
        }
    }
}

bool encode_args_ok(const EncodeArgs& a, bool gemm) {
    if (a.n < 0 || a.D < 1 || a.n_bits < 1 || a.n_bits > kEncMaxBits || a.n_bytes != enc_bytes(a.n_bits) || !a.V) return false;
    if (!gemm) return true;
    return a.P && a.pn && a.xn && a.Dp >= a.D && a.Dp % 64 == 0 && a.ldv == a.Dp && a.stride == enc_word_stride(a.n_bits);
}

}  // namespace

hipError_t launch_encode_prep(const float* src, int64_t n, int64_t n_pad, int D, int Dp, float* dst, double* nrm,
                              hipStream_t st) {
    if (n_pad <= 0) return hipSuccess;
    if (!src || !dst || !nrm || n < 0 || n > n_pad || D < 1 || Dp < D || Dp % 64 != 0) return hipErrorInvalidValue;
    const int64_t blocks = (n_pad + 3) / 4;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(encode_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, st, src, n, n_pad, D, Dp, dst, nrm);
    return hipGetLastError();
}

hipError_t launch_encode_gemm(const EncodeArgs& a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    if (!encode_args_ok(a, true) || !a.cw || !a.uw) return hipErrorInvalidValue;
    static_assert(sizeof(float) * (kEncBM + kEncBN) * kEncLdsStride + sizeof(double) * kEncBM +
                          sizeof(uint32_t) * 2 * kEncBM * kEncBlockWords <= kEncLdsLimit,
                  "the workgroup's static LDS");
    const int n_bb = enc_bit_blocks(a.n_bits);
    const int64_t blocks = enc_row_blocks(a.n) * n_bb;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(encode_gemm_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, n_bb);
    return hipGetLastError();
}

hipError_t launch_encode_drain(const EncodeArgs& a, bool all, int n_cu, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    if (!encode_args_ok(a, false) || !a.P || !a.out || !a.exact_pairs || a.Dp % 64 != 0 || a.ldv != a.Dp ||
        (!all && (!a.cw || !a.uw)))
        return hipErrorInvalidValue;
    const int64_t total = a.n * enc_words(a.n_bits);
    int64_t blocks = (total + 255) / 256;  // a wave per 64 words, capped at what is resident: the rest by stride
    blocks = std::min<int64_t>(blocks, (int64_t)(n_cu > 0 ? n_cu : 256) * 8);
    hipLaunchKernelGGL(encode_drain_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, all ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_encode_sign(const EncodeArgs& a, hipStream_t st) {
    if (a.n <= 0) return hipSuccess;
    if (!encode_args_ok(a, false) || !a.out || a.n_bits != a.D || a.ldv < a.D) return hipErrorInvalidValue;
    const int64_t blocks = (a.n + 3) / 4;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(encode_sign_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace vdb
