// vdb_encode_plan.h — the arithmetic vdb_index_encode_codes / vdb_index_encode (vdb_api.cpp) share
// with their kernels (vdb_encode.hip): the limits and the validation, the bit / byte / word addressing
// of a code, the GEMM's tiling and LDS layout, the decision of one (vector, bit) pair with its margin,
// and the per-call scratch.
// Plain C++ with no HIP in it, so a stand-alone CPU program can sweep it under a sanitizer
// (tools/encode_plan_check.cpp).
//
// The tile, derived.  The fp32 MFMA (v_mfma_f32_32x32x2_f32) does 32 x 32 x 2 multiply-adds in 16
// passes of 4 cycles: 256 flop per cycle and CU, 157 Tflop/s over 256 CUs at 2.4 GHz.  A workgroup of
// 4 waves owns 128 vectors x 128 bits, a wave 64 x 64 as 2 x 2 accumulators.  Per K step of 8 dims a
// wave reads four 16-byte operands from LDS and issues 16 MFMAs (1 024 cycles of the matrix pipe), so
// LDS is idle 15 cycles in 16.  From HBM a workgroup brings (128 + 128) x 32 floats per K chunk of 32
// dims, 32 KiB, for 128 x 128 x 32 x 2 = 1 Mflop: 32 flop per byte.  The machine's balance is 157
// Tflop/s over about 5 TB/s of achievable HBM, also 32 flop per byte, if every operand byte came from
// HBM; but the grid's x dimension is the bit block, so the n_bits / 128 workgroups that share a chunk
// of vectors run side by side and all but the first find it in L2, and the projection (3 MiB at 1 024
// x 768) never leaves it.  What HBM then supplies is each vector once: at 1M x 768 -> 1 024 bits 3 GB
// against 1.6 Tflop, 520 flop per byte, MFMA-bound by a factor of 16 (10.3 ms of matrix work, 0.6 ms
// of HBM).
// Without any cache reuse the vectors would be read 8 times: 24 GB, 5 ms, still under the matrix time.
// A 256-bit block would halve that again but takes 128 accumulator registers per lane and with the
// epilogue's fp64 decision no longer leaves two workgroups per CU, which the loads' latency wants.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define VDB_ENC_HD __host__ __device__
#else
#define VDB_ENC_HD
#endif

namespace vdb {

// ---- limits, validation ---------------------------------------------------------------------------
constexpr int kEncMaxBits = 8192;   // the widest code column (vdb_hamming_plan.h kHamMaxBytes * 8)
constexpr int64_t kEncMaxVectors = 0x7FFFFFFFll;  // vectors of one call (every grid stays inside 2^31 workgroups)
constexpr int kEncMaxDim = 65536;   // the margin's constant covers gamma_n up to here; past it every pair is undecided
enum EncodeCause { kEncOk = 0, kEncBadBits, kEncIdentityWidth, kEncBadMem, kEncNullPointer, kEncBadCount };
// mem: 0 host, 1 device (include/vdb.h VDB_MEM_*).  io_ok: vectors and out_codes are given (or none is needed).
VDB_ENC_HD inline int encode_validate(int64_t n, int dim, int n_bits, bool has_proj, int mem, bool io_ok) {
    if (mem != 0 && mem != 1) return kEncBadMem;
    if (n_bits < 1 || n_bits > kEncMaxBits) return kEncBadBits;
    if (!has_proj && n_bits != dim) return kEncIdentityWidth;
    if (n < 0 || n > kEncMaxVectors) return kEncBadCount;
    if (n > 0 && !io_ok) return kEncNullPointer;
    return kEncOk;
}
// knob "encode_mfma": 0 = the MFMA kernel and the undecided pass, 2 = every pair in fp64.
VDB_ENC_HD inline bool encode_knob_ok(int64_t knob) { return knob == 0 || knob == 2; }

// ---- a code's addressing --------------------------------------------------------------------------
// Bit j of a code is bit j % 8 of byte j / 8 (least significant first); the kernels build 32-bit words,
// bit j = bit j % 32 of word j / 32, whose byte b (little endian) is code byte 4 (j / 32) + b.
VDB_ENC_HD inline int enc_bytes(int n_bits) { return (n_bits + 7) / 8; }
VDB_ENC_HD inline int enc_words(int n_bits) { return (n_bits + 31) / 32; }
// The row stride of the word buffers: whole 16-byte groups, so a workgroup's four words of a row are one aligned store.
VDB_ENC_HD inline int enc_word_stride(int n_bits) { return (enc_words(n_bits) + 3) / 4 * 4; }
// The bits of word w that are bits of the code (the pad bits of the last word are 0 in every output).
VDB_ENC_HD inline uint32_t enc_valid_bits(int w, int n_bits) {
    const int left = n_bits - w * 32;
    return left >= 32 ? 0xFFFFFFFFu : left <= 0 ? 0u : ((1u << left) - 1u);
}
// How many bytes of word w belong to a code of n_bytes bytes.
VDB_ENC_HD inline int enc_word_bytes(int w, int n_bytes) {
    const int left = n_bytes - 4 * w;
    return left >= 4 ? 4 : left <= 0 ? 0 : left;
}

// ---- the GEMM's tiling ----------------------------------------------------------------------------
// A workgroup: 4 waves as 2 x 2, kEncBM vectors x kEncBN bits; wave (wm, wn) owns vectors [64 wm, +64)
// and bits [64 wn, +64) of it as 2 x 2 accumulators of 32 x 32, vectors on M and bits on N.  K runs in
// chunks of kEncKC dims through LDS rows padded to kEncLdsStride floats (16-byte operand reads of 16
// lanes hit 64 distinct banks), both operands in registers one chunk ahead.
constexpr int kEncWaves = 4;
constexpr int kEncBM = 128, kEncBN = 128;
constexpr int kEncWaveM = 64, kEncWaveN = 64;
constexpr int kEncKC = 32;
constexpr int kEncLdsStride = kEncKC + 4;
constexpr int kEncSteps = kEncKC / 8;
constexpr int kEncLoads = kEncBM * kEncKC / (256 * 4);  // 16-byte loads per thread, operand and chunk: 4
static_assert(kEncBM == kEncBN, "one load map serves both operands");
static_assert(kEncLdsStride % 4 == 0, "16-byte operand reads stay aligned");
// load i of thread t: row i * 32 + t / 8 of the block, floats [4 (t % 8), +4) of the chunk
VDB_ENC_HD inline int enc_load_row(int i, int t) { return i * 32 + t / 8; }
VDB_ENC_HD inline int enc_load_col(int t) { return (t % 8) * 4; }
// lane half h of step s supplies floats [8 s + 4 h, +4) of its row to four MFMAs (both operands alike)
VDB_ENC_HD inline int enc_operand_col(int step, int half) { return 8 * step + 4 * half; }
// accumulator v of lane half h of a 32 x 32 tile: vector 8 (v / 4) + 4 h + v % 4, bit lane % 32
VDB_ENC_HD inline int enc_acc_row(int v, int half) { return 8 * (v / 4) + 4 * half + v % 4; }
VDB_ENC_HD inline int enc_k_chunks(int Dp) { return (Dp + kEncKC - 1) / kEncKC; }
// the block's output words in LDS: [kEncBM][4] decided-one words, then as many undecided words
constexpr int kEncBlockWords = kEncBN / 32;
VDB_ENC_HD inline int64_t enc_lds_bytes() {
    return (int64_t)(kEncBM + kEncBN) * kEncLdsStride * 4 + (int64_t)kEncBM * 8 + (int64_t)2 * kEncBM * kEncBlockWords * 4;
}
constexpr int64_t kEncLdsLimit = 64 * 1024;
VDB_ENC_HD inline int64_t enc_row_blocks(int64_t n) { return (n + kEncBM - 1) / kEncBM; }
VDB_ENC_HD inline int enc_bit_blocks(int n_bits) { return (n_bits + kEncBN - 1) / kEncBN; }

// ---- the decision of one pair ---------------------------------------------------------------------
// a: the fp32 MFMA dot product of projection row and vector (any summation order).  With S the real dot
// product, s the canonical fp64 one and pn, xn the canonical fp64 norms, the analysis of
// range_mfma_decide (vdb_range_mfma_plan.h) gives
//   |a - s| <= crel pn xn + cabs (1 + pn + xn)       whenever a is finite and pn xn <= 2^126:
// crel = 2.02 (D + 8) 2^-24 is twice the round-to-nearest bound (it holds for an accumulator that
// truncates) plus (D + 8) 2^-50 for s against S; cabs = (D + 8) 2^-124 covers operands, products and
// partial sums flushed to zero or rounded as denormals.  The threshold is compared as it is given
// (fp64, no conversion); |t| 2^-48 covers the rounding of the subtraction a - t.  One and zero are
// certain for s > t; everything else, a NaN or an infinity among it, is undecided and pays fp64.
constexpr double kEncSlack64 = 0x1p-48;
VDB_ENC_HD inline double enc_crel(int D) { return 2.02 * (double)(D + 8) * 0x1p-24 + (double)(D + 8) * 0x1p-50; }
VDB_ENC_HD inline double enc_cabs(int D) { return (double)(D + 8) * 0x1p-124; }
enum { kEncZero = 0, kEncOne = 1, kEncUndecided = 2 };
VDB_ENC_HD inline int encode_decide(float af, double t, double pn, double xn, int D) {
    if (t != t) return kEncZero;  // a NaN threshold: no sum is above it
    const double a = (double)af;
    if (D > kEncMaxDim) return kEncUndecided;
    // fp32 overflow: nothing is known.  No partial sum passes pn xn in magnitude, so below 2^126 none overflowed.
    if (!(fabs(a) <= 3.4028234663852886e38) || !(pn * xn <= 0x1p126)) return kEncUndecided;
    const double e = enc_crel(D) * pn * xn + enc_cabs(D) * (1.0 + pn + xn) + fabs(t) * kEncSlack64;
    if (a - t >= e) return kEncOne;
    if (t - a >= e) return kEncZero;
    return kEncUndecided;  // (an infinite threshold of a's side, or e not finite)
}

// ---- scratch --------------------------------------------------------------------------------------
// One carve serves both calls (byte offsets, 256-aligned).  Host-memory arguments occupy [in0, in0 +
// in_bytes) in the order vectors, proj, thresholds and go up in one copy; the code bytes come down from
// [out, out + out_bytes).  Device-memory arguments are read where they are, and vdb_index_encode writes
// the caller's out_codes directly (out_bytes = 0 then unless `keep_out`: vdb_index_encode_codes keeps
// the row-major bytes here for the pack kernel).  The rest: the projection padded to [n_bits rounded
// up to 32][Dp] with its norms pn, the staged vectors [n][Dp] with their norms xn (vdb_index_encode
// with a projection), and the two word buffers [n][enc_word_stride] of the GEMM (knob 0 with a projection).
struct EncodeScratch {
    int64_t in0 = 0, in_bytes = 0, vec = 0, proj = 0, thr = 0;
    int64_t pw = 0, pn = 0, vw = 0, xn = 0, cw = 0, uw = 0, out = 0, out_bytes = 0, total = 0;
    int n_bytes = 0, stride = 0, pad_bits = 0;
};
// own_vectors: the call brings its vectors (vdb_index_encode); else they are the index's rows.
inline EncodeScratch encode_scratch(int64_t n, int dim, int Dp, int n_bits, bool has_proj, bool has_thr, bool host,
                                    bool own_vectors, bool words, bool keep_out) {
    EncodeScratch s;
    auto take = [&](int64_t bytes) {
        const int64_t at = (s.total + 255) / 256 * 256;
        s.total = at + bytes;
        return at;
    };
    s.n_bytes = enc_bytes(n_bits);
    s.stride = enc_word_stride(n_bits);
    s.pad_bits = (n_bits + 31) / 32 * 32;
    if (host) {
        s.in0 = take(0);
        s.vec = take(own_vectors ? n * dim * 4 : 0);
        s.proj = take(has_proj ? (int64_t)n_bits * dim * 4 : 0);
        s.thr = take(has_thr ? (int64_t)n_bits * 8 : 0);
        s.in_bytes = s.total - s.in0;
    }
    if (has_proj) {
        s.pw = take((int64_t)s.pad_bits * Dp * 4);
        s.pn = take((int64_t)s.pad_bits * 8);
        if (own_vectors) {
            s.vw = take(n * Dp * 4);
            s.xn = take(n * 8);
        }
        if (words) {
            s.cw = take(n * s.stride * 4);
            s.uw = take(n * s.stride * 4);
        }
    }
    if (host || keep_out) {
        s.out_bytes = n * s.n_bytes;
        s.out = take(s.out_bytes);
    }
    s.total = (s.total + 255) / 256 * 256;
    return s;
}

}  // namespace vdb
