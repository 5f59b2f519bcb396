// vdb_row_ops.h — the per-row bodies of the ingest kernels, shared by the range kernels
// (rows [row0, row0 + n): vdb_ingest.hip, vdb_scan8.hip) and the row-list kernels of
// vdb_index_update (rows ids[0..n): vdb_update.hip).  One definition of each row's arithmetic,
// so a row written by an update is bit for bit the row an add would have written.
// Every file that includes this is built with -ffp-contract=off.
#pragma once
#include "vdb_common.h"

namespace vdb {

// pack_rows: one wave (lane = 0..63) stores source row s [D] as row r of X (padding dims zero)
// with its canonical fp64 norm, the fp32 row terms and the running maxima of xmax_bits.
__device__ __forceinline__ void pack_row(const float* __restrict__ s, uint64_t r, int lane, int D, int G,
                                         float* __restrict__ X, double* __restrict__ nrm64,
                                         float* __restrict__ inv32, float* __restrict__ sq32,
                                         float* __restrict__ rinit32, int normalise,
                                         unsigned long long* __restrict__ xmax_bits, int* __restrict__ nonfinite) {
    const int Dp = G * GROUP_DIMS;
    const int np = (D + 255) / 256;
    double acc = 0.0;
    int bad = 0;
    for (int m = 0; m < np; ++m) {
        const int p = m * 64 + lane;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = 4 * p + j;
            v[j] = d < D ? s[d] : 0.0f;
            bad |= !isfinite(v[j]);
            const double dv = (double)v[j];
            acc = acc + dv * dv;
        }
        if (4 * p < Dp) *(f32x4*)(X + row_piece_offset(r, p, G)) = v;
    }
    acc = wave_sum_butterfly(acc);
    const double nr = sqrt(acc);
    const float iv = (float)(1.0 / fmax(nr, 1e-8));
    // the split copy's row and its bf16 residual |y - bf16(y)|
    double res = 0.0, yy = 0.0;
    for (int m = 0; m < np; ++m) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = 4 * (m * 64 + lane) + j;
            const float x = d < D ? s[d] : 0.0f;
            const float y = normalise ? x * iv : x;
            const double rv = (double)y - (double)__uint_as_float(bf16_rne_bits(y) << 16);
            res = res + rv * rv;
            yy = yy + (double)y * (double)y;
        }
    }
    res = wave_sum_butterfly(res);
    yy = wave_sum_butterfly(yy);
    const int anybad = __any(bad);
    if (lane == 0) {
        nrm64[r] = nr;
        inv32[r] = iv;
        sq32[r] = (float)acc;
        rinit32[r] = -0.5f * (float)acc;
        if (anybad) {
            atomicAdd(nonfinite, 1);
        } else {
            // xmax_bits[0] max |x|; [1] max |y - bf16(y)| / max(|y|, 1e-8); [2] max |y - bf16(y)|
            // (non-negative doubles order like their bit patterns; a plain read first: the
            // maxima are monotone, so a stale value only lets an atomic through)
            const double dr = sqrt(res);
            const unsigned long long v[3] = {(unsigned long long)__double_as_longlong(nr),
                                             (unsigned long long)__double_as_longlong(dr / fmax(sqrt(yy), 1e-8)),
                                             (unsigned long long)__double_as_longlong(dr)};
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (v[i] > __atomic_load_n(xmax_bits + i, __ATOMIC_RELAXED)) atomicMax(xmax_bits + i, v[i]);
        }
    }
}

// resid_dir: one wave, |dir . (y - bf16(y))| of row r, maximum into *out (fp64 bits).
__device__ __forceinline__ void resid_dir_row(const float* __restrict__ X, const float* __restrict__ inv32,
                                              uint64_t r, int lane, int D, int G, const float* __restrict__ dir,
                                              unsigned long long* __restrict__ out) {
    const float iv = inv32 ? inv32[r] : 1.0f;
    const int np = (D + 255) / 256;
    double acc = 0.0;
    for (int m = 0; m < np; ++m) {
        const int p = m * 64 + lane;
        if (4 * p >= D) break;
        const f32x4 xv = *(const f32x4*)(X + row_piece_offset(r, p, G));
        const f32x4 dv = *(const f32x4*)(dir + 4 * p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = inv32 ? xv[j] * iv : xv[j];
            const double rv = (double)y - (double)__uint_as_float(bf16_rne_bits(y) << 16);
            acc = acc + (double)dv[j] * rv;
        }
    }
    acc = wave_sum_butterfly(acc);
    if (lane == 0) {
        const unsigned long long v = (unsigned long long)__double_as_longlong(fabs(acc));
        if (v > __atomic_load_n(out, __ATOMIC_RELAXED)) atomicMax(out, v);
    }
}

// split_rows: one thread, the 8 dims 8 g8 .. 8 g8 + 7 of row r (times inv32[r] for cosine) ->
// lane (r & 31) + 32 (g8 & 1) of the hi and lo blocks of 16-dim group g8 >> 1 of tile r >> 5.
__device__ __forceinline__ void split_row_piece(const float* __restrict__ X, int G, uint64_t r, int g8,
                                                const float* __restrict__ inv32, float* __restrict__ Xs) {
    const int i = (int)(r & 31);
    const uint64_t t = r >> 5;
    const float* src = X + row_piece_offset(t * 32 + i, 2 * g8, G);
    f32x4 a = *(const f32x4*)src;
    f32x4 b = *(const f32x4*)(src + 4);
    if (inv32) {
        const float iv = inv32[t * 32 + i];
        a *= iv;
        b *= iv;
    }
    f32x4 hi, lo;
    split8(a, b, hi, lo);
    float* dst = Xs + corpus_block(t, g8 >> 1, 0, G >> 1) + (size_t)(i + 32 * (g8 & 1)) * 4;
    *(f32x4*)dst = hi;
    *(f32x4*)(dst + corpus_plane(G >> 1)) = lo;
}

// tile_rows: one thread, piece p of row r -> its place in the fp32 tiles.
__device__ __forceinline__ void tile_row_piece(const float* __restrict__ X, int G, uint64_t r, int p,
                                               float* __restrict__ Xt) {
    *(f32x4*)(Xt + tiled_piece_offset(r, p, G)) = *(const f32x4*)(X + row_piece_offset(r, p, G));
}

// 16 values -> 16 int8 (byte j = element j) in one f32x4
__device__ __forceinline__ f32x4 pack_i8x16(const int (&v)[16]) {
    f32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t u = (uint32_t)(v[4 * w] & 255) | ((uint32_t)(v[4 * w + 1] & 255) << 8) |
                           ((uint32_t)(v[4 * w + 2] & 255) << 16) | ((uint32_t)(v[4 * w + 3] & 255) << 24);
        o[w] = __uint_as_float(u);
    }
    return o;
}

// t -> (hi, lo) with t ~ hi + lo / 256, |hi|, |lo| <= 127 (values past the range clip; the
// residual the statistics measure then shows it)
__device__ __forceinline__ void split_i8(float t, int& hi, int& lo) {
    hi = (int)fminf(fmaxf(rintf(t), -127.0f), 127.0f);
    lo = (int)fminf(fmaxf(rintf((t - (float)hi) * 256.0f), -127.0f), 127.0f);
}

// float offset of the 16 bytes of plane pl, 16-dim chunk c of row r in the int8 copy
__device__ __forceinline__ size_t i8_chunk_offset(uint64_t r, int c, int pl, int G8) {
    return corpus_block(r >> 5, c >> 1, 0, G8) + (size_t)((r & 31) + 32 * (c & 1)) * 4 + (pl ? corpus_plane(G8) : 0);
}

// quant_rows: one wave, z = y - mu of row r -> the xh / xl planes of the int8 copy (block (tile,
// 32-dim group g, plane) lane i + 32 h holds dims 32 g + 16 h .. + 15 of row 32 t + i), the
// row-major xh (optional) and the row statistics (fp64 bits, running maxima) stats[0] |z - s_x xh|,
// [1] |dir.(z - s_x xh)|, [2] |z - z~|, [3] |dir.(z - z~)| (z~ = s_x (xh + xl/256)), [4] |s_x xh|,
// [5] |s_x xl / 256|.
__device__ __forceinline__ void quant_row(const float* __restrict__ X, const float* __restrict__ inv32,
                                          const float* __restrict__ mu, const float* __restrict__ dir, float sx,
                                          uint64_t r, int lane, int G, float* __restrict__ Xq,
                                          unsigned long long* __restrict__ stats, int8_t* __restrict__ xh_rm) {
    const float iv = inv32 ? inv32[r] : 1.0f;
    const float isx = 1.0f / sx;
    const int G8 = G >> 2;
    const int nc = 2 * G8;  // 16-dim chunks
    double s_r8 = 0.0, s_d8 = 0.0, s_r16 = 0.0, s_d16 = 0.0, s_h = 0.0, s_l = 0.0;
    for (int c = lane; c < nc; c += 64) {
        const float* src = X + (size_t)r * (size_t)(8 * G) + 16 * c;
        int hv[16], lv[16];
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            const f32x4 xv = *(const f32x4*)(src + 4 * j4);
            const f32x4 mv = *(const f32x4*)(mu + 16 * c + 4 * j4);
            const f32x4 dv = *(const f32x4*)(dir + 16 * c + 4 * j4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float z = (inv32 ? xv[j] * iv : xv[j]) - mv[j];
                int h, l;
                split_i8(z * isx, h, l);
                hv[4 * j4 + j] = h;
                lv[4 * j4 + j] = l;
                const double zh = (double)sx * h, zl = (double)sx * l / 256.0;
                const double r8 = (double)z - zh, r16 = r8 - zl;
                s_r8 += r8 * r8;
                s_r16 += r16 * r16;
                s_d8 += (double)dv[j] * r8;
                s_d16 += (double)dv[j] * r16;
                s_h += zh * zh;
                s_l += zl * zl;
            }
        }
        const uint64_t t = r >> 5;
        float* dst = Xq + corpus_block(t, c >> 1, 0, G8) + (size_t)((r & 31) + 32 * (c & 1)) * 4;
        *(f32x4*)dst = pack_i8x16(hv);
        *(f32x4*)(dst + corpus_plane(G8)) = pack_i8x16(lv);
        // the xh plane row-major too (as xh + 128): the finish's refinement reads candidates' rows whole
        if (xh_rm) {  // biased to unsigned (xh + 128): one v_cvt_f32_ubyte per element in the finish
            int uv[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) uv[j] = hv[j] + 128;
            *(f32x4*)(xh_rm + r * (size_t)(8 * G) + 16 * c) = pack_i8x16(uv);
        }
    }
    s_r8 = wave_sum_butterfly(s_r8);
    s_d8 = wave_sum_butterfly(s_d8);
    s_r16 = wave_sum_butterfly(s_r16);
    s_d16 = wave_sum_butterfly(s_d16);
    s_h = wave_sum_butterfly(s_h);
    s_l = wave_sum_butterfly(s_l);
    if (lane == 0) {
        const double v[6] = {sqrt(s_r8), fabs(s_d8), sqrt(s_r16), fabs(s_d16), sqrt(s_h), sqrt(s_l)};
        bool fin = true;  // a non-finite row (the whole add is rejected) leaves no statistics
#pragma unroll
        for (int k = 0; k < 6; ++k) fin = fin && isfinite(v[k]);
#pragma unroll
        for (int k = 0; k < 6 && fin; ++k) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(v[k]);
            if (b > __atomic_load_n(stats + k, __ATOMIC_RELAXED)) atomicMax(stats + k, b);
        }
    }
}

// 16 int8 of one f32x4 added (sign +1) to or taken from (sign -1) 16 running column sums
__device__ __forceinline__ void colsum_acc16(const f32x4 v, int sign, int (&acc)[16]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t u = __float_as_uint(v[w]);
#pragma unroll
        for (int bt = 0; bt < 4; ++bt) acc[4 * w + bt] += sign * (int)(int8_t)((u >> (8 * bt)) & 255u);
    }
}

}  // namespace vdb
