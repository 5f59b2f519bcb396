// vdb_exact_keys.h: the exact fp64 key of a (query, row) pair, one wave per row, and its batched
// forms (several rows' pieces in flight per wave).  Shared by the exact paths of vdb_exact.hip
// (rerank, finish, exact scan), the row-list search (vdb_subset.hip) and the range search
// (vdb_range.hip): every form accumulates in the canonical order of vdb_common.h, so their keys are
// bit-identical.  Built with -ffp-contract=off.
#pragma once
#include "vdb_common.h"

namespace vdb {

// =============================================================================
// Exact fp64 keys
// =============================================================================
// key(q, r): cosine  dot / (max(|q|,1e-8) * max(|x|,1e-8))
//            L2      -(sum (x-q)^2)
// in the canonical order (vdb_common.h).  One wave per (query, row); up to four
// 16-byte corpus pieces per lane in flight.
template <int METRIC>
__device__ __forceinline__ double exact_key(const float* __restrict__ q, double qn, const float* __restrict__ X, int G,
                                            int D, uint64_t r, double xn) {
    const int lane = threadIdx.x & 63;
    const int Dp = G * GROUP_DIMS;
    const int np = (D + 255) / 256;
    double acc = 0.0;
    for (int m0 = 0; m0 < np; m0 += 4) {
        f32x4 xv[4];
        float qv[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = (m0 + u) * 64 + lane;
            const bool in = (m0 + u) < np;
            xv[u] = (in && 4 * p < Dp) ? *(const f32x4*)(X + row_piece_offset(r, p, G)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) qv[u][j] = (in && 4 * p + j < D) ? q[4 * p + j] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if ((m0 + u) < np) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double qd = (double)qv[u][j];
                    const double xd = (double)xv[u][j];
                    if (METRIC == 0) {
                        acc = acc + qd * xd;
                    } else {
                        const double df = xd - qd;
                        acc = acc + df * df;
                    }
                }
            }
        }
    }
    acc = wave_sum_butterfly(acc);
    if (METRIC == 0) return acc / (fmax(qn, 1e-8) * fmax(xn, 1e-8));
    return -acc;
}

// The same keys (same canonical order) for NB rows at once, rows of up to 256 MP dims: every
// piece of the NB rows in flight at once, the query's pieces read from memory (L1-resident) as
// each is consumed instead of held in registers.
template <int METRIC, int NB, int MP>
__device__ __forceinline__ void exact_keys_rows(const float* __restrict__ q, int D, double qn,
                                                const float* __restrict__ X, int G, int np, const uint32_t* rows,
                                                const double* xn, int nb, double* out) {
    const int lane = threadIdx.x & 63;
    const int Dp = G * GROUP_DIMS;
    f32x4 xv[MP][NB];
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        const int p = m * 64 + lane;
#pragma unroll
        for (int u = 0; u < NB; ++u)
            xv[m][u] = (m < np && u < nb && 4 * p < Dp) ? *(const f32x4*)(X + row_piece_offset(rows[u], p, G))
                                                       : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    double acc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) acc[u] = 0.0;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        if (m < np) {
            float qv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = 4 * (m * 64 + lane) + j;
                qv[j] = d < D ? q[d] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < NB; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double qd = (double)qv[j];
                    const double xd = (double)xv[m][u][j];
                    if (METRIC == 0) {
                        acc[u] = acc[u] + qd * xd;
                    } else {
                        const double df = xd - qd;
                        acc[u] = acc[u] + df * df;
                    }
                }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int u = 0; u < NB; ++u) acc[u] = acc[u] + __shfl_xor(acc[u], off, 64);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (u < nb) out[u] = METRIC == 0 ? acc[u] / (fmax(qn, 1e-8) * fmax(xn[u], 1e-8)) : -acc[u];
    }
}

// The multi-query form of exact_keys_rows (the range scan, vdb_range.hip): the pieces of NB rows
// are loaded once (rows_pieces_load; a row whose ok[u] is false is not read and holds zeros) and
// then scored against one query after another (exact_keys_held), each key in the same canonical
// order, so a block of queries costs one read of the rows.
template <int NB, int MP>
__device__ __forceinline__ void rows_pieces_load(const float* __restrict__ X, int G, int np, const uint32_t* rows,
                                                 const bool* ok, f32x4 (&xv)[MP][NB]) {
    const int lane = threadIdx.x & 63;
    const int Dp = G * GROUP_DIMS;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        const int p = m * 64 + lane;
#pragma unroll
        for (int u = 0; u < NB; ++u)
            xv[m][u] = (m < np && ok[u] && 4 * p < Dp) ? *(const f32x4*)(X + row_piece_offset(rows[u], p, G))
                                                       : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
template <int METRIC, int NB, int MP>
__device__ __forceinline__ void exact_keys_held(const float* __restrict__ q, int D, double qn, int np,
                                                const f32x4 (&xv)[MP][NB], const double* xn, double* out) {
    const int lane = threadIdx.x & 63;
    double acc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) acc[u] = 0.0;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        if (m < np) {
            float qv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int d = 4 * (m * 64 + lane) + j;
                qv[j] = d < D ? q[d] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < NB; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double qd = (double)qv[j];
                    const double xd = (double)xv[m][u][j];
                    if (METRIC == 0) {
                        acc[u] = acc[u] + qd * xd;
                    } else {
                        const double df = xd - qd;
                        acc[u] = acc[u] + df * df;
                    }
                }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int u = 0; u < NB; ++u) acc[u] = acc[u] + __shfl_xor(acc[u], off, 64);
#pragma unroll
    for (int u = 0; u < NB; ++u) out[u] = METRIC == 0 ? acc[u] / (fmax(qn, 1e-8) * fmax(xn[u], 1e-8)) : -acc[u];
}

// ... and for rows of any length: one piece of each of the NB rows in flight per trip.
template <int METRIC, int NB>
__device__ __forceinline__ void exact_keys_batch(const float* __restrict__ q, double qn, const float* __restrict__ X,
                                                 int G, int D, const uint32_t* rows, const double* xn, int nb,
                                                 double* out) {
    const int lane = threadIdx.x & 63;
    const int Dp = G * GROUP_DIMS;
    const int np = (D + 255) / 256;
    double acc[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) acc[u] = 0.0;
    for (int m = 0; m < np; ++m) {
        const int p = m * 64 + lane;
        float qv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) qv[j] = 4 * p + j < D ? q[4 * p + j] : 0.0f;
        f32x4 xv[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u)
            xv[u] = (u < nb && 4 * p < Dp) ? *(const f32x4*)(X + row_piece_offset(rows[u], p, G)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < NB; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double qd = (double)qv[j];
                const double xd = (double)xv[u][j];
                if (METRIC == 0) {
                    acc[u] = acc[u] + qd * xd;
                } else {
                    const double df = xd - qd;
                    acc[u] = acc[u] + df * df;
                }
            }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int u = 0; u < NB; ++u) acc[u] = acc[u] + __shfl_xor(acc[u], off, 64);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (u < nb) out[u] = METRIC == 0 ? acc[u] / (fmax(qn, 1e-8) * fmax(xn[u], 1e-8)) : -acc[u];
    }
}

}  // namespace vdb
