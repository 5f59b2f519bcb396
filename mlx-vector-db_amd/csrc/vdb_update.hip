// vdb_update.hip: in-place row update (vdb_index_update, vdb_api.cpp) — the validation pass over
// the staged ids and rows, and the row-list forms of the ingest kernels: the same per-row bodies
// (vdb_row_ops.h) over rows ids[0 .. n) instead of [row0, row0 + n), plus the signed column sums
// of the int8 copy over a row list.  Built with -ffp-contract=off like the range kernels.
//
// Every kernel here checks ids[i] against [0, count) itself and skips a row outside it: the
// validation pass has already rejected such a call, so this only keeps a list changed under a
// running call from addressing memory past the index.
#include <hip/hip_runtime.h>

#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_row_ops.h"

namespace vdb {

namespace {

__device__ __forceinline__ bool id_ok(int64_t id, int64_t count) { return (uint64_t)id < (uint64_t)count; }

// One wave per staged row i.  flags[0] |= 1: ids[i] outside [0, count); flags[1] |= 1: ids[i]
// given before (bit ids[i] of the bitmap, ceil(count / 32) words zeroed by the caller, was already
// set -- across all chunks of a call); flags[2] += 1: the row holds a NaN or Inf.
__global__ void __launch_bounds__(256) update_validate_kernel(const int64_t* __restrict__ ids,
                                                              const float* __restrict__ src, int64_t n, int D,
                                                              int64_t count, uint32_t* __restrict__ bitmap,
                                                              uint32_t* __restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    if (lane == 0) {
        const int64_t id = ids[i];
        if (!id_ok(id, count)) {
            atomicOr(flags, 1u);
        } else {
            const uint32_t bit = 1u << (int)(id & 31);
            if (atomicOr(bitmap + (id >> 5), bit) & bit) atomicOr(flags + 1, 1u);
        }
    }
    const float* s = src + i * (int64_t)D;
    int bad = 0;
    for (int d = lane; d < D; d += 64) bad |= !isfinite(s[d]);
    if (__any(bad) && lane == 0) atomicAdd(flags + 2, 1u);
}

__global__ void __launch_bounds__(256) update_pack_rows_kernel(const float* __restrict__ src,
                                                               const int64_t* __restrict__ ids, int64_t n,
                                                               int64_t count, int D, int G, float* __restrict__ X,
                                                               double* __restrict__ nrm64, float* __restrict__ inv32,
                                                               float* __restrict__ sq32, float* __restrict__ rinit32,
                                                               int normalise,
                                                               unsigned long long* __restrict__ xmax_bits,
                                                               int* __restrict__ nonfinite) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t id = ids[i];
    if (!id_ok(id, count)) return;
    pack_row(src + i * (int64_t)D, (uint64_t)id, lane, D, G, X, nrm64, inv32, sq32, rinit32, normalise, xmax_bits,
             nonfinite);
}

__global__ void __launch_bounds__(256) update_resid_dir_kernel(const float* __restrict__ X,
                                                               const float* __restrict__ inv32,
                                                               const int64_t* __restrict__ ids, int64_t n,
                                                               int64_t count, int D, int G,
                                                               const float* __restrict__ dir,
                                                               unsigned long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t id = ids[i];
    if (!id_ok(id, count)) return;
    resid_dir_row(X, inv32, (uint64_t)id, lane, D, G, dir, out);
}

// Thread (list entry i, fp32 group g8): that row's 8 dims into its split tile.  Rows of one
// tile write disjoint lanes of its blocks.
__global__ void __launch_bounds__(256) update_split_rows_kernel(const float* __restrict__ X, int G,
                                                                const int64_t* __restrict__ ids, int64_t n,
                                                                int64_t count, const float* __restrict__ inv32,
                                                                float* __restrict__ Xs) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = idx / G;
    if (i >= n) return;
    const int g8 = (int)(idx - i * G);
    const int64_t id = ids[i];
    if (!id_ok(id, count)) return;
    split_row_piece(X, G, (uint64_t)id, g8, inv32, Xs);
}

// Thread (list entry i, piece p): that row's 16 bytes into its fp32 tile.
__global__ void __launch_bounds__(256) update_tile_rows_kernel(const float* __restrict__ X, int G,
                                                               const int64_t* __restrict__ ids, int64_t n,
                                                               int64_t count, float* __restrict__ Xt) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = idx / (2 * G);
    if (i >= n) return;
    const int p = (int)(idx - i * (2 * G));
    const int64_t id = ids[i];
    if (!id_ok(id, count)) return;
    tile_row_piece(X, G, (uint64_t)id, p, Xt);
}

__global__ void __launch_bounds__(256) update_quant_rows_kernel(const float* __restrict__ X,
                                                                const float* __restrict__ inv32,
                                                                const float* __restrict__ mu,
                                                                const float* __restrict__ dir, float sx,
                                                                const int64_t* __restrict__ ids, int64_t n,
                                                                int64_t count, int G, float* __restrict__ Xq,
                                                                unsigned long long* __restrict__ stats,
                                                                int8_t* __restrict__ xh_rm) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t id = ids[i];
    if (!id_ok(id, count)) return;
    quant_row(X, inv32, mu, dir, sx, (uint64_t)id, lane, G, Xq, stats, xh_rm);
}

// csum[pl * Dp + d] += sign * (sum over rows ids[0 .. n) of plane pl), mod 2^32 -- colsum8_kernel
// (vdb_scan8.hip) over a row list, with a sign: an update takes the old bytes of its rows out
// (sign -1, before they are overwritten) and puts the new ones in (+1, after).  One thread per
// (plane, 16-dim chunk); a workgroup reduces `per` list entries in registers before its one atomic
// per column, so n rows cost 2 Dp ceil(n / per) atomics, not 2 Dp n.  per = kUpdColsumRows for a
// short list (more workgroups: 10 000 rows are 79 of them) and kUpdColsumRowsLong for a long one
// (fewer atomics per address: at 128 a 500 000-row update spent more time here than at 256).
// The rows are scattered, so each load is a latency of its own: kUpdColsumDepth of them are in
// flight per thread (with one at a time this kernel was half of a 10 000-row update's 0.6 ms).
constexpr int kUpdColsumRows = 128;
constexpr int kUpdColsumRowsLong = 512;
constexpr int64_t kUpdColsumLongFrom = 32768;  // list entries from which the long form runs
constexpr int kUpdColsumDepth = 8;
static_assert(kUpdColsumRows % kUpdColsumDepth == 0 && kUpdColsumRowsLong % kUpdColsumDepth == 0,
              "whole batches of loads per workgroup");
__global__ void __launch_bounds__(256) update_colsum8_kernel(const float* __restrict__ Xq,
                                                             const int64_t* __restrict__ ids, int64_t n,
                                                             int64_t count, int G8, int sign, int per,
                                                             uint32_t* __restrict__ csum) {
    const int nc = 2 * G8;  // 16-dim chunks per plane
    const int tid = threadIdx.x + blockIdx.y * 256;
    if (tid >= 2 * nc) return;
    const int pl = tid / nc, c = tid - pl * nc;
    const int64_t i0 = (int64_t)blockIdx.x * per;
    const int64_t i1 = min(i0 + (int64_t)per, n);
    int acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0;
    for (int64_t i = i0; i < i1; i += kUpdColsumDepth) {
        f32x4 v[kUpdColsumDepth];
#pragma unroll
        for (int u = 0; u < kUpdColsumDepth; ++u) {
            const int64_t id = i + u < i1 ? ids[i + u] : -1;
            v[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};  // (sixteen zero bytes add nothing)
            if (id_ok(id, count)) v[u] = *(const f32x4*)(Xq + i8_chunk_offset((uint64_t)id, c, pl, G8));
        }
#pragma unroll
        for (int u = 0; u < kUpdColsumDepth; ++u) colsum_acc16(v[u], sign, acc);
    }
    if (i0 < i1)
#pragma unroll
        for (int j = 0; j < 16; ++j) atomicAdd(csum + (size_t)pl * 32 * G8 + 16 * c + j, (uint32_t)acc[j]);
}

inline dim3 wave_per_row(int64_t n) { return dim3((unsigned)((n + 3) / 4)); }

}  // namespace

hipError_t launch_update_validate(const int64_t* ids, const float* src, int64_t n, int D, int64_t count,
                                  uint32_t* bitmap, uint32_t* flags, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(update_validate_kernel, wave_per_row(n), dim3(256), 0, st, ids, src, n, D, count, bitmap, flags);
    return hipGetLastError();
}

hipError_t launch_update_pack_rows(const float* src, const int64_t* ids, int64_t n, int64_t count, int D, int G,
                                   float* X, double* nrm64, float* inv32, float* sq32, float* rinit32, int normalise,
                                   unsigned long long* xmax_bits, int* nonfinite, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(update_pack_rows_kernel, wave_per_row(n), dim3(256), 0, st, src, ids, n, count, D, G, X, nrm64,
                       inv32, sq32, rinit32, normalise, xmax_bits, nonfinite);
    return hipGetLastError();
}

hipError_t launch_update_resid_dir(const float* X, const float* inv32, const int64_t* ids, int64_t n, int64_t count,
                                   int D, int G, const float* dir, unsigned long long* out, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(update_resid_dir_kernel, wave_per_row(n), dim3(256), 0, st, X, inv32, ids, n, count, D, G, dir,
                       out);
    return hipGetLastError();
}

hipError_t launch_update_split_rows(const float* X, int G, const int64_t* ids, int64_t n, int64_t count,
                                    const float* inv32, float* Xs, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t total = n * G;
    hipLaunchKernelGGL(update_split_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, G, ids, n,
                       count, inv32, Xs);
    return hipGetLastError();
}

hipError_t launch_update_tile_rows(const float* X, int G, const int64_t* ids, int64_t n, int64_t count, float* Xt,
                                   hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t total = n * 2 * G;
    hipLaunchKernelGGL(update_tile_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, X, G, ids, n,
                       count, Xt);
    return hipGetLastError();
}

hipError_t launch_update_quant_rows(const float* X, const float* inv32, const float* mu, const float* dir, float sx,
                                    const int64_t* ids, int64_t n, int64_t count, int G, float* Xq,
                                    unsigned long long* stats, int8_t* xh_rm, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(update_quant_rows_kernel, wave_per_row(n), dim3(256), 0, st, X, inv32, mu, dir, sx, ids, n,
                       count, G, Xq, stats, xh_rm);
    return hipGetLastError();
}

hipError_t launch_update_colsum8(const float* Xq, const int64_t* ids, int64_t n, int64_t count, int G8, int sign,
                                 uint32_t* csum, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int threads = 4 * G8;  // 2 planes x 2 G8 chunks
    const int per = n >= kUpdColsumLongFrom ? kUpdColsumRowsLong : kUpdColsumRows;
    hipLaunchKernelGGL(update_colsum8_kernel, dim3((unsigned)((n + per - 1) / per), (unsigned)((threads + 255) / 256)),
                       dim3(256), 0, st, Xq, ids, n, count, G8, sign, per, csum);
    return hipGetLastError();
}

}  // namespace vdb
