// vdb_compact.hip: row removal (vdb_index_remove, vdb_api.cpp) — the keep-count scan over the
// remove bitmap and the stable, in-order gather of the surviving row-major rows and their per-row
// scalars.  The candidate copies are rebuilt from the moved rows by the ingest kernels
// (build_candidate_rows); only the tail of the int8 copy is zeroed here.
//
// Bitmap words are 32 rows, so every popcount here is the 32-bit one; nothing depends on the
// 64-lane ballot width.
#include <hip/hip_runtime.h>

#include "vdb_common.h"
#include "vdb_compact_plan.h"
#include "vdb_internal.h"

namespace vdb {

namespace {

constexpr int kScanThreads = 256;
constexpr int kScanPerThread = (int)(kScanWgWords / kScanThreads);  // 4 words per thread
static_assert(kScanThreads * kScanPerThread == kScanWgWords, "scan workgroup shape");

// The kept rows of word w: the valid bits the mask does not remove.
__device__ __forceinline__ uint32_t keep_bits(const uint32_t* __restrict__ mask, int64_t w, int64_t count) {
    const int64_t left = count - w * 32;
    const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : left <= 0 ? 0u : ((1u << (int)left) - 1u);
    return ~mask[w] & valid;
}

// Exclusive scan of v over the 256 threads of a workgroup; *total = the workgroup's sum.
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();  // s_wave may be reused by the caller's next round
    *total = all;
    return before + inc - v;
}

// Level 1.  Workgroup g handles words [g kScanWgWords, (g + 1) kScanWgWords): base[w] = kept rows
// of the workgroup's words below w, part[g] = its kept rows, info[1] = min over the words with a
// removed row (0xFFFFFFFF: none).
__global__ void __launch_bounds__(kScanThreads) keep_count_kernel(const uint32_t* __restrict__ mask, int64_t n_words,
                                                                  int64_t count, uint32_t* __restrict__ base,
                                                                  uint32_t* __restrict__ part,
                                                                  uint32_t* __restrict__ info) {
    __shared__ uint32_t s_wave[kScanThreads / 64];
    __shared__ uint32_t s_first;
    if (threadIdx.x == 0) s_first = 0xFFFFFFFFu;
    __syncthreads();
    const int64_t w0 = (int64_t)blockIdx.x * kScanWgWords + (int64_t)threadIdx.x * kScanPerThread;
    uint32_t cnt[kScanPerThread];
    uint32_t sum = 0, first = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        const int64_t w = w0 + j;
        cnt[j] = 0;
        if (w < n_words) {
            const uint32_t keep = keep_bits(mask, w, count);
            cnt[j] = (uint32_t)__popc(keep);
            const int64_t left = count - w * 32;
            const uint32_t rows = left >= 32 ? 32u : (uint32_t)left;
            if (cnt[j] != rows && first == 0xFFFFFFFFu) first = (uint32_t)w;
        }
        sum += cnt[j];
    }
    uint32_t total;
    uint32_t run = wg_exclusive_scan(sum, s_wave, &total);
#pragma unroll
    for (int j = 0; j < kScanPerThread; ++j) {
        const int64_t w = w0 + j;
        if (w < n_words) base[w] = run;
        run += cnt[j];
    }
    if (first != 0xFFFFFFFFu) atomicMin(&s_first, first);
    __syncthreads();
    if (threadIdx.x == 0) {
        part[blockIdx.x] = total;
        if (s_first != 0xFFFFFFFFu) atomicMin(info + 1, s_first);  // one per workgroup
    }
}

// Level 2, one workgroup: part[] -> its exclusive prefix sums in place; info[0] = the total.
__global__ void __launch_bounds__(kScanThreads) scan_partials_kernel(uint32_t* __restrict__ part, int64_t n_part,
                                                                     uint32_t* __restrict__ info) {
    __shared__ uint32_t s_wave[kScanThreads / 64];
    uint32_t carry = 0;
    for (int64_t i0 = 0; i0 < n_part; i0 += kScanThreads) {
        const int64_t i = i0 + threadIdx.x;
        const uint32_t v = i < n_part ? part[i] : 0u;
        uint32_t total;
        const uint32_t ex = wg_exclusive_scan(v, s_wave, &total);
        if (i < n_part) part[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) info[0] = carry;
}

// Level 3: base[w] += its workgroup's prefix; base[n_words] = the total.
__global__ void __launch_bounds__(256) add_base_kernel(uint32_t* __restrict__ base, const uint32_t* __restrict__ part,
                                                       int64_t n_words, const uint32_t* __restrict__ info) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (w < n_words) base[w] += part[w / kScanWgWords];
    else if (w == n_words) base[w] = info[0];
}

// Source rows of words [w0, w1) -> scratch: kept row r lands at scratch row
// base[r / 32] - base[w0] + popcount(kept bits of its word below r).  One thread per 16-byte
// piece of a row (Dp4 = Dp / 4 pieces); the thread of piece 0 also moves the row's scalars.
__global__ void __launch_bounds__(256) gather_rows_kernel(const float* __restrict__ X, const double* __restrict__ nrm64,
                                                          const float* __restrict__ inv32,
                                                          const float* __restrict__ sq32,
                                                          const float* __restrict__ rinit32,
                                                          const uint32_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ base, int64_t count, int64_t w0,
                                                          int64_t w1, int Dp4, float* __restrict__ sX,
                                                          double* __restrict__ sN, float* __restrict__ sI,
                                                          float* __restrict__ sS, float* __restrict__ sR) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t lr = idx / Dp4;
    const int c = (int)(idx - lr * Dp4);
    if (lr >= (w1 - w0) * 32) return;
    const int64_t r = w0 * 32 + lr;
    if (r >= count) return;
    const int64_t w = r >> 5;
    const int bit = (int)(r & 31);
    const uint32_t keep = keep_bits(mask, w, count);
    if (!((keep >> bit) & 1u)) return;
    const size_t pos = (size_t)(base[w] - base[w0]) + (size_t)__popc(keep & ((1u << bit) - 1u));
    const f32x4* src = (const f32x4*)X + (size_t)r * (size_t)Dp4 + c;
    f32x4* dst = (f32x4*)sX + pos * (size_t)Dp4 + c;
    *dst = *src;
    if (c == 0) {
        sN[pos] = nrm64[r];
        sI[pos] = inv32[r];
        sS[pos] = sq32[r];
        sR[pos] = rinit32[r];
    }
}

// Scratch rows [0, n) -> rows [base[w0], base[w0] + n) of the index, n = base[w1] - base[w0]
// (read here: the host never learns a chunk's row count).  The destination ends at or before
// row 32 w1, so no later chunk's source rows are overwritten.
__global__ void __launch_bounds__(256) place_rows_kernel(const float* __restrict__ sX, const double* __restrict__ sN,
                                                         const float* __restrict__ sI, const float* __restrict__ sS,
                                                         const float* __restrict__ sR,
                                                         const uint32_t* __restrict__ base, int64_t w0, int64_t w1,
                                                         int Dp4, float* __restrict__ X, double* __restrict__ nrm64,
                                                         float* __restrict__ inv32, float* __restrict__ sq32,
                                                         float* __restrict__ rinit32) {
    const size_t d0 = base[w0];
    const size_t n = (size_t)(base[w1] - base[w0]);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * (size_t)Dp4) return;
    ((f32x4*)X)[d0 * (size_t)Dp4 + idx] = ((const f32x4*)sX)[idx];
    if (idx < n) {
        nrm64[d0 + idx] = sN[idx];
        inv32[d0 + idx] = sI[idx];
        sq32[d0 + idx] = sS[idx];
        rinit32[d0 + idx] = sR[idx];
    }
}

// Both planes of rows [row0, row0 + n) of the int8 copy := 0 (one thread per plane and 16-dim
// chunk of a row, quant_rows' addressing).
__global__ void __launch_bounds__(256) zero_rows8_kernel(float* __restrict__ Xq, int64_t row0, int64_t n, int G8) {
    const int per_row = 4 * G8;  // 2 planes x 2 G8 chunks
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = idx / per_row;
    if (i >= n) return;
    const int t = (int)(idx - i * per_row);
    const int nc = 2 * G8;
    const int pl = t / nc, c = t - pl * nc;
    const uint64_t r = (uint64_t)(row0 + i);
    float* p = Xq + corpus_block(r >> 5, c >> 1, 0, G8) + (size_t)((r & 31) + 32 * (c & 1)) * 4 +
               (pl ? corpus_plane(G8) : 0);
    *(f32x4*)p = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
}

}  // namespace

size_t remove_scan_bytes(int64_t n_words) {
    const int64_t n_part = (n_words + kScanWgWords - 1) / kScanWgWords;
    return ((size_t)(n_words + 1) + (size_t)n_part + 2) * sizeof(uint32_t) + 512;
}

hipError_t launch_remove_scan(const uint32_t* mask, int64_t n_words, int64_t count, uint32_t* base, uint32_t* part,
                              uint32_t* info, hipStream_t st) {
    if (n_words <= 0) return hipSuccess;
    const int64_t n_part = (n_words + kScanWgWords - 1) / kScanWgWords;
    hipError_t e = hipMemsetAsync(info, 0, sizeof(uint32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(info + 1, 0xFF, sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(keep_count_kernel, dim3((unsigned)n_part), dim3(kScanThreads), 0, st, mask, n_words, count, base,
                       part, info);
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, st, part, n_part, info);
    hipLaunchKernelGGL(add_base_kernel, dim3((unsigned)((n_words + 1 + 255) / 256)), dim3(256), 0, st, base, part,
                       n_words, info);
    return hipGetLastError();
}

hipError_t launch_remove_chunk(const RemoveRows& a, const uint32_t* mask, const uint32_t* base, int64_t count,
                               int64_t w0, int64_t w1, const RemoveScratch& s, hipStream_t st) {
    if (w1 <= w0) return hipSuccess;
    const int Dp4 = a.Dp / 4;
    const int64_t pieces = (w1 - w0) * 32 * Dp4;
    const unsigned blocks = (unsigned)((pieces + 255) / 256);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, st, a.X, a.nrm64, a.inv32, a.sq32, a.rinit32,
                       mask, base, count, w0, w1, Dp4, s.X, s.nrm64, s.inv32, s.sq32, s.rinit32);
    hipLaunchKernelGGL(place_rows_kernel, dim3(blocks), dim3(256), 0, st, s.X, s.nrm64, s.inv32, s.sq32, s.rinit32,
                       base, w0, w1, Dp4, a.X, a.nrm64, a.inv32, a.sq32, a.rinit32);
    return hipGetLastError();
}

hipError_t launch_zero_rows8(float* Xq, int64_t row0, int64_t n, int G8, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int64_t total = n * 4 * G8;
    hipLaunchKernelGGL(zero_rows8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, Xq, row0, n, G8);
    return hipGetLastError();
}

}  // namespace vdb
