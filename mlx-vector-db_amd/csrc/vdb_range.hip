// vdb_range.hip: range search (vdb_index_search_range) — every row whose canonical fp64 key is at
// or above a per-query bound, with exact counts; part of the gfx950 kernels of the brute-force
// path (pipeline overview: vdb_scan.hip).  Built with -ffp-contract=off.
//
// The rows come from the row-major fp32 copy and the keys from the canonical helpers of
// vdb_exact_keys.h, so the candidate copies are never read and the result is the oracle's set
// whatever the index's precision.  A batch runs in blocks of up to 64 queries (vdb_range_plan.h
// range_query_block), each block in four launches over the same scratch:
//
//   scan    grid = chunks of 512 rows, 4 waves.  A wave owns whole 32-row bitmap words: it holds
//           the pieces of 4 rows in registers and scores them against every query of the block
//           (the queries are read through L1, as exact_keys_rows reads its one), so the corpus is
//           read once per block and not once per query.  Lane j keeps query j's word in a register
//           and stores it once to H [block][n_words] (the row_mask layout): no atomics.  Masked-out
//           rows are skipped before their keys are computed.  part [block][n_chunks] = the
//           workgroup's hits per query (sums of popcounts).
//   prefix  one workgroup per query: part -> its exclusive prefix sums in place, the total to
//           cnt [block] and to the caller's counts.
//   emit    one thread per word: the hit at position p = prefix + popcount(bits below) with
//           p < cap gets its row id written to slot p; a workgroup whose first prefix is already
//           at or past cap returns at once.
//   score   one wave per filled slot recomputes the row's key with exact_key (the same canonical
//           order, so the same bits as the scan's) and writes score and key; the slots from
//           min(count, cap) to cap get the "no result" values.  Nothing is written at or past cap.
//
// A count-only call (cap == 0) runs scan and prefix alone.  Device-memory calls are not validated
// on the host: a NaN threshold or a negative radius becomes a NaN bound, which no key reaches.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_exact_keys.h"
#include "vdb_range_plan.h"

namespace vdb {

namespace {

// MP: 4 / 8 = rows of up to 256 MP dims, the pieces of kRangeNB rows held in registers across the
// block's queries; 0 = any length: one piece per row in flight per trip and the rows read again
// (through the caches) for each query.
template <int METRIC, int MP>
__global__ void __launch_bounds__(256) range_scan_kernel(RangeArgs a, int b0, int qb) {
    constexpr int NB = kRangeNB;
    __shared__ uint32_t s_cnt[kRangeWaves][64];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int64_t chunk = blockIdx.x;
    const int64_t n_words = range_n_words(a.N);
    const int64_t n_chunks = range_n_chunks(n_words);
    const int np = (a.D + 255) / 256;
    const float* Q = a.Q + (int64_t)b0 * a.D;
    const double* qn64 = a.qn64 + b0;
    // lane j: the bound of query j of the block
    const double kt = lane < qb ? range_kt(METRIC, a.thr[b0 + lane]) : (double)NAN;
    uint32_t total = 0;
    for (int i = 0; i < kRangeWaveWords; ++i) {
        const int64_t w = range_wave_word(chunk, wv, i);
        if (w >= n_words) break;
        const uint32_t elig = range_valid_bits(w, a.N) & (a.mask ? a.mask[w] : 0xFFFFFFFFu);
        uint32_t word = 0;
        for (int t = 0; t < 32 / NB; ++t) {
            const uint32_t e = (elig >> (t * NB)) & ((1u << NB) - 1u);
            if (e == 0) continue;  // no eligible row among these: nothing is read
            uint32_t rws[NB];
            double xn[NB];
            bool ok[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                ok[u] = (e >> u) & 1u;
                rws[u] = ok[u] ? (uint32_t)(w * 32 + t * NB + u) : 0u;  // (an ineligible row is not scored)
                xn[u] = (METRIC == 0 && ok[u]) ? a.nrm64[rws[u]] : 1.0;
            }
            f32x4 xv[MP > 0 ? MP : 1][NB];
            if constexpr (MP > 0) rows_pieces_load<NB, MP>(a.X, a.G, np, rws, ok, xv);
            for (int j = 0; j < qb; ++j) {
                const float* q = Q + (int64_t)j * a.D;
                const double qn = qn64[j];
                double keys[NB];
                if constexpr (MP > 0)
                    exact_keys_held<METRIC, NB, MP>(q, a.D, qn, np, xv, xn, keys);
                else
                    exact_keys_batch<METRIC, NB>(q, qn, a.X, a.G, a.D, rws, xn, NB, keys);
                const double ktj = __shfl(kt, j, 64);
                uint32_t bits = 0;
#pragma unroll
                for (int u = 0; u < NB; ++u)
                    if (ok[u] && keys[u] >= ktj) bits |= 1u << u;
                if (lane == j) word |= bits << (t * NB);
            }
        }
        if (lane < qb) a.H[(size_t)lane * (size_t)n_words + (size_t)w] = word;
        total += (uint32_t)__popc(word);
    }
    s_cnt[wv][lane] = total;
    __syncthreads();
    if (wv == 0 && lane < qb) {
        uint32_t c = 0;
#pragma unroll
        for (int x = 0; x < kRangeWaves; ++x) c += s_cnt[x][lane];
        a.part[(size_t)lane * (size_t)n_chunks + (size_t)chunk] = c;
    }
}

// Exclusive scan of v over the 256 threads of a workgroup; *total = the workgroup's sum.
__device__ __forceinline__ uint32_t wg256_exclusive_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
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
    for (int w = 0; w < 4; ++w) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();  // s_wave is reused by the next round
    *total = all;
    return before + inc - v;
}

// Workgroup q: part[q][0 .. n_chunks) -> its exclusive prefix sums in place (a count is at most the
// row count, below 2^32); the total to cnt[q] and the caller's counts[b0 + q].
__global__ void __launch_bounds__(256) range_prefix_kernel(uint32_t* __restrict__ part, int64_t n_chunks,
                                                           int64_t* __restrict__ cnt, int64_t* __restrict__ out_c,
                                                           int b0) {
    __shared__ uint32_t s_wave[4];
    const int q = blockIdx.x;
    uint32_t* p = part + (size_t)q * (size_t)n_chunks;
    uint32_t carry = 0;
    for (int64_t i0 = 0; i0 < n_chunks; i0 += 256) {
        const int64_t i = i0 + threadIdx.x;
        const uint32_t v = i < n_chunks ? p[i] : 0u;
        uint32_t total;
        const uint32_t ex = wg256_exclusive_scan(v, s_wave, &total);
        if (i < n_chunks) p[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        cnt[q] = (int64_t)carry;
        out_c[b0 + q] = (int64_t)carry;
    }
}

// grid (range_emit_wgs, qb): thread t of workgroup g takes word 256 g + t of query blockIdx.y.
__global__ void __launch_bounds__(kRangeEmitWords) range_emit_kernel(RangeArgs a, int b0) {
    const int q = blockIdx.y;
    const int64_t n_words = range_n_words(a.N);
    const int64_t n_chunks = range_n_chunks(n_words);
    const uint32_t* part = a.part + (size_t)q * (size_t)n_chunks;
    const int64_t w0 = (int64_t)blockIdx.x * kRangeEmitWords;
    if (!range_emit_live((int64_t)part[w0 / kRangeWgWords], a.cap)) return;  // prefixes ascend: nothing below cap here
    const int64_t w = w0 + threadIdx.x;
    const bool in = w < n_words;
    uint32_t word = in ? a.H[(size_t)q * (size_t)n_words + (size_t)w] : 0u;
    // exclusive prefix of the popcounts within the word's chunk (16 consecutive lanes)
    const uint32_t c = (uint32_t)__popc(word);
    uint32_t inc = c;
#pragma unroll
    for (int off = 1; off < kRangeWgWords; off <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, off, kRangeWgWords);
        if ((int)(threadIdx.x & (kRangeWgWords - 1)) >= off) inc += o;
    }
    if (!in) return;
    int64_t p = (int64_t)part[w / kRangeWgWords] + (int64_t)(inc - c);
    int64_t* out = a.out_i + (int64_t)(b0 + q) * a.cap;
    while (word && p < a.cap) {
        const int bit = __ffs((int)word) - 1;
        out[p++] = w * 32 + bit + a.index_offset;
        word &= word - 1u;
    }
}

// grid (range_score_wgs, qb), 4 waves: slots [0, n) one wave each (n = min(count, cap)), the row id
// read back from the slot; slots [n, cap) one thread each.
template <int METRIC>
__global__ void __launch_bounds__(256) range_score_kernel(RangeArgs a, int b0) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.y;
    const int b = b0 + q;
    const int64_t n = range_filled(a.cnt[q], a.cap);
    const float* qv = a.Q + (int64_t)b * a.D;
    const double qn = a.qn64[b];
    int64_t* oi = a.out_i + (int64_t)b * a.cap;
    float* os = a.out_s + (int64_t)b * a.cap;
    double* ok = a.out_k ? a.out_k + (int64_t)b * a.cap : nullptr;
    const int64_t n_waves = (int64_t)gridDim.x * kRangeWaves;
    for (int64_t p = (int64_t)blockIdx.x * kRangeWaves + (threadIdx.x >> 6); p < n; p += n_waves) {
        const int64_t id = oi[p];
        const uint64_t r = (uint64_t)(id - a.index_offset);
        const double key = exact_key<METRIC>(qv, qn, a.X, a.G, a.D, r, METRIC == 0 ? a.nrm64[r] : 1.0);
        if (lane == 0) write_result(METRIC, key, (uint64_t)id, true, os + p, oi + p, ok ? ok + p : nullptr);
    }
    const int64_t n_thr = (int64_t)gridDim.x * 256;
    for (int64_t p = n + (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.cap; p += n_thr)
        write_result(METRIC, -INFINITY, 0, false, os + p, oi + p, ok ? ok + p : nullptr);
}

}  // namespace

hipError_t launch_range_block(int metric, const RangeArgs& a, int b0, int qb, hipStream_t st) {
    if (qb <= 0) return hipSuccess;
    if (qb > kRangeMaxBlock || b0 < 0 || a.N <= 0 || a.cap < 0 || (metric != 0 && metric != 1) || !a.H || !a.part ||
        !a.cnt || !a.out_c || (a.cap > 0 && (!a.out_i || !a.out_s)))
        return hipErrorInvalidValue;
    const int64_t n_words = range_n_words(a.N);
    const int64_t n_chunks = range_n_chunks(n_words);
    const int mp = a.D <= 1024 ? 4 : a.D <= 2048 ? 8 : 0;
    bool launched = false;
#define VDB_RANGE_SCAN(M, MPV)                                                                                      \
    if (metric == M && mp == MPV) {                                                                                 \
        hipLaunchKernelGGL((range_scan_kernel<M, MPV>), dim3((unsigned)n_chunks), dim3(256), 0, st, a, b0, qb);     \
        launched = true;                                                                                            \
    }
    VDB_RANGE_SCAN(0, 4) VDB_RANGE_SCAN(0, 8) VDB_RANGE_SCAN(0, 0)
    VDB_RANGE_SCAN(1, 4) VDB_RANGE_SCAN(1, 8) VDB_RANGE_SCAN(1, 0)
#undef VDB_RANGE_SCAN
    if (!launched) return hipErrorInvalidValue;
    hipLaunchKernelGGL(range_prefix_kernel, dim3(qb), dim3(256), 0, st, a.part, n_chunks, a.cnt, a.out_c, b0);
    if (a.cap > 0) {
        hipLaunchKernelGGL(range_emit_kernel, dim3((unsigned)range_emit_wgs(n_words), qb), dim3(kRangeEmitWords), 0, st,
                           a, b0);
        const dim3 sg(range_score_wgs(a.cap), qb);
        if (metric == 0)
            hipLaunchKernelGGL((range_score_kernel<0>), sg, dim3(256), 0, st, a, b0);
        else
            hipLaunchKernelGGL((range_score_kernel<1>), sg, dim3(256), 0, st, a, b0);
    }
    return hipGetLastError();
}

}  // namespace vdb
