// vdb_filter.hip: predicate masks over the index's numeric columns (vdb_index_filter_mask) — up to
// 256 predicates, each the AND of up to 8 interval clauses on fp64 columns, evaluated in one launch
// into row bitmaps of the row_mask layout, with exact counts; part of the gfx950 kernels of the
// brute-force path (pipeline overview: vdb_scan.hip).
//
// One kernel.  A workgroup (4 waves) stages the call's clauses and offsets in LDS once (dynamic LDS
// sized by the call: 24 B a clause, 12 B a predicate, 52 KB for the largest call) and then
// walks pairs of mask words round robin (vdb_filter_plan.h filter_wave_pair): a wave owns the 64
// rows of one pair, a lane one row.  The lane loads its row's value from every column the call
// uses, once (coalesced 8-byte loads, one column at a time; a tail row loads nothing and holds NaN),
// and then loops over the predicates with the values in registers, so the column bytes are read
// once for all the predicates of the call.  A 64-lane ballot gives the two words of a predicate;
// lane j keeps the words of predicate j of the current block of 64 and, the block done, ANDs them
// with the base words and stores them: two 32-bit stores, because a mask is only 4-byte aligned
// (predicate p starts at word p * W, odd for odd W), and the high word only where it exists (odd W:
// the last pair has none).  Counts are popcounts of the stored words, summed per lane, then per
// workgroup in LDS, then into the caller's counts with one 64-bit integer atomic per predicate and
// workgroup: integer sums, so the order does not show.  There is no arithmetic on the values.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_filter_plan.h"

namespace vdb {

namespace {

// The value of slot `col` (wave-uniform) among the 16 held in registers: a scalar branch, since a
// register array indexed at run time would live in scratch memory.
__device__ __forceinline__ double pick_value(const double (&v)[kFilterSlots], int col) {
    switch (col) {
        case 0: return v[0];
        case 1: return v[1];
        case 2: return v[2];
        case 3: return v[3];
        case 4: return v[4];
        case 5: return v[5];
        case 6: return v[6];
        case 7: return v[7];
        case 8: return v[8];
        case 9: return v[9];
        case 10: return v[10];
        case 11: return v[11];
        case 12: return v[12];
        case 13: return v[13];
        case 14: return v[14];
        default: return v[15];
    }
}

__global__ void __launch_bounds__(kFilterWgRows) filter_mask_kernel(FilterArgs a) {
    // dynamic LDS of filter_lds_bytes(n_clauses, n_preds): the clauses, the counts, the offsets
    extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
    FilterClause* const s_cl = reinterpret_cast<FilterClause*>(s_mem);
    unsigned long long* const s_cnt = reinterpret_cast<unsigned long long*>(s_mem + filter_lds_counts(a.n_clauses));
    int32_t* const s_off = reinterpret_cast<int32_t*>(s_mem + filter_lds_offsets(a.n_clauses, a.n_preds));
    const int tid = threadIdx.x;
    for (int i = tid; i < a.n_clauses; i += kFilterWgRows) s_cl[i] = a.clauses[i];
    for (int i = tid; i <= a.n_preds; i += kFilterWgRows) s_off[i] = a.offsets[i];
    for (int i = tid; i < a.n_preds; i += kFilterWgRows) s_cnt[i] = 0ull;
    __syncthreads();

    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t n_words = a.n_words;
    const int64_t n_pairs = filter_n_pairs(n_words);
    const int64_t n_wgs = gridDim.x;
    const int64_t trips = filter_trips(n_pairs, n_wgs);
    constexpr int kBlocks = kFilterMaxPreds / 64;
    unsigned long long cnt[kBlocks] = {0ull, 0ull, 0ull, 0ull};

    for (int64_t trip = 0; trip < trips; ++trip) {
        const int64_t pair = filter_wave_pair(trip, n_wgs, blockIdx.x, wave);
        if (pair >= n_pairs) break;  // (wave-uniform; later trips are further still)
        const int64_t row = filter_lane_row(pair, lane);
        const bool live = filter_row_live(row, a.N);
        const bool high = filter_has_high(pair, n_words);
        double v[kFilterSlots];
#pragma unroll
        for (int s = 0; s < kFilterSlots; ++s)
            v[s] = (live && ((a.used >> s) & 1u)) ? a.cols[s][row] : __builtin_nan("");
#pragma unroll
        for (int pb = 0; pb < kBlocks; ++pb) {
            const int p0 = pb * 64;
            if (p0 < a.n_preds) {
                const int pe = a.n_preds - p0 < 64 ? a.n_preds - p0 : 64;
                uint32_t my_lo = 0u, my_hi = 0u;
                for (int j = 0; j < pe; ++j) {
                    const int c0 = s_off[p0 + j], c1 = s_off[p0 + j + 1];
                    bool pass = live;
                    for (int c = c0; c < c1; ++c) {
                        const FilterClause cl = s_cl[c];
                        const int col = __builtin_amdgcn_readfirstlane(cl.column);
                        pass = pass && clause_passes(pick_value(v, col), cl);
                    }
                    const unsigned long long b = __ballot(pass);
                    if (lane == j) {
                        my_lo = (uint32_t)b;
                        my_hi = (uint32_t)(b >> 32);
                    }
                }
                if (lane < pe) {
                    const size_t w = (size_t)(p0 + lane) * (size_t)n_words + (size_t)pair * 2;
                    if (a.base) {
                        my_lo &= a.base[w];
                        if (high) my_hi &= a.base[w + 1];
                    }
                    a.out[w] = my_lo;
                    if (high)
                        a.out[w + 1] = my_hi;
                    else
                        my_hi = 0u;
                    cnt[pb] += (unsigned long long)(__popc(my_lo) + __popc(my_hi));
                }
            }
        }
    }
    if (!a.counts) return;  // (uniform over the launch)
#pragma unroll
    for (int pb = 0; pb < kBlocks; ++pb)
        if (pb * 64 + lane < a.n_preds && cnt[pb]) atomicAdd(&s_cnt[pb * 64 + lane], cnt[pb]);
    __syncthreads();
    for (int i = tid; i < a.n_preds; i += kFilterWgRows)
        if (s_cnt[i]) atomicAdd(a.counts + i, s_cnt[i]);
}

}  // namespace

hipError_t launch_filter_mask(const FilterArgs& a, int n_cu, hipStream_t st) {
    if (a.n_preds <= 0 || a.N <= 0) return hipSuccess;
    if (a.n_preds > kFilterMaxPreds || a.n_clauses < 0 || a.n_clauses > kFilterMaxTotal || !a.offsets || !a.out ||
        (a.n_clauses > 0 && !a.clauses) || a.n_words != filter_n_words(a.N))
        return hipErrorInvalidValue;
    for (int s = 0; s < kFilterSlots; ++s)
        if (((a.used >> s) & 1u) && !a.cols[s]) return hipErrorInvalidValue;
    const int64_t n_wgs = filter_n_wgs(filter_n_pairs(a.n_words), n_cu);
    const size_t lds = (size_t)filter_lds_bytes(a.n_clauses, a.n_preds);
    hipLaunchKernelGGL(filter_mask_kernel, dim3((unsigned)n_wgs), dim3(kFilterWgRows), lds, st, a);
    return hipGetLastError();
}

}  // namespace vdb
