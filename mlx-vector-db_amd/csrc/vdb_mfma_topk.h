// vdb_mfma_topk.h: the top-k of the integer-MFMA searches over the code column (vdb_hamming_mfma.hip,
// vdb_code_dot_mfma.hip, vdb_jaccard_mfma.hip), on the device.  Each holds, per trip and wave, four 32 x 32 i32 accumulators
// (two 32-row sub-tiles of a tile against two tiles of 32 queries) and rank rows by a 64-bit key,
// smaller is better: key = hi << 32 | row, where hi comes from an accumulator value by the one thing
// the searches differ in, the `rank` object.  rank.hi(qt, rt, v, value) is the key's upper half of the
// value in register v of the accumulator of sub-tile rt and query tile qt (the lane's query: 32 qt + lane
// % 32; the row within the sub-tile: mfma_acc_row(v)); rank.pass(qt, rt, v, value, row, th) says whether
// that entry's key is below the threshold th, and may do so without forming the key (the Jaccard search,
// vdb_jaccard_mfma.hip, whose key costs a division and depends on the row's popcount).  The Hamming and
// the code-dot search need the value alone: MfmaValueKey wraps their `key_hi(qt, value)` functor (the
// distance; the biased negated score).
//
// Each query has, in LDS, its threshold (the k-th best key so far) and one candidate buffer shared by
// the four waves.  A lane holds one query and 16 rows of an accumulator; it tests a register against
// its query's threshold, one ballot skips the register when nothing passes, and a passing entry takes
// its place in the buffer by an LDS atomic add on the query's count.  The order of the appends varies
// from run to run; the result does not: the keys of a query are distinct, the ranking is a total
// order, a compaction keeps exactly the k smallest keys of what the buffer holds, and an entry is only
// ever dropped by a test against the k-th smallest key of some subset of the rows.  Compaction (one
// wave per query): every lane ranks its two entries against the whole buffer and stores those of rank
// < k at their rank, which also sorts them.
//
// A buffer cannot be compacted by one wave while the others append, so the trips are uniform across
// the workgroup and each ends in mfma_rank_trip with a barrier and a flag word.  Bit 1: some buffer
// passed kHamMfmaHigh entries; the buffers above it are compacted.  Bit 0: an append found its buffer
// full.  Then the counts go back to their values at the trip's start, every buffer is compacted to k,
// and the four waves offer their accumulators again one after the other with a compaction between
// them; one wave's offers always fit (vdb_hamming_plan.h).
#pragma once
#include "vdb_common.h"
#include "vdb_hamming_plan.h"

namespace vdb {

typedef int ham_i32x4 __attribute__((ext_vector_type(4)));
typedef int ham_i32x16 __attribute__((ext_vector_type(16)));

constexpr int QT = kHamMfmaQT;
constexpr int QB = kHamMfmaQB;
constexpr int RT = kHamTileRows / 32;  // sub-tiles of a tile
constexpr int CAP = kHamMfmaCap;
static_assert(CAP == 128, "a lane ranks two entries of a buffer");
constexpr uint64_t kNoKey = ~0ull;

// 16 bits of a word from bit `sh` up as one MFMA operand: bit i to byte i.
__device__ __forceinline__ ham_i32x4 expand_row16(uint64_t x, int sh) {
    ham_i32x4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d) r[d] = (int)ham_mfma_row4((uint32_t)(x >> (sh + 4 * d)));
    return r;
}

// The accumulator layout: the row, within its sub-tile of 32, of register v of a lane.
__device__ __forceinline__ int mfma_acc_row(int v) { return 8 * (v >> 2) + 4 * (int)((threadIdx.x & 63) >> 5) + (v & 3); }

// A key that is a function of the accumulator value (and the query tile) alone.
template <class KeyHi>
struct MfmaValueKey {
    KeyHi key_hi;
    __device__ __forceinline__ uint32_t hi(int qt, int, int, int value) const { return key_hi(qt, value); }
    __device__ __forceinline__ bool pass(int qt, int, int, int value, uint32_t row, uint64_t th) const {
        return (((uint64_t)key_hi(qt, value) << 32) | row) < th;
    }
};
template <class KeyHi>
__device__ __forceinline__ MfmaValueKey<KeyHi> mfma_value_key(KeyHi key_hi) { return MfmaValueKey<KeyHi>{key_hi}; }

// A wave offers its tile's accumulators.  vm[rt]: the candidate rows of sub-tile rt as bits;
// rank: the key of an entry (the header comment).  Returns the flag bits of the header comment.
template <class Rank>
__device__ __forceinline__ int mfma_offer(const ham_i32x16 (&acc)[RT][QT], const uint32_t (&vm)[RT], int64_t t, const Rank& rank,
                                          int nq, int k_high, uint64_t* cand, const uint64_t* thr, int* cnt) {
    const int lane = threadIdx.x & 63;
    const int col = lane & 31;
    int flag = 0;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        if (vm[rt] == 0) continue;  // (wave-uniform) a sub-tile with no candidate row
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            if (32 * qt >= nq) continue;  // (uniform) a query tile with no query
            const int q = 32 * qt + col;
            const uint64_t th = q < nq ? thr[q] : 0ull;  // an absent query passes nothing
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int rl = mfma_acc_row(v);
                const uint32_t row = (uint32_t)(t * kHamTileRows + 32 * rt + rl);
                const int value = acc[rt][qt][v];
                const bool pass = ((vm[rt] >> rl) & 1u) && rank.pass(qt, rt, v, value, row, th);
                if (__ballot(pass) == 0ull) continue;
                if (pass) {
                    const uint64_t key = ((uint64_t)rank.hi(qt, rt, v, value) << 32) | row;
                    const int pos = atomicAdd(&cnt[q], 1);
                    if (pos < CAP) {
                        cand[(size_t)q * CAP + pos] = key;
                        if (pos >= k_high) flag |= 2;
                    } else {
                        flag |= 1;
                    }
                }
            }
        }
    }
    return flag;
}

__device__ __forceinline__ uint64_t lane_key(uint64_t v, int src /* wave-uniform */) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// One wave compacts query q's buffer: the k smallest keys, sorted, and the threshold once there are k.
__device__ __forceinline__ void mfma_compact(int q, int k, uint64_t* cand, uint64_t* thr, int* cnt) {
    const int lane = threadIdx.x & 63;
    uint64_t* b = cand + (size_t)q * CAP;
    const int c = __builtin_amdgcn_readfirstlane(cnt[q]);
    const uint64_t m0 = lane < c ? b[lane] : kNoKey;
    const uint64_t m1 = lane + 64 < c ? b[lane + 64] : kNoKey;
    // entry j comes out of lane j % 64's register (a lane read with a uniform index): no LDS round
    // trip per entry
    int r0 = 0, r1 = 0;
    for (int j = 0; j < (c < 64 ? c : 64); ++j) {
        const uint64_t kj = lane_key(m0, j);
        r0 += kj < m0;
        r1 += kj < m1;
    }
    for (int j = 64; j < c; ++j) {
        const uint64_t kj = lane_key(m1, j - 64);
        r0 += kj < m0;
        r1 += kj < m1;
    }
    // every read above is complete before the stores below (LDS accesses of a wave complete in order)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < c && r0 < k) b[r0] = m0;
    if (lane + 64 < c && r1 < k) b[r1] = m1;
    if (c >= k) {
        if (lane < c && r0 == k - 1) thr[q] = m0;
        if (lane + 64 < c && r1 == k - 1) thr[q] = m1;
    }
    if (lane == 0) cnt[q] = c < k ? c : k;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// Wave wv compacts queries wv, wv + 4, ... whose buffers hold more than `above` entries.
__device__ __forceinline__ void mfma_compact_all(int above, int nq, int k, uint64_t* cand, uint64_t* thr, int* cnt) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int q = wv; q < nq; q += kHamWaves)
        if (cnt[q] > above) mfma_compact(q, k, cand, thr, cnt);
}

// The end of a trip, reached by all four waves: the accumulators of the waves that have a tile go to
// the buffers.  Round 0: every wave offers its tile; rounds 1..4, after a full buffer only: wave r - 1
// alone.  (The first trip starts at round 1: without thresholds every row passes and round 0 would
// only find the buffers full.)  s_flag: two words of LDS, zero before the first trip; cnt0: thread q <
// QB's copy of query q's count at the trip's start, kept up to date here.
template <class Rank>
__device__ __forceinline__ void mfma_rank_trip(const ham_i32x16 (&acc)[RT][QT], const uint32_t (&vm)[RT], int64_t t,
                                               const Rank& rank, int nq, int k, int trip, int* s_flag, int& cnt0, uint64_t* cand,
                                               uint64_t* thr, int* cnt) {
    const int wv = threadIdx.x >> 6;
    const bool has_tile = (vm[0] | vm[1]) != 0u;
    for (int r = trip == 0 ? 1 : 0; r <= kHamWaves; ++r) {
        if (has_tile && (r == 0 || wv == r - 1)) {
            const int flag = mfma_offer(acc, vm, t, rank, nq, kHamMfmaHigh, cand, thr, cnt);
            if (r == 0 && flag) atomicOr(&s_flag[trip & 1], flag);
        }
        __syncthreads();  // the round's appends are made
        if (r == 0) {
            const int f = s_flag[trip & 1];
            if (threadIdx.x == 0) s_flag[(trip + 1) & 1] = 0;  // (last read a trip ago, next set after this trip's last barrier)
            if (!(f & 1)) {
                if (f & 2) {
                    mfma_compact_all(kHamMfmaHigh, nq, k, cand, thr, cnt);
                    __syncthreads();
                }
                break;
            }
            // a full buffer: back to the trip's start and compact, then one wave's offers at a time
            if (threadIdx.x < QB) cnt[threadIdx.x] = cnt0;
            __syncthreads();
        }
        mfma_compact_all(k, nq, k, cand, thr, cnt);
        __syncthreads();
    }
    if (threadIdx.x < QB) cnt0 = cnt[threadIdx.x];
    __syncthreads();  // the counts are read before the next trip's appends
}

}  // namespace vdb
