// vdb_group.hip: grouped search (vdb_index_search_groups), part of the gfx950 kernels of the
// brute-force distance + top-k path (pipeline overview: vdb_scan.hip).  Built with
// -ffp-contract=off.
//
// Every row carries an int32 group id (negative: no group, not eligible); a query gets its k best
// distinct groups, each with its best row, ranked by (best key desc, best row asc) on the canonical
// fp64 keys (vdb_exact_keys.h).  Three steps, all queued on one stream:
//   1. the ordinary certified search fetches the best k' >= k eligible rows with their keys;
//   2. group_select_kernel, one workgroup per query, marks each group's first occurrence in that
//      list (already in (key desc, row asc) order: a first occurrence is the group's best row),
//      compacts them and writes the first k.  A list with k groups, or a short list (every eligible
//      row seen), settles the query; else the query is flagged on the device;
//   3. group_exact_kernel, launched for the whole batch, whose workgroups return at once for
//      unflagged queries: the shape of the exact scan (grid (segments, queries), 4 waves, one wave
//      per row over the row-major fp32 copy), keys streamed through GroupTopK, the workgroup that
//      finishes a query last merges the segments' lists and writes the slots.
#include "vdb_common.h"
#include "vdb_internal.h"
#include "vdb_exact_keys.h"
#include "vdb_group_plan.h"

namespace vdb {

// ---- the group column's bitmap ------------------------------------------------------------------------
// bit r of word r / 32 = row r < n has a group (id >= 0); words up to n_words are written whole;
// *n_valid += the rows that have one.
__global__ void __launch_bounds__(256) group_valid_kernel(const int32_t* __restrict__ groups, int64_t n,
                                                          uint32_t* __restrict__ bitmap, int64_t n_words,
                                                          unsigned long long* __restrict__ n_valid) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in = r < n;
    const bool has = in && groups[r] >= 0;
    const unsigned long long m = __ballot(has);
    const int64_t w = r >> 5;
    if ((lane & 31) == 0 && w < n_words) bitmap[w] = (uint32_t)(m >> (lane & 32));
    if (lane == 0 && m) atomicAdd(n_valid, (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(256) group_and_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                        uint32_t* __restrict__ out, int64_t n_words,
                                                        unsigned long long* __restrict__ n_set) {
    const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t v = w < n_words ? a[w] & b[w] : 0u;
    if (w < n_words) out[w] = v;
    // the bits set, summed over the wave first: one atomic per wave
    int c = __popc(v);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(n_set, (unsigned long long)c);
}

hipError_t launch_group_valid(const int32_t* groups, int64_t n, uint32_t* bitmap, int64_t n_words,
                              unsigned long long* n_valid, hipStream_t st) {
    if (n_words <= 0) return hipSuccess;
    const int64_t blocks = (n_words * 32 + 255) / 256;
    hipLaunchKernelGGL(group_valid_kernel, dim3((unsigned)blocks), dim3(256), 0, st, groups, n, bitmap, n_words, n_valid);
    return hipGetLastError();
}

hipError_t launch_group_and(const uint32_t* a, const uint32_t* b, uint32_t* out, int64_t n_words,
                            unsigned long long* n_set, hipStream_t st) {
    if (n_words <= 0) return hipSuccess;
    hipLaunchKernelGGL(group_and_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, st, a, b, out, n_words, n_set);
    return hipGetLastError();
}

// ---- step 2: select -----------------------------------------------------------------------------------
__device__ __forceinline__ void write_group_slot(int metric, double key, uint64_t row_plus_off, int32_t g, bool valid,
                                                 float* os, int64_t* oi, int32_t* og, double* ok) {
    write_result(metric, key, row_plus_off, valid, os, oi, ok);
    *og = valid ? g : -1;
}

__global__ void __launch_bounds__(256) group_select_kernel(GroupSelectArgs a) {
    __shared__ int32_t sg[256];
    __shared__ unsigned char sf[256];
    const int b = blockIdx.x;
    const int j = threadIdx.x;
    if (a.force) {  // every query takes the exact fallback
        if (j == 0) {
            a.need[b] = 1;
            atomicAdd(a.fallback_total, 1ull);
        }
        return;
    }
    const int kf = a.k_fetch;
    const size_t fo = (size_t)b * kf + j;
    const int64_t row = j < kf ? a.fi[fo] : (int64_t)-1;
    const bool valid = row >= 0 && row < a.count;
    const int32_t g = valid ? a.groups[row] : -1;
    sg[j] = g;
    const int n_valid = __syncthreads_count(valid);
    const bool first = j < kf && group_first_occurrence(sg, j);
    sf[j] = first ? 1 : 0;
    const int n_first = __syncthreads_count(first);
    const int64_t eligible = a.eligible_dev ? (int64_t)*a.eligible_dev : a.eligible;
    if (!group_complete(n_first, n_valid, a.k, kf, eligible)) {
        if (j == 0) {
            a.need[b] = 1;
            atomicAdd(a.fallback_total, 1ull);
        }
        return;
    }
    if (j == 0) a.need[b] = 0;
    int rank = 0;
    for (int i = 0; i < j; ++i) rank += sf[i];
    if (first && rank < a.k) {
        const size_t o = (size_t)b * a.k + rank;
        a.out_s[o] = a.fs[fo];
        a.out_i[o] = row + a.index_offset;
        a.out_g[o] = g;
        if (a.out_k) a.out_k[o] = a.fk[fo];
    }
    if (j >= n_first && j < a.k) {
        const size_t o = (size_t)b * a.k + j;
        write_group_slot(0, -INFINITY, 0, -1, false, a.out_s + o, a.out_i + o, a.out_g + o, a.out_k ? a.out_k + o : nullptr);
    }
}

hipError_t launch_group_select(const GroupSelectArgs& a, int n_queries, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (a.k < 1 || a.k > kGroupMaxK || a.k_fetch < a.k || a.k_fetch > 256) return hipErrorInvalidValue;
    hipLaunchKernelGGL(group_select_kernel, dim3(n_queries), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- step 3: the exact fallback -------------------------------------------------------------------------
// Bitonic sort, best first by (key desc, row asc), of n (a power of two) LDS entries of one wave, the
// group ids carried along (wave_lds_sort_desc with a third array).
__device__ __attribute__((noinline)) void group_lds_sort_desc(double* k, uint32_t* r, int32_t* g, int n) {
    const int lane = threadIdx.x & 63;
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = lane; e < (n >> 1); e += 64) {
                const int lo = 2 * stride * (e / stride) + (e % stride);
                const int hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const double ka = k[lo], kb = k[hi];
                const uint32_t ra = r[lo], rb = r[hi];
                const bool sw = desc ? better(kb, rb, ka, ra) : better(ka, ra, kb, rb);
                if (sw) {
                    const int32_t ga = g[lo], gb = g[hi];
                    k[lo] = kb; k[hi] = ka;
                    r[lo] = rb; r[hi] = ra;
                    g[lo] = gb; g[hi] = ga;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// Streaming "best row of each of the k best groups" for ONE wave, the group-aware form of WaveTopK:
// the LDS buffer holds (key, row, group); a candidate that beats the threshold is appended; a full
// buffer is sorted by (key desc, row asc), every entry that is not the first of its group is dropped,
// the rest is cut to k groups, and the threshold becomes the k-th group's (key, row).  A row at or
// below the threshold is the best row of no group among the best k: k groups already have a better
// one.  The same step folds lists of disjoint row sets (the answer merges).
struct GroupTopK {
    static constexpr int kMaxCap = 256;  // group_topk_cap(kGroupMaxK)
    double* bk;
    uint32_t* br;
    int32_t* bg;
    int K, cap, cnt;
    double tk;
    uint32_t tr;
    __device__ void init(double* k, uint32_t* r, int32_t* g, int kk) {
        bk = k; br = r; bg = g; K = kk; cap = group_topk_cap(kk); cnt = 0;
        tk = -INFINITY; tr = 0xFFFFFFFFu;
    }
    __device__ void compact() {
        const int lane = threadIdx.x & 63;
        for (int e = cnt + lane; e < cap; e += 64) {
            bk[e] = -INFINITY;
            br[e] = 0xFFFFFFFFu;
            bg[e] = -1;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        group_lds_sort_desc(bk, br, bg, cap);
        // first occurrences of the cnt sorted entries (the padding, group -1, is none)
        bool f[kMaxCap / 64];
#pragma unroll
        for (int i = 0; i < kMaxCap / 64; ++i) {
            const int e = i * 64 + lane;
            f[i] = e < cnt && group_first_occurrence(bg, e);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // ... moved to the front in order: chunk i's entries are read by every lane before any is
        // written, and land at or below their own position
        int out = 0;
#pragma unroll
        for (int i = 0; i < kMaxCap / 64; ++i) {
            if (i * 64 < cap) {
                const int e = i * 64 + lane;
                const double key = bk[e];
                const uint32_t row = br[e];
                const int32_t g = bg[e];
                const unsigned long long m = __ballot(f[i]);
                const int pos = out + __popcll(m & ((1ull << lane) - 1ull));
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (f[i] && pos < K) {
                    bk[pos] = key;
                    br[pos] = row;
                    bg[pos] = g;
                }
                out += __popcll(m);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }
        cnt = out < K ? out : K;
        if (cnt == K) {
            tk = bk[K - 1];
            tr = br[K - 1];
        }
    }
    __device__ void offer(bool valid, double key, uint32_t row, int32_t g) {
        const int lane = threadIdx.x & 63;
        bool pass = valid && better(key, row, tk, tr);
        unsigned long long m = __ballot(pass);
        if (m == 0) return;
        if (cnt + __popcll(m) > cap) {
            compact();
            pass = valid && better(key, row, tk, tr);
            m = __ballot(pass);
        }
        const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
        if (pass) {
            bk[pos] = key;
            br[pos] = row;
            bg[pos] = g;
        }
        cnt += __popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    }
    // afterwards entries [0, cnt) are the result, best group first
    __device__ void finish() { compact(); }
};

size_t group_exact_lds_bytes(int k) {
    return (size_t)kGroupWaves * group_topk_cap(k) * (sizeof(double) + sizeof(uint32_t) + sizeof(int32_t)) +
           kGroupWaves * sizeof(int);
}

// MP: 4 / 8 = rows of up to 256 MP dims with every piece of a batch in flight; 0 = any length, one
// row at a time.
template <int METRIC, int MP>
__global__ void __launch_bounds__(256) group_exact_kernel(GroupExactArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NB = kGroupNB;
    const int b = blockIdx.y;
    if (!a.need[b]) return;  // settled by the select: nothing to do
    const int s = blockIdx.x;
    const int n_seg = (int)gridDim.x;
    const int live = group_live_segs(a.N, n_seg);
    if (s >= live) return;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int K = a.k;
    const int cap = group_topk_cap(K);
    double* kbase = reinterpret_cast<double*>(smem);
    uint32_t* rbase = reinterpret_cast<uint32_t*>(smem + (size_t)kGroupWaves * cap * sizeof(double));
    int32_t* gbase = reinterpret_cast<int32_t*>(smem + (size_t)kGroupWaves * cap * (sizeof(double) + sizeof(uint32_t)));
    int* wcnt = reinterpret_cast<int*>(smem + (size_t)kGroupWaves * cap * (sizeof(double) + 2 * sizeof(uint32_t)));
    GroupTopK tk;
    tk.init(kbase + (size_t)wv * cap, rbase + (size_t)wv * cap, gbase + (size_t)wv * cap, K);

    const float* q = a.Q + (int64_t)b * a.D;
    const double qn = a.qn64[b];
    const int np = (a.D + 255) / 256;
    const GroupRange rg = group_seg_range(a.N, n_seg, s);
    for (int64_t base = rg.r0 + (int64_t)wv * NB; base < rg.r1; base += (int64_t)kGroupWaves * NB) {
        // the NB rows of a trip share a mask word (base is a multiple of NB, NB divides 32); a row is
        // read only when its mask bit is set and it has a group
        const uint32_t word = a.mask ? a.mask[base >> 5] >> (base & 31) : 0xFFFFFFFFu;
        if ((word & ((1u << NB) - 1u)) == 0) continue;
        uint32_t rws[NB];
        int32_t gs[NB];
        double xn[NB];
        bool ok[NB];
        bool any = false;
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int64_t r = base + u;
            ok[u] = r < rg.r1 && ((word >> u) & 1u);
            rws[u] = ok[u] ? (uint32_t)r : 0u;
            gs[u] = ok[u] ? a.groups[r] : -1;
            ok[u] = ok[u] && gs[u] >= 0;
            xn[u] = (METRIC == 0 && ok[u]) ? a.nrm64[rws[u]] : 1.0;
            any = any || ok[u];
        }
        if (!any) continue;
        double keys[NB];
        if constexpr (MP > 0) {
            f32x4 xv[MP][NB];
            rows_pieces_load<NB, MP>(a.X, a.G, np, rws, ok, xv);
            exact_keys_held<METRIC, NB, MP>(q, a.D, qn, np, xv, xn, keys);
        } else {
#pragma unroll
            for (int u = 0; u < NB; ++u)
                keys[u] = ok[u] ? exact_key<METRIC>(q, qn, a.X, a.G, a.D, rws[u], xn[u]) : -INFINITY;
        }
        // lane u < NB offers row u of the trip
        double key = -INFINITY;
        uint32_t row = 0xFFFFFFFFu;
        int32_t g = -1;
        bool valid = false;
#pragma unroll
        for (int u = 0; u < NB; ++u)
            if (lane == u) {
                valid = ok[u];
                key = ok[u] ? keys[u] : -INFINITY;
                row = rws[u];
                g = gs[u];
            }
        tk.offer(valid, key, row, g);
    }
    tk.finish();
    if (lane == 0) wcnt[wv] = tk.cnt;
    __syncthreads();
    if (wv == 0) {  // fold the four waves' lists: disjoint rows, the same step
        for (int w = 1; w < kGroupWaves; ++w) {
            const int n = wcnt[w];
            for (int e0 = 0; e0 < n; e0 += 64) {
                const int e = e0 + lane;
                const bool in = e < n;
                tk.offer(in, in ? kbase[(size_t)w * cap + e] : -INFINITY, in ? rbase[(size_t)w * cap + e] : 0xFFFFFFFFu,
                         in ? gbase[(size_t)w * cap + e] : -1);
            }
        }
        tk.finish();
        if (live > 1) {
            const size_t base = ((size_t)b * n_seg + s) * K;
            for (int e = lane; e < K; e += 64) {
                const bool in = e < tk.cnt;
                a.lk[base + e] = in ? tk.bk[e] : -INFINITY;
                a.lr[base + e] = in ? tk.br[e] : 0xFFFFFFFFu;
                a.lg[base + e] = in ? tk.bg[e] : -1;
            }
        }
    }
    if (live > 1) {
        // the last workgroup of this query merges its `live` lists (release: wave 0's list stores
        // before the count; acquire: the other lists after it)
        __shared__ int s_last;
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            s_last = atomicAdd(a.done + b, 1) == live - 1;
        }
        __syncthreads();
        if (!s_last) return;
        __threadfence();
        if (wv != 0) return;
        tk.init(kbase, rbase, gbase, K);
        for (int sg = 0; sg < live; ++sg) {
            const size_t base = ((size_t)b * n_seg + sg) * K;
            for (int e0 = 0; e0 < K; e0 += 64) {
                const int e = e0 + lane;
                const uint32_t r = e < K ? a.lr[base + e] : 0xFFFFFFFFu;
                const bool in = r != 0xFFFFFFFFu;
                tk.offer(in, in ? a.lk[base + e] : -INFINITY, r, in ? a.lg[base + e] : -1);
            }
        }
        tk.finish();
        if (lane == 0) a.done[b] = 0;  // left zero for the next call on this workspace
    }
    if (wv != 0) return;
    for (int e = lane; e < K; e += 64) {
        const bool valid = e < tk.cnt;
        const size_t o = (size_t)b * K + e;
        write_group_slot(METRIC, valid ? tk.bk[e] : -INFINITY, valid ? (uint64_t)tk.br[e] + (uint64_t)a.index_offset : 0,
                         valid ? tk.bg[e] : -1, valid, a.out_s + o, a.out_i + o, a.out_g + o,
                         a.out_k ? a.out_k + o : nullptr);
    }
}

hipError_t launch_group_exact(int metric, const GroupExactArgs& a, int n_queries, int n_seg, hipStream_t st) {
    if (n_queries <= 0) return hipSuccess;
    if (n_queries > kGroupMaxQueries || n_seg < 1 || n_seg > kGroupMaxSeg || a.k < 1 || a.k > kGroupMaxK || a.N <= 0 ||
        (n_seg > 1 && (!a.lk || !a.lr || !a.lg || !a.done)))
        return hipErrorInvalidValue;
    const size_t lds = group_exact_lds_bytes(a.k);
    const dim3 grid(n_seg, n_queries);
    const int mp = a.D <= 1024 ? 4 : a.D <= 2048 ? 8 : 0;
#define VDB_GRP(M, MPV)                                                                        \
    if (metric == M && mp == MPV) {                                                            \
        hipLaunchKernelGGL((group_exact_kernel<M, MPV>), grid, dim3(256), lds, st, a);         \
        return hipGetLastError();                                                              \
    }
    VDB_GRP(0, 4) VDB_GRP(0, 8) VDB_GRP(0, 0)
    VDB_GRP(1, 4) VDB_GRP(1, 8) VDB_GRP(1, 0)
#undef VDB_GRP
    return hipErrorInvalidValue;
}

}  // namespace vdb
