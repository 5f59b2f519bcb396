// vdb_exact.hip: exact fp64 keys: candidate rerank + certificate, exact full scan — part of the gfx950 kernels of the brute-force distance + top-k path
// (pipeline overview: vdb_scan.hip).  Built with -ffp-contract=off.
#include "vdb_common.h"
#include "vdb_internal.h"
#include <type_traits>
#include "vdb_merge_block.h"
#include "vdb_exact_keys.h"  // exact_key, exact_keys_rows, exact_keys_batch

namespace vdb {

// Rerank: exact keys of the KP candidates (16 waves, one candidate per wave at a
// time), best k out, and the certificate that the exact top-k lies inside the
// candidate set:
//   every non-candidate row r has approx a_r <= a_KP (scan invariant), and
//   |approx - exact| <= eps, so if a_KP + eps < a_k - eps no non-candidate can
//   reach the top k.  A failed certificate queues the query for exact_scan.
constexpr int RERANK_WAVES = 16;

// Same keys (same canonical order) with the query pieces in registers and every
// row piece of NB rows requested before the first FMA: one dependent round trip
// per batch instead of np of them (D <= 256 MP).
// In three steps, so that the finish requests a batch's pieces (exact_rows_load) before the batch
// ahead of it is reduced: the pieces, the per-lane sums (exact_rows_sum), the butterfly and the keys
// (exact_rows_keys).
template <int NB, int MP>
__device__ __forceinline__ void exact_rows_load(const float* __restrict__ X, int G, int np, const uint32_t* rows,
                                                int nb, f32x4 (&xv)[MP][NB]) {
    const int lane = threadIdx.x & 63;
    const int Dp = G * GROUP_DIMS;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        const int p = m * 64 + lane;
#pragma unroll
        for (int u = 0; u < NB; ++u)
            xv[m][u] = (m < np && u < nb && 4 * p < Dp) ? *(const f32x4*)(X + row_piece_offset(rows[u], p, G))
                                                       : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
template <int METRIC, int NB, int MP>
__device__ __forceinline__ void exact_rows_sum(const float (&qv)[MP][4], const f32x4 (&xv)[MP][NB], int np,
                                               double (&acc)[NB]) {
#pragma unroll
    for (int u = 0; u < NB; ++u) acc[u] = 0.0;
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        if (m < np) {
#pragma unroll
            for (int u = 0; u < NB; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double qd = (double)qv[m][j];
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
}
// (the same sums, in the order of exact_keys_rows of vdb_exact_keys.h, with the query's pieces read
// from memory -- L1-resident -- per batch instead of held across batches: the 8-wave form's rows)
template <int METRIC, int NB, int MP>
__device__ __forceinline__ void exact_rows_sum_mem(const float* __restrict__ q, int D, const f32x4 (&xv)[MP][NB],
                                                   int np, double (&acc)[NB]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int u = 0; u < NB; ++u) acc[u] = 0.0;
    // every piece's loads first and unconditional, an element past the row's end reading the
    // row's last: behind a predicate each was a load and a wait of its own, 32 dependent (L1)
    // trips a batch at C3
    float qa[MP][4];
#pragma unroll
    for (int m = 0; m < MP; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int d = 4 * (m * 64 + lane) + j;
            const float v = q[min(d, D - 1)];
            qa[m][j] = d < D ? v : 0.0f;
        }
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        if (m < np) {
            const float (&qv)[4] = qa[m];
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
}
template <int METRIC, int NB>
__device__ __forceinline__ void exact_rows_keys(double (&acc)[NB], double qn, const double* xn, int nb, double* out) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int u = 0; u < NB; ++u) acc[u] = acc[u] + __shfl_xor(acc[u], off, 64);
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        if (u < nb) out[u] = METRIC == 0 ? acc[u] / (fmax(qn, 1e-8) * fmax(xn[u], 1e-8)) : -acc[u];
    }
}

// (for longer rows: exact_keys_rows, vdb_exact_keys.h)

// waves of the finish's one workgroup per query (1024 threads: 128 VGPRs each)
// 16 (1024 threads, 128 VGPRs, a few spills) measured faster than 8 (512 threads, no spills) on
// every config, same box, bench's 3 streams: C2 370K vs 364K QPS, C6 261K vs 255K, C3 365K vs
// 360K (profiles/r04_ab/mx2; the 8-wave build define stays for A/B)
#ifndef VDB_FIN_WAVES
#define VDB_FIN_WAVES 16
#endif
constexpr int FIN_MP = 4;   // fast path: D <= 1024
constexpr int FIN_NB4 = VDB_FIN_WAVES > 8 ? 3 : 6;  // rows per wave per batch on the fast path (4 spills at 128 VGPRs)
// D <= 2048 (C3: 1536): 1 row per wave per batch, all 8 of its pieces in flight (8 KiB
// of row pieces in flight per wave; the loop form below keeps one 1 KiB piece per row in flight
// and ran C3's exact keys at 150 us for 256 candidates x 256 queries, profiles/r04 fin stamps)
constexpr int FIN_MP8 = 8;
// (2 rows: C3 p50 0.522 -> 0.516 ms, QPS +0.3% now that its finish never runs beside the long-row
// wide scan, profiles/r06_nb2; 175 VGPRs, no spills; round 5 had measured 1 better beside scan8)
#ifndef VDB_FIN_NB8
#define VDB_FIN_NB8 2
#endif
constexpr int FIN_NB8 = VDB_FIN_NB8;

template <int METRIC, int KP>
__global__ void __launch_bounds__(64 * RERANK_WAVES) rerank_kernel(RerankArgs a) {
    constexpr int E = KP >= 64 ? KP / 64 : 1;
    __shared__ double s_k[KP];
    __shared__ uint32_t s_i[KP];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const float* q = a.Q + (int64_t)b * a.D;
    const double qn = a.qn64[b];
    for (int c = wv; c < KP; c += RERANK_WAVES) {
        const uint32_t r = a.app_i[(size_t)b * KP + c];
        double key = -INFINITY;
        if (r != 0xFFFFFFFFu) key = exact_key<METRIC>(q, qn, a.X, a.G, a.D, r, a.nrm64[r]);
        if (lane == 0) {
            s_k[c] = key;
            s_i[c] = r;
        }
    }
    __syncthreads();
    if (wv != 0) return;
    double kv[E];
    uint32_t iv[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = i * 64 + lane;
        kv[i] = e < KP ? s_k[e] : -INFINITY;
        iv[i] = e < KP ? s_i[e] : 0xFFFFFFFFu;
    }
    wave_sort_desc<double, uint32_t, E>(kv, iv);
#pragma unroll
    for (int i = 0; i < E; ++i) {
        const int e = i * 64 + lane;
        if (e < a.k) {
            const size_t o = (size_t)b * a.k + e;
            write_result(METRIC, kv[i], (uint64_t)iv[i] + a.index_offset, iv[i] != 0xFFFFFFFFu, a.out_s + o,
                         a.out_i + o, a.out_k ? a.out_k + o : nullptr);
        }
    }
    if (lane == 0) {
        // Rows never in a candidate list scored (approx) <= max(a_KP, T): a_KP for rows a
        // workgroup dropped against its own KP-th best (the merged KP-th is >= it), T (the
        // final shared bound; every bound used during the scan was <= it) for rows dropped
        // against the shared bound.  Empty list tail and no bound = fewer eligible rows.
        const bool full = a.app_i[(size_t)b * KP + KP - 1] != 0xFFFFFFFFu;
        const double T = a.gthr ? (double)key_to_float(a.gthr[b]) : -INFINITY;
        bool ok = true;
        if (full || T > -INFINITY) {
            const bool have_k = a.app_i[(size_t)b * KP + a.k - 1] != 0xFFFFFFFFu;
            const double ak = have_k ? (double)a.app_s[(size_t)b * KP + a.k - 1] : -INFINITY;
            const double akp = full ? (double)a.app_s[(size_t)b * KP + KP - 1] : -INFINITY;
            const double acut = fmax(akp, T);
            double eps;
            if (METRIC == 0) {
                eps = a.eps_rel;
            } else {
                eps = a.eps_rel * (2.0 * qn * a.xmax + a.xmax * a.xmax) + 2.4e-7 * fmax(fabs(ak), fabs(acut));
            }
            ok = have_k && acut + eps < ak - eps;
        }
        if (!ok) {
            const int pos = atomicAdd(a.flag_count, 1);
            a.flag_list[pos] = b;
        }
    }
}

hipError_t launch_rerank(int metric, int KP, const RerankArgs& a, int B, hipStream_t st) {
#define VDB_RR(M, KPV)                                                                       \
    if (metric == M && KP == KPV) {                                                          \
        hipLaunchKernelGGL((rerank_kernel<M, KPV>), dim3(B), dim3(64 * RERANK_WAVES), 0, st, a);           \
        return hipGetLastError();                                                            \
    }
    VDB_RR(0, 32) VDB_RR(0, 64) VDB_RR(0, 128) VDB_RR(0, 256)
    VDB_RR(1, 32) VDB_RR(1, 64) VDB_RR(1, 128) VDB_RR(1, 256)
#undef VDB_RR
    return hipErrorInvalidValue;
}

// =============================================================================
// finish: select + exact rerank + certificate, one workgroup per query
// =============================================================================
// Input: the query's global candidate list (entries the candidate pass appended
// above its shared bound; typically tens to a few hundred).  Entries below the final
// bound are dropped while loading; the best min(KP, n) of the rest by (approx score
// desc, row asc) come from a radix select over all waves (no sort); thread 0 checks the
// certificate on the approximate scores (a_k, a_KP by rank counting); then only the
// candidates that can still be in the exact top k (approx >= a_k - 2 eps: ~2.5 k of KP = 128
// at C2 bf16) get exact fp64 keys, all waves, batched NB candidates per wave so the corpus
// loads of a batch are in flight together; exact ranks come from counting (no sort),
// several threads per candidate.  A list longer than FIN_CAP goes to the exact scan.
#ifndef VDB_FIN_CAP
#define VDB_FIN_CAP 16384
#endif
constexpr int FIN_CAP = VDB_FIN_CAP;  // 128 KiB of (key, row) in LDS
constexpr int FIN_NB = 2;        // candidates per wave per batch
constexpr int FIN_WAVES = VDB_FIN_WAVES;

#ifdef VDB_STAMP
// Diagnostic build only: per-query phase timestamps of finish_kernel + list length.
// [0..5] phase starts / end, [6] refinement ticks | rerank set << 40, [7] list length, [8..15]
// sub-phase stamps of the certificate and the refinement (thread 0's view)
__device__ unsigned long long g_fin_stamps[8192][16];
#define FIN_STAMP(i) do { if (threadIdx.x == 0) g_fin_stamps[blockIdx.x][i] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define FIN_STAMP(i) do { } while (0)
#endif

// (rows of any length: exact_keys_batch, vdb_exact_keys.h)

// FW waves per workgroup: 16 (FIN_WAVES), or 8 for rows of more than 1024 dims (no spills at the
// 8-piece exact keys: C3 400-413 K -> 419-421 K QPS; C2 / C4 / C6 -0.5..-1% at 8, so they keep 16;
// profiles/r05_ab/ab34_finish_waves.log)
// The small form (FW = 4, CAP = FIN_CAP_SMALL: 4 waves of <= 168 VGPRs, ~51 KiB of LDS, so three
// workgroups a CU at the most: the launch bound) fits beside a
// long-row wide scan workgroup (vdb_scan8wl.hip: 8 waves of 170 VGPRs, 98 KiB of LDS at 768 dims),
// so under several streams a batch's finish runs beside the next batch's scan instead of after it;
// a list longer than CAP goes to the exact path.
constexpr int FIN_CAP_SMALL = 4096;
template <int METRIC, int KP, int FW = FIN_WAVES, int CAP = FIN_CAP>
__global__ void __launch_bounds__(64 * FW, FW <= 4 ? 3 : 1) finish_kernel(FinishArgs a) {
    constexpr int FIN_WAVES = FW;  // (shadows the default inside this kernel)
    constexpr int FIN_NB4 = FW > 8 || FW <= 4 ? 3 : 6;
    constexpr int FIN_CAP = CAP;   // (likewise)
    __shared__ uint32_t s_key[FIN_CAP];
    __shared__ uint32_t s_row[FIN_CAP];
    __shared__ __attribute__((aligned(16))) uint32_t s_ck[KP];
    __shared__ __attribute__((aligned(16))) uint32_t s_cr[KP];
    __shared__ __attribute__((aligned(16))) double s_ek[KP];
    __shared__ uint32_t s_ock[KP];  // split > 1: this workgroup's share of the candidates
    __shared__ uint32_t s_ocr[KP];
    __shared__ double s_oek[KP];
    __shared__ int s_m, s_mown, s_last;
    __shared__ uint32_t s_ak, s_akp;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int b = blockIdx.x;
    const int S = a.split, sp = blockIdx.y;  // split > 1: S workgroups per query share the rerank
    if (a.gate && b >= *a.gate) return;  // device re-pass: a slot past the gathered count
    FIN_STAMP(0);
    // Every per-query value a later phase reads is requested here, ahead of the list load, and
    // published in LDS at the barrier that ends the list load: the first thread of the last wave
    // takes the scalars (wave 0 has the checksum's words to fetch), every thread its elements of
    // the query row (the exact keys' register path) and of the rounding residual (the
    // refinement's).  Each of them was a dependent round trip of its own behind a barrier of the
    // certificate, the refinement or the exact keys; beside two scans such a trip costs several
    // times its stand-alone 2 us.  (The scalars' addresses are uniform, so they compile to
    // scalar loads that the one thread waits for at once, *chkr after the others: two short
    // trips of the last wave beside wave 0's, not under the list load.)
    // launch_finish runs the 16- and 4-wave forms for D <= 1024 alone (when the default form has
    // more than 8 waves), so they compile the register path only: 212 -> 0 bytes of scratch per
    // lane, c4 shard +1.5% (profiles/r06_nosp; the 8-wave form keeps every path: pruned, C3 -1%)
    constexpr bool kShortOnly = FW != 8 && VDB_FIN_WAVES > 8;
    // The copies are sized by the rows a form is launched with.  The query row: 1024 dims in the
    // 4- and 16-wave forms; none in the 8-wave form, whose rows (D > 1024 in the default build)
    // take exact_keys_rows, which reads the query from memory as it goes.  The residual: 1024
    // dims, or VDB_FIN_RES8 in the 8-wave form (C3: 1536; longer rows read it from memory).
#ifndef VDB_FIN_RES8
#define VDB_FIN_RES8 2048
#endif
    constexpr bool kStageQ = FW != 8;
    constexpr int QLQ = kStageQ ? 1024 : 0, QLR = FW == 8 ? VDB_FIN_RES8 : 1024;
    constexpr int NQQ = QLQ / (64 * FW), NQR = QLR / (64 * FW);
    static_assert(QLQ % (64 * FW) == 0 && QLR % (64 * FW) == 0, "whole turns of the workgroup");
    __shared__ __attribute__((aligned(16))) float s_q[QLQ > 0 ? QLQ : 4];
    __shared__ __attribute__((aligned(16))) float s_res[QLR > 0 ? QLR : 4];
    __shared__ double s_qn, s_qc[3];
    __shared__ float s_qe, s_qe2, s_qsc;
    __shared__ uint32_t s_chkr;
    const bool r_lds = QLR > 0 && a.xh_rm != nullptr && a.qres != nullptr && (kShortOnly || a.Dp <= QLR);
    float t_q[NQQ > 0 ? NQQ : 1], t_r[NQR > 0 ? NQR : 1];
#pragma unroll
    for (int i = 0; i < NQQ; ++i) {
        const int d = tid + 64 * FW * i;
        t_q[i] = d < a.D ? a.Q[(int64_t)b * a.D + d] : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < NQR; ++i) {
        const int d = tid + 64 * FW * i;
        t_r[i] = r_lds && d < a.Dp ? a.qres[(size_t)b * a.Dp + d] : 0.0f;
    }
    double t_qn = 0.0, t_qc[3] = {0.0, 0.0, 0.0};
    float t_qe = 0.0f, t_qe2 = 0.0f, t_qsc = 0.0f;
    uint32_t t_chkr = 0u;
    constexpr int kScalarTid = 64 * (FW - 1);
    if (tid == kScalarTid) {
        t_qn = a.qn64[b];
        if (a.qconst) {
#pragma unroll
            for (int i = 0; i < 3; ++i) t_qc[i] = a.qconst[3 * (size_t)b + i];
        }
        if (a.qerr) t_qe = a.qerr[b];
        if (a.qerr2) t_qe2 = a.qerr2[b];
        if (a.xh_rm && a.qscal) t_qsc = a.qscal[0];
        if (a.chkp && a.chkr) t_chkr = *a.chkr;
    }
    // The int8 pass's checksum (vdb_scan8.hip): the workgroups' partial sums of this query's H (and
    // L) accumulators ([plane][query][workgroup], one coalesced read per lane), loaded here and
    // compared at the end against the value the stored operands imply.
    __shared__ int s_ckbad;
    uint32_t ck_h = 0u, ck_l = 0u, ck_eh = 0u, ck_el = 0u;
    if (a.chkp && tid < 64) {
        // (four words per lane requested together: with one per turn, the usual 256 workgroups
        // were four dependent round trips of wave 0 ahead of the first barrier; the sums are
        // integers modulo 2^32, so the order of the additions does not matter)
        for (int w0 = tid; w0 < a.chk_nw; w0 += 256) {
            uint32_t h4[4], l4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int w = min(w0 + 64 * u, a.chk_nw - 1);  // (past the end: the last word again, not added)
                h4[u] = a.chkp[(size_t)b * a.chk_nw + w];
                l4[u] = a.chk_l ? a.chkp[((size_t)a.chk_ld + b) * a.chk_nw + w] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (w0 + 64 * u < a.chk_nw) {
                    ck_h += h4[u];
                    ck_l += l4[u];
                }
            }
        }
        if (a.chke && tid == 0) {  // the expectations the pilot computed
            ck_eh = a.chke[2 * (size_t)b];
            ck_el = a.chke[2 * (size_t)b + 1];
        }
    }
    if (tid == 0) s_ckbad = 0;
    // ... or, without a pilot (a gated re-pass sub-search), computed here by the second wave:
    // sum_d CH[d] qh[d] (+ for L: CH ql + CL qh) from the query's int8 tiles (prep8 layout: s2_blk
    // of vdb_scan2_kernel.h, G8 + QG_EXTRA groups)
    if (a.chkp && !a.chke && tid >= 64 && tid < 128) {
        const int l = tid - 64, G8 = a.chk_g8, GQ = G8 + QG_EXTRA, Dp = 32 * G8;
        for (int cc = l; cc < 2 * G8; cc += 64) {
            const int g = cc >> 1, h = cc & 1, d0 = 32 * g + 16 * h;
            const float* src = a.chk_q + ((((size_t)(b >> 5) >> 2) * GQ + g) * 8 + ((b >> 5) & 3)) * BLOCK_FLOATS +
                               (size_t)((b & 31) + 32 * h) * 4;
            const f32x4 qh4 = *(const f32x4*)src;
            const f32x4 ql4 = a.chk_l ? *(const f32x4*)(src + 4 * BLOCK_FLOATS) : qh4;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t uh = __float_as_uint(qh4[w]), ul = __float_as_uint(ql4[w]);
#pragma unroll
                for (int bt = 0; bt < 4; ++bt) {
                    const int d = d0 + 4 * w + bt;
                    const uint32_t hv = (uint32_t)(int)(int8_t)((uh >> (8 * bt)) & 255u);
                    const uint32_t ch = a.chk_csum[d];
                    ck_eh += hv * ch;
                    if (a.chk_l) ck_el += (uint32_t)(int)(int8_t)((ul >> (8 * bt)) & 255u) * ch + hv * a.chk_csum[Dp + d];
                }
            }
        }
    }
    const int64_t c = a.seg_cnt ? 0 : min((int64_t)a.gl_cnt[b], a.gl_cap);
#ifdef VDB_STAMP
    if (threadIdx.x == 0) g_fin_stamps[b][7] = (unsigned long long)c;
#endif
    if (!a.seg_cnt && c > FIN_CAP) {
        if (tid == 0 && sp == 0) {
            const int pos = atomicAdd(a.flag_count, 1);
            a.flag_list[pos] = b;
            if (a.overflow_count) atomicAdd(a.overflow_count, 1);
        }
        return;
    }
    const float* ls = a.gl_s + (size_t)b * a.gl_cap;
    const uint32_t* li = a.gl_i + (size_t)b * a.gl_cap;
    // Entries below the final shared bound T cannot be among the KP best (T is at most the
    // KP-th best approx score, or the certificate fails on it anyway) and rows outside the
    // candidates only need approx <= max(a_KP, T): drop them while loading.  Lists are
    // appended by workgroups that flushed against older, lower bounds, so this typically
    // leaves about KP entries.
    const uint32_t tkey = a.gthr[b];
    __shared__ int s_n, s_ovf;
    __shared__ uint32_t s_cbmax;  // the refinement's largest per-row rounding bound (zeroed here: no barrier of its own)
    if (tid == 0) {
        s_ak = 0;
        s_akp = 0;
        s_n = 0;
        s_ovf = 0;
        s_cbmax = 0u;
    }
    __syncthreads();
    // the wide int8 pass's lists: one segment of W8_CH slots per scan workgroup, wave wv taking
    // segments wv, wv + FW, ...; a segment that overflowed sends the query to the exact path
    // (lane l of wave wv takes segment 64 (wv + FW i) + l: one round of count loads, then one
    // round per entry slot up to the wave's fullest segment -- typically a few entries each;
    // one wave per segment took a dependent round trip per segment, 32 per wave at C3 / C4)
    for (int sg0 = a.seg_cnt ? wv * 64 : a.seg_n; sg0 < a.seg_n; sg0 += FIN_WAVES * 64) {
        const int sg = sg0 + lane;
        const bool sin = sg < a.seg_n;
        uint32_t cnt = sin ? a.seg_cnt[(size_t)b * a.seg_n + sg] : 0u;
        // the segment's first four entry slots with its count (slots past the count hold stale
        // entries, masked below; all inside the segment, W8_CH >= 4): the usual segment of at most
        // four entries is one round trip instead of two
        // (an address of the query's own lists for every lane, a lane past the last segment
        // reading segment 0, so that the loads are unconditional: behind a predicate the compiler
        // moved them to their uses, after the wait for the count)
        const size_t sg_at = sin ? (size_t)sg * W8_CH : 0;
        const f32x4 f0 = *(const f32x4*)(ls + sg_at);
        uint4 r4 = *(const uint4*)(li + sg_at);
        uint32_t k0[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) k0[u] = order_key(f0[u]);
        asm volatile("" : "+v"(r4.x), "+v"(r4.y), "+v"(r4.z), "+v"(r4.w));  // (the rows' use, here: see above)
        const uint32_t r0[4] = {r4.x, r4.y, r4.z, r4.w};
        if (cnt > (uint32_t)W8_CH) {
            s_ovf = 1;
            cnt = 0;
        }
        uint32_t most = cnt;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) most = max(most, (uint32_t)__shfl_xor((int)most, off, 64));
        for (uint32_t j = 0; j < most; j += 4) {
            uint32_t key[4], row[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {  // (four entry slots' loads in flight together)
                const bool in = j + u < cnt;
                if (j == 0) {
                    key[u] = in ? k0[u] : 0u;
                    row[u] = in ? r0[u] : 0u;
                } else {
                    key[u] = in ? order_key(ls[(size_t)sg * W8_CH + j + u]) : 0u;
                    row[u] = in ? li[(size_t)sg * W8_CH + j + u] : 0u;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool keep = j + u < cnt && key[u] >= tkey;
                const unsigned long long bm = __ballot(keep);
                int base = 0;
                if (lane == 0 && bm) base = atomicAdd(&s_n, __popcll(bm));
                base = __shfl(base, 0, 64);
                if (keep) {
                    const int pos = base + __popcll(bm & ((1ull << lane) - 1ull));
                    if (pos < FIN_CAP) {  // (more: the list overflows this form's buffer, below)
                        s_key[pos] = key[u];
                        s_row[pos] = row[u];
                    }
                }
            }
        }
    }
    for (int e0 = wv * 64; e0 < c; e0 += 64 * FIN_WAVES) {
        const int e = e0 + lane;
        const uint32_t key = e < c ? order_key(ls[e]) : 0u;
        const uint32_t row = e < c ? li[e] : 0u;
        const bool keep = e < c && key >= tkey;
        const unsigned long long bm = __ballot(keep);
        int base = 0;
        if (lane == 0 && bm) base = atomicAdd(&s_n, __popcll(bm));
        base = __shfl(base, 0, 64);
        if (keep) {
            const int pos = base + __popcll(bm & ((1ull << lane) - 1ull));
            s_key[pos] = key;
            s_row[pos] = row;
        }
    }
    // publish the values requested at the top
#pragma unroll
    for (int i = 0; i < NQQ; ++i) s_q[tid + 64 * FW * i] = t_q[i];
#pragma unroll
    for (int i = 0; i < NQR; ++i) s_res[tid + 64 * FW * i] = t_r[i];
    if (tid == kScalarTid) {
        s_qn = t_qn;
#pragma unroll
        for (int i = 0; i < 3; ++i) s_qc[i] = t_qc[i];
        s_qe = t_qe;
        s_qe2 = t_qe2;
        s_qsc = t_qsc;
        s_chkr = t_chkr;
    }
    __syncthreads();
    if (s_ovf || s_n > FIN_CAP) {  // (uniform: every thread returns)
        if (tid == 0 && sp == 0) {
            const int pos = atomicAdd(a.flag_count, 1);
            a.flag_list[pos] = b;
            if (a.overflow_count) atomicAdd(a.overflow_count, 1);
        }
        return;
    }
    FIN_STAMP(1);
    const int n = s_n;
    // Select the KP best by (approx key desc, row asc): T = the KP-th largest key by an 8-bit
    // radix select over all waves (4 rounds: LDS histogram of the next digit among the
    // entries matching the prefix, one wave finds the digit holding the KP-th), then, only
    // if several entries tie at T, the rows kept at T by bisection on the row.
    __shared__ int s_cnt2[2];
    __shared__ uint32_t s_T, s_I, s_pref;
    __shared__ int s_hist[256];
    __shared__ int s_need, s_eq;
    if (n > KP) {
        uint32_t prefix = 0u, pmask = 0u;
        int need = KP;
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) s_hist[tid] = 0;
            __syncthreads();
            for (int e = tid; e < n; e += 64 * FIN_WAVES) {
                const uint32_t kk = s_key[e];
                if ((kk & pmask) == prefix) atomicAdd(&s_hist[(kk >> shift) & 255u], 1);
            }
            __syncthreads();
            if (wv == 0) {
                int h[4], sum = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {  // lane l: digits 255 - 4l .. 252 - 4l (descending)
                    h[j] = s_hist[255 - 4 * lane - j];
                    sum += h[j];
                }
                int incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int t = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += t;
                }
                int dsel = -1, above = incl - sum;
                if (incl - sum < need && need <= incl) {  // exactly one lane
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (dsel < 0) {
                            if (above + h[j] >= need) dsel = 255 - 4 * lane - j;
                            else above += h[j];
                        }
                    }
                }
                const int src = __ffsll((unsigned long long)__ballot(dsel >= 0)) - 1;
                dsel = __shfl(dsel, src, 64);
                above = __shfl(above, src, 64);
                if (lane == 0) {
                    s_pref = prefix | ((uint32_t)dsel << shift);
                    s_need = need - above;
                    s_eq = s_hist[dsel];
                }
            }
            __syncthreads();
            prefix = s_pref;
            pmask |= 255u << shift;
            need = s_need;
        }
        uint32_t I = 0xFFFFFFFFu;
        if (s_eq > need) {  // ties at T: keep the `need` lowest rows among them
            auto count_all = [&](auto pred, int parity) -> int {
                int cnt = 0;
                for (int e0 = wv * 64; e0 < n; e0 += 64 * FIN_WAVES) {
                    const int e = e0 + lane;
                    cnt += __popcll(__ballot(e < n && pred(e)));
                }
                if (lane == 0 && cnt) atomicAdd(&s_cnt2[parity], cnt);
                __syncthreads();
                const int total = s_cnt2[parity];
                __syncthreads();
                if (tid == 0) s_cnt2[parity] = 0;
                return total;
            };
            if (tid == 0) s_cnt2[0] = s_cnt2[1] = 0;
            __syncthreads();
            I = 0;
            for (int bit = 31; bit >= 0; --bit) {
                const uint32_t cand = I | (1u << bit);
                if (count_all([&](int e) { return s_key[e] == prefix && s_row[e] < cand; }, bit & 1) < need) I = cand;
            }
        }
        if (tid == 0) {
            s_T = prefix;
            s_I = I;
        }
        __syncthreads();
    }
    if (wv == 0) {
        const int m = n < KP ? n : KP;
        const uint32_t T = n > KP ? s_T : 0u, I = n > KP ? s_I : 0xFFFFFFFFu;
        int base = 0;
        for (int e0 = 0; e0 < n; e0 += 64) {
            const int e = e0 + lane;
            const bool in = e < n;
            const uint32_t kk = in ? s_key[e] : 0u;
            const uint32_t rr = in ? s_row[e] : 0u;
            const bool keep = in && (n <= KP || kk > T || (kk == T && rr <= I));
            const unsigned long long bm = __ballot(keep);
            const int pos = base + __popcll(bm & ((1ull << lane) - 1ull));
            if (keep && pos < KP) {
                s_ck[pos] = kk;
                s_cr[pos] = rr;
            }
            base += __popcll(bm);
        }
        if (lane == 0) s_m = m;
    }
    __syncthreads();
    FIN_STAMP(2);
    int m = s_m;
    const double qn = s_qn;
    // The I8 refinement's row loads (below, after the certificate), two batches of NBR rows per
    // wave in flight: batch t + 1 is requested before batch t is reduced, and batch 0 here, as
    // soon as the selection is final, so the rank counts and the certificate run under it.  Only
    // rows s_cr[j], j < m, of a query that has its k candidates are requested (fewer: the
    // certificate sets no cut and there is no refinement); where the certificate then sets no cut
    // after all, the values are dropped.  Step t = (batch, 1024-dim chunk of the row).
#ifndef VDB_FIN_NBR
#define VDB_FIN_NBR (FIN_WAVES > 8 ? 4 : 8)
#endif
    constexpr int NBR = VDB_FIN_NBR;  // candidates per wave per batch (row loads in flight together)
    const int rf_nch = kShortOnly ? 1 : (a.Dp + 1023) >> 10;
    const int rf_T = a.xh_rm != nullptr && m >= a.k && m > wv * NBR
                         ? (m - wv * NBR + FIN_WAVES * NBR - 1) / (FIN_WAVES * NBR) * rf_nch : 0;
    // A step's NBR loads are unconditional (t < rf_T, the wave's own step): behind per-load
    // predicates the compiler cannot count what is in flight and waits for everything, the batch
    // just requested included.  The last batch's slots past m repeat candidate m - 1 and a lane
    // past the row's end its first 16 bytes: addresses of validated rows, values never used.
    auto rf_issue = [&](int t, f32x4 (&xv)[NBR]) {
        const int bi = rf_nch == 1 ? t : t / rf_nch;
        const int j0 = (wv + FIN_WAVES * bi) * NBR, off = (t - bi * rf_nch) * 1024 + 16 * lane;
        const int offc = off < a.Dp ? off : 0;
#pragma unroll
        for (int u = 0; u < NBR; ++u)
            xv[u] = *(const f32x4*)(a.xh_rm + (size_t)s_cr[min(j0 + u, m - 1)] * a.Dp + offc);
    };
    f32x4 rf_xa[NBR], rf_xb[NBR];
    if (rf_T > 0) rf_issue(0, rf_xa);
    // ---- the certificate first, from the approximate scores alone ----
    // a_k / a_KP: the k-th / KP-th best approx key of the selection (rank counting, TPC threads
    // per candidate).  Rows outside the candidates scored (approx) <= acut = max(a_KP, T)
    // (DESIGN.md §3.2); with |approx - exact| <= eps per row the certificate is
    // acut + eps < a_k - eps.
    constexpr int TPC = KP >= 64 * FIN_WAVES ? 1 : (64 * FIN_WAVES) / KP > 64 ? 64 : (64 * FIN_WAVES) / KP;
    // Only the VALUES of the k-th and KP-th are needed: the candidate whose key v has fewer than
    // k keys above it and at least k at or above it holds it (ties give the same value), so each
    // of TPC threads counts a contiguous chunk with 16-byte LDS reads (the rank by (key, row) of
    // every candidate was ~20 K cycles at KP = 256: an unpipelined LDS round trip per entry)
    const int chunk = ((m + TPC - 1) / TPC + 3) & ~3;
    for (int jt = tid; jt < KP * TPC; jt += 64 * FIN_WAVES) {
        const int j = jt / TPC, sub = jt % TPC;
        int g = 0, ge = 0;
        uint32_t ck = 0u;
        if (j < m) {
            ck = s_ck[j];
            const int i0 = sub * chunk, i1 = min(m, i0 + chunk);
            int i = i0;
            for (; i + 4 <= i1; i += 4) {
                const uint4 v = *(const uint4*)(s_ck + i);
                g += (v.x > ck) + (v.y > ck) + (v.z > ck) + (v.w > ck);
                ge += (v.x >= ck) + (v.y >= ck) + (v.z >= ck) + (v.w >= ck);
            }
            for (; i < i1; ++i) {
                const uint32_t v = s_ck[i];
                g += v > ck;
                ge += v >= ck;
            }
        }
#pragma unroll
        for (int off = 1; off < TPC; off <<= 1) {
            g += __shfl_xor(g, off, 64);
            ge += __shfl_xor(ge, off, 64);
        }
        if (sub == 0 && j < m) {
            if (g < a.k && ge >= a.k) s_ak = ck;
            if (g < KP && ge >= KP) s_akp = ck;
        }
    }
    FIN_STAMP(13);
    // bf16 corpus rounding: |q.(y - bf16(y))| <= bq, Cauchy-Schwarz |q| R or, along the index's
    // residual direction, |q - c dir| R + |c| M with c = q.dir (vdb_ingest.hip resid_dir_kernel);
    // cosine on the unit query
    __shared__ double s_bq, s_shift;
    if (wv == 1) {
        // exact = approx + shift, per query: the candidate passes score 2 q.x - |x|^2 for L2
        // (-|q|^2 to the exact key), the int8 pass leaves out mu.q' (cosine) / 2 mu.q (L2) as
        // the same constant for every row (vdb_scan8_kernel.h).  The approximate certificate
        // and the rerank cut only compare approximate scores with each other; the exact-key
        // test compares an exact key with them.
        double mq = 0.0;
        if (a.mu && a.qconst) {
            mq = s_qc[0];
        } else if (a.mu) {
            const float* qq = a.Q + (int64_t)b * a.D;
            const double qs = METRIC == 0 ? 1.0 / fmax(qn, 1e-8) : 1.0;
            for (int d = lane; d < a.D; d += 64) mq += (double)qq[d] * qs * (double)a.mu[d];
            mq = wave_sum_butterfly(mq);
        }
        if (lane == 0) s_shift = METRIC == 0 ? mq : 2.0 * mq - qn * qn;
    }
    if (wv == 0) {
        double bq = 0.0;
        if (a.xres > 0.0) {
            bq = METRIC == 0 ? a.xres : qn * a.xres;
            if (a.dir) {
                double c = 0.0, w2 = 0.0;
                if (a.qconst) {
                    c = s_qc[1];
                    w2 = s_qc[2];
                } else {
                    const float* qq = a.Q + (int64_t)b * a.D;
                    const double qs = METRIC == 0 ? 1.0 / fmax(qn, 1e-8) : 1.0;
                    for (int d = lane; d < a.D; d += 64) c += (double)qq[d] * qs * (double)a.dir[d];
                    c = wave_sum_butterfly(c);
                    for (int d = lane; d < a.D; d += 64) {
                        const double w = (double)qq[d] * qs - c * (double)a.dir[d];
                        w2 += w * w;
                    }
                    w2 = wave_sum_butterfly(w2);
                }
                // (1 + 1e-6) and + 1e-6 R: the fp64 evaluation and the fp32-normalised query
                const double bd = (sqrt(w2) * a.xres + fabs(c) * a.dres) * (1.0 + 1e-6) + 1e-6 * a.xres;
                bq = fmin(bq, bd);
            }
        }
        if (lane == 0) s_bq = bq;
    }
    __shared__ double s_cut;
    // the exact-key certificate (one workgroup per query): when the approximate one fails, the
    // query is still certified if the exact k-th best of the reranked candidates beats every
    // row outside them, e_k > acut + eps (those score <= acut + eps).  The rerank set holds
    // every candidate that can be in the exact top k (approx >= a_k - 2 eps), so e_k >= a_k -
    // eps: this never fails where the approximate test (a_k - eps > acut + eps) passes, and
    // needs one eps of gap instead of two.  s_bar = acut + eps, or +inf where it cannot apply.
    __shared__ double s_bar, s_ekk;
    __shared__ int s_ok1;  // 0 = deferred to the exact-key test
    // The consistency guard: every certificate above assumes |approx - (exact - shift)| <= eps
    // for every row.  The reranked candidates have both values, so check it for them: a query
    // with a reranked row outside its bound goes to the exact path instead of being certified
    // (a pass that scored with a wrong operand -- VERDICT r3: a stale start value -- shows
    // up in the rows it over-scored).  s_epsb = eps without the L2 rounding term in |approx|.
    __shared__ double s_epsb;
    __shared__ int s_fl0, s_bad;
    __shared__ uint32_t s_ckeh, s_ckel;
    if (a.chkp && tid < 128) {  // the checksum's verdict (its loads were issued at the start)
        // wave 0: the pass's sums (+ the pilot's expectations in lane 0); wave 1: the expectations
        // when there was no pilot
        const bool w1 = tid >= 64;
        uint32_t x = w1 ? ck_eh : ck_h, y = w1 ? ck_el : ck_l;
        if (w1 && a.chke) x = y = 0u;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            x += (uint32_t)__shfl_xor((int)x, off, 64);
            y += (uint32_t)__shfl_xor((int)y, off, 64);
        }
        if (tid == 64 && !a.chke) {
            s_ckeh = x;
            s_ckel = y;
        }
        ck_h = x;
        ck_l = y;
    }
    FIN_STAMP(14);
    __syncthreads();
    FIN_STAMP(15);
    if (tid == 0) {
        if (a.chkp) {
            const uint32_t eh = (a.chke ? ck_eh : s_ckeh) + s_chkr;
            const uint32_t el = a.chke ? ck_el : s_ckel;
            s_ckbad = ck_h != eh || (a.chk_l && ck_l != el);
        }
        const bool full = m == KP;
        const double T = (double)key_to_float(tkey);
        const bool have_k = m >= a.k;
        const double ak = have_k ? (double)key_to_float(s_ak) : -INFINITY;
        const double qe = (double)s_qe;  // the int8 pass's per-query share (0 without one)
        bool ok = true;
        double eps = 0.0;
        if (full || T > -INFINITY) {
            const double akp = full ? (double)key_to_float(s_akp) : -INFINITY;
            const double acut = fmax(akp, T);
            if (METRIC == 0) {
                eps = a.eps_rel + s_bq + qe;
            } else {
                eps = a.eps_rel * (2.0 * qn * a.xmax + a.xmax * a.xmax) + 2.0 * s_bq +
                      2.4e-7 * fmax(fabs(ak), fabs(acut)) + qe;
            }
            ok = have_k && acut + eps < ak - eps;
        } else if (have_k) {  // the list holds every eligible row: only the rerank cut needs eps
            eps = METRIC == 0 ? a.eps_rel + s_bq + qe
                              : a.eps_rel * (2.0 * qn * a.xmax + a.xmax * a.xmax) + 2.0 * s_bq +
                                    2.4e-7 * fabs(ak) + qe;
        }
        s_epsb = METRIC == 0 ? a.eps_rel + s_bq + qe
                             : a.eps_rel * (2.0 * qn * a.xmax + a.xmax * a.xmax) + 2.0 * s_bq + qe;
        s_bad = 0;
        // decided after the exact keys (split > 1: by the workgroup that gathers the shares)
        const bool defer = have_k && !ok;
        s_fl0 = !ok && !defer;  // flagged here (the same decision in every workgroup of the query)
        if (!ok && !defer && sp == 0) {
            const int pos = atomicAdd(a.flag_count, 1);
            a.flag_list[pos] = b;
            if (s_ckbad && a.incons_count) atomicAdd(a.incons_count, 1);
        }
        s_ok1 = defer ? 0 : 1;  // 0: the exact-key test decides the flag
        s_ekk = -INFINITY;
        if (defer) {
            const double akp = full ? (double)key_to_float(s_akp) : -INFINITY;
            s_bar = fmax(akp, T) + eps;
        } else {
            s_bar = INFINITY;
        }
        // Rerank cut: the k best approx rows score (exact) >= a_k - eps, so the exact k-th best
        // is >= a_k - eps, and a row with approx < a_k - 2 eps scores (exact) < a_k - eps:
        // only candidates with approx >= a_k - 2 eps can be in the exact top k (2.001: the L2
        // bound's rounding term grows with |approx| below a_k).  Valid whether or not the
        // approximate certificate passed (it only compares candidates with each other).
        s_cut = (ok || defer) && have_k ? ak - 2.001 * eps : -INFINITY;
    }
    __syncthreads();
    // ---- the I8 refinement: a' = a + f s_x xh.r per candidate (xh the row's 8-bit plane, r the
    // query's rounding residual), then the rerank cut on a' with eps' = eps without the query's
    // rounding term (prep8 qerr2) plus the refinement's own fp32 rounding per row.  The pass's
    // wide 8-bit-query bound left every one of KP = 256 candidates within 2 eps of a_k at C2 /
    // C3 (finish stamps, profiles/r04): each then cost a whole fp32 row of exact key.
#ifdef VDB_STAMP
    if (threadIdx.x == 0) g_fin_stamps[blockIdx.x][6] = __builtin_amdgcn_s_memtime();
#endif
    __shared__ __attribute__((aligned(16))) float s_ca[KP];
    __shared__ float s_ak2;
    __shared__ double s_e2;  // the refined bound eps' (the consistency guard checks a' against it too)
    const bool refine = a.xh_rm != nullptr && s_cut > -INFINITY;
    if (refine) {
        const float fsx = (METRIC == 0 ? 1.0f : 2.0f) * a.sx;
        const float qmx = 127.0f * s_qsc / a.sx;  // s_q * 127 = max |q'|
        // rd(o): 16 bytes of the residual at element o, from the LDS copy made at the top or, rows
        // of more than QLR dims, from memory: one instance of the loops each (a pointer chosen at run
        // time makes them flat loads, which wait for every vector load in flight)
        auto rf_run = [&](auto rd) {
            // the rows are stored as u = xh + 128: xh.r = u.r - 128 sum(r); sum(r) and sum|r| once
            float rsum = 0.0f, rabs = 0.0f;
            for (int off = 16 * lane; off < a.Dp; off += 1024)
#pragma unroll
                for (int w4 = 0; w4 < 4; ++w4) {
                    const f32x4 rv = rd(off + 4 * w4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        rsum += rv[e];
                        rabs += fabsf(rv[e]);
                    }
                }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                rsum += __shfl_xor(rsum, off, 64);
                rabs += __shfl_xor(rabs, off, 64);
            }
            // fp32 bound of the correction, per query: the D biased products and their sum (|u r|
            // <= 256 |r|), the subtraction of 128 sum(r), r = q' - s_q qh itself (<= 2 ulp of |q'|
            // per element), times f s_x; plus (per row) the roundings of a'
            const float bq2 = fsx * (((float)a.Dp + 8.0f) * 5.97e-8f * 256.0f * rabs + 1.2e-7f * qmx * 127.0f * (float)a.D);
            FIN_STAMP(8);
            // one step: the chunk's products added to the batch's sums in the order of `off`, and
            // after the row's last chunk the butterfly and a' (the same operations per candidate in
            // the same order whatever is in flight)
            float sum[NBR];
            auto rf_step = [&](int t, const f32x4 (&xv)[NBR]) {
                const int bi = rf_nch == 1 ? t : t / rf_nch, ci = t - bi * rf_nch;
                const int j0 = (wv + FIN_WAVES * bi) * NBR, off = ci * 1024 + 16 * lane;
                if (ci == 0) {
#pragma unroll
                    for (int u = 0; u < NBR; ++u) sum[u] = 0.0f;
                }
                if (off < a.Dp) {
                    f32x4 rv[4];
#pragma unroll
                    for (int w4 = 0; w4 < 4; ++w4)
                        rv[w4] = rd(off + 4 * w4);
#pragma unroll
                    for (int u = 0; u < NBR; ++u)
#pragma unroll
                        for (int w4 = 0; w4 < 4; ++w4) {
                            const uint32_t word = __float_as_uint(xv[u][w4]);
#pragma unroll
                            for (int bt = 0; bt < 4; ++bt)
                                sum[u] = fmaf((float)((word >> (8 * bt)) & 255u), rv[w4][bt], sum[u]);
                        }
                }
                if (ci != rf_nch - 1) return;
#pragma unroll
                for (int off2 = 32; off2 >= 1; off2 >>= 1)
#pragma unroll
                    for (int u = 0; u < NBR; ++u) sum[u] += __shfl_xor(sum[u], off2, 64);
                if (lane == 0) {
                    float bmax = 0.0f;
#pragma unroll
                    for (int u = 0; u < NBR; ++u) {
                        const int j = j0 + u;
                        if (j < m) {
                            const float ap = key_to_float(s_ck[j]) + fsx * (sum[u] - 128.0f * rsum);
                            s_ca[j] = ap;
                            bmax = fmaxf(bmax, 2.4e-7f * fabsf(ap));
                        }
                    }
                    atomicMax(&s_cbmax, __float_as_uint((bq2 + bmax) * 1.01f));
                }
            };
            // (step 0 was requested before the certificate; the steady state requests unconditionally,
            // so each wait leaves exactly the step just requested in flight, and the last one or two
            // steps are taken without a request after them)
            int t = 0;
            for (; t + 2 < rf_T; t += 2) {
                rf_issue(t + 1, rf_xb);
                rf_step(t, rf_xa);
                rf_issue(t + 2, rf_xa);
                rf_step(t + 1, rf_xb);
            }
            if (t + 2 == rf_T) {
                rf_issue(t + 1, rf_xb);
                rf_step(t, rf_xa);
                rf_step(t + 1, rf_xb);
            } else if (t + 1 == rf_T) {
                rf_step(t, rf_xa);
            }
        };
        if (kShortOnly || r_lds) {
            rf_run([&](int o) { return *(const f32x4*)(s_res + o); });
        } else {
            const float* rq = a.qres + (size_t)b * a.Dp;
            rf_run([&](int o) { return *(const f32x4*)(rq + o); });
        }
        FIN_STAMP(9);
        __syncthreads();
        FIN_STAMP(10);
        // a'_k by rank counting over (a' desc, row asc), TPC threads per candidate
        for (int jt = tid; jt < KP * TPC; jt += 64 * FIN_WAVES) {  // (the value alone, as above)
            const int j = jt / TPC, sub = jt % TPC;
            int g = 0, ge = 0;
            float cj = 0.0f;
            if (j < m) {
                cj = s_ca[j];
                const int i0 = sub * chunk, i1 = min(m, i0 + chunk);
                int i = i0;
                for (; i + 4 <= i1; i += 4) {
                    const f32x4 v = *(const f32x4*)(s_ca + i);
                    g += (v[0] > cj) + (v[1] > cj) + (v[2] > cj) + (v[3] > cj);
                    ge += (v[0] >= cj) + (v[1] >= cj) + (v[2] >= cj) + (v[3] >= cj);
                }
                for (; i < i1; ++i) {
                    const float v = s_ca[i];
                    g += v > cj;
                    ge += v >= cj;
                }
            }
#pragma unroll
            for (int off = 1; off < TPC; off <<= 1) {
                g += __shfl_xor(g, off, 64);
                ge += __shfl_xor(ge, off, 64);
            }
            if (sub == 0 && j < m && g < a.k && ge >= a.k) s_ak2 = cj;
        }
        __syncthreads();
        FIN_STAMP(11);
        if (tid == 0) {
            const double ak2 = (double)s_ak2;
            const double qe2 = (double)s_qe2;
            const double e2 = (METRIC == 0 ? a.eps_rel + s_bq + qe2
                                           : a.eps_rel * (2.0 * qn * a.xmax + a.xmax * a.xmax) + 2.0 * s_bq + qe2) +
                              (double)__uint_as_float(s_cbmax);
            s_cut = fmax(ak2 - 2.001 * e2, -3.0e38);  // never below the unrefined cut's domain
            s_e2 = e2;
        }
        __syncthreads();
        FIN_STAMP(12);
    }
    if (s_cut > -INFINITY) {
        const double cut = s_cut;
        if (wv == 0) {
            int base = 0;
            for (int e0 = 0; e0 < m; e0 += 64) {  // in-place compaction (reads run ahead of writes)
                const int e = e0 + lane;
                const bool in = e < m;
                const uint32_t kk = in ? s_ck[e] : 0u, rr = in ? s_cr[e] : 0u;
                const float ca = in && refine ? s_ca[e] : 0.0f;
                const bool keep = in && (refine ? (double)ca : (double)key_to_float(kk)) >= cut;
                const unsigned long long bm = __ballot(keep);
                if (keep) {
                    const int pos = base + __popcll(bm & ((1ull << lane) - 1ull));
                    s_ck[pos] = kk;
                    s_cr[pos] = rr;
                    if (refine) s_ca[pos] = ca;  // (carried for the consistency guard)
                }
                base += __popcll(bm);
            }
            if (lane == 0) s_m = base;
        }
        __syncthreads();
        m = s_m;
    }
#ifdef VDB_STAMP
    // [6] (time after the certificate) -> ticks of the refinement and the cut; the rerank set
    // size in the high bits
    if (threadIdx.x == 0) g_fin_stamps[b][6] = (__builtin_amdgcn_s_memtime() - g_fin_stamps[b][6]) | ((unsigned long long)m << 40);
#endif
    // split > 1: the candidates with row % S == sp are this workgroup's (the selected set is
    // the same in every workgroup of the query, its LDS order is not)
    uint32_t* xr = s_cr;
    double* xek = s_ek;
    int mx = m;
    if (S > 1) {
        if (wv == 0) {
            int base = 0;
            for (int e0 = 0; e0 < m; e0 += 64) {
                const int e = e0 + lane;
                const bool mine = e < m && (int)(s_cr[e] % (uint32_t)S) == sp;
                const unsigned long long bm = __ballot(mine);
                if (mine) {
                    const int pos = base + __popcll(bm & ((1ull << lane) - 1ull));
                    s_ock[pos] = s_ck[e];
                    s_ocr[pos] = s_cr[e];
                }
                base += __popcll(bm);
            }
            if (lane == 0) s_mown = base;
        }
        __syncthreads();
        xr = s_ocr;
        xek = s_oek;
        mx = s_mown;
    }
    FIN_STAMP(3);
    const float* q = a.Q + (int64_t)b * a.D;
    // exact keys: wave wv takes candidates wv NB, ... in batches of NB
    const int np = (a.D + 255) / 256;
    // The batched paths (rows of up to 256 MP dims): every piece of NB rows requested at once.  HELD:
    // the query's pieces in registers, from their LDS copy (the 4- and 16-wave forms); else read
    // from memory (L1-resident) as each piece is consumed (the 8-wave form: C3's 8 pieces).
    auto keys_ahead = [&](auto mp_c, auto nb_c, auto held_c) {
        constexpr int MP = decltype(mp_c)::value, NB = decltype(nb_c)::value;
        constexpr bool HELD = decltype(held_c)::value;
        // a batch's norms and row pieces, requested together; the next batch's are requested once
        // this batch's products are summed (its pieces' registers are free again), before its fp64
        // butterfly, and the first batch before the query pieces are read
        f32x4 xv[MP][NB];
        double xnl = 1.0;  // row u's norm in lane u (one register pair for the batch)
        auto issue = [&](int j0) {
            const int nb = min(NB, mx - j0);  // (<= 0 past the wave's last batch: nothing is requested)
            uint32_t rows[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) rows[u] = u < nb ? xr[j0 + u] : 0u;
            xnl = (METRIC == 0 && lane < nb) ? a.nrm64[xr[j0 + lane]] : 1.0;
            exact_rows_load<NB, MP>(a.X, a.G, np, rows, nb, xv);
        };
        issue(wv * NB);
        float qv[HELD ? MP : 1][4];
        if (HELD) {
#pragma unroll
            for (int mm = 0; mm < (HELD ? MP : 0); ++mm) {
                // (rows of at most 256 MP <= 1024 dims: the query is in s_q, zeros from D on)
                const f32x4 ql = *(const f32x4*)(s_q + 4 * (mm * 64 + lane));
#pragma unroll
                for (int j = 0; j < 4; ++j) qv[mm][j] = ql[j];
            }
        }
        // (the 16-wave form requests the next batch after the butterfly: beside it the pieces in
        // flight cost 36 bytes of scratch per lane at its 128 registers, and with 48 rows a round
        // few of its waves have a second batch at all)
        constexpr bool kAhead = FIN_WAVES <= 8;
        for (int j0 = wv * NB; j0 < mx; j0 += FIN_WAVES * NB) {
            const int nb = min(NB, mx - j0);
            if (!kAhead && j0 != wv * NB) issue(j0);
            double acc[NB], xnc[NB];
            if constexpr (HELD) exact_rows_sum<METRIC, NB, MP>(qv, xv, np, acc);
            else exact_rows_sum_mem<METRIC, NB, MP>(q, a.D, xv, np, acc);
            const double xnh = xnl;
            if (kAhead) issue(j0 + FIN_WAVES * NB);
#pragma unroll
            for (int u = 0; u < NB; ++u) xnc[u] = __shfl(xnh, u, 64);
            double keys[NB];
            exact_rows_keys<METRIC, NB>(acc, s_qn, xnc, nb, keys);
            if (lane == 0) {
#pragma unroll
                for (int u = 0; u < NB; ++u)
                    if (u < nb) xek[j0 + u] = keys[u];
            }
        }
    };
    // (kShortOnly, at the top: the 16- and 4-wave forms compile the register path only)
    if (kShortOnly || np <= FIN_MP) {
        keys_ahead(std::integral_constant<int, FIN_MP>{}, std::integral_constant<int, FIN_NB4>{},
                   std::integral_constant<bool, kStageQ>{});
    } else if (np <= FIN_MP8) {
        keys_ahead(std::integral_constant<int, FIN_MP8>{}, std::integral_constant<int, FIN_NB8>{},
                   std::integral_constant<bool, false>{});
    } else if (!kShortOnly)
    for (int j0 = wv * FIN_NB; j0 < mx; j0 += FIN_WAVES * FIN_NB) {
        uint32_t rows[FIN_NB];
        double xn[FIN_NB];
        const int nb = min(FIN_NB, mx - j0);
#pragma unroll
        for (int u = 0; u < FIN_NB; ++u) {
            rows[u] = u < nb ? xr[j0 + u] : 0u;
            xn[u] = (METRIC == 0 && u < nb) ? a.nrm64[rows[u]] : 1.0;
        }
        double keys[FIN_NB];
        exact_keys_batch<METRIC, FIN_NB>(q, qn, a.X, a.G, a.D, rows, xn, nb, keys);
        if (lane == 0) {
#pragma unroll
            for (int u = 0; u < FIN_NB; ++u)
                if (u < nb) xek[j0 + u] = keys[u];
        }
    }
    __syncthreads();
    if (S > 1) {
        // publish this share; the workgroup that finishes the query's shares last gathers them
        // (release: the share before the count; acquire: the other shares after it)
        const size_t base = ((size_t)b * S + sp) * KP;
        for (int j = tid; j < mx; j += 64 * FIN_WAVES) {
            a.sx_ek[base + j] = s_oek[j];
            a.sx_ck[base + j] = s_ock[j];
            a.sx_cr[base + j] = s_ocr[j];
        }
        if (tid == 0) a.sx_n[(size_t)b * S + sp] = mx;
        __syncthreads();
        if (tid == 0) {
            __threadfence();
            s_last = atomicAdd(a.done + b, 1) == S - 1;
        }
        __syncthreads();
        if (!s_last) return;
        __threadfence();
        int off = 0;
        for (int p = 0; p < S; ++p) {
            const int np_ = a.sx_n[(size_t)b * S + p];
            const size_t pb = ((size_t)b * S + p) * KP;
            for (int j = tid; j < np_; j += 64 * FIN_WAVES) {
                s_ek[off + j] = a.sx_ek[pb + j];
                s_ck[off + j] = a.sx_ck[pb + j];
                s_cr[off + j] = a.sx_cr[pb + j];
            }
            off += np_;
        }
        if (tid == 0) a.done[b] = 0;  // the gated fallback counts from zero again
        m = off;
        __syncthreads();
    }
    FIN_STAMP(4);
    // exact ranks by counting (output order), TPC threads per candidate as above, each over a
    // contiguous chunk in 16-byte LDS reads; a count that reaches k stops (only ranks < k are
    // written, and rank k - 1's key)
    const int chunk2 = ((m + TPC - 1) / TPC + 3) & ~3;
    for (int jt = tid; jt < KP * TPC; jt += 64 * FIN_WAVES) {
        const int j = jt / TPC, sub = jt % TPC;
        int er = 0;
        double ek = 0.0;
        uint32_t r = 0u;
        if (j < m) {
            ek = s_ek[j];
            r = s_cr[j];
            const int i0 = sub * chunk2, i1 = min(m, i0 + chunk2);
            for (int i = i0; i < i1 && er < a.k; i += 2) {
                const double2 e2 = *(const double2*)(s_ek + i);
                const uint2 r2 = *(const uint2*)(s_cr + i);
                er += (e2.x > ek || (e2.x == ek && r2.x < r)) ? 1 : 0;
                if (i + 1 < i1) er += (e2.y > ek || (e2.y == ek && r2.y < r)) ? 1 : 0;
            }
        }
#pragma unroll
        for (int off = 1; off < TPC; off <<= 1) er += __shfl_xor(er, off, 64);
        if (sub != 0) continue;
        if (j < m) {
            if (er == a.k - 1) s_ekk = ek;
            if (er < a.k) {
                const size_t o = (size_t)b * a.k + er;
                write_result(METRIC, ek, global_row(a.row_ids, r, a.index_offset), true, a.out_s + o, a.out_i + o,
                             a.out_k ? a.out_k + o : nullptr);
            }
        } else if (j < a.k) {
            const size_t o = (size_t)b * a.k + j;
            write_result(METRIC, -INFINITY, 0, false, a.out_s + o, a.out_i + o, a.out_k ? a.out_k + o : nullptr);
        }
    }
    for (int j = KP + tid; j < a.k; j += 64 * FIN_WAVES) {  // k > KP cannot happen on this path; defensive
        const size_t o = (size_t)b * a.k + j;
        write_result(METRIC, -INFINITY, 0, false, a.out_s + o, a.out_i + o, a.out_k ? a.out_k + o : nullptr);
    }
    {
        const double sh = s_shift, eb = s_epsb;
        bool bad = false;
        // with the I8 refinement the rerank cut relied on |a' - (exact - shift)| <= eps' (the
        // refined bound): a stale or misindexed row-major xh plane breaks that one, so it is
        // checked too.  (split > 1 reorders the candidates: the refined check is
        // skipped there; the refinement runs with split 1.)
        const bool chk2 = refine && S == 1;
        const double e2 = chk2 ? s_e2 : 0.0;
        for (int j = tid; j < m; j += 64 * FIN_WAVES) {
            const double ap = (double)key_to_float(s_ck[j]), ex = s_ek[j] - sh;
            const double fr = 4e-16 * (fabs(s_ek[j]) + fabs(sh));
            const double bound = 1.01 * (eb + (METRIC == 1 ? 2.4e-7 * fmax(fabs(ap), fabs(ex)) : 0.0)) + fr;
            bad |= !(fabs(ap - ex) <= bound);
            if (chk2) {
                const double a2 = (double)s_ca[j];
                const double bound2 = 1.01 * (e2 + (METRIC == 1 ? 2.4e-7 * fmax(fabs(a2), fabs(ex)) : 0.0)) + fr;
                bad |= !(fabs(a2 - ex) <= bound2);
            }
        }
        if (__any(bad) && lane == 0) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    if (tid == 0 && !s_fl0) {
        const double ekk = s_ekk - s_shift;  // the exact k-th best in approximate units (+ fp64 rounding)
        const double tol = 4e-16 * (fabs(s_ekk) + fabs(s_shift));
        // neither certificate, or a reranked row outside its bound: the exact path rewrites
        // the query
        if ((!s_ok1 && !(ekk - tol > s_bar)) || s_bad || s_ckbad) {
            const int pos = atomicAdd(a.flag_count, 1);
            a.flag_list[pos] = b;
            if ((s_bad || s_ckbad) && a.incons_count) atomicAdd(a.incons_count, 1);
        }
    }
    FIN_STAMP(5);
}

hipError_t launch_finish(int metric, int KP, const FinishArgs& a, int B, hipStream_t st) {
    if (a.split < 1 || (a.split > 1 && (!a.sx_ek || !a.sx_ck || !a.sx_cr || !a.sx_n || !a.done)))
        return hipErrorInvalidValue;
    const bool w8 = FIN_WAVES > 8 && a.D > 1024;
    // (the forms' exact-key paths are compiled per row length, finish_kernel kShortOnly)
    if (a.small && a.D > 1024) return hipErrorInvalidValue;
#define VDB_FIN(M, KPV)                                                                                    \
    if (metric == M && KP == KPV) {                                                                        \
        if (a.small)                                                                                       \
            hipLaunchKernelGGL((finish_kernel<M, KPV, 4, FIN_CAP_SMALL>), dim3(B, a.split), dim3(64 * 4), 0, st, a); \
        else if (w8)                                                                                       \
            hipLaunchKernelGGL((finish_kernel<M, KPV, 8>), dim3(B, a.split), dim3(64 * 8), 0, st, a);      \
        else                                                                                               \
            hipLaunchKernelGGL((finish_kernel<M, KPV>), dim3(B, a.split), dim3(64 * FIN_WAVES), 0, st, a); \
        return hipGetLastError();                                                                          \
    }
    VDB_FIN(0, 32) VDB_FIN(0, 64) VDB_FIN(0, 128) VDB_FIN(0, 256)
    VDB_FIN(1, 32) VDB_FIN(1, 64) VDB_FIN(1, 128) VDB_FIN(1, 256)
#undef VDB_FIN
    return hipErrorInvalidValue;
}

// Exact scan (certificate fallback, and the path for k > 200): every eligible
// row of a workgroup's range gets its exact key (one wave per row); each wave
// streams its rows through a WaveTopK (LDS buffer), then wave 0 folds the other
// three waves' lists into its own and writes the workgroup's sorted top-KE.
template <int METRIC>
__global__ void __launch_bounds__(256)
exact_scan_kernel(const float* __restrict__ Q, const double* __restrict__ qn64, const int* __restrict__ qlist,
                  const float* __restrict__ X, int G, int D, const double* __restrict__ nrm64,
                  const uint32_t* __restrict__ mask, int64_t N, int64_t rows_per_wg, int KE,
                  double* __restrict__ lk, uint32_t* __restrict__ li, const int* __restrict__ qcount, int nq_max,
                  const int* __restrict__ ovf, unsigned long long* __restrict__ totals, ExactTail tail,
                  char* __restrict__ gscr) {
    // The per-wave top-k buffers and the tail merge's scratch: LDS, or -- the device-gated form --
    // the workspace (gscr: this launch's [slot][range][wave] buffers, then one merge scratch per
    // slot), so the launch holds no LDS: an empty gated launch (nothing flagged, the common case)
    // then retires beside another batch's scan instead of waiting for a CU with free LDS (C3's
    // scan leaves ~3 KiB of its CU's 160)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int cap = WaveTopK<double, uint32_t>::capacity(KE);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const size_t nbuf = (size_t)gridDim.y * gridDim.x * 4;  // wave buffers of the launch (gscr)
    const size_t b0 = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 4;
    double* kbase = gscr ? reinterpret_cast<double*>(gscr) + b0 * cap : reinterpret_cast<double*>(smem);
    uint32_t* ibase = gscr ? reinterpret_cast<uint32_t*>(gscr + nbuf * cap * sizeof(double)) + b0 * cap
                           : reinterpret_cast<uint32_t*>(smem + (size_t)4 * cap * sizeof(double));
    char* mscr = gscr ? gscr + nbuf * cap * (sizeof(double) + sizeof(uint32_t)) +
                            (size_t)blockIdx.y * merge_block_lds<double, uint32_t>(KE)
                      : smem;
    double* bk = kbase + (size_t)wv * cap;
    uint32_t* bi = ibase + (size_t)wv * cap;
    // device-gated launch (qcount): the flagged queries are known only on the device;
    // query slots qi = blockIdx.y, + gridDim.y, ... below min(*qcount, nq_max)
    int nq = (int)gridDim.y;
    if (qcount) {
        const int c = *qcount;
        nq = c < nq_max ? c : nq_max;
        if (totals && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
            if (c) {
                atomicAdd(totals, (unsigned long long)c);
                if (tail.host_totals) {  // a bf16 search (VDB_PREC_AUTO): its own counter, mirrored to the host
                    const unsigned long long old = atomicAdd(totals + 2, (unsigned long long)c);
                    tail.host_totals[0] = old + (unsigned long long)c;
                }
            }
            if (ovf && *ovf) atomicAdd(totals + 1, (unsigned long long)*ovf);
        }
    }
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t r1 = r0 + rows_per_wg < N ? r0 + rows_per_wg : N;
    for (int qi = blockIdx.y; qi < nq; qi += gridDim.y) {
        const int b = qlist ? qlist[qi] : qi;
        const float* q = Q + (int64_t)b * D;
        const double qn = qn64[b];
        WaveTopK<double, uint32_t> tk;
        tk.init(bk, bi, KE);
        for (int64_t r = r0 + wv; r < r1; r += 4) {
            if (mask && !((mask[r >> 5] >> (r & 31)) & 1u)) continue;
            const double key = exact_key<METRIC>(q, qn, X, G, D, (uint64_t)r, nrm64[r]);
            tk.offer(lane == 0, key, (uint32_t)r);
        }
        tk.finish();
        __syncthreads();
        if (wv == 0) {
            for (int w = 1; w < 4; ++w) {
                const double* ok = kbase + (size_t)w * cap;
                const uint32_t* oi = ibase + (size_t)w * cap;
                for (int e0 = 0; e0 < KE; e0 += 64) {
                    const int e = e0 + lane;
                    const bool in = e < KE && oi[e] != 0xFFFFFFFFu;
                    tk.offer(in, in ? ok[e] : -INFINITY, in ? oi[e] : 0xFFFFFFFFu);
                }
            }
            tk.finish();
            const size_t base = ((size_t)qi * gridDim.x + blockIdx.x) * KE;
            for (int e = lane; e < KE; e += 64) {
                lk[base + e] = bk[e];
                li[base + e] = bi[e];
            }
        }
        __syncthreads();  // the LDS buffers are reused by the next query slot
        if (tail.done) {
            // the last workgroup of this query slot merges every workgroup's list (release:
            // wave 0's list stores before the count; acquire: the other lists after it)
            __shared__ int s_last;
            if (threadIdx.x == 0) {
                __threadfence();
                s_last = atomicAdd(tail.done + qi, 1) == (int)gridDim.x - 1;
            }
            __syncthreads();
            if (s_last) {
                __threadfence();
                const size_t q0 = (size_t)qi * gridDim.x * KE;
                merge_block<double, uint32_t>(lk + q0, li + q0, (int)gridDim.x, KE, KE, KE, tail.mk + (size_t)qi * KE,
                                              tail.mi + (size_t)qi * KE, mscr);
                __syncthreads();
                for (int e = threadIdx.x; e < tail.k; e += 256) {
                    const double key = tail.mk[(size_t)qi * KE + e];
                    const uint32_t r = tail.mi[(size_t)qi * KE + e];
                    const bool valid = r != 0xFFFFFFFFu;
                    const size_t o = (size_t)b * tail.k + e;
                    write_result(METRIC, key, valid ? global_row(tail.row_ids, (uint64_t)r, tail.index_offset) : 0,
                                 valid && key != -INFINITY, tail.out_s + o, tail.out_i + o,
                                 tail.out_k ? tail.out_k + o : nullptr);
                }
                __syncthreads();
            }
        }
    }
}

size_t exact_scan_scratch_bytes(int KE, int n_wg, int slots) {
    return (size_t)slots * n_wg * 4 * WaveTopK<double, uint32_t>::capacity(KE) * (sizeof(double) + sizeof(uint32_t)) +
           (size_t)slots * merge_block_lds<double, uint32_t>(KE) + 256;
}

hipError_t launch_exact_scan(int metric, int KE, const float* Q, const double* qn64, const int* qlist, int nq,
                             const float* X, int G, int D, const double* nrm64, const uint32_t* mask, int64_t N,
                             int n_wg, int64_t rows_per_wg, double* lk, uint32_t* li, hipStream_t st,
                             const int* qcount, const int* ovf, unsigned long long* totals, const ExactTail* tail,
                             int gate_slots, char* gscr) {
    size_t lds = (size_t)4 * WaveTopK<double, uint32_t>::capacity(KE) * (sizeof(double) + sizeof(uint32_t));
    ExactTail tl{};
    if (tail) {
        if (!qcount || KE > 1024) return hipErrorInvalidValue;  // the fused tail is the gated form's
        tl = *tail;
        lds = std::max(lds, merge_block_lds<double, uint32_t>(KE));
    }
    if (gscr) lds = 0;  // (the buffers in the workspace: exact_scan_scratch_bytes)
    if (lds > 160 * 1024) return hipErrorInvalidValue;
    // gated: a few query slots per row range, each looping over the flagged queries
    const dim3 grid(n_wg, qcount ? (nq < gate_slots ? nq : gate_slots) : nq);
    if (metric == 0)
        hipLaunchKernelGGL((exact_scan_kernel<0>), grid, dim3(256), lds, st, Q, qn64, qlist, X, G, D, nrm64, mask, N,
                           rows_per_wg, KE, lk, li, qcount, nq, ovf, totals, tl, gscr);
    else
        hipLaunchKernelGGL((exact_scan_kernel<1>), grid, dim3(256), lds, st, Q, qn64, qlist, X, G, D, nrm64, mask, N,
                           rows_per_wg, KE, lk, li, qcount, nq, ovf, totals, tl, gscr);
    return hipGetLastError();
}

}  // namespace vdb

#ifdef VDB_STAMP
extern "C" int vdb_debug_finish_stamps(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(vdb::g_fin_stamps), (size_t)n * 16 * sizeof(unsigned long long));
}
#endif
