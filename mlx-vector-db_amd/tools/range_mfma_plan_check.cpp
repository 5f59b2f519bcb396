// range_mfma_plan_check.cpp — the arithmetic of the MFMA form of the range scan
// (csrc/vdb_range_mfma_plan.h) swept on the CPU.  Stand-alone: build with -fsanitize=address,undefined
// and -ffp-contract=off (make range-mfma-plan-check) and run.
//
//   layout    the loads of a K chunk, the LDS positions, the operand reads and the accumulator rows
//             are replayed on heap blocks of exactly the kernel's sizes: an index that is off is a
//             sanitizer report, an element moved twice or never is a mismatch reported here.
//   decision  range_mfma_decide against the canonical fp64 key (the order of csrc/vdb_common.h
//             restated here) for fp32 dot products summed in three orders, with round-to-nearest,
//             with truncation and with denormals flushed, at bounds on, beside and around the key,
//             for ordinary, tiny, huge, clamped and coinciding vectors: a hit or a miss it declares
//             must be the key's own answer.
#include <algorithm>
#include <cfenv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/vdb_range_mfma_plan.h"

using namespace vdb;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                   \
            std::fprintf(stderr, "\n");                                          \
            if (++g_fail > 20) std::exit(1);                                     \
        }                                                                        \
    } while (0)

template <typename T>
T* exact_alloc(size_t n) {
    return (T*)std::calloc(n ? n : 1, sizeof(T));
}

// ---- layout -----------------------------------------------------------------------------------------
void check_layout() {
    const int ST = kRangeMfmaLdsStride, KC = kRangeMfmaKC;
    CHECK(range_mfma_lds_bytes() <= kRangeMfmaLdsLimit, "LDS %lld bytes", (long long)range_mfma_lds_bytes());
    CHECK(kRangeMfmaXLoads * 64 * 4 == kRangeMfmaPassRows * KC && kRangeMfmaQLoads * 256 == kRangeMfmaQB * KC, "loads per chunk");
    // a wave's row chunk: every (row, float) of [64][KC] lands once, inside the wave's LDS block
    int* sx = exact_alloc<int>((size_t)range_mfma_lds_x_floats());
    for (int i = 0; i < kRangeMfmaXLoads; ++i)
        for (int lane = 0; lane < 64; ++lane) {
            const int r = range_mfma_xload_row(i, lane), col = range_mfma_xload_col(lane);
            CHECK(r >= 0 && r < kRangeMfmaPassRows && col >= 0 && col + 4 <= KC && col % 4 == 0, "load (%d, %d) -> row %d col %d", i, lane, r, col);
            CHECK(r / 32 == i / (kRangeMfmaXLoads / kRangeMfmaPassTiles), "load %d crosses its tile", i);
            for (int e = 0; e < 4; ++e) sx[r * ST + col + e] += 1 + r * KC + col + e;
        }
    for (int r = 0; r < kRangeMfmaPassRows; ++r)
        for (int k = 0; k < KC; ++k) CHECK(sx[r * ST + k] == 1 + r * KC + k, "row %d float %d stored %d", r, k, sx[r * ST + k]);
    // the queries' chunk
    int* sq = exact_alloc<int>((size_t)range_mfma_lds_q_floats());
    for (int i = 0; i < kRangeMfmaQLoads; ++i)
        for (int t = 0; t < 256; ++t) {
            const int idx = i * 256 + t;
            sq[(idx / KC) * ST + idx % KC] += 1 + idx;
        }
    for (int j = 0; j < kRangeMfmaQB; ++j)
        for (int k = 0; k < KC; ++k) CHECK(sq[j * ST + k] == 1 + j * KC + k, "query %d float %d", j, k);
    // operand reads: every float of a row's chunk feeds one MFMA K slot, the same slot for both operands,
    // and the 16-byte reads of 16 consecutive lanes cover 64 distinct banks
    for (int tile = 0; tile < kRangeMfmaPassTiles; ++tile) {
        std::vector<int> used((size_t)KC, 0);
        for (int s = 0; s < kRangeMfmaSteps; ++s)
            for (int h = 0; h < 2; ++h) {
                const int col = range_mfma_operand_col(s, h);
                CHECK(col % 4 == 0 && col + 4 <= KC, "operand col %d", col);
                for (int e = 0; e < 4; ++e) used[(size_t)(col + e)]++;
                for (int g = 0; g < 2; ++g) {
                    std::vector<int> bank(64, 0);
                    for (int c = 16 * g; c < 16 * g + 16; ++c) {
                        const int at = (tile * 32 + c) * ST + col;
                        CHECK(sx[at] && sx[at + 3] && sq[at + 3], "read at %d", at);  // (inside both blocks)
                        for (int e = 0; e < 4; ++e) bank[(size_t)((at + e) % 64)]++;
                    }
                    for (int b = 0; b < 64; ++b) CHECK(bank[(size_t)b] == 1, "bank %d read %d times", b, bank[(size_t)b]);
                }
            }
        for (int k = 0; k < KC; ++k) CHECK(used[(size_t)k] == 1, "float %d feeds %d slots", k, used[(size_t)k]);
    }
    std::free(sx);
    std::free(sq);
    // accumulators: the two lane halves hold each of the 32 rows once
    std::vector<int> rows(32, 0);
    for (int h = 0; h < 2; ++h)
        for (int v = 0; v < 16; ++v) {
            const int i = range_mfma_acc_row(v, h);
            CHECK(i >= 0 && i < 32, "accumulator row %d", i);
            rows[(size_t)i]++;
        }
    for (int i = 0; i < 32; ++i) CHECK(rows[(size_t)i] == 1, "row %d held %d times", i, rows[(size_t)i]);
    // passes: a wave's words, each once, the fp64 scan's words
    for (int64_t chunk : {(int64_t)0, (int64_t)5, (int64_t)1 << 30})
        for (int wv = 0; wv < kRangeMfmaWaves; ++wv) {
            int n = 0;
            for (int p = 0; p < kRangeMfmaPasses; ++p)
                for (int t = 0; t < kRangeMfmaPassTiles; ++t, ++n)
                    CHECK(range_mfma_pass_word(chunk, wv, p) + t == range_wave_word(chunk, wv, n), "pass %d tile %d", p, t);
            CHECK(n == kRangeWaveWords, "words of a wave");
        }
    for (int Dp : {8, 24, 32, 40, 64, 768, 2112})
        CHECK(range_mfma_k_chunks(Dp) * KC >= Dp && (range_mfma_k_chunks(Dp) - 1) * KC < Dp, "K chunks of %d", Dp);
}

// ---- which form, block, scratch -----------------------------------------------------------------------
void check_host() {
    for (int64_t knob = -1; knob <= 3; ++knob) CHECK(range_mfma_knob_ok(knob) == (knob >= 0 && knob <= 2), "knob %lld", (long long)knob);
    for (int B : {0, 1, 8, 63, 64, 65, 256, 100000})
        for (int D : {0, 1, 768, kRangeMfmaMaxDim, kRangeMfmaMaxDim + 1}) {
            const bool can = B >= 1 && D >= 1 && D <= kRangeMfmaMaxDim;
            CHECK(!range_use_mfma(2, B, D), "never");
            CHECK(range_use_mfma(1, B, D) == can, "always: %d x %d", B, D);
            CHECK(range_use_mfma(0, B, D) == (can && kRangeMfmaMinQueries > 0 && B >= kRangeMfmaMinQueries), "auto: %d x %d", B, D);
            const int blk = range_mfma_block(B);
            CHECK(blk >= 1 && blk <= kRangeMfmaQB && blk <= std::max(B, 1) && (blk == kRangeMfmaQB || blk >= B), "block %d of %d", blk, B);
        }
    for (int B : {1, 33, 64, 65, 200})
        for (int dim : {1, 768, 2100, 40000})
            for (int64_t N : {(int64_t)1, (int64_t)513, (int64_t)100000})
                for (int flags = 0; flags < 8; ++flags) {
                    const int64_t cap = flags & 4 ? 77 : 0;
                    const RangeScratch s = range_mfma_scratch(B, dim, N, cap, flags & 1, flags & 2, true);
                    CHECK(s.block == range_mfma_block(B), "scratch block %d", s.block);
                    const int64_t regs[][2] = {{s.qn64, (int64_t)B * 8}, {s.H, (int64_t)s.block * s.n_words * 4},
                                               {s.part, (int64_t)s.block * s.n_chunks * 4}, {s.cnt, (int64_t)s.block * 8}};
                    char* mem = exact_alloc<char>((size_t)s.total);
                    int64_t end = 0;
                    for (const auto& r : regs) {
                        CHECK(r[0] % 256 == 0 && r[0] >= end && r[0] + r[1] <= s.total, "region at %lld + %lld", (long long)r[0], (long long)r[1]);
                        std::fill(mem + r[0], mem + r[0] + r[1], 1);
                        end = r[0] + r[1];
                    }
                    std::free(mem);
                }
}

// ---- decision ---------------------------------------------------------------------------------------
// The canonical order (csrc/vdb_common.h): lane l owns pieces p = 64 m + l, accumulates in (m, j)
// order with separate multiply and add, then the xor butterfly 32 .. 1.
template <typename F>
double canonical_sum(int D, F term) {
    double acc[64];
    const int np = (D + 255) / 256;
    for (int l = 0; l < 64; ++l) {
        acc[l] = 0.0;
        for (int m = 0; m < np; ++m)
            for (int j = 0; j < 4; ++j) {
                const int d = 4 * (64 * m + l) + j;
                acc[l] = acc[l] + (d < D ? term(d) : 0.0);
            }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        double nx[64];
        for (int l = 0; l < 64; ++l) nx[l] = acc[l] + acc[l ^ off];
        std::copy(nx, nx + 64, acc);
    }
    return acc[0];
}
double canonical_norm(const std::vector<float>& v) {
    return std::sqrt(canonical_sum((int)v.size(), [&](int d) { return (double)v[(size_t)d] * (double)v[(size_t)d]; }));
}
double canonical_key(int metric, const std::vector<float>& q, const std::vector<float>& x, double qn, double xn) {
    const int D = (int)q.size();
    if (metric == 0) {
        const double acc = canonical_sum(D, [&](int d) { return (double)q[(size_t)d] * (double)x[(size_t)d]; });
        return acc / (std::fmax(qn, 1e-8) * std::fmax(xn, 1e-8));
    }
    return -canonical_sum(D, [&](int d) {
        const double df = (double)x[(size_t)d] - (double)q[(size_t)d];
        return df * df;
    });
}
float ftz(float v) { return std::fabs(v) < 0x1p-126f ? 0.0f : v; }
// An fp32 dot product: order 0 = ascending, 1 = the kernel's K slots (pairs 4 apart), 2 = descending;
// flush: denormal operands, products and sums become zero.  The rounding mode is the caller's.
float dot32(const std::vector<float>& q, const std::vector<float>& x, int order, bool flush) {
    const int D = (int)q.size();
    volatile float acc = 0.0f;
    auto step = [&](int d) {
        if (d >= D) return;
        volatile float a = q[(size_t)d], b = x[(size_t)d];
        if (flush) a = ftz(a), b = ftz(b);
        volatile float p = a * b;
        if (flush) p = ftz(p);
        acc = acc + p;
        if (flush) acc = ftz(acc);
    };
    if (order == 0)
        for (int d = 0; d < D; ++d) step(d);
    else if (order == 2)
        for (int d = D - 1; d >= 0; --d) step(d);
    else
        for (int d0 = 0; d0 < D; d0 += 8)
            for (int e = 0; e < 4; ++e) step(d0 + e), step(d0 + 4 + e);
    return acc;
}

int64_t g_pairs = 0, g_undecided = 0;
void check_pair(int metric, const std::vector<float>& q, const std::vector<float>& x, std::mt19937_64& rng, bool count) {
    const int D = (int)q.size();
    const double qn = canonical_norm(q), xn = canonical_norm(x);
    const double key = canonical_key(metric, q, x, qn, xn);
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> kts = {key, std::nextafter(key, inf), std::nextafter(key, -inf), key * (1 + 1e-12), key * (1 - 1e-12),
                               key * (1 + 1e-7), key * (1 - 1e-7), key * 1.001, key * 0.999, key + 1e-3, key - 1e-3,
                               0.0, -0.0, 1e-300, -1e-300, inf, -inf, 0.5, -0.5, 2.0 * key, 0.5 * key};
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (int i = 0; i < 4; ++i) kts.push_back(key + std::fabs(key) * u(rng) * std::ldexp(1.0, -8 * i - 10));
    const int modes[] = {FE_TONEAREST, FE_TOWARDZERO};
    for (int mode : modes)
        for (int order = 0; order < 3; ++order)
            for (int flush = 0; flush < 2; ++flush) {
                std::fesetround(mode);
                const float a = dot32(q, x, order, flush != 0);
                std::fesetround(FE_TONEAREST);
                for (double kt : kts) {
                    if (metric == 1 && kt > 0.0) kt = -kt;  // a euclidean bound is -(t t)
                    const int d = range_mfma_decide(metric, a, kt, qn, xn, D);
                    const bool truth = key >= kt;
                    CHECK(d != kRangeMfmaHit || truth, "metric %d D %d: hit declared, key %.17g bound %.17g a %.9g", metric, D, key, kt, (double)a);
                    CHECK(d != kRangeMfmaMiss || !truth, "metric %d D %d: miss declared, key %.17g bound %.17g a %.9g", metric, D, key, kt, (double)a);
                    if (!std::isfinite(a)) CHECK(d == kRangeMfmaExact, "a non-finite dot product was decided");
                }
                if (count && mode == FE_TONEAREST && !flush) {  // the fast path is the common path: a bound a hundredth away
                    const double kt = metric == 0 ? key - 0.01 : key * 1.01;
                    ++g_pairs;
                    g_undecided += range_mfma_decide(metric, a, kt, qn, xn, D) == kRangeMfmaExact;
                }
            }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(range_mfma_decide(metric, 1.0f, nan, qn, xn, D) == kRangeMfmaMiss, "a NaN bound");
    for (float bad : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()})
        for (double kt : {-1.0, 0.0, -inf, metric == 0 ? inf : -1e300})
            CHECK(range_mfma_decide(metric, bad, kt, qn, xn, D) == kRangeMfmaExact, "non-finite a decided at bound %g", kt);
}

void check_decisions() {
    std::mt19937_64 rng(424242);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    for (int D : {1, 2, 7, 33, 260, 768, 2100}) {
        const int reps = D > 1000 ? 6 : 20;
        for (int rep = 0; rep < reps; ++rep)
            for (int kind = 0; kind < 8; ++kind) {
                std::vector<float> q((size_t)D), x((size_t)D);
                for (auto& v : q) v = nd(rng);
                for (auto& v : x) v = nd(rng);
                float sq = 1.0f, sx = 1.0f;
                switch (kind) {
                    case 1: sq = sx = 0x1p-70f; break;                  // products underflow
                    case 2: sq = sx = 0x1p63f; break;                   // sums overflow
                    case 3: sx = 0x1p-40f; break;                       // a row under the cosine clamp
                    case 4: x = q; break;                               // the row is the query
                    case 5: x = q; x[(size_t)(rep % D)] = std::nextafter(x[(size_t)(rep % D)], 10.0f); break;
                    case 6: sq = 0x1p-100f, sx = 0x1p-30f; break;       // denormal operands beside normal ones
                    case 7: std::fill(x.begin(), x.end(), 0.0f); break; // a zero row
                    default: break;
                }
                for (auto& v : q) v *= sq;
                for (auto& v : x) v *= sx;
                for (int metric = 0; metric < 2; ++metric) check_pair(metric, q, x, rng, kind == 0 && D >= 33);
            }
    }
    CHECK(g_pairs > 0 && g_undecided * 50 <= g_pairs, "%lld of %lld ordinary pairs undecided a hundredth from the bound",
          (long long)g_undecided, (long long)g_pairs);
}

}  // namespace

int main() {
    check_layout();
    check_host();
    check_decisions();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("range mfma plan ok: %lld pairs decided, %lld undecided a hundredth from the bound\n", (long long)g_pairs,
                (long long)g_undecided);
    return 0;
}
