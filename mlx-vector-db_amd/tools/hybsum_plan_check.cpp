// hybsum_plan_check.cpp — the host arithmetic of vdb_index_search_hybrid_sum (csrc/vdb_hybsum_plan.h)
// swept on the CPU against naive loops: the deal of rows to segments, waves and lanes and of a wave's
// rows to the batches of the dense keys (every row exactly once, lane 4 t + u keeps its own row), the
// workgroups per query, the scratch layout (aligned, disjoint, inside the total), the LDS budget, the
// validation of a call, one cause at a time, and the combination of a row's two keys, -0.0 and both
// zero weights included.  A stand-alone host program (its own main, no GPU, nothing loaded into
// another process); `make hybsum-plan-check` builds it with -fsanitize=address,undefined and
// -ffp-contract=off and runs it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/vdb_hybsum_plan.h"

using namespace vdb;

static long g_checks = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        ++g_checks;                           \
        if (!(cond)) {                        \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");       \
            std::exit(1);                     \
        }                                     \
    } while (0)

static const double kNan = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();

static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

static void check_deal() {
    CHECK(kSparseWaveRows % kHybsumNB == 0, "a wave's rows do not split into whole batches");
    for (int64_t N : {0, 1, 3, 37, 63, 64, 65, 255, 256, 257, 513, 1300, 5000}) {
        const int64_t chunks = sparse_n_chunks(N);
        for (int n_seg : {1, 2, 7, 64, 512}) {
            const int live = sparse_live_segs(N, n_seg);
            CHECK(live == (int)std::min<int64_t>(chunks, n_seg), "live segments N %lld n_seg %d", (long long)N, n_seg);
            std::vector<int> sparse_seen((size_t)N, 0), dense_seen((size_t)N, 0);
            for (int s = 0; s < live; ++s)
                for (int64_t c = s; c < chunks; c += n_seg)
                    for (int wv = 0; wv < kSparseWaves; ++wv) {
                        // the lanes' own rows (the sparse walk, the offer)
                        for (int lane = 0; lane < kSparseWaveRows; ++lane) {
                            const int64_t r = sparse_row_of(c, wv, lane);
                            if (r < N) ++sparse_seen[(size_t)r];
                        }
                        // the batches of the dense keys: batch t, slot u is the row of lane NB t + u
                        const int64_t w0 = sparse_row_of(c, wv, 0);
                        for (int t = 0; t < kSparseWaveRows / kHybsumNB; ++t)
                            for (int u = 0; u < kHybsumNB; ++u) {
                                const int lane = t * kHybsumNB + u;
                                const int64_t r = w0 + t * kHybsumNB + u;
                                CHECK(r == sparse_row_of(c, wv, lane), "batch %d slot %d is not lane %d's row", t, u, lane);
                                CHECK(hybsum_batch_of(lane) == t && hybsum_slot_of(lane) == u, "lane %d", lane);
                                if (r < N) ++dense_seen[(size_t)r];
                            }
                    }
            for (int s = live; s < n_seg; ++s) CHECK(s >= chunks, "segment %d of %d has a chunk", s, n_seg);
            for (int64_t r = 0; r < N; ++r)
                CHECK(sparse_seen[(size_t)r] == 1 && dense_seen[(size_t)r] == 1, "row %lld seen %d / %d times", (long long)r,
                      sparse_seen[(size_t)r], dense_seen[(size_t)r]);
        }
    }
    // the knob and the auto rule
    for (int64_t N : {0, 1, 256, 257, 100000, 1000000})
        for (int B : {1, 5, 64, 2000, kHybsumMaxQueries}) {
            const int a = hybsum_n_seg(0, N, B, 256);
            CHECK(a == sparse_n_seg(0, N, B, 256), "auto differs from the sparse search's");
            CHECK(a >= 1 && a <= kHybsumMaxSeg, "auto n_seg %d", a);
            CHECK(a <= std::max<int64_t>(1, sparse_n_chunks(N)), "more segments than chunks");
            CHECK((int64_t)a * B <= std::max<int64_t>(B, 256 * kSparseWgPerCu), "grid too large: %d x %d", a, B);
            for (int64_t knob : {1, 2, 7, 512, 9999})
                CHECK(hybsum_n_seg(knob, N, B, 256) == (int)std::min<int64_t>(knob, kHybsumMaxSeg), "knob %lld", (long long)knob);
        }
    // the dense key's form
    for (int d = 1; d <= 4100; ++d) CHECK(hybsum_mp(d) == (d <= 1024 ? 4 : d <= 2048 ? 8 : 0), "mp of dim %d", d);
    // the pieces of a row (256 dims each) fit the registers of the chosen form
    for (int d : {1, 16, 256, 257, 260, 1024, 1025, 1100, 2048})
        CHECK((d + 255) / 256 <= hybsum_mp(d), "dim %d has more pieces than its form holds", d);
}

static void check_ranges_disjoint(const std::vector<std::pair<int64_t, int64_t>>& r, int64_t total, const char* what) {
    for (size_t i = 0; i < r.size(); ++i) {
        CHECK(r[i].first % 256 == 0, "%s: offset %lld not aligned", what, (long long)r[i].first);
        CHECK(r[i].first >= 0 && r[i].first + r[i].second <= total, "%s: range %zu outside the total", what, i);
        for (size_t j = 0; j < i; ++j)
            CHECK(r[i].second == 0 || r[j].second == 0 || r[i].first >= r[j].first + r[j].second ||
                      r[j].first >= r[i].first + r[i].second,
                  "%s: ranges %zu and %zu overlap", what, i, j);
    }
}

static void check_scratch() {
    for (int B : {1, 5, 64, kHybsumMaxQueries})
        for (int dim : {1, 16, 768, 2100})
            for (int k : {1, 10, 200, 1024})
                for (int n_seg : {1, 2, 7, 512})
                    for (int64_t q_nnz : {0, 1, 1024, 70000})
                        for (int64_t rows : {0, 3, 1300, 1000000})
                            for (int flags = 0; flags < 32; ++flags) {
                                if (B == kHybsumMaxQueries && (n_seg > 2 || (flags & 0x1c) != 0x1c)) continue;  // (keeps the sweep short)
                                const bool host = flags & 1, masked = flags & 2, fused = flags & 4, dense = flags & 8,
                                           sparse = flags & 16;
                                const int64_t KE = sparse_ke(k);
                                const HybsumScratch s = hybsum_scratch(B, dim, k, n_seg, q_nnz, rows, host, masked, fused, dense, sparse);
                                std::vector<std::pair<int64_t, int64_t>> r = {
                                    {s.done, (int64_t)B * 4},
                                    {s.qn64, (int64_t)B * 8},
                                    {s.lk, n_seg > 1 ? (int64_t)B * n_seg * KE * 8 : 0},
                                    {s.li, n_seg > 1 ? (int64_t)B * n_seg * KE * 4 : 0},
                                    {s.mk, n_seg > 1 ? B * KE * 8 : 0},
                                    {s.mi, n_seg > 1 ? B * KE * 4 : 0},
                                    {s.rows, dense || sparse ? (int64_t)B * k * 4 : 0}};
                                if (host) {
                                    r.push_back({s.q, (int64_t)B * dim * 4});
                                    r.push_back({s.indptr, ((int64_t)B + 1) * 8});
                                    r.push_back({s.terms, q_nnz * 4});
                                    r.push_back({s.weights, q_nnz * 4});
                                    r.push_back({s.mask, masked ? s.mask_words * 4 : 0});
                                    r.push_back({s.out_s, (int64_t)B * k * 4});
                                    r.push_back({s.out_i, (int64_t)B * k * 8});
                                    r.push_back({s.out_f, fused ? (int64_t)B * k * 8 : 0});
                                    r.push_back({s.out_d, dense ? (int64_t)B * k * 8 : 0});
                                    r.push_back({s.out_p, sparse ? (int64_t)B * k * 8 : 0});
                                    CHECK(s.in0 <= s.q && s.mask + (masked ? s.mask_words * 4 : 0) <= s.in0 + s.in_bytes,
                                          "staged arguments outside [in0, in0 + in_bytes)");
                                    CHECK(s.out0 == s.in0 + s.in_bytes && s.out0 + s.out_bytes == s.total, "staging not back to back");
                                    CHECK(s.out0 <= s.out_s, "results before out0");
                                } else {
                                    CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device call stages");
                                }
                                CHECK(s.mask_words == (rows + 31) / 32, "mask words");
                                check_ranges_disjoint(r, s.total, "hybrid-sum scratch");
                            }
    // LDS: the query and the four buffers at k = 1024 (capacity 2048 entries of 12 bytes): 104 KiB, inside 160 KiB
    CHECK(hybsum_lds_bytes(2048, 2048 * 12) == 8192 + 4 * 2048 * 12, "LDS at k = 1024");
    CHECK(hybsum_lds_bytes(2048, 2048 * 12) == 104 * 1024 && hybsum_lds_bytes(2048, 2048 * 12) <= 160 * 1024, "LDS budget");
    CHECK(hybsum_lds_bytes(128, 1024 * 12) == 8192 + 1024 * 12, "the merge buffer is the larger at k = 32");
}

static void check_calls() {
    auto v = [](int64_t B, int64_t nnz, int k, double wd = 1.0, double ws = 1.0, bool q = true, bool ip = true, bool t = true,
                bool w = true, bool s = true, bool i = true, int mem = 0, bool col = true) {
        return hybsum_validate_call(B, nnz, k, wd, ws, q, ip, t, w, s, i, mem, col);
    };
    CHECK(v(3, 10, 10) == kHybsumOk, "a plain call refused");
    CHECK(v(0, 0, 1, 1.0, 1.0, false, false, false, false, false, false, 1) == kHybsumOk, "an empty call refused");
    CHECK(v(3, 0, 10, 1.0, 1.0, true, true, false, false) == kHybsumOk, "queries without terms need no arrays");
    CHECK(v(-1, 0, 1) == kHybsumBadCounts && v(1, -1, 1) == kHybsumBadCounts, "counts");
    for (int k = -2; k <= kHybsumMaxK + 2; ++k)
        CHECK(v(1, 1, k) == ((k < 1 || k > kHybsumMaxK) ? kHybsumBadK : kHybsumOk), "k %d", k);
    CHECK(v(1, 1, 1, 1.0, 1.0, false) == kHybsumNullPointer, "NULL dense queries");
    CHECK(v(1, 1, 1, 1.0, 1.0, true, false) == kHybsumNullPointer && v(1, 1, 1, 1.0, 1.0, true, true, false) == kHybsumNullPointer &&
              v(1, 1, 1, 1.0, 1.0, true, true, true, false) == kHybsumNullPointer &&
              v(1, 1, 1, 1.0, 1.0, true, true, true, true, false) == kHybsumNullPointer &&
              v(1, 1, 1, 1.0, 1.0, true, true, true, true, true, false) == kHybsumNullPointer,
          "NULL pointers");
    for (int mem : {-1, 2, 7}) CHECK(v(1, 1, 1, 1.0, 1.0, true, true, true, true, true, true, mem) == kHybsumBadMem, "mem %d", mem);
    CHECK(v(1, 1, 1, 1.0, 1.0, true, true, true, true, true, true, 1) == kHybsumOk, "device memory refused");
    CHECK(v(1, 1, 1, 1.0, 1.0, true, true, true, true, true, true, 0, false) == kHybsumNoColumn, "no column");
    CHECK(v(kHybsumMaxQueries, 1, 1) == kHybsumOk && v(kHybsumMaxQueries + 1, 1, 1) == kHybsumTooManyQueries, "n_queries cap");
    // the weights: [0, 2^64], NaN refused
    const double top = kHybsumMaxWeight;
    CHECK(top == std::ldexp(1.0, 64), "the cap is not 2^64");
    for (double x : {0.0, -0.0, 1e-300, 0.3, 1.0, 1e19, top})
        CHECK(v(1, 1, 1, x, 1.0) == kHybsumOk && v(1, 1, 1, 1.0, x) == kHybsumOk && hybsum_weight_ok(x), "weight %g refused", x);
    for (double x : {-1.0, -1e-300, kNan, kInf, -kInf, std::nextafter(top, kInf), 1e300})
        CHECK(v(1, 1, 1, x, 1.0) == kHybsumBadWeight && v(1, 1, 1, 1.0, x) == kHybsumBadWeight && !hybsum_weight_ok(x),
              "weight %g accepted", x);
    CHECK(v(1, 1, 1, 0.0, 0.0) == kHybsumOk, "both zero weights refused");
}

static void check_combine() {
    std::mt19937_64 rng(3);
    std::uniform_real_distribution<double> u(-4.0, 4.0);
    const double ws[] = {0.0, 0.3, 0.7, 1.0, 2.0, kHybsumMaxWeight};
    for (int trial = 0; trial < 20000; ++trial) {
        const double kd = u(rng), ks = u(rng) * 9.0, wd = ws[rng() % 6], wsp = ws[rng() % 6];
        // the naive form: four separate operations through volatile, so nothing is fused or folded
        volatile double t1 = wd * kd;
        volatile double t2 = wsp * ks;
        volatile double s = t1 + t2;
        volatile double c = s + 0.0;
        const double got = hybsum_combine(wd, kd, wsp, ks);
        CHECK(bits(got) == bits(c), "combine(%a, %a, %a, %a) = %a, naive %a", wd, kd, wsp, ks, got, (double)c);
        CHECK(!(got == 0.0 && std::signbit(got)), "a value of -0.0");
        CHECK(std::isfinite(got), "a value that is not finite");
    }
    // -0.0 becomes +0.0: the euclidean key of an exact match, products with a zero weight and a negative key
    for (double wd : {0.0, 1.0, kHybsumMaxWeight})
        for (double wsp : {0.0, 1.0, kHybsumMaxWeight})
            for (double kd : {-0.0, 0.0}) {
                const double got = hybsum_combine(wd, kd, wsp, 0.0);
                CHECK(bits(got) == 0, "combine(%g, %g, %g, 0) is not +0.0", wd, kd, wsp);
            }
    CHECK(bits(hybsum_combine(0.0, -0.5, 0.0, 0.0)) == 0 && bits(hybsum_combine(0.0, -0.5, 0.0, -3.0)) == 0, "both zero weights");
    CHECK(bits(hybsum_combine(0.0, -0.5, 0.0, 7.0)) == 0 && bits(hybsum_combine(0.0, 0.5, 0.0, 7.0)) == 0, "both zero weights");
    // one zero weight leaves the other key (+ 0.0)
    CHECK(bits(hybsum_combine(1.0, -0.25, 0.0, 9.0)) == bits(-0.25) && bits(hybsum_combine(0.0, -0.25, 1.0, 9.0)) == bits(9.0),
          "a zero weight");
    CHECK(bits(hybsum_combine(0.0, -0.25, 1.0, -9.0)) == bits(-9.0) && bits(hybsum_combine(1.0, 0.5, 0.0, -9.0)) == bits(0.5),
          "a zero weight");
    // the greatest weights with the greatest keys: finite, and no inf - inf
    const double big = std::ldexp(1.0, 279);
    for (double a : {-big, big})
        for (double b : {-big, big}) {
            const double got = hybsum_combine(kHybsumMaxWeight, a, kHybsumMaxWeight, b);
            CHECK(std::isfinite(got), "2^64 * %a + 2^64 * %a is not finite", a, b);
        }
    CHECK(hybsum_combine(kHybsumMaxWeight, big, kHybsumMaxWeight, -big) == 0.0, "cancelling products");
    // a fused multiply-add would differ here: t1 is rounded before the sum
    const double a = 1.0 + std::ldexp(1.0, -30);
    volatile double p = a * a;
    volatile double q = -(1.0 + std::ldexp(1.0, -29));
    CHECK(bits(hybsum_combine(a, a, 1.0, q)) == bits((double)p + (double)q + 0.0), "the product is not rounded on its own");
    CHECK(hybsum_combine(a, a, 1.0, q) == 0.0 && std::fma(a, a, (double)q) != 0.0, "the case does not tell a fused form apart");
}

int main() {
    check_deal();
    check_scratch();
    check_calls();
    check_combine();
    std::printf("hybsum plan ok (%ld checks)\n", g_checks);
    return 0;
}
