// mmr_plan_check.cpp — the host arithmetic of vdb_index_search_mmr (csrc/vdb_mmr_plan.h) swept on the
// CPU against naive loops: the query-block size, the deal of (i < j) position pairs to workgroups and
// waves (every pair exactly once for every list length up to 200), the scratch layout, the validation,
// and the selection function against a naive greedy loop on inputs full of ties.  A stand-alone host
// program (its own main, no GPU, nothing loaded into another process); `make mmr-plan-check` builds
// it with -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/vdb_mmr_plan.h"

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

static void check_block() {
    for (int f = 1; f <= kMmrMaxFetch; ++f) {
        const int qb = mmr_query_block(f);
        const int64_t per = (int64_t)f * f * 8;
        const int64_t want = std::max<int64_t>(1, std::min<int64_t>(kMmrPairBytes / per, kMmrMaxBlock));
        CHECK(qb == want, "block %d, want %lld (fetch %d)", qb, (long long)want, f);
        CHECK(qb >= 1 && qb <= kMmrMaxBlock && qb <= 65535, "block %d is no grid dimension", qb);
        CHECK(qb == 1 || (int64_t)qb * per <= kMmrPairBytes, "block %d of fetch %d exceeds the bound", qb, f);
    }
    CHECK(mmr_query_block(200) == 209, "fetch 200 runs %d queries per block, want 209", mmr_query_block(200));
    CHECK(kMmrLanePos * 64 >= kMmrMaxFetch, "a wave's lanes do not hold %d positions", kMmrMaxFetch);
}

static void check_deal() {
    for (int F = 1; F <= kMmrMaxFetch; ++F) {
        std::vector<int> seen((size_t)F * F, 0);
        const int wgs = mmr_pair_wgs(F);
        CHECK(wgs >= 0 && (F < 2 || wgs > 0), "%d workgroups for %d positions", wgs, F);
        for (int wg = 0; wg < wgs; ++wg)
            for (int w = 0; w < kMmrWaves; ++w) {
                const MmrPairTask t = mmr_pair_task(F, wg, w);
                CHECK(t.j1 - t.j0 <= kMmrNB && t.j1 - t.j0 >= 0, "a batch of %d positions", t.j1 - t.j0);
                if (t.j0 >= t.j1) continue;
                CHECK(t.i >= 0 && t.i < F && t.j0 > t.i && t.j1 <= F, "task (%d, [%d, %d)) outside %d", t.i, t.j0,
                      t.j1, F);
                for (int j = t.j0; j < t.j1; ++j) ++seen[(size_t)t.i * F + j];
            }
        for (int i = 0; i < F; ++i)
            for (int j = 0; j < F; ++j)
                CHECK(seen[(size_t)i * F + j] == (i < j ? 1 : 0), "pair (%d, %d) of %d dealt %d times", i, j, F,
                      seen[(size_t)i * F + j]);
        // a workgroup past the last deals nothing
        for (int w = 0; w < kMmrWaves; ++w) {
            const MmrPairTask t = mmr_pair_task(F, wgs, w);
            CHECK(t.j0 >= t.j1, "workgroup %d of %d deals a pair", wgs, wgs);
        }
    }
}

static void check_scratch(std::mt19937& rng) {
    for (int trial = 0; trial < 20000; ++trial) {
        const int B = 1 + (int)(rng() % (trial % 5 ? 300 : 70000));
        const int dim = 1 + (int)(rng() % 3000);
        const int k = 1 + (int)(rng() % kMmrMaxK);
        const int F = k + (int)(rng() % (kMmrMaxFetch - k + 1));
        const int64_t rows = (int64_t)(rng() % 3 ? rng() % 100000 : rng() % 40);
        const bool host = rng() & 1, masked = rng() & 1, keys = rng() & 1, mmr = rng() & 1;
        const MmrScratch s = mmr_scratch(B, dim, k, F, rows, host, masked, keys, mmr);
        const int64_t qb = std::min<int64_t>(B, mmr_query_block(F));
        struct Span {
            int64_t at, bytes;
        };
        std::vector<Span> spans = {{s.fs, (int64_t)B * F * 4}, {s.fi, (int64_t)B * F * 8}, {s.fk, (int64_t)B * F * 8},
                                   {s.S, qb * F * F * 8}};
        CHECK(s.mask_words == (rows + 31) / 32, "mask words %lld for %lld rows", (long long)s.mask_words, (long long)rows);
        if (host) {
            spans.push_back({s.q, (int64_t)B * dim * 4});
            if (masked) spans.push_back({s.mask, (s.mask_words + 64) * 4});
            spans.push_back({s.out_s, (int64_t)B * k * 4});
            spans.push_back({s.out_i, (int64_t)B * k * 8});
            if (keys) spans.push_back({s.out_k, (int64_t)B * k * 8});
            if (mmr) spans.push_back({s.out_m, (int64_t)B * k * 8});
            CHECK(s.q >= s.in0 && s.q + (int64_t)B * dim * 4 <= s.in0 + s.in_bytes, "queries outside the upload");
            CHECK(!masked || s.mask + (s.mask_words + 64) * 4 <= s.in0 + s.in_bytes, "mask outside the upload");
            CHECK(s.out0 == s.in0 + s.in_bytes, "the download does not follow the upload");
            CHECK(s.out_s >= s.out0 && s.out0 + s.out_bytes == s.total, "results outside the download");
        } else {
            CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device-memory call stages %lld + %lld bytes",
                  (long long)s.in_bytes, (long long)s.out_bytes);
        }
        int64_t end = 0;
        for (const Span& p : spans) {  // in layout order: aligned, no overlap, inside the total
            CHECK(p.at % 256 == 0, "offset %lld is not 256-byte aligned", (long long)p.at);
            CHECK(p.at >= end, "a span at %lld overlaps one ending at %lld", (long long)p.at, (long long)end);
            end = p.at + p.bytes;
            CHECK(end <= s.total, "a span ends at %lld past the total %lld", (long long)end, (long long)s.total);
        }
    }
}

static void check_validate() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(mmr_validate(1, 1, 1, 0.5, true, true, true, 0) == kMmrOk, "a plain call refused");
    CHECK(mmr_validate(0, 200, 200, 0.0, true, true, true, 1) == kMmrOk, "no queries refused");
    CHECK(mmr_validate(-1, 1, 1, 0.5, true, true, true, 0) == kMmrBadQueries, "n_queries -1");
    for (int k = -2; k <= kMmrMaxK + 2; ++k)
        for (int f = -2; f <= kMmrMaxFetch + 2; ++f) {
            const int want = (k < 1 || k > kMmrMaxK) ? kMmrBadK : (f < k || f > kMmrMaxFetch) ? kMmrBadFetch : kMmrOk;
            CHECK(mmr_validate(3, k, f, 1.0, true, true, true, 0) == want, "k %d fetch %d", k, f);
        }
    for (double l : {-0.1, 1.1, nan, inf, -inf, std::nextafter(1.0, 2.0), -std::numeric_limits<double>::denorm_min()})
        CHECK(mmr_validate(1, 1, 1, l, true, true, true, 0) == kMmrBadLambda, "lambda %g accepted", l);
    for (double l : {0.0, -0.0, 1.0, 0.25, std::nextafter(1.0, 0.0)})
        CHECK(mmr_validate(1, 1, 1, l, true, true, true, 0) == kMmrOk, "lambda %g refused", l);
    CHECK(mmr_validate(1, 1, 1, 0.5, false, true, true, 0) == kMmrNullPointer, "NULL queries");
    CHECK(mmr_validate(1, 1, 1, 0.5, true, false, true, 0) == kMmrNullPointer, "NULL scores");
    CHECK(mmr_validate(1, 1, 1, 0.5, true, true, false, 0) == kMmrNullPointer, "NULL indices");
    CHECK(mmr_validate(1, 1, 1, 0.5, true, true, true, 2) == kMmrBadMem, "mem 2");
}

// The selection against the contract written out naively (its own value expression, its own tie
// loop), on similarities drawn from a few values so that ties are the rule.
static void check_select(std::mt19937& rng) {
    const double lambdas[] = {0.0, 0.25, 0.5, 1.0, std::nextafter(1.0, 0.0)};
    const double vals[] = {-1.0, -0.5, -0.0, 0.0, 0.5, 1.0};
    for (int trial = 0; trial < 3000; ++trial) {
        const int n = (int)(rng() % (trial % 10 ? 24 : 201));
        const int k = 1 + (int)(rng() % (trial % 3 ? 12 : kMmrMaxK));
        const int ld = n + (int)(rng() % 3);
        const double lambda = lambdas[rng() % 5];
        const bool ties = trial % 4 != 0;
        std::uniform_real_distribution<double> u(-1.0, 1.0);
        std::vector<double> rel(n), S((size_t)std::max(n, 1) * std::max(ld, 1));
        for (int i = 0; i < n; ++i) rel[i] = ties ? vals[rng() % 6] : u(rng);
        std::sort(rel.begin(), rel.end(), [](double a, double b) { return a > b; });
        for (int i = 0; i < n; ++i)
            for (int j = i; j < n; ++j) S[(size_t)i * ld + j] = S[(size_t)j * ld + i] = ties ? vals[rng() % 6] : u(rng);
        std::vector<int> pos(k, -7), want_pos;
        std::vector<double> mmr(k, 7.0), want_mmr, pen(n), npen(n);
        std::vector<unsigned char> picked(n), np(n, 0);
        const int m = mmr_select(n, k, lambda, rel.data(), S.data(), ld, pos.data(), mmr.data(), pen.data(), picked.data());
        for (int s = 0; s < std::min(k, n); ++s) {
            int best = -1;
            double bv = 0.0;
            if (s == 0) {
                best = 0;
                bv = lambda * rel[0];
            } else {
                for (int i = n - 1; i >= 0; --i) {  // descending: an equal value at a lower position replaces
                    if (np[i]) continue;
                    const double v = lambda * rel[i] - (1.0 - lambda) * npen[i];
                    if (best < 0 || v >= bv) {
                        best = i;
                        bv = v;
                    }
                }
            }
            want_pos.push_back(best);
            want_mmr.push_back(bv);
            np[best] = 1;
            for (int i = 0; i < n; ++i) {
                const double sv = S[(size_t)i * ld + best];
                npen[i] = s == 0 ? sv : (sv > npen[i] ? sv : npen[i]);
            }
        }
        CHECK(m == std::min(k, n), "%d picks, want %d", m, std::min(k, n));
        for (int s = 0; s < m; ++s) {
            CHECK(pos[s] == want_pos[s], "slot %d picks %d, want %d (n %d, lambda %g)", s, pos[s], want_pos[s], n, lambda);
            CHECK(mmr[s] == want_mmr[s] && std::signbit(mmr[s]) == std::signbit(want_mmr[s]), "slot %d value %g, want %g",
                  s, mmr[s], want_mmr[s]);
            if (lambda == 1.0) CHECK(pos[s] == s, "lambda 1 picks %d at slot %d", pos[s], s);
        }
        for (int s = m; s < k; ++s) CHECK(pos[s] == -7 && mmr[s] == 7.0, "slot %d past the picks written", s);
    }
    // the tie rule and the penalty update on their own
    CHECK(mmr_better(1.0, 5, 0.5, 1) && !mmr_better(0.5, 1, 1.0, 5), "value order");
    CHECK(mmr_better(0.0, 1, -0.0, 2) && !mmr_better(-0.0, 2, 0.0, 1), "equal zeros: the lower position");
    CHECK(std::signbit(mmr_pen_update(0.0, -0.0)) && !std::signbit(mmr_pen_update(-0.0, 0.0)),
          "the penalty keeps the old zero when the new one is not greater");
}

int main() {
    std::mt19937 rng(20240917);
    check_block();
    check_deal();
    check_scratch(rng);
    check_validate();
    check_select(rng);
    std::printf("mmr plan ok (%ld checks)\n", g_checks);
    return 0;
}
