// jaccard_range_plan_check.cpp — the host arithmetic of vdb_index_search_jaccard_range
// (csrc/vdb_jaccard_range_plan.h) swept on the CPU against naive loops: the threshold test against
// 128-bit cross-multiplication (every i <= u <= 64 against every threshold of small denominators and of
// the largest, and the extremes i = u = 8 192, den = 2^18), what makes a threshold bad and the pair that
// stands in for one, the block size and LDS layouts of the two scans (disjoint, aligned, two workgroups
// inside the budget at the longest code), the scratch layout (aligned, disjoint, inside the total), the
// validation causes and the choice of scan.  A stand-alone host program (its own main, no GPU, nothing
// loaded into another process); `make jaccard-range-plan-check` builds it with
// -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../csrc/vdb_jaccard_range_plan.h"

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

// The definition: i / u >= num / den by cross-multiplication in 128 bits, u == 0 as 1 / 1.
static bool naive_pass(int i, int u, int num, int den) {
    if (u == 0) i = u = 1;
    return (__int128)i * den >= (__int128)num * u;
}

static void check_pass() {
    const int max_bits = kHamMaxBytes * 8;
    std::vector<int> dens;
    for (int d = 1; d <= 130; ++d) dens.push_back(d);
    for (int d : {8191, 8192, 8193, 65535, 65536, kJacRangeMaxDen - 1, kJacRangeMaxDen}) dens.push_back(d);
    for (int den : dens) {
        std::vector<int> nums;
        if (den <= 130)
            for (int n = 0; n <= den; ++n) nums.push_back(n);
        else
            for (int n : {0, 1, den / 3, den / 2 - 1, den / 2, den / 2 + 1, den - 1, den}) nums.push_back(n);
        for (int num : nums) {
            CHECK(!jac_range_bad_threshold(num, den), "%d / %d is a threshold", num, den);
            for (int u = 0; u <= 64; ++u)
                for (int i = 0; i <= u; ++i)
                    CHECK(jac_range_pass(i, u, num, den) == naive_pass(i, u, num, den), "i %d u %d against %d / %d", i, u, num, den);
            // the largest sets: the products reach 2^31
            for (int u : {max_bits - 1, max_bits})
                for (int i : {0, 1, u / 2, u - 1, u})
                    CHECK(jac_range_pass(i, u, num, den) == naive_pass(i, u, num, den), "i %d u %d against %d / %d", i, u, num, den);
        }
    }
    CHECK(jac_range_pass(max_bits, max_bits, kJacRangeMaxDen, kJacRangeMaxDen), "2^31 >= 2^31");
    CHECK(!jac_range_pass(max_bits - 1, max_bits, kJacRangeMaxDen, kJacRangeMaxDen), "one bit short of 1");
    CHECK(jac_range_pass(0, 0, 1, 1) && jac_range_pass(0, 0, kJacRangeMaxDen, kJacRangeMaxDen), "two empty sets are identical");
    CHECK(jac_range_pass(2, 4, 1, 2) && jac_range_pass(3, 6, 1 << 17, 1 << 18) && !jac_range_pass(3, 7, 1, 2), "at and below a half");
    // the stand-in of a bad threshold and of an absent query passes nothing
    for (int u = 0; u <= max_bits; ++u)
        for (int i : {0, u / 2, u}) CHECK(!jac_range_pass(i, u, kJacRangeNoneNum, kJacRangeNoneDen), "nothing passes: i %d u %d", i, u);
    for (auto [n, d] : {std::pair<int, int>{0, 0}, {1, 0}, {0, -1}, {-1, 4}, {5, 4}, {1, kJacRangeMaxDen + 1}, {INT32_MIN, 1},
                        {1, INT32_MIN}, {INT32_MAX, INT32_MAX}})
        CHECK(jac_range_bad_threshold(n, d), "%d / %d is no threshold", n, d);
}

static void check_lds() {
    for (int W = 1; W <= kHamMaxWords; ++W) {
        for (int B : {1, 2, 3, 5, 16, 17, 1000}) {
            const int blk = jac_range_pop_block(B, W);
            CHECK(blk >= 1 && blk <= 16 && (blk & (blk - 1)) == 0 && (blk >= B || blk == 16) && (blk < 2 * B), "block of B %d W %d", B, W);
            CHECK(2 * jac_range_pop_lds(blk, W) <= kHamLdsLimit, "popcount LDS of B %d W %d", B, W);
            CHECK(jac_range_block(false, B, W) == blk && jac_range_block(true, B, W) == 64, "block of B %d W %d", B, W);
        }
        for (int qb : {1, 2, 4, 8, 16}) {
            const int64_t q_end = (int64_t)qb * ((W + 15) / 16 * 16) * 8;
            CHECK(jac_range_pop_qpop_off(qb, W) == q_end, "|q| offset qb %d W %d", qb, W);
            CHECK(jac_range_pop_num_off(qb, W) == q_end + 4 * qb && jac_range_pop_den_off(qb, W) == q_end + 8 * qb &&
                      jac_range_pop_lds(qb, W) == q_end + 12 * qb,
                  "popcount LDS qb %d W %d", qb, W);
        }
        const int64_t q_end = (int64_t)((W + 1) / 2 * 2) * 64 * 8;
        CHECK(jac_range_mfma_stage_off(W) == q_end, "stage offset W %d", W);
        CHECK(jac_range_mfma_qpop_off(W) == q_end + 64 * 17 * 4, "|q| offset W %d", W);
        CHECK(jac_range_mfma_num_off(W) == jac_range_mfma_qpop_off(W) + 256 && jac_range_mfma_den_off(W) == jac_range_mfma_num_off(W) + 256 &&
                  jac_range_mfma_xpop_off(W) == jac_range_mfma_den_off(W) + 256,
              "scalar offsets W %d", W);
        CHECK(jac_range_mfma_lds(W) == jac_range_mfma_xpop_off(W) + 4 * 64 * 4, "MFMA LDS W %d", W);
        CHECK(jac_range_mfma_stage_off(W) % 8 == 0 && jac_range_mfma_xpop_off(W) % 4 == 0, "alignment W %d", W);
        CHECK(kHamWgPerCuLds * jac_range_mfma_lds(W) <= kHamLdsLimit, "two workgroups of the MFMA scan at W %d", W);
    }
}

static void check_scratch() {
    for (int B : {1, 5, 64, 70})
        for (int n_bytes : {1, 24, 1024})
            for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)513, (int64_t)100000})
                for (int64_t cap : {(int64_t)0, (int64_t)7})
                    for (int host = 0; host < 2; ++host)
                        for (int masked = 0; masked < 2; ++masked)
                            for (int mfma = 0; mfma < 2; ++mfma) {
                                const int block = jac_range_block(mfma, B, ham_words(n_bytes));
                                const JacRangeScratch s = jaccard_range_scratch(B, n_bytes, block, N, cap, host, masked);
                                CHECK(s.block == std::min(block, B) && s.n_words == (N + 31) / 32 && s.n_chunks == (s.n_words + 15) / 16, "sizes");
                                std::vector<std::pair<int64_t, int64_t>> r = {{s.H, (int64_t)s.block * s.n_words * 4},
                                                                              {s.part, (int64_t)s.block * s.n_chunks * 4},
                                                                              {s.cnt, (int64_t)s.block * 8}};
                                if (host) {
                                    r.push_back({s.q, (int64_t)B * n_bytes});
                                    r.push_back({s.num, (int64_t)B * 4});
                                    r.push_back({s.den, (int64_t)B * 4});
                                    r.push_back({s.mask, masked ? s.n_words * 4 : 0});
                                    r.push_back({s.out_c, (int64_t)B * 8});
                                    r.push_back({s.out_i, B * cap * 8});
                                    r.push_back({s.out_n, B * cap * 4});
                                    r.push_back({s.out_u, B * cap * 4});
                                    CHECK(s.in0 <= s.q && s.mask + (masked ? s.n_words * 4 : 0) <= s.in0 + s.in_bytes, "inputs inside their run");
                                    CHECK(s.out0 == s.in0 + s.in_bytes && s.out0 <= s.out_c && s.out_u + B * cap * 4 <= s.out0 + s.out_bytes,
                                          "outputs inside their run");
                                } else {
                                    CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device call stages nothing");
                                }
                                int64_t end = 0;
                                for (auto [at, bytes] : r) {  // in order, aligned, disjoint
                                    CHECK(at % 256 == 0 && at >= end, "region at %lld after %lld", (long long)at, (long long)end);
                                    end = at + bytes;
                                }
                                CHECK(end <= s.total, "total");
                            }
}

static void check_validation() {
    const int32_t gn[3] = {0, 1, 1 << 18}, gd[3] = {1, 2, 1 << 18};
    const int32_t bn[3] = {0, 3, 1}, bd[3] = {1, 2, 2};
    const int32_t zd[3] = {1, 2, 0};
    int64_t at = -1;
    auto v = [&](bool col, int64_t B, int64_t cap, int mem, bool q, bool n, bool d, bool c, bool i, bool in, bool un,
                 const int32_t* num, const int32_t* den) {
        return jaccard_range_validate(col, B, cap, mem, q, n, d, c, i, in, un, num, den, &at);
    };
    CHECK(v(true, 3, 4, 0, true, true, true, true, true, true, true, gn, gd) == kJacRangeOk, "a good host call");
    CHECK(v(true, 3, 4, 1, true, true, true, true, true, true, true, nullptr, nullptr) == kJacRangeOk, "a good device call (thresholds not read)");
    CHECK(v(false, 3, 4, 0, true, true, true, true, true, true, true, gn, gd) == kJacRangeNoColumn, "no column");
    CHECK(v(false, 0, 0, 0, false, false, false, false, false, false, false, nullptr, nullptr) == kJacRangeNoColumn, "no column, no query");
    CHECK(v(true, -1, 4, 0, true, true, true, true, true, true, true, gn, gd) == kJacRangeBadCount, "negative batch");
    CHECK(v(true, 65536, 4, 0, true, true, true, true, true, true, true, gn, gd) == kJacRangeBadCount, "batch too large");
    CHECK(v(true, 65535, 0, 1, true, true, true, true, false, false, false, nullptr, nullptr) == kJacRangeOk, "the largest batch");
    CHECK(v(true, 3, -1, 0, true, true, true, true, true, true, true, gn, gd) == kJacRangeBadCap, "negative cap");
    CHECK(v(true, 3, ((int64_t)1 << 36) / 3 + 1, 1, true, true, true, true, true, true, true, nullptr, nullptr) == kJacRangeBadCap, "cap too large");
    CHECK(v(true, 3, 4, 2, true, true, true, true, true, true, true, gn, gd) == kJacRangeBadMem, "bad mem");
    CHECK(v(true, 0, 4, 0, false, false, false, false, false, false, false, nullptr, nullptr) == kJacRangeOk, "no queries");
    CHECK(v(true, 3, 4, 0, false, true, true, true, true, true, true, gn, gd) == kJacRangeNullPointer, "NULL queries");
    CHECK(v(true, 3, 4, 0, true, false, true, true, true, true, true, nullptr, gd) == kJacRangeNullPointer, "NULL thr_num");
    CHECK(v(true, 3, 4, 0, true, true, false, true, true, true, true, gn, nullptr) == kJacRangeNullPointer, "NULL thr_den");
    CHECK(v(true, 3, 4, 1, true, true, true, false, true, true, true, nullptr, nullptr) == kJacRangeNullPointer, "NULL counts");
    CHECK(v(true, 3, 4, 0, true, true, true, true, false, true, true, gn, gd) == kJacRangeNullLists, "NULL indices");
    CHECK(v(true, 3, 4, 1, true, true, true, true, true, false, true, nullptr, nullptr) == kJacRangeNullLists, "NULL intersections");
    CHECK(v(true, 3, 4, 0, true, true, true, true, true, true, false, gn, gd) == kJacRangeNullLists, "NULL unions");
    CHECK(v(true, 3, 0, 0, true, true, true, true, false, false, false, gn, gd) == kJacRangeOk, "count only needs no lists");
    CHECK(v(true, 3, 4, 0, true, true, true, true, true, true, true, bn, bd) == kJacRangeBadThreshold && at == 1, "num > den, host");
    CHECK(v(true, 3, 4, 0, true, true, true, true, true, true, true, gn, zd) == kJacRangeBadThreshold && at == 2, "den == 0, host");

    for (int B : {1, 15, 16, 63, 64, 65, 1024, 65535}) {
        CHECK(jaccard_range_use_mfma(0, B) == (kJacRangeMfmaMinQueries > 0 && B >= kJacRangeMfmaMinQueries), "auto at B %d", B);
        CHECK(jaccard_range_use_mfma(1, B), "forced at B %d", B);
        CHECK(!jaccard_range_use_mfma(2, B), "never at B %d", B);
    }
    CHECK(!jaccard_range_use_mfma(1, 0), "no queries, no scan");
    CHECK(jaccard_range_knob_ok(0) && jaccard_range_knob_ok(2) && !jaccard_range_knob_ok(3) && !jaccard_range_knob_ok(-1), "the knob's values");
}

int main() {
    check_pass();
    check_lds();
    check_scratch();
    check_validation();
    std::printf("jaccard range plan ok (%ld checks)\n", g_checks);
    return 0;
}
