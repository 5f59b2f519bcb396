// jaccard_plan_check.cpp — the host arithmetic of vdb_index_search_jaccard (csrc/vdb_jaccard_plan.h) swept
// on the CPU against naive integer arithmetic: the two exact keys (order and injectivity over every pair
// among the Farey neighbours of denominators near 8 192 and over every pair of small ratios, the u == 0
// case, the truncated fp64 quotient against the integer division at every (i, u), and the fact the
// design rests on, that fp32 ties two distinct ratios), the threshold test against the key compare, the
// popcount form's block sizes and LDS layout, the MFMA form's LDS layout at every width, the scratch, the
// validation causes and the choice of form.  A stand-alone host program (its own main, no GPU, nothing
// loaded into another process); `make jaccard-plan-check` builds it with -fsanitize=address,undefined and
// runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../csrc/vdb_jaccard_plan.h"

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

typedef std::pair<int, int> Ratio;  // (i, u)

// Every pair of a set of ratios: both keys order them as the cross-multiplication does, equal ratios
// get equal keys, distinct ratios distinct keys.
static void check_pairs(const std::vector<Ratio>& rs, const char* what) {
    for (const Ratio& a : rs)
        for (const Ratio& b : rs) {
            const bool gt = jac_greater(a.first, a.second, b.first, b.second);
            const bool lt = jac_greater(b.first, b.second, a.first, a.second);
            const double ka = jac_key(a.first, a.second), kb = jac_key(b.first, b.second);
            const uint32_t ha = jac_key_hi(a.first, a.second), hb = jac_key_hi(b.first, b.second);
            CHECK((ka > kb) == gt && (ka < kb) == lt, "%s: fp64 key of %d/%d against %d/%d", what, a.first, a.second, b.first, b.second);
            CHECK((ha < hb) == gt && (ha > hb) == lt, "%s: integer key of %d/%d against %d/%d", what, a.first, a.second, b.first, b.second);
        }
}

static void check_keys(std::mt19937& rng) {
    // the integer key is the floor of the rational at every (i, u), and fits 28 bits
    for (int u = 1; u <= 8 * kHamMaxBytes; ++u)
        for (int i = 0; i <= u; ++i) {
            const uint64_t want = ((uint64_t)(u - i) << kJacKeyShift) / (uint64_t)u;
            CHECK(jac_key_hi(i, u) == want, "key of %d/%d: %u, integer division %llu", i, u, jac_key_hi(i, u), (unsigned long long)want);
        }
    CHECK(jac_key_hi(0, 0) == 0 && jac_key(0, 0) == 1.0 && jac_key_hi(5, 5) == 0 && jac_key(5, 5) == 1.0, "u == 0 ranks as 1");
    CHECK(jac_key_hi(0, 8192) == 1u << kJacKeyShift && jac_key(0, 3) == 0.0, "s == 0");
    CHECK(!jac_greater(0, 0, 7, 7) && !jac_greater(7, 7, 0, 0) && jac_greater(0, 0, 8191, 8192), "u == 0 in the order");
    // what fp32 cannot do, and the reason for all this
    CHECK((float)8190 / (float)8191 == (float)8191 / (float)8192, "fp32 separates the closest pair after all");
    CHECK(jac_key(8190, 8191) < jac_key(8191, 8192) && jac_key_hi(8190, 8191) > jac_key_hi(8191, 8192), "the closest pair");
    // Farey neighbours: for denominators near the top, every fraction i / u of them, its neighbours
    // (i +- 1) / u, and the nearest fractions of the adjacent denominators, all pairs
    for (int u0 : {8192, 8191, 8190, 8189, 4097, 4096, 2048}) {
        std::vector<Ratio> rs = {{0, 0}, {0, u0}, {u0, u0}};
        for (int rep = 0; rep < 40; ++rep) {
            const int i = rep < 4 ? u0 - 1 - rep : (int)(rng() % (unsigned)u0);
            for (int du = -2; du <= 0; ++du) {
                const int u = u0 + du;
                if (u < 1) continue;
                const int64_t c = (int64_t)i * u / u0;  // i / u0 lies in [c / u, (c + 1) / u]
                for (int64_t j = c - 1; j <= c + 2; ++j)
                    if (j >= 0 && j <= u) rs.push_back({(int)j, u});
            }
        }
        check_pairs(rs, "Farey neighbours");
    }
    // every ratio of small sets: the ties (1/2 = 2/4 = 3/6) and their order
    std::vector<Ratio> small = {{0, 0}};
    for (int u = 1; u <= 40; ++u)
        for (int i = 0; i <= u; ++i) small.push_back({i, u});
    check_pairs(small, "small ratios");
    // the threshold test is the key compare
    for (int rep = 0; rep < 400000; ++rep) {
        const int u = (int)(rng() % 8193u), i = u ? (int)(rng() % (unsigned)(u + 1)) : 0;
        const uint32_t row = rng() % 5u;
        int ut = u, it = i;
        if (rep % 3) {
            ut = (int)(rng() % 8193u);
            it = ut ? (int)(rng() % (unsigned)(ut + 1)) : 0;
        } else if (rep % 2 && 2 * u <= 8192) {  // the same ratio, other terms
            ut = 2 * u;
            it = 2 * i;
        }
        const uint64_t thr = jac_key64(it, ut, rng() % 5u);
        CHECK(jac_pass(i, u, row, thr) == (jac_key64(i, u, row) < thr), "threshold test of %d/%d row %u against %d/%d", i, u, row, it, ut);
    }
    CHECK(jac_pass(0, 8192, 0xFFFFFFFEu, ~0ull) && !jac_pass(0, 0, 0, 0ull), "the empty threshold passes all, an absent query's none");
}

static void check_lds() {
    // the merge's buffer and the top-k buffers, restated: 12 bytes an entry
    CHECK(2 * jac_lds_bytes(16, kHamMaxWords, 32, true) > kHamLdsLimit, "sixteen queries fit twice: kJacMaxQB is too small");
    CHECK(jac_qb(1) == 8 && jac_qb(64) == 8 && jac_qb(65) == 4 && jac_qb(128) == 4 && jac_qb(129) == 2 && jac_qb(256) == 2 &&
              jac_qb(257) == 1 && jac_qb(1024) == 1,
          "block sizes");
    for (int n_bytes = 1; n_bytes <= kHamMaxBytes; ++n_bytes) {
        const int W = ham_words(n_bytes);
        for (int k : {1, 10, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024}) {
            const int KE = ham_ke(k), qb = jac_qb(k);
            CHECK(qb >= 1 && qb <= kJacMaxQB && (qb & (qb - 1)) == 0, "qb %d", qb);
            CHECK(jac_lds_bytes(qb, W, KE, true) + 64 <= kHamLdsLimit, "one workgroup fits at k %d, %d bytes", k, n_bytes);
            if (k <= 512) CHECK(kHamWgPerCuLds * jac_lds_bytes(qb, kHamMaxWords, KE, true) <= kHamLdsLimit, "two fit at k %d", k);
            if (qb < kJacMaxQB) CHECK(kHamWgPerCuLds * jac_lds_bytes(2 * qb, kHamMaxWords, KE, true) > kHamLdsLimit, "qb %d is not the largest", qb);
            // regions in order, aligned, disjoint
            CHECK(jac_qpop_off(qb, W) == (int64_t)qb * ham_query_stride(W) * 8 && jac_qpop_off(qb, W) + qb * 4 <= jac_query_lds(qb, W), "|q| words");
            CHECK(jac_lds_key_off(0, 0, qb, W, KE) == jac_query_lds(qb, W) && jac_lds_key_off(0, 0, qb, W, KE) % 8 == 0, "keys follow the queries");
            CHECK(jac_lds_key_off(kHamWaves - 1, qb - 1, qb, W, KE) + ham_cap(KE) * 8 == jac_lds_row_off(0, 0, qb, W, KE), "rows follow the keys");
            CHECK(jac_lds_row_off(kHamWaves - 1, qb - 1, qb, W, KE) + ham_cap(KE) * 4 == jac_query_lds(qb, W) + jac_topk_lds(qb, KE), "rows end");
            CHECK(jac_lds_bytes(qb, W, KE, true) >= jac_query_lds(qb, W) + jac_merge_lds(KE), "the merge buffer fits");
            for (int nq : {1, 2, 3, qb, qb + 1, 1000}) {
                const int b = jac_block(k, nq);
                CHECK(b <= qb && (b & (b - 1)) == 0 && (b >= nq || b == qb), "block %d of %d queries", b, nq);
            }
        }
        CHECK(jac_mfma_lds_bytes(W) + kHamMfmaStaticLds <= kHamLdsLimit, "mfma form at %d bytes", n_bytes);
        CHECK(jac_mfma_qpop_off(W) == ham_mfma_lds_bytes(W) && jac_mfma_qpop_off(W) % 4 == 0, "|q| follows the counts");
        CHECK(jac_mfma_xpop_off(W) == jac_mfma_qpop_off(W) + kHamMfmaQB * 4, "|x| follows |q|");
        CHECK(jac_mfma_lds_bytes(W) == jac_mfma_xpop_off(W) + kHamWaves * kHamTileRows * 4, "|x| of four tiles ends the layout");
    }
    CHECK(jac_mfma_qb(1) == kHamMfmaQB && jac_mfma_qb(kHamMfmaMaxK) == kHamMfmaQB && jac_mfma_qb(kHamMfmaMaxK + 1) == 0 && jac_mfma_qb(0) == 0, "mfma k range");
}

static void check_form_validation_scratch() {
    for (int knob = -1; knob <= 3; ++knob) CHECK(jaccard_knob_ok(knob) == (knob >= 0 && knob <= 2), "knob %d", knob);
    CHECK(jaccard_use_mfma(1, 1, kHamMfmaMaxK, 1) && !jaccard_use_mfma(1, 1000, kHamMfmaMaxK + 1, 1), "knob 1");
    CHECK(!jaccard_use_mfma(2, 1000, 10, 128) && !jaccard_use_mfma(1, 0, 10, 128) && !jaccard_use_mfma(1, 5, 10, 1025), "knob 2, no query, no width");
    if (kJacMfmaMinQueries > 0)
        CHECK(!jaccard_use_mfma(0, kJacMfmaMinQueries - 1, 10, 128) && jaccard_use_mfma(0, kJacMfmaMinQueries, 10, 128), "auto threshold");
    else
        CHECK(!jaccard_use_mfma(0, 1, 10, 128) && !jaccard_use_mfma(0, kHamMaxQueries, 10, 128), "auto without a measurement");
    // validation: one cause each, in order
    CHECK(jaccard_validate_call(0, 1, false, false, false, false, 0, true) == kJacOk, "an empty batch");
    CHECK(jaccard_validate_call(-1, 1, true, true, true, true, 0, true) == kJacBadCount, "count");
    CHECK(jaccard_validate_call(kHamMaxQueries + 1, 1, true, true, true, true, 0, true) == kJacBadCount, "count");
    CHECK(jaccard_validate_call(1, 0, true, true, true, true, 0, true) == kJacBadK, "k");
    CHECK(jaccard_validate_call(1, kHamMaxK + 1, true, true, true, true, 0, true) == kJacBadK, "k");
    CHECK(jaccard_validate_call(1, 1, true, true, true, true, 2, true) == kJacBadMem, "mem");
    for (int missing = 0; missing < 4; ++missing)
        CHECK(jaccard_validate_call(1, 1, missing != 0, missing != 1, missing != 2, missing != 3, 1, true) == kJacNullPointer, "pointer %d", missing);
    CHECK(jaccard_validate_call(1, 1, true, true, true, true, 1, false) == kJacNoColumn, "column");
    // scratch: fp64 lists, three result regions, everything aligned and in order
    for (int n_bytes : {1, 9, 1024})
        for (int nq : {1, 65})
            for (int n_seg : {1, 3}) {
                const int k = 10, KE = ham_ke(k);
                const JaccardScratch sc = jaccard_scratch(nq, n_bytes, k, 8, n_seg, 1300, true, true);
                CHECK(sc.li - sc.lk >= (n_seg > 1 ? (int64_t)nq * n_seg * KE * 8 : 0) && sc.lk % 256 == 0, "list keys");
                CHECK(sc.mi - sc.mk >= (n_seg > 1 ? (int64_t)nq * KE * 8 : 0) && sc.mk % 256 == 0, "merged keys");
                CHECK(sc.mask - sc.q >= (int64_t)nq * n_bytes && sc.q % 256 == 0 && sc.in_bytes >= sc.mask - sc.in0 + sc.mask_words * 4, "arguments");
                CHECK(sc.out_u - sc.out_n >= (int64_t)nq * k * 4 && sc.out_i - sc.out_u >= (int64_t)nq * k * 4 && sc.out_i % 8 == 0 &&
                          sc.total >= sc.out_i + (int64_t)nq * k * 8 && sc.out_bytes == sc.total - sc.out0,
                      "results");
            }
}

int main() {
    std::mt19937 rng(12345);
    check_keys(rng);
    check_lds();
    check_form_validation_scratch();
    std::printf("jaccard plan ok: %ld checks, popcount blocks %d / %d / %d / %d at k 64 / 128 / 256 / 1024\n", g_checks, jac_qb(64),
                jac_qb(128), jac_qb(256), jac_qb(1024));
    return 0;
}
