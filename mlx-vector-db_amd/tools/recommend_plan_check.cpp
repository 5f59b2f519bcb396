// recommend_plan_check.cpp — the host arithmetic of vdb_index_search_recommend
// (csrc/vdb_recommend_plan.h) swept on the CPU against naive restatements: the validation of the
// scalars and of the CSR lists, the clamp of a device call's offsets, the list state, the fetch size,
// the scratch layout (aligned, disjoint, inside the total), the per-element step with its rounding
// (overflow to +-inf, round to nearest even at fp32 ties) and the compaction rule on lists full of
// examples.  A stand-alone host program (its own main, no GPU, nothing loaded into another process);
// `make recommend-plan-check` builds it with -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "../csrc/vdb_recommend_plan.h"

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

static void check_limits() {
    CHECK(kRecMaxExamples == 64 && kRecMaxFetch == 200 && kRecMaxK == 136, "limits %d %d %d", kRecMaxExamples,
          kRecMaxFetch, kRecMaxK);
    CHECK(kRecLanePos * 64 >= kRecMaxFetch, "a wave's lanes do not hold %d positions", kRecMaxFetch);
    CHECK(kRecMaxExamples <= kRecBuildThreads, "the build's id check has a thread per example");
    for (int k = 1; k <= kRecMaxK; ++k)
        for (int e = 0; e <= kRecMaxExamples; ++e) {
            const int f = rec_fetch_k(k, e);
            CHECK(f == k + e && f >= k && f <= kRecMaxFetch, "fetch %d for k %d, %d examples", f, k, e);
        }
    const int64_t big = std::numeric_limits<int64_t>::max() / 2;
    const int64_t cases[][3] = {{0, 0, 0}, {1, 0, 1}, {3, 4, 7}, {64, 0, 64}, {40, 40, 64}, {big, big, 64}, {0, 65, 64}};
    for (const auto& c : cases)
        CHECK(rec_fetch_examples_device(c[0], c[1]) == c[2], "device examples of (%lld, %lld)", (long long)c[0],
              (long long)c[1]);
}

static void check_clamp(std::mt19937_64& rng) {
    const int64_t lim = std::numeric_limits<int64_t>::max(), lo = std::numeric_limits<int64_t>::min();
    const int64_t edge[] = {lo, lo + 1, -1, 0, 1, 63, 64, 65, 1000, lim - 1, lim};
    for (int trial = 0; trial < 200000; ++trial) {
        const int64_t n = trial % 3 ? (int64_t)(rng() % 100) : (int64_t)(rng() % 3 ? edge[3 + rng() % 8] : 0);
        const int64_t a = trial % 2 ? edge[rng() % 11] : (int64_t)(rng() % 140) - 20;
        const int64_t b = trial % 5 ? (int64_t)(rng() % 140) - 20 : edge[rng() % 11];
        const RecRange r = rec_range(a, b, n);
        const int64_t w0 = std::min(std::max<int64_t>(a, 0), n);
        const int64_t w1 = std::min(std::max(b, w0), n);
        CHECK(r.o0 == w0 && r.o1 == w1, "range (%lld, %lld) of %lld -> [%lld, %lld)", (long long)a, (long long)b,
              (long long)n, (long long)r.o0, (long long)r.o1);
        CHECK(0 <= r.o0 && r.o0 <= r.o1 && r.o1 <= n, "range outside [0, %lld]", (long long)n);
        if (0 <= a && a <= b && b <= n) CHECK(r.o0 == a && r.o1 == b, "a valid range moved");
    }
    for (int64_t np = -1; np <= 70; ++np)
        for (int64_t nn = 0; nn <= 70; ++nn) {
            const int want = np <= 0 ? kRecListEmpty : np + nn > 64 ? kRecListBad : kRecListOk;
            CHECK(rec_list_state(np, nn) == want, "state of (%lld, %lld)", (long long)np, (long long)nn);
        }
    CHECK(rec_list_state(lim, lim) == kRecListBad && rec_list_state(1, lim) == kRecListBad, "huge lists");
    CHECK(rec_id_ok(0, 1) && !rec_id_ok(1, 1) && !rec_id_ok(-1, 1) && !rec_id_ok(0, 0) && !rec_id_ok(lo, lim), "ids");
}

// The validation against a restatement that looks at every entry with its own loops.
static int naive_lists(const std::vector<int64_t>& po, const std::vector<int64_t>& pr, const std::vector<int64_t>* no,
                       const std::vector<int64_t>& nr, int B, int64_t count) {
    auto offs_ok = [&](const std::vector<int64_t>& o, int64_t n) {
        for (int b = 0; b <= B; ++b)
            if (o[b] < 0 || o[b] > n || (b > 0 && o[b] < o[b - 1])) return false;
        return true;
    };
    auto ids_ok = [&](const std::vector<int64_t>& o, const std::vector<int64_t>& r) {
        for (int64_t i = o[0]; i < o[B]; ++i)
            if (r[i] < 0 || r[i] >= count) return false;
        return true;
    };
    if (!offs_ok(po, (int64_t)pr.size())) return kRecBadOffsets;
    if (!ids_ok(po, pr)) return kRecBadId;
    if (no) {
        if (!offs_ok(*no, (int64_t)nr.size())) return kRecBadOffsets;
        if (!ids_ok(*no, nr)) return kRecBadId;
    }
    for (int b = 0; b < B; ++b)
        if ((po[b + 1] - po[b]) + (no ? (*no)[b + 1] - (*no)[b] : 0) > 64) return kRecTooMany;
    return kRecOk;
}

static void check_validate(std::mt19937_64& rng) {
    auto v = [](int B, int k, int64_t np, int64_t nn, unsigned has, int mem) {
        return rec_validate(B, k, np, nn, has & 1, has & 2, has & 4, has & 8, has & 16, has & 32, mem);
    };
    CHECK(v(1, 1, 1, 0, 0x3f, 0) == kRecOk && v(3, 136, 5, 5, 0x3f, 1) == kRecOk, "a plain call refused");
    CHECK(v(0, 1, 0, 0, 0, 0) == kRecOk, "no queries refused");
    CHECK(v(-1, 1, 0, 0, 0x3f, 0) == kRecBadQueries, "n_queries -1");
    for (int k = -2; k <= kRecMaxK + 3; ++k)
        CHECK(v(2, k, 2, 0, 0x3f, 0) == ((k < 1 || k > 136) ? kRecBadK : kRecOk), "k %d", k);
    CHECK(v(2, 10, 2, 0, 0x3f, 2) == kRecBadMem && v(2, 10, 2, 0, 0x3f, -1) == kRecBadMem, "mem");
    CHECK(v(2, 10, -1, 0, 0x3f, 0) == kRecBadCounts && v(2, 10, 1, -1, 0x3f, 0) == kRecBadCounts, "negative counts");
    CHECK(v(2, 10, 2, 1, 0x3f & ~4u, 0) == kRecBadCounts, "negatives without neg_offsets");
    CHECK(v(2, 10, 2, 0, 0x3f & ~(4u | 8u), 0) == kRecOk, "no negatives at all");
    CHECK(v(2, 10, 2, 0, 0x3f & ~1u, 0) == kRecNullPointer, "NULL pos_offsets");
    CHECK(v(2, 10, 2, 0, 0x3f & ~2u, 0) == kRecNullPointer && v(2, 10, 0, 0, 0x3f & ~2u, 0) == kRecOk, "NULL pos_rows");
    CHECK(v(2, 10, 2, 1, 0x3f & ~8u, 0) == kRecNullPointer && v(2, 10, 2, 0, 0x3f & ~8u, 0) == kRecOk, "NULL neg_rows");
    CHECK(v(2, 10, 2, 0, 0x3f & ~16u, 0) == kRecNullPointer, "NULL scores");
    CHECK(v(2, 10, 2, 0, 0x3f & ~32u, 0) == kRecNullPointer, "NULL indices");

    int seen[kRecTooMany + 1] = {0};
    for (int trial = 0; trial < 40000; ++trial) {
        const int B = 1 + (int)(rng() % 6);
        const int64_t count = (int64_t)(rng() % 50);
        const bool has_neg = rng() & 1;
        auto make = [&](std::vector<int64_t>& o, std::vector<int64_t>& r, int most) {
            o.assign(B + 1, 0);
            for (int b = 0; b < B; ++b) o[b + 1] = o[b] + (int64_t)(rng() % (most + 1));
            r.resize((size_t)o[B] + rng() % 3);
            for (auto& x : r) x = count > 0 ? (int64_t)(rng() % count) : 0;
        };
        std::vector<int64_t> po, pr, no, nr;
        const int shape = (int)(rng() % 4);  // short lists, lists around the limit
        make(po, pr, shape == 0 ? 70 : shape == 1 ? 33 : 5);
        make(no, nr, shape == 1 ? 33 : 4);
        switch (rng() % 8) {  // a fault, sometimes
            case 0: po[rng() % (B + 1)] = (int64_t)(rng() % 9) - 4; break;
            case 1: no[rng() % (B + 1)] = (int64_t)nr.size() + 1; break;
            case 2: if (!pr.empty()) pr[rng() % pr.size()] = rng() & 1 ? -1 : count; break;
            case 3: if (!nr.empty()) nr[rng() % nr.size()] = rng() & 1 ? -1 : count; break;
            default: break;
        }
        if (count == 0 && rng() % 2) {  // an empty index takes empty lists only
            po.assign(B + 1, 0);
            no.assign(B + 1, 0);
        }
        int64_t at = -5;
        int which = -5, most = -5;
        const int got = rec_validate_lists(po.data(), pr.data(), (int64_t)pr.size(), has_neg ? no.data() : nullptr,
                                           nr.data(), (int64_t)nr.size(), B, count, &at, &which, &most);
        const int want = naive_lists(po, pr, has_neg ? &no : nullptr, nr, B, count);
        CHECK(got == want, "lists: %d, want %d (trial %d)", got, want, trial);
        ++seen[got];
        if (got == kRecOk) {
            int m = 0;
            for (int b = 0; b < B; ++b)
                m = std::max<int>(m, (int)((po[b + 1] - po[b]) + (has_neg ? no[b + 1] - no[b] : 0)));
            CHECK(most == m && most <= 64, "largest example count %d, want %d", most, m);
        } else if (got == kRecBadId) {
            const std::vector<int64_t>& r = which ? nr : pr;
            CHECK(at >= 0 && at < (int64_t)r.size() && !rec_id_ok(r[at], count), "bad id reported at %lld", (long long)at);
        } else if (got == kRecBadOffsets) {
            CHECK(at >= 0 && at <= B && (which == 0 || has_neg), "bad offset reported at %lld", (long long)at);
        }
        CHECK(rec_validate_lists(po.data(), pr.data(), (int64_t)pr.size(), has_neg ? no.data() : nullptr, nr.data(),
                                 (int64_t)nr.size(), B, count, nullptr, nullptr, nullptr) == got,
              "NULL report pointers change the answer");
    }
    for (int c : {kRecOk, kRecBadOffsets, kRecBadId, kRecTooMany}) CHECK(seen[c] > 100, "case %d drawn %d times", c, seen[c]);
    // exactly at the limit
    std::vector<int64_t> o = {0, 64}, r(64, 3), o2 = {0, 1}, r2 = {0};
    CHECK(rec_validate_lists(o.data(), r.data(), 64, nullptr, nullptr, 0, 1, 4, nullptr, nullptr, nullptr) == kRecOk, "64");
    CHECK(rec_validate_lists(o.data(), r.data(), 64, o2.data(), r2.data(), 1, 1, 4, nullptr, nullptr, nullptr) ==
              kRecTooMany, "64 + 1");
}

static void check_scratch(std::mt19937_64& rng) {
    for (int trial = 0; trial < 20000; ++trial) {
        const int B = 1 + (int)(rng() % (trial % 5 ? 300 : 70000));
        const int dim = 1 + (int)(rng() % 3000);
        const int k = 1 + (int)(rng() % kRecMaxK);
        const int F = rec_fetch_k(k, (int)(rng() % (kRecMaxExamples + 1)));
        const int64_t rows = (int64_t)(rng() % 3 ? rng() % 100000 : rng() % 40);
        const int64_t n_pos = (int64_t)(rng() % (64 * (uint64_t)B + 1)), n_neg = (int64_t)(rng() % (64 * (uint64_t)B + 1));
        const bool host = rng() & 1, has_neg = rng() & 1, masked = rng() & 1, keys = rng() & 1, queries = rng() & 1;
        const RecScratch s = rec_scratch(B, dim, k, F, rows, n_pos, has_neg ? n_neg : 0, host, has_neg, masked, keys, queries);
        struct Span {
            int64_t at, bytes;
        };
        std::vector<Span> spans;
        const Span q = {s.q, (int64_t)B * dim * 4};
        if (!(host && queries)) spans.push_back(q);
        spans.push_back({s.flag, (int64_t)B * 4});
        spans.push_back({s.fs, (int64_t)B * F * 4});
        spans.push_back({s.fi, (int64_t)B * F * 8});
        spans.push_back({s.fk, (int64_t)B * F * 8});
        CHECK(s.mask_words == (rows + 31) / 32, "mask words %lld for %lld rows", (long long)s.mask_words, (long long)rows);
        if (host) {
            const size_t first_in = spans.size();
            spans.push_back({s.pos_offs, (int64_t)(B + 1) * 8});
            spans.push_back({s.pos_rows, n_pos * 8});
            if (has_neg) spans.push_back({s.neg_offs, (int64_t)(B + 1) * 8});
            if (has_neg) spans.push_back({s.neg_rows, n_neg * 8});
            if (masked) spans.push_back({s.mask, (s.mask_words + 64) * 4});
            for (size_t i = first_in; i < spans.size(); ++i)
                CHECK(spans[i].at >= s.in0 && spans[i].at + spans[i].bytes <= s.in0 + s.in_bytes, "an argument outside the upload");
            const size_t first_out = spans.size();
            spans.push_back({s.out_s, (int64_t)B * k * 4});
            spans.push_back({s.out_i, (int64_t)B * k * 8});
            if (keys) spans.push_back({s.out_k, (int64_t)B * k * 8});
            if (queries) spans.push_back(q);
            for (size_t i = first_out; i < spans.size(); ++i)
                CHECK(spans[i].at >= s.out0 && spans[i].at + spans[i].bytes <= s.out0 + s.out_bytes, "a result outside the download");
            CHECK(s.out0 == s.in0 + s.in_bytes, "the download does not follow the upload");
            CHECK(s.out0 + s.out_bytes == s.total, "the download does not end the workspace");
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

static uint32_t fbits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// fp64 -> fp32, round to nearest even, written out on the bits (finite input of fp32's normal range).
static float naive_round(double t) {
    if (std::fabs(t) >= 0x1.ffffffp127) return t < 0 ? -INFINITY : INFINITY;  // at or past the midpoint above FLT_MAX
    uint64_t u;
    std::memcpy(&u, &t, 8);
    const uint32_t sign = (uint32_t)(u >> 63) << 31;
    const int exp = (int)((u >> 52) & 0x7ff) - 1023;
    const uint64_t man = u & ((1ull << 52) - 1);
    uint32_t m = (uint32_t)(man >> 29);
    const uint64_t rest = man & ((1ull << 29) - 1), half = 1ull << 28;
    uint32_t e = (uint32_t)(exp + 127);
    if (rest > half || (rest == half && (m & 1))) {
        if (++m == (1u << 23)) {
            m = 0;
            ++e;
        }
    }
    return from_bits(sign | (e << 23) | m);
}

static void check_element(std::mt19937_64& rng) {
    const double inf = std::numeric_limits<double>::infinity();
    // the terms
    CHECK(rec_term(3.0f, 123.0, 1) == 3.0 && rec_term(-0.0f, 0.0, 1) == 0.0 && std::signbit(rec_term(-0.0f, 0.0, 1)), "euclidean term");
    CHECK(rec_term(3.0f, 2.0, 0) == 1.5 && rec_term(3.0f, 0.0, 0) == 3.0 / 1e-8 && rec_term(3.0f, 1e-9, 0) == 3.0 / 1e-8 &&
              rec_term(1.0f, 1e-8, 0) == 1.0 / 1e-8, "cosine term and its clamp");
    for (int i = 0; i < 20000; ++i) {  // the identity behind the euclidean single-positive property
        const float x = from_bits((uint32_t)rng());
        if (!std::isfinite(x)) continue;
        const float back = rec_combine(rec_mean(0.0 + rec_term(x, 1.0, 1), 1), 0.0, false);
        CHECK(fbits(back) == fbits(x) || (x == 0.0f && back == 0.0f), "a single positive is not itself: %a -> %a", x, back);
    }
    CHECK(rec_mean(6.0, 4) == 1.5 && rec_mean(1.0, 3) == 1.0 / 3.0, "mean");
    // combine: the rule
    CHECK(rec_combine(1.5, 99.0, false) == 1.5f && rec_combine(1.5, 0.25, true) == 2.75f, "average-vector rule");
    // overflow to +-inf and the finite test
    const double fm = FLT_MAX;
    CHECK(rec_combine(fm, 0, false) == FLT_MAX && rec_finite(rec_combine(fm, 0, false)), "FLT_MAX stays");
    CHECK(rec_combine(1.2e38, -1.2e38, true) == INFINITY && !rec_finite(rec_combine(1.2e38, -1.2e38, true)), "3.6e38 -> inf");
    CHECK(rec_combine(-1.2e38, 1.2e38, true) == -INFINITY && !rec_finite(rec_combine(-1.2e38, 1.2e38, true)), "-3.6e38 -> -inf");
    CHECK(rec_combine(1.2e38, 1.2e38, true) == 1.2e38f, "(mp + mp) - mn in fp64 does not overflow on the way");
    CHECK(rec_combine(0x1.fffffefp127, 0, false) == FLT_MAX && rec_combine(0x1.ffffffp127, 0, false) == INFINITY,
          "the midpoint above FLT_MAX rounds to inf (even), below it to FLT_MAX");
    CHECK(!rec_finite((float)inf) && !rec_finite(-(float)inf) && !rec_finite(std::nanf("")) && rec_finite(0.0f) &&
              rec_finite(-FLT_MAX) && rec_finite(FLT_MIN / 4), "finite test");
    // round to nearest even at ties: exactly half way between two neighbouring floats
    for (int i = 0; i < 20000; ++i) {
        const uint32_t b = ((uint32_t)rng() & 0x7fffffu) | ((1u + (uint32_t)(rng() % 253)) << 23);
        const float lo = from_bits(b), hi = from_bits(b + 1);
        const double mid = ((double)lo + (double)hi) / 2.0;  // exact in fp64
        const float even = (b & 1) ? hi : lo;
        for (double s : {1.0, -1.0}) {
            CHECK(rec_combine(s * mid, 0, false) == (float)s * even, "tie %a does not go to even", mid);
            CHECK(rec_combine(std::nextafter(s * mid, s * inf), 0, false) == (float)s * hi, "above the tie");
            CHECK(rec_combine(std::nextafter(s * mid, 0.0), 0, false) == (float)s * lo, "below the tie");
        }
        // and through the rule: (mp + mp) - mn landing on the tie
        CHECK(rec_combine(mid, mid, true) == even, "the rule onto a tie");
    }
    for (int i = 0; i < 200000; ++i) {  // any value of the normal range against the rounding on the bits
        std::uniform_real_distribution<double> u(-1.0, 1.0);
        const double t = std::ldexp(u(rng), (int)(rng() % 250) - 120);
        if (std::fabs(t) < FLT_MIN) continue;
        CHECK(fbits(rec_combine(t, 0, false)) == fbits(naive_round(t)), "rounding of %a", t);
    }
}

static void check_compact(std::mt19937_64& rng) {
    for (int trial = 0; trial < 20000; ++trial) {
        const int64_t count = 1 + (int64_t)(rng() % (trial % 4 ? 300 : 80));
        const int np = 1 + (int)(rng() % 64), nn = (int)(rng() % (65 - np));
        std::vector<int64_t> pos(np), neg(nn);
        for (auto& x : pos) x = (int64_t)(rng() % count);
        for (auto& x : neg) x = (int64_t)(rng() % count);
        if (nn && rng() % 2) neg[0] = pos[0];   // a row in both lists
        if (np > 1 && rng() % 2) pos[1] = pos[0];  // a repeated row
        const int k = 1 + (int)(rng() % kRecMaxK);
        const int F = rec_fetch_k(k, np + nn);
        // a fetched list: distinct rows, the examples crowded to the front in some trials, -1 after the valid prefix
        std::vector<int64_t> all(count);
        for (int64_t i = 0; i < count; ++i) all[i] = i;
        std::shuffle(all.begin(), all.end(), rng);
        if (trial % 2) {
            std::set<int64_t> ex(pos.begin(), pos.end());
            ex.insert(neg.begin(), neg.end());
            std::stable_partition(all.begin(), all.end(), [&](int64_t r) { return ex.count(r) != 0; });
        }
        std::vector<int64_t> fi(F, -1);
        for (int p = 0; p < F && p < count; ++p) fi[p] = all[p];
        std::vector<int> got(k, -7), want;
        const int m = rec_compact(fi.data(), F, k, count, pos.data(), np, neg.empty() ? nullptr : neg.data(), nn, got.data());
        for (int p = 0; p < F && (int)want.size() < k; ++p) {
            const int64_t r = fi[p];
            if (r < 0 || r >= count) continue;
            if (std::find(pos.begin(), pos.end(), r) != pos.end() || std::find(neg.begin(), neg.end(), r) != neg.end()) continue;
            want.push_back(p);
        }
        CHECK(m == (int)want.size(), "%d kept, want %d", m, (int)want.size());
        for (int s = 0; s < m; ++s) CHECK(got[s] == want[s], "slot %d holds position %d, want %d", s, got[s], want[s]);
        for (int s = m; s < k; ++s) CHECK(got[s] == -7, "slot %d past the kept written", s);
        // the fetch is large enough: a list that was not cut short by the corpus fills all k slots
        std::set<int64_t> ex(pos.begin(), pos.end());
        ex.insert(neg.begin(), neg.end());
        if (count >= F) CHECK(m == k, "k' = k + examples left %d of %d slots empty", k - m, k);
        else CHECK(m == std::min<int64_t>(k, count - (int64_t)ex.size()), "a short corpus keeps %d", m);
        // the wave's form of the same rule: ballots over 64 positions at a time, prefix popcounts
        std::vector<int> wave(k, -7);
        int kept = 0;
        for (int t = 0; t < kRecLanePos; ++t) {
            uint64_t mask = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int p = lane + 64 * t;
                if (p < F && rec_keep(fi[p], count, pos.data(), np, neg.data(), nn)) mask |= 1ull << lane;
            }
            for (int lane = 0; lane < 64; ++lane) {
                const int slot = kept + __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                if ((mask >> lane & 1) && slot < k) wave[slot] = lane + 64 * t;
            }
            kept += __builtin_popcountll(mask);
        }
        CHECK(wave == got, "the ballot form differs from the in-order form");
    }
}

int main() {
    std::mt19937_64 rng(20241020);
    check_limits();
    check_clamp(rng);
    check_validate(rng);
    check_scratch(rng);
    check_element(rng);
    check_compact(rng);
    std::printf("recommend plan ok (%ld checks)\n", g_checks);
    return 0;
}
