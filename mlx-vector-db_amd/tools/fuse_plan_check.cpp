// fuse_plan_check.cpp — the host arithmetic of vdb_index_search_fused (csrc/vdb_fuse_plan.h) swept on
// the CPU against naive loops: the validation, the clamp of a device call's offsets, the two packed
// sort words and the order key of a fused value, the sort length with the workgroup size and LDS it
// leads to, the pair order of a bitonic step, the scratch layout, and the fusion of one set: against
// a naive map-and-sort, and against a host replay of the kernel's own steps (pack, sort, walk the
// runs, order-key sort) over the same plan functions.  A stand-alone host program (its own main, no
// GPU, nothing loaded into another process); `make fuse-plan-check` builds it with
// -fsanitize=address,undefined and -ffp-contract=off and runs it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>
#include <vector>

#include "../csrc/vdb_fuse_plan.h"

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

static void check_validate() {
    auto v = [](int64_t ns, int64_t nsets, int k, int f, int fusion, double c, bool q = true, bool o = true,
                bool w = false, bool s = true, bool i = true, int mem = 0) {
        return fuse_validate(ns, nsets, k, f, fusion, c, q, o, w, s, i, mem);
    };
    CHECK(v(4, 1, 10, 40, kFuseRrf, 60.0) == kFuseOk, "a plain call refused");
    CHECK(v(0, 0, 1, 1, kFuseMaxFusion, kNan, false, false, false, false, false, 1) == kFuseOk, "an empty call refused");
    CHECK(v(0, 3, 1, 1, kFuseRrf, 0.0, false) == kFuseOk, "sets without sub-queries refused");
    CHECK(v(-1, 1, 1, 1, kFuseRrf, 60.0) == kFuseBadCounts && v(1, -1, 1, 1, kFuseRrf, 60.0) == kFuseBadCounts, "counts");
    for (int k = -2; k <= kFuseMaxK + 2; ++k)
        for (int f = -2; f <= kFuseMaxFetch + 2; ++f) {
            const int want = (k < 1 || k > kFuseMaxK) ? kFuseBadK : (f < k || f > kFuseMaxFetch) ? kFuseBadFetch : kFuseOk;
            CHECK(v(3, 1, k, f, kFuseRrf, 60.0) == want, "k %d fetch %d", k, f);
        }
    for (int fusion : {-1, 2, 7}) CHECK(v(1, 1, 1, 1, fusion, 60.0) == kFuseBadFusion, "fusion %d", fusion);
    for (double c : {-1.0, kNan, kInf, -kInf, -std::numeric_limits<double>::denorm_min()}) {
        CHECK(v(1, 1, 1, 1, kFuseRrf, c) == kFuseBadC, "rrf_c %g accepted", c);
        CHECK(v(1, 1, 1, 1, kFuseMaxFusion, c) == kFuseOk, "MAX looks at rrf_c %g", c);
    }
    for (double c : {0.0, -0.0, 60.0, std::numeric_limits<double>::max()})
        CHECK(v(1, 1, 1, 1, kFuseRrf, c) == kFuseOk, "rrf_c %g refused", c);
    CHECK(v(1, 1, 1, 1, kFuseRrf, 60.0, false) == kFuseNullPointer, "NULL queries");
    CHECK(v(1, 1, 1, 1, kFuseRrf, 60.0, true, false) == kFuseNullPointer, "NULL offsets");
    CHECK(v(1, 1, 1, 1, kFuseRrf, 60.0, true, true, false, false) == kFuseNullPointer, "NULL scores");
    CHECK(v(1, 1, 1, 1, kFuseRrf, 60.0, true, true, false, true, false) == kFuseNullPointer, "NULL indices");
    CHECK(v(1, 1, 1, 1, kFuseRrf, 60.0, true, true, false, true, true, 2) == kFuseBadMem, "mem 2");
    CHECK(v(1, 1, 1, 1, kFuseRrf, 60.0, true, true, true) == kFuseOk, "weights with RRF refused");
    CHECK(v(1, 1, 1, 1, kFuseMaxFusion, 60.0, true, true, true) == kFuseWeightsWithMax, "weights with MAX");

    int64_t at = -1;
    const int64_t ok[] = {0, 0, 16, 16, 20};
    CHECK(fuse_validate_lists(ok, 4, 20, nullptr, &at) == kFuseListsOk, "good offsets refused");
    const int64_t dec[] = {0, 5, 4};
    CHECK(fuse_validate_lists(dec, 2, 20, nullptr, &at) == kFuseBadOffsets && at == 2, "decreasing offsets");
    const int64_t past[] = {0, 5, 21};
    CHECK(fuse_validate_lists(past, 2, 20, nullptr, &at) == kFuseBadOffsets && at == 2, "offsets past n_sub");
    const int64_t neg[] = {-1, 5};
    CHECK(fuse_validate_lists(neg, 1, 20, nullptr, &at) == kFuseBadOffsets && at == 0, "a negative offset");
    const int64_t lng[] = {0, 3, 20};
    CHECK(fuse_validate_lists(lng, 2, 20, nullptr, &at) == kFuseSetTooLong && at == 1, "a set of 17");
    for (double bad : {-1.0, kNan, kInf, -kInf}) {
        const double w[] = {1.0, 0.0, bad, 3.0};
        const int64_t o[] = {0, 4};
        CHECK(fuse_validate_lists(o, 1, 4, w, &at) == kFuseBadWeight && at == 2, "weight %g accepted", bad);
        CHECK(!fuse_weight_ok(bad), "weight %g ok", bad);
    }
    const double good[] = {1.0, 0.0, -0.0, std::numeric_limits<double>::max()};
    const int64_t o4[] = {0, 4};
    CHECK(fuse_validate_lists(o4, 1, 4, good, &at) == kFuseListsOk, "good weights refused");
}

static void check_range(std::mt19937& rng) {
    for (int trial = 0; trial < 200000; ++trial) {
        const int64_t n = rng() % 40;
        auto draw = [&]() -> int64_t {
            switch (rng() % 6) {
                case 0: return -(int64_t)(rng() % 5) - 1;
                case 1: return n + 1 + rng() % 5;
                case 2: return (rng() & 1) ? std::numeric_limits<int64_t>::min() : std::numeric_limits<int64_t>::max();
                default: return n ? rng() % (n + 1) : 0;
            }
        };
        const int64_t lo = draw(), hi = draw();
        const FuseRange r = fuse_range(lo, hi, n);
        CHECK(r.o0 >= 0 && r.o0 <= n && r.m >= 0 && r.m <= kFuseMaxLists && r.o0 + r.m <= n, "range [%lld + %d) of %lld",
              (long long)r.o0, r.m, (long long)n);
        const bool good = lo >= 0 && hi <= n && lo <= hi && hi - lo <= kFuseMaxLists;
        CHECK(r.bad == !good, "offsets %lld %lld of %lld: bad %d", (long long)lo, (long long)hi, (long long)n, (int)r.bad);
        if (good) CHECK(r.o0 == lo && r.m == hi - lo, "a good range changed");
        else CHECK(r.m == 0, "a bad set fuses %d lists", r.m);
    }
}

static void check_words(std::mt19937& rng) {
    for (int trial = 0; trial < 200000; ++trial) {
        const uint64_t row = trial % 3 ? rng() % 5000 : ((uint64_t)rng() << 12 | rng()) & ((1ull << 44) - 1);
        const int l = rng() % kFuseMaxLists, p = rng() % kFuseMaxFetch, hits = 1 + rng() % kFuseMaxLists;
        const uint64_t w = fuse_pack_entry(row, l, p);
        CHECK(fuse_entry_row(w) == row && fuse_entry_list(w) == l && fuse_entry_pos(w) == p && w != kFusePad, "entry word");
        const uint64_t c = fuse_pack_cand(row, l, p, hits);
        CHECK(fuse_cand_row(c) == row && fuse_cand_list(c) == l && fuse_cand_pos(c) == p && fuse_cand_hits(c) == hits &&
                  c != kFusePad,
              "candidate word");
        // (row, l, p) orders entry words; the row orders candidate words
        const uint64_t row2 = rng() % 5000;
        const int l2 = rng() % kFuseMaxLists, p2 = rng() % kFuseMaxFetch;
        const bool lt = row < row2 || (row == row2 && (l < l2 || (l == l2 && p < p2)));
        CHECK((w < fuse_pack_entry(row2, l2, p2)) == lt, "entry order");
        if (row != row2) CHECK((c < fuse_pack_cand(row2, l2, p2, 1)) == (row < row2), "candidate order");
        CHECK(fuse_entry_row(kFusePad) > row, "a pad's row field names a row");
    }
    // the order key: monotone, zeros equal, the value back for what RRF can produce
    std::vector<double> v = {-kInf, -1e300, -2.0, -1.0, -1e-300, -std::numeric_limits<double>::denorm_min(), -0.0, 0.0,
                             std::numeric_limits<double>::denorm_min(), 1e-300, 0.5, 1.0, 1.0 / 61.0, 2.0, 1e300, kInf};
    std::uniform_real_distribution<double> u(-2.0, 2.0);
    for (int i = 0; i < 2000; ++i) v.push_back(u(rng));
    for (double a : v)
        for (double b : v) {
            const uint64_t ka = fuse_order_key(a), kb = fuse_order_key(b);
            CHECK((ka > kb) == (a > b) && (ka == kb) == (a == b), "order key of %g against %g", a, b);
            CHECK(ka != 0, "a value shares the pad's key");
        }
    for (double a : v) {
        const double back = fuse_key_value(fuse_order_key(a));
        CHECK(back == a && (a == 0.0 ? !std::signbit(back) : fuse_bits(back) == fuse_bits(a)), "key value of %g is %g", a, back);
    }
    CHECK(fuse_cand_before(5, 9, 4, 1) && !fuse_cand_before(4, 1, 5, 9), "key order");
    CHECK(fuse_cand_before(5, 1, 5, 9) && !fuse_cand_before(5, 9, 5, 1), "equal keys: the lower row");
    CHECK(fuse_cand_before(fuse_order_key(-kInf), 1, 0, kFusePad), "a pad before a candidate");
}

static void check_sizes() {
    for (int e = -1; e <= kFuseMaxEntries; ++e) {
        const int L = fuse_sort_len(e);
        if (e <= 0) {
            CHECK(L == 0, "sort length %d of %d entries", L, e);
            continue;
        }
        CHECK(L >= 64 && L >= e && (L & (L - 1)) == 0 && (L == 64 || L / 2 < e) && L <= kFuseMaxSort, "sort length %d of %d", L, e);
        const int T = fuse_threads(L);
        CHECK(T >= kFuseMinThreads && T <= kFuseMaxThreads && T % 64 == 0 && (int64_t)T * kFusePosPerThread >= L,
              "%d threads for %d positions", T, L);
        CHECK(fuse_lds_bytes(L) == (int64_t)L * 16 && fuse_lds_bytes(L) <= 65536, "LDS of %d positions", L);
    }
    CHECK(fuse_sort_len(kFuseMaxEntries) == kFuseMaxSort && fuse_threads(kFuseMaxSort) == kFuseMaxThreads, "the largest set");
    for (int64_t n_sub : {0ll, 1ll, 4ll, 15ll, 16ll, 17ll, 1000ll, 1ll << 31})
        for (int F = 1; F <= kFuseMaxFetch; ++F) {
            const int L = fuse_call_sort_len(n_sub, F);
            for (int m = 0; m <= kFuseMaxLists && m <= n_sub; ++m)
                CHECK(fuse_sort_len(m * F) <= L, "a set of %d lists sorts more than the call's %d", m, L);
        }
    // a bitonic step: every position in exactly one pair, and for small strides every half-wave's
    // first and second touches are 32 consecutive positions
    for (int L : {64, 128, 4096})
        for (int stride = 1; stride < L; stride <<= 1) {
            std::vector<int> seen(L, 0);
            for (int e = 0; e < L / 2; ++e) {
                const int lo = fuse_pair_lo(e, stride);
                CHECK(lo >= 0 && lo + stride < L && (lo & stride) == 0, "pair %d of stride %d", e, stride);
                ++seen[lo];
                ++seen[lo + stride];
                const int first = fuse_pair_first(lo, stride);
                CHECK(first == lo || first == lo + stride, "first touch");
            }
            for (int i = 0; i < L; ++i) CHECK(seen[i] == 1, "position %d in %d pairs (stride %d)", i, seen[i], stride);
            for (int h = 0; h < L / 64; ++h) {  // the 32 pairs e = 32 h ..
                unsigned long long a = 0, b = 0;
                for (int e = 32 * h; e < 32 * h + 32; ++e) {
                    const int lo = fuse_pair_lo(e, stride);
                    const int first = fuse_pair_first(lo, stride), second = first == lo ? lo + stride : lo;
                    a |= 1ull << (first % 32);
                    b |= 1ull << (second % 32);
                }
                CHECK(a == 0xFFFFFFFFull && b == 0xFFFFFFFFull, "stride %d: a half-wave meets a bank twice", stride);
            }
        }
}

static void check_scratch(std::mt19937& rng) {
    for (int trial = 0; trial < 20000; ++trial) {
        const int64_t n_sub = rng() % (trial % 5 ? 300 : 70000);
        const int64_t n_sets = 1 + rng() % 3000;
        const int dim = 1 + (int)(rng() % 3000);
        const int k = 1 + (int)(rng() % kFuseMaxK);
        const int F = k + (int)(rng() % (kFuseMaxFetch - k + 1));
        const int64_t rows = (int64_t)(rng() % 3 ? rng() % 100000 : rng() % 40);
        const bool host = rng() & 1, weighted = rng() & 1, masked = rng() & 1, fused = rng() & 1, hits = rng() & 1;
        const FuseScratch s = fuse_scratch(n_sub, n_sets, dim, k, F, rows, host, weighted, masked, fused, hits);
        struct Span {
            int64_t at, bytes;
        };
        std::vector<Span> spans = {{s.fs, n_sub * F * 4}, {s.fi, n_sub * F * 8}, {s.fk, n_sub * F * 8}};
        CHECK(s.mask_words == (rows + 31) / 32, "mask words");
        if (host) {
            spans.push_back({s.q, n_sub * dim * 4});
            spans.push_back({s.offs, (n_sets + 1) * 8});
            if (weighted) spans.push_back({s.w, n_sub * 8});
            if (masked) spans.push_back({s.mask, (s.mask_words + 64) * 4});
            const size_t first_out = spans.size();
            spans.push_back({s.out_s, n_sets * k * 4});
            spans.push_back({s.out_i, n_sets * k * 8});
            if (fused) spans.push_back({s.out_f, n_sets * k * 8});
            if (hits) spans.push_back({s.out_h, n_sets * k * 4});
            for (size_t i = 3; i < spans.size(); ++i) {
                const bool in = i < first_out;
                const int64_t b0 = in ? s.in0 : s.out0, b1 = in ? s.in0 + s.in_bytes : s.out0 + s.out_bytes;
                CHECK(spans[i].at >= b0 && spans[i].at + spans[i].bytes <= b1, "span %zu outside its copy", i);
            }
            CHECK(s.out0 == s.in0 + s.in_bytes && s.out0 + s.out_bytes == s.total, "the download does not follow the upload");
        } else {
            CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device-memory call stages bytes");
        }
        int64_t end = 0;
        for (const Span& p : spans) {
            CHECK(p.at % 256 == 0, "offset %lld is not 256-byte aligned", (long long)p.at);
            CHECK(p.at >= end, "a span at %lld overlaps one ending at %lld", (long long)p.at, (long long)end);
            end = p.at + p.bytes;
            CHECK(end <= s.total, "a span ends past the total");
        }
    }
}

// The kernel's steps replayed on the host over the plan's functions: pack, sort ascending, the head
// of each run walks it, the candidates sorted by (key desc, pay asc), the first k unpacked.
static int replay(int m, int F, int k, int fusion, double c, const int64_t* rows, const double* keys, const double* w,
                  int64_t count, int64_t* orow, double* ofused, int* ohits, int* oat) {
    const int L = fuse_sort_len(m * F);
    std::vector<uint64_t> a(L, kFusePad);
    for (int e = 0; e < m * F; ++e)
        if (rows[e] >= 0 && rows[e] < count) a[e] = fuse_pack_entry((uint64_t)rows[e], e / F, e % F);
    std::sort(a.begin(), a.end());
    std::vector<std::pair<uint64_t, uint64_t>> cand;
    for (int i = 0; i < L; ++i) {
        if (a[i] == kFusePad) continue;
        const uint64_t row = fuse_entry_row(a[i]);
        if (i > 0 && fuse_entry_row(a[i - 1]) == row) continue;
        double fused = 0.0;
        int hits = 0, bl = 0, bp = 0;
        for (int e = i; e < L && hits < kFuseMaxLists && fuse_entry_row(a[e]) == row; ++e) {
            const int l = fuse_entry_list(a[e]), p = fuse_entry_pos(a[e]);
            if (fusion == kFuseRrf) {
                fused = fuse_rrf_add(fused, w ? w[l] : 1.0, c, p);
            } else if (hits == 0 || fuse_max_takes(keys[l * F + p], fused)) {
                fused = keys[l * F + p];
                bl = l;
                bp = p;
            }
            ++hits;
        }
        cand.push_back({fuse_order_key(fused), fuse_pack_cand(row, bl, bp, hits)});
    }
    std::sort(cand.begin(), cand.end(), [](const auto& x, const auto& y) { return fuse_cand_before(x.first, x.second, y.first, y.second); });
    const int n = std::min<int>(k, (int)cand.size());
    for (int j = 0; j < n; ++j) {
        const uint64_t p = cand[j].second;
        const int at = fuse_cand_list(p) * F + fuse_cand_pos(p);
        orow[j] = (int64_t)fuse_cand_row(p);
        ofused[j] = fusion == kFuseRrf ? fuse_key_value(cand[j].first) : keys[at];
        ohits[j] = fuse_cand_hits(p);
        oat[j] = fusion == kFuseRrf ? -1 : at;
    }
    return n;
}

static void check_select(std::mt19937& rng) {
    const double key_vals[] = {-1.0, -0.5, -0.0, 0.0, 0.5, 1.0};
    const double w_vals[] = {0.0, 0.5, 1.0, 3.0};
    for (int trial = 0; trial < 4000; ++trial) {
        const bool big = trial % 50 == 0;
        const int m = big ? kFuseMaxLists : (int)(rng() % 6);
        const int F = big ? kFuseMaxFetch : 1 + (int)(rng() % 12);
        const int k = 1 + (int)(rng() % F);
        const int fusion = trial & 1;
        const double c = trial % 7 == 0 ? 0.0 : 60.0;
        const int64_t count = big ? 5000 : 1 + rng() % 30;
        const bool weighted = fusion == kFuseRrf && (rng() & 1);
        const bool ties = trial % 4 != 0;
        std::uniform_real_distribution<double> u(-1.0, 1.0);
        std::vector<int64_t> rows((size_t)m * F, -1);
        std::vector<double> keys((size_t)m * F, -kInf), w(m);
        for (int l = 0; l < m; ++l) {
            // a list: distinct rows, keys descending, a -1 tail, now and then a row >= count
            std::vector<int64_t> perm(count);
            for (int64_t i = 0; i < count; ++i) perm[i] = i;
            std::shuffle(perm.begin(), perm.end(), rng);
            const int n = (int)std::min<int64_t>(count, rng() % (F + 1));
            std::vector<double> ks(n);
            for (double& x : ks) x = ties ? key_vals[rng() % 6] : u(rng);
            std::sort(ks.begin(), ks.end(), [](double x, double y) { return x > y; });
            for (int p = 0; p < n; ++p) {
                rows[l * F + p] = (rng() % 40 == 0) ? count + (int64_t)(rng() % 3) : perm[p];
                keys[l * F + p] = ks[p];
            }
            w[l] = w_vals[rng() % 4];
        }
        const double* wp = weighted ? w.data() : nullptr;
        std::vector<int64_t> r1(k, -7), r2(k, -7);
        std::vector<double> f1(k, 7.0), f2(k, 7.0);
        std::vector<int> h1(k, -7), h2(k, -7), a1(k, -7), a2(k, -7);
        const int n1 = fuse_select(m, F, k, fusion, c, rows.data(), keys.data(), wp, count, r1.data(), f1.data(), h1.data(), a1.data());
        const int n2 = replay(m, F, k, fusion, c, rows.data(), keys.data(), wp, count, r2.data(), f2.data(), h2.data(), a2.data());
        // the contract written out naively: a map from row to its terms in list order
        struct Acc {
            double fused;
            int hits;
        };
        std::map<int64_t, Acc> acc;
        for (int l = 0; l < m; ++l)
            for (int p = 0; p < F; ++p) {
                const int64_t r = rows[l * F + p];
                if (r < 0 || r >= count) continue;
                auto it = acc.find(r);
                if (fusion == kFuseRrf) {
                    if (it == acc.end()) it = acc.insert({r, {0.0, 0}}).first;
                    const double t = c + (double)(p + 1);
                    const double q = (wp ? wp[l] : 1.0) / t;
                    it->second.fused = it->second.fused + q;
                } else if (it == acc.end()) {
                    it = acc.insert({r, {keys[l * F + p], 0}}).first;
                } else {
                    it->second.fused = keys[l * F + p] > it->second.fused ? keys[l * F + p] : it->second.fused;
                }
                ++it->second.hits;
            }
        std::vector<std::pair<int64_t, Acc>> want(acc.begin(), acc.end());  // rows ascending
        std::stable_sort(want.begin(), want.end(), [](const auto& x, const auto& y) { return x.second.fused > y.second.fused; });
        const int n = std::min<int>(k, (int)want.size());
        CHECK(n1 == n && n2 == n, "%d / %d candidates written, want %d", n1, n2, n);
        for (int j = 0; j < n; ++j) {
            CHECK(r1[j] == want[j].first && r2[j] == want[j].first, "slot %d rows %lld / %lld, want %lld (trial %d)", j,
                  (long long)r1[j], (long long)r2[j], (long long)want[j].first, trial);
            CHECK(fuse_bits(f1[j]) == fuse_bits(want[j].second.fused) && fuse_bits(f2[j]) == fuse_bits(want[j].second.fused),
                  "slot %d fused %a / %a, want %a", j, f1[j], f2[j], want[j].second.fused);
            CHECK(h1[j] == want[j].second.hits && h2[j] == h1[j], "slot %d hits %d / %d", j, h1[j], h2[j]);
            if (fusion == kFuseMaxFusion) {
                CHECK(a1[j] >= 0 && a1[j] < m * F && rows[a1[j]] == r1[j] && fuse_bits(keys[a1[j]]) == fuse_bits(f1[j]),
                      "slot %d: the entry named does not hold the maximum", j);
                CHECK(a2[j] == a1[j], "slot %d: entries %d / %d", j, a1[j], a2[j]);
            } else {
                CHECK(a1[j] == -1 && a2[j] == -1, "RRF names an entry");
            }
        }
        for (int j = n; j < k; ++j) CHECK(r1[j] == -7 && f1[j] == 7.0 && h1[j] == -7, "slot %d past the candidates written", j);
    }
    // the term and the maximum on their own
    CHECK(fuse_rrf_add(0.0, 1.0, 60.0, 0) == 1.0 / 61.0 && fuse_rrf_add(0.0, 0.0, 0.0, 0) == 0.0, "an RRF term");
    CHECK(!fuse_max_takes(0.0, -0.0) && !fuse_max_takes(-0.0, 0.0) && fuse_max_takes(0.5, 0.25), "the maximum keeps the first of equals");
}

int main() {
    std::mt19937 rng(20241021);
    check_validate();
    check_range(rng);
    check_words(rng);
    check_sizes();
    check_scratch(rng);
    check_select(rng);
    std::printf("fuse plan ok (%ld checks)\n", g_checks);
    return 0;
}
