// maxsim_plan_check.cpp — the host arithmetic of vdb_index_search_maxsim (csrc/vdb_maxsim_plan.h)
// swept on the CPU against naive loops: the validation, the table size check, the order-preserving
// encoding of a maximum (round trip, order, the + 0.0 of the contract, 0 below every value), the
// clamp of a device call's offsets, the deal of slots to the rank kernel's segments, waves and
// lanes (every slot exactly once), the scratch layout, and the ranking of one set: against a naive
// sort, and against a host replay of the two kernels' own steps (runs of one slot folded as
// encoded maxima in any grouping, the entries summed in sub-query order, a top-k per segment and a
// merge) over the same plan functions.  A stand-alone host program (its own main, no GPU, nothing
// loaded into another process); `make maxsim-plan-check` builds it with
// -fsanitize=address,undefined and -ffp-contract=off and runs it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/vdb_maxsim_plan.h"

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

static const double kInf = std::numeric_limits<double>::infinity();

static void check_validate() {
    auto v = [](int64_t ns, int64_t nsets, int64_t slots, int k, bool q = true, bool o = true, bool s = true,
                bool g = true, int mem = 0) { return maxsim_validate(ns, nsets, slots, k, q, o, s, g, mem); };
    CHECK(v(4, 1, 10, 10) == kMaxsimOk, "a plain call refused");
    CHECK(v(0, 0, 1, 1, false, false, false, false, 1) == kMaxsimOk, "an empty call refused");
    CHECK(v(0, 3, 1, 1, false) == kMaxsimOk, "sets without sub-queries refused");
    CHECK(v(-1, 1, 1, 1) == kMaxsimBadCounts && v(1, -1, 1, 1) == kMaxsimBadCounts, "counts");
    for (int k = -2; k <= kMaxsimMaxK + 2; ++k)
        CHECK(v(3, 1, 5, k) == ((k < 1 || k > kMaxsimMaxK) ? kMaxsimBadK : kMaxsimOk), "k %d", k);
    for (int64_t slots : {(int64_t)-5, (int64_t)0}) CHECK(v(1, 1, slots, 1) == kMaxsimBadSlots, "slots %lld", (long long)slots);
    // the table: n_sub * slots <= 2^27, by division
    for (int64_t ns : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)64, (int64_t)65, (int64_t)1000, (int64_t)(1 << 27),
                       (int64_t)0x7FFFFFFF})
        for (int64_t slots : {(int64_t)1, (int64_t)2, (int64_t)1000, (int64_t)(1 << 20), (int64_t)(1 << 21), (int64_t)(1 << 26),
                              (int64_t)((1 << 26) + 1), (int64_t)(1 << 27), (int64_t)((1 << 27) + 1), (int64_t)0x7FFFFFFF}) {
            const bool want = (__int128)ns * slots <= (__int128)kMaxsimMaxCells;
            CHECK(maxsim_table_ok(ns, slots) == want, "table %lld x %lld", (long long)ns, (long long)slots);
            CHECK((v(ns, 1, slots, 1) == kMaxsimOk) == want, "validate %lld x %lld", (long long)ns, (long long)slots);
        }
    CHECK(v(1, 1, 1, 1, false) == kMaxsimNullPointer, "NULL queries");
    CHECK(v(1, 1, 1, 1, true, false) == kMaxsimNullPointer, "NULL offsets");
    CHECK(v(1, 1, 1, 1, true, true, false) == kMaxsimNullPointer, "NULL scores");
    CHECK(v(1, 1, 1, 1, true, true, true, false) == kMaxsimNullPointer, "NULL groups");
    CHECK(v(1, 1, 1, 1, true, true, true, true, 2) == kMaxsimBadMem && v(1, 1, 1, 1, true, true, true, true, -1) == kMaxsimBadMem,
          "mem");

    int64_t at = -1;
    const int64_t ok[] = {0, 0, 64, 64, 70};
    CHECK(maxsim_validate_sets(ok, 4, 70, &at) == kMaxsimSetsOk, "good offsets refused");
    const int64_t dec[] = {0, 5, 4};
    CHECK(maxsim_validate_sets(dec, 2, 9, &at) == kMaxsimBadOffsets && at == 2, "decreasing offsets");
    const int64_t past[] = {0, 5, 10};
    CHECK(maxsim_validate_sets(past, 2, 9, &at) == kMaxsimBadOffsets && at == 2, "offsets past n_sub");
    const int64_t neg[] = {-1, 5};
    CHECK(maxsim_validate_sets(neg, 1, 9, &at) == kMaxsimBadOffsets && at == 0, "a negative offset");
    const int64_t lng[] = {0, 3, 68};
    CHECK(maxsim_validate_sets(lng, 2, 70, &at) == kMaxsimSetTooLong && at == 1, "a set of 65");
    CHECK(maxsim_validate_sets(nullptr, 0, 0, &at) == kMaxsimSetsOk, "no sets");
}

static void check_encoding() {
    std::vector<double> vals = {-kInf, -1.7976931348623157e308, -1e300, -2.0, -1.0, -1e-300,
                                -std::numeric_limits<double>::denorm_min(), -0.0, 0.0,
                                std::numeric_limits<double>::denorm_min(), 1e-300, 0.5, 1.0, 1.0000000000000002, 2.0, 1e300,
                                1.7976931348623157e308, kInf};
    std::mt19937_64 rng(1);
    for (int i = 0; i < 2000; ++i) {
        const double x = maxsim_from_bits(rng());
        if (x == x) vals.push_back(x);
    }
    for (double a : vals) {
        const uint64_t ea = maxsim_encode(a);
        CHECK(ea != 0, "%g encodes to the empty entry", a);
        CHECK(maxsim_bits(maxsim_decode(ea)) == maxsim_bits(a), "round trip of %g", a);
        CHECK(maxsim_bits(maxsim_decode(maxsim_entry(a))) == maxsim_bits(a + 0.0), "entry of %g", a);
        for (double b : vals) {
            const uint64_t eb = maxsim_encode(b);
            if (a < b) CHECK(ea < eb, "%g < %g but not their encodings", a, b);
            if (a == b && maxsim_bits(a) == maxsim_bits(b)) CHECK(ea == eb, "equal bits, different encodings");
        }
    }
    CHECK(maxsim_encode(-0.0) < maxsim_encode(0.0), "the zeros' encodings");
    CHECK(maxsim_entry(-0.0) == maxsim_entry(0.0), "+ 0.0 does not merge the zeros");
    CHECK(maxsim_bits(maxsim_decode(maxsim_entry(-0.0))) == 0, "the entry of -0.0 is not +0.0");
    CHECK(maxsim_encode(-kInf) == 0x000FFFFFFFFFFFFFull, "-inf");
    for (int32_t g : {-2147483647 - 1, -1, 0, 1, 6, 7, 8, 2147483647})
        CHECK(maxsim_slot(g, 7) == ((g >= 0 && g < 7) ? g : -1), "slot of %d", g);
}

static void check_range() {
    for (int64_t n_sub : {0, 1, 5, 64, 65, 200})
        for (int64_t lo = -3; lo <= n_sub + 3; ++lo)
            for (int64_t hi = -3; hi <= n_sub + 70; ++hi) {
                const MaxsimRange r = maxsim_range(lo, hi, n_sub);
                const bool good = lo >= 0 && hi >= lo && hi <= n_sub && hi - lo <= kMaxsimMaxVectors;
                CHECK(r.bad == !good, "set [%lld, %lld) of %lld", (long long)lo, (long long)hi, (long long)n_sub);
                CHECK(r.o0 >= 0 && r.o0 <= n_sub && r.m >= 0 && r.m <= kMaxsimMaxVectors && r.o0 + r.m <= n_sub,
                      "range of [%lld, %lld) of %lld leaves the sub-queries", (long long)lo, (long long)hi, (long long)n_sub);
                if (good) CHECK(r.o0 == lo && r.m == hi - lo, "a good set's range");
                else CHECK(r.m == 0, "a bad set sums something");
            }
    const int64_t big = std::numeric_limits<int64_t>::max(), small = std::numeric_limits<int64_t>::min();
    CHECK(maxsim_range(small, big, 10).bad && maxsim_range(big, small, 10).bad && maxsim_range(0, big, 10).bad, "extremes");
}

static void check_deal() {
    for (int k = 1; k <= kMaxsimMaxK; ++k) {
        const int ke = maxsim_ke(k);
        CHECK(ke >= k && ke < 2 * k + 1 && (ke & (ke - 1)) == 0 && ke <= kMaxsimMaxK, "KE of %d", k);
    }
    for (int64_t n_slots : {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 5000, 300000})
        for (int64_t n_sets : {1, 2, 7, 100, 2048, 5000}) {
            const int n_seg = maxsim_n_seg(n_slots, n_sets);
            CHECK(n_seg >= 1 && n_seg <= kMaxsimMaxSeg, "n_seg %d", n_seg);
            CHECK(n_seg == 1 || (int64_t)(n_seg - 1) * kMaxsimSegSlots < n_slots, "a segment without a slot");
            CHECK(n_seg == 1 || (int64_t)n_seg * n_sets <= kMaxsimCallWgs, "too many workgroups");
            if (n_slots > 5000) continue;
            std::vector<int> seen((size_t)n_slots, 0);
            for (int seg = 0; seg < n_seg; ++seg)
                for (int wave = 0; wave < kMaxsimThreads / 64; ++wave)
                    for (int64_t i = 0;; ++i) {
                        const int64_t g0 = maxsim_trip_slot(seg, n_seg, wave, i);
                        if (g0 >= n_slots) break;
                        for (int lane = 0; lane < 64; ++lane)
                            if (g0 + lane < n_slots) ++seen[(size_t)(g0 + lane)];
                    }
            for (int64_t g = 0; g < n_slots; ++g) CHECK(seen[(size_t)g] == 1, "slot %lld dealt %d times", (long long)g, seen[(size_t)g]);
        }
}

static void check_scratch() {
    for (int64_t n_sub : {0, 1, 65, 4096})
        for (int64_t n_sets : {1, 3, 70})
            for (int64_t n_slots : {1, 7, 1300, 32768})
                for (int k : {1, 5, 128})
                    for (int host = 0; host < 2; ++host)
                        for (int masked = 0; masked < 2; ++masked)
                            for (int sums = 0; sums < 2; ++sums) {
                                const int64_t rows = 1300;
                                const int dim = 100;
                                const MaxsimScratch s = maxsim_scratch(n_sub, n_sets, n_slots, dim, 64, k, rows, host, masked, sums);
                                CHECK(s.KE == maxsim_ke(k) && s.n_seg == maxsim_n_seg(n_slots, n_sets), "KE / n_seg");
                                struct R { int64_t at, bytes; };
                                std::vector<R> rs = {{s.qn64, n_sub * 8}, {s.T, n_sub * n_slots * 8}, {s.done, n_sets * 4}};
                                if (s.n_seg > 1) {
                                    rs.push_back({s.lk, n_sets * s.n_seg * s.KE * 8});
                                    rs.push_back({s.li, n_sets * s.n_seg * s.KE * 4});
                                    rs.push_back({s.mk, n_sets * s.KE * 8});
                                    rs.push_back({s.mi, n_sets * s.KE * 4});
                                }
                                if (host) {
                                    rs.push_back({s.q, n_sub * dim * 4});
                                    rs.push_back({s.offs, (n_sets + 1) * 8});
                                    if (masked) rs.push_back({s.mask, s.mask_words * 4});
                                    rs.push_back({s.out_s, n_sets * k * 4});
                                    rs.push_back({s.out_g, n_sets * k * 4});
                                    if (sums) rs.push_back({s.out_sum, n_sets * k * 8});
                                }
                                int64_t end = 0;
                                for (const R& r : rs) {
                                    CHECK(r.at % 256 == 0 && r.at >= end && r.at + r.bytes <= s.total, "a region overlaps or leaves");
                                    end = r.at + r.bytes;
                                }
                                CHECK(s.zero_bytes == s.done + maxsim_align(n_sets * 4) - s.T && s.T + s.zero_bytes <= s.lk,
                                      "the zeroed span");
                                CHECK(s.mask_words == (rows + 31) / 32, "mask words");
                                if (host) {
                                    CHECK(s.in0 <= s.q && s.in0 + s.in_bytes == s.out0 && s.out0 + s.out_bytes == s.total, "staging spans");
                                    CHECK(s.offs + (n_sets + 1) * 8 <= s.in0 + s.in_bytes && s.out_s >= s.out0, "staged regions");
                                } else {
                                    CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device call stages something");
                                }
                            }
}

// One set over random data: the scan's fold (runs of one slot as encoded maxima, flushed into the
// table in a shuffled order and random groupings), the rank's sums and top-k per segment and the
// merge, against a naive ranking over doubles.
static void check_select() {
    std::mt19937_64 rng(7);
    for (int round = 0; round < 300; ++round) {
        const int n_rows = 1 + (int)(rng() % 400);
        const int n_slots = 1 + (int)(rng() % (round % 3 == 0 ? 3000 : 40));
        const int n_sub = 1 + (int)(rng() % 70);
        const int k = 1 + (int)(rng() % kMaxsimMaxK);
        std::vector<int32_t> grp((size_t)n_rows);
        for (auto& g : grp) g = (int32_t)(rng() % (uint64_t)(n_slots + 3)) - 1;  // -1 and ids past the slots too
        if (round % 4 == 0) std::sort(grp.begin(), grp.end());                   // runs
        std::vector<double> key((size_t)n_sub * n_rows);
        for (auto& x : key) {
            const int c = (int)(rng() % 16);  // few distinct values: ties, and both zeros
            x = c == 0 ? -0.0 : c == 1 ? 0.0 : (double)((int)(rng() % 7) - 3) * 0.25 - (c > 12 ? 1e-3 * (double)(rng() % 5) : 0.0);
        }
        // the table, by flushes of runs cut at random places, applied in a shuffled order
        struct Flush { size_t cell; uint64_t v; };
        std::vector<Flush> fl;
        for (int t = 0; t < n_sub; ++t) {
            int32_t cur_slot = -1;
            uint64_t cur = 0;
            for (int r = 0; r < n_rows; ++r) {
                const int32_t sl = maxsim_slot(grp[(size_t)r], n_slots);
                if (sl < 0) continue;
                if (sl != cur_slot || rng() % 5 == 0) {
                    if (cur_slot >= 0) fl.push_back({(size_t)t * n_slots + (size_t)cur_slot, cur});
                    cur_slot = sl;
                    cur = 0;
                }
                const uint64_t e = maxsim_entry(key[(size_t)t * n_rows + r]);
                cur = e > cur ? e : cur;
            }
            if (cur_slot >= 0) fl.push_back({(size_t)t * n_slots + (size_t)cur_slot, cur});
        }
        std::shuffle(fl.begin(), fl.end(), rng);
        std::vector<uint64_t> T((size_t)n_sub * n_slots, 0);
        for (const Flush& f : fl) T[f.cell] = std::max(T[f.cell], f.v);
        // naive maxima over doubles
        for (int t = 0; t < n_sub; ++t)
            for (int g = 0; g < n_slots; ++g) {
                bool any = false;
                double m = 0.0;
                for (int r = 0; r < n_rows; ++r)
                    if (grp[(size_t)r] == g) {
                        const double x = key[(size_t)t * n_rows + r] + 0.0;
                        m = (!any || x > m) ? x : m;
                        any = true;
                    }
                const uint64_t e = T[(size_t)t * n_slots + g];
                CHECK((e != 0) == any, "slot %d: eligibility", g);
                if (any) CHECK(maxsim_bits(maxsim_decode(e)) == maxsim_bits(m), "slot %d: maximum", g);
            }
        // a set
        const int o0 = (int)(rng() % (uint64_t)n_sub);
        const int m = std::min<int>(n_sub - o0, (int)(rng() % (kMaxsimMaxVectors + 1)));
        struct C { double sum; int32_t g; };
        std::vector<C> cand;
        if (m > 0)
            for (int g = 0; g < n_slots; ++g) {
                if (T[(size_t)o0 * n_slots + g] == 0) continue;
                double acc = 0.0;
                for (int t = 0; t < m; ++t) acc = acc + maxsim_decode(T[(size_t)(o0 + t) * n_slots + g]);
                CHECK(maxsim_bits(acc) == maxsim_bits(maxsim_sum(&T[(size_t)o0 * n_slots + g], m, n_slots)), "maxsim_sum");
                cand.push_back({acc, g});
            }
        std::stable_sort(cand.begin(), cand.end(), [](const C& a, const C& b) { return a.sum > b.sum || (a.sum == b.sum && a.g < b.g); });
        std::vector<int32_t> og((size_t)k, -7);
        std::vector<double> os((size_t)k, 0.0);
        const int n = maxsim_select(T.data(), n_slots, o0, m, k, og.data(), os.data());
        CHECK(n == (int)std::min<size_t>(cand.size(), (size_t)k), "select returns %d of %zu", n, cand.size());
        for (int i = 0; i < n; ++i)
            CHECK(og[(size_t)i] == cand[(size_t)i].g && maxsim_bits(os[(size_t)i]) == maxsim_bits(cand[(size_t)i].sum), "slot %d of the ranking", i);
        // the rank kernel's way: a top-k per segment over its dealt slots, merged
        const int n_seg = maxsim_n_seg(n_slots, 1 + (int)(rng() % 4));
        std::vector<C> merged;
        for (int seg = 0; seg < n_seg; ++seg) {
            std::vector<C> mine;
            for (int wave = 0; wave < kMaxsimThreads / 64; ++wave)
                for (int64_t i = 0;; ++i) {
                    const int64_t g0 = maxsim_trip_slot(seg, n_seg, wave, i);
                    if (g0 >= n_slots) break;
                    for (int lane = 0; lane < 64 && g0 + lane < n_slots && m > 0; ++lane) {
                        const int64_t g = g0 + lane;
                        if (T[(size_t)o0 * n_slots + (size_t)g] == 0) continue;
                        mine.push_back({maxsim_sum(&T[(size_t)o0 * n_slots + (size_t)g], m, n_slots), (int32_t)g});
                    }
                }
            std::sort(mine.begin(), mine.end(), [](const C& a, const C& b) { return a.sum > b.sum || (a.sum == b.sum && a.g < b.g); });
            if ((int)mine.size() > k) mine.resize((size_t)k);
            merged.insert(merged.end(), mine.begin(), mine.end());
        }
        std::sort(merged.begin(), merged.end(), [](const C& a, const C& b) { return a.sum > b.sum || (a.sum == b.sum && a.g < b.g); });
        CHECK((int)std::min<size_t>(merged.size(), (size_t)k) == n, "segments lose a candidate");
        for (int i = 0; i < n; ++i) CHECK(merged[(size_t)i].g == og[(size_t)i], "segment merge, slot %d", i);
    }
}

int main() {
    check_validate();
    check_encoding();
    check_range();
    check_deal();
    check_scratch();
    check_select();
    std::printf("maxsim plan ok: %ld checks\n", g_checks);
    return 0;
}
