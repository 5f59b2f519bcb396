// sparse_plan_check.cpp — the host arithmetic of vdb_index_set_sparse, vdb_index_search_sparse and
// vdb_index_search_hybrid (csrc/vdb_sparse_plan.h) swept on the CPU against naive loops: the deal of
// rows to segments, waves and lanes (every row exactly once), the clamp of a device call's offsets
// and what makes a query bad, the term search, the key of a row against a dense-table restatement,
// the scratch layouts (aligned, disjoint, inside the total), the LDS budget, and the validation of
// the column and of the queries, one cause at a time.  A stand-alone host program (its own main, no
// GPU, nothing loaded into another process); `make sparse-plan-check` builds it with
// -fsanitize=address,undefined and -ffp-contract=off and runs it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <vector>

#include "../csrc/vdb_sparse_plan.h"

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

static const float kNanF = std::numeric_limits<float>::quiet_NaN();
static const float kInfF = std::numeric_limits<float>::infinity();
static const double kNan = std::numeric_limits<double>::quiet_NaN();
static const double kInf = std::numeric_limits<double>::infinity();

static void check_deal() {
    for (int64_t N : {0, 1, 3, 37, 63, 64, 65, 255, 256, 257, 513, 1300, 5000}) {
        const int64_t chunks = sparse_n_chunks(N);
        CHECK(chunks == (N + 255) / 256, "chunks of %lld", (long long)N);
        for (int n_seg : {1, 2, 7, 64, 512}) {
            const int live = sparse_live_segs(N, n_seg);
            CHECK(live == (int)std::min<int64_t>(chunks, n_seg), "live segments N %lld n_seg %d", (long long)N, n_seg);
            std::vector<int> seen((size_t)N, 0);
            for (int s = 0; s < live; ++s)
                for (int64_t c = s; c < chunks; c += n_seg)
                    for (int wv = 0; wv < kSparseWaves; ++wv)
                        for (int lane = 0; lane < kSparseWaveRows; ++lane) {
                            const int64_t r = sparse_row_of(c, wv, lane);
                            CHECK(r >= 0, "negative row");
                            if (r < N) ++seen[(size_t)r];
                        }
            // the segments at or past `live` have no chunk
            for (int s = live; s < n_seg; ++s) CHECK(s >= chunks, "segment %d of %d has a chunk", s, n_seg);
            for (int64_t r = 0; r < N; ++r) CHECK(seen[(size_t)r] == 1, "row %lld seen %d times", (long long)r, seen[(size_t)r]);
        }
    }
    // the knob and the auto rule
    for (int64_t N : {0, 1, 256, 257, 100000, 1000000})
        for (int B : {1, 5, 64, 2000}) {
            const int a = sparse_n_seg(0, N, B, 256);
            CHECK(a >= 1 && a <= kSparseMaxSeg, "auto n_seg %d", a);
            CHECK(a <= std::max<int64_t>(1, sparse_n_chunks(N)), "more segments than chunks");
            CHECK((int64_t)a * B <= std::max<int64_t>(B, 256 * kSparseWgPerCu), "grid too large: %d x %d", a, B);
            for (int64_t knob : {1, 2, 7, 512, 9999})
                CHECK(sparse_n_seg(knob, N, B, 256) == (int)std::min<int64_t>(knob, kSparseMaxSeg), "knob %lld", (long long)knob);
        }
    CHECK(sparse_ke(1) == 32 && sparse_ke(32) == 32 && sparse_ke(33) == 64 && sparse_ke(200) == 256 && sparse_ke(1024) == 1024,
          "the top-k width");
}

static void check_query_range() {
    const int64_t big = (int64_t)1 << 62;
    for (int64_t q_nnz : {0, 1, 5, 1024, 1025, 5000})
        for (int64_t lo : {-big, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)4, q_nnz - 1, q_nnz, q_nnz + 1, big})
            for (int64_t hi : {-big, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)5, lo + 1024, lo + 1025, q_nnz, q_nnz + 1, big}) {
                const SparseQRange r = sparse_query_range(lo, hi, q_nnz);
                CHECK(r.o0 >= 0 && r.o0 <= q_nnz && r.len >= 0 && r.o0 + r.len <= q_nnz, "range outside [0, q_nnz]");
                CHECK(r.len <= kSparseMaxQueryTerms, "a range longer than a query");
                const bool good = lo >= 0 && hi >= lo && hi <= q_nnz && hi - lo <= kSparseMaxQueryTerms;
                CHECK(r.bad == !good, "lo %lld hi %lld nnz %lld: bad %d", (long long)lo, (long long)hi, (long long)q_nnz, r.bad);
                if (good) CHECK(r.o0 == lo && r.len == hi - lo, "a good range changed");
                else CHECK(r.len == 0, "a bad range reads entries");
            }
    CHECK(sparse_term_ok(0, -1, 1) && sparse_term_ok(4, 3, 5) && !sparse_term_ok(5, 3, 5) && !sparse_term_ok(3, 3, 5) &&
              !sparse_term_ok(2, 3, 5) && !sparse_term_ok(-1, -1, 5) && sparse_term_ok(2147483646, 7, 2147483647),
          "term eligibility");
    for (float w : {0.0f, -0.0f, 1.0f, -3.5f, std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(),
                    std::numeric_limits<float>::denorm_min()})
        CHECK(sparse_weight_ok(w), "weight %g refused", w);
    for (float w : {kNanF, kInfF, -kInfF}) CHECK(!sparse_weight_ok(w), "weight %g accepted", w);
}

static void check_find_and_key() {
    std::mt19937_64 rng(7);
    for (int len : {0, 1, 2, 3, 63, 64, 65, 1000, 1024}) {
        for (int32_t n_terms : {5, 30522, 2147483647}) {
            if (len > n_terms) continue;
            // len distinct ascending terms, with 0 and n_terms - 1 among them when there is room
            std::vector<int32_t> qt;
            std::map<int32_t, int> pos;
            while ((int)pos.size() < len) {
                int32_t t = (int32_t)(rng() % (uint64_t)n_terms);
                if (pos.size() == 0) t = 0;
                if (pos.size() == 1) t = n_terms - 1;
                pos[t] = 0;
            }
            for (auto& kv : pos) {
                kv.second = (int)qt.size();
                qt.push_back(kv.first);
            }
            for (int i = 0; i < len; ++i) CHECK(sparse_find(qt.data(), len, qt[(size_t)i]) == i, "listed term not found");
            for (int t = 0; t < 200; ++t) {
                const int32_t x = (int32_t)(rng() % (uint64_t)n_terms);
                const auto it = pos.find(x);
                CHECK(sparse_find(qt.data(), len, x) == (it == pos.end() ? -1 : it->second), "term %d", x);
            }
            CHECK(sparse_find(qt.data(), len, -1) == -1 && sparse_find(qt.data(), len, 2147483647) == -1, "outside terms");
            // the key of random rows: the listed pairs alone against every pair over a dense map
            std::vector<float> qw((size_t)len);
            for (auto& w : qw) w = (float)((int)(rng() % 9) - 4) * 0.37f;
            for (int trial = 0; trial < 20; ++trial) {
                const int n_e = (int)(rng() % 70);
                std::map<int32_t, float> rowm;
                for (int e = 0; e < n_e; ++e) {
                    const int32_t t = (len > 0 && rng() % 2) ? qt[(size_t)(rng() % (uint64_t)len)] : (int32_t)(rng() % (uint64_t)n_terms);
                    rowm[t] = (float)((int)(rng() % 7) - 3) * 1.25f;
                }
                std::vector<SparsePair> row;
                for (auto& kv : rowm) row.push_back(SparsePair{kv.first, kv.second});
                bool matched = false;
                const double key = sparse_row_key(row.data(), (int64_t)row.size(), qt.data(), qw.data(), len, &matched);
                double acc = 0.0;
                bool m = false;
                for (const SparsePair& p : row) {  // the contract's first form: every entry, qd = 0.0 when not listed
                    const auto it = pos.find(p.term);
                    const double qd = it == pos.end() ? 0.0 : (double)qw[(size_t)it->second];
                    const double prod = (double)p.weight * qd;
                    acc = acc + prod;
                    m = m || (p.weight != 0.0f && qd != 0.0);
                }
                uint64_t a, b;
                std::memcpy(&a, &key, 8);
                std::memcpy(&b, &acc, 8);
                CHECK(a == b && matched == m, "row key %a against %a", key, acc);
                CHECK(!(key == 0.0 && std::signbit(key)), "a key of -0.0");
            }
        }
    }
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
    for (int B : {1, 5, 64})
        for (int k : {1, 10, 200, 1024})
            for (int n_seg : {1, 2, 7, 512})
                for (int64_t q_nnz : {0, 1, 1024, 70000})
                    for (int64_t rows : {0, 3, 1300, 1000000})
                        for (int flags = 0; flags < 8; ++flags) {
                            const bool host = flags & 1, masked = flags & 2, keys = flags & 4;
                            const int64_t KE = sparse_ke(k);
                            const SparseScratch s = sparse_scratch(B, k, n_seg, q_nnz, rows, host, masked, keys);
                            std::vector<std::pair<int64_t, int64_t>> r = {
                                {s.done, B * 4},
                                {s.lk, n_seg > 1 ? (int64_t)B * n_seg * KE * 8 : 0},
                                {s.li, n_seg > 1 ? (int64_t)B * n_seg * KE * 4 : 0},
                                {s.mk, n_seg > 1 ? B * KE * 8 : 0},
                                {s.mi, n_seg > 1 ? B * KE * 4 : 0}};
                            if (host) {
                                r.push_back({s.indptr, (B + 1) * 8});
                                r.push_back({s.terms, q_nnz * 4});
                                r.push_back({s.weights, q_nnz * 4});
                                r.push_back({s.mask, masked ? s.mask_words * 4 : 0});
                                r.push_back({s.out_s, (int64_t)B * k * 4});
                                r.push_back({s.out_i, (int64_t)B * k * 8});
                                r.push_back({s.out_k, keys ? (int64_t)B * k * 8 : 0});
                                CHECK(s.in0 <= s.indptr && s.mask + (masked ? s.mask_words * 4 : 0) <= s.in0 + s.in_bytes,
                                      "staged arguments outside [in0, in0 + in_bytes)");
                                CHECK(s.out0 == s.in0 + s.in_bytes && s.out0 + s.out_bytes == s.total, "staging not back to back");
                            } else {
                                CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device call stages");
                            }
                            CHECK(s.mask_words == (rows + 31) / 32, "mask words");
                            check_ranges_disjoint(r, s.total, "sparse scratch");
                        }
    for (int B : {1, 5, 64})
        for (int k : {1, 10, 200})
            for (int F : {k, 200})
                for (int n_seg : {1, 7})
                    for (int64_t q_nnz : {0, 1024})
                        for (int64_t rows : {0, 1300})
                            for (int flags = 0; flags < 16; ++flags) {
                                const bool host = flags & 1, masked = flags & 2, fused = flags & 4, hits = flags & 8;
                                const int dim = 48;
                                const int64_t KE = sparse_ke(F);
                                const HybridScratch s = hybrid_scratch(B, dim, k, F, n_seg, q_nnz, rows, host, masked, fused, hits);
                                std::vector<std::pair<int64_t, int64_t>> r = {
                                    {s.ds, (int64_t)B * F * 4}, {s.di, (int64_t)B * F * 8}, {s.dk, (int64_t)B * F * 8},
                                    {s.fs, (int64_t)2 * B * F * 4}, {s.fi, (int64_t)2 * B * F * 8}, {s.fk, (int64_t)2 * B * F * 8},
                                    {s.offs, (B + 1) * 8}, {s.w, 2 * B * 8}, {s.done, B * 4},
                                    {s.lk, n_seg > 1 ? (int64_t)B * n_seg * KE * 8 : 0},
                                    {s.li, n_seg > 1 ? (int64_t)B * n_seg * KE * 4 : 0},
                                    {s.mk, n_seg > 1 ? B * KE * 8 : 0}, {s.mi, n_seg > 1 ? B * KE * 4 : 0}};
                                if (host) {
                                    r.push_back({s.q, (int64_t)B * dim * 4});
                                    r.push_back({s.indptr, (B + 1) * 8});
                                    r.push_back({s.terms, q_nnz * 4});
                                    r.push_back({s.weights, q_nnz * 4});
                                    r.push_back({s.mask, masked ? (s.mask_words + 64) * 4 : 0});
                                    r.push_back({s.out_s, (int64_t)B * k * 4});
                                    r.push_back({s.out_i, (int64_t)B * k * 8});
                                    r.push_back({s.out_f, fused ? (int64_t)B * k * 8 : 0});
                                    r.push_back({s.out_h, hits ? (int64_t)B * k * 4 : 0});
                                    CHECK(s.out0 == s.in0 + s.in_bytes && s.out0 + s.out_bytes == s.total, "staging not back to back");
                                }
                                check_ranges_disjoint(r, s.total, "hybrid scratch");
                                // the sparse list of the last query ends inside fs / fi / fk: list 2 b + 1 of [2 B][F]
                                CHECK(((int64_t)(B - 1) * 2 * F + F + F) * 8 <= (int64_t)2 * B * F * 8, "the odd lists leave fi");
                            }
    // LDS: the query and the four buffers at k = 1024 (capacity 2048 entries of 12 bytes) stay inside 160 KiB
    CHECK(sparse_lds_bytes(2048, 2048 * 12) == 8192 + 4 * 2048 * 12, "LDS at k = 1024");
    CHECK(sparse_lds_bytes(2048, 2048 * 12) <= 160 * 1024, "LDS budget");
    CHECK(sparse_lds_bytes(128, 1024 * 12) == 8192 + 1024 * 12, "the merge buffer is the larger at k = 32");
    CHECK(kSparseQueryLds % 16 == 0, "the top-k buffers start 16-byte aligned");
}

static void check_column() {
    CHECK(sparse_column_args(false, false, false, 0, 0, 0, 77) == kSparseColOk, "detach refused");
    CHECK(sparse_column_args(false, false, false, 3, 0, 1, 3) == kSparseColBadCounts, "NULL indptr with rows");
    CHECK(sparse_column_args(true, true, true, 3, 5, 10, 3) == kSparseColOk, "a plain column refused");
    CHECK(sparse_column_args(true, false, false, 3, 0, 10, 3) == kSparseColOk, "an all-empty column needs no arrays");
    CHECK(sparse_column_args(true, true, true, 0, 0, 1, 0) == kSparseColOk, "an empty column on an empty index");
    CHECK(sparse_column_args(true, true, true, 2, 5, 10, 3) == kSparseColBadCounts, "n != count");
    CHECK(sparse_column_args(true, true, true, 3, -1, 10, 3) == kSparseColBadCounts, "nnz < 0");
    CHECK(sparse_column_args(true, true, true, 3, 5, 0, 3) == kSparseColBadCounts, "n_terms 0");
    CHECK(sparse_column_args(true, true, true, 3, 5, 2147483647, 3) == kSparseColOk, "n_terms 2^31 - 1");
    CHECK(sparse_column_args(true, false, true, 3, 5, 10, 3) == kSparseColNullPointer, "NULL terms");
    CHECK(sparse_column_args(true, true, false, 3, 5, 10, 3) == kSparseColNullPointer, "NULL weights");

    const int64_t ind[] = {0, 2, 2, 5};
    const int32_t t[] = {0, 9, 1, 4, 7};
    const float w[] = {1.f, -2.f, 0.f, 3.f, .5f};
    int64_t at = -1;
    CHECK(sparse_validate_column(ind, t, w, 3, 5, 10, &at) == kSparseColOk, "a good column refused");
    struct Bad { std::vector<int64_t> ind; std::vector<int32_t> t; std::vector<float> w; int64_t nnz; int32_t nt; int cause; int64_t row; };
    const std::vector<Bad> bad = {
        {{1, 2, 2, 5}, {0, 9, 1, 4, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColBadIndptr, 0},
        {{0, 1, 0, 5}, {0, 9, 1, 4, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColBadIndptr, 1},
        {{0, 2, 2, 4}, {0, 9, 1, 4, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColBadIndptr, 2},
        {{0, 2, 2, 6}, {0, 9, 1, 4, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColBadIndptr, 2},
        {{0, -1, 2, 5}, {0, 9, 1, 4, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColBadIndptr, 0},
        {{0, 2, 2, 5}, {0, 10, 1, 4, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColBadTerm, 0},
        {{0, 2, 2, 5}, {-1, 9, 1, 4, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColBadTerm, 0},
        {{0, 2, 2, 5}, {0, 9, 1, 1, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColUnsorted, 2},
        {{0, 2, 2, 5}, {0, 9, 4, 1, 7}, {1, 1, 1, 1, 1}, 5, 10, kSparseColUnsorted, 2},
        {{0, 2, 2, 5}, {0, 9, 1, 4, 7}, {1, 1, 1, kInfF, 1}, 5, 10, kSparseColNonFinite, 2},
        {{0, 2, 2, 5}, {0, 9, 1, 4, 7}, {1, kNanF, 1, 1, 1}, 5, 10, kSparseColNonFinite, 0},
    };
    for (size_t i = 0; i < bad.size(); ++i) {
        const Bad& b = bad[i];
        CHECK(sparse_validate_column(b.ind.data(), b.t.data(), b.w.data(), 3, b.nnz, b.nt, &at) == b.cause && at == b.row,
              "bad column %zu: row %lld", i, (long long)at);
        // the device form: a flag word of the rows' causes reports the same cause when only one is planted
        uint32_t flags = 0;
        for (int64_t r = 0; r < 3; ++r)
            if (!sparse_column_offsets_ok(b.ind.data(), r, 3, b.nnz)) flags |= sparse_column_flag(kSparseColBadIndptr);
        if (!flags)
            for (int64_t r = 0; r < 3; ++r)
                flags |= sparse_column_flag(sparse_column_row(b.ind.data(), b.t.data(), b.w.data(), r, b.nt));
        CHECK(sparse_column_cause(flags) == b.cause, "bad column %zu: flags %u", i, flags);
    }
    CHECK(sparse_column_cause(0) == kSparseColOk, "no flag is no cause");
    // garbage offsets: a row's entries are read only when its range lies inside [0, nnz] (ASan watches)
    std::mt19937_64 rng(11);
    for (int trial = 0; trial < 2000; ++trial) {
        const int64_t n = 1 + (int64_t)(rng() % 6), nnz = (int64_t)(rng() % 9);
        std::vector<int64_t> gi((size_t)n + 1);
        for (auto& v : gi) v = (int64_t)(rng() % 14) - 3;
        if (rng() % 4 == 0) gi[rng() % gi.size()] = (int64_t)1 << 61;
        std::vector<int32_t> gt((size_t)nnz);
        std::vector<float> gw((size_t)nnz, 1.0f);
        for (auto& v : gt) v = (int32_t)(rng() % 12) - 2;
        if (trial % 3 == 0) {  // (and some that pass the first pass)
            std::sort(gi.begin(), gi.end());
            gi.front() = 0;
            gi.back() = nnz;
        }
        bool offsets_ok = true;
        for (int64_t r = 0; r < n; ++r) offsets_ok = offsets_ok && sparse_column_offsets_ok(gi.data(), r, n, nnz);
        if (!offsets_ok) continue;  // the second pass does not run
        int64_t walked = 0;
        for (int64_t r = 0; r < n; ++r) {
            (void)sparse_column_row(gi.data(), gt.data(), gw.data(), r, 8);
            walked += gi[(size_t)r + 1] - gi[(size_t)r];
        }
        CHECK(walked == nnz, "the rows walked do not tile: %lld entries of %lld", (long long)walked, (long long)nnz);
    }
    const int64_t zero[] = {0}, one[] = {1};
    CHECK(sparse_validate_column(zero, nullptr, nullptr, 0, 0, 1, &at) == kSparseColOk, "the empty column refused");
    CHECK(sparse_validate_column(one, nullptr, nullptr, 0, 0, 1, &at) == kSparseColBadIndptr, "indptr[0] != 0 accepted");
}

static void check_calls() {
    auto v = [](int64_t B, int64_t nnz, int k, bool ip = true, bool t = true, bool w = true, bool s = true, bool i = true,
                int mem = 0, bool col = true) { return sparse_validate_call(B, nnz, k, ip, t, w, s, i, mem, col); };
    CHECK(v(3, 10, 10) == kSparseOk, "a plain call refused");
    CHECK(v(0, 0, 1, false, false, false, false, false, 1) == kSparseOk, "an empty call refused");
    CHECK(v(3, 0, 10, true, false, false) == kSparseOk, "queries without terms need no arrays");
    CHECK(v(-1, 0, 1) == kSparseBadCounts && v(1, -1, 1) == kSparseBadCounts, "counts");
    for (int k = -2; k <= kSparseMaxK + 2; ++k)
        CHECK(v(1, 1, k) == ((k < 1 || k > kSparseMaxK) ? kSparseBadK : kSparseOk), "k %d", k);
    CHECK(v(1, 1, 1, false) == kSparseNullPointer && v(1, 1, 1, true, false) == kSparseNullPointer &&
              v(1, 1, 1, true, true, false) == kSparseNullPointer && v(1, 1, 1, true, true, true, false) == kSparseNullPointer &&
              v(1, 1, 1, true, true, true, true, false) == kSparseNullPointer,
          "NULL pointers");
    CHECK(v(1, 1, 1, true, true, true, true, true, 2) == kSparseBadMem, "mem 2");
    CHECK(v(1, 1, 1, true, true, true, true, true, 0, false) == kSparseNoColumn, "no column");

    auto h = [](int k, int f, double wd, double ws, double c, bool q = true, bool col = true) {
        return hybrid_validate_call(2, 4, k, f, wd, ws, c, q, true, true, true, true, true, 0, col);
    };
    CHECK(h(10, 40, 1.0, 1.0, 60.0) == kSparseOk, "a plain hybrid call refused");
    for (int k = -1; k <= kFuseMaxK + 1; ++k)
        for (int f = -1; f <= kFuseMaxFetch + 1; ++f) {
            const int want = (k < 1 || k > kFuseMaxK) ? kSparseBadK : (f < k || f > kFuseMaxFetch) ? kHybridBadFetch : kSparseOk;
            CHECK(h(k, f, 1.0, 1.0, 60.0) == want, "k %d fetch %d", k, f);
        }
    for (double x : {-1.0, kNan, kInf, -kInf}) {
        CHECK(h(1, 1, x, 1.0, 60.0) == kHybridBadWeight && h(1, 1, 1.0, x, 60.0) == kHybridBadWeight, "weight %g", x);
        CHECK(h(1, 1, 1.0, 1.0, x) == kHybridBadC, "rrf_c %g", x);
    }
    CHECK(h(1, 1, 0.0, 0.0, 0.0) == kSparseOk, "zeros refused");
    CHECK(h(1, 1, 1.0, 1.0, 60.0, false) == kSparseNullPointer, "NULL dense queries");
    CHECK(h(1, 1, 1.0, 1.0, 60.0, true, false) == kSparseNoColumn, "no column");

    // a host call's queries, one cause at a time; the device rule agrees on which queries are bad
    const int32_t nt = 30522;
    std::vector<int64_t> ip = {0, 2, 2, 5};
    std::vector<int32_t> t = {0, 30521, 3, 4, 9};
    std::vector<float> w = {1.f, 0.f, -2.f, 3.f, .5f};
    int64_t at = -1;
    CHECK(sparse_validate_queries(ip.data(), t.data(), w.data(), 3, 5, nt, &at) == kSparseOk, "good queries refused");
    for (int b = 0; b < 3; ++b) CHECK(!sparse_query_bad(ip.data(), t.data(), w.data(), b, 5, nt), "good query %d bad", b);
    struct Case { std::vector<int64_t> ip; std::vector<int32_t> t; std::vector<float> w; int cause; std::vector<int> bad; };
    const std::vector<Case> cases = {
        {{0, 3, 2, 5}, t, w, kSparseBadOffsets, {0, 1}},  // (query 0 then reads the unsorted 0, 30521, 3)
        {{0, 2, 2, 6}, t, w, kSparseBadOffsets, {2}},
        {{-1, 2, 2, 5}, t, w, kSparseBadOffsets, {0}},
        {ip, {0, 30522, 3, 4, 9}, w, kSparseBadTerm, {0}},
        {ip, {-1, 30521, 3, 4, 9}, w, kSparseBadTerm, {0}},
        {ip, {0, 30521, 3, 3, 9}, w, kSparseUnsorted, {2}},
        {ip, {0, 30521, 4, 3, 9}, w, kSparseUnsorted, {2}},
        {ip, t, {1.f, 0.f, -2.f, kNanF, .5f}, kSparseNonFinite, {2}},
        {ip, t, {1.f, -kInfF, -2.f, 3.f, .5f}, kSparseNonFinite, {0}},
    };
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        CHECK(sparse_validate_queries(c.ip.data(), c.t.data(), c.w.data(), 3, 5, nt, &at) == c.cause, "query case %zu", i);
        for (int b = 0; b < 3; ++b) {
            const bool want = std::find(c.bad.begin(), c.bad.end(), b) != c.bad.end();
            CHECK(sparse_query_bad(c.ip.data(), c.t.data(), c.w.data(), b, 5, nt) == want, "query case %zu query %d", i, b);
        }
    }
    // 1 024 terms pass, 1 025 do not
    std::vector<int32_t> lt(1025);
    std::vector<float> lw(1025, 1.0f);
    for (int i = 0; i < 1025; ++i) lt[(size_t)i] = i;
    const int64_t ip1024[] = {0, 1024}, ip1025[] = {0, 1025};
    CHECK(sparse_validate_queries(ip1024, lt.data(), lw.data(), 1, 1024, nt, &at) == kSparseOk, "1 024 terms refused");
    CHECK(sparse_validate_queries(ip1025, lt.data(), lw.data(), 1, 1025, nt, &at) == kSparseTooLong && at == 0, "1 025 terms");
    CHECK(!sparse_query_bad(ip1024, lt.data(), lw.data(), 0, 1024, nt) && sparse_query_bad(ip1025, lt.data(), lw.data(), 0, 1025, nt),
          "the device rule on 1 024 / 1 025 terms");
}

int main() {
    check_deal();
    check_query_range();
    check_find_and_key();
    check_scratch();
    check_column();
    check_calls();
    std::printf("sparse plan ok (%ld checks)\n", g_checks);
    return 0;
}
