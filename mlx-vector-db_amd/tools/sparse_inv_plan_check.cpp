// sparse_inv_plan_check.cpp — the host arithmetic of the inverted sparse search
// (csrc/vdb_sparse_inv_plan.h) swept on the CPU against naive loops: R(KE) and the LDS layout
// (disjoint, inside 160 KiB), the deal of row blocks to segments and waves (every row exactly once),
// the lower bound and a term's range in a wave's rows, when postings are built and serve, and the
// walk of the postings as the kernel does it (blocks, waves, terms ascending, one accumulator a row)
// against sparse_row_key over the stored rows, bit for bit, on random columns.  A stand-alone host
// program (its own main, no GPU, nothing loaded into another process); `make sparse-inv-plan-check`
// builds it with -fsanitize=address,undefined and -ffp-contract=off and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../csrc/vdb_sparse_inv_plan.h"

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

static void check_lds_and_choice() {
    for (int KE = 32; KE <= kSparseMaxK; KE <<= 1) {
        const int R = sparse_inv_block_rows(KE);
        CHECK(R == (KE <= 512 ? 8192 : 4096), "R(%d) = %d", KE, R);
        CHECK(R % (kSparseWaves * 64) == 0 && (R & (R - 1)) == 0, "R %d", R);
        int64_t cap = 1;
        while (cap < std::max(2 * KE, KE + 64)) cap <<= 1;
        CHECK(sparse_inv_topk_cap(KE) == cap, "cap(%d)", KE);
        CHECK(sparse_inv_merge_lds(KE) == std::max<int64_t>(cap, 1024) * 12, "merge lds(%d)", KE);
        for (bool merge : {false, true}) {
            const SparseInvLds l = sparse_inv_lds(R, KE, merge);
            CHECK(l.acc == kSparseQueryLds && l.flags == l.acc + 8 * (int64_t)R, "acc / flags");
            CHECK(l.tk >= l.flags + R / 8 && l.tk % 16 == 0, "top-k buffers overlap the flags");
            CHECK(l.total >= l.tk + 4 * cap * 12 && (!merge || l.total >= l.tk + sparse_inv_merge_lds(KE)), "total");
            CHECK(l.total <= kSparseInvLdsLimit, "KE %d: %lld bytes of LDS", KE, (long long)l.total);
        }
        if (R < kSparseInvMaxBlockRows) CHECK(sparse_inv_lds(2 * R, KE, true).total > kSparseInvLdsLimit, "a larger R fits");
    }
    for (int64_t knob : {-1, 0, 1, 2, 3}) CHECK(sparse_inv_knob_ok(knob) == (knob >= 0 && knob <= 2), "knob %lld", (long long)knob);
    for (int64_t knob : {0, 1, 2})
        for (int32_t nt : {1, 30522, kSparseInvMaxTerms, kSparseInvMaxTerms + 1, 2147483647}) {
            CHECK(sparse_inv_builds(knob, nt) == (knob != 2 && nt <= kSparseInvMaxTerms), "builds");
            for (bool built : {false, true})
                for (int64_t N : {(int64_t)0, kSparseInvAutoRows - 1, kSparseInvAutoRows, (int64_t)1 << 31})
                    CHECK(sparse_inv_serves(knob, built, N) == (built && (knob == 1 || (knob == 0 && N >= kSparseInvAutoRows))),
                          "serves knob %lld built %d N %lld", (long long)knob, (int)built, (long long)N);
        }
    for (int32_t nt : {1, 2, 3, 5, 256, 257, 30522, kSparseInvMaxTerms}) {
        const int b = sparse_inv_term_bits(nt);
        CHECK(b >= 1 && ((int64_t)1 << b) >= nt && (b == 1 || ((int64_t)1 << (b - 1)) < nt), "bits(%d) = %d", nt, b);
    }
}

static void check_deal() {
    for (int R : {256, 4096, 8192})
        for (int64_t N : {0, 1, 65, 2047, 2049, 4095, 4097, 8193, 3 * 8192 + 5}) {
            const int64_t blocks = sparse_inv_n_blocks(N, R);
            CHECK(blocks == (N + R - 1) / R, "blocks");
            for (int n_seg : {1, 2, 7, 512}) {
                const int live = sparse_inv_live_segs(N, R, n_seg);
                CHECK(live == (int)std::min<int64_t>(blocks, n_seg), "live");
                std::vector<int> seen((size_t)N, 0);
                for (int s = 0; s < live; ++s)
                    for (int64_t c = s; c < blocks; c += n_seg)
                        for (int wv = 0; wv < kSparseWaves; ++wv) {
                            const SparseInvRows r = sparse_inv_wave_rows(c, wv, R, N);
                            CHECK(r.lo <= r.hi && r.hi <= N && r.hi - r.lo <= R / 4, "wave rows");
                            CHECK(r.lo >= r.hi || (r.lo >= c * R + wv * (R / 4) && r.hi <= c * R + (wv + 1) * (R / 4)), "outside the quarter");
                            for (int64_t x = r.lo; x < r.hi; ++x) ++seen[(size_t)x];
                        }
                for (int64_t x = 0; x < N; ++x) CHECK(seen[(size_t)x] == 1, "row %lld seen %d times", (long long)x, seen[(size_t)x]);
            }
        }
}

// A random column (ascending terms within a row, zero and negative weights among them), its postings
// by a stable sort, and queries against it: the kernel's walk against sparse_row_key.
static void check_walk(std::mt19937& rng, int64_t N, int32_t n_terms, int R) {
    std::vector<int64_t> indptr(1, 0);
    std::vector<SparsePair> pairs;
    for (int64_t r = 0; r < N; ++r) {
        const int len = (int)(rng() % 9) * (rng() % 4 == 0 ? 0 : 1);
        std::vector<int32_t> ts;
        for (int i = 0; i < len; ++i) ts.push_back((int32_t)(rng() % (uint32_t)n_terms));
        if (rng() % 3 == 0) ts.push_back(0);  // a term most rows hold
        std::sort(ts.begin(), ts.end());
        ts.erase(std::unique(ts.begin(), ts.end()), ts.end());
        for (int32_t t : ts) pairs.push_back(SparsePair{t, (float)((int)(rng() % 9) - 3) * (rng() % 2 ? 0.37f : 1.0f)});
        indptr.push_back((int64_t)pairs.size());
    }
    const int64_t nnz = (int64_t)pairs.size();
    // the postings: (term, row) order defines them
    std::vector<int64_t> order((size_t)nnz), row_of((size_t)nnz);
    for (int64_t r = 0; r < N; ++r)
        for (int64_t e = indptr[(size_t)r]; e < indptr[(size_t)r + 1]; ++e) row_of[(size_t)e] = r;
    for (int64_t e = 0; e < nnz; ++e) order[(size_t)e] = e;
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return pairs[(size_t)x].term < pairs[(size_t)y].term; });
    std::vector<SparsePost> posts((size_t)nnz);
    std::vector<int64_t> tptr((size_t)n_terms + 1, 0);
    for (int64_t i = 0; i < nnz; ++i) {
        posts[(size_t)i] = SparsePost{(uint32_t)row_of[(size_t)order[(size_t)i]], pairs[(size_t)order[(size_t)i]].weight};
        ++tptr[(size_t)pairs[(size_t)order[(size_t)i]].term + 1];
    }
    for (int32_t t = 0; t < n_terms; ++t) tptr[(size_t)t + 1] += tptr[(size_t)t];
    // lower bound and range against naive loops
    for (int rep = 0; rep < 50; ++rep) {
        const int32_t t = (int32_t)(rng() % (uint32_t)n_terms);
        const int64_t b = tptr[(size_t)t], e = tptr[(size_t)t + 1];
        const int64_t row = (int64_t)(rng() % (uint64_t)(N + 2));
        int64_t want = b;
        while (want < e && (int64_t)posts[(size_t)want].row < row) ++want;
        CHECK(sparse_inv_lower_bound(posts.data(), b, e, row) == want, "lower bound");
    }
    for (int qn = 0; qn < 6; ++qn) {
        std::vector<int32_t> qt;
        const int want_len = qn == 0 ? 0 : qn == 1 ? 1 : (int)std::min<int64_t>(n_terms, qn == 2 ? 200 : 7);
        for (int i = 0; i < want_len; ++i) qt.push_back(i == 0 ? 0 : (int32_t)(rng() % (uint32_t)n_terms));
        std::sort(qt.begin(), qt.end());
        qt.erase(std::unique(qt.begin(), qt.end()), qt.end());
        std::vector<float> qw;
        for (size_t i = 0; i < qt.size(); ++i) qw.push_back((float)((int)(rng() % 7) - 2) * 0.73f);
        const int len = (int)qt.size();
        // the kernel's walk: blocks, waves, terms ascending, one accumulator and one flag a row
        std::vector<double> acc((size_t)N, 0.0);
        std::vector<char> flag((size_t)N, 0);
        for (int64_t c = 0; c < sparse_inv_n_blocks(N, R); ++c)
            for (int wv = 0; wv < kSparseWaves; ++wv) {
                const SparseInvRows rows = sparse_inv_wave_rows(c, wv, R, N);
                for (int j = 0; j < len && rows.lo < rows.hi; ++j) {
                    int64_t p0, p1;
                    sparse_inv_range(tptr.data(), posts.data(), qt[(size_t)j], rows, &p0, &p1);
                    int64_t n0 = tptr[(size_t)qt[(size_t)j]], n1;
                    while (n0 < tptr[(size_t)qt[(size_t)j] + 1] && (int64_t)posts[(size_t)n0].row < rows.lo) ++n0;
                    for (n1 = n0; n1 < tptr[(size_t)qt[(size_t)j] + 1] && (int64_t)posts[(size_t)n1].row < rows.hi;) ++n1;
                    CHECK(p0 == n0 && p1 == n1, "range of term %d in rows [%lld, %lld)", qt[(size_t)j], (long long)rows.lo, (long long)rows.hi);
                    for (int64_t p = p0; p < p1; ++p) {
                        const uint32_t r = posts[(size_t)p].row;
                        const double qd = (double)qw[(size_t)j];
                        acc[r] = sparse_step(acc[r], posts[(size_t)p].weight, qd);
                        if (sparse_entry_matches(posts[(size_t)p].weight, qd)) flag[r] = 1;
                    }
                }
            }
        for (int64_t r = 0; r < N; ++r) {
            bool m = false, mi = false;
            const double want = sparse_row_key(pairs.data() + indptr[(size_t)r], indptr[(size_t)r + 1] - indptr[(size_t)r], qt.data(),
                                               qw.data(), len, &m);
            const double inv = sparse_inv_row_key(tptr.data(), posts.data(), r, qt.data(), qw.data(), len, &mi);
            CHECK(std::memcmp(&want, &acc[(size_t)r], 8) == 0 && m == (flag[(size_t)r] != 0), "row %lld: walk %a, rows %a", (long long)r,
                  acc[(size_t)r], want);
            CHECK(std::memcmp(&want, &inv, 8) == 0 && m == mi, "row %lld: by postings %a, rows %a", (long long)r, inv, want);
            // a row that was added to but never matched holds +0.0 (the kernel skips clearing it)
            if (!m) CHECK(std::memcmp(&acc[(size_t)r], "\0\0\0\0\0\0\0\0", 8) == 0, "an unmatched row's accumulator is not +0.0");
        }
    }
}

int main() {
    check_lds_and_choice();
    check_deal();
    std::mt19937 rng(12345);
    for (int R : {256, 4096})
        for (int64_t N : {1, 65, 257, 2049, 4097})
            for (int32_t n_terms : {1, 5, 300}) check_walk(rng, N, n_terms, R);
    std::printf("sparse inverted plan ok (%ld checks)\n", g_checks);
    return 0;
}
