// filter_plan_check.cpp — the host arithmetic of vdb_index_set_column / vdb_index_filter_mask
// (csrc/vdb_filter_plan.h) swept on the CPU against naive loops.  Stand-alone: build with
// -fsanitize=address,undefined (make filter-plan-check) and run; every buffer is a heap allocation
// of exactly the size the library gives it, so a word, a staged clause or a scratch extent that is
// off by one is an out-of-bounds access the sanitizer reports, and a row visited twice or never, a
// high word written where none exists or a wrong bit is a mismatch reported here.
//
// The model follows the kernel (csrc/vdb_filter.hip) step by step: the clauses staged in the layout
// of filter_stage, the deal of word pairs to workgroups, waves and trips, a lane per row with tail
// rows never loaded, the ballot's two words, the base AND, the two 32-bit stores with the last-word
// rule, and the counts as sums of popcounts.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/vdb_filter_plan.h"

using namespace vdb;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__); \
            std::fprintf(stderr, "\n");       \
            if (++g_fail > 20) std::exit(1);  \
        }                                     \
    } while (0)

template <typename T>
T* exact_alloc(size_t n) {  // exactly n elements (n == 0: a 1-byte block nothing may touch as T)
    return (T*)std::malloc(n ? n * sizeof(T) : 1);
}

const double kInf = std::numeric_limits<double>::infinity();
const double kNan = std::numeric_limits<double>::quiet_NaN();

// The definition, written out without the header's helper.
bool naive_clause(double v, int col_flags, double lo, double hi) {
    if (std::isnan(v)) return (col_flags & 4) != 0;
    bool t = true;
    if (col_flags & 1) { if (!(v >= lo)) t = false; } else { if (!(v > lo)) t = false; }
    if (col_flags & 2) { if (!(v <= hi)) t = false; } else { if (!(v < hi)) t = false; }
    return (col_flags & 4) ? !t : t;
}

void check_clause_semantics() {
    const double vals[] = {kNan, -kInf, -2.5, -0.0, 0.0, 1.0, 3.0, 1e300, kInf};
    const double bounds[] = {-kInf, -2.5, -0.0, 0.0, 1.0, 3.0, kInf};
    for (double v : vals)
        for (double lo : bounds)
            for (double hi : bounds)
                for (int f = 0; f < 8; ++f) {
                    const FilterClause c{0, f, lo, hi};
                    CHECK(clause_passes(v, c) == naive_clause(v, f, lo, hi), "v %g [%g, %g] flags %d", v, lo, hi, f);
                }
    // the two idioms of the header: equality and "exists"; -0.0 equals +0.0
    CHECK(clause_passes(-0.0, FilterClause{0, 3, 0.0, 0.0}), "-0 == +0");
    CHECK(clause_passes(kInf, FilterClause{0, 3, -kInf, kInf}) && !clause_passes(kNan, FilterClause{0, 3, -kInf, kInf}),
          "exists");
    CHECK(clause_passes(kNan, FilterClause{0, 7, 1.0, 1.0}) && !clause_passes(kNan, FilterClause{0, 0, -kInf, kInf}),
          "a row without a value: plain fails, negated passes");
    CHECK(!clause_passes(1.0, FilterClause{0, 3, 2.0, 0.0}) && clause_passes(1.0, FilterClause{0, 7, 2.0, 0.0}), "lo > hi");
}

// One call, the way the kernel runs it, against the naive per-row loop.
void run_case(int64_t N, int n_cols, const std::vector<std::vector<double>>& cols, const std::vector<FilterClause>& cl,
              const std::vector<int32_t>& off, const uint32_t* base, int n_cu) {
    const int32_t P = (int32_t)off.size() - 1;
    const int64_t W = filter_n_words(N);
    CHECK(W * 32 >= N && (W == 0 || (W - 1) * 32 < N), "n_words %lld for %lld rows", (long long)W, (long long)N);
    uint32_t attached = 0;
    for (int s = 0; s < n_cols; ++s) attached |= 1u << s;
    int64_t where = -1;
    uint32_t used = 0;
    const int rc = filter_validate(cl.data(), off.data(), P, attached, &where, &used);
    CHECK(rc == kFilterOk, "a valid call was refused: cause %d at %lld", rc, (long long)where);
    uint32_t want_used = 0;
    for (const FilterClause& c : cl) want_used |= 1u << c.column;
    CHECK(used == want_used, "used slots %x, want %x", used, want_used);

    // staging: a block of exactly filter_stage's bytes, which never passes kFilterStageBytes
    const FilterStage fs = filter_stage((int32_t)cl.size(), P);
    CHECK(fs.bytes <= kFilterStageBytes && fs.offsets % 256 == 0, "stage %lld bytes", (long long)fs.bytes);
    char* stage = exact_alloc<char>((size_t)fs.bytes);
    if (!cl.empty()) std::memcpy(stage + fs.clauses, cl.data(), cl.size() * sizeof(FilterClause));
    std::memcpy(stage + fs.offsets, off.data(), off.size() * 4);
    const FilterClause* s_cl = (const FilterClause*)(stage + fs.clauses);
    const int32_t* s_off = (const int32_t*)(stage + fs.offsets);

    // the scratch of a host-memory call: the extents are disjoint, aligned and inside total
    for (int hb = 0; hb < 4; ++hb) {
        const FilterScratch sc = filter_scratch(P, N, hb & 1, hb & 2);
        CHECK(sc.n_words == W && sc.stage == 0 && sc.in0 >= kFilterStageBytes, "scratch head");
        CHECK(sc.in0 + sc.in_bytes == sc.out0 && sc.out0 + sc.out_bytes == sc.total, "scratch extents");
        if (hb & 1) {
            CHECK(sc.base == sc.in0 && sc.out_m == sc.out0, "scratch order");
            CHECK(sc.out_m + (int64_t)P * W * 4 <= sc.out_c && sc.out_c + (int64_t)P * 8 <= sc.total, "scratch sizes");
            CHECK(!(hb & 2) || sc.base + (int64_t)P * W * 4 <= sc.out0, "base extent");
            CHECK(sc.out_m % 256 == 0 && sc.out_c % 256 == 0, "scratch alignment");
        } else {
            CHECK(sc.in_bytes == 0 && sc.out_bytes == 0, "a device-memory call stages no masks");
        }
    }

    uint32_t* out = exact_alloc<uint32_t>((size_t)P * (size_t)W);
    std::memset(out, 0xAB, (size_t)P * (size_t)W * 4);
    char* wseen = exact_alloc<char>((size_t)P * (size_t)W);
    std::memset(wseen, 0, (size_t)P * (size_t)W);
    char* rseen = exact_alloc<char>((size_t)N);
    std::memset(rseen, 0, (size_t)N);
    int64_t* counts = exact_alloc<int64_t>((size_t)P);
    for (int32_t p = 0; p < P; ++p) counts[p] = 0;

    const int64_t n_pairs = filter_n_pairs(W);
    const int64_t n_wgs = filter_n_wgs(n_pairs, n_cu);
    const int64_t trips = filter_trips(n_pairs, n_wgs);
    CHECK(n_wgs >= 1 && n_wgs <= (int64_t)(n_cu > 0 ? n_cu : 1) * kFilterWgsPerCu, "n_wgs %lld", (long long)n_wgs);
    CHECK(trips * n_wgs * kFilterWaves >= n_pairs, "the trips cover the pairs");
    if (N > 0) {
        for (int64_t wg = 0; wg < n_wgs; ++wg)
            for (int wave = 0; wave < kFilterWaves; ++wave)
                for (int64_t trip = 0; trip < trips; ++trip) {
                    const int64_t pair = filter_wave_pair(trip, n_wgs, wg, wave);
                    if (pair >= n_pairs) break;
                    const bool high = filter_has_high(pair, W);
                    CHECK(pair * 2 < W, "a pair without a low word");
                    std::vector<double> v((size_t)64 * (size_t)(n_cols > 0 ? n_cols : 1), kNan);
                    bool live[64];
                    for (int lane = 0; lane < 64; ++lane) {
                        const int64_t row = filter_lane_row(pair, lane);
                        live[lane] = filter_row_live(row, N);
                        if (!live[lane]) continue;  // a tail row is never loaded
                        CHECK(!rseen[row], "row %lld visited twice", (long long)row);
                        rseen[row] = 1;
                        for (int s = 0; s < n_cols; ++s)
                            if ((used >> s) & 1u) v[(size_t)lane * n_cols + s] = cols[(size_t)s][(size_t)row];
                    }
                    for (int32_t p = 0; p < P; ++p) {
                        uint64_t ballot = 0;
                        for (int lane = 0; lane < 64; ++lane) {
                            bool pass = live[lane];
                            for (int32_t c = s_off[p]; c < s_off[p + 1]; ++c)
                                pass = pass && clause_passes(v[(size_t)lane * n_cols + s_cl[c].column], s_cl[c]);
                            if (pass) ballot |= (uint64_t)1 << lane;
                        }
                        uint32_t lo = (uint32_t)ballot, hi = (uint32_t)(ballot >> 32);
                        const size_t w = (size_t)p * (size_t)W + (size_t)pair * 2;
                        if (base) {
                            lo &= base[w];
                            if (high) hi &= base[w + 1];
                        }
                        CHECK(!wseen[w], "word written twice");
                        wseen[w] = 1;
                        out[w] = lo;
                        if (high) {
                            CHECK(!wseen[w + 1], "word written twice");
                            wseen[w + 1] = 1;
                            out[w + 1] = hi;
                        } else {
                            CHECK(hi == 0, "rows past the last word passed");
                            hi = 0;
                        }
                        counts[p] += __builtin_popcount(lo) + __builtin_popcount(hi);
                    }
                }
    }
    for (int64_t r = 0; r < N; ++r) CHECK(rseen[r], "row %lld never visited", (long long)r);
    for (size_t i = 0; i < (size_t)P * (size_t)W; ++i) CHECK(wseen[i], "word %zu never written", i);

    // naive: row by row, bit by bit
    for (int32_t p = 0; p < P; ++p) {
        int64_t cnt = 0;
        for (int64_t r = 0; r < W * 32; ++r) {
            bool want = r < N;
            for (int32_t c = off[(size_t)p]; want && c < off[(size_t)p + 1]; ++c)
                want = naive_clause(cols[(size_t)cl[(size_t)c].column][(size_t)r], cl[(size_t)c].flags, cl[(size_t)c].lo,
                                    cl[(size_t)c].hi);
            if (want && base) want = (base[(size_t)p * W + (r >> 5)] >> (r & 31)) & 1u;
            const bool got = (out[(size_t)p * W + (r >> 5)] >> (r & 31)) & 1u;
            CHECK(got == want, "N %lld pred %d row %lld: got %d want %d", (long long)N, p, (long long)r, got, want);
            cnt += want;
        }
        CHECK(counts[p] == cnt, "count of pred %d: %lld, want %lld", p, (long long)counts[p], (long long)cnt);
    }
    std::free(stage);
    std::free(out);
    std::free(wseen);
    std::free(rseen);
    std::free(counts);
}

void check_validation() {
    const uint32_t attached = 0x5;  // slots 0 and 2
    int64_t at = -1;
    uint32_t used = 0;
    const FilterClause ok{0, 3, 0.0, 1.0};
    {
        const int32_t off[] = {0, 1};
        CHECK(filter_validate(&ok, off, 1, attached, &at, &used) == kFilterOk && used == 1u, "plain call");
        CHECK(filter_validate(&ok, off, -1, attached, &at, &used) == kFilterBadPreds, "n_preds < 0");
        CHECK(filter_validate(&ok, off, 257, attached, &at, &used) == kFilterBadPreds, "n_preds > 256");
        CHECK(filter_validate(nullptr, nullptr, 0, attached, &at, &used) == kFilterOk, "no predicates");
        CHECK(filter_validate(&ok, nullptr, 1, attached, &at, &used) == kFilterNullArgs, "NULL offsets");
        CHECK(filter_validate(nullptr, off, 1, attached, &at, &used) == kFilterNullArgs, "NULL clauses");
        CHECK(filter_validate(&ok, off, 1, attached, nullptr, nullptr) == kFilterOk, "optional outputs");
    }
    {
        const int32_t off[] = {1, 1};
        CHECK(filter_validate(&ok, off, 1, attached, &at, &used) == kFilterBadOffsets, "offsets start past 0");
    }
    {
        const int32_t off[] = {0, 1, 0};
        CHECK(filter_validate(&ok, off, 2, attached, &at, &used) == kFilterBadOffsets && at == 1, "offsets decrease");
    }
    {
        std::vector<FilterClause> nine(9, ok);
        const int32_t off9[] = {0, 9};
        CHECK(filter_validate(nine.data(), off9, 1, attached, &at, &used) == kFilterTooMany, "9 clauses");
        const int32_t off8[] = {0, 8};
        CHECK(filter_validate(nine.data(), off8, 1, attached, &at, &used) == kFilterOk, "8 clauses");
        const int32_t offmin[] = {0, std::numeric_limits<int32_t>::min()};
        CHECK(filter_validate(nine.data(), offmin, 1, attached, &at, &used) == kFilterBadOffsets, "offset INT_MIN");
        const int32_t offmax[] = {0, std::numeric_limits<int32_t>::max()};
        CHECK(filter_validate(nine.data(), offmax, 1, attached, &at, &used) == kFilterTooMany, "offset INT_MAX");
    }
    const int32_t off2[] = {0, 2};
    for (int which = 0; which < 7; ++which) {
        FilterClause two[2] = {ok, ok};
        int want = kFilterOk;
        switch (which) {
            case 0: two[1].column = -1, want = kFilterBadSlot; break;
            case 1: two[1].column = 16, want = kFilterBadSlot; break;
            case 2: two[1].column = 1, want = kFilterNotAttached; break;
            case 3: two[1].flags = 8, want = kFilterBadFlags; break;
            case 4: two[1].flags = -1, want = kFilterBadFlags; break;
            case 5: two[1].lo = kNan, want = kFilterNanBound; break;
            default: two[1].hi = kNan, want = kFilterNanBound; break;
        }
        CHECK(filter_validate(two, off2, 1, attached, &at, &used) == want && at == 1 && used == 0, "clause cause %d", which);
    }
    // the workgroup's LDS: parts in order, aligned, disjoint, and the largest call inside 64 KB
    for (int nc : {0, 1, 7, 2048})
        for (int np : {1, 3, 255, 256}) {
            CHECK(filter_lds_counts(nc) == (int64_t)nc * (int64_t)sizeof(FilterClause) && filter_lds_counts(nc) % 8 == 0,
                  "lds counts at %d", nc);
            CHECK(filter_lds_offsets(nc, np) == filter_lds_counts(nc) + (int64_t)np * 8, "lds offsets");
            CHECK(filter_lds_bytes(nc, np) == filter_lds_offsets(nc, np) + (int64_t)(np + 1) * 4, "lds bytes");
        }
    CHECK(filter_lds_bytes(kFilterMaxTotal, kFilterMaxPreds) == 52228 && filter_lds_bytes(kFilterMaxTotal, kFilterMaxPreds) <= 65536,
          "largest LDS");
    // the full 256 x 8 call fits the staging exactly
    CHECK(filter_stage(kFilterMaxTotal, kFilterMaxPreds).bytes == kFilterStageBytes, "largest stage");
    // vdb_index_set_column's rule
    CHECK(filter_column_ok(0, true, 5, 5) && filter_column_ok(15, true, 0, 0) && filter_column_ok(3, false, 0, 7), "column ok");
    CHECK(!filter_column_ok(-1, true, 5, 5) && !filter_column_ok(16, true, 5, 5) && !filter_column_ok(0, true, 4, 5) &&
              !filter_column_ok(0, false, 5, 5),
          "column refused");
}

}  // namespace

int main() {
    check_clause_semantics();
    check_validation();
    std::mt19937_64 rng(20250611);
    const double pool[] = {kNan, -kInf, kInf, -0.0, 0.0, 1.0, 2.0, 3.0, -7.5, 1e18};
    const int64_t sizes[] = {0, 1, 31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 255, 256, 257, 511, 513, 1000, 4099};
    int cases = 0;
    for (int64_t N : sizes)
        for (int P : {1, 3, 64, 65, 256})
            for (int n_cu : {1, 2, 256}) {
                if (N > 600 && P > 65 && n_cu != 2) continue;  // (the large ones once)
                const int n_cols = 3;
                std::vector<std::vector<double>> cols(n_cols, std::vector<double>((size_t)N));
                for (auto& c : cols)
                    for (auto& x : c) x = pool[rng() % 10];
                std::vector<FilterClause> cl;
                std::vector<int32_t> off{0};
                for (int p = 0; p < P; ++p) {
                    const int nc = p == 0 ? 0 : p == 1 ? 8 : (int)(rng() % 4);
                    for (int c = 0; c < nc; ++c) {
                        double lo = pool[1 + rng() % 9], hi = pool[1 + rng() % 9];
                        cl.push_back(FilterClause{(int32_t)(rng() % n_cols), (int32_t)(rng() % 8), lo, hi});
                    }
                    off.push_back((int32_t)cl.size());
                }
                const int64_t W = filter_n_words(N);
                uint32_t* base = exact_alloc<uint32_t>((size_t)P * (size_t)W);
                for (size_t i = 0; i < (size_t)P * (size_t)W; ++i) base[i] = (uint32_t)rng();
                run_case(N, n_cols, cols, cl, off, nullptr, n_cu);
                run_case(N, n_cols, cols, cl, off, base, n_cu);
                std::free(base);
                cases += 2;
            }
    if (g_fail) {
        std::fprintf(stderr, "filter plan check: %d failures\n", g_fail);
        return 1;
    }
    std::printf("filter plan ok: %d cases\n", cases);
    return 0;
}
