// subset_plan_check.cpp — the host arithmetic of vdb_index_search_rows (csrc/vdb_subset_plan.h)
// swept on the CPU against a naive reference.  Stand-alone: build with
// -fsanitize=address,undefined (make subset-plan-check) and run; every buffer is a heap allocation
// of exactly the size the library gives it, so a position, an offset or a scratch extent that is
// off by one is an out-of-bounds access the sanitizer reports, and a row visited twice, never, or
// with the wrong eligibility is a mismatch reported here.
//
// The model follows the kernel (csrc/vdb_subset.hip) step by step: the query's list from
// query_list and the clamped offsets, the live segments, each segment's chunks, each wave's 16
// positions with the one id load that brings the ids and their predecessors (lane i holds
// position w0 - 1 + i), the batches of kSubsetNB rows and the eligibility of every id.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../csrc/vdb_subset_plan.h"

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

// One call: what the kernel's grid (n_seg, n_queries) visits, against the naive reading of the
// arguments.  Returns the ids the model skipped as ineligible.
int64_t run_case(const std::vector<int64_t>& offs_v, const std::vector<int64_t>& rows_v, const std::vector<int32_t>* ql_v,
                 int n_queries, int64_t count, int n_seg, bool well_formed) {
    const int n_lists = (int)offs_v.size() - 1;
    const int64_t n_ids = (int64_t)rows_v.size();
    int64_t* offs = exact_alloc<int64_t>(offs_v.size());
    int64_t* rows = exact_alloc<int64_t>(rows_v.size());
    int32_t* ql = ql_v ? exact_alloc<int32_t>(ql_v->size()) : nullptr;
    std::memcpy(offs, offs_v.data(), offs_v.size() * sizeof(int64_t));
    if (n_ids) std::memcpy(rows, rows_v.data(), rows_v.size() * sizeof(int64_t));
    if (ql && !ql_v->empty()) std::memcpy(ql, ql_v->data(), ql_v->size() * sizeof(int32_t));
    int64_t where = -1;
    const int verdict = subset_validate(offs, n_lists, rows, n_ids, ql, n_queries, count, &where);
    CHECK((verdict == kSubsetOk) == well_formed, "validate gave %d at %lld, well formed %d", verdict, (long long)where,
          (int)well_formed);
    int64_t bad_total = 0;
    for (int b = 0; b < n_queries; ++b) {
        // the naive reading: the list's range clamped, ids taken in order, eligible by the rule
        const int64_t l = ql ? (int64_t)ql[b] : (int64_t)b;
        std::vector<int64_t> want;  // eligible ids in list order
        int64_t want_bad = 0, len = 0, o0 = 0;
        if (l >= 0 && l < n_lists) {
            int64_t lo = std::min<int64_t>(std::max<int64_t>(offs[l], 0), n_ids);
            int64_t hi = std::min<int64_t>(std::max<int64_t>(offs[l + 1], lo), n_ids);
            o0 = lo;
            len = hi - lo;
            for (int64_t p = lo; p < hi; ++p) {
                const int64_t prev = p > lo ? rows[p - 1] : -1;
                if (rows[p] >= 0 && rows[p] < count && rows[p] > prev) want.push_back(rows[p]);
                else ++want_bad;
            }
        }
        if (well_formed) CHECK(want_bad == 0, "query %d: a valid list lost %lld ids", b, (long long)want_bad);
        // the kernel's walk
        SubsetRange rg{0, 0};
        if (l >= 0 && l < n_lists) rg = subset_range(offs[l], offs[l + 1], n_ids);
        CHECK(rg.o0 >= 0 && rg.o0 <= rg.o1 && rg.o1 <= n_ids, "range [%lld, %lld) of %lld", (long long)rg.o0,
              (long long)rg.o1, (long long)n_ids);
        CHECK(rg.o1 - rg.o0 == len && (len == 0 || rg.o0 == o0), "query %d: range length %lld want %lld", b,
              (long long)(rg.o1 - rg.o0), (long long)len);
        const int64_t klen = rg.o1 - rg.o0;
        const int live = subset_live_segs(klen, n_seg);
        CHECK(live >= 0 && live <= n_seg && (live == 0) == (klen == 0), "live %d of %d, len %lld", live, n_seg,
              (long long)klen);
        char* seen = exact_alloc<char>((size_t)klen);
        if (klen) std::memset(seen, 0, (size_t)klen);
        std::vector<int64_t> got;
        int64_t got_bad = 0;
        const int64_t* ids = rows + rg.o0;
        const int64_t n_chunks = subset_n_chunks(klen);
        for (int s = 0; s < n_seg; ++s) {
            int64_t visited = 0;
            for (int64_t c = s; c < n_chunks; c += n_seg)
                for (int wv = 0; wv < kSubsetWaves; ++wv) {
                    const int64_t w0 = c * kSubsetChunk + (int64_t)wv * kSubsetWaveRows;
                    const int64_t w1 = std::min<int64_t>(w0 + kSubsetWaveRows, klen);
                    if (w0 >= w1) continue;
                    int64_t idv[64];
                    for (int lane = 0; lane < 64; ++lane) {
                        const int64_t pp = w0 - 1 + lane;
                        idv[lane] = (lane <= kSubsetWaveRows && pp >= 0 && pp < w1) ? ids[pp] : -1;
                    }
                    for (int t = 0; t < kSubsetWaveRows / kSubsetNB; ++t) {
                        const int64_t j0 = w0 + t * kSubsetNB;
                        if (j0 >= w1) break;
                        const int nb = (int)std::min<int64_t>(w1 - j0, kSubsetNB);
                        for (int u = 0; u < nb; ++u) {
                            const int64_t id = idv[1 + t * kSubsetNB + u], prev = idv[t * kSubsetNB + u];
                            const int64_t p = j0 + u;
                            CHECK(p >= 0 && p < klen, "position %lld of %lld", (long long)p, (long long)klen);
                            CHECK(!seen[p], "query %d: position %lld visited twice (n_seg %d)", b, (long long)p, n_seg);
                            seen[p] = 1;
                            ++visited;
                            if (subset_id_ok(id, prev, count)) {
                                CHECK(id >= 0 && id < count, "row %lld of %lld", (long long)id, (long long)count);
                                got.push_back(id);
                            } else {
                                ++got_bad;
                            }
                        }
                    }
                }
            CHECK((visited > 0) == (s < live), "query %d: segment %d of %d visited %lld, live %d", b, s, n_seg,
                  (long long)visited, live);
        }
        for (int64_t p = 0; p < klen; ++p) CHECK(seen[p], "query %d: position %lld never visited", b, (long long)p);
        std::free(seen);
        std::vector<int64_t> a = want, g = got;
        std::sort(a.begin(), a.end());
        std::sort(g.begin(), g.end());
        CHECK(a == g, "query %d: %zu eligible ids, want %zu (n_seg %d)", b, g.size(), a.size(), n_seg);
        CHECK(got_bad == want_bad, "query %d: %lld skipped, want %lld", b, (long long)got_bad, (long long)want_bad);
        bad_total += got_bad;
    }
    std::free(offs);
    std::free(rows);
    std::free(ql);
    return bad_total;
}

// The scratch layout: every region inside the total, aligned, and none overlapping the next.
void check_scratch(int B, int dim, int k, int n_seg, int n_lists, int64_t n_ids, bool host, bool has_ql, bool keys) {
    const SubsetScratch s = subset_scratch(B, dim, k, n_seg, n_lists, n_ids, host, has_ql, keys);
    const int64_t KE = subset_ke(k);
    CHECK(KE >= 32 && KE >= k && (KE & (KE - 1)) == 0 && (KE == 32 || KE / 2 < k), "KE %lld for k %d", (long long)KE, k);
    struct Reg { int64_t at, bytes; };
    std::vector<Reg> regs = {{s.qn64, (int64_t)B * 8}, {s.done, (int64_t)B * 4}};
    if (n_seg > 1) {
        regs.push_back({s.lk, (int64_t)B * n_seg * KE * 8});
        regs.push_back({s.li, (int64_t)B * n_seg * KE * 4});
        regs.push_back({s.mk, (int64_t)B * KE * 8});
        regs.push_back({s.mi, (int64_t)B * KE * 4});
    }
    if (host) {
        regs.push_back({s.q, (int64_t)B * dim * 4});
        regs.push_back({s.offs, ((int64_t)n_lists + 1) * 8});
        regs.push_back({s.rows, n_ids * 8});
        if (has_ql) regs.push_back({s.qlist, (int64_t)B * 4});
        regs.push_back({s.out_s, (int64_t)B * k * 4});
        regs.push_back({s.out_i, (int64_t)B * k * 8});
        if (keys) regs.push_back({s.out_k, (int64_t)B * k * 8});
        CHECK(s.q == s.in0 && s.in0 + s.in_bytes == s.out0 && s.out_s == s.out0 && s.out0 + s.out_bytes == s.total,
              "staged blocks");
    }
    char* mem = exact_alloc<char>((size_t)s.total);  // touch every region: past the total is a sanitizer report
    int64_t end = 0;
    for (const Reg& r : regs) {
        CHECK(r.at % 256 == 0 && r.at >= end && r.at + r.bytes <= s.total, "region at %lld + %lld (previous end %lld, total %lld)",
              (long long)r.at, (long long)r.bytes, (long long)end, (long long)s.total);
        if (r.bytes) std::memset(mem + r.at, 1, (size_t)r.bytes);
        end = r.at + r.bytes;
    }
    std::free(mem);
}

}  // namespace

int main() {
    std::mt19937_64 rng(4321);
    const int64_t count = 5000;
    const int C = kSubsetChunk;
    const int64_t lens[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, C - 1, C, C + 1, 2 * C - 1, 2 * C, 2 * C + 1, 7 * C + 5, 1000, 4999, 5000};
    const int segs[] = {1, 2, 3, 7, 64, 512};
    int64_t cases = 0;
    auto ascending = [&](int64_t len) {  // len distinct rows of [0, count), ascending
        std::vector<int64_t> all((size_t)count);
        for (int64_t i = 0; i < count; ++i) all[(size_t)i] = i;
        std::shuffle(all.begin(), all.end(), rng);
        all.resize((size_t)len);
        std::sort(all.begin(), all.end());
        return all;
    };
    // one list per length, alone and all together, identity map and query_list forms
    for (int64_t len : lens)
        for (int n_seg : segs) {
            std::vector<int64_t> rows = ascending(len);
            CHECK(run_case({0, len}, rows, nullptr, 1, count, n_seg, true) == 0, "bad ids in a valid list");
            ++cases;
        }
    {
        std::vector<int64_t> offs = {0}, rows;
        for (int64_t len : lens) {
            const std::vector<int64_t> r = ascending(len);
            rows.insert(rows.end(), r.begin(), r.end());
            offs.push_back((int64_t)rows.size());
        }
        const int n_lists = (int)offs.size() - 1;
        for (int n_seg : segs) {
            CHECK(run_case(offs, rows, nullptr, n_lists, count, n_seg, true) == 0, "identity map");
            std::vector<int32_t> ql;  // shared lists, a permutation, an unused list
            for (int b = 0; b < 3 * n_lists; ++b) ql.push_back((int32_t)((b * 7 + 3) % (n_lists - 1)));
            CHECK(run_case(offs, rows, &ql, (int)ql.size(), count, n_seg, true) == 0, "query_list");
            cases += 2;
        }
        // rows 0 and count - 1, the last row alone, every row
        std::vector<int64_t> every((size_t)count);
        for (int64_t i = 0; i < count; ++i) every[(size_t)i] = i;
        for (int n_seg : segs) {
            run_case({0, 2}, {0, count - 1}, nullptr, 1, count, n_seg, true);
            run_case({0, 1}, {count - 1}, nullptr, 1, count, n_seg, true);
            run_case({0, count}, every, nullptr, 1, count, n_seg, true);
            run_case({0, 0, 0}, {}, nullptr, 2, count, n_seg, true);  // no ids at all
            cases += 4;
        }
        // malformed: what a device-memory call may hold; the walk stays in bounds and skips by the rule
        for (int n_seg : segs) {
            std::vector<int64_t> r = ascending(3 * C + 7);
            std::vector<int64_t> badid = r;
            badid[5] = -1;                       // negative
            badid[C] = badid[C - 1];             // repeated
            badid.push_back(count);              // >= count, last
            CHECK(run_case({0, (int64_t)badid.size()}, badid, nullptr, 1, count, n_seg, false) == 3, "three bad ids");
            std::vector<int64_t> unsorted = r;
            std::swap(unsorted[10], unsorted[11]);
            CHECK(run_case({0, (int64_t)unsorted.size()}, unsorted, nullptr, 1, count, n_seg, false) == 1, "one descent");
            run_case({0, (int64_t)r.size() + 9}, r, nullptr, 1, count, n_seg, false);        // offset past n_ids
            run_case({5, 2, (int64_t)r.size()}, r, nullptr, 2, count, n_seg, false);         // offsets descend
            run_case({-4, 10}, r, nullptr, 1, count, n_seg, false);                          // negative offset
            std::vector<int32_t> ql = {0, 1, -1, 0};
            run_case({0, 10}, r, &ql, 4, count, n_seg, false);                               // query_list out of range
            run_case({0, 10}, r, nullptr, 2, count, n_seg, false);                           // n_lists != n_queries
            std::vector<int64_t> junk((size_t)(2 * C + 3));
            for (auto& v : junk) v = (int64_t)(rng() % 20000) - 10000;                       // anything at all
            run_case({0, (int64_t)junk.size()}, junk, nullptr, 1, count, n_seg, false);
            cases += 8;
        }
    }
    // n_seg: within [1, kSubsetMaxSeg], the knob wins, auto never exceeds the average list's chunks
    for (int64_t knob : {0, 1, 2, 7, 512, 100000})
        for (int64_t n_ids : {0ll, 1ll, 63ll, 64ll, 65ll, 1000ll, 250000ll, 1ll << 33})
            for (int B : {1, 4, 64, 65, 4096})
                for (int n_lists : {1, 2, 64, 4096})
                    for (int n_cu : {1, 64, 256}) {
                        const int n = subset_n_seg(knob, n_ids, B, n_lists, n_cu);
                        CHECK(n >= 1 && n <= kSubsetMaxSeg, "n_seg %d", n);
                        if (knob > 0) CHECK(n == std::min<int64_t>(knob, kSubsetMaxSeg), "knob %lld gave %d", (long long)knob, n);
                        else {
                            const int64_t avg = n_ids / std::max(1, std::min(B, n_lists));
                            CHECK(n == 1 || (int64_t)(n - 1) * kSubsetChunk < avg, "auto n_seg %d for an average of %lld ids", n, (long long)avg);
                            CHECK(n == 1 || (int64_t)n * B <= (int64_t)n_cu * kSubsetWgPerCu, "auto n_seg %d x %d queries on %d CUs", n, B, n_cu);
                        }
                        ++cases;
                    }
    for (int B : {1, 4, 65})
        for (int k : {1, 10, 32, 33, 200, 201, 1024})
            for (int n_seg : {1, 2, 7})
                for (int64_t n_ids : {0ll, 1ll, 1000ll})
                    for (int flags = 0; flags < 8; ++flags) {
                        check_scratch(B, 100, k, n_seg, B, n_ids, flags & 1, flags & 2, flags & 4);
                        ++cases;
                    }
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("subset plan ok: %lld cases\n", (long long)cases);
    return 0;
}
