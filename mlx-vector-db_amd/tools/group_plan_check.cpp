// group_plan_check.cpp — the host arithmetic of vdb_index_search_groups (csrc/vdb_group_plan.h) swept
// on the CPU against naive loops: the fetch rule, the first-occurrence / complete decision the select
// kernel shares (the whole "select" step replayed against a brute-force grouped ranking), the deal of
// rows to the exact fallback's segments, the GroupTopK buffer size, the scratch layout and the
// validation.  A stand-alone host program (its own main, no GPU, nothing loaded into another
// process); `make group-plan-check` builds it with -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../csrc/vdb_group_plan.h"

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

static void check_fetch() {
    for (int k = 1; k <= kGroupMaxK; ++k)
        for (int64_t knob = 0; knob <= kGroupMaxFetch; ++knob) {
            const int f = group_fetch_k(knob, k);
            int64_t want = knob > 0 ? knob : (k == 1 ? 1 : 200);
            want = std::max<int64_t>(std::min<int64_t>(want, kGroupMaxFetch), k);
            CHECK(f == want, "fetch %d, want %lld (knob %lld, k %d)", f, (long long)want, (long long)knob, k);
            CHECK(f >= k && f <= kGroupMaxFetch, "fetch %d outside [k, %d]", f, kGroupMaxFetch);
        }
}

// The select step on the host: rows ranked best first (position = rank), `elig` of them eligible
// in all, the best k_fetch fetched.  Returns whether the list settles the query; when it does the
// slots must equal the naive grouped ranking over ALL eligible rows.
static void check_select(std::mt19937& rng) {
    for (int trial = 0; trial < 4000; ++trial) {
        const int k = 1 + (int)(rng() % 12);
        const int kf = group_fetch_k(rng() % 3 == 0 ? 0 : 1 + rng() % 40, k);
        const int elig = (int)(rng() % (3 * kf + 2));
        const int n_groups = 1 + (int)(rng() % (trial % 2 ? 4 : 40));
        std::vector<int32_t> all(elig);  // group of the eligible row at each rank
        for (auto& g : all) g = (int32_t)(rng() % n_groups) * (trial % 7 == 0 ? 53687091 : 1);
        // the fetched list, padded with "no row" (-1) as the search pads it
        std::vector<int32_t> g(kf, -1);
        const int n_valid = std::min(elig, kf);
        for (int j = 0; j < n_valid; ++j) g[j] = all[j];
        std::vector<int> firsts;
        for (int j = 0; j < kf; ++j) {
            bool naive = g[j] >= 0;
            for (int i = 0; i < j && naive; ++i) naive = g[i] != g[j];
            CHECK(group_first_occurrence(g.data(), j) == naive, "first occurrence at %d", j);
            if (naive) firsts.push_back(j);
        }
        const bool complete = group_complete((int)firsts.size(), n_valid, k, kf, elig);
        // the naive answer over every eligible row
        std::vector<int> want;
        std::map<int32_t, bool> seen;
        for (int j = 0; j < elig && (int)want.size() < k; ++j)
            if (!seen[all[j]]) {
                seen[all[j]] = true;
                want.push_back(j);
            }
        // the flagged set as the tests state it: fewer than k groups in the best kf, and more than kf eligible
        const bool flagged = (int)firsts.size() < k && elig > kf;
        CHECK(complete == !flagged, "complete %d, flagged %d (k %d, kf %d, eligible %d)", (int)complete, (int)flagged, k, kf, elig);
        if (complete) {
            const size_t n = std::min<size_t>(firsts.size(), (size_t)k);
            CHECK(n == want.size(), "%zu groups from the list, %zu naive", n, want.size());
            for (size_t e = 0; e < n; ++e) CHECK(firsts[e] == want[e], "slot %zu: rank %d, want %d", e, firsts[e], want[e]);
        }
    }
}

static void check_segments() {
    const int64_t rows_list[] = {1, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 4097, 70000, 1000000, 4294967294ll};
    for (int64_t N : rows_list)
        for (int B : {1, 2, 64, 130, 4096})
            for (int k : {1, 5, 128}) {
                const int n_seg = group_n_seg(N, B, k);
                CHECK(n_seg >= 1 && n_seg <= kGroupMaxSeg, "n_seg %d", n_seg);
                CHECK(n_seg == 1 || (int64_t)B * n_seg * k * kGroupEntryBytes <= kGroupListBytes, "lists of %d x %d x %d over the bound", B, n_seg, k);
                const int64_t per = group_seg_rows(N, n_seg);
                CHECK(per % kGroupSegAlign == 0 && per * n_seg >= N, "segment rows %lld", (long long)per);
                const int live = group_live_segs(N, n_seg);
                CHECK(live >= 1 && live <= n_seg, "live %d of %d", live, n_seg);
                int64_t next = 0;
                int with_rows = 0;
                for (int s = 0; s < n_seg; ++s) {
                    const GroupRange r = group_seg_range(N, n_seg, s);
                    CHECK(r.r0 <= r.r1 && r.r1 <= N, "range [%lld, %lld) of %lld", (long long)r.r0, (long long)r.r1, (long long)N);
                    CHECK(r.r0 == next || r.r0 == r.r1, "segment %d starts at %lld, the rows so far end at %lld", s, (long long)r.r0, (long long)next);
                    CHECK(r.r0 % kGroupSegAlign == 0 || r.r0 == r.r1, "segment %d starts inside a mask word", s);
                    if (r.r1 > r.r0) {
                        CHECK(s == with_rows, "a segment with rows after an empty one");
                        ++with_rows;
                        next = r.r1;
                        // a wave's trips: rows base .. base + NB of one mask word, every row once
                        if (N <= 4097) {
                            int64_t covered = 0;
                            for (int wv = 0; wv < kGroupWaves; ++wv)
                                for (int64_t base = r.r0 + wv * kGroupNB; base < r.r1; base += kGroupWaves * kGroupNB) {
                                    CHECK((base & 31) + kGroupNB <= 32, "a trip crosses a mask word at %lld", (long long)base);
                                    covered += std::min<int64_t>(kGroupNB, r.r1 - base);
                                }
                            CHECK(covered == r.r1 - r.r0, "trips cover %lld of %lld rows", (long long)covered, (long long)(r.r1 - r.r0));
                        }
                    }
                }
                CHECK(next == N, "segments end at %lld of %lld", (long long)next, (long long)N);
                CHECK(with_rows == live, "%d segments hold rows, live says %d", with_rows, live);
            }
    for (int k = 1; k <= kGroupMaxK; ++k) {
        const int cap = group_topk_cap(k);
        CHECK((cap & (cap - 1)) == 0 && cap >= 2 * k && cap >= k + 64 && cap <= 256, "cap %d for k %d", cap, k);
    }
}

static void check_scratch() {
    for (int B : {1, 3, 64, 130})
        for (int dim : {1, 33, 768, 2100})
            for (int k : {1, 5, 128})
                for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)33, (int64_t)4097, (int64_t)70000})
                    for (int flags = 0; flags < 8; ++flags) {
                        const bool host = flags & 1, masked = (flags & 2) && N > 0, keys = flags & 4;
                        const int kf = group_fetch_k(0, k);
                        const int n_seg = N > 0 ? group_n_seg(N, B, k) : 1;
                        const GroupScratch s = group_scratch(B, dim, k, kf, n_seg, N, host, masked, keys);
                        CHECK(s.mask_words * 32 >= N && (s.mask_words == 0 || (s.mask_words - 1) * 32 < N), "mask words");
                        struct Region { int64_t at, bytes; };
                        std::vector<Region> rs = {
                            {s.qn64, (int64_t)B * 8}, {s.done, (int64_t)B * 4}, {s.need, (int64_t)B * 4}, {s.elig, 8},
                            {s.fmask, masked ? (s.mask_words + 64) * 4 : 0},
                            {s.fs, (int64_t)B * kf * 4}, {s.fi, (int64_t)B * kf * 8}, {s.fk, (int64_t)B * kf * 8},
                            {s.lk, n_seg > 1 ? (int64_t)B * n_seg * k * 8 : 0}, {s.lr, n_seg > 1 ? (int64_t)B * n_seg * k * 4 : 0},
                            {s.lg, n_seg > 1 ? (int64_t)B * n_seg * k * 4 : 0}};
                        if (host) {
                            rs.push_back({s.q, (int64_t)B * dim * 4});
                            rs.push_back({s.mask, masked ? s.mask_words * 4 : 0});
                            rs.push_back({s.out_s, (int64_t)B * k * 4});
                            rs.push_back({s.out_i, (int64_t)B * k * 8});
                            rs.push_back({s.out_g, (int64_t)B * k * 4});
                            rs.push_back({s.out_k, keys ? (int64_t)B * k * 8 : 0});
                            CHECK(s.q == s.in0 && s.in0 + s.in_bytes == s.out0 && s.out_s == s.out0 && s.out0 + s.out_bytes == s.total,
                                  "staged regions are not two contiguous runs");
                        } else {
                            CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device-memory call stages nothing");
                        }
                        int64_t end = 0;
                        for (const Region& r : rs) {
                            CHECK(r.at % 256 == 0 && r.at >= end && r.at + r.bytes <= s.total, "region at %lld + %lld (previous end %lld, total %lld)",
                                  (long long)r.at, (long long)r.bytes, (long long)end, (long long)s.total);
                            end = r.at + r.bytes;
                        }
                    }
}

static void check_validate() {
    CHECK(group_validate(-1, 5, true, true, true, true, 0, true, 10, 10) == kGroupBadQueries, "negative queries");
    CHECK(group_validate(kGroupMaxQueries + 1, 5, true, true, true, true, 0, true, 10, 10) == kGroupBadQueries, "too many queries");
    CHECK(group_validate(kGroupMaxQueries, 5, true, true, true, true, 0, true, 10, 10) == kGroupOk, "the most queries");
    CHECK(group_validate(1, 0, true, true, true, true, 0, true, 10, 10) == kGroupBadK, "k = 0");
    CHECK(group_validate(1, kGroupMaxK + 1, true, true, true, true, 0, true, 10, 10) == kGroupBadK, "k = 129");
    CHECK(group_validate(1, kGroupMaxK, true, true, true, true, 0, true, 10, 10) == kGroupOk, "k = 128");
    for (int miss = 0; miss < 4; ++miss)
        CHECK(group_validate(1, 1, miss != 0, miss != 1, miss != 2, miss != 3, 1, true, 10, 10) == kGroupNullPointer, "NULL pointer %d", miss);
    CHECK(group_validate(1, 1, true, true, true, true, 2, true, 10, 10) == kGroupBadMem, "mem kind");
    CHECK(group_validate(1, 1, true, true, true, true, 1, false, 10, 10) == kGroupNoColumn, "no column");
    CHECK(group_validate(1, 1, true, true, true, true, 1, true, 9, 10) == kGroupNoColumn, "a stale column");
    CHECK(group_validate(1, 1, true, true, true, true, 1, true, 0, 0) == kGroupOk, "an empty index with its empty column");
    CHECK(group_set_ok(false, 0, 10) && !group_set_ok(false, 1, 10), "detach");
    CHECK(group_set_ok(true, 10, 10) && !group_set_ok(true, 9, 10) && !group_set_ok(true, 11, 10) && group_set_ok(true, 0, 0), "attach");
}

int main() {
    std::mt19937 rng(20261020u);
    check_fetch();
    check_select(rng);
    check_segments();
    check_scratch();
    check_validate();
    std::printf("group plan ok: %ld checks\n", g_checks);
    return 0;
}
