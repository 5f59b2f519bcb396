// range_plan_check.cpp — the host arithmetic of vdb_index_search_range (csrc/vdb_range_plan.h)
// swept on the CPU against naive loops.  Stand-alone: build with -fsanitize=address,undefined
// (make range-plan-check) and run; every buffer is a heap allocation of exactly the size the
// library gives it, so a word, a slot or a scratch extent that is off by one is an out-of-bounds
// access the sanitizer reports, and a row visited twice, never, or written to the wrong slot is a
// mismatch reported here.
//
// The model follows the kernels (csrc/vdb_range.hip) step by step: the scan's deal of bitmap words
// to workgroups and waves with the rows of each 4-row trip, the per-chunk counts, the prefix, the
// emit's early return and slot positions, and the score kernel's split of [0, cap) into filled
// and "no result" slots.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/vdb_range_plan.h"

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

int popc(uint32_t v) { return __builtin_popcount(v); }

// One query of one block: `pass` says which rows pass (before the mask).  Runs the four kernels'
// index arithmetic and compares with the naive list of eligible passing rows.
void run_case(int64_t N, const std::vector<char>& pass, const uint32_t* mask, int64_t cap, int64_t index_offset) {
    const int64_t n_words = range_n_words(N);
    const int64_t n_chunks = range_n_chunks(n_words);
    CHECK(n_words * 32 >= N && (n_words - 1) * 32 < N, "n_words %lld for %lld rows", (long long)n_words, (long long)N);
    CHECK(n_chunks * kRangeWgWords >= n_words && (n_chunks - 1) * kRangeWgWords < n_words, "n_chunks %lld",
          (long long)n_chunks);
    // naive
    std::vector<int64_t> want;
    for (int64_t r = 0; r < N; ++r)
        if (pass[(size_t)r] && (!mask || ((mask[r >> 5] >> (r & 31)) & 1u))) want.push_back(r);
    const int64_t count = (int64_t)want.size();

    uint32_t* H = exact_alloc<uint32_t>((size_t)n_words);
    uint32_t* part = exact_alloc<uint32_t>((size_t)n_chunks);
    char* seen = exact_alloc<char>((size_t)N);
    std::memset(seen, 0, (size_t)N);
    char* wseen = exact_alloc<char>((size_t)n_words);
    std::memset(wseen, 0, (size_t)n_words);
    // scan: grid n_chunks, 4 waves, kRangeWaveWords words per wave, 32 / kRangeNB trips per word
    for (int64_t chunk = 0; chunk < n_chunks; ++chunk) {
        uint32_t total = 0;
        for (int wv = 0; wv < kRangeWaves; ++wv)
            for (int i = 0; i < kRangeWaveWords; ++i) {
                const int64_t w = range_wave_word(chunk, wv, i);
                if (w >= n_words) break;
                CHECK(w >= 0 && !wseen[w], "word %lld visited twice", (long long)w);
                wseen[w] = 1;
                const uint32_t elig = range_valid_bits(w, N) & (mask ? mask[w] : 0xFFFFFFFFu);
                uint32_t word = 0;
                for (int t = 0; t < 32 / kRangeNB; ++t) {
                    const uint32_t e = (elig >> (t * kRangeNB)) & ((1u << kRangeNB) - 1u);
                    if (e == 0) continue;
                    uint32_t bits = 0;
                    for (int u = 0; u < kRangeNB; ++u) {
                        if (!((e >> u) & 1u)) continue;
                        const int64_t r = w * 32 + t * kRangeNB + u;
                        CHECK(r >= 0 && r < N, "row %lld of %lld", (long long)r, (long long)N);
                        CHECK(!seen[r], "row %lld scored twice", (long long)r);
                        seen[r] = 1;
                        if (pass[(size_t)r]) bits |= 1u << u;
                    }
                    word |= bits << (t * kRangeNB);
                }
                H[w] = word;
                total += (uint32_t)popc(word);
            }
        part[chunk] = total;
    }
    for (int64_t w = 0; w < n_words; ++w) CHECK(wseen[w], "word %lld never visited", (long long)w);
    for (int64_t r = 0; r < N; ++r) {
        const bool elig = !mask || ((mask[r >> 5] >> (r & 31)) & 1u);
        CHECK((bool)seen[r] == elig, "row %lld: scored %d, eligible %d", (long long)r, (int)seen[r], (int)elig);
    }
    // prefix: exclusive, in place
    uint32_t carry = 0;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const uint32_t v = part[c];
        part[c] = carry;
        carry += v;
    }
    CHECK((int64_t)carry == count, "count %lld, want %lld", (long long)carry, (long long)count);
    // emit: grid range_emit_wgs, one thread per word; then score: filled and "no result" slots
    const int64_t filled = range_filled(count, cap);
    CHECK(filled >= 0 && filled <= cap && filled <= count && (filled == cap || filled == count), "filled %lld",
          (long long)filled);
    int64_t* out = exact_alloc<int64_t>((size_t)cap);
    char* written = exact_alloc<char>((size_t)cap);
    if (cap) std::memset(written, 0, (size_t)cap);
    int64_t emit_words = 0;
    if (cap > 0) {
        const int64_t wgs = range_emit_wgs(n_words);
        CHECK(wgs * kRangeEmitWords >= n_words && (wgs - 1) * kRangeEmitWords < n_words, "emit wgs %lld", (long long)wgs);
        for (int64_t g = 0; g < wgs; ++g) {
            const int64_t w0 = g * kRangeEmitWords;
            CHECK(w0 / kRangeWgWords < n_chunks, "emit workgroup %lld reads part[%lld] of %lld", (long long)g,
                  (long long)(w0 / kRangeWgWords), (long long)n_chunks);
            if (!range_emit_live((int64_t)part[w0 / kRangeWgWords], cap)) continue;
            for (int t = 0; t < kRangeEmitWords; ++t) {
                const int64_t w = w0 + t;
                if (w >= n_words) continue;
                ++emit_words;
                // the 16-lane scan: the popcounts of the chunk's words below w
                uint32_t below = 0;
                for (int64_t x = w - (w % kRangeWgWords); x < w; ++x) below += (uint32_t)popc(H[x]);
                int64_t p = (int64_t)part[w / kRangeWgWords] + below;
                uint32_t word = H[w];
                while (word && p < cap) {
                    const int bit = __builtin_ctz(word);
                    CHECK(p >= 0 && p < cap && !written[p], "slot %lld of %lld written twice", (long long)p, (long long)cap);
                    out[p] = w * 32 + bit + index_offset;
                    written[p] = 1;
                    ++p;
                    word &= word - 1u;
                }
            }
        }
        const int sg = range_score_wgs(cap);
        CHECK(sg >= 1 && sg <= kRangeScoreWgs, "score workgroups %d", sg);
        // the score kernel's two strided loops cover [0, filled) and [filled, cap) once each
        const int64_t n_waves = (int64_t)sg * kRangeWaves, n_thr = (int64_t)sg * 256;
        std::vector<char> cov((size_t)cap, 0);
        for (int64_t wid = 0; wid < n_waves; ++wid)
            for (int64_t p = wid; p < filled; p += n_waves) {
                CHECK(written[p] && !cov[(size_t)p], "slot %lld scored without an id or twice", (long long)p);
                cov[(size_t)p] = 1;
            }
        for (int64_t tid = 0; tid < n_thr; ++tid)
            for (int64_t p = filled + tid; p < cap; p += n_thr) {
                CHECK(!written[p] && !cov[(size_t)p], "slot %lld filled over an id or twice", (long long)p);
                cov[(size_t)p] = 1;
            }
        for (int64_t p = 0; p < cap; ++p) CHECK(cov[(size_t)p], "slot %lld left unwritten", (long long)p);
        for (int64_t p = 0; p < filled; ++p)
            CHECK(out[p] == want[(size_t)p] + index_offset, "slot %lld holds %lld, want %lld", (long long)p,
                  (long long)out[p], (long long)(want[(size_t)p] + index_offset));
        // work proportional to min(count, cap): the words the emit reads end with the workgroup
        // that holds the cap-th hit
        if (filled < count) {
            const int64_t last_w = want[(size_t)filled] / 32;  // the first hit that is not written
            CHECK(emit_words <= (last_w / kRangeEmitWords + 1) * kRangeEmitWords, "emit read %lld words for %lld slots",
                  (long long)emit_words, (long long)cap);
        }
    }
    std::free(H);
    std::free(part);
    std::free(seen);
    std::free(wseen);
    std::free(out);
    std::free(written);
}

// The scratch layout: every region inside the total, aligned, and none overlapping the next.
void check_scratch(int B, int dim, int Dp, int64_t N, int64_t cap, bool host, bool has_mask, bool keys) {
    const RangeScratch s = range_scratch(B, dim, Dp, N, cap, host, has_mask, keys);
    CHECK(s.block >= 1 && s.block <= kRangeMaxBlock && s.block <= std::max(B, 1), "block %d for %d queries", s.block, B);
    CHECK(s.n_words == range_n_words(N) && s.n_chunks == range_n_chunks(s.n_words), "words / chunks");
    struct Reg { int64_t at, bytes; };
    std::vector<Reg> regs = {{s.qn64, (int64_t)B * 8},
                             {s.H, (int64_t)s.block * s.n_words * 4},
                             {s.part, (int64_t)s.block * s.n_chunks * 4},
                             {s.cnt, (int64_t)s.block * 8}};
    if (host) {
        regs.push_back({s.q, (int64_t)B * dim * 4});
        regs.push_back({s.thr, (int64_t)B * 8});
        if (has_mask) regs.push_back({s.mask, s.n_words * 4});
        regs.push_back({s.out_c, (int64_t)B * 8});
        regs.push_back({s.out_i, (int64_t)B * cap * 8});
        regs.push_back({s.out_s, (int64_t)B * cap * 4});
        if (keys) regs.push_back({s.out_k, (int64_t)B * cap * 8});
        CHECK(s.q == s.in0 && s.in0 + s.in_bytes == s.out0 && s.out_c == s.out0 && s.out0 + s.out_bytes == s.total,
              "staged blocks");
    } else {
        CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device-memory call stages nothing");
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
    std::mt19937_64 rng(97531);
    int64_t cases = 0;
    const int R = kRangeWgRows, E = kRangeEmitWords * 32;
    const int64_t Ns[] = {1, 2, 31, 32, 33, 63, 64, 65, R - 1, R, R + 1, 2 * R + 5, E - 1, E, E + 1, 3 * E + 77};
    for (int64_t N : Ns) {
        const int64_t n_words = range_n_words(N);
        // hit patterns: none, all, first word, last word, one per word, random at three densities
        std::vector<std::vector<char>> pats;
        pats.emplace_back((size_t)N, 0);
        pats.emplace_back((size_t)N, 1);
        {
            std::vector<char> p((size_t)N, 0);
            for (int64_t r = 0; r < std::min<int64_t>(N, 32); ++r) p[(size_t)r] = 1;
            pats.push_back(p);
            std::fill(p.begin(), p.end(), 0);
            for (int64_t r = (n_words - 1) * 32; r < N; ++r) p[(size_t)r] = 1;
            pats.push_back(p);
            std::fill(p.begin(), p.end(), 0);
            for (int64_t w = 0; w < n_words; ++w) {
                const int64_t r = std::min<int64_t>(w * 32 + (int64_t)(rng() % 32), N - 1);
                p[(size_t)r] = 1;
            }
            pats.push_back(p);
            for (double dens : {0.01, 0.3, 0.9}) {
                for (auto& v : p) v = (rng() % 1000) < dens * 1000;
                pats.push_back(p);
            }
        }
        // masks: none, all zero, a single bit, random (with junk in the bits at or past N)
        std::vector<std::vector<uint32_t>> masks;
        masks.emplace_back();
        masks.emplace_back((size_t)n_words, 0u);
        {
            std::vector<uint32_t> m((size_t)n_words, 0u);
            const int64_t r = (int64_t)(rng() % (uint64_t)N);
            m[(size_t)(r >> 5)] |= 1u << (r & 31);
            masks.push_back(m);
            for (auto& v : m) v = (uint32_t)rng();
            masks.push_back(m);
        }
        for (const auto& p : pats) {
            int64_t hits = 0;
            for (char c : p) hits += c;
            for (size_t mi = 0; mi < masks.size(); ++mi) {
                const uint32_t* mask = mi == 0 ? nullptr : masks[mi].data();
                uint32_t* mcopy = nullptr;
                if (mask) {  // exactly n_words words
                    mcopy = exact_alloc<uint32_t>((size_t)n_words);
                    std::memcpy(mcopy, mask, (size_t)n_words * 4);
                }
                for (int64_t cap : {(int64_t)0, (int64_t)1, hits - 1, hits, hits + 1, N, N + 3}) {
                    if (cap < 0) continue;
                    run_case(N, p, mcopy, cap, mi == 1 ? 1000 : 0);
                    ++cases;
                }
                std::free(mcopy);
            }
        }
    }
    // the query block: within [1, 64], inside the byte budget unless it is one query, and maximal
    for (int Dp : {8, 40, 104, 256, 264, 512, 520, 768, 1536, 2104, 4096, 32768, 65536}) {
        const int qb = range_query_block(Dp);
        CHECK(qb >= 1 && qb <= kRangeMaxBlock, "block %d for %d dims", qb, Dp);
        CHECK(qb == 1 || (int64_t)qb * Dp * 4 <= kRangeQueryBytes, "block %d x %d dims over the budget", qb, Dp);
        CHECK(qb == kRangeMaxBlock || (int64_t)(qb + 1) * Dp * 4 > kRangeQueryBytes, "block %d for %d dims is not the largest", qb, Dp);
        ++cases;
    }
    // threshold -> key bound, against the documented formula; NaN where the call is invalid
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double t : {0.0, -0.0, 0.25, 1.0, 5.0, std::nextafter(5.0, 0.0), 1e200, -1.0, -1e-300, inf, -inf, nan}) {
        const double kc = range_kt(0, t), ke = range_kt(1, t);
        CHECK((t != t) ? (kc != kc) : (kc == t), "cosine kt of %g is %g", t, kc);
        if (t != t || t < 0.0) CHECK(ke != ke, "euclidean kt of %g is %g, want NaN", t, ke);
        else CHECK(ke == -(t * t), "euclidean kt of %g is %g", t, ke);
        double thr[3] = {0.5, t, 0.5};
        int64_t where = -1;
        const int vc = range_validate(0, thr, 3, &where), ve = range_validate(1, thr, 3, &where);
        CHECK(vc == ((t != t) ? kRangeNanThreshold : kRangeOk), "cosine validate of %g gave %d", t, vc);
        CHECK(ve == ((t != t) ? kRangeNanThreshold : t < 0.0 ? kRangeNegRadius : kRangeOk), "euclidean validate of %g gave %d", t, ve);
        CHECK(ve == kRangeOk || where == 1, "offending query %lld", (long long)where);
        // a device-memory call: the bound the kernel forms passes nothing exactly when the host refuses
        CHECK((ve != kRangeOk) == (ke != ke) && (vc != kRangeOk) == (kc != kc), "kernel and host disagree on %g", t);
        ++cases;
    }
    {
        double thr[1] = {0.5};
        CHECK(range_validate(1, thr, 0, nullptr) == kRangeOk, "no queries");
        // the cap: never negative, and n_queries * cap within kRangeMaxSlots for every batch size, so
        // that no byte count of the scratch can leave int64 (the naive product in 128 bits)
        const int64_t S = kRangeMaxSlots;
        for (int B : {0, 1, 2, 3, 64, 65, 1 << 24, (1 << 24) + 1, 2147483647})
            for (int64_t cap : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)1024, S / 65, S / 64, S / 64 + 1, S / 3, S / 2,
                                S / 2 + 1, S - 1, S, S + 1, (int64_t)1 << 40, std::numeric_limits<int64_t>::max()}) {
                const __int128 slots = (__int128)(B > 0 ? B : 1) * cap;
                const bool ok = cap >= 0 && slots <= (__int128)S;
                CHECK((range_validate_cap(B, cap) == kRangeOk) == ok, "cap %lld for %d queries", (long long)cap, B);
                if (ok && B > 0) {  // the largest byte counts range_scratch forms, without overflow
                    const RangeScratch sc = range_scratch(B, 1, 8, 1, cap, true, false, true);
                    CHECK(sc.total > 0 && sc.out_bytes >= (int64_t)(slots * 20) && sc.total < ((int64_t)1 << 45),
                          "scratch total %lld for %d x %lld slots", (long long)sc.total, B, (long long)cap);
                }
                ++cases;
            }
    }
    for (int B : {1, 2, 63, 64, 65, 131})
        for (int dim : {1, 100, 1536, 2100})
            for (int64_t N : {(int64_t)0, (int64_t)1, (int64_t)513, (int64_t)100000})
                for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)1024})
                    for (int flags = 0; flags < 8; ++flags) {
                        check_scratch(B, dim, (dim + 7) / 8 * 8, N, cap, flags & 1, flags & 2, flags & 4);
                        ++cases;
                    }
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("range plan ok: %lld cases\n", (long long)cases);
    return 0;
}
