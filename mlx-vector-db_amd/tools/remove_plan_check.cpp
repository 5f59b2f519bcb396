// remove_plan_check.cpp — the host arithmetic of vdb_index_remove (csrc/vdb_compact_plan.h) swept
// on the CPU against a naive reference.  Stand-alone: build with -fsanitize=address,undefined
// (make plan-check) and run; every buffer is a heap allocation of exactly the size the library
// gives it, so an off-by-one in a chunk bound, a destination range or a tail extent is an
// out-of-bounds access the sanitizer reports, and a wrong row is a mismatch reported here.
//
// The model follows the device code step by step: the keep counts and their exclusive prefix
// (base), the gather of each chunk's kept rows into a scratch of chunk_words * 32 rows, the copy
// of the scratch to rows [base[w0], base[w1]), then the tail extents.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../csrc/vdb_compact_plan.h"

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

int popc(uint32_t v) { return __builtin_popcount(v); }

// One remove of `mask` (n_words words + `extra` words past them that must be ignored) from an
// index of `count` rows, chunks of `knob_rows` rows; rows are W ints wide.
void run_case(int64_t count, const std::vector<uint32_t>& mask, int64_t knob_rows, int Dp) {
    const int W = 2;                               // ints per modelled row
    const int64_t cap = (count + 1023) / 1024 * 1024;  // the index's capacity granule
    const int64_t n_words = remove_mask_words(count);
    // rows as the index holds them: row r = {r + 1, ~r}, zero past count
    int64_t* X = (int64_t*)std::calloc((size_t)cap * W, sizeof(int64_t));
    for (int64_t r = 0; r < count; ++r) {
        X[r * W] = r + 1;
        X[r * W + 1] = ~r;
    }
    // naive reference
    std::vector<int64_t> want;
    int64_t first_removed = -1;
    for (int64_t r = 0; r < count; ++r) {
        const bool rm = (mask[r / 32] >> (r % 32)) & 1u;
        if (rm && first_removed < 0) first_removed = r;
        if (!rm) want.push_back(r);
    }
    // the scan: base[w] = kept rows below word w, base[n_words] = total
    uint32_t* base = (uint32_t*)std::malloc((size_t)(n_words + 1) * sizeof(uint32_t));
    int64_t first_word = -1;
    uint32_t run = 0;
    for (int64_t w = 0; w < n_words; ++w) {
        const uint32_t valid = remove_valid_bits(w, count);
        const uint32_t keep = ~mask[w] & valid;
        base[w] = run;
        run += (uint32_t)popc(keep);
        if (keep != valid && first_word < 0) first_word = w;
    }
    base[n_words] = run;
    const int64_t kept = run;
    CHECK(kept == (int64_t)want.size(), "count %lld: kept %lld want %zu", (long long)count, (long long)kept, want.size());
    CHECK((first_removed < 0) == (first_word < 0), "first word");
    if (first_removed >= 0) CHECK(first_word == first_removed / 32, "first word %lld row %lld", (long long)first_word, (long long)first_removed);
    if (kept == count || kept == 0) {  // no-op / clear path: no chunk runs
        std::free(X);
        std::free(base);
        return;
    }
    // the gather
    const int64_t cw = std::min(remove_chunk_words(knob_rows, Dp), n_words - first_word);
    CHECK(cw >= 1, "chunk words %lld", (long long)cw);
    CHECK(cw * 32 * ((int64_t)Dp * 4 + kRowScalarBytes) <= kRemoveScratchBytes || cw == 1, "scratch bytes");
    const int64_t crows = cw * 32;
    int64_t* S = (int64_t*)std::malloc((size_t)crows * W * sizeof(int64_t));
    const int64_t n_chunks = remove_n_chunks(first_word, n_words, cw);
    int64_t covered = first_word;
    for (int64_t c = 0; c < n_chunks; ++c) {
        const RemoveChunk k = remove_chunk(first_word, n_words, cw, c);
        CHECK(k.w0 == covered && k.w1 > k.w0 && k.w1 <= n_words && k.w1 - k.w0 <= cw, "chunk %lld: [%lld, %lld)",
              (long long)c, (long long)k.w0, (long long)k.w1);
        covered = k.w1;
        for (int64_t lr = 0; lr < (k.w1 - k.w0) * 32; ++lr) {  // gather_rows_kernel
            const int64_t r = k.w0 * 32 + lr;
            if (r >= count) continue;
            const int64_t w = r >> 5;
            const int bit = (int)(r & 31);
            const uint32_t keep = ~mask[w] & remove_valid_bits(w, count);
            if (!((keep >> bit) & 1u)) continue;
            const int64_t pos = (int64_t)(base[w] - base[k.w0]) + popc(keep & ((1u << bit) - 1u));
            for (int j = 0; j < W; ++j) S[pos * W + j] = X[r * W + j];
        }
        const int64_t d0 = base[k.w0], n = base[k.w1] - base[k.w0];  // place_rows_kernel
        CHECK(d0 + n <= k.w1 * 32 && d0 + n <= count, "destination [%lld, %lld) past source end %lld", (long long)d0,
              (long long)(d0 + n), (long long)(k.w1 * 32));
        for (int64_t i = 0; i < n * W; ++i) X[d0 * W + i] = S[i];
    }
    CHECK(covered == n_words, "chunks end at word %lld of %lld", (long long)covered, (long long)n_words);
    std::free(S);
    // the tail
    const RemoveTail t = remove_tail(first_word, kept, count);
    CHECK(t.rebuild0 % 32 == 0 && t.rebuild0 <= kept && t.rebuild0 <= first_removed, "rebuild0 %lld", (long long)t.rebuild0);
    CHECK(t.tiles_end % 128 == 0 && t.tiles_end >= kept && t.tiles_end <= cap, "tiles_end %lld", (long long)t.tiles_end);
    CHECK(t.st_end % 128 == 0 && t.st_end >= t.tiles_end && t.st_end <= cap, "st_end %lld", (long long)t.st_end);
    CHECK(t.rowz_end >= kept && t.rowz_end <= count && t.rowz_end <= t.tiles_end, "rowz_end %lld", (long long)t.rowz_end);
    // row-major memset [kept, count)
    for (int64_t i = kept * W; i < count * W; ++i) X[i] = 0;
    // the tiled copies, one flag per row of capacity: 1 = holds a row's data, 0 = zero
    char* tiled = (char*)std::malloc((size_t)cap);   // split / fp32 tiles
    char* quant = (char*)std::malloc((size_t)cap);   // int8 planes
    for (int64_t r = 0; r < cap; ++r) tiled[r] = quant[r] = r < count;
    for (int64_t r = t.rebuild0; r < t.tiles_end; ++r) tiled[r] = X[r * W] != 0;  // whole tiles, from X
    for (int64_t r = t.tiles_end; r < t.st_end; ++r) tiled[r] = quant[r] = 0;       // memset of super tiles
    for (int64_t r = t.rebuild0; r < kept; ++r) quant[r] = 1;                       // row by row
    for (int64_t r = kept; r < t.rowz_end; ++r) quant[r] = 0;                       // zero_rows8
    for (int64_t r = 0; r < cap; ++r) {
        CHECK(tiled[r] == (r < kept), "tiled copy row %lld (kept %lld of %lld)", (long long)r, (long long)kept, (long long)count);
        CHECK(quant[r] == (r < kept), "int8 copy row %lld (kept %lld of %lld)", (long long)r, (long long)kept, (long long)count);
    }
    std::free(tiled);
    std::free(quant);
    // the rows
    for (int64_t i = 0; i < kept; ++i) {
        const int64_t r = want[(size_t)i];
        CHECK(X[i * W] == r + 1 && X[i * W + 1] == ~r, "row %lld holds %lld, want %lld (count %lld chunk %lld)", (long long)i,
              (long long)(X[i * W] - 1), (long long)r, (long long)count, (long long)knob_rows);
    }
    for (int64_t i = kept * W; i < cap * W; ++i) CHECK(X[i] == 0, "tail not zero at %lld", (long long)i);
    std::free(X);
    std::free(base);
}

}  // namespace

int main() {
    std::mt19937_64 rng(12345);
    const int64_t counts[] = {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1000, 1023, 1024, 1025, 2047, 2050, 5003};
    const int64_t knobs[] = {0, 1, 31, 32, 33, 64, 100, 1000, 1024, 100000};
    int64_t cases = 0;
    for (int64_t count : counts) {
        const int64_t nw = remove_mask_words(count);
        std::vector<std::vector<uint32_t>> masks;
        auto blank = [&]() { return std::vector<uint32_t>((size_t)nw, 0u); };
        auto set = [](std::vector<uint32_t>& m, int64_t r) { m[(size_t)(r / 32)] |= 1u << (r % 32); };
        {
            auto m = blank(); masks.push_back(m);                       // nothing
            m = blank(); set(m, 0); masks.push_back(m);                 // first
            m = blank(); set(m, count - 1); masks.push_back(m);         // last
            m = blank(); for (int64_t r = 0; r < count; r += 2) set(m, r); masks.push_back(m);  // every other
            m = blank(); for (int64_t r = 0; r < count; ++r) set(m, r); masks.push_back(m);     // all
            m = blank(); for (int64_t r = 1; r < count; ++r) set(m, r); masks.push_back(m);     // all but the first
            m = blank(); for (int64_t r = 0; r + 1 < count; ++r) set(m, r); masks.push_back(m); // all but the last
            m = blank(); for (int64_t r = count / 3; r < count / 3 + 32 && r < count; ++r) set(m, r); masks.push_back(m);
            m = blank(); for (int64_t r = count / 2; r < count; ++r) set(m, r); masks.push_back(m);  // the upper half
            // only bits at or past count (ignored)
            m = blank(); if (count % 32) m[(size_t)nw - 1] = ~remove_valid_bits(nw - 1, count); masks.push_back(m);
            for (double p : {0.01, 0.3, 0.5, 0.95}) {
                m = blank();
                for (int64_t r = 0; r < count; ++r)
                    if ((double)(rng() >> 11) * (1.0 / 9007199254740992.0) < p) set(m, r);
                if (count % 32) m[(size_t)nw - 1] |= ~remove_valid_bits(nw - 1, count);  // + stray high bits
                masks.push_back(m);
            }
        }
        for (const auto& m : masks)
            for (int64_t knob : knobs) {
                run_case(count, m, knob, 64);
                ++cases;
            }
    }
    // the default chunk for every row width the index accepts: at least a word, within the bytes
    for (int Dp = 64; Dp <= 65536; Dp += 64) {
        const int64_t cw = remove_chunk_words(0, Dp);
        CHECK(cw >= 1, "Dp %d", Dp);
        CHECK(cw * 32 * ((int64_t)Dp * 4 + kRowScalarBytes) <= kRemoveScratchBytes, "Dp %d: %lld words", Dp, (long long)cw);
        CHECK(remove_chunk_words(1, Dp) == 1 && remove_chunk_words(1ll << 40, Dp) == cw, "Dp %d knob clamp", Dp);
    }
    for (int64_t count = 1; count < 200; ++count)
        for (int64_t w = 0; w < remove_mask_words(count); ++w) {
            uint32_t want = 0;
            for (int b = 0; b < 32; ++b)
                if (w * 32 + b < count) want |= 1u << b;
            CHECK(remove_valid_bits(w, count) == want, "valid bits word %lld count %lld", (long long)w, (long long)count);
        }
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("remove plan ok: %lld cases\n", (long long)cases);
    return 0;
}
