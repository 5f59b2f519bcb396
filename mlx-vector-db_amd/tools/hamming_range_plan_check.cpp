// hamming_range_plan_check.cpp — the host arithmetic of vdb_index_search_hamming_range
// (csrc/vdb_hamming_range_plan.h) swept on the CPU against naive loops: the block size of the two
// scans, the chunk / tile / word mapping (every row of every chunk in exactly one lane of one wave's
// tile, its bit where the dense range search's emit kernel looks for it), the accumulator-row mapping
// the MFMA scan packs bits by (a lane pair's 32 bits are the 32 rows, once each), a scan restated from
// the mapping against a brute-force enumeration of rows, the LDS layouts (disjoint, aligned, two
// workgroups inside the budget), the scratch layout (aligned, disjoint, inside the total), the
// validation causes and the choice of scan.  A stand-alone host program (its own main, no GPU, nothing
// loaded into another process); `make hamming-range-plan-check` builds it with
// -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../csrc/vdb_hamming_range_plan.h"

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

static void check_blocks() {
    for (int W = 1; W <= kHamMaxWords; ++W) {
        CHECK(ham_range_long(W) == (W > 16), "long at W %d", W);
        for (int B : {1, 2, 3, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 65535}) {
            int want = 1;
            while (want < B && want < 16) want *= 2;
            const int blk = ham_range_pop_block(B, W);
            CHECK(blk == want, "popcount block of B %d W %d: %d, naive %d", B, W, blk, want);
            CHECK(2 * ham_range_pop_lds(blk, W) <= kHamLdsLimit, "popcount LDS of B %d W %d", B, W);
            CHECK(ham_range_block(false, B, W) == blk && ham_range_block(true, B, W) == 64, "block of B %d W %d", B, W);
        }
        // LDS of the popcount scan: queries then radii, 4-byte aligned, nothing else
        for (int qb : {1, 2, 4, 8, 16}) {
            CHECK(ham_range_pop_radius_off(qb, W) == (int64_t)qb * ((W + 15) / 16 * 16) * 8, "radius offset qb %d W %d", qb, W);
            CHECK(ham_range_pop_lds(qb, W) == ham_range_pop_radius_off(qb, W) + 4 * qb, "popcount LDS qb %d W %d", qb, W);
            CHECK(ham_lds_query_off(qb - 1, W) + (int64_t)ham_query_stride(W) * 8 <= ham_range_pop_radius_off(qb, W),
                  "the last query ends before the radii, qb %d W %d", qb, W);
        }
        // LDS of the MFMA scan: queries, staging, radii, popcounts in that order, disjoint, inside two per CU
        const int64_t q_end = (int64_t)ham_mfma_words(W) * 64 * 8;
        CHECK(ham_range_mfma_stage_off(W) == q_end, "stage offset W %d", W);
        CHECK(ham_range_mfma_radius_off(W) == q_end + 64 * 17 * 4, "radius offset W %d", W);
        CHECK(ham_range_mfma_pop_off(W) == ham_range_mfma_radius_off(W) + 256, "popcount offset W %d", W);
        CHECK(ham_range_mfma_lds(W) == ham_range_mfma_pop_off(W) + 256, "MFMA LDS W %d", W);
        CHECK(ham_range_mfma_stage_off(W) % 8 == 0 && ham_range_mfma_radius_off(W) % 4 == 0, "alignment W %d", W);
        CHECK(kHamWgPerCuLds * ham_range_mfma_lds(W) <= kHamLdsLimit, "two workgroups of the MFMA scan at W %d", W);
    }
    CHECK(kHamRangeStageStride % 2 == 1 && kHamRangeStageStride >= kRangeWgWords, "stage stride");
    // the staged word of (query q, chunk word cw) never collides with another's
    std::vector<int> seen(64 * kHamRangeStageStride, 0);
    for (int q = 0; q < 64; ++q)
        for (int cw = 0; cw < kRangeWgWords; ++cw) CHECK(seen[q * kHamRangeStageStride + cw]++ == 0, "stage slot q %d cw %d", q, cw);
}

// Every row below N lies in exactly one (chunk, wave, tile, lane); its bit is bit row % 32 of word
// row / 32, inside the chunk the dense range search's prefix and emit expect; tiles past the end are
// recognised; the second word of the last tile may lie past n_words.
static void check_mapping() {
    for (int64_t N : {1ll, 31ll, 32ll, 33ll, 63ll, 64ll, 65ll, 511ll, 512ll, 513ll, 1023ll, 1100ll, 4097ll}) {
        const int64_t n_words = range_n_words(N), n_chunks = range_n_chunks(n_words), n_tiles = ham_n_tiles(N);
        CHECK(n_chunks == (N + 511) / 512, "chunks of %lld", (long long)N);
        std::vector<int> hit(N, 0);
        std::vector<int> word_owner(n_chunks * kRangeWgWords, 0);
        for (int64_t c = 0; c < n_chunks; ++c)
            for (int wv = 0; wv < kHamRangeWaves; ++wv)
                for (int i = 0; i < kHamRangeWaveTiles; ++i) {
                    const int64_t t = ham_range_tile(c, wv, i);
                    CHECK(t == c * 8 + wv * 2 + i, "tile of chunk %lld wave %d", (long long)c, wv);
                    for (int h = 0; h < kHamRangeTileWords; ++h) {
                        const int64_t w = ham_range_word(t, h);
                        const int cw = ham_range_chunk_word(wv, i, h);
                        CHECK(w == c * kRangeWgWords + cw, "word %lld is chunk word %d", (long long)w, cw);
                        CHECK(w == range_wave_word(c, wv, i * kHamRangeTileWords + h), "the dense scan's word of the wave");
                        CHECK(word_owner[w]++ == 0, "word %lld owned once", (long long)w);
                        if (t >= n_tiles) CHECK(w >= n_words, "a tile past the end has no word below n_words");
                        const uint32_t el = ham_range_eligible(w, N, 0xFFFFFFFFu);
                        if (w >= n_words) CHECK(el == 0, "a word past n_words has no eligible row");
                        for (int bit = 0; bit < 32; ++bit) {
                            const int64_t row = t * kHamTileRows + 32 * h + bit;  // lane 32 h + bit of the tile
                            CHECK(row == w * 32 + bit, "row of lane");
                            CHECK((((el >> bit) & 1u) != 0) == (row < N), "eligibility of row %lld", (long long)row);
                            if (row < N) ++hit[row];
                        }
                    }
                }
        for (int64_t r = 0; r < N; ++r) CHECK(hit[r] == 1, "row %lld of %lld taken %d times", (long long)r, (long long)N, hit[r]);
        // the last tile's second word
        if (N % 64 >= 1 && N % 64 <= 32) CHECK(ham_range_word(n_tiles - 1, 1) >= n_words, "N %lld: the second word is past", (long long)N);
        // a mask with stray bits at and past N never makes a row past N eligible
        CHECK((ham_range_eligible(n_words - 1, N, 0xFFFFFFFFu) & ~range_valid_bits(n_words - 1, N)) == 0, "stray bits");
        CHECK(ham_range_eligible(0, N, 0u) == 0, "an empty mask word");
    }
    // the accumulator layout: a lane pair (half 0, half 1) covers the 32 rows once each
    for (int half = 0; half < 2; ++half) {
        uint32_t bits = 0;
        for (int v = 0; v < 16; ++v) {
            const int r = ham_range_acc_row(v, half);
            CHECK(r >= 0 && r < 32 && !((bits >> r) & 1u), "accumulator row %d", r);
            CHECK(r == 8 * (v / 4) + 4 * half + v % 4, "accumulator row formula");
            bits |= 1u << r;
        }
        CHECK(bits == (half ? 0xF0F0F0F0u : 0x0F0F0F0Fu), "the bits of lane half %d", half);
    }
}

// Both scans restated on the CPU from the plan's mapping (the popcount form lane by lane; the MFMA
// form through the int8 operands, the accumulator-row packing, the lane exchange and the staging)
// give the brute-force bitmap and chunk counts.
static void check_scan() {
    std::mt19937_64 rng(7);
    for (int64_t N : {1ll, 31ll, 65ll, 513ll, 1100ll})
        for (int n_bytes : {1, 3, 9, 24}) {
            const int W = ham_words(n_bytes), nq = 5;
            const int64_t n_words = range_n_words(N), n_chunks = range_n_chunks(n_words), n_tiles = ham_n_tiles(N);
            std::vector<uint8_t> X(N * n_bytes), Q(nq * n_bytes);
            for (auto& b : X) b = (uint8_t)rng();
            for (auto& b : Q) b = (uint8_t)rng();
            std::vector<uint32_t> mask(n_words);
            for (auto& m : mask) m = (uint32_t)rng();
            std::vector<uint64_t> packed(ham_packed_words(N, W), 0);
            for (int64_t r = 0; r < N; ++r)
                for (int w = 0; w < W; ++w) packed[ham_word_index(r, w, W)] = ham_word_of(&X[r * n_bytes], n_bytes, w);
            const int radii[nq] = {-1, 0, 4 * n_bytes - 2, 8 * n_bytes, 8 * n_bytes + 7};
            // brute force
            std::vector<uint32_t> Hn((size_t)nq * n_words, 0), Pn((size_t)nq * n_chunks, 0);
            for (int q = 0; q < nq; ++q)
                for (int64_t r = 0; r < N; ++r) {
                    int d = 0;
                    for (int j = 0; j < n_bytes; ++j) d += __builtin_popcount(X[r * n_bytes + j] ^ Q[q * n_bytes + j]);
                    if (((mask[r / 32] >> (r % 32)) & 1u) && d <= radii[q]) {
                        Hn[q * n_words + r / 32] |= 1u << (r % 32);
                        ++Pn[q * n_chunks + r / 512];
                    }
                }
            for (int form = 0; form < 2; ++form) {
                std::vector<uint32_t> H((size_t)nq * n_words, 0xDEADBEEFu), P((size_t)nq * n_chunks, 0xDEADBEEFu);
                for (int64_t c = 0; c < n_chunks; ++c) {
                    std::vector<uint32_t> stage(64 * kHamRangeStageStride, 0xDEADBEEFu);
                    std::vector<uint32_t> tot(nq, 0);
                    for (int wv = 0; wv < kHamRangeWaves; ++wv)
                        for (int i = 0; i < kHamRangeWaveTiles; ++i) {
                            const int64_t t = ham_range_tile(c, wv, i);
                            for (int h = 0; h < 2; ++h) {
                                const int64_t w = ham_range_word(t, h);
                                const uint32_t el = (t < n_tiles && w < n_words) ? ham_range_eligible(w, N, mask[w]) : 0u;
                                for (int q = 0; q < nq; ++q) {
                                    uint32_t word = 0;
                                    if (form == 0) {  // one lane per row, a ballot
                                        for (int bit = 0; bit < 32 && el; ++bit) {
                                            const int64_t row = t * 64 + 32 * h + bit;
                                            int d = 0;
                                            for (int x = 0; x < W; ++x)
                                                d += __builtin_popcountll(packed[ham_word_index(row, x, W)] ^ ham_word_of(&Q[q * n_bytes], n_bytes, x));
                                            if (((el >> bit) & 1u) && d <= radii[q]) word |= 1u << bit;
                                        }
                                    } else {  // d = |q| - dot by the operand mapping, packed by accumulator row
                                        int qpop = 0;
                                        for (int x = 0; x < W; ++x) qpop += __builtin_popcountll(ham_word_of(&Q[q * n_bytes], n_bytes, x));
                                        uint32_t lanes[2] = {0, 0};
                                        for (int half = 0; half < 2 && el; ++half)
                                            for (int v = 0; v < 16; ++v) {
                                                const int rl = ham_range_acc_row(v, half);
                                                const int64_t row = t * 64 + 32 * h + rl;
                                                int dot = 0;
                                                for (int bit = 0; bit < 64 * ham_mfma_words(W); ++bit) {
                                                    const int x = bit / 64;
                                                    const uint64_t xw = x < W ? packed[ham_word_index(row, x, W)] : 0ull;
                                                    const uint64_t qw = x < W ? ham_word_of(&Q[q * n_bytes], n_bytes, x) : 0ull;
                                                    dot += (int)((xw >> (bit % 64)) & 1u) * (((qw >> (bit % 64)) & 1u) ? 1 : -1);
                                                }
                                                if (qpop - dot <= radii[q]) lanes[half] |= 1u << rl;
                                            }
                                        word = (lanes[0] | lanes[1]) & el;
                                        stage[q * kHamRangeStageStride + ham_range_chunk_word(wv, i, h)] = word;
                                    }
                                    if (form == 0 && w < n_words) H[q * n_words + w] = word;
                                    if (form == 0) tot[q] += (uint32_t)__builtin_popcount(word);
                                }
                            }
                        }
                    if (form == 1)
                        for (int q = 0; q < nq; ++q)
                            for (int cw = 0; cw < kRangeWgWords; ++cw) {
                                const uint32_t word = stage[q * kHamRangeStageStride + cw];
                                CHECK(word != 0xDEADBEEFu, "every staged word is written");
                                if (c * kRangeWgWords + cw < n_words) H[q * n_words + c * kRangeWgWords + cw] = word;
                                tot[q] += (uint32_t)__builtin_popcount(word);
                            }
                    for (int q = 0; q < nq; ++q) P[q * n_chunks + c] = tot[q];
                }
                CHECK(H == Hn, "bitmap of form %d at N %lld bytes %d", form, (long long)N, n_bytes);
                CHECK(P == Pn, "chunk counts of form %d at N %lld bytes %d", form, (long long)N, n_bytes);
            }
        }
}

static void check_scratch() {
    for (int B : {1, 5, 16, 17, 64, 65, 65535})
        for (int n_bytes : {1, 9, 1024})
            for (int64_t N : {0ll, 1ll, 513ll, 10000000ll})
                for (int64_t cap : {0ll, 1ll, 1000ll})
                    for (int host = 0; host < 2; ++host)
                        for (int masked = 0; masked < 2; ++masked)
                            for (int mfma = 0; mfma < 2; ++mfma) {
                                const int block = ham_range_block(mfma, B, ham_words(n_bytes));
                                const HamRangeScratch s = hamming_range_scratch(B, n_bytes, block, N, cap, host, masked);
                                CHECK(s.block == std::min(block, B) && s.block >= 1, "block");
                                CHECK(s.n_words == (N + 31) / 32 && s.n_chunks == (s.n_words + 15) / 16, "geometry");
                                std::vector<std::pair<int64_t, int64_t>> seg = {{s.H, (int64_t)s.block * s.n_words * 4},
                                                                                {s.part, (int64_t)s.block * s.n_chunks * 4},
                                                                                {s.cnt, (int64_t)s.block * 8}};
                                if (host) {
                                    seg.push_back({s.q, (int64_t)B * n_bytes});
                                    seg.push_back({s.radii, (int64_t)B * 4});
                                    if (masked) seg.push_back({s.mask, s.n_words * 4});
                                    seg.push_back({s.out_c, (int64_t)B * 8});
                                    seg.push_back({s.out_i, (int64_t)B * cap * 8});
                                    seg.push_back({s.out_d, (int64_t)B * cap * 4});
                                    CHECK(s.in0 <= s.q && s.radii + B * 4 <= s.in0 + s.in_bytes, "inputs inside the upload");
                                    CHECK(s.out0 == s.in0 + s.in_bytes && s.out0 <= s.out_c, "outputs behind the inputs");
                                    CHECK(s.out_d + B * cap * 4 <= s.out0 + s.out_bytes, "outputs inside the download");
                                } else {
                                    CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device call stages nothing");
                                }
                                int64_t end = 0;
                                for (auto& p : seg) {
                                    CHECK(p.first % 256 == 0, "alignment");
                                    CHECK(p.first >= end, "overlap");
                                    end = p.first + p.second;
                                }
                                CHECK(end <= s.total && s.total == s.out0 + s.out_bytes, "total");
                            }
}

static void check_validation() {
    const int32_t good[3] = {0, 5, 1 << 30}, bad[3] = {0, -1, 5};
    int64_t at = -1;
    auto v = [&](bool col, int64_t B, int64_t cap, int mem, bool q, bool r, bool c, bool i, bool d, const int32_t* radii) {
        return hamming_range_validate(col, B, cap, mem, q, r, c, i, d, radii, &at);
    };
    CHECK(v(true, 3, 4, 0, true, true, true, true, true, good) == kHamRangeOk, "a good host call");
    CHECK(v(true, 3, 4, 1, true, true, true, true, true, nullptr) == kHamRangeOk, "a good device call (radii not read)");
    CHECK(v(false, 3, 4, 0, true, true, true, true, true, good) == kHamRangeNoColumn, "no column");
    CHECK(v(false, 0, 0, 0, false, false, false, false, false, nullptr) == kHamRangeNoColumn, "no column, no query");
    CHECK(v(true, -1, 4, 0, true, true, true, true, true, good) == kHamRangeBadCount, "negative batch");
    CHECK(v(true, 65536, 4, 0, true, true, true, true, true, good) == kHamRangeBadCount, "batch too large");
    CHECK(v(true, 65535, 0, 1, true, true, true, false, false, nullptr) == kHamRangeOk, "the largest batch");
    CHECK(v(true, 3, -1, 0, true, true, true, true, true, good) == kHamRangeBadCap, "negative cap");
    CHECK(v(true, 3, ((int64_t)1 << 36) / 3 + 1, 1, true, true, true, true, true, nullptr) == kHamRangeBadCap, "cap too large");
    CHECK(v(true, 3, ((int64_t)1 << 36) / 3, 1, true, true, true, true, true, nullptr) == kHamRangeOk, "the largest cap");
    CHECK(v(true, 3, 4, 2, true, true, true, true, true, good) == kHamRangeBadMem, "bad mem");
    CHECK(v(true, 0, 4, 0, false, false, false, false, false, nullptr) == kHamRangeOk, "no queries");
    CHECK(v(true, 3, 4, 0, false, true, true, true, true, good) == kHamRangeNullPointer, "NULL queries");
    CHECK(v(true, 3, 4, 0, true, false, true, true, true, nullptr) == kHamRangeNullPointer, "NULL radii");
    CHECK(v(true, 3, 4, 1, true, true, false, true, true, nullptr) == kHamRangeNullPointer, "NULL counts");
    CHECK(v(true, 3, 4, 0, true, true, true, false, true, good) == kHamRangeNullLists, "NULL indices");
    CHECK(v(true, 3, 4, 1, true, true, true, true, false, nullptr) == kHamRangeNullLists, "NULL distances");
    CHECK(v(true, 3, 0, 0, true, true, true, false, false, good) == kHamRangeOk, "count only needs no lists");
    CHECK(v(true, 3, 4, 0, true, true, true, true, true, bad) == kHamRangeNegRadius && at == 1, "a negative radius, host");
    // the choice of scan
    for (int B : {1, 16, 63, 64, 65, 65535}) {
        CHECK(ham_range_use_mfma(0, B) == (B >= kHamRangeMfmaMinQueries), "auto at B %d", B);
        CHECK(ham_range_use_mfma(1, B), "forced at B %d", B);
        CHECK(!ham_range_use_mfma(2, B), "never at B %d", B);
    }
    CHECK(!ham_range_use_mfma(1, 0), "no queries, no scan");
    for (int64_t cap : {(int64_t)0, (int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)100000, (int64_t)1 << 36}) {
        const int g = ham_range_fill_wgs(cap);
        CHECK(g >= 1 && g <= kHamRangeFillWgs, "fill workgroups of cap %lld", (long long)cap);
        if (cap <= (int64_t)kHamRangeFillWgs * kHamRangeFillSlots) CHECK((int64_t)g * kHamRangeFillSlots >= cap, "one trip covers cap %lld", (long long)cap);
    }
}

int main() {
    check_blocks();
    check_mapping();
    check_scan();
    check_scratch();
    check_validation();
    std::printf("hamming range plan ok: %ld checks\n", g_checks);
    return 0;
}
