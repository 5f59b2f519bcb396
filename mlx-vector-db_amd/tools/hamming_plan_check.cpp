// hamming_plan_check.cpp — the host arithmetic of vdb_index_set_codes and vdb_index_search_hamming
// (csrc/vdb_hamming_plan.h) swept on the CPU against naive loops: the query-block size QB, the deal
// of tiles to segments and waves (every row exactly once), the tile / word / lane address of a row's
// byte (a packed column restated from it gives the naive distances), the LDS layout (disjoint,
// inside the budget), the validation causes and the scratch layout (aligned, disjoint, inside the
// total), and the integer-MFMA form's bit mapping, operands, LDS layout and eligibility.  A stand-alone host program (its own main, no GPU, nothing loaded into another process);
// `make hamming-plan-check` builds it with -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../csrc/vdb_hamming_plan.h"

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

static int naive_pow2_at_least(int v) {
    int p = 1;
    while (p < v) p *= 2;
    return p;
}

static void check_qb() {
    for (int k = 1; k <= kHamMaxK; ++k) {
        const int KE = ham_ke(k);
        CHECK(KE == std::max(32, naive_pow2_at_least(k)), "KE of %d", k);
        CHECK(ham_cap(KE) == naive_pow2_at_least(std::max(2 * KE, KE + 64)), "cap of %d", KE);
        CHECK(ham_merge_lds(KE) == (int64_t)std::max(ham_cap(KE), 1024) * 8, "merge lds of %d", KE);
        // naive: try every power of two from the largest down
        int want = 1;
        for (int qb = kHamMaxQB; qb >= 1; qb /= 2) {
            const int64_t tk = (int64_t)4 * qb * ham_cap(KE) * 8;
            const int64_t lds = (int64_t)qb * kHamMaxBytes + std::max(tk, ham_merge_lds(KE));
            if (2 * lds <= 160 * 1024) {
                want = qb;
                break;
            }
        }
        const int qb = ham_qb(k);
        CHECK(qb == want, "QB of k %d: %d, naive %d", k, qb, want);
        CHECK((qb & (qb - 1)) == 0 && qb >= 1 && qb <= kHamMaxQB, "QB %d", qb);
        if (k <= 16) CHECK(qb >= 16, "QB %d at k %d", qb, k);
        // every width fits the launch's limit with that block, merge buffer or not
        for (int W : {1, 2, 16, 17, 128})
            for (bool merge : {false, true})
                CHECK(ham_lds_bytes(qb, W, KE, merge) <= kHamLdsLimit, "LDS of k %d W %d", k, W);
        for (int B : {1, 2, 3, 15, 16, 17, 1000}) {
            const int blk = ham_block(k, B);
            CHECK(blk == std::min(qb, naive_pow2_at_least(B)), "block of k %d B %d: %d", k, B, blk);
            const int nb = ham_n_blocks(B, blk);
            CHECK((int64_t)nb * blk >= B && (int64_t)(nb - 1) * blk < B, "blocks of B %d", B);
        }
    }
    CHECK(ham_qb(1) == 16 && ham_qb(10) == 16 && ham_qb(64) == 16 && ham_qb(128) == 8 && ham_qb(256) == 4 &&
              ham_qb(512) == 2 && ham_qb(1024) == 1,
          "the QB table");
}

static void check_deal() {
    for (int64_t N : {0, 1, 3, 63, 64, 65, 255, 256, 257, 513, 1300, 5000}) {
        const int64_t tiles = ham_n_tiles(N), chunks = ham_n_chunks(N);
        CHECK(tiles == (N + 63) / 64 && chunks == (N + 255) / 256, "tiles / chunks of %lld", (long long)N);
        CHECK(ham_mask_words(N) == (N + 31) / 32, "mask words");
        for (int n_seg : {1, 2, 7, 64, 512}) {
            const int live = ham_live_segs(N, n_seg);
            CHECK(live == (int)std::min<int64_t>(chunks, n_seg), "live segments N %lld n_seg %d", (long long)N, n_seg);
            std::vector<int> seen((size_t)N, 0);
            for (int s = 0; s < live; ++s)
                for (int64_t c = s; c < chunks; c += n_seg)
                    for (int wv = 0; wv < kHamWaves; ++wv) {
                        const int64_t t = ham_tile_of(c, wv);
                        if (t >= tiles) continue;
                        // the mask words the wave's two lanes load
                        for (int l = 0; l < 2; ++l)
                            if (2 * t + l >= ham_mask_words(N)) CHECK((2 * t + l) * 32 >= N, "a mask word with rows is skipped");
                        for (int lane = 0; lane < kHamTileRows; ++lane) {
                            const int64_t r = t * kHamTileRows + lane;
                            if (r < N) ++seen[(size_t)r];
                        }
                    }
            for (int s = live; s < n_seg; ++s) CHECK(s >= chunks, "segment %d of %d has a chunk", s, n_seg);
            for (int64_t r = 0; r < N; ++r) CHECK(seen[(size_t)r] == 1, "row %lld seen %d times", (long long)r, seen[(size_t)r]);
        }
    }
    for (int64_t N : {0, 1, 256, 257, 100000, 1000000})
        for (int nb : {1, 5, 64, 2000}) {
            const int a = ham_n_seg(0, N, nb, 256);
            CHECK(a >= 1 && a <= kHamMaxSeg, "auto n_seg %d", a);
            CHECK(a <= std::max<int64_t>(1, ham_n_chunks(N)), "more segments than chunks");
            CHECK((int64_t)a * nb <= std::max<int64_t>(nb, 256 * kHamWgPerCu), "grid too large: %d x %d", a, nb);
            for (int64_t knob : {1, 2, 7, 512, 9999})
                CHECK(ham_n_seg(knob, N, nb, 256) == (int)std::min<int64_t>(knob, kHamMaxSeg), "knob %lld", (long long)knob);
        }
}

static int naive_distance(const uint8_t* a, const uint8_t* b, int n_bytes) {
    int d = 0;
    for (int j = 0; j < n_bytes; ++j)
        for (int bit = 0; bit < 8; ++bit) d += ((a[j] ^ b[j]) >> bit) & 1;
    return d;
}

static void check_layout() {
    std::mt19937 rng(7);
    for (int64_t N : {1, 63, 64, 65, 200})
        for (int n_bytes : {1, 7, 8, 9, 128, 136, 1024}) {
            const int W = ham_words(n_bytes);
            CHECK(W == (n_bytes + 7) / 8, "words of %d", n_bytes);
            std::vector<uint8_t> codes((size_t)N * n_bytes), q((size_t)n_bytes);
            for (auto& b : codes) b = (uint8_t)rng();
            for (auto& b : q) b = (uint8_t)rng();
            // pack as the kernel does: one packed word per (tile, w, lane)
            const int64_t words = ham_packed_words(N, W);
            CHECK(words == (N + 63) / 64 * W * 64, "packed words");
            std::vector<uint64_t> packed((size_t)words, ~0ull);
            std::vector<int> hit((size_t)words, 0);
            for (int64_t o = 0; o < words; ++o) {
                const int lane = (int)(o & 63);
                const int64_t tw = o >> 6;
                const int w = (int)(tw % W);
                const int64_t r = (tw / W) * kHamTileRows + lane;
                packed[(size_t)o] = r < N ? ham_word_of(codes.data() + r * n_bytes, n_bytes, w) : 0ull;
                if (r < N) {
                    CHECK(ham_word_index(r, w, W) == o, "word index of row %lld word %d", (long long)r, w);
                    ++hit[(size_t)o];
                }
            }
            // byte j of row r is where the header says, and the pad bytes are zero
            for (int64_t r = 0; r < N; ++r)
                for (int j = 0; j < 8 * W; ++j) {
                    const int64_t o = ham_word_index(r, j / 8, W);
                    CHECK(o >= 0 && o < words && hit[(size_t)o] == 1, "address of row %lld byte %d", (long long)r, j);
                    const uint8_t got = (uint8_t)(packed[(size_t)o] >> (8 * (j % 8)));
                    CHECK(got == (j < n_bytes ? codes[(size_t)(r * n_bytes + j)] : 0), "row %lld byte %d", (long long)r, j);
                }
            // the distance a lane forms, pass by pass over the padded query, is the naive one
            const int WS = ham_query_stride(W);
            CHECK(WS % kHamPassWords == 0 && WS >= W && WS - W < kHamPassWords, "query stride of %d", W);
            std::vector<uint64_t> qw((size_t)WS, 0);
            for (int w = 0; w < W; ++w) qw[(size_t)w] = ham_word_of(q.data(), n_bytes, w);
            for (int64_t r = 0; r < N; ++r) {
                int d = 0;
                for (int w0 = 0; w0 < W; w0 += kHamPassWords)
                    for (int j = 0; j < kHamPassWords; ++j) {
                        const uint64_t x = w0 + j < W ? packed[(size_t)ham_word_index(r, w0 + j, W)] : 0ull;
                        d += __builtin_popcountll(x ^ qw[(size_t)(w0 + j)]);
                    }
                CHECK(d == naive_distance(codes.data() + r * n_bytes, q.data(), n_bytes), "distance of row %lld", (long long)r);
            }
        }
}

static void check_lds() {
    for (int k : {1, 10, 64, 65, 128, 256, 512, 1024})
        for (int B : {1, 3, 16, 100})
            for (int W : {1, 16, 17, 128}) {
                const int KE = ham_ke(k), qb = ham_block(k, B), cap = ham_cap(KE);
                const int64_t total = ham_lds_bytes(qb, W, KE, false);
                std::vector<std::pair<int64_t, int64_t>> spans;  // [lo, hi)
                for (int q = 0; q < qb; ++q) spans.push_back({ham_lds_query_off(q, W), ham_lds_query_off(q, W) + ham_query_stride(W) * 8});
                for (int wv = 0; wv < kHamWaves; ++wv)
                    for (int q = 0; q < qb; ++q) {
                        spans.push_back({ham_lds_key_off(wv, q, qb, W, KE), ham_lds_key_off(wv, q, qb, W, KE) + cap * 4});
                        spans.push_back({ham_lds_row_off(wv, q, qb, W, KE), ham_lds_row_off(wv, q, qb, W, KE) + cap * 4});
                    }
                std::sort(spans.begin(), spans.end());
                CHECK(spans.front().first == 0 && spans.back().second == total, "LDS extent k %d B %d W %d", k, B, W);
                for (size_t i = 0; i + 1 < spans.size(); ++i)
                    CHECK(spans[i].second == spans[i + 1].first, "LDS spans overlap or gap at %zu", i);
                for (auto& sp : spans) CHECK(sp.first % 8 == 0, "LDS alignment");
                // the merge buffer starts where the top-k buffers do and fits the launch's size
                CHECK(ham_query_lds(qb, W) + ham_merge_lds(KE) <= ham_lds_bytes(qb, W, KE, true), "merge buffer");
                CHECK(ham_lds_bytes(qb, W, KE, true) <= kHamLdsLimit, "LDS limit");
            }
}

static void check_validation() {
    CHECK(hamming_column_args(false, 0, 0, 5) == kHamColOk, "detach");
    CHECK(hamming_column_args(false, 1, 8, 5) == kHamColBadRows, "detach with rows");
    CHECK(hamming_column_args(true, 4, 8, 5) == kHamColBadRows, "row count");
    CHECK(hamming_column_args(true, 5, 0, 5) == kHamColBadWidth, "zero width");
    CHECK(hamming_column_args(true, 5, 1025, 5) == kHamColBadWidth, "too wide");
    CHECK(hamming_column_args(true, 5, -1, 5) == kHamColBadWidth, "negative width");
    CHECK(hamming_column_args(true, 5, 1, 5) == kHamColOk && hamming_column_args(true, 5, 1024, 5) == kHamColOk, "widths");
    CHECK(hamming_column_args(true, 0, 16, 0) == kHamColOk, "an empty column");
    CHECK(hamming_validate_call(1, 10, true, true, true, 0, true) == kHamOk, "a good call");
    CHECK(hamming_validate_call(0, 10, false, false, false, 1, true) == kHamOk, "no queries");
    CHECK(hamming_validate_call(-1, 10, true, true, true, 0, true) == kHamBadCount, "negative count");
    CHECK(hamming_validate_call(65536, 10, true, true, true, 0, true) == kHamBadCount, "too many queries");
    CHECK(hamming_validate_call(65535, 10, true, true, true, 0, true) == kHamOk, "the most queries");
    CHECK(hamming_validate_call(1, 0, true, true, true, 0, true) == kHamBadK, "k 0");
    CHECK(hamming_validate_call(1, 1025, true, true, true, 0, true) == kHamBadK, "k 1025");
    CHECK(hamming_validate_call(1, 1024, true, true, true, 1, true) == kHamOk, "k 1024");
    CHECK(hamming_validate_call(1, 10, true, true, true, 2, true) == kHamBadMem, "mem");
    CHECK(hamming_validate_call(1, 10, false, true, true, 0, true) == kHamNullPointer, "NULL queries");
    CHECK(hamming_validate_call(1, 10, true, false, true, 0, true) == kHamNullPointer, "NULL distances");
    CHECK(hamming_validate_call(1, 10, true, true, false, 1, true) == kHamNullPointer, "NULL indices");
    CHECK(hamming_validate_call(1, 10, true, true, true, 0, false) == kHamNoColumn, "no column");
    CHECK(hamming_validate_call(0, 10, false, false, false, 0, false) == kHamNoColumn, "no column, no queries");
}

static void check_scratch() {
    for (int B : {1, 16, 17, 300})
        for (int k : {1, 10, 1024})
            for (int n_bytes : {1, 9, 1024})
                for (int n_seg : {1, 2, 7})
                    for (int64_t rows : {0, 1, 65, 1300})
                        for (int flags = 0; flags < 4; ++flags) {
                            const bool host = flags & 1, masked = flags & 2;
                            const int qb = ham_block(k, B);
                            const int64_t KE = ham_ke(k), nb = ham_n_blocks(B, qb);
                            const HammingScratch s = hamming_scratch(B, n_bytes, k, qb, n_seg, rows, host, masked);
                            std::vector<std::pair<int64_t, int64_t>> spans;
                            auto add = [&](int64_t at, int64_t bytes) {
                                CHECK(at % 256 == 0 && at >= 0 && at + bytes <= s.total, "scratch span");
                                if (bytes > 0) spans.push_back({at, at + bytes});
                            };
                            add(s.done, nb * 4);
                            if (n_seg > 1) {
                                add(s.lk, (int64_t)B * n_seg * KE * 4);
                                add(s.li, (int64_t)B * n_seg * KE * 4);
                                add(s.mk, B * KE * 4);
                                add(s.mi, B * KE * 4);
                            }
                            if (host) {
                                add(s.q, (int64_t)B * n_bytes);
                                if (masked) add(s.mask, s.mask_words * 4);
                                add(s.out_d, (int64_t)B * k * 4);
                                add(s.out_i, (int64_t)B * k * 8);
                                CHECK(s.q == s.in0 && s.out_d == s.out0, "staging starts");
                                CHECK(s.in0 + s.in_bytes == s.out0 && s.out0 + s.out_bytes == s.total, "staging extents");
                            } else {
                                CHECK(s.in_bytes == 0 && s.out_bytes == 0, "a device call stages nothing");
                            }
                            CHECK(s.mask_words == (rows + 31) / 32, "mask words");
                            std::sort(spans.begin(), spans.end());
                            for (size_t i = 0; i + 1 < spans.size(); ++i)
                                CHECK(spans[i].second <= spans[i + 1].first, "scratch spans overlap");
                        }
}

// The integer-MFMA form: the bit-to-slot mapping is a bijection and agrees with what a lane reads and
// expands, the operands give the distance by |q| - dot, the LDS layout is disjoint and inside the
// budget, and ham_use_mfma decides as stated at every boundary.
static void check_mfma() {
    std::mt19937 rng(11);
    for (int n_bytes : {1, 3, 4, 5, 8, 9, 16, 24, 136, 1023, 1024}) {
        const int W = ham_words(n_bytes), steps = ham_mfma_steps(W);
        CHECK(ham_mfma_words(W) == W + W % 2 && steps == 4 * ((W + 1) / 2), "steps of W %d", W);
        // every bit (pad bits of the last word included) lands in exactly one (step, half, byte) slot
        std::vector<int> hit((size_t)steps * 32, 0);
        for (int bit = 0; bit < 64 * W; ++bit) {
            const HamMfmaSlot sl = ham_mfma_slot(bit);
            CHECK(sl.step >= 0 && sl.step < steps && (sl.half == 0 || sl.half == 1) && sl.byte >= 0 && sl.byte < 16, "slot of bit %d", bit);
            ++hit[(size_t)(sl.step * 2 + sl.half) * 16 + sl.byte];
            // and it is where a lane of that half finds it: word, shift and byte of the expansion
            CHECK(ham_mfma_word(sl.step, sl.half) == bit / 64 && ham_mfma_shift(sl.step) + sl.byte == bit % 64, "read of bit %d", bit);
        }
        int used = 0;
        for (int h : hit) {
            CHECK(h <= 1, "a slot taken twice");
            used += h;
        }
        CHECK(used == 64 * W, "slots used");
        for (int st = 0; st < steps; ++st)
            for (int h = 0; h < 2; ++h) CHECK(ham_mfma_word(st, h) < ham_mfma_words(W), "a word past the padded row");
        // the operands: rows 0 / 1, queries -1 / +1, distance = |q| - dot, the missing pair word zero
        for (int rep = 0; rep < 4; ++rep) {
            std::vector<uint8_t> x((size_t)n_bytes), q((size_t)n_bytes);
            for (auto& b : x) b = rep == 1 ? 0xFF : rep == 2 ? 0 : (uint8_t)rng();
            for (auto& b : q) b = rep == 1 ? 0 : rep == 2 ? 0xFF : (uint8_t)rng();
            int dot = 0, qpop = 0;
            for (int w = 0; w < W; ++w) qpop += __builtin_popcountll(ham_word_of(q.data(), n_bytes, w));
            for (int st = 0; st < steps; ++st)
                for (int h = 0; h < 2; ++h) {
                    const int w = ham_mfma_word(st, h);
                    const uint64_t xw = w < W ? ham_word_of(x.data(), n_bytes, w) : 0ull;
                    const uint64_t qw = w < W ? ham_word_of(q.data(), n_bytes, w) : 0ull;
                    for (int d = 0; d < 4; ++d) {
                        const uint32_t xe = ham_mfma_row4((uint32_t)(xw >> (ham_mfma_shift(st) + 4 * d)));
                        const uint32_t qe = ham_mfma_query4((uint32_t)(qw >> (ham_mfma_shift(st) + 4 * d)));
                        for (int i = 0; i < 4; ++i) {
                            const int xb = (int8_t)(xe >> (8 * i)), qb = (int8_t)(qe >> (8 * i));
                            const int bit = ham_mfma_shift(st) + 4 * d + i;
                            CHECK(xb == (int)((xw >> bit) & 1) && qb == 2 * (int)((qw >> bit) & 1) - 1, "expansion of bit %d", bit);
                            dot += xb * qb;
                        }
                    }
                }
            CHECK(qpop - dot == naive_distance(x.data(), q.data(), n_bytes), "distance by the dot product, %d bytes", n_bytes);
            CHECK(dot >= -8192 && dot <= 8192, "dot range");
        }
    }
    // eligibility and LDS
    CHECK(kHamMfmaMinQueries >= 32, "the auto threshold");
    for (int k = 1; k <= kHamMaxK; ++k) {
        const int qb = ham_mfma_qb(k);
        CHECK(qb == (k <= kHamMfmaMaxK ? kHamMfmaQB : 0), "mfma QB of k %d", k);
        if (!qb) continue;
        CHECK(ham_merge_lds(ham_ke(k)) <= 64 * 1024, "the merge launch's LDS needs no opt-in");
        CHECK(k + kHamTileRows <= kHamMfmaCap && kHamMfmaHigh < kHamMfmaCap, "one wave's offers fit");
    }
    CHECK(ham_mfma_qb(10) == 64 && ham_mfma_qb(0) == 0, "k = 10 is served");
    for (int W = 1; W <= kHamMaxWords; ++W) {
        std::vector<std::pair<int64_t, int64_t>> spans;
        spans.push_back({0, ham_mfma_query_lds(W)});
        for (int q = 0; q < kHamMfmaQB; ++q) spans.push_back({ham_mfma_cand_off(W) + (int64_t)q * kHamMfmaCap * 8, ham_mfma_cand_off(W) + (int64_t)(q + 1) * kHamMfmaCap * 8});
        spans.push_back({ham_mfma_thr_off(W), ham_mfma_thr_off(W) + kHamMfmaQB * 8});
        spans.push_back({ham_mfma_cnt_off(W), ham_mfma_cnt_off(W) + kHamMfmaQB * 4});
        std::sort(spans.begin(), spans.end());
        CHECK(spans.front().first == 0 && spans.back().second == ham_mfma_lds_bytes(W), "mfma LDS extent W %d", W);
        for (size_t i = 0; i + 1 < spans.size(); ++i) CHECK(spans[i].second == spans[i + 1].first, "mfma LDS overlap or gap");
        for (auto& sp : spans) CHECK(sp.first % 8 == 0, "mfma LDS alignment");
        CHECK(ham_mfma_query_lds(W) == (int64_t)(W + W % 2) * 64 * 8, "query words of W %d", W);
        CHECK(ham_mfma_lds_bytes(W) + kHamMfmaStaticLds <= 160 * 1024, "mfma LDS limit W %d", W);
    }
    for (int64_t knob : {0, 1, 2})
        for (int B : {1, 31, 32, kHamMfmaMinQueries - 1, kHamMfmaMinQueries, kHamMfmaMinQueries + 1, 1024, kHamMaxQueries})
            for (int k : {1, 10, kHamMfmaMaxK, kHamMfmaMaxK + 1, 1024})
                for (int n_bytes : {1, 24, 1024}) {
                    const bool want = knob != 2 && k <= kHamMfmaMaxK && (knob == 1 || B >= kHamMfmaMinQueries);
                    CHECK(ham_use_mfma(knob, B, k, n_bytes) == want, "use_mfma knob %lld B %d k %d", (long long)knob, B, k);
                }
    CHECK(!ham_use_mfma(1, 0, 10, 8) && !ham_use_mfma(1, 64, 10, 0) && !ham_use_mfma(1, 64, 10, 1025), "degenerate calls");
}

int main() {
    check_qb();
    check_deal();
    check_layout();
    check_lds();
    check_validation();
    check_scratch();
    check_mfma();
    std::printf("hamming plan ok: %ld checks\n", g_checks);
    return 0;
}
