// code_dot_plan_check.cpp — the host arithmetic of vdb_index_search_code_dot (csrc/vdb_code_dot_plan.h)
// swept on the CPU against naive loops: both forms' block sizes and LDS layouts at every width 1..1024
// bytes (inside the limit, regions disjoint), the plane count rule and the plane sum against the plain
// dot for all 256 int8 values at every plane count that admits them, a whole query against a whole
// code through the plane layout, the piece mapping of the MFMA query operand (a bijection, consistent
// with ham_mfma_slot), the K chunking, the key encoding (monotone over the whole score range), the
// validation causes, the scratch and the choice of form.  A stand-alone host program (its own main, no
// GPU, nothing loaded into another process); `make code-dot-plan-check` builds it with
// -fsanitize=address,undefined and runs it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../csrc/vdb_code_dot_plan.h"

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

// Every int8 value: the fewest bits, and at every m that admits it the weighted planes give it back.
static void check_planes_of_a_value() {
    for (int v = -128; v <= 127; ++v) {
        int want = 1;
        while (v < -(1 << (want - 1)) || v > (1 << (want - 1)) - 1) ++want;
        CHECK(cd_bits_needed((int8_t)v) == want, "bits of %d: %d, naive %d", v, cd_bits_needed((int8_t)v), want);
        for (int m = want; m <= kCdMaxPlanes; ++m) {
            int sum = 0;
            for (int p = 0; p < m; ++p) sum += (((uint8_t)v >> p) & 1) * cd_plane_weight(p, m);
            CHECK(sum == v, "plane sum of %d at m %d: %d", v, m, sum);
        }
        // eight at once, the value in any byte among smaller ones
        for (int at = 0; at < 8; ++at) {
            uint64_t v8 = 0;
            for (int i = 0; i < 8; ++i) v8 |= (uint64_t)(uint8_t)(i == at ? v : (i & 1 ? -1 : 0)) << (8 * i);
            CHECK(cd_bits_needed8(v8) == want, "bits of eight with %d at %d", v, at);
            for (int p = 0; p < 8; ++p)
                CHECK(((cd_plane_byte(v8, p) >> at) & 1u) == (((uint8_t)v >> p) & 1u), "plane byte of %d, p %d", v, p);
        }
    }
}

// A query against a code through the plane layout of a block: the sum over m planes of weighted
// popcounts of AND words equals the plain dot, for value ranges of every plane count.
static void check_plane_dot(std::mt19937& rng) {
    for (int n_bytes : {1, 3, 8, 9, 24, 129, 136, 1024}) {
        const int W = ham_words(n_bytes), WS = ham_query_stride(W), n_bits = 8 * n_bytes;
        CHECK(WS % kHamPassWords == 0 && WS >= W, "stride of %d", W);
        for (int m_want = 1; m_want <= kCdMaxPlanes; ++m_want) {
            const int lo = -(1 << (m_want - 1)), hi = (1 << (m_want - 1)) - 1;
            std::vector<int8_t> q(n_bits);
            std::vector<uint8_t> code(n_bytes);
            for (auto& v : q) v = (int8_t)(lo + (int)(rng() % (unsigned)(hi - lo + 1)));
            q[rng() % n_bits] = (int8_t)lo;  // the value that needs all m_want bits
            for (auto& c : code) c = (uint8_t)rng();
            // the kernel's staging: byte g of every plane from the eight values of code byte g
            std::vector<uint8_t> lds((size_t)cd_plane_lds(1, W), 0);
            int m = 1;
            for (int g = 0; g < n_bytes; ++g) {
                uint64_t v8;
                std::memcpy(&v8, q.data() + 8 * g, 8);
                m = std::max(m, cd_bits_needed8(v8));
                for (int p = 0; p < kCdMaxPlanes; ++p) {
                    const int64_t o = cd_plane_byte_off(0, p, W) + g;
                    CHECK(o >= 0 && o < (int64_t)lds.size(), "plane byte offset %lld", (long long)o);
                    lds[(size_t)o] = (uint8_t)cd_plane_byte(v8, p);
                }
            }
            CHECK(m == m_want, "m %d of range %d at %d bytes", m, m_want, n_bytes);
            int64_t s = 0, want = 0;
            for (int p = 0; p < m; ++p) {
                int c = 0;
                for (int w = 0; w < W; ++w) {
                    uint64_t pw;
                    std::memcpy(&pw, lds.data() + cd_plane_byte_off(0, p, W) + 8 * w, 8);
                    c += __builtin_popcountll(pw & ham_word_of(code.data(), n_bytes, w));
                }
                s += (int64_t)c * cd_plane_weight(p, m);
            }
            for (int j = 0; j < n_bits; ++j) want += q[j] * ((code[j / 8] >> (j % 8)) & 1);
            CHECK(s == want, "plane dot %lld, plain %lld at %d bytes, m %d", (long long)s, (long long)want, n_bytes, m);
        }
    }
}

// Both forms at every width: inside the LDS limit, regions disjoint and in order.
static void check_lds() {
    for (int n_bytes = 1; n_bytes <= kHamMaxBytes; ++n_bytes) {
        const int W = ham_words(n_bytes);
        for (int k : {1, 10, 32, 33, 64, 65, 128, 256, 257, 512, 1024}) {
            const int KE = ham_ke(k), qb = cd_qb(k, W);
            CHECK(qb >= 1 && qb <= kCdMaxQB && (qb & (qb - 1)) == 0, "qb %d", qb);
            CHECK(kHamWgPerCuLds * (cd_lds_bytes(qb, W, KE, true) + kCdStaticLds) <= kHamLdsLimit, "plane form k %d bytes %d", k, n_bytes);
            // the largest that fits (kCdMaxQB is no limit of its own: twice it never fits)
            CHECK(kHamWgPerCuLds * (cd_lds_bytes(2 * qb, W, KE, true) + kCdStaticLds) > kHamLdsLimit, "qb %d is not the largest", qb);
            CHECK(cd_plane_byte_off(qb - 1, kCdMaxPlanes - 1, W) + ham_query_stride(W) * 8 == cd_plane_lds(qb, W), "planes end");
            CHECK(cd_lds_key_off(0, 0, qb, W, KE) == cd_plane_lds(qb, W), "keys follow the planes");
            CHECK(cd_lds_row_off(kHamWaves - 1, qb - 1, qb, W, KE) + ham_cap(KE) * 4 <= cd_lds_bytes(qb, W, KE, false), "rows end");
            for (int nq : {1, 2, 3, qb, qb + 1, 1000}) {
                const int b = cd_block(k, W, nq);
                CHECK(b <= qb && (b & (b - 1)) == 0 && (b >= nq || b == qb), "block %d of %d queries", b, nq);
            }
        }
        CHECK(cd_mfma_lds_bytes(W) + kHamMfmaStaticLds <= kHamLdsLimit, "mfma form at %d bytes", n_bytes);
        const int pairs = cd_mfma_pairs(W), kch = cd_mfma_k_chunks(W);
        CHECK(pairs * 2 >= W && pairs * 2 <= W + 1, "pairs of %d words", W);
        CHECK((kch == 1) == (n_bytes <= kCdMfmaChunkBytes), "chunks of %d bytes: %d", n_bytes, kch);
        CHECK((kch - 1) * kCdMfmaChunkPairs < pairs && pairs <= kch * kCdMfmaChunkPairs, "chunks cover the pairs");
        CHECK(cd_mfma_cand_off(W) == (int64_t)std::min(pairs, kCdMfmaChunkPairs) * kCdPairLds, "pieces end");
        CHECK(cd_mfma_cnt_off(W) + kHamMfmaQB * 4 == cd_mfma_lds_bytes(W) && cd_mfma_thr_off(W) % 8 == 0, "tail regions");
    }
    CHECK((kCdMfmaChunkPairs + 1) * kCdPairLds + kCdMfmaTopkLds + kHamMfmaStaticLds > kHamLdsLimit, "the chunk is the largest");
    CHECK(cd_qb(64, kHamMaxWords) == 4 && cd_qb(1024, kHamMaxWords) == 1 && cd_qb(10, 4) == 8 && cd_qb(64, 80) == 8 && cd_qb(64, 81) == 4, "block sizes");
}

// The piece mapping: every dimension of a code of W words is read by exactly one (step, half, byte),
// the one ham_mfma_slot sends its code bit to; LDS offsets of a chunk's pieces are distinct and inside.
static void check_pieces() {
    for (int W : {1, 2, 3, 22, 23, 24, 127, 128}) {
        const int n_dims = 64 * ham_mfma_words(W);
        std::vector<int> seen(n_dims, 0);
        for (int step = 0; step < ham_mfma_steps(W); ++step)
            for (int half = 0; half < 2; ++half) {
                const int piece = cd_mfma_piece(step, half);
                CHECK(kCdPieceBytes * piece == 64 * ham_mfma_word(step, half) + ham_mfma_shift(step), "piece %d", piece);
                for (int byte = 0; byte < kCdPieceBytes; ++byte) {
                    const int dim = kCdPieceBytes * piece + byte;
                    CHECK(dim < n_dims, "dim %d", dim);
                    ++seen[dim];
                    const HamMfmaSlot sl = ham_mfma_slot(dim);
                    CHECK(sl.step == step && sl.half == half && sl.byte == byte, "dim %d against the row side", dim);
                }
                // inside its chunk's LDS
                const int ch = (step / 4) / kCdMfmaChunkPairs, lp = piece - kCdPiecesPerPair * ch * kCdMfmaChunkPairs;
                CHECK(lp >= 0 && cd_mfma_piece_off(lp, kHamMfmaQB - 1) + kCdPieceBytes <= cd_mfma_cand_off(W), "piece %d in LDS", piece);
                CHECK(cd_mfma_piece_off(lp, 1) - cd_mfma_piece_off(lp, 0) == kCdPieceBytes, "queries of a piece are adjacent");
            }
        for (int d = 0; d < n_dims; ++d) CHECK(seen[d] == 1, "dim %d read %d times", d, seen[d]);
    }
}

static void check_key_and_form() {
    uint64_t last = 0;
    for (int32_t s = kCdBias; s >= -kCdBias; --s) {  // the best score first
        const uint64_t lo = cd_key(s, 0), hi = cd_key(s, 0xFFFFFFFEu);
        CHECK(lo < hi && (s == kCdBias || last < lo), "key order at %d", s);
        CHECK(cd_score_of_key_hi((uint32_t)(lo >> 32)) == s, "score back from the key at %d", s);
        CHECK((float)(uint32_t)(lo >> 32) == (double)(uint32_t)(lo >> 32), "fp32 holds the key of %d", s);
        CHECK((int32_t)(float)s == s, "fp32 holds %d", s);
        last = hi;
    }
    CHECK(last < ~0ull, "the worst key is below the empty one");
    for (int knob = -1; knob <= 3; ++knob) CHECK(code_dot_knob_ok(knob) == (knob >= 0 && knob <= 2), "knob %d", knob);
    CHECK(!code_dot_use_mfma(0, kCdMfmaMinQueries - 1, 10, 128) && code_dot_use_mfma(0, kCdMfmaMinQueries, 10, 128), "auto threshold");
    CHECK(code_dot_use_mfma(1, 1, kHamMfmaMaxK, 1) && !code_dot_use_mfma(1, 1000, kHamMfmaMaxK + 1, 1), "knob 1");
    CHECK(!code_dot_use_mfma(2, 1000, 10, 128) && !code_dot_use_mfma(1, 0, 10, 128), "knob 2, no query");
    // validation: one cause each, in order
    CHECK(code_dot_validate_call(0, 1, false, false, false, 0, true) == kCdOk, "an empty batch");
    CHECK(code_dot_validate_call(-1, 1, true, true, true, 0, true) == kCdBadCount, "count");
    CHECK(code_dot_validate_call(kHamMaxQueries + 1, 1, true, true, true, 0, true) == kCdBadCount, "count");
    CHECK(code_dot_validate_call(1, 0, true, true, true, 0, true) == kCdBadK, "k");
    CHECK(code_dot_validate_call(1, kHamMaxK + 1, true, true, true, 0, true) == kCdBadK, "k");
    CHECK(code_dot_validate_call(1, 1, true, true, true, 2, true) == kCdBadMem, "mem");
    for (int missing = 0; missing < 3; ++missing)
        CHECK(code_dot_validate_call(1, 1, missing != 0, missing != 1, missing != 2, 1, true) == kCdNullPointer, "pointer %d", missing);
    CHECK(code_dot_validate_call(1, 1, true, true, true, 1, false) == kCdNoColumn, "column");
    // scratch: the queries region holds 8 * n_bytes bytes per query
    for (int n_bytes : {1, 9, 1024})
        for (int nq : {1, 65}) {
            const HammingScratch sc = code_dot_scratch(nq, n_bytes, 10, 16, 3, 1300, true, true);
            CHECK(sc.mask - sc.q >= (int64_t)nq * 8 * n_bytes && sc.q % 256 == 0, "queries region");
            CHECK(sc.out_i - sc.out_d >= (int64_t)nq * 10 * 4 && sc.total >= sc.out_i + (int64_t)nq * 10 * 8, "results region");
        }
}

int main() {
    std::mt19937 rng(12345);
    check_planes_of_a_value();
    check_plane_dot(rng);
    check_lds();
    check_pieces();
    check_key_and_form();
    std::printf("code dot plan ok: %ld checks, K chunk %d pairs (%d bytes)\n", g_checks, kCdMfmaChunkPairs, kCdMfmaChunkBytes);
    return 0;
}
