// encode_plan_check.cpp — the arithmetic of vdb_index_encode_codes / vdb_index_encode
// (csrc/vdb_encode_plan.h) swept on the CPU.  Stand-alone: build with -fsanitize=address,undefined and
// -ffp-contract=off (make encode-plan-check) and run.
//
//   decision    encode_decide against the canonical fp64 sum (the order of csrc/vdb_common.h restated
//               here) for fp32 dot products summed in three orders, with round-to-nearest, with
//               truncation and with denormals flushed, at thresholds on, beside and around the sum, for
//               ordinary, 2^-70-scaled, 2^63-scaled and zero vectors: a one or a zero it declares must be
//               the answer of s > t.
//   layout      the GEMM's loads, LDS positions, operand reads and accumulator rows replayed on heap
//               blocks of exactly the kernel's sizes; the epilogue's words against a plain packing.
//   addressing  bits, bytes and words of a code with the pad bits, against a bit-by-bit restatement.
//   scratch     every region of encode_scratch inside the total, aligned, disjoint.
//   validation  every cause.
#include <algorithm>
#include <cfenv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../csrc/vdb_encode_plan.h"

using namespace vdb;

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                   \
            std::fprintf(stderr, "\n");                                          \
            if (++g_fail > 20) std::exit(1);                                     \
        }                                                                        \
    } while (0)

// ---- decision ---------------------------------------------------------------------------------------
template <typename F>
double canonical_sum(int D, F term) {
    double acc[64];
    const int np = (D + 255) / 256;
    for (int l = 0; l < 64; ++l) {
        acc[l] = 0.0;
        for (int m = 0; m < np; ++m)
            for (int j = 0; j < 4; ++j) {
                const int d = 4 * (64 * m + l) + j;
                acc[l] = acc[l] + (d < D ? term(d) : 0.0);
            }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        double nx[64];
        for (int l = 0; l < 64; ++l) nx[l] = acc[l] + acc[l ^ off];
        std::copy(nx, nx + 64, acc);
    }
    return acc[0];
}
double canonical_norm(const std::vector<float>& v) {
    return std::sqrt(canonical_sum((int)v.size(), [&](int d) { return (double)v[(size_t)d] * (double)v[(size_t)d]; }));
}
float ftz(float v) { return std::fabs(v) < 0x1p-126f ? 0.0f : v; }
// An fp32 dot product: order 0 = ascending, 1 = the kernel's K slots (pairs 4 apart), 2 = descending;
// flush: denormal operands, products and sums become zero.  The rounding mode is the caller's.
float dot32(const std::vector<float>& q, const std::vector<float>& x, int order, bool flush) {
    const int D = (int)q.size();
    volatile float acc = 0.0f;
    auto step = [&](int d) {
        if (d >= D) return;
        volatile float a = q[(size_t)d], b = x[(size_t)d];
        if (flush) a = ftz(a), b = ftz(b);
        volatile float p = a * b;
        if (flush) p = ftz(p);
        acc = acc + p;
        if (flush) acc = ftz(acc);
    };
    if (order == 0)
        for (int d = 0; d < D; ++d) step(d);
    else if (order == 2)
        for (int d = D - 1; d >= 0; --d) step(d);
    else
        for (int d0 = 0; d0 < D; d0 += 8)
            for (int e = 0; e < 4; ++e) step(d0 + e), step(d0 + 4 + e);
    return acc;
}

int64_t g_pairs = 0, g_undecided = 0;
void check_pair(const std::vector<float>& p, const std::vector<float>& x, std::mt19937_64& rng, bool count) {
    const int D = (int)p.size();
    const double pn = canonical_norm(p), xn = canonical_norm(x);
    const double s = canonical_sum(D, [&](int d) { return (double)p[(size_t)d] * (double)x[(size_t)d]; });
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> ts = {s, std::nextafter(s, inf), std::nextafter(s, -inf), s * (1 + 1e-12), s * (1 - 1e-12),
                              s * (1 + 1e-7), s * (1 - 1e-7), s * 1.001, s * 0.999, s + 1e-3, s - 1e-3, s + 1.0, s - 1.0,
                              0.0, -0.0, 1e-300, -1e-300, inf, -inf, 0.5, -0.5, 2.0 * s, 0.5 * s, -s};
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    for (int i = 0; i < 4; ++i) ts.push_back(s + std::fabs(s) * u(rng) * std::ldexp(1.0, -8 * i - 10));
    const int modes[] = {FE_TONEAREST, FE_TOWARDZERO};
    for (int mode : modes)
        for (int order = 0; order < 3; ++order)
            for (int flush = 0; flush < 2; ++flush) {
                std::fesetround(mode);
                const float a = dot32(p, x, order, flush != 0);
                std::fesetround(FE_TONEAREST);
                for (double t : ts) {
                    const int d = encode_decide(a, t, pn, xn, D);
                    const bool truth = s > t;
                    CHECK(d != kEncOne || truth, "D %d: one declared, s %.17g t %.17g a %.9g", D, s, t, (double)a);
                    CHECK(d != kEncZero || !truth, "D %d: zero declared, s %.17g t %.17g a %.9g", D, s, t, (double)a);
                    if (!std::isfinite(a)) CHECK(d == kEncUndecided, "a non-finite dot product was decided");
                }
                CHECK(encode_decide(a, s, pn, xn, D) != kEncOne, "a sum on its threshold is no one");
                if (count && mode == FE_TONEAREST && !flush) {  // the fast path is the common path: the zero threshold
                    ++g_pairs;
                    g_undecided += encode_decide(a, 0.0, pn, xn, D) == kEncUndecided;
                }
            }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(encode_decide(1.0f, nan, pn, xn, D) == kEncZero, "a NaN threshold");
    for (float bad : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()})
        for (double t : {-1.0, 0.0, 1e300})
            CHECK(encode_decide(bad, t, pn, xn, D) == kEncUndecided, "non-finite a decided at threshold %g", t);
    for (double badn : {inf, nan}) {
        CHECK(encode_decide(1.0f, 0.0, pn, badn, D) == kEncUndecided, "a vector with a non-finite norm was decided");
        CHECK(encode_decide(1.0f, 0.0, badn, xn, D) == kEncUndecided, "a projection row with a non-finite norm was decided");
    }
    CHECK(encode_decide(1e30f, 0.0, 1.0, 1.0, kEncMaxDim + 1) == kEncUndecided, "a dim past the constant's reach was decided");
}

void check_decisions() {
    std::mt19937_64 rng(20240607);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    for (int D : {1, 2, 7, 33, 260, 768, 2100}) {
        const int reps = D > 1000 ? 6 : 20;
        for (int rep = 0; rep < reps; ++rep)
            for (int kind = 0; kind < 7; ++kind) {
                std::vector<float> p((size_t)D), x((size_t)D);
                for (auto& v : p) v = nd(rng);
                for (auto& v : x) v = nd(rng);
                float sp = 1.0f, sx = 1.0f;
                switch (kind) {
                    case 1: sx = 0x1p-70f; break;                       // tiny rows
                    case 2: sx = 0x1p63f; break;                        // huge rows
                    case 3: sp = sx = 0x1p-70f; break;                  // products underflow
                    case 4: sp = sx = 0x1p63f; break;                   // sums overflow
                    case 5: std::fill(x.begin(), x.end(), 0.0f); break; // a zero row
                    case 6:                                             // small integers: the fp32 sum is exact
                        for (auto& v : p) v = std::nearbyint(2.0f * v);
                        for (auto& v : x) v = std::nearbyint(2.0f * v);
                        break;
                    default: break;
                }
                for (auto& v : p) v *= sp;
                for (auto& v : x) v *= sx;
                check_pair(p, x, rng, kind == 0 && D >= 33);
            }
    }
    // the derived share at the zero threshold is about 0.8 * 2.02 (D + 8) 2^-24 sqrt(D): under 1% at these dims
    CHECK(g_pairs > 0 && g_undecided * 50 <= g_pairs, "%lld of %lld ordinary pairs undecided at the zero threshold",
          (long long)g_undecided, (long long)g_pairs);
}

// ---- layout -----------------------------------------------------------------------------------------
void check_layout() {
    const int ST = kEncLdsStride, KC = kEncKC;
    CHECK(enc_lds_bytes() <= kEncLdsLimit, "LDS %lld bytes", (long long)enc_lds_bytes());
    CHECK(kEncLoads * 256 * 4 == kEncBM * KC && kEncBlockWords * 32 == kEncBN && 2 * kEncWaveM == kEncBM && 2 * kEncWaveN == kEncBN,
          "tile constants");
    int* sx = (int*)std::calloc((size_t)kEncBM * ST, sizeof(int));
    for (int i = 0; i < kEncLoads; ++i)
        for (int t = 0; t < 256; ++t) {
            const int r = enc_load_row(i, t), col = enc_load_col(t);
            CHECK(r >= 0 && r < kEncBM && col >= 0 && col + 4 <= KC && col % 4 == 0, "load (%d, %d) -> row %d col %d", i, t, r, col);
            for (int e = 0; e < 4; ++e) sx[r * ST + col + e] += 1 + r * KC + col + e;
        }
    for (int r = 0; r < kEncBM; ++r)
        for (int k = 0; k < KC; ++k) CHECK(sx[r * ST + k] == 1 + r * KC + k, "row %d float %d stored %d", r, k, sx[r * ST + k]);
    // operand reads: every float of a chunk feeds one K slot; 16 consecutive lanes cover 64 distinct banks
    for (int w = 0; w < 2; ++w)
        for (int tile = 0; tile < 2; ++tile) {
            std::vector<int> used((size_t)KC, 0);
            for (int s = 0; s < kEncSteps; ++s)
                for (int h = 0; h < 2; ++h) {
                    const int col = enc_operand_col(s, h);
                    CHECK(col % 4 == 0 && col + 4 <= KC, "operand col %d", col);
                    for (int e = 0; e < 4; ++e) used[(size_t)(col + e)]++;
                    for (int g = 0; g < 2; ++g) {
                        std::vector<int> bank(64, 0);
                        for (int c = 16 * g; c < 16 * g + 16; ++c) {
                            const int at = (w * kEncWaveM + tile * 32 + c) * ST + col;
                            CHECK(sx[at] && sx[at + 3], "read at %d", at);
                            for (int e = 0; e < 4; ++e) bank[(size_t)((at + e) % 64)]++;
                        }
                        for (int b = 0; b < 64; ++b) CHECK(bank[(size_t)b] == 1, "bank %d read %d times", b, bank[(size_t)b]);
                    }
                }
            for (int k = 0; k < KC; ++k) CHECK(used[(size_t)k] == 1, "float %d feeds %d slots", k, used[(size_t)k]);
        }
    std::free(sx);
    // the epilogue: the ballots of the 16 accumulator registers, taken by lanes enc_acc_row(v, 0 / 1),
    // give lane i < 32 the word of vector i whose bit c is the decision of (vector i, bit c)
    std::mt19937_64 rng(7);
    bool dec[32][32];
    for (auto& row : dec)
        for (bool& b : row) b = (rng() & 1) != 0;
    uint32_t word[64] = {};
    int taken[64] = {};
    for (int v = 0; v < 16; ++v) {
        uint64_t bal = 0;
        for (int lane = 0; lane < 64; ++lane)
            if (dec[enc_acc_row(v, lane >> 5)][lane & 31]) bal |= (uint64_t)1 << lane;
        const int i0 = enc_acc_row(v, 0), i1 = enc_acc_row(v, 1);
        CHECK(i0 >= 0 && i0 < 32 && i1 >= 0 && i1 < 32 && i0 != i1, "accumulator rows %d %d", i0, i1);
        word[i0] = (uint32_t)bal, taken[i0]++;
        word[i1] = (uint32_t)(bal >> 32), taken[i1]++;
    }
    for (int i = 0; i < 32; ++i) {
        uint32_t want = 0;
        for (int c = 0; c < 32; ++c) want |= (uint32_t)dec[i][c] << c;
        CHECK(taken[i] == 1 && word[i] == want, "vector %d: word %08x, want %08x, taken %d", i, word[i], want, taken[i]);
    }
    for (int Dp : {64, 128, 768, 2112}) CHECK(enc_k_chunks(Dp) * KC == Dp, "K chunks of %d", Dp);
    for (int64_t n : {(int64_t)1, (int64_t)128, (int64_t)129, kEncMaxVectors})
        CHECK(enc_row_blocks(n) * kEncBM >= n && (enc_row_blocks(n) - 1) * kEncBM < n, "row blocks of %lld", (long long)n);
    CHECK(enc_row_blocks(kEncMaxVectors) * enc_bit_blocks(kEncMaxBits) <= 0x7FFFFFFFll, "the largest grid");
}

// ---- addressing -------------------------------------------------------------------------------------
void check_addressing() {
    for (int n_bits = 1; n_bits <= kEncMaxBits; n_bits += (n_bits < 200 ? 1 : 97)) {
        const int nb = enc_bytes(n_bits), W = enc_words(n_bits), S = enc_word_stride(n_bits);
        CHECK(nb * 8 >= n_bits && (nb - 1) * 8 < n_bits && W * 32 >= n_bits && (W - 1) * 32 < n_bits, "sizes of %d bits", n_bits);
        CHECK(S >= W && S % 4 == 0 && S < W + 4 && enc_bit_blocks(n_bits) * kEncBlockWords == S, "stride %d of %d words", S, W);
        // a code of all ones through the words: exactly n_bits bits set, byte j bit j % 8, nothing past n_bytes
        uint8_t* out = (uint8_t*)std::calloc((size_t)nb, 1);
        int bytes = 0;
        for (int w = 0; w < W; ++w) {
            const uint32_t code = 0xFFFFFFFFu & enc_valid_bits(w, n_bits);
            const int k = enc_word_bytes(w, nb);
            CHECK(k >= 1 && k <= 4, "word %d of %d bytes holds %d", w, nb, k);
            for (int b = 0; b < k; ++b) out[4 * w + b] = (uint8_t)(code >> (8 * b));
            bytes += k;
        }
        CHECK(bytes == nb && enc_word_bytes(W, nb) == 0 && enc_valid_bits(W, n_bits) == 0u, "bytes written %d of %d", bytes, nb);
        for (int j = 0; j < nb * 8; ++j)
            CHECK(((out[j / 8] >> (j % 8)) & 1) == (j < n_bits ? 1 : 0), "%d bits: bit %d", n_bits, j);
        std::free(out);
    }
}

// ---- scratch ----------------------------------------------------------------------------------------
void check_scratch() {
    for (int64_t n : {(int64_t)1, (int64_t)129, (int64_t)100000})
        for (int dim : {1, 33, 768})
            for (int n_bits : {1, 20, 128, 129, 8192})
                for (int flags = 0; flags < 64; ++flags) {
                    const bool has_proj = flags & 1, has_thr = flags & 2, host = flags & 4, own = flags & 8, words = (flags & 16) && has_proj,
                               keep = flags & 32;
                    const int Dp = (dim + 63) / 64 * 64;
                    const int nbits = has_proj ? n_bits : dim;
                    const EncodeScratch s = encode_scratch(n, dim, Dp, nbits, has_proj, has_thr, host, own, words, keep);
                    CHECK(s.n_bytes == enc_bytes(nbits) && s.stride == enc_word_stride(nbits) && s.pad_bits % 32 == 0 &&
                              s.pad_bits >= nbits && s.pad_bits < nbits + 32, "sizes");
                    std::vector<std::pair<int64_t, int64_t>> regs;
                    if (host) {
                        if (own) regs.push_back({s.vec, n * dim * 4});
                        if (has_proj) regs.push_back({s.proj, (int64_t)nbits * dim * 4});
                        if (has_thr) regs.push_back({s.thr, (int64_t)nbits * 8});
                        for (const auto& r : regs) CHECK(r.first >= s.in0 && r.first + r.second <= s.in0 + s.in_bytes, "an argument outside the upload");
                    }
                    if (has_proj) {
                        regs.push_back({s.pw, (int64_t)s.pad_bits * Dp * 4});
                        regs.push_back({s.pn, (int64_t)s.pad_bits * 8});
                        if (own) regs.push_back({s.vw, n * Dp * 4}), regs.push_back({s.xn, n * 8});
                        if (words) regs.push_back({s.cw, n * s.stride * 4}), regs.push_back({s.uw, n * s.stride * 4});
                    }
                    if (host || keep) {
                        CHECK(s.out_bytes == n * s.n_bytes, "out bytes");
                        regs.push_back({s.out, s.out_bytes});
                    } else {
                        CHECK(s.out_bytes == 0, "no out region");
                    }
                    int64_t end = 0;
                    for (const auto& r : regs) {
                        CHECK(r.first % 256 == 0 && r.first >= end && r.first + r.second <= s.total, "region at %lld + %lld of %lld",
                              (long long)r.first, (long long)r.second, (long long)s.total);
                        end = r.first + r.second;
                    }
                }
}

// ---- validation -------------------------------------------------------------------------------------
void check_validation() {
    CHECK(encode_validate(5, 64, 128, true, 0, true) == kEncOk && encode_validate(0, 64, 64, false, 1, false) == kEncOk, "good calls");
    CHECK(encode_validate(5, 64, 128, true, 2, true) == kEncBadMem && encode_validate(5, 64, 128, true, -1, true) == kEncBadMem, "mem");
    CHECK(encode_validate(5, 64, 0, true, 0, true) == kEncBadBits && encode_validate(5, 64, kEncMaxBits + 1, true, 0, true) == kEncBadBits &&
              encode_validate(5, 64, kEncMaxBits, true, 0, true) == kEncOk && encode_validate(5, 64, 1, true, 0, true) == kEncOk, "bits");
    CHECK(encode_validate(5, 64, 63, false, 0, true) == kEncIdentityWidth && encode_validate(5, 64, 64, false, 0, true) == kEncOk, "identity");
    CHECK(encode_validate(-1, 64, 64, true, 0, true) == kEncBadCount && encode_validate(kEncMaxVectors + 1, 64, 64, true, 0, true) == kEncBadCount, "count");
    CHECK(encode_validate(5, 64, 64, true, 0, false) == kEncNullPointer, "pointers");
    for (int64_t knob = -1; knob <= 3; ++knob) CHECK(encode_knob_ok(knob) == (knob == 0 || knob == 2), "knob %lld", (long long)knob);
}

}  // namespace

int main() {
    check_decisions();
    check_layout();
    check_addressing();
    check_scratch();
    check_validation();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("encode plan ok: %lld ordinary pairs at the zero threshold, %lld undecided\n", (long long)g_pairs, (long long)g_undecided);
    return 0;
}
