// combine_check.cpp -- the host restatement of the weighted channel combinations
// (dcrmontecarlo_amd/csrc/wost_combine.cpp) on exactly sized heap arrays, meant to be built
// with -fsanitize=address,undefined and run directly: a read past a partial block, a walk's
// channels or the weights is then an error. It also compares the rows with a second,
// plainly written restatement of the order (16 strided passes, then the halving tree) and a
// unit row with the channel's own sums.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "wost_combine.h"

namespace {

int failed = 0;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            ++failed;                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
        }                                                               \
    } while (0)

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
double uniform() {   // xorshift64*: (-1, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (double)((rng_state * 2685821657736338717ull) >> 11) / 4503599627370496.0 - 1.0;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// the order written out: thread t's walks pass by pass, then 256 -> 128 -> ... -> 1
void plain_rows(const float* val, int64_t lo, int64_t hi, int C, const double* w, double* s_out, double* q_out) {
    double s[256], q[256];
    for (int t = 0; t < 256; ++t) s[t] = q[t] = 0.0;
    const int64_t passes = (hi - lo + 255) / 256;
    for (int64_t r = 0; r < passes; ++r)
        for (int t = 0; t < 256; ++t) {
            const int64_t i = lo + r * 256 + t;
            if (i >= hi) continue;
            double v = 0.0;
            for (int c = 0; c < C; ++c) {
                if (w[c] == 0.0) continue;
                volatile double p = w[c] * (double)val[i * C + c];   // (a rounded product)
                v = v + p;
            }
            s[t] = s[t] + v;
            q[t] = std::fma(v, v, q[t]);
        }
    for (int h = 128; h > 0; h /= 2)
        for (int t = 0; t < h; ++t) {
            s[t] = s[t] + s[t + h];
            q[t] = q[t] + q[t + h];
        }
    *s_out = s[0];
    *q_out = q[0];
}

void check_shape(int C, int L, bool sparse) {
    // a full block, a 904-walk block, a block shorter than 256 walks, a 1-walk block
    const int64_t begin_v[5] = {0, 4096, 5000, 5100, 5101};
    const int64_t n = begin_v[4];
    std::unique_ptr<float[]> val(new float[(size_t)(n * C)]);
    std::unique_ptr<double[]> w(new double[(size_t)(L * C)]);
    std::unique_ptr<int64_t[]> begin(new int64_t[5]);
    std::unique_ptr<double[]> out(new double[(size_t)(4 * 2 * L)]);
    std::memcpy(begin.get(), begin_v, sizeof(begin_v));
    for (int64_t i = 0; i < n * C; ++i) val[(size_t)i] = (float)(3.0 * uniform());
    for (int i = 0; i < L * C; ++i) w[(size_t)i] = sparse && (i % 3) ? 0.0 : 2.0 * uniform();
    for (int c = 0; c < C && c < L; ++c) {   // row c < min(L, C) of every odd shape: a unit row
        if (!sparse) break;
        for (int k = 0; k < C; ++k) w[(size_t)(c * C + k)] = k == c ? 1.0 : 0.0;
    }
    wost::combine_blocks_host(val.get(), begin.get(), 4, C, w.get(), L, out.get());
    for (int b = 0; b < 4; ++b)
        for (int l = 0; l < L; ++l) {
            double s, q;
            plain_rows(val.get(), begin[b], begin[b + 1], C, w.get() + (size_t)l * C, &s, &q);
            CHECK(same_bits(s, out[(size_t)(b * 2 * L + 2 * l)]));
            CHECK(same_bits(q, out[(size_t)(b * 2 * L + 2 * l + 1)]));
        }
    if (sparse)   // unit row c: channel c's own sums
        for (int b = 0; b < 4; ++b)
            for (int c = 0; c < C && c < L; ++c) {
                const double one = 1.0;
                std::vector<float> ch((size_t)n);
                for (int64_t i = 0; i < n; ++i) ch[(size_t)i] = val[(size_t)(i * C + c)];
                double s, q;
                plain_rows(ch.data(), begin[b], begin[b + 1], 1, &one, &s, &q);
                CHECK(same_bits(s, out[(size_t)(b * 2 * L + 2 * c)]));
                CHECK(same_bits(q, out[(size_t)(b * 2 * L + 2 * c + 1)]));
            }
}

}  // namespace

int main() {
    const int Cs[4] = {1, 6, 15, 16}, Ls[3] = {1, 3, 16};
    for (int C : Cs)
        for (int L : Ls) {
            check_shape(C, L, false);
            check_shape(C, L, true);
        }
    // a zero weight next to a NaN and an infinity: skipped
    {
        std::unique_ptr<float[]> val(new float[6]{1.f, NAN, INFINITY, 2.f, NAN, -INFINITY});
        std::unique_ptr<double[]> w(new double[3]{1.0, 0.0, 0.0});
        std::unique_ptr<int64_t[]> begin(new int64_t[2]{0, 2});
        std::unique_ptr<double[]> out(new double[2]);
        wost::combine_blocks_host(val.get(), begin.get(), 1, 3, w.get(), 1, out.get());
        CHECK(out[0] == 3.0 && out[1] == 5.0);
    }
    // the weights' refusals
    {
        char msg[128];
        const double good[2] = {1.0, -2.0}, nan_w[2] = {1.0, NAN}, inf_w[2] = {INFINITY, 0.0};
        CHECK(wost::combine_check_weights(good, 1, 2, msg, sizeof(msg)) == 0);
        CHECK(wost::combine_check_weights(good, 0, 2, msg, sizeof(msg)) != 0);
        CHECK(wost::combine_check_weights(good, 17, 2, msg, sizeof(msg)) != 0);
        CHECK(wost::combine_check_weights(nullptr, 1, 2, msg, sizeof(msg)) != 0);
        CHECK(wost::combine_check_weights(nan_w, 1, 2, msg, sizeof(msg)) != 0);
        CHECK(wost::combine_check_weights(inf_w, 1, 2, msg, sizeof(msg)) != 0);
    }
    std::printf("combine_check: %d failed checks\n", failed);
    return failed ? 1 : 0;
}
