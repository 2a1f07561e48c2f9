// variant_models_check.cpp -- KernelVariant::n_models (wost_variant.h, model batching) takes
// part in the comparison the handle's kernel cache makes: variants that differ only in
// n_models are different kernels. 0 (no model set) and 1 (one set: the program carries its
// fields) generate the same source but are distinct states of a handle, and every count from
// 2 up is a kernel of its own. Plain C++17, built with g++ from the header alone
// (tests/test_models_source.py); variant_check.cpp covers the other fields.
#include <cstdio>

#include "../../dcrmontecarlo_amd/csrc/wost_variant.h"

static int fails = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            ++fails;                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
        }                                                                \
    } while (0)

int main() {
    using wost::KernelVariant;
    using wost::WalkTraits;
    const WalkTraits delta{.neu = true, .src = true, .delta = true};
    KernelVariant base;
    base.traits = delta;
    CHECK(base.n_models == 0);   // the default: none set
    CHECK(base == base);
    const int counts[] = {0, 1, 2, 3, 4, 8, 16};
    for (int a : counts)
        for (int b : counts) {
            KernelVariant va = base, vb = base;
            va.n_models = a;
            vb.n_models = b;
            CHECK((va == vb) == (a == b));
            // ... whatever the other channel counts are
            va.n_sources = vb.n_sources = 2;
            va.n_wavenumbers = vb.n_wavenumbers = 2;
            CHECK((va == vb) == (a == b));
        }
    // n_models does not stand in for another count
    KernelVariant m2 = base, k2 = base, s2 = base;
    m2.n_models = 2;
    k2.n_wavenumbers = 2;
    s2.n_sources = 2;
    CHECK(!(m2 == k2) && !(m2 == s2) && !(k2 == s2));
    std::printf("variant_models_check: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
