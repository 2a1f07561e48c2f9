// variant_point_list_check.cpp -- KernelVariant::point_list (wost_variant.h; the point-list
// kernels of wost_solve_range_points) takes part in the comparison the handle's kernel cache
// makes: variants that differ only in point_list are different kernels, whatever the other
// fields are, so a list solve never runs the plain kernel's code or the other way round.
// Plain C++17, built with g++ from the header alone (tests/test_point_list_source.py);
// variant_check.cpp covers the other fields.
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
    KernelVariant base;
    CHECK(!base.point_list);   // the default: no list
    CHECK(base == base);
    const WalkTraits traits[] = {{}, {.neu = true, .src = true, .delta = true},
                                 {.neu = true, .src = true, .delta = true, .tree = true},
                                 {.neu = true, .src = true, .delta = true, .fix = true}};
    for (const WalkTraits& t : traits)
        for (int ns : {1, 3})
            for (int nk : {0, 2})
                for (int nm : {0, 2})
                    for (int pc : {0, 2}) {
                        KernelVariant a = base;
                        a.traits = t;
                        a.n_sources = ns;
                        a.n_wavenumbers = nk;
                        a.n_models = nm;
                        a.n_charges = pc;
                        KernelVariant b = a;
                        CHECK(a == b);
                        b.point_list = true;
                        CHECK(!(a == b) && !(b == a));
                        a.point_list = true;
                        CHECK(a == b);
                    }
    // point_list does not stand in for another flag
    KernelVariant l = base, r = base, d = base;
    l.point_list = true;
    r.record = true;
    d.dirichlet_tree = true;
    CHECK(!(l == r) && !(l == d) && !(r == d));
    std::printf("variant_point_list_check: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
