// variant_tally_check.cpp -- KernelVariant::tally (wost_variant.h; the tally kernels of
// wost_solve_range_tally) takes part in the comparison the handle's kernel cache makes:
// variants that differ only in tally are different kernels, whatever the other fields are,
// so a tally solve never runs the plain kernel's code or the other way round.
// Plain C++17, built from the header alone (tests/test_tally_host.py); variant_check.cpp and
// variant_point_list_check.cpp cover the other fields.
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
    CHECK(!base.tally);   // the default: no tally
    CHECK(base == base);
    const WalkTraits traits[] = {{.src = true, .fix = true},
                                 {.neu = true, .src = true, .delta = true, .fix = true},
                                 {.neu = true, .src = true, .delta = true, .tree = true, .fix = true}};
    for (const WalkTraits& t : traits)
        for (int block : {256, 512, 1024})
            for (int stage : {0, 1, 2})
                for (bool trig : {false, true})
                    for (bool dtree : {false, true}) {
                        KernelVariant a = base;
                        a.traits = t;
                        a.block = block;
                        a.tree_stage = stage;
                        a.exact_trig = trig;
                        a.dirichlet_tree = dtree;
                        KernelVariant b = a;
                        CHECK(a == b);
                        b.tally = true;
                        CHECK(!(a == b) && !(b == a));
                        a.tally = true;
                        CHECK(a == b);
                    }
    // tally does not stand in for another flag
    KernelVariant t = base, l = base, r = base, d = base;
    t.tally = true;
    l.point_list = true;
    r.record = true;
    d.dirichlet_tree = true;
    CHECK(!(t == l) && !(t == r) && !(t == d));
    std::printf("variant_tally_check: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
