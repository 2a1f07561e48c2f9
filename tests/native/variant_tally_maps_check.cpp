// variant_tally_maps_check.cpp -- KernelVariant::tally_maps (wost_variant.h; the channel-map
// kernels of wost_solve_range_tally_channels) takes part in the comparison the handle's kernel
// cache makes: variants that differ only in the number of maps are different kernels, whatever
// the channel counts are, and tally_maps does not stand in for tally (the one-channel kernel)
// or the other way round.
// Plain C++17, built from the header alone (tests/test_tally_channels_host.py);
// variant_tally_check.cpp covers tally itself.
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
    CHECK(base.tally_maps == 0);   // the default: no maps
    CHECK(base == base);
    const WalkTraits traits[] = {{.neu = true, .src = true, .delta = true, .fix = true},
                                 {.neu = true, .src = true, .delta = true, .tree = true, .fix = true}};
    for (const WalkTraits& t : traits)
        for (int nk : {0, 1, 3, 8})
            for (int nm : {0, 2})
                for (int block : {256, 1024})
                    for (int maps = 1; maps <= 4; ++maps) {
                        KernelVariant a = base;
                        a.traits = t;
                        a.n_wavenumbers = nk;
                        a.n_models = nm;
                        a.block = block;
                        KernelVariant b = a;
                        CHECK(a == b);
                        b.tally_maps = maps;
                        CHECK(!(a == b) && !(b == a));
                        a.tally_maps = maps;
                        CHECK(a == b);
                        a.tally_maps = maps % 4 + 1;   // another count of maps: another kernel
                        CHECK(!(a == b) && !(b == a));
                    }
    // one map is not the one-channel tally, nor any other flag
    KernelVariant m = base, t = base, l = base, r = base;
    m.tally_maps = 1;
    t.tally = true;
    l.point_list = true;
    r.record = true;
    CHECK(!(m == t) && !(t == m) && !(m == l) && !(m == r));
    CHECK(!m.tally && t.tally_maps == 0);
    std::printf("variant_tally_maps_check: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
