// TEST HARNESS -- which walk kernel (dcrmontecarlo_amd/csrc/wost_variant.h): the valid trait
// combinations and their spellings, KernelVariant's equality (the handle's kernel cache
// compares with it) and, built as HIP for the host, the walk kernels' LDS size
// (wost_walk.h walk_lds_bytes) against the values of the function it replaced.
// Built by tests/test_kernel_variant.py twice: with g++ from wost_variant.h alone (the header
// is HIP-free), and with hipcc --offload-host-only for the LDS part as well.
#include <cstddef>
#include <cstdio>
#include <set>
#include <string>

#if defined(__HIP__)
#include "../../dcrmontecarlo_amd/csrc/wost_walk.h"
#else
#include "../../dcrmontecarlo_amd/csrc/wost_variant.h"
#endif

using namespace wost;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

// The 18 kernels of the mode table this struct replaced (commit 9350d62, wost_kernels.hip
// WOST_FOR_MODE, in its order): neu, src, delta, tree, fix.
static const WalkTraits kValid[18] = {
    {false, false, false, false, false}, {false, true, false, false, false}, {true, false, false, false, false},
    {true, true, false, false, false},   {false, true, true, false, false},  {true, true, true, false, false},
    {true, false, false, true, false},   {true, true, false, true, false},   {true, true, true, true, false},
    {false, false, false, false, true},  {false, true, false, false, true},  {true, false, false, false, true},
    {true, true, false, false, true},    {false, true, true, false, true},   {true, true, true, false, true},
    {true, false, false, true, true},    {true, true, false, true, true},    {true, true, true, true, true},
};

static void check_traits() {
    std::set<std::string> names;
    int n_valid = 0;
    for (int m = 0; m < 32; ++m) {
        const WalkTraits t{(m & 1) != 0, (m & 2) != 0, (m & 4) != 0, (m & 8) != 0, (m & 16) != 0};
        bool listed = false;
        for (const WalkTraits& v : kValid) listed = listed || v == t;
        CHECK(t.valid() == listed);
        n_valid += t.valid() ? 1 : 0;
        names.insert(traits_name(t));
        for (int k = 0; k < 32; ++k) {
            const WalkTraits u{(k & 1) != 0, (k & 2) != 0, (k & 4) != 0, (k & 8) != 0, (k & 16) != 0};
            CHECK((t == u) == (m == k));
        }
    }
    CHECK(n_valid == 18);
    CHECK(names.size() == 32);   // every spelling distinct
    CHECK(traits_name(WalkTraits{true, true, true, false, false}) == "neumann+source+delta");
}

// Two variants that differ in one field are different kernels: every field, from several
// bases, to the values the packed integer key this replaced sat closest to its radices with.
static void check_variant_equality() {
    KernelVariant bases[3];
    bases[1].traits = WalkTraits{true, true, true, true, true};
    bases[1].record = true;
    bases[1].n_sources = 16;
    bases[1].n_wavenumbers = 16;
    bases[1].n_charges = 32;
    bases[1].block = 1024;
    bases[1].global_polylines = true;
    bases[1].tree_stage = 2;
    bases[1].exact_trig = false;
    bases[2].traits = WalkTraits{true, true, false, false, false};
    bases[2].n_sources = 2;
    bases[2].block = 64;
    bases[2].tree_stage = 1;
    for (const KernelVariant& b : bases) {
        CHECK(b == b);
        int n = 0;
        auto differs = [&](const KernelVariant& v) {
            CHECK(!(v == b) && !(b == v));
            ++n;
        };
        KernelVariant v;
        v = b; v.traits.neu = !b.traits.neu; differs(v);
        v = b; v.traits.src = !b.traits.src; differs(v);
        v = b; v.traits.delta = !b.traits.delta; differs(v);
        v = b; v.traits.tree = !b.traits.tree; differs(v);
        v = b; v.traits.fix = !b.traits.fix; differs(v);
        v = b; v.record = !b.record; differs(v);
        v = b; v.global_polylines = !b.global_polylines; differs(v);
        v = b; v.exact_trig = !b.exact_trig; differs(v);
        for (int x : {1, 2, 15, 16}) if (x != b.n_sources) { v = b; v.n_sources = x; differs(v); }
        for (int x : {0, 1, 15, 16}) if (x != b.n_wavenumbers) { v = b; v.n_wavenumbers = x; differs(v); }
        for (int x : {0, 1, 31, 32}) if (x != b.n_charges) { v = b; v.n_charges = x; differs(v); }
        for (int x : {64, 256, 512, 960, 1024}) if (x != b.block) { v = b; v.block = x; differs(v); }
        for (int x : {0, 1, 2}) if (x != b.tree_stage) { v = b; v.tree_stage = x; differs(v); }
        CHECK(n >= 8 + 3 + 3 + 3 + 4 + 2);
    }
}

#if defined(__HIP__)
// walk_lds_bytes of commit 9350d62 (wost_internal.h) over: the 18 traits of kValid x
// (nd, nn) in {(5, 0), (5, 2), (300, 10001)} x const_d in {0, 1} x global_polylines in {0, 1}
// and, for the tree traits, x tree_lds in {0, 85} x tree_verts in {0, 10001} x block in
// {256, 1024}; the last varies fastest. Printed by that commit's function.
static const size_t kLdsExpected[] = {
    48, 0, 0, 0, 48, 0, 0, 0, 2400, 0, 0, 0,
    16448, 16400, 16400, 16400, 16448, 16400, 16400, 16400, 18800, 16400, 16400, 16400,
    48, 0, 0, 0, 80, 0, 32, 0, 122416, 0, 120016, 0,
    16448, 16400, 16400, 16400, 16480, 16400, 16432, 16400, 138816, 16400, 136416, 16400,
    20528, 20480, 20480, 20480, 20528, 20480, 20480, 20480, 22880, 20480, 20480, 20480,
    20528, 20480, 20480, 20480, 20560, 20480, 20512, 20480, 142896, 20480, 140496, 20480,
    3120, 12336, 83136, 92352, 14000, 23216, 94016, 103232, 3072, 12288, 83088, 92304,
    13952, 23168, 93968, 103184, 3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184,
    3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184, 3120, 12336, 83136, 92352,
    14000, 23216, 94016, 103232, 3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184,
    3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184, 3072, 12288, 83088, 92304,
    13952, 23168, 93968, 103184, 5472, 14688, 85488, 94704, 16352, 25568, 96368, 105584,
    3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184, 3072, 12288, 83088, 92304,
    13952, 23168, 93968, 103184, 3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184,
    19520, 28736, 99536, 108752, 30400, 39616, 110416, 119632, 19472, 28688, 99488, 108704,
    30352, 39568, 110368, 119584, 19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584,
    19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584, 19520, 28736, 99536, 108752,
    30400, 39616, 110416, 119632, 19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584,
    19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584, 19472, 28688, 99488, 108704,
    30352, 39568, 110368, 119584, 21872, 31088, 101888, 111104, 32752, 41968, 112768, 121984,
    19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584, 19472, 28688, 99488, 108704,
    30352, 39568, 110368, 119584, 19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584,
    23600, 32816, 103616, 112832, 34480, 43696, 114496, 123712, 23552, 32768, 103568, 112784,
    34432, 43648, 114448, 123664, 23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664,
    23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664, 23600, 32816, 103616, 112832,
    34480, 43696, 114496, 123712, 23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664,
    23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664, 23552, 32768, 103568, 112784,
    34432, 43648, 114448, 123664, 25952, 35168, 105968, 115184, 36832, 46048, 116848, 126064,
    23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664, 23552, 32768, 103568, 112784,
    34432, 43648, 114448, 123664, 23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664,
    48, 0, 0, 0, 48, 0, 0, 0, 2400, 0, 0, 0,
    16448, 16400, 16400, 16400, 16448, 16400, 16400, 16400, 18800, 16400, 16400, 16400,
    48, 0, 0, 0, 80, 0, 32, 0, 122416, 0, 120016, 0,
    16448, 16400, 16400, 16400, 16480, 16400, 16432, 16400, 138816, 16400, 136416, 16400,
    20528, 20480, 20480, 20480, 20528, 20480, 20480, 20480, 22880, 20480, 20480, 20480,
    20528, 20480, 20480, 20480, 20560, 20480, 20512, 20480, 142896, 20480, 140496, 20480,
    3120, 12336, 83136, 92352, 14000, 23216, 94016, 103232, 3072, 12288, 83088, 92304,
    13952, 23168, 93968, 103184, 3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184,
    3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184, 3120, 12336, 83136, 92352,
    14000, 23216, 94016, 103232, 3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184,
    3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184, 3072, 12288, 83088, 92304,
    13952, 23168, 93968, 103184, 5472, 14688, 85488, 94704, 16352, 25568, 96368, 105584,
    3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184, 3072, 12288, 83088, 92304,
    13952, 23168, 93968, 103184, 3072, 12288, 83088, 92304, 13952, 23168, 93968, 103184,
    19520, 28736, 99536, 108752, 30400, 39616, 110416, 119632, 19472, 28688, 99488, 108704,
    30352, 39568, 110368, 119584, 19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584,
    19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584, 19520, 28736, 99536, 108752,
    30400, 39616, 110416, 119632, 19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584,
    19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584, 19472, 28688, 99488, 108704,
    30352, 39568, 110368, 119584, 21872, 31088, 101888, 111104, 32752, 41968, 112768, 121984,
    19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584, 19472, 28688, 99488, 108704,
    30352, 39568, 110368, 119584, 19472, 28688, 99488, 108704, 30352, 39568, 110368, 119584,
    23600, 32816, 103616, 112832, 34480, 43696, 114496, 123712, 23552, 32768, 103568, 112784,
    34432, 43648, 114448, 123664, 23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664,
    23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664, 23600, 32816, 103616, 112832,
    34480, 43696, 114496, 123712, 23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664,
    23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664, 23552, 32768, 103568, 112784,
    34432, 43648, 114448, 123664, 25952, 35168, 105968, 115184, 36832, 46048, 116848, 126064,
    23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664, 23552, 32768, 103568, 112784,
    34432, 43648, 114448, 123664, 23552, 32768, 103568, 112784, 34432, 43648, 114448, 123664,
};

static void check_lds() {
    const int shapes[3][2] = {{5, 0}, {5, 2}, {300, 10001}};
    size_t i = 0;
    const size_t n = sizeof(kLdsExpected) / sizeof(kLdsExpected[0]);
    auto expect = [&](const WalkLds& k) {
        if (i >= n || walk_lds_bytes(k) != kLdsExpected[i]) {
            std::fprintf(stderr, "walk_lds_bytes: value %zu is %zu, expected %zu (%s, nd %d, nn %d)\n", i,
                         walk_lds_bytes(k), i < n ? kLdsExpected[i] : (size_t)0, traits_name(k.traits).c_str(), k.nd, k.nn);
            ++fails;
        }
        ++i;
    };
    for (const WalkTraits& t : kValid)
        for (const auto& s : shapes)
            for (int cd = 0; cd < 2; ++cd)
                for (int gp = 0; gp < 2; ++gp) {
                    WalkLds k{.traits = t, .nd = s[0], .nn = s[1], .const_d = cd != 0, .global_polylines = gp != 0};
                    if (!t.tree) {
                        expect(k);
                        continue;
                    }
                    for (int tl : {0, 85})
                        for (int tv : {0, 10001})
                            for (int blk : {256, 1024}) {
                                k.tree_lds = tl;
                                k.tree_verts = tv;
                                k.block = blk;
                                expect(k);
                            }
                }
    CHECK(i == n && n == 12 * 12 + 6 * 12 * 8);
}
#endif

int main() {
    check_traits();
    check_variant_equality();
#if defined(__HIP__)
    check_lds();
    std::printf("variant_check (with the LDS size): %d failed checks\n", fails);
#endif
    std::printf("variant_check: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
