// TEST HARNESS -- host build of wost_device.h and wost_tree.cpp: the Dirichlet distance
// through the segment tree (poly_distance_tree) against the full scan (poly_distance), bit
// for bit, on caller-supplied polylines and points; the tree's usability rule; and the
// KernelVariant field that selects it. Built by tests/test_dirichlet_tree.py.
#include <cstring>
#include <vector>

#define WOST_TREE_STATS 1

#include "../../dcrmontecarlo_amd/csrc/wost_device.h"
#include "../../dcrmontecarlo_amd/csrc/wost_tree.h"
#include "../../dcrmontecarlo_amd/csrc/wost_variant.h"

using namespace wost;

#if !defined(__HIP_DEVICE_COMPILE__)
long wost::g_tree_stats[4];
#endif

namespace {
bool same(float a, float b) {
    uint32_t x, y;
    std::memcpy(&x, &a, 4);
    std::memcpy(&y, &b, 4);
    return x == y || (a != a && b != b);
}
}  // namespace

extern "C" {

int dtree_usable(const float* xy, int nv) { return dirichlet_tree_usable(xy, nv) ? 1 : 0; }

// Queries pts[2 * n] against the polyline xy[2 * nv] with `leaf` segments per leaf.
// out[0] = mismatches between the tree and the scan, out[1] = record visits, out[2] = leaf
// visits of the tree queries, out[3] = the tree's leaf count; first_bad (may be null): the
// index of the first mismatching query, or -1. Returns 1 when no tree can be built.
int dtree_check(const float* xy, int nv, int leaf, const float* pts, long n, long* out, long* first_bad) {
    SegmentTreeHost th;
    if (!build_segment_tree(xy, nv, leaf, &th)) return 1;
    const SegTree t{reinterpret_cast<const float4*>(th.rec.data()), reinterpret_cast<const float2*>(xy), nv,
                    th.first_leaf, th.depth, th.leaf, th.tol, th.kmax};
    const float2* v = reinterpret_cast<const float2*>(xy);
    long bad = 0;
    if (first_bad) *first_bad = -1;
#if !defined(__HIP_DEVICE_COMPILE__)
    g_tree_stats[0] = g_tree_stats[1] = 0;
#endif
    for (long i = 0; i < n; ++i) {
        const float px = pts[2 * i], py = pts[2 * i + 1];
        if (!same(poly_distance(v, nv, px, py), poly_distance_tree(t, px, py))) {
            if (bad == 0 && first_bad) *first_bad = i;
            ++bad;
        }
    }
    out[0] = bad;
#if !defined(__HIP_DEVICE_COMPILE__)
    out[1] = g_tree_stats[0];
    out[2] = g_tree_stats[1];
#endif
    out[3] = (nv - 1 + th.leaf - 1) / th.leaf;
    return 0;
}

// Two kernel variants that differ only in dirichlet_tree: 1 when they compare unequal and
// each equals itself.
int dtree_variant_differs() {
    KernelVariant a, b;
    b.dirichlet_tree = true;
    return (!(a == b) && a == a && b == b) ? 1 : 0;
}

}  // extern "C"
