// wost_variant.h -- which walk kernel: the traits of a walk (WalkTraits, the template
// arguments of wost_walk_kernel / walk_body) and everything else the source of a
// field-specialised kernel depends on besides the program (KernelVariant). Plain C++17,
// no HIP: tests/native/variant_check.cpp builds it with g++.
#pragma once

#include <string>

namespace wost {

struct WalkTraits {
    bool neu = false;     // a Neumann polyline
    bool src = false;     // a source term (the Green's sampler)
    bool delta = false;   // delta tracking: needs a source
    bool tree = false;    // the Neumann queries through the segment tree (else scans)
    bool fix = false;     // compat="fixed" estimators (wost_walk.h FIX)
    constexpr bool valid() const { return (!delta || src) && (!tree || neu); }   // 18 of the 32
};

inline bool operator==(const WalkTraits& a, const WalkTraits& b) {
    return a.neu == b.neu && a.src == b.src && a.delta == b.delta && a.tree == b.tree && a.fix == b.fix;
}

// The traits spelled out, e.g. "neumann+source+delta": the header line of a generated
// source (wost_jit.cpp) and messages. Distinct for every combination.
inline std::string traits_name(const WalkTraits& t) {
    std::string s = t.neu ? "neumann" : "dirichlet";
    if (t.src) s += "+source";
    if (t.delta) s += "+delta";
    if (t.tree) s += "+tree";
    if (t.fix) s += "+fixed";
    return s;
}

// A field-specialised kernel of one handle: everything its source depends on besides the
// program (wost_api.hip kernel_variant builds it, wost_jit.cpp jit_generate reads it).
struct KernelVariant {
    WalkTraits traits;
    bool record = false;             // the walk recorder compiled in (return_history)
    int n_sources = 1;               // NS: sources a walk scores (SLOT_F, SLOT_EXTRA..)
    int n_wavenumbers = 0;           // NK: attenuations a walk carries; 0: none set (no k2 read)
    int n_charges = 0;               // PC: point charges a walk scores (the count only: they are run-time data)
    int n_models = 0;                // NM: (sigma, alpha) models a walk scores (wost_set_models); 0: none set, 1: one
                                     // set (the program carries its fields: the kernel of a handle made with them)
    int block = 256;                 // threads per workgroup the kernel is launched with
    bool global_polylines = false;   // polylines not compiled in are read from global memory (wost_walk.h GL)
    int tree_stage = 0;              // tree kernels: 0 = the tree through L1/L2, 1 = its records in LDS
                                     // (WOST_TREE_STAGED), 2 = and the Neumann vertices (WOST_TREE_VSTAGED)
    bool exact_trig = true;          // wost_set_trig: correctly rounded directions
    bool dirichlet_tree = false;     // the Dirichlet distance through the Dirichlet polyline's segment tree
                                     // (poly_distance_tree; records and vertices through L1/L2, nothing staged)
    bool point_list = false;         // walk-range batches take their points from WalkArgs::point_list
                                     // (WOST_POINT_LIST; wost_solve_range_points)
    bool tally = false;              // the source samples' deposits go to WalkArgs::tally
                                     // (WOST_TALLY; wost_solve_range_tally)
    int tally_maps = 0;              // T: weighted channel maps a step deposits (WOST_TALLY_MAPS;
                                     // wost_solve_range_tally_channels); 0: none. Not `tally`: that one stays
                                     // the one-channel kernel
};

inline bool operator==(const KernelVariant& a, const KernelVariant& b) {
    return a.traits == b.traits && a.record == b.record && a.n_sources == b.n_sources &&
           a.n_wavenumbers == b.n_wavenumbers && a.n_charges == b.n_charges && a.n_models == b.n_models &&
           a.block == b.block &&
           a.global_polylines == b.global_polylines && a.tree_stage == b.tree_stage && a.exact_trig == b.exact_trig &&
           a.dirichlet_tree == b.dirichlet_tree && a.point_list == b.point_list &&
           a.tally == b.tally && a.tally_maps == b.tally_maps;
}

}  // namespace wost
