// wost_internal.h -- launch interface between libwost's host code (wost_api.hip,
// wost_jit.cpp) and its gfx950 kernels (wost_kernels.hip). Not part of the
// public ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wost_walk.h"

namespace wost {

// floats of the sampler / G_norm table buffer (WalkArgs::table); compat="fixed" delta
// tracking appends the corrected screened sampler's [kFixRows][kFixCols] nodes
inline size_t table_floats(bool delta, bool fixed_delta = false) {
    return (size_t)kSamplerFloatsPadded + (delta ? 4 * (size_t)kGnormCells : 0) +
           (fixed_delta ? (size_t)kFixTableFloats : 0);
}


// alpha at the query points with the interpreted fields (delta tracking)
hipError_t launch_point_alpha(const char* prog, const float2* pts, int64_t n, float* out, hipStream_t s);

// precompiled (interpreted-field) walk kernels: one instantiation per valid WalkTraits
// (wost_variant.h), hipErrorInvalidValue for the rest
hipError_t walk_occupancy(const WalkTraits& t, int nd, int nn, int* blocks_per_cu);
hipError_t launch_walk(const WalkTraits& t, const WalkArgs& a, int grid, hipStream_t s);

// Per-block reduction: block b covers local walks [begin[b], begin[b+1]).
// ns values per walk (multi-source: val[walk * ns + k]); rows of 2*ns+1 doubles
// (sum_k, sumsq_k for each k, then steps).
// ctl (may be null): the walk launch's control words (wost_walk.h kCtlWords), the queue
// head reset for the next walk launch. lstats (may be null): the solve's launch statistics
// [8] (wost_kernels.hip reduce_wave_stats) from the walk launch's n_waves per-wave records
// and its walks' step counts; first_batch: the solve's first launch.
hipError_t launch_block_reduce(const float* val, const uint32_t* steps, const int64_t* begin,
                               int64_t nblocks, int ns, double* out, unsigned long long* ctl,
                               hipStream_t s, int64_t n_waves = 0, unsigned long long* lstats = nullptr,
                               int first_batch = 1);

// Weighted channel combinations (wost_combine.h): rows of 2L+1 doubles (sum_l, sumsq_l for
// each of the L = n_combinations rows of weights [L][n_channels], a device array, then the
// block's steps) of the same blocks, in wost_block_reduce's summation order.
hipError_t launch_block_combine(const float* val, const uint32_t* steps, const int64_t* begin, int64_t nblocks,
                                int n_channels, const double* weights, int n_combinations, double* out,
                                hipStream_t s);

hipError_t launch_geometry_query(int op, const float2* verts, int nv, const float2* pts,
                                 const float2* dirs, const float* radii, int64_t n,
                                 float* out_f, uint8_t* out_mask, hipStream_t s);
// op 0 / 2 / 4 through the segment tree (records rec of SegmentTreeHost), one query per lane
hipError_t launch_geometry_tree_query(int op, const float2* verts, int nv, const float4* rec, int first_leaf,
                                      int depth, int leaf, float tol, float kmax, const float2* pts,
                                      const float2* dirs, const float* radii, int64_t n, float* out_f,
                                      hipStream_t s);

hipError_t launch_eval_field(const char* prog, int which, const float2* pts, int64_t n,
                             float4* out, hipStream_t s);

}  // namespace wost
