// wost_launch.h -- the launch plan of a solve: which walks its blocks cover, how they are
// batched into launches, and each launch's shape (grid, static chunk, dequeue size).
//
// Pure integer functions of the call, the kernel's occupancy and the handle's options: no
// HIP here, so tests/native/launch_check.cpp drives all of it on the host (the multi-batch
// paths included, which a solve reaches only above 2^26 walks). wost_api.hip solve_impl
// executes the plan.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "wost.h"
#include "wost_options.h"

namespace wost {

// The blocks and walks a solve covers. Block mode: blocks [block_begin, block_end) of the
// n_points * nbpp blocks of the whole solve, point-major. Walk-range mode (wost_solve_range;
// walk_begin/walk_end != 0/W): walks [walk_begin, walk_end) of every point; blocks are then
// (point, block of the range), point-major, and the block range given is ignored.
// Point list (wost_solve_range_points; point_ids != nullptr): always walk-range mode, [0, W)
// included, over the n_sel listed points only. The plan's "points" are then list positions:
// blocks are [n_sel][nbr], point_of() and a batch's p0 / range_point0 index the list, and the
// kernel (WOST_POINT_LIST) takes the point itself from the list.
struct SolveRanges {
    int64_t n_points = 0, W = 0;
    int64_t nbpp = 0;                         // blocks per point of the whole solve
    bool range = false;
    int64_t walk_begin = 0, walk_end = 0;
    int64_t Wr = 0;                           // walks per point solved
    int64_t nbr = 0;                          // blocks per point solved
    int64_t block_begin = 0, block_end = 0;   // resolved (range mode: [0, n_points * nbr))
    int64_t nblk = 0;
    int64_t walks_total = 0;
    const int32_t* point_ids = nullptr;       // the point list: n_sel strictly ascending ids in [0, n_points)
    int64_t n_sel = 0;
    // the points the plan covers: list positions with a list, else every point
    int64_t plan_points() const { return point_ids ? n_sel : n_points; }

    // block -> global walk range (block mode)
    int64_t blk_begin(int64_t j) const { return (j / nbpp) * W + (j % nbpp) * WOST_BLOCK_WALKS; }
    int64_t blk_end(int64_t j) const {
        const int64_t p = j / nbpp, b = j % nbpp, e = (b + 1) * WOST_BLOCK_WALKS;
        return p * W + (e < W ? e : W);
    }
    // the point of block j (either mode)
    int64_t point_of(int64_t j) const { return j / (range ? nbr : nbpp); }
};

// Resolves and validates the ranges of a solve of n_points >= 0 points with W >= 1 walks
// each (walk_end < 0: W). point_ids: the point list of n_sel ids, or null. Returns WOST_OK,
// or WOST_ERR_INVALID_ARG with the message in msg (a list that is empty, not strictly
// ascending or that names a point outside [0, n_points) among them).
int plan_ranges(int64_t n_points, int64_t W, int64_t block_begin, int64_t block_end, int64_t walk_begin,
                int64_t walk_end, SolveRanges* out, char* msg, size_t msg_cap, const int32_t* point_ids = nullptr,
                int64_t n_sel = 0);

// One launch's blocks [j, j2) and the WalkArgs fields that place its walks.
struct Batch {
    std::vector<int64_t> begins;   // the blocks' first local walks, then count
    int64_t count = 0;             // walks of the launch
    int64_t j2 = 0;                // the next batch's first block
    int64_t wid_begin = 0, base_pid = 0;
    uint32_t base_off = 0;
    int32_t small32 = 0;
    int64_t range_walks = 0, range_offset = 0, range_point0 = 0;
    double inv_range_walks = 0.0;
};

// The batch that starts at block j: whole blocks (range mode: whole points' ranges; with a
// point list, whole list positions' ranges) of at most batch_limit walks together. false:
// block j alone exceeds batch_limit.
bool next_batch(const SolveRanges& r, int64_t j, int64_t batch_limit, Batch* b);

struct LaunchIn {
    bool short_walks = false;   // no Neumann boundary
    bool tree = false;          // a segment-tree kernel
    int64_t count = 0;          // walks of the launch
    int block = 256;            // threads per workgroup
    int blocks_per_cu = 1;      // the kernel's occupancy
    int num_cus = 1;
    const Options* opt = nullptr;   // chunk0, chunk_min, chunk_max, adaptive_chunk, grid_blocks_per_cu
    bool clock_is_100mhz = true;    // the device wall clock the waves' rate floor assumes
};

struct LaunchShape {
    int64_t bpc = 0;          // workgroups per CU
    int grid = 0;
    int64_t waves = 0;
    int64_t chunk0 = 0;       // static first chunk of walks per wave
    int chunk = 0;            // the host's dequeue size
    int64_t queue_base = 0;   // the counter's dequeues start here (waves * chunk0)
    uint32_t chunk_share = 0; // adaptive dequeues' cap (0: not adaptive)
    bool adaptive = false;
};

LaunchShape launch_shape(const LaunchIn& in);

}  // namespace wost
