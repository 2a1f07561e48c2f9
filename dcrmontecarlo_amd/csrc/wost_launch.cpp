// wost_launch.cpp -- the launch plan of a solve (wost_launch.h).
#include "wost_launch.h"

#include <algorithm>
#include <cstdio>

namespace wost {

int plan_ranges(int64_t n_points, int64_t W, int64_t block_begin, int64_t block_end, int64_t walk_begin,
                int64_t walk_end, SolveRanges* out, char* msg, size_t msg_cap, const int32_t* point_ids,
                int64_t n_sel) {
    SolveRanges r;
    r.n_points = n_points;
    r.W = W;
    r.nbpp = (W + WOST_BLOCK_WALKS - 1) / WOST_BLOCK_WALKS;
    const int64_t nb_total = n_points * r.nbpp;
    if (walk_end < 0) walk_end = W;
    r.range = walk_begin != 0 || walk_end != W || point_ids != nullptr;
    if (point_ids) {
        if (n_sel < 1) {
            std::snprintf(msg, msg_cap, "a point list needs at least one id (got %lld)", (long long)n_sel);
            return WOST_ERR_INVALID_ARG;
        }
        for (int64_t i = 0; i < n_sel; ++i)
            if (point_ids[i] < 0 || point_ids[i] >= n_points || (i > 0 && point_ids[i] <= point_ids[i - 1])) {
                std::snprintf(msg, msg_cap,
                              "point list entry %lld is %d: the ids must be strictly ascending within [0, %lld)",
                              (long long)i, (int)point_ids[i], (long long)n_points);
                return WOST_ERR_INVALID_ARG;
            }
        r.point_ids = point_ids;
        r.n_sel = n_sel;
    }
    if (r.range && (walk_begin < 0 || walk_end <= walk_begin || walk_end > W || walk_begin % WOST_BLOCK_WALKS != 0 ||
                    (walk_end % WOST_BLOCK_WALKS != 0 && walk_end != W))) {
        std::snprintf(msg, msg_cap,
                      "walk range [%lld,%lld) of %lld walks must be non-empty with block-aligned ends (multiples of %d, "
                      "or the end at W)", (long long)walk_begin, (long long)walk_end, (long long)W, WOST_BLOCK_WALKS);
        return WOST_ERR_INVALID_ARG;
    }
    r.walk_begin = walk_begin;
    r.walk_end = walk_end;
    r.Wr = walk_end - walk_begin;
    r.nbr = (r.Wr + WOST_BLOCK_WALKS - 1) / WOST_BLOCK_WALKS;
    if (r.range) {
        block_begin = 0;
        block_end = r.plan_points() * r.nbr;
    } else if (block_begin < 0 || block_end < block_begin || block_end > nb_total) {
        std::snprintf(msg, msg_cap, "block range [%lld,%lld) outside [0,%lld)", (long long)block_begin,
                      (long long)block_end, (long long)nb_total);
        return WOST_ERR_INVALID_ARG;
    }
    r.block_begin = block_begin;
    r.block_end = block_end;
    r.nblk = block_end - block_begin;
    r.walks_total = r.nblk == 0 ? 0 : r.range ? r.plan_points() * r.Wr : r.blk_end(block_end - 1) - r.blk_begin(block_begin);
    *out = r;
    return WOST_OK;
}

bool next_batch(const SolveRanges& r, int64_t j, int64_t batch_limit, Batch* b) {
    std::vector<int64_t>& begins = b->begins;
    begins.clear();
    int64_t j2 = j, count = 0;
    b->wid_begin = b->base_pid = 0;
    b->base_off = 0;
    b->small32 = 0;
    b->range_walks = b->range_offset = b->range_point0 = 0;
    b->inv_range_walks = 0.0;
    if (r.range) {
        // whole points' ranges: local walk l is walk walk_begin + l % Wr of point p0 + l / Wr
        // (with a point list: of the point at list position p0 + l / Wr)
        if (r.Wr > batch_limit) return false;
        const int64_t p0 = j / r.nbr;
        const int64_t p1 = std::min<int64_t>(r.plan_points(), p0 + std::max<int64_t>(1, batch_limit / r.Wr));
        for (int64_t p = p0; p < p1; ++p)
            for (int64_t k = 0; k < r.nbr; ++k) begins.push_back((p - p0) * r.Wr + k * WOST_BLOCK_WALKS);
        count = (p1 - p0) * r.Wr;
        j2 = p1 * r.nbr;
        b->range_walks = r.Wr;
        b->range_offset = r.walk_begin;
        b->range_point0 = p0;
        b->inv_range_walks = 1.0 / (double)r.Wr;
    } else {
        // gather whole blocks into a batch of at most batch_limit walks
        const int64_t wb = r.blk_begin(j);
        while (j2 < r.block_end && r.blk_end(j2) - wb <= batch_limit) {
            begins.push_back(r.blk_begin(j2) - wb);
            ++j2;
        }
        if (j2 == j) return false;
        count = r.blk_end(j2 - 1) - wb;
        b->wid_begin = wb;
        b->base_pid = wb / r.W;
        const int64_t off = wb - b->base_pid * r.W;
        b->base_off = (uint32_t)std::min<int64_t>(off, INT32_MAX);
        b->small32 = (r.W < (int64_t(1) << 31) && off + count < (int64_t(1) << 31)) ? 1 : 0;
    }
    begins.push_back(count);
    b->count = count;
    b->j2 = j2;
    return true;
}

LaunchShape launch_shape(const LaunchIn& in) {
    const Options& O = *in.opt;
    const int64_t count = in.count;
    const int block = in.block;
    LaunchShape s;
    // The launch's shape is a function of this call alone (never of an earlier solve:
    // the reference calls solve() once per script, so the first call is the one that
    // counts). Walks without a Neumann boundary (Laplace, Poisson, delta tracking on a
    // Dirichlet-only domain) are short (13-17 steps); those with one (C3's circle, the
    // DCR scenarios, C5) run 17-208.
    const bool short_walks = in.short_walks;
    // Resident workgroups: few short walks per lane (C2: 640k walks, ~1.2 per lane at
    // full occupancy) leave the launch as long as its longest walk chains, whose steps
    // run faster with fewer waves per SIMD: ~2 walks per lane, at least 2 workgroups per
    // CU (C2: 8 -> 2 per CU took 0.21 -> 0.18 ms, profiles/r05_ab/grid_c2/; with the
    // all-static first chunk below 4 per CU beat 2: 0.127 -> 0.110 ms, and 8 stays best
    // at 4x C2's walks, profiles/r06_ab/r06s37/)
    int64_t bpc = in.blocks_per_cu;
    if (short_walks && bpc > 2)
        bpc = std::max<int64_t>(2, std::min<int64_t>(bpc, count / ((int64_t)in.num_cus * block * 2)));
    if (O.grid_blocks_per_cu > 0)
        bpc = std::max<int64_t>(1, std::min<int64_t>(in.blocks_per_cu, O.grid_blocks_per_cu));
    const int64_t max_grid = bpc * in.num_cus;
    const int64_t want = (count + block - 1) / block;
    const int grid = (int)std::max<int64_t>(1, std::min(max_grid, want));
    const int64_t waves = (int64_t)grid * (block / 64);
    // The work queue (wost_walk.h): a static chunk of walks per wave (below), then
    // chunks of the rest from one global counter. Every dequeue of that
    // counter serialises at its address (~11-16 ns): C2's 640k walks took 34k dequeues of
    // 19 walks, all waves hitting the counter at the launch's start, 0.60 ms for 47 us of
    // work (profiles/r05_ab/queue_chunk/, queue_static/).
    // - static chunks except for the segment-tree kernels: their long walks lose by them
    //   when launches run concurrently (the C5 survey's handle pairs: a late-starting
    //   wave still owns its 64 walks; 1.38e10 -> 1.34e10, profiles/r05_ab/queue_c5/);
    // - the dequeue's size: max(floor, min(cap, count / (waves * 4))), floor 64 for short
    //   walks and 1 otherwise; cap 64 walks (one per lane), 16 for the segment-tree
    //   kernels' long walks (C5: 208 steps; a wave's last chunk is work no other wave can
    //   take: the survey 1.42e10 -> 1.46e10, profiles/r05_ab/chunk_cap/); each wave then
    //   raises it to the floor its measured walk rate needs (WalkArgs::adaptive).
    // - the static first chunk: at most one walk per lane (64) for long walks; for short
    //   ones every walk of the launch when that is at most 6 per lane (no wave dequeues at
    //   all), else 4 per lane (256). C2's 640k walks: 313 per wave, kernel 0.176 ->
    //   0.129 ms; 12.8M walks of Laplace / Poisson: 256, +12% / +6% (64 took one walk
    //   per lane and left ~8k dequeues serialised at the counter; profiles/r06_ab/r06s3[12]/)
    const int64_t per_wave = (count + waves - 1) / waves;
    int64_t chunk0 = in.tree          ? 0
                     : !short_walks   ? std::min<int64_t>(64, per_wave)
                     : per_wave <= 384 ? per_wave
                                       : 256;
    if (O.chunk0 >= 0) chunk0 = O.chunk0;
    const int64_t share = std::max<int64_t>(1, std::min<int64_t>(1 << 20, count / (waves * 4)));
    int64_t chunk_min = short_walks ? 64 : 1;
    if (O.chunk_min >= 1) chunk_min = O.chunk_min;
    int64_t chunk_max = in.tree ? 16 : 64;
    if (O.chunk_max >= 1) chunk_max = O.chunk_max;
    s.bpc = bpc;
    s.grid = grid;
    s.waves = waves;
    s.chunk0 = chunk0;
    s.queue_base = waves * chunk0;
    s.chunk = (int)std::max<int64_t>(chunk_min, std::min<int64_t>(chunk_max, share));
    // (a guided queue -- the last ~4 walks per lane in chunks of 64 -- measured no faster
    // on C4 and 10-14% slower on the short-walk scenarios: profiles/r02_ab/guided_queue.log)
    // (the waves' rate floor assumes the 100 MHz wall clock of gfx950; the segment-tree
    // kernels keep their host-sized dequeues)
    s.adaptive = !in.tree && O.adaptive_chunk != 0 && O.chunk_min < 1 && O.chunk_max < 1 && in.clock_is_100mhz;
    s.chunk_share = s.adaptive ? (uint32_t)std::max<int64_t>(share, s.chunk) : 0u;
    return s;
}

}  // namespace wost
