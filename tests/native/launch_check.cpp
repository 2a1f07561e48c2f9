// TEST HARNESS -- the launch plan of a solve (dcrmontecarlo_amd/csrc/wost_launch.cpp) on the
// host: range validation, batch planning (with a limit of three blocks' walks, so that the
// multi-batch paths a solve reaches only above 2^26 walks run here) and worked launch shapes.
// Built by tests/test_launch_plan.py from wost_launch.cpp and wost_options.cpp alone.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "../../dcrmontecarlo_amd/csrc/wost_launch.h"

using namespace wost;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

constexpr int64_t B = WOST_BLOCK_WALKS;
constexpr int64_t kTwo31 = int64_t(1) << 31;

// Plans the solve and checks every batch against the unbatched enumeration of its walks:
// block by block, (point, walk of the point).
static void check_plan(int64_t n_points, int64_t W, int64_t bb, int64_t be, int64_t wb, int64_t we, int64_t limit) {
    SolveRanges r;
    char msg[512];
    CHECK(plan_ranges(n_points, W, bb, be, wb, we, &r, msg, sizeof(msg)) == WOST_OK);
    if (we < 0) we = W;
    const bool range = wb != 0 || we != W;
    CHECK(r.range == range && r.nbpp == (W + B - 1) / B && r.Wr == we - wb && r.nbr == (we - wb + B - 1) / B);
    if (range) { bb = 0; be = n_points * r.nbr; }
    CHECK(r.block_begin == bb && r.block_end == be && r.nblk == be - bb);
    // the first walk (point, walk) and the walk count of block j
    auto block = [&](int64_t j, int64_t* p, int64_t* w0) {
        const int64_t per = range ? r.nbr : r.nbpp, lo = range ? wb : 0, hi = range ? we : W;
        *p = j / per;
        *w0 = lo + (j % per) * B;
        return (*w0 + B < hi ? *w0 + B : hi) - *w0;
    };
    int64_t total = 0;
    Batch b;
    int64_t j = bb;
    for (int guard = 0; j < be; ++guard) {
        if (guard > 1 << 20) { CHECK(!"next_batch makes no progress"); return; }
        if (!next_batch(r, j, limit, &b)) { CHECK(!"a block exceeds the batch limit"); return; }
        CHECK(b.j2 > j && b.j2 <= be);                         // tiles the block range, no gap or overlap
        CHECK(b.count > 0 && b.count <= limit);
        CHECK((int64_t)b.begins.size() == b.j2 - j + 1 && b.begins.back() == b.count);
        for (size_t k = 1; k < b.begins.size(); ++k) CHECK(b.begins[k] > b.begins[k - 1]);
        int64_t l = 0;
        for (int64_t blk = j; blk < b.j2; ++blk) {
            int64_t p, w0;
            const int64_t n = block(blk, &p, &w0);
            CHECK(b.begins[(size_t)(blk - j)] == l);
            for (int64_t i = 0; i < n; ++i, ++l) {             // local walk l is walk w0 + i of point p
                int64_t gp, gw;
                if (range) {
                    CHECK(b.range_walks == r.Wr && b.wid_begin == 0);
                    gp = b.range_point0 + l / b.range_walks;
                    gw = b.range_offset + l % b.range_walks;
                } else {
                    CHECK(b.range_walks == 0);
                    const int64_t wid = b.wid_begin + l;
                    gp = wid / W;
                    gw = wid % W;
                    if (b.wid_begin % W <= INT32_MAX)   // (else base_off saturates, and small32 is 0)
                        CHECK(gp == b.base_pid + ((int64_t)b.base_off + l) / W && gw == ((int64_t)b.base_off + l) % W);
                }
                if (gp != p || gw != w0 + i) { CHECK(!"a local walk maps to another (point, walk)"); return; }
            }
        }
        CHECK(l == b.count);
        if (range) {
            CHECK(b.inv_range_walks == 1.0 / (double)r.Wr && b.small32 == 0);
        } else {
            const int64_t off = b.wid_begin % W;
            CHECK(b.small32 == ((W < kTwo31 && off + b.count < kTwo31) ? 1 : 0));
            CHECK(b.base_pid == b.wid_begin / W && (int64_t)b.base_off == (off < INT32_MAX ? off : INT32_MAX));
        }
        total += b.count;
        j = b.j2;
    }
    CHECK(j == be && total == r.walks_total);
}

static void rejected(int64_t n_points, int64_t W, int64_t bb, int64_t be, int64_t wb, int64_t we, const char* want) {
    SolveRanges r;
    char msg[512] = "";
    CHECK(plan_ranges(n_points, W, bb, be, wb, we, &r, msg, sizeof(msg)) == WOST_ERR_INVALID_ARG);
    if (std::strcmp(msg, want) != 0) {
        std::fprintf(stderr, "message: \"%s\"\n   want: \"%s\"\n", msg, want);
        ++fails;
    }
}

struct ShapeWant {
    int64_t bpc; int grid; int64_t waves, chunk0; int chunk; int64_t queue_base; uint32_t chunk_share; bool adaptive;
};

static LaunchShape shape(bool short_walks, bool tree, int64_t count, int block, int occupancy, const Options& o,
                         bool clock_100mhz = true) {
    LaunchIn in;
    in.short_walks = short_walks;
    in.tree = tree;
    in.count = count;
    in.block = block;
    in.blocks_per_cu = occupancy;
    in.num_cus = 256;
    in.opt = &o;
    in.clock_is_100mhz = clock_100mhz;
    return launch_shape(in);
}

static void check_shape(const LaunchShape& s, const ShapeWant& w, int line) {
    const bool same = s.bpc == w.bpc && s.grid == w.grid && s.waves == w.waves && s.chunk0 == w.chunk0 &&
                      s.chunk == w.chunk && s.queue_base == w.queue_base && s.chunk_share == w.chunk_share &&
                      s.adaptive == w.adaptive;
    if (!same) {
        std::fprintf(stderr, "shape of line %d: bpc %lld grid %d waves %lld chunk0 %lld chunk %d queue_base %lld "
                     "chunk_share %u adaptive %d\n", line, (long long)s.bpc, s.grid, (long long)s.waves,
                     (long long)s.chunk0, s.chunk, (long long)s.queue_base, s.chunk_share, (int)s.adaptive);
        ++fails;
    }
}

int main() {
    const int64_t limit = 3 * B;
    // --- batch planning: whole solves
    for (int64_t n : {1, 2, 5})
        for (int64_t W : {int64_t(1), int64_t(7), B - 1, B, B + 1, int64_t(5000), 2 * B + 904, 3 * B, 3 * B + 1, 7 * B + 13})
            check_plan(n, W, 0, n * ((W + B - 1) / B), 0, -1, limit);
    check_plan(5, 3 * B, 0, 5 * 3, 0, -1, limit);               // every batch ends at a point boundary
    check_plan(5, 1, 0, 5, 0, -1, limit);                       // W = 1: one walk per block
    check_plan(5, 1, 0, 5, 0, -1, 2);
    // block ranges starting and ending mid-point, empty ranges
    check_plan(5, 2 * B + 904, 1, 14, 0, -1, limit);
    check_plan(5, 2 * B + 904, 4, 5, 0, -1, limit);
    check_plan(2, 7 * B + 13, 3, 11, 0, -1, limit);
    check_plan(5, 5000, 3, 3, 0, -1, limit);
    check_plan(0, 5000, 0, 0, 0, -1, limit);
    // walk ranges: one point's range per batch, several, ranges ending at W
    check_plan(5, 7 * B + 13, 0, 0, B, 3 * B, limit);
    check_plan(5, 7 * B + 13, 0, 0, 5 * B, 7 * B + 13, limit);
    check_plan(5, 7 * B + 13, 0, 0, 0, B, limit);
    check_plan(2, 3 * B + 1, 0, 0, 3 * B, 3 * B + 1, limit);
    check_plan(1, 9000, 0, 0, B, 9000, limit);
    // 32-bit walk offsets: W = 2^31 never; below it until a batch's walks pass 2^31
    check_plan(1, kTwo31, 0, 3, 0, -1, limit);
    check_plan(1, kTwo31, (kTwo31 / B) - 2, kTwo31 / B, 0, -1, limit);
    check_plan(2, kTwo31 - 1, (kTwo31 / B) - 2, (kTwo31 / B) + 2, 0, -1, limit);
    check_plan(2, kTwo31 + 5, (kTwo31 / B) - 1, (kTwo31 / B) + 3, 0, -1, limit);
    {   // a block larger than the limit: the internal error, not a loop
        SolveRanges r;
        char msg[512];
        Batch b;
        CHECK(plan_ranges(2, 5000, 0, 4, 0, -1, &r, msg, sizeof(msg)) == WOST_OK);
        CHECK(!next_batch(r, 0, 100, &b));
        CHECK(next_batch(r, 1, 904, &b) && b.j2 == 2 && b.count == 904);   // (the point's short last block fits)
        CHECK(plan_ranges(2, 3 * B, 0, 0, B, 3 * B, &r, msg, sizeof(msg)) == WOST_OK);
        CHECK(!next_batch(r, 0, B, &b));
    }
    // --- range validation: the shapes tests/test_gpu_distributed.py rejects on the GPU
    rejected(2, 3 * B, 0, 0, 100, 2 * B, "walk range [100,8192) of 12288 walks must be non-empty with block-aligned "
             "ends (multiples of 4096, or the end at W)");
    rejected(2, 3 * B, 0, 0, B, B + 7, "walk range [4096,4103) of 12288 walks must be non-empty with block-aligned "
             "ends (multiples of 4096, or the end at W)");
    rejected(2, 3 * B, 0, 0, 2 * B, B, "walk range [8192,4096) of 12288 walks must be non-empty with block-aligned "
             "ends (multiples of 4096, or the end at W)");
    rejected(2, 3 * B, 0, 0, -B, B, "walk range [-4096,4096) of 12288 walks must be non-empty with block-aligned "
             "ends (multiples of 4096, or the end at W)");
    rejected(2, 3 * B, 0, 0, B, 4 * B, "walk range [4096,16384) of 12288 walks must be non-empty with block-aligned "
             "ends (multiples of 4096, or the end at W)");
    rejected(2, 3 * B, 0, 7, 0, -1, "block range [0,7) outside [0,6)");
    rejected(2, 3 * B, -1, 2, 0, -1, "block range [-1,2) outside [0,6)");
    rejected(2, 3 * B, 4, 3, 0, -1, "block range [4,3) outside [0,6)");

    // --- launch shapes at 256 CUs (worked by hand from the rules in launch_shape)
    const Options def;
    // short walks, 640,000 of them, occupancy 8
    check_shape(shape(true, false, 640000, 256, 8, def), {4, 1024, 4096, 157, 64, 643072, 64, true}, __LINE__);
    // long walks without a tree, 48M, occupancy 8
    check_shape(shape(false, false, 48000000, 256, 8, def), {8, 2048, 8192, 64, 64, 524288, 1464, true}, __LINE__);
    // a tree kernel: 1000 walks, one 1024-thread workgroup per CU
    check_shape(shape(false, true, 1000, 1024, 1, def), {1, 1, 16, 0, 15, 0, 0, false}, __LINE__);
    // one walk
    check_shape(shape(true, false, 1, 256, 8, def), {2, 1, 4, 1, 64, 4, 64, true}, __LINE__);
    check_shape(shape(false, false, 1, 256, 8, def), {8, 1, 4, 1, 1, 4, 1, true}, __LINE__);
    check_shape(shape(false, true, 1, 1024, 1, def), {1, 1, 16, 0, 1, 0, 0, false}, __LINE__);
    // another wall clock: the waves' rate floor does not hold, host-sized dequeues
    check_shape(shape(true, false, 640000, 256, 8, def, false), {4, 1024, 4096, 157, 64, 643072, 0, false}, __LINE__);
    // the forced shapes of tests/test_gpu_queue.py (16 points x 700 walks = 11,200)
    for (int kind = 0; kind < 3; ++kind) {   // short walks, long walks, the tree kernel
        const bool sw = kind == 0, tree = kind == 2;
        const int block = tree ? 1024 : 256, occ = tree ? 1 : 8;
        const LaunchShape d = shape(sw, tree, 11200, block, occ, def);
        Options o;
        o.adaptive_chunk = 0;
        LaunchShape s = shape(sw, tree, 11200, block, occ, o);
        CHECK(!s.adaptive && s.chunk_share == 0 && s.chunk == d.chunk && s.chunk0 == d.chunk0 && s.grid == d.grid);
        o = Options();
        o.chunk0 = 0;
        s = shape(sw, tree, 11200, block, occ, o);
        CHECK(s.chunk0 == 0 && s.queue_base == 0 && s.adaptive == d.adaptive && s.chunk == d.chunk);
        o.chunk0 = o.chunk_min = o.chunk_max = 1;
        s = shape(sw, tree, 11200, block, occ, o);
        CHECK(s.chunk0 == 1 && s.chunk == 1 && s.queue_base == s.waves && !s.adaptive && s.chunk_share == 0);
        o = Options();
        o.chunk0 = o.chunk_max = 1024;
        s = shape(sw, tree, 11200, block, occ, o);
        CHECK(s.chunk0 == 1024 && s.queue_base == 1024 * s.waves && !s.adaptive);
        CHECK(s.chunk == (sw ? 64 : (int)(11200 / (s.waves * 4))));   // (the floor, or the even share below the cap)
        o = Options();
        o.grid_blocks_per_cu = 1;
        s = shape(sw, tree, 11200, block, occ, o);
        CHECK(s.bpc == 1 && s.grid == (tree ? 11 : 44) && s.adaptive == d.adaptive);
    }
    {   // short walks, 11,200: 2 workgroups per CU, every walk in the static chunks
        check_shape(shape(true, false, 11200, 256, 8, def), {2, 44, 176, 64, 64, 11264, 64, true}, __LINE__);
        check_shape(shape(false, false, 11200, 256, 8, def), {8, 44, 176, 64, 15, 11264, 15, true}, __LINE__);
        check_shape(shape(false, true, 11200, 1024, 1, def), {1, 11, 176, 0, 15, 0, 0, false}, __LINE__);
    }
    std::printf("launch_check: %d failed checks\n", fails);
    return fails ? 1 : 0;
}
