// TEST HARNESS -- the launch plan and the walk kernels' id arithmetic with a point list
// (wost_solve_range_points): wost_walk.h WOST_WALK_OF_LOCAL built with WOST_POINT_LIST, through
// walk_of_local, over every batch that plan_ranges / next_batch (wost_launch.cpp) make of a
// walk range of a list of points. In range mode the plan's points are list positions; the
// kernel takes the point from the list. Every local index of every batch is mapped and its
// (walk id, point) compared with plain integer arithmetic on the listed point's id.
// Lists: every point, the last point alone, a list with gaps. Shapes: n_sel * Wr above the
// batch limit (several batches, range_point0 > 0), Wr = 49 at walk_begin = 4096 (the ++q
// correction of the quotient estimate fires: counted), W = 2^40 + 1000 (ids beyond 2^32).
// Built and run by tests/test_point_list_plan.py (hipcc, host code only; its own main, so it
// also builds with -Xarch_host -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <vector>

static uint64_t g_corrected[3][2];   // [path: range, small32, 64-bit][--q, ++q]
#define WOST_WALK_ID_CORRECTED(path, dir) ++g_corrected[path][(dir) > 0];
#define WOST_POINT_LIST 1
#include "../../dcrmontecarlo_amd/csrc/wost_walk.h"
#include "../../dcrmontecarlo_amd/csrc/wost_launch.h"

using namespace wost;

constexpr int64_t B = WOST_BLOCK_WALKS;

static long fails = 0;
static uint64_t g_checked = 0, g_batches = 0, g_late_batches = 0;   // late: range_point0 > 0
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

// The id fields of the kernel's arguments, as wost_solve.cpp fill_walk_args / set_batch_args set them.
static WalkArgs args_of(const SolveRanges& r, const Batch& b) {
    WalkArgs a{};
    a.walks_per_point = r.W;
    a.inv_walks_per_point = 1.0 / (double)r.W;
    a.wid_begin = b.wid_begin;
    a.base_pid = b.base_pid;
    a.base_off = b.base_off;
    a.small32 = b.small32;
    a.range_walks = b.range_walks;
    a.range_offset = b.range_offset;
    a.range_point0 = b.range_point0;
    a.inv_range_walks = b.inv_range_walks;
    a.count = b.count;
    a.point_list = r.point_ids;
    return a;
}

// Walks [wb, we) of the listed points of n_points x W, in batches of at most `limit` walks.
// Returns the batches planned.
static int check_list(int64_t n_points, int64_t W, const std::vector<int32_t>& ids, int64_t wb, int64_t we,
                      int64_t limit) {
    SolveRanges r;
    char msg[512];
    const int64_t n_sel = (int64_t)ids.size();
    if (plan_ranges(n_points, W, 0, 0, wb, we, &r, msg, sizeof(msg), ids.data(), n_sel) != WOST_OK) {
        std::fprintf(stderr, "plan_ranges: %s\n", msg);
        ++fails;
        return 0;
    }
    const int64_t Wr = we - wb, nbr = (Wr + B - 1) / B;
    CHECK(r.range && r.Wr == Wr && r.nbr == nbr && r.plan_points() == n_sel);
    CHECK(r.block_begin == 0 && r.block_end == n_sel * nbr && r.nblk == n_sel * nbr && r.walks_total == n_sel * Wr);
    Batch b;
    int batches = 0;
    int64_t walks = 0;
    for (int64_t j = r.block_begin; j < r.block_end; j = b.j2, ++batches) {
        if (!next_batch(r, j, limit, &b) || b.j2 <= j) { CHECK(!"next_batch made no batch"); return batches; }
        CHECK(b.count <= limit && b.count % Wr == 0 && j % nbr == 0 && b.j2 % nbr == 0);   // whole points' ranges
        CHECK(b.range_walks == Wr && b.range_offset == wb && b.range_point0 == j / nbr);
        CHECK((int64_t)b.begins.size() == b.j2 - j + 1 && b.begins.back() == b.count);
        const WalkArgs a = args_of(r, b);
        ++g_batches;
        if (b.range_point0 > 0) ++g_late_batches;
        long bad = 0;
        for (int64_t blk = j; blk < b.j2; ++blk) {
            // block blk by plain integer arithmetic: its list position, point and first walk
            const int64_t pos = blk / nbr, w0 = wb + (blk % nbr) * B, n = (w0 + B < we ? w0 + B : we) - w0;
            CHECK(r.point_of(blk) == pos);
            const uint64_t p = (uint64_t)ids[(size_t)pos];
            const int64_t l0 = b.begins[(size_t)(blk - j)];
            CHECK(b.begins[(size_t)(blk - j) + 1] - l0 == n);
            for (int64_t i = 0; i < n; ++i) {
                uint64_t wid = ~0ull;
                const uint64_t pid = walk_of_local(a, (uint64_t)(l0 + i), &wid);
                const uint64_t want = p * (uint64_t)W + (uint64_t)(w0 + i);
                if (wid != want || pid != p || wid / (uint64_t)W != p || wid % (uint64_t)W != (uint64_t)(w0 + i)) {
                    if (bad++ == 0 && fails < 20)
                        std::fprintf(stderr, "W %lld block %lld local %lld: walk %llu of point %llu, want walk %llu of "
                                     "point %llu\n", (long long)W, (long long)blk, (long long)(l0 + i),
                                     (unsigned long long)wid, (unsigned long long)pid, (unsigned long long)want,
                                     (unsigned long long)p);
                }
            }
            g_checked += (uint64_t)n;
        }
        fails += bad;
        walks += b.count;
    }
    CHECK(walks == r.walks_total);
    return batches;
}

static std::vector<int32_t> all_ids(int32_t n) {
    std::vector<int32_t> v((size_t)n);
    for (int32_t i = 0; i < n; ++i) v[(size_t)i] = i;
    return v;
}

int main() {
    const int32_t N = 700;
    std::vector<int32_t> gaps;   // every third point, a run of neighbours, the last point
    for (int32_t i = 1; i < N - 20; i += 3) gaps.push_back(i);
    for (int32_t i = N - 20; i < N - 14; ++i) gaps.push_back(i);
    gaps.push_back(N - 1);
    const std::vector<std::vector<int32_t>> lists = {all_ids(N), {N - 1}, gaps};

    for (const auto& ids : lists) {
        const int64_t n_sel = (int64_t)ids.size();
        // one launch holds everything
        CHECK(check_list(N, 3 * B + 49, ids, B, 2 * B, int64_t(1) << 26) == 1);
        // the whole range [0, W) with a list is a range all the same
        check_list(N, 2 * B + 5, ids, 0, 2 * B + 5, int64_t(1) << 26);
        // n_sel * Wr above the batch limit: several batches, range_point0 > 0
        const int batches = check_list(N, 4 * B, ids, B, 3 * B, 5 * B);
        CHECK(batches == (n_sel + 1) / 2);
        // Wr = 49 at walk_begin = 4096: the quotient estimate needs its ++q correction
        const uint64_t up0 = g_corrected[0][1];
        check_list(N, B + 49, ids, B, B + 49, 40 * 49);
        if (n_sel > 1) CHECK(g_corrected[0][1] > up0);
        // W = 2^40 + 1000: ids beyond 2^32, the last two blocks of every listed point
        const int64_t W = (int64_t(1) << 40) + 1000, nbpp = (W + B - 1) / B;
        check_list(N, W, ids, (nbpp - 2) * B, W, 3 * (B + 1000));
    }
    CHECK(g_late_batches > 0);
    CHECK(g_corrected[0][1] > 0);
    CHECK(g_corrected[1][0] + g_corrected[1][1] + g_corrected[2][0] + g_corrected[2][1] == 0);   // the range path only

    // refusals: an empty list, ids out of order, twice, or outside [0, n_points)
    SolveRanges r;
    char msg[512];
    const int32_t one[] = {3}, unsorted[] = {4, 2}, twice[] = {2, 2}, high[] = {1, N}, low[] = {-1, 2};
    CHECK(plan_ranges(N, 2 * B, 0, 0, 0, B, &r, msg, sizeof(msg), one, 1) == WOST_OK);
    CHECK(plan_ranges(N, 2 * B, 0, 0, 0, B, &r, msg, sizeof(msg), one, 0) == WOST_ERR_INVALID_ARG);
    CHECK(plan_ranges(N, 2 * B, 0, 0, 0, B, &r, msg, sizeof(msg), unsorted, 2) == WOST_ERR_INVALID_ARG);
    CHECK(plan_ranges(N, 2 * B, 0, 0, 0, B, &r, msg, sizeof(msg), twice, 2) == WOST_ERR_INVALID_ARG);
    CHECK(plan_ranges(N, 2 * B, 0, 0, 0, B, &r, msg, sizeof(msg), high, 2) == WOST_ERR_INVALID_ARG);
    CHECK(plan_ranges(N, 2 * B, 0, 0, 0, B, &r, msg, sizeof(msg), low, 2) == WOST_ERR_INVALID_ARG);
    // ... and without a list the plan is what it was: [0, W) is no range
    CHECK(plan_ranges(N, 2 * B, 0, N * 2, 0, -1, &r, msg, sizeof(msg)) == WOST_OK && !r.range && r.plan_points() == N);

    std::printf("point_list_check: %llu indices in %llu batches (%llu with range_point0 > 0), ++q %llu, --q %llu\n",
                (unsigned long long)g_checked, (unsigned long long)g_batches, (unsigned long long)g_late_batches,
                (unsigned long long)g_corrected[0][1], (unsigned long long)g_corrected[0][0]);
    std::printf("point_list_check: %ld failed checks\n", fails);
    return fails ? 1 : 0;
}
