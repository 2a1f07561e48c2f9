// TEST HARNESS -- the walk kernels' id arithmetic (wost_walk.h WOST_WALK_OF_LOCAL, through
// walk_of_local: the text walk_body expands at its refill) on the host, against exact integer
// division. The refill takes a walk's point index from a double estimate and one correction,
// on one of three paths (walk-range batches, 32-bit offsets, 64 bits); every local index of
// every batch that the real launch plan (wost_launch.cpp plan_ranges / next_batch) makes of
// the solves below is mapped and compared with (point, walk) by / and %, and the
// corrections that fire are counted per path.
// Built and run by tests/test_walk_ids.py (hipcc, host code only; its own main, so it also
// builds with -Xarch_host -fsanitize=address,undefined).
#include <cstdint>
#include <cstdio>
#include <initializer_list>

static uint64_t g_corrected[3][2];   // [path: range, small32, 64-bit][--q, ++q]
#define WOST_WALK_ID_CORRECTED(path, dir) ++g_corrected[path][(dir) > 0];
#include "../../dcrmontecarlo_amd/csrc/wost_walk.h"
#include "../../dcrmontecarlo_amd/csrc/wost_launch.h"

using namespace wost;

constexpr int64_t B = WOST_BLOCK_WALKS;
constexpr int64_t kBatchLimit = int64_t(1) << 26;   // wost_handle.h kMaxBatchWalks

static long fails = 0;
static uint64_t g_checked[3];    // indices checked per path
static uint64_t g_batches[3];
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
    return a;
}

// Plans blocks [bb, be) (or the walk range [wb, we) of every point) with batches of at most
// `limit` walks and checks every local index of every batch. want_path >= 0: every batch
// must take that path. Returns the batches planned.
static int check_solve(int64_t n_points, int64_t W, int64_t bb, int64_t be, int64_t wb, int64_t we, int64_t limit,
                       int want_path) {
    SolveRanges r;
    char msg[512];
    if (plan_ranges(n_points, W, bb, be, wb, we, &r, msg, sizeof(msg)) != WOST_OK) {
        std::fprintf(stderr, "plan_ranges(%lld, %lld, [%lld,%lld), [%lld,%lld)): %s\n", (long long)n_points, (long long)W,
                     (long long)bb, (long long)be, (long long)wb, (long long)we, msg);
        ++fails;
        return 0;
    }
    Batch b;
    int batches = 0;
    for (int64_t j = r.block_begin; j < r.block_end; j = b.j2, ++batches) {
        if (!next_batch(r, j, limit, &b) || b.j2 <= j) { CHECK(!"next_batch made no batch"); return batches; }
        const WalkArgs a = args_of(r, b);
        const int path = a.range_walks > 0 ? 0 : a.small32 ? 1 : 2;
        CHECK(want_path < 0 || path == want_path);
        ++g_batches[path];
        long bad = 0;
        for (int64_t blk = j; blk < b.j2; ++blk) {
            // block blk, by exact integer arithmetic: its point and its first walk of the point
            const int64_t per = r.range ? r.nbr : r.nbpp, lo = r.range ? r.walk_begin : 0, hi = r.range ? r.walk_end : W;
            const int64_t p = blk / per, w0 = lo + (blk % per) * B, n = (w0 + B < hi ? w0 + B : hi) - w0;
            const int64_t l0 = b.begins[(size_t)(blk - j)];
            CHECK(b.begins[(size_t)(blk - j) + 1] - l0 == n);
            for (int64_t i = 0; i < n; ++i) {
                uint64_t wid = ~0ull;
                const uint64_t pid = walk_of_local(a, (uint64_t)(l0 + i), &wid);
                const uint64_t want = (uint64_t)p * (uint64_t)W + (uint64_t)(w0 + i);
                if (wid != want || pid != wid / (uint64_t)W || pid != (uint64_t)p || wid % (uint64_t)W != (uint64_t)(w0 + i)) {
                    if (bad++ == 0 && fails < 20)
                        std::fprintf(stderr, "W %lld path %d block %lld local %lld: walk %llu of point %llu, want walk "
                                     "%llu of point %lld\n", (long long)W, path, (long long)blk, (long long)(l0 + i),
                                     (unsigned long long)wid, (unsigned long long)pid, (unsigned long long)want, (long long)p);
                }
            }
            g_checked[path] += (uint64_t)n;
        }
        fails += bad;
    }
    return batches;
}

// Blocks around every point boundary and at both ends of the id space of n_points x W walks:
// planned together (one batch per group of neighbours) and each block alone.
static void check_boundaries(int64_t n_points, int64_t W) {
    const int64_t nbpp = (W + B - 1) / B, nb = n_points * nbpp;
    for (int64_t p = 0; p <= n_points; ++p) {
        const int64_t b0 = p * nbpp - 2 < 0 ? 0 : p * nbpp - 2, b1 = p * nbpp + 2 > nb ? nb : p * nbpp + 2;
        check_solve(n_points, W, b0, b1, 0, -1, kBatchLimit, -1);
        for (int64_t j = b0; j < b1; ++j) check_solve(n_points, W, j, j + 1, 0, -1, kBatchLimit, -1);
    }
}

int main() {
    const int64_t two31 = int64_t(1) << 31, two15 = int64_t(1) << 15;
    // --- every W in [1, 8192], at least 2^15 walks: whole solves of enough points to cross
    // several point boundaries (32-bit offsets), and Wr = W as a walk range after one block
    for (int64_t W = 1; W <= 8192; ++W) {
        const int64_t n = (two15 + W - 1) / W + 1;
        check_solve(n, W, 0, n * ((W + B - 1) / B), 0, -1, kBatchLimit, 1);
        check_solve(n, B + W, 0, 0, B, B + W, kBatchLimit, 0);   // several points per batch
    }
    // walk ranges with a batch limit of three blocks: one or few points per batch, many batches
    for (int64_t Wr : {int64_t(1), int64_t(49), int64_t(98), int64_t(4097), int64_t(8192)})
        check_solve(300, 2 * B + Wr, 0, 0, 2 * B, 2 * B + Wr, 3 * B, 0);
    // whole multi-batch solves with a small limit: base_pid and base_off move with the batch
    for (int64_t W : {int64_t(49), int64_t(98), int64_t(5000), 3 * B + 49})
        check_solve(700, W, 0, 700 * ((W + B - 1) / B), 0, -1, 3 * B, 1);
    // --- 49 * 2^k and 98 * 2^k up to 2^40: W = 49 needs the correction at q = 1, 2, 3, 4, 6, ...
    for (int64_t m : {int64_t(49), int64_t(98)})
        for (int k = 0; (m << k) <= (int64_t(1) << 40); ++k) {
            const int64_t W = m << k;
            check_boundaries(5, W);
            if (W < two15) { const int64_t n = two15 / W + 2; check_solve(n, W, 0, n * ((W + B - 1) / B), 0, -1, kBatchLimit, 1); }
        }
    // --- around 2^31 (the switch between 32-bit offsets and 64 bits) and far above it
    const int64_t big = ((int64_t(1) << 53) / 3) / B * B;
    for (int64_t W : {two31 - 1000, two31 - 1, two31, two31 + 2048, (int64_t(1) << 30) + 123, (int64_t(1) << 40) + 1000, big})
        check_boundaries(3, W);
    {   // both sides of the switch: the same block alone (32-bit offsets) and with its neighbours (64 bits)
        const int64_t W = two31 - 1000, nbpp = (W + B - 1) / B;
        check_solve(3, W, nbpp - 2, nbpp - 1, 0, -1, kBatchLimit, 1);
        check_solve(3, W, nbpp - 1, nbpp, 0, -1, kBatchLimit, 1);
        check_solve(3, W, nbpp - 2, nbpp + 1, 0, -1, kBatchLimit, 2);
        // 49 * 2^25 < 2^31: 32-bit offsets across the point boundary too (offset + count = W + 4096 < 2^31),
        // where local = W needs the correction
        const int64_t W2 = int64_t(49) << 25, nb2 = (W2 + B - 1) / B;
        check_solve(3, W2, nb2 - 1, nb2, 0, -1, kBatchLimit, 1);
        check_solve(3, W2, nb2 - 1, nb2 + 1, 0, -1, kBatchLimit, 1);
        // a full batch (2^26 walks) at the top of a point's 32-bit offsets, then across it
        check_solve(2, two31 - 1, nbpp - (kBatchLimit / B) - 1, nbpp - 1, 0, -1, kBatchLimit, 1);
        check_solve(2, two31 - 1, (two31 / B) - (kBatchLimit / B) + 1, (two31 / B) + 1, 0, -1, kBatchLimit, 2);
    }
    const char* name[3] = {"range", "small32", "64-bit"};
    for (int p = 0; p < 3; ++p)
        std::printf("walk_ids_check: path %-7s %12llu indices in %8llu batches, ++q %9llu, --q %9llu\n", name[p],
                    (unsigned long long)g_checked[p], (unsigned long long)g_batches[p],
                    (unsigned long long)g_corrected[p][1], (unsigned long long)g_corrected[p][0]);
    if (g_corrected[0][0] + g_corrected[1][0] + g_corrected[2][0] == 0)
        std::printf("walk_ids_check: --q never fired (the estimate was never too large)\n");
    for (int p = 0; p < 3; ++p) {
        CHECK(g_checked[p] > 0);
        CHECK(g_corrected[p][1] > 0);   // the ++q branch of each path ran (and gave the exact quotient)
    }
    std::printf("walk_ids_check: %ld failed checks\n", fails);
    return fails ? 1 : 0;
}
