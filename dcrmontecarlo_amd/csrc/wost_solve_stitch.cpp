// wost_solve_stitch.cpp -- the wost_solve* entry points, and the solves they stitch from
// several solve_impl calls: wost_solve_range beyond one launch per point, and the solve
// that starts on the precompiled kernel while its own compiles (option jit_race).
#include <algorithm>
#include <chrono>

#include "wost_combine.h"
#include "wost_handle.h"

using namespace wost;

namespace {

SolveRequest whole_request(const float* points, int64_t n_points, int64_t W, int32_t max_steps, float eps,
                           uint64_t seed) {
    return SolveRequest{.points = points, .n_points = n_points, .W = W, .max_steps = max_steps, .eps = eps,
                        .seed = seed, .block_end = wost_num_blocks(n_points, W)};
}

// Accumulates a piece's timing into a multi-launch solve's (wost_solve_range, solve_race).
void add_timing(wost_timing& acc, const wost_timing& t) {
    acc.walk_kernel_ms += t.walk_kernel_ms;
    acc.reduce_kernel_ms += t.reduce_kernel_ms;
    acc.total_ms += t.total_ms;
    acc.n_launches += t.n_launches;
    acc.total_steps += t.total_steps;
    acc.total_walks += t.total_walks;
    acc.grid_blocks = t.grid_blocks;
    acc.jit = t.jit;
    acc.tree = t.tree;
    acc.blocks_per_cu = t.blocks_per_cu;
    acc.block_threads = t.block_threads;
    acc.chunk0 = t.chunk0;
    acc.chunk = t.chunk;
    acc.adaptive = t.adaptive;
    acc.max_walk_steps = std::max(acc.max_walk_steps, t.max_walk_steps);
    acc.jit_ms += t.jit_ms;
    acc.span_ms += t.span_ms;
    acc.tail_ms = t.tail_ms;
    acc.last_wave_ms = t.last_wave_ms;
    acc.last_wave_iters = t.last_wave_iters;
    acc.max_wave_iters = std::max(acc.max_wave_iters, t.max_wave_iters);
    acc.precompiled_walks += t.precompiled_walks;
}

// A solve of walks [w_begin, w_begin + Wr) of every point (with a point list: of every listed
// point, one row each) that takes several solves of
// block-aligned sub-ranges (wost_solve_range beyond one launch per point, solve_race): each
// piece's block rows, values and steps are scattered into the whole range's layout, so the
// block sums, their order and every output are those of one solve.
struct Stitch {
    SolveRequest rq;       // the whole solve (its ranges set per piece)
    SolveOutputs out;
    int ns = 1;            // values per walk
    int64_t w_begin = 0, Wr = 0, nbr = 0;
    std::vector<double> all, part;   // block rows of the range / of a piece
    std::vector<double> call, cpart;   // ... and their weighted combinations' (rows of crow doubles; 0: none)
    int crow = 0;
    double combine_ms = 0.0;
    std::vector<float> pv;
    std::vector<uint32_t> ps;
    wost_timing acc{};
    double solve_ms = 0.0;   // host time of the last piece's solve

    Stitch(const SolveRequest& whole, const SolveOutputs& o, int ns_, int64_t w0, int64_t w1)
        : rq(whole), out(o), ns(ns_), w_begin(w0), Wr(w1 - w0), nbr((w1 - w0 + WOST_BLOCK_WALKS - 1) / WOST_BLOCK_WALKS),
          all((size_t)whole.rows() * nbr * (2 * ns_ + 1)), crow(o.weights ? 2 * o.n_combinations + 1 : 0) {
        if (crow > 0) call.resize((size_t)whole.rows() * nbr * crow);
    }
};

// Solves walks [c0, c1) of every point into the stitched solve's outputs and timing.
int solve_piece(wost_handle* h, Stitch& s, int64_t c0, int64_t c1) {
    const int row = 2 * s.ns + 1;
    const int64_t n_points = s.rq.rows();   // (point rows of the outputs)
    const int64_t wc = c1 - c0, nbc = (wc + WOST_BLOCK_WALKS - 1) / WOST_BLOCK_WALKS;
    const int64_t woff = c0 - s.w_begin, boff = woff / WOST_BLOCK_WALKS;
    s.part.resize((size_t)n_points * nbc * row);
    if (s.out.walk_values) s.pv.resize((size_t)n_points * wc * s.ns);
    if (s.out.walk_steps) s.ps.resize((size_t)n_points * wc);
    // (the whole of [0, W) is an ordinary solve of every block: solve_impl takes it as no range)
    s.rq.walk_begin = c0;
    s.rq.walk_end = c1;
    SolveOutputs piece;
    piece.block_stats = s.part.data();
    piece.walk_values = s.out.walk_values ? s.pv.data() : nullptr;
    piece.walk_steps = s.out.walk_steps ? s.ps.data() : nullptr;
    if (s.crow > 0) {
        s.cpart.resize((size_t)n_points * nbc * s.crow);
        piece.weights = s.out.weights;
        piece.n_combinations = s.out.n_combinations;
        piece.combined_block_stats = s.cpart.data();
    }
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = solve_impl(h, s.rq, piece);
    s.solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != WOST_OK) return rc;
    for (int64_t p = 0; p < n_points; ++p) {
        std::memcpy(&s.all[((size_t)p * s.nbr + boff) * row], &s.part[(size_t)p * nbc * row], sizeof(double) * nbc * row);
        if (s.crow > 0)
            std::memcpy(&s.call[((size_t)p * s.nbr + boff) * s.crow], &s.cpart[(size_t)p * nbc * s.crow],
                        sizeof(double) * nbc * s.crow);
        if (s.out.walk_values)
            std::memcpy(s.out.walk_values + ((size_t)p * s.Wr + woff) * s.ns, &s.pv[(size_t)p * wc * s.ns],
                        sizeof(float) * wc * s.ns);
        if (s.out.walk_steps)
            std::memcpy(s.out.walk_steps + (size_t)p * s.Wr + woff, &s.ps[(size_t)p * wc], sizeof(uint32_t) * wc);
    }
    add_timing(s.acc, h->timing);
    s.combine_ms += h->combine_ms;
    return WOST_OK;
}

// The stitched solve's block rows and point sums (in the range's block order) to the caller.
void stitched_rows(const Stitch& s, const std::vector<double>& all, int row, double* block_stats, double* point_stats) {
    if (block_stats) std::memcpy(block_stats, all.data(), sizeof(double) * all.size());
    if (!point_stats) return;
    std::fill(point_stats, point_stats + (size_t)row * s.rq.rows(), 0.0);
    for (int64_t p = 0; p < s.rq.rows(); ++p)
        for (int64_t k = 0; k < s.nbr; ++k)
            for (int c = 0; c < row; ++c) point_stats[(size_t)row * p + c] += all[((size_t)p * s.nbr + k) * row + c];
}

void stitched_stats(const Stitch& s) {
    stitched_rows(s, s.all, 2 * s.ns + 1, s.out.block_stats, s.out.point_stats);
    if (s.crow > 0) stitched_rows(s, s.call, s.crow, s.out.combined_block_stats, s.out.combined_point_stats);
}

// A whole single-source solve whose field-specialised kernel is in no cache (option
// jit_race; the reference calls solve() once per script): its compile starts in a helper
// process, and meanwhile the precompiled kernel -- the same bits walk for walk
// (test_jit_kernel_matches_interpreted_kernel) but 2-5x slower -- runs the walks in ranges
// of every point (the first ~2^19 walks, then ~16 ms of work each); once the compile is
// done the specialised kernel runs the rest. Ranges of walks are whole blocks, so the
// block sums, their order and every output are those of one launch (as wost_solve_range's).
// A solve that finds the compile already running waits for it instead (jit_get_kernel).
constexpr double kCompileExpectMs = 300.0;   // a specialised kernel's compile (MI355X box: 180-600 ms)

int solve_race(wost_handle* h, const SolveRequest& rq, const SolveOutputs& out) {
    const float* points = rq.points;
    const int64_t n_points = rq.n_points, W = rq.W;
    if (!points) return solve_impl(h, rq, out);
    for (int64_t i = 0; i < 2 * n_points; ++i)
        if (!std::isfinite(points[i])) return solve_impl(h, rq, out);   // (its error message)
    const WalkTraits t = walk_traits(h);
    if (t.delta && !h->fields[SLOT_F].present) return solve_impl(h, rq, out);
    HIP_TRY(hipSetDevice(h->device));
    int rc;
    if ((rc = upload_program(h)) != WOST_OK) return rc;
    if (t.tree && (rc = ensure_tree(h)) != WOST_OK) return rc;
    KernelShape ks;
    if ((rc = first_kernel_shape(h, t, &ks)) != WOST_OK) return rc;
    JitTicket ticket;
    if (jit_kernel_try(h, kernel_variant(h, t, ks, false, 1), &ticket) != JitTry::kStarted)
        return solve_impl(h, rq, out);

    const int64_t max_piece = kMaxBatchWalks / WOST_BLOCK_WALKS * WOST_BLOCK_WALKS;   // walks of a point per launch
    auto blocks_up = [](double walks) {
        const double b = std::ceil(std::max(walks, 1.0) / WOST_BLOCK_WALKS);
        return (int64_t)std::min(b, 1e15) * WOST_BLOCK_WALKS;
    };
    int64_t piece = std::min(max_piece, blocks_up((double)(1 << 19) / (double)n_points));
    const auto race_t0 = std::chrono::steady_clock::now();
    Stitch st(rq, out, 1, 0, W);
    bool jit_now = false;
    const bool saved = h->jit_enabled;
    for (int64_t w0 = 0; w0 < W;) {
        if (!jit_now && ticket.done()) jit_now = true;
        const int64_t w1 = std::min(W, w0 + (jit_now ? max_piece : piece));
        const int64_t wc = w1 - w0;
        h->jit_enabled = jit_now;
        rc = solve_piece(h, st, w0, w1);
        h->jit_enabled = saved;
        if (rc == WOST_ERR_UNSUPPORTED && !jit_now) {   // (a shape only the specialised kernel runs)
            jit_now = true;
            continue;
        }
        if (rc != WOST_OK) return rc;
        if (!jit_now) {
            st.acc.precompiled_walks += (uint64_t)(n_points * wc);
            // the next range, from this one's rate: all the rest when the precompiled kernel
            // finishes it before the compile is likely done (every range ends in a tail of
            // the longest walks: one launch, not many); else about half the compile's
            // expected remaining time, at least 16 ms of work, at most 8x this range
            const double rate = (double)wc / std::max(st.solve_ms, 0.05);   // walks per point per ms
            const double since = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() -
                                                                            race_t0).count();
            const double compile_left = std::max(0.0, kCompileExpectMs - since);
            if ((double)(W - w1) / rate <= compile_left) {
                piece = std::min(max_piece, W - w1);
            } else {
                const double target = std::max(16.0, 0.5 * compile_left);
                piece = std::min(max_piece, std::max(piece, std::min(8 * piece, blocks_up(rate * target))));
            }
        }
        w0 = w1;
    }
    stitched_stats(st);
    st.acc.jit = jit_now ? 1 : 0;
    h->timing = st.acc;
    return WOST_OK;
}

// The entry points' output pointers.
SolveOutputs outputs(double* block_stats, double* point_stats, float* walk_values, uint32_t* walk_steps,
                     float* records = nullptr) {
    return SolveOutputs{.block_stats = block_stats, .point_stats = point_stats, .walk_values = walk_values,
                        .walk_steps = walk_steps, .records = records};
}

// wost_solve_range_points' body: one solve, or block-aligned pieces stitched.
int solve_range(wost_handle* h, SolveRequest rq, const SolveOutputs& out, int64_t walk_begin, int64_t walk_end) {
    const int64_t W = rq.W, n_points = rq.n_points, n_ids = rq.n_ids;
    const int32_t* const point_ids = rq.point_ids;
    // the whole range of every point: an ordinary solve (of a list: a range all the same)
    if (walk_begin == 0 && walk_end == W && !point_ids) return solve_impl(h, rq, out);
    const int ns = h->channels();
    const int64_t chunk = (kMaxBatchWalks / ns) / WOST_BLOCK_WALKS * WOST_BLOCK_WALKS;   // walks of a point per launch
    if (walk_end - walk_begin <= chunk || walk_begin < 0 || walk_end <= walk_begin || n_points <= 0 ||
        (point_ids && n_ids < 1)) {
        rq.block_end = 0;   // (a range names its walks only)
        rq.walk_begin = walk_begin;
        rq.walk_end = walk_end;
        return solve_impl(h, rq, out);
    }
    // a range longer than one launch holds per point: block-aligned sub-ranges, one solve
    // each, scattered into the range's layout; point sums in the range's block order
    Stitch st(rq, out, ns, walk_begin, walk_end);
    for (int64_t c0 = walk_begin; c0 < walk_end; c0 += chunk)
        if (int rc = solve_piece(h, st, c0, std::min(walk_end, c0 + chunk))) return rc;
    stitched_stats(st);
    h->timing = st.acc;
    h->combine_ms = st.combine_ms;
    return WOST_OK;
}

}  // namespace

extern "C" {

int wost_solve(wost_handle* h, const float* points, int64_t n_points, int64_t W,
               int64_t block_begin, int64_t block_end, int32_t max_steps, float eps, uint64_t seed,
               double* block_stats, double* point_stats, float* walk_values, uint32_t* walk_steps) {
    SolveRequest rq = whole_request(points, n_points, W, max_steps, eps, seed);
    const SolveOutputs out = outputs(block_stats, point_stats, walk_values, walk_steps);
    // a whole single-source solve may start on the precompiled kernel while its specialised
    // one compiles (solve_race)
    if (h && h->jit_enabled && h->opt.jit_race && h->channels() == 1 && h->charges.empty() && n_points > 0 && W > 0 &&
        block_begin == 0 &&
        block_end == rq.block_end && max_steps >= 0 && eps == eps)
        return solve_race(h, rq, out);
    rq.block_begin = block_begin;
    rq.block_end = block_end;
    return solve_impl(h, rq, out);
}

int wost_solve_range(wost_handle* h, const float* points, int64_t n_points, int64_t W, int64_t walk_begin,
                     int64_t walk_end, int32_t max_steps, float eps, uint64_t seed, double* block_stats,
                     double* point_stats, float* walk_values, uint32_t* walk_steps) {
    return wost_solve_range_points(h, points, n_points, nullptr, 0, W, walk_begin, walk_end, max_steps, eps, seed,
                                   block_stats, point_stats, walk_values, walk_steps);
}

int wost_solve_range_points(wost_handle* h, const float* points, int64_t n_points, const int32_t* point_ids,
                            int64_t n_ids, int64_t W, int64_t walk_begin, int64_t walk_end, int32_t max_steps,
                            float eps, uint64_t seed, double* block_stats, double* point_stats, float* walk_values,
                            uint32_t* walk_steps) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    SolveRequest rq = whole_request(points, n_points, W, max_steps, eps, seed);
    rq.multi = true;
    rq.point_ids = point_ids;   // (null: every point, wost_solve_range)
    rq.n_ids = point_ids ? n_ids : 0;
    return solve_range(h, rq, outputs(block_stats, point_stats, walk_values, walk_steps), walk_begin, walk_end);
}

}  // extern "C"

namespace {

// wost_solve_range_tally (n_maps 0, weights null) and wost_solve_range_tally_channels (n_maps
// maps of the handle's channels): the refusals, the buffers, the solve, the flag, the copy.
int solve_tally(wost_handle* h, const float* points, int64_t n_points, int64_t W, int64_t walk_begin,
                int64_t walk_end, int32_t max_steps, float eps, uint64_t seed, const wost_tally_grid* grid,
                int32_t replicas, int32_t scale_log2, const float* weights, int32_t n_maps, bool channels,
                double* block_stats, double* point_stats, float* walk_values, uint32_t* walk_steps, int64_t* tally,
                int64_t* row_walks) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (h->compat != WOST_COMPAT_FIXED)
        return fail(WOST_ERR_UNSUPPORTED, "a tally needs compat=\"fixed\": the reference's source sample does not estimate "
                                          "the integral of G f (quirks Q3, Q13)");
    if (!h->charges.empty())
        return fail(WOST_ERR_UNSUPPORTED, "a tally rides the source sample: a handle with point sources "
                                          "(wost_set_point_sources) samples none; clear them first");
    if (channels && h->n_sources != 1)
        return fail(WOST_ERR_UNSUPPORTED, "channel maps take one source: the handle scores %d (wost_set_sources); the map "
                                          "does not depend on f", h->n_sources);
    if (!channels && (h->n_sources != 1 || h->n_wavenumbers > 0 || h->n_models > 0))
        return fail(WOST_ERR_UNSUPPORTED, "a tally takes one channel: the handle scores %d sources x %d wavenumbers x %d "
                                          "models (wost_set_sources / wost_set_wavenumbers / wost_set_models)",
                    h->n_sources, std::max(h->n_wavenumbers, 1), std::max(h->n_models, 1));
    if (!h->fields[SLOT_F].present)
        return fail(WOST_ERR_INVALID_ARG, "a tally rides the source sample: the handle needs a source field (a constant "
                                          "0 is enough)");
    if (!h->jit_enabled)
        return fail(WOST_ERR_UNSUPPORTED, "a tally needs the field-specialised kernel (disabled by wost_set_jit)");
    const int64_t maps = channels ? n_maps : 1;   // sub-rows per replica row
    if (channels)
        if (int rc = tally_check_weights(weights, n_maps, h->channels())) return rc;
    if (!tally) return fail(WOST_ERR_INVALID_ARG, "NULL tally");
    if (int rc = tally_grid_check(grid)) return rc;
    if (n_points < 0 || W < 1 || W >= (int64_t(1) << 43))
        return fail(WOST_ERR_INVALID_ARG, "a tally takes 1 <= walks_per_point < 2^43 and n_points >= 0");
    if (scale_log2 < -100 || scale_log2 > 100) return fail(WOST_ERR_INVALID_ARG, "scale_log2 must be in [-100, 100]");
    TallyRequest T;
    T.grid = *grid;
    T.replicas = replicas;
    T.scale_log2 = scale_log2;
    if (int rc = tally_limit(W, walk_begin, walk_end, replicas, max_steps, &T.limit)) return rc;
    const int64_t bins = (int64_t)grid->nx * grid->ny + 1;
    const int64_t row_cap = WOST_TALLY_MAX_BYTES / 8 / bins / maps;   // replica rows the buffer may hold
    if (n_points > 0 && (replicas > row_cap || n_points > row_cap / replicas)) {
        if (channels)
            return fail(WOST_ERR_INVALID_ARG, "a tally of %lld points x %d replicas x %d maps x %lld bins exceeds %lld bytes",
                        (long long)n_points, (int)replicas, (int)n_maps, (long long)bins, (long long)WOST_TALLY_MAX_BYTES);
        return fail(WOST_ERR_INVALID_ARG, "a tally of %lld points x %d replicas x %lld bins exceeds %lld bytes",
                    (long long)n_points, (int)replicas, (long long)bins, (long long)WOST_TALLY_MAX_BYTES);
    }
    const size_t entries = (size_t)(n_points * replicas * maps * bins);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->d_tally.reserve(std::max<size_t>(entries, 1)));
    HIP_TRY(h->d_tally_flag.reserve(1));
    HIP_TRY(hipMemsetAsync(h->d_tally, 0, sizeof(long long) * entries, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_tally_flag, 0, sizeof(uint32_t), h->stream));
    if (channels) {   // (a blocking copy of at most 64 floats: done before any launch of the solve)
        const size_t nw = (size_t)n_maps * (size_t)h->channels();
        HIP_TRY(h->d_tally_weights.reserve(nw));
        HIP_TRY(hipMemcpy(h->d_tally_weights, weights, sizeof(float) * nw, hipMemcpyHostToDevice));
        T.n_maps = n_maps;
        T.weights = weights;
    }

    SolveRequest rq = whole_request(points, n_points, W, max_steps, eps, seed);
    rq.multi = true;
    rq.tally = &T;
    if (int rc = solve_range(h, rq, outputs(block_stats, point_stats, walk_values, walk_steps), walk_begin, walk_end))
        return rc;
    uint32_t flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, h->d_tally_flag, sizeof(flag), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (flag != 0u) {
        // flag - 1 is the largest float32 exponent field E of a scaled deposit that did not fit:
        // |d * 2^s| < 2^(E - 126). One more bit covers the rounding to the quantum.
        const int l = (int)std::ilogb((double)T.limit), E = (int)flag - 1;
        const long long rw = (long long)tally_row_walks(walk_begin, walk_end, replicas, nullptr);
        const int fit = (int)scale_log2 - (E - 126 - l + 1);
        if (E >= 255 || fit < -100)
            return fail(WOST_ERR_INVALID_ARG,
                        "tally: a deposit is infinite, NaN or beyond every quantum (at the quantum 2^%d its scaled value "
                        "has float32 exponent field %d; %lld walks x %d steps per row leave 2^%d quanta): the walks' "
                        "weights diverge, no quantum fits", -(int)scale_log2, E, rw, (int)max_steps, l);
        return fail(WOST_ERR_INVALID_ARG,
                    "tally: a deposit reached 2^%d quanta of 2^%d, the most that %lld walks x %d steps per row can sum in "
                    "64 bits; the largest deposit of this solve lies below 2^%d: pass the quantum 2^%d (scale_log2 %d) or "
                    "a coarser one", l, -(int)scale_log2, rw, (int)max_steps, E - 126 - (int)scale_log2, -fit, fit);
    }
    HIP_TRY(hipMemcpyAsync(tally, h->d_tally, sizeof(long long) * entries, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (row_walks)
        for (int64_t p = 0; p < n_points; ++p) tally_row_walks(walk_begin, walk_end, replicas, row_walks + p * replicas);
    return WOST_OK;
}

}  // namespace

extern "C" {

int wost_solve_range_tally(wost_handle* h, const float* points, int64_t n_points, int64_t W, int64_t walk_begin,
                           int64_t walk_end, int32_t max_steps, float eps, uint64_t seed, const wost_tally_grid* grid,
                           int32_t replicas, int32_t scale_log2, double* block_stats, double* point_stats,
                           float* walk_values, uint32_t* walk_steps, int64_t* tally, int64_t* row_walks) {
    return solve_tally(h, points, n_points, W, walk_begin, walk_end, max_steps, eps, seed, grid, replicas, scale_log2,
                       nullptr, 0, false, block_stats, point_stats, walk_values, walk_steps, tally, row_walks);
}

int wost_solve_range_tally_channels(wost_handle* h, const float* points, int64_t n_points, int64_t W,
                                    int64_t walk_begin, int64_t walk_end, int32_t max_steps, float eps, uint64_t seed,
                                    const wost_tally_grid* grid, int32_t replicas, int32_t scale_log2,
                                    const float* weights, int32_t n_maps, double* block_stats, double* point_stats,
                                    float* walk_values, uint32_t* walk_steps, int64_t* tally, int64_t* row_walks) {
    return solve_tally(h, points, n_points, W, walk_begin, walk_end, max_steps, eps, seed, grid, replicas, scale_log2,
                       weights, n_maps, true, block_stats, point_stats, walk_values, walk_steps, tally, row_walks);
}

int wost_solve_range_combined(wost_handle* h, const float* points, int64_t n_points, const int32_t* point_ids,
                              int64_t n_ids, int64_t W, int64_t walk_begin, int64_t walk_end, int32_t max_steps,
                              float eps, uint64_t seed, const double* weights, int32_t n_combinations,
                              double* block_stats, double* point_stats, double* channel_point_stats) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    char msg[128];
    if (combine_check_weights(weights, n_combinations, h->channels(), msg, sizeof(msg)))
        return fail(WOST_ERR_INVALID_ARG, "wost_solve_range_combined: %s", msg);
    SolveRequest rq = whole_request(points, n_points, W, max_steps, eps, seed);
    rq.multi = true;
    rq.point_ids = point_ids;
    rq.n_ids = point_ids ? n_ids : 0;
    SolveOutputs out = outputs(nullptr, channel_point_stats, nullptr, nullptr);
    out.weights = weights;
    out.n_combinations = n_combinations;
    out.combined_block_stats = block_stats;
    out.combined_point_stats = point_stats;
    return solve_range(h, rq, out, walk_begin, walk_end);
}

int wost_combine_blocks_host(const float* values, const int64_t* begin, int64_t n_blocks, int32_t n_channels,
                             const double* weights, int32_t n_combinations, double* out) {
    char msg[128];
    if (combine_check_weights(weights, n_combinations, n_channels, msg, sizeof(msg)))
        return fail(WOST_ERR_INVALID_ARG, "wost_combine_blocks_host: %s", msg);
    if (n_blocks < 0 || !begin || !out || (n_blocks > 0 && begin[n_blocks] > begin[0] && !values))
        return fail(WOST_ERR_INVALID_ARG, "wost_combine_blocks_host: bad arguments");
    for (int64_t b = 0; b < n_blocks; ++b)
        if (begin[b] < 0 || begin[b + 1] < begin[b])
            return fail(WOST_ERR_INVALID_ARG, "wost_combine_blocks_host: block %lld's range is not ascending", (long long)b);
    combine_blocks_host(values, begin, n_blocks, n_channels, weights, n_combinations, out);
    return WOST_OK;
}

int wost_last_combine_ms(const wost_handle* h, double* ms) {
    if (!h || !ms) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    *ms = h->combine_ms;
    return WOST_OK;
}

int wost_solve_history(wost_handle* h, const float* points, int64_t n_points, int64_t W, int32_t max_steps,
                       float eps, uint64_t seed, double* point_stats, float* walk_values, uint32_t* walk_steps,
                       float* records) {
    if (!records) return fail(WOST_ERR_INVALID_ARG, "NULL records");
    return solve_impl(h, whole_request(points, n_points, W, max_steps, eps, seed),
                      outputs(nullptr, point_stats, walk_values, walk_steps, records));
}

int wost_solve_multi(wost_handle* h, const float* points, int64_t n_points, int64_t W, int64_t block_begin,
                     int64_t block_end, int32_t max_steps, float eps, uint64_t seed, double* block_stats,
                     double* point_stats, float* walk_values, uint32_t* walk_steps) {
    SolveRequest rq = whole_request(points, n_points, W, max_steps, eps, seed);
    rq.multi = true;
    rq.block_begin = block_begin;
    rq.block_end = block_end;
    return solve_impl(h, rq, outputs(block_stats, point_stats, walk_values, walk_steps));
}

}  // extern "C"
