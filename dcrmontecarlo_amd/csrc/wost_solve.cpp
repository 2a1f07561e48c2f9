// wost_solve.cpp -- a solve on the handle's stream: the request's checks, the per-solve
// steps and solve_impl's launch loop (wost_launch.h plans it). Everything a solve runs
// once per launch or per solve is here or inline in wost_handle.h.
// Mirrors WostSolver_2D.solve / _solveUnified (solvers/WoStSolver.py:162-353).
#include <algorithm>

#include "wost_combine.h"
#include "wost_handle.h"

using namespace wost;

namespace {

constexpr int64_t kMaxRecordBatchBytes = int64_t(1) << 30;   // device buffer of the walk recorder

// The solve's launch statistics (the walk kernel's per-wave records, wost_block_reduce)
// ride in front of the block sums in d_bstats, so that one copy brings both to the host.
constexpr int64_t kLstatsWords = 8;

// The largest float x with sqrtf(x) <= rmin (IEEE sqrt, as the kernels take it): a
// silhouette vertex at squared distance <= x makes r = max(rmin, min(dn, dd)) equal
// rmin whatever the other vertices are (silhouette_distance_tree's early stop).
float silhouette_stop2(float rmin) {
    if (!(rmin > 0.0f) || !std::isfinite(rmin)) return -1.0f;
    float x = rmin * rmin;
    while (x > 0.0f && std::sqrt(x) > rmin) x = std::nextafter(x, 0.0f);
    while (std::sqrt(std::nextafter(x, INFINITY)) <= rmin) x = std::nextafter(x, INFINITY);
    return x;
}

// A buffer of at least `need` elements.
template <class T>
int ensure_cap(DeviceBuffer<T>& buf, int64_t need) {
    const hipError_t e = buf.reserve((size_t)std::max<int64_t>(need, 0));
    if (e != hipSuccess) return fail(WOST_ERR_OOM, "hipMalloc(%lld bytes): %s", (long long)(sizeof(T) * need), hipGetErrorString(e));
    return WOST_OK;
}

// pinned host staging of at least `need` bytes
int ensure_pin(wost_handle* h, size_t need) {
    if (need <= h->h_pin.capacity()) return WOST_OK;
    // (a solve that failed mid-way may have left copies from it queued)
    if (h->h_pin) (void)hipStreamSynchronize(h->stream);
    need = std::max<size_t>(need, 4096);
    const hipError_t e = h->h_pin.reserve(need);
    if (e != hipSuccess) return fail(WOST_ERR_OOM, "hipHostMalloc(%zu bytes): %s", need, hipGetErrorString(e));
    return WOST_OK;
}

// Per-walk results of `need` walks with `ns` values each.
int ensure_workspace(wost_handle* h, int64_t need, int ns = 1) {
    hipError_t e = h->d_val.reserve((size_t)need * (size_t)ns);
    if (e == hipSuccess) e = h->d_steps.reserve((size_t)need);
    if (e != hipSuccess) return fail(WOST_ERR_OOM, "per-walk workspace of %lld walks: %s", (long long)need, hipGetErrorString(e));
    return WOST_OK;
}

// The argument checks of a solve, its ranges, and the compat="fixed" step-count refusal.
int check_request(const wost_handle* h, const SolveRequest& rq, SolveRanges* ranges) {
    const int n_src = h->n_sources;
    const int ns = h->channels();   // values per walk: channel c = j * n_src + s (wavenumber j, source s)
    const float* points = rq.points;
    const int64_t n_points = rq.n_points, W = rq.W;
    if (ns != 1 && !rq.multi)
        return fail(WOST_ERR_INVALID_ARG,
                    "the handle scores %d channels (%d sources of wost_set_sources x %d wavenumbers of "
                    "wost_set_wavenumbers x %d models of wost_set_models): use wost_solve_multi", ns, n_src,
                    std::max(h->n_wavenumbers, 1), std::max(h->n_models, 1));
    if (h->n_models > 1 && n_points > INT32_MAX)
        return fail(WOST_ERR_INVALID_ARG, "model batching takes at most 2^31 - 1 query points per solve");
    if (n_points < 0 || (n_points > 0 && !points)) return fail(WOST_ERR_INVALID_ARG, "bad points");
    if (W <= 0) return fail(WOST_ERR_INVALID_ARG, "nWalks must be >= 1 (got %lld)", (long long)W);
    if (rq.max_steps < 0) return fail(WOST_ERR_INVALID_ARG, "maxSteps must be >= 0");
    if (!(rq.eps == rq.eps)) return fail(WOST_ERR_INVALID_ARG, "eps is NaN");
    if (n_points > 0 && W > (int64_t(1) << 53) / n_points)
        return fail(WOST_ERR_INVALID_ARG, "n_points * nWalks must stay below 2^53 walks");
    char msg[512];
    if (rq.point_ids && n_points > INT32_MAX)
        return fail(WOST_ERR_INVALID_ARG, "a point list takes at most 2^31 - 1 query points per solve");
    if (int rc = plan_ranges(n_points, W, rq.block_begin, rq.block_end, rq.walk_begin, rq.walk_end, ranges, msg,
                             sizeof(msg), rq.point_ids, rq.n_ids))
        return fail(rc, "%s", msg);
    for (int64_t i = 0; i < 2 * n_points; ++i)
        if (!std::isfinite(points[i])) return fail(WOST_ERR_INVALID_ARG, "solve point %lld is not finite", (long long)(i / 2));
    if (h->delta && !h->has_source())
        return fail(WOST_ERR_INVALID_ARG,
                    "delta tracking (sigma/alpha given) needs a source term: the reference raises "
                    "UnboundLocalError at solvers/WoStSolver.py:281 (quirk Q14)");
    if (h->compat == WOST_COMPAT_FIXED && h->delta && h->fixed_step_check && n_points > 0 && rq.max_steps > 0 &&
        h->dverts.size() >= 4) {
        // compat="fixed" delta tracking draws each collision from the ball's own screened
        // law: with R sqrt(sigma_bar) >> 1 a step moves ~2/sqrt(sigma_bar) (E[l^2] = 4 /
        // sigma_bar), so leaving a point at Dirichlet distance d takes ~d^2 sigma_bar / 4
        // steps. When that exceeds maxSteps at the median point, every walk would end
        // truncated at maxSteps (the DCR configurations: sigma_bar = 10, d ~ 100): refuse.
        std::vector<double> est((size_t)n_points);
        const auto* dv = reinterpret_cast<const float2*>(h->dverts.data());
        const int nd = (int)(h->dverts.size() / 2);
        for (int64_t i = 0; i < n_points; ++i) {
            const double d = poly_distance(dv, nd, points[2 * i], points[2 * i + 1]);
            est[(size_t)i] = d * d * h->sigma_bar / 4.0;
        }
        std::nth_element(est.begin(), est.begin() + n_points / 2, est.end());
        const double med = est[(size_t)(n_points / 2)];
        if (med > (double)rq.max_steps)
            return fail(WOST_ERR_INVALID_ARG,
                        "compat=\"fixed\" delta tracking would truncate the walks: at the median query point a walk "
                        "needs ~%.3g steps (d^2 sigma_bar / 4, sigma_bar = %g) to reach the Dirichlet boundary, "
                        "maxSteps is %d; raise maxSteps, lower sigma_bar, or disable this check "
                        "(wost_set_fixed_step_check / WostSolver_2D.set_fixed_step_check(False))",
                        med, h->sigma_bar, (int)rq.max_steps);
    }
    return WOST_OK;
}

// Pinned staging: [points | one batch's block ranges | the block sums | the point list],
// 64-byte aligned; the device holds the first two parts in one buffer of the same layout
// (h->d_points, h->d_begin), so that one copy brings the points and the first batch's block
// ranges (C2: a copy and its ~6 us gap less). The point list (wost_solve_range_points; n_sel
// ids, 0: none) has a device buffer of its own (h->d_point_list). A solve with L weighted
// combinations (crow = 2L+1 doubles per block, 0: none) adds their weights [L][C] and the
// combined block rows at the end.
struct Staging {
    float* points = nullptr;
    int64_t* begin = nullptr;
    double* bstats = nullptr;
    int32_t* ids = nullptr;
    double* cweights = nullptr;
    double* cstats = nullptr;
    size_t pts_bytes = 0, beg_bytes = 0, bs_bytes = 0, ids_bytes = 0, cw_bytes = 0, cs_bytes = 0;
};

int stage_buffers(wost_handle* h, int64_t n_points, int64_t nblk, int row, int64_t n_sel, int crow, Staging* st) {
    auto al64 = [](size_t b) { return (b + 63) / 64 * 64; };
    st->pts_bytes = al64(sizeof(float2) * (size_t)std::max<int64_t>(n_points, 1));
    st->beg_bytes = al64(sizeof(int64_t) * (size_t)(nblk + 1));
    st->bs_bytes = al64(sizeof(double) * (size_t)(kLstatsWords + row * nblk));
    st->ids_bytes = al64(sizeof(int32_t) * (size_t)std::max<int64_t>(n_sel, 0));
    st->cw_bytes = al64(sizeof(double) * (size_t)(crow > 0 ? kCombineMax * kCombineMax : 0));
    st->cs_bytes = al64(sizeof(double) * (size_t)(crow * nblk));
    const size_t dev_bytes = st->pts_bytes + st->beg_bytes;
    if (int rc = ensure_pin(h, dev_bytes + st->bs_bytes + st->ids_bytes + st->cw_bytes + st->cs_bytes)) return rc;
    if (int rc = ensure_cap(h->d_stage, (int64_t)dev_bytes)) return rc;
    char* const dev = h->d_stage;
    char* const pin = h->h_pin;
    h->d_points = reinterpret_cast<float2*>(dev);
    h->d_begin = reinterpret_cast<int64_t*>(dev + st->pts_bytes);
    st->points = reinterpret_cast<float*>(pin);
    st->begin = reinterpret_cast<int64_t*>(pin + st->pts_bytes);
    st->bstats = reinterpret_cast<double*>(pin + dev_bytes);
    st->ids = reinterpret_cast<int32_t*>(pin + dev_bytes + st->bs_bytes);
    st->cweights = reinterpret_cast<double*>(pin + dev_bytes + st->bs_bytes + st->ids_bytes);
    st->cstats = reinterpret_cast<double*>(pin + dev_bytes + st->bs_bytes + st->ids_bytes + st->cw_bytes);
    return WOST_OK;
}

// The walk kernel's arguments that hold for every launch of the solve (the batch's and the
// launch shape's are set per launch; the pools and point_alpha by the two steps below).
WalkArgs fill_walk_args(const wost_handle* h, const SolveRequest& rq, const WalkTraits& t, const KernelChoice& kc,
                        float* d_rec) {
    WalkArgs a{};
    a.points = h->d_points;
    a.dverts = h->d_dverts;
    a.nverts = h->d_nverts;
    a.seg_phi = h->d_seg_phi;
    a.table = h->d_table;
    a.prog = h->d_prog;
    a.counter = h->d_counter;
    a.walks_per_point = rq.W;
    a.nd = (int)(h->dverts.size() / 2);
    a.nn = (int)(h->nverts.size() / 2);
    a.max_steps = rq.max_steps;
    a.eps = rq.eps;
    a.rmin = rq.eps / 2.0f;
    a.key0 = (uint32_t)rq.seed;
    a.key1 = (uint32_t)(rq.seed >> 32);
    a.n_points = (int32_t)std::min<int64_t>(rq.n_points, INT32_MAX);
    a.inv_walks_per_point = 1.0 / (double)rq.W;
    a.rec = d_rec;
    a.rec_stride = (int32_t)((int64_t)rq.max_steps + 1);
    a.exact_trig = exact_trig_of(h) ? 1 : 0;
    for (int j = 0; j < h->n_wavenumbers; ++j) a.k2[j] = h->k2[j];   // (the rest 0)
    a.charges = h->charges.empty() ? nullptr : h->d_charges;
    if (t.tree) {
        const float* const rec = h->d_tree;
        a.tree = reinterpret_cast<const float4*>(rec);
        a.tree_first_leaf = h->tree.first_leaf;
        a.tree_leaf = h->tree.leaf;
        a.tree_tol = h->tree.tol;
        a.tree_stop2 = silhouette_stop2(a.rmin);
        a.tree_kmax = h->tree.kmax;
        a.tree_lds_records = kc.shape.tree_lds;
        a.tree_lds_verts = kc.shape.tree_verts;
        a.tree_depth = h->tree.depth;
    }
    if (kc.jfn && kc.shape.dtree) {   // (ensure_dtree has run: solve_impl)
        const float* const rec = h->d_dtree;
        a.dtree = reinterpret_cast<const float4*>(rec);
        a.dtree_first_leaf = h->dtree.first_leaf;
        a.dtree_depth = h->dtree.depth;
        a.dtree_leaf = h->dtree.leaf;
        a.dtree_kmax = h->dtree.kmax;
    }
    return a;
}

// walk pools of the tree kernels (wost_walk.h): near = within pool_near (default 0.1) of the
// Neumann polyline's largest extent from its bounding box; tree_pool = 0 turns them off,
// pool_slots (default 128) walks per class and workgroup
// (a parked walk holds one attenuation: launches of several wavenumbers run without pools)
int setup_pools(wost_handle* h, const WalkTraits& t, int n_src, int blocks_per_cu, WalkArgs* a) {
    const Options& O = h->opt;
    if (!t.tree || O.tree_pool == 0 || h->nverts.size() < 4 || h->n_wavenumbers > 1 || !h->charges.empty() ||
        h->n_models > 1)
        return WOST_OK;
    Box b;
    grow_box(b, h->nverts);
    const float m = (float)O.pool_near * std::max(b.x1 - b.x0, b.y1 - b.y0);
    // (study builds, tree_iter_stats: 16 counter words after each workgroup's pools)
    const int64_t words = (int64_t)pool_wg_words(n_src, O.pool_slots) + (O.tree_iter_stats ? 16 : 0);
    if (int rc = ensure_cap(h->d_pool, words * (int64_t)blocks_per_cu * h->num_cus)) return rc;
    a->pool = h->d_pool;
    a->pool_slots = O.pool_slots;
    a->pool_wg_words = (int32_t)words;
    a->pool_box = make_float4(b.x0 - m, b.y0 - m, b.x1 + m, b.y1 + m);
    if (O.tree_iter_stats)
        HIP_TRY(hipMemsetAsync(h->d_pool, 0, sizeof(uint32_t) * (size_t)(words * blocks_per_cu * h->num_cus), h->stream));
    a->pool_near_waves = O.pool_near_waves;   // (0: by majority)
    return WOST_OK;
}

// Delta tracking: alpha at the query points, with the walk kernel's fields.
int launch_point_alpha_for(wost_handle* h, const WalkTraits& t, hipFunction_t jfn, int64_t n_points, WalkArgs* a) {
    if (!t.delta || n_points <= 0) return WOST_OK;
    // (a model-batched kernel's wost_point_alpha_jit writes every model's: [models][n_points])
    const int64_t nm = jfn && h->n_models > 1 ? h->n_models : 1;
    if (int rc = ensure_cap(h->d_point_alpha, nm * n_points)) return rc;
    if (jfn) {
        const float2* pts = h->d_points;
        long long n = (long long)n_points;
        float* out = h->d_point_alpha;
        const char* prog = h->d_prog;
        void* args[] = {&prog, &pts, &n, &out};
        const int grid = (int)std::min<int64_t>((n_points + 255) / 256, 4096);
        HIP_TRY(hipModuleLaunchKernel(h->jit_alpha_fn, grid, 1, 1, 256, 1, 1, 0, h->stream, args, nullptr));
    } else {
        HIP_TRY(launch_point_alpha(h->d_prog, h->d_points, n_points, h->d_point_alpha, h->stream));
    }
    a->point_alpha = h->d_point_alpha;
    return WOST_OK;
}

// A point-source solve's per-solve data: alpha at the charges with the walk kernel's own
// fields (delta tracking; the kernel that evaluates it at the query points), and the query
// points' boundary codes (a Neumann polyline).
int setup_point_sources(wost_handle* h, const WalkTraits& t, const SolveRequest& rq, WalkArgs* a) {
    if (h->charges.empty()) return WOST_OK;
    if (t.delta) {
        if (!h->jit_alpha_fn) return fail(WOST_ERR_UNSUPPORTED, "point sources need the field-specialised kernel");
        const float2* pts = reinterpret_cast<const float2*>(h->d_charges + CHG_XY);
        long long n = (long long)h->charges.size();
        float* out = h->d_charges + CHG_ALPHA;
        const char* prog = h->d_prog;
        void* args[] = {&prog, &pts, &n, &out};
        HIP_TRY(hipModuleLaunchKernel(h->jit_alpha_fn, 1, 1, 1, 256, 1, 1, 0, h->stream, args, nullptr));
    }
    if (!t.neu || rq.n_points <= 0) return WOST_OK;
    const int nn = (int)(h->nverts.size() / 2);
    std::vector<int32_t> code((size_t)rq.n_points, 0);
    std::vector<int32_t> seg_code((size_t)std::max(nn - 1, 0), INT32_MIN);   // (each segment's, found once)
    for (int64_t i = 0; i < rq.n_points; ++i) {
        int32_t s0, s1;
        segments_at(h->nverts.data(), nn, rq.points[2 * i], rq.points[2 * i + 1], &s0, &s1);
        if (s0 < 0) continue;
        if (seg_code[s0] == INT32_MIN) seg_code[s0] = code_of_segment(h, s0);
        if (seg_code[s0] == 0)
            return fail(WOST_ERR_INVALID_ARG,
                        "solve point %lld lies on Neumann segment %d, whose inner side cannot be told: with point "
                        "sources the Dirichlet and Neumann polylines must close the domain", (long long)i, s0);
        code[(size_t)i] = seg_code[s0];
    }
    if (int rc = ensure_cap(h->d_point_code, rq.n_points)) return rc;
    HIP_TRY(hipMemcpy(h->d_point_code, code.data(), sizeof(int32_t) * code.size(), hipMemcpyHostToDevice));
    a->point_code = h->d_point_code;
    return WOST_OK;
}

// One launch's walks (wost_launch.h next_batch) in the kernel's arguments.
void set_batch_args(const wost_handle* h, const Batch& b, WalkArgs* a) {
    a->wid_begin = b.wid_begin;
    a->base_pid = b.base_pid;
    a->base_off = b.base_off;
    a->small32 = b.small32;
    a->range_walks = b.range_walks;
    a->range_offset = b.range_offset;
    a->range_point0 = b.range_point0;
    a->inv_range_walks = b.inv_range_walks;
    a->out_val = h->d_val;
    a->out_steps = h->d_steps;
    a->count = b.count;
}

// One launch's shape (wost_launch.h launch_shape) in the kernel's arguments and wost_timing.
void set_shape_args(wost_handle* h, const LaunchShape& s, int block, WalkArgs* a) {
    a->chunk0 = (int32_t)s.chunk0;
    a->queue_base = s.queue_base;
    a->chunk = s.chunk;
    a->chunk_share = s.chunk_share;
    a->waves = (uint32_t)std::min<int64_t>(s.waves, INT32_MAX);
    h->timing.blocks_per_cu = (int32_t)s.bpc;
    h->timing.block_threads = block;
    h->timing.chunk0 = (int32_t)s.chunk0;
    h->timing.chunk = s.chunk;
    h->timing.adaptive = s.adaptive ? 1 : 0;
    h->timing.grid_blocks = s.grid;
}

// A control block (h->d_counter) that holds the records of `waves` waves.
int ensure_control_block(wost_handle* h, int64_t waves, WalkArgs* a) {
    if (ctl_words(waves) <= h->d_counter.capacity()) return WOST_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(h->d_counter.reserve(ctl_words(waves)));
    HIP_TRY(hipMemset(h->d_counter, 0, sizeof(unsigned long long) * ctl_words(waves)));   // synchronous
    a->counter = h->d_counter;
    return WOST_OK;
}

// The launch statistics (wost_kernels.hip reduce_wave_stats) in front of the block sums,
// wall-clock ticks.
void read_launch_stats(wost_handle* h, const double* pin_bstats) {
    unsigned long long ls[kLstatsWords];
    std::memcpy(ls, pin_bstats, sizeof(ls));
    const double ms_per_tick = 1.0 / h->tick_khz;
    h->timing.max_walk_steps = (uint32_t)std::min<unsigned long long>(ls[3], 0xFFFFFFFFull);
    h->timing.span_ms = ls[2] > ls[0] ? (double)(ls[2] - ls[0]) * ms_per_tick : 0.0;
    h->timing.tail_ms = ls[2] > ls[1] ? (double)(ls[2] - ls[1]) * ms_per_tick : 0.0;
    h->timing.last_wave_ms = (double)ls[5] * ms_per_tick;
    h->timing.last_wave_iters = (uint32_t)ls[4];
    h->timing.max_wave_iters = (uint32_t)ls[6];
}

// Study builds (vote_stats): the wave votes' counters of the field-specialised kernel
// (wost_device.h WOST_VOTE: per site the times it ran, the times a lane needed the slow
// side, the lanes that needed it), a module-scope array the waves add to at their ends.
constexpr int kVoteWords = 3 * 16;

int vote_stats_begin(const wost_handle* h, hipFunction_t jfn, void** d_votes) {
    *d_votes = nullptr;
    if (!h->opt.vote_stats || !jfn) return WOST_OK;
    size_t bytes = 0;
    if (!jit_kernel_global(jfn, "wost_vote_words", d_votes, &bytes) || bytes != sizeof(uint64_t) * kVoteWords) {
        *d_votes = nullptr;   // (a kernel from before the option was set)
        return WOST_OK;
    }
    HIP_TRY(hipMemsetAsync(*d_votes, 0, bytes, h->stream));
    return WOST_OK;
}

int dump_vote_stats(const void* d_votes) {   // (after the solve's last wait)
    if (!d_votes) return WOST_OK;
    uint64_t c[kVoteWords];
    HIP_TRY(hipMemcpy(c, d_votes, sizeof(c), hipMemcpyDeviceToHost));
    std::fprintf(stderr, "vote_stats:");
    for (int i = 0; i < kVoteWords; ++i) std::fprintf(stderr, " %llu", (unsigned long long)c[i]);
    std::fprintf(stderr, "\n");
    return WOST_OK;
}

// Study builds (tree_iter_stats): the tree queries' loop counters, summed over the workgroups.
int dump_tree_iter_stats(const wost_handle* h, const WalkArgs& a, int blocks_per_cu) {
    if (!h->opt.tree_iter_stats || a.pool == nullptr) return WOST_OK;
    const int64_t nwg = (int64_t)blocks_per_cu * h->num_cus;
    std::vector<uint32_t> pw((size_t)(a.pool_wg_words * nwg));
    HIP_TRY(hipMemcpy(pw.data(), a.pool, sizeof(uint32_t) * pw.size(), hipMemcpyDeviceToHost));
    const int64_t off = a.pool_wg_words - 16;
    double c[16] = {};
    for (int64_t g = 0; g < nwg; ++g)
        for (int i = 0; i < 16; ++i) c[i] += pw[(size_t)(g * a.pool_wg_words + off + i)];
    std::fprintf(stderr, "tree_iter_stats:");
    for (int i = 0; i < 16; ++i) std::fprintf(stderr, " %.0f", c[i]);
    std::fprintf(stderr, "\n");
    return WOST_OK;
}

}  // namespace

// Every solve: checks, the kernel, then one walk launch and one block reduce per batch of
// the plan (wost_launch.h), all on the handle's stream.
int wost::solve_impl(wost_handle* h, const SolveRequest& rq, const SolveOutputs& out) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    SolveRanges R;
    int rc;
    if ((rc = check_request(h, rq, &R)) != WOST_OK) return rc;
    const int n_src = h->n_sources;
    const int ns = h->channels();
    const int row = 2 * ns + 1;   // doubles per block / point row
    const int64_t n_points = rq.n_points;
    const bool listed = rq.point_ids != nullptr;   // (R.plan_points() rows then: list order)
    const WalkTraits t = walk_traits(h);

    HIP_TRY(hipSetDevice(h->device));
    if ((rc = upload_program(h)) != WOST_OK) return rc;
    if (h->has_source() && (rc = ensure_table(h)) != WOST_OK) return rc;
    if (t.tree && (rc = ensure_tree(h)) != WOST_OK) return rc;
    if (use_dtree(h) && (rc = ensure_dtree(h)) != WOST_OK) return rc;
    if (out.records && !h->charges.empty())
        return fail(WOST_ERR_UNSUPPORTED, "wost_solve_history does not record point sources (a step scores every "
                                          "charge in its ball: there is no sample point)");

    h->timing = wost_timing{};
    h->combine_ms = 0.0;
    // weighted combinations of the channels, reduced on the device after the ordinary rows
    const int L = out.weights ? out.n_combinations : 0;
    const int crow = L > 0 ? 2 * L + 1 : 0;   // doubles per combined block / point row
    if (out.weights || out.n_combinations != 0) {
        char msg[128];
        if (combine_check_weights(out.weights, out.n_combinations, ns, msg, sizeof(msg)))
            return fail(WOST_ERR_INVALID_ARG, "weighted combinations: %s", msg);
        if (out.records) return fail(WOST_ERR_UNSUPPORTED, "wost_solve_history takes no weighted combinations");
    }
    if (out.combined_point_stats)
        std::fill(out.combined_point_stats, out.combined_point_stats + (size_t)crow * rq.rows(), 0.0);
    if (out.records && listed) return fail(WOST_ERR_UNSUPPORTED, "wost_solve_history takes no point list");
    if (out.point_stats) std::fill(out.point_stats, out.point_stats + row * rq.rows(), 0.0);
    if (R.nblk == 0) return WOST_OK;

    // walks per launch: the recorder's device buffer bounds it
    int64_t batch_limit = kMaxBatchWalks / ns;
    const int64_t rec_stride = (int64_t)rq.max_steps + 1;
    const int64_t rec_walk_bytes = rec_stride * kRecFloats * (int64_t)sizeof(float);
    if (out.records) {
        batch_limit = std::min<int64_t>(kMaxBatchWalks, kMaxRecordBatchBytes / rec_walk_bytes);
        if (batch_limit < std::min<int64_t>(rq.W, WOST_BLOCK_WALKS))
            return fail(WOST_ERR_INVALID_ARG,
                        "return_history: %lld recorded steps per walk need more than %lld bytes per walk block; "
                        "lower maxSteps or nWalks", (long long)rec_stride, (long long)kMaxRecordBatchBytes);
    }
    if (R.range && R.Wr > batch_limit)
        return fail(WOST_ERR_INVALID_ARG, "walk range of %lld walks per point exceeds one launch (%lld walks)",
                    (long long)R.Wr, (long long)batch_limit);

    Staging st;
    if ((rc = stage_buffers(h, n_points, R.nblk, row, listed ? R.n_sel : 0, crow, &st)) != WOST_OK) return rc;
    std::memcpy(st.points, rq.points, sizeof(float2) * (size_t)n_points);
    if (listed) {   // the point list, through the staging (its copy is done when the solve's last wait is)
        if ((rc = ensure_cap(h->d_point_list, R.n_sel)) != WOST_OK) return rc;
        std::memcpy(st.ids, rq.point_ids, sizeof(int32_t) * (size_t)R.n_sel);
        HIP_TRY(hipMemcpyAsync(h->d_point_list, st.ids, sizeof(int32_t) * (size_t)R.n_sel, hipMemcpyHostToDevice, h->stream));
    }
    if (L > 0) {   // the weights, through the staging like the point list; the combined rows' buffer
        if ((rc = ensure_cap(h->d_cweights, kCombineMax * kCombineMax)) != WOST_OK) return rc;
        if ((rc = ensure_cap(h->d_cstats, R.nblk * crow)) != WOST_OK) return rc;
        std::memcpy(st.cweights, out.weights, sizeof(double) * (size_t)(L * ns));
        HIP_TRY(hipMemcpyAsync(h->d_cweights, st.cweights, sizeof(double) * (size_t)(L * ns), hipMemcpyHostToDevice,
                               h->stream));
    }
    // the points go with the first batch's block ranges, unless the query points' alpha
    // (delta tracking) needs them first
    bool points_pending = true;
    if (t.delta && n_points > 0) {
        HIP_TRY(hipMemcpyAsync(h->d_points, st.points, sizeof(float2) * n_points, hipMemcpyHostToDevice, h->stream));
        points_pending = false;
    }
    if ((rc = ensure_workspace(h, std::min<int64_t>(R.walks_total, batch_limit), ns)) != WOST_OK) return rc;
    if ((rc = ensure_cap(h->d_bstats, kLstatsWords + R.nblk * row)) != WOST_OK) return rc;
    // (the launch statistics in front of the block sums: one copy brings both)
    double* const d_rows = h->d_bstats + kLstatsWords;
    unsigned long long* const d_lstats = reinterpret_cast<unsigned long long*>(d_rows - kLstatsWords);
    DeviceBuffer<float> d_rec;   // the walk recorder's, for this solve
    if (out.records)
        HIP_TRY(d_rec.reserve((size_t)(std::min<int64_t>(R.walks_total, batch_limit) * rec_stride * kRecFloats)));

    KernelChoice kc;
    const int tally_maps = rq.tally ? rq.tally->n_maps : 0;   // (0: none, or the one-channel tally)
    if (rq.tally && (listed || out.records || (tally_maps > 0 ? n_src : ns) != 1 || !h->charges.empty() || !t.src))
        return fail(WOST_ERR_UNSUPPORTED, "internal: a tally takes one sampled channel (channel maps: one source), no "
                                          "point list, no recorder");
    if ((rc = choose_kernel(h, t, out.records != nullptr, n_src, ns, &kc, listed, rq.tally && tally_maps == 0,
                            tally_maps)) != WOST_OK)
        return rc;
    const int block = kc.shape.block;
    WalkArgs a = fill_walk_args(h, rq, t, kc, d_rec);
    if (listed) a.point_list = h->d_point_list;
    if (rq.tally) {   // (wost_solve_range_tally has sized and zeroed the buffers)
        const TallyRequest& T = *rq.tally;
        a.tally = h->d_tally;
        a.tally_flag = h->d_tally_flag;
        a.tally_x0 = T.grid.x0; a.tally_y0 = T.grid.y0;
        a.tally_dx = T.grid.dx; a.tally_dy = T.grid.dy;
        a.tally_inv_dx = 1.0f / T.grid.dx; a.tally_inv_dy = 1.0f / T.grid.dy;
        a.tally_nx = T.grid.nx; a.tally_ny = T.grid.ny;
        a.tally_replicas = T.replicas;
        a.tally_scale = std::ldexp(1.0f, T.scale_log2);
        a.tally_limit = (float)T.limit;
        if (tally_maps > 0) {   // (... and uploaded the weights)
            a.tally_weights = h->d_tally_weights;
            a.tally_n_weights = tally_maps * ns;
        }
    }
    // (a tally kernel runs without walk pools: a parked walk holds no tally row)
    if (!rq.tally && (rc = setup_pools(h, t, n_src, kc.blocks_per_cu, &a)) != WOST_OK) return rc;
    if ((rc = launch_point_alpha_for(h, t, kc.jfn, n_points, &a)) != WOST_OK) return rc;
    if ((rc = setup_point_sources(h, t, rq, &a)) != WOST_OK) return rc;

    LaunchIn shape_in;
    shape_in.short_walks = !t.neu;
    shape_in.tree = t.tree;
    shape_in.block = block;
    shape_in.blocks_per_cu = kc.blocks_per_cu;
    shape_in.num_cus = h->num_cus;
    shape_in.opt = &h->opt;
    shape_in.clock_is_100mhz = h->tick_khz == 100000.0;

    // study builds (vote_stats): the specialised kernel's vote counters, zeroed before the launches
    void* d_votes = nullptr;
    if ((rc = vote_stats_begin(h, kc.jfn, &d_votes)) != WOST_OK) return rc;

    Batch& b = h->batch;
    HIP_TRY(hipEventRecord(h->ev[4], h->stream));
    int64_t walks_done = 0;
    int launches = 0;
    double walk_ms = 0.0, red_ms = 0.0, comb_ms = 0.0;
    for (int64_t j = R.block_begin; j < R.block_end; j = b.j2) {
        // plan the batch: blocks [j, b.j2), b.count walks
        if (!next_batch(R, j, batch_limit, &b)) return fail(WOST_ERR_INVALID_ARG, "internal: block larger than a batch");
        const int64_t nb = b.j2 - j, count = b.count;
        set_batch_args(h, b, &a);

        // copy its block ranges
        // (the previous batch's copy from the staging has completed: its events were waited on)
        std::memcpy(st.begin, b.begins.data(), sizeof(int64_t) * (size_t)(nb + 1));
        if (points_pending) {   // points and block ranges in one copy
            HIP_TRY(hipMemcpyAsync(h->d_stage, h->h_pin, st.pts_bytes + sizeof(int64_t) * (size_t)(nb + 1),
                                   hipMemcpyHostToDevice, h->stream));
            points_pending = false;
        } else {
            HIP_TRY(hipMemcpyAsync(h->d_begin, st.begin, sizeof(int64_t) * (nb + 1), hipMemcpyHostToDevice, h->stream));
        }
        // the queue head: zeroed by the previous launch's block reduce, or here after a
        // solve that stopped between a walk launch and its reduce
        if (!h->counter_zero)
            HIP_TRY(hipMemsetAsync(h->d_counter, 0, sizeof(unsigned long long) * kCtlWords, h->stream));
        h->counter_zero = false;

        // shape the launch
        shape_in.count = count;
        const LaunchShape s = launch_shape(shape_in);
        set_shape_args(h, s, block, &a);
        if ((rc = ensure_control_block(h, s.waves, &a)) != WOST_OK) return rc;   // (more waves than it holds)

        // walk, then reduce the blocks
        HIP_TRY(hipEventRecord(h->ev[0], h->stream));
        if (kc.jfn) {
            void* args[] = {&a};
            HIP_TRY(hipModuleLaunchKernel(kc.jfn, s.grid, 1, 1, block, 1, 1, (unsigned)kc.lds, h->stream, args, nullptr));
        } else {
            HIP_TRY(launch_walk(t, a, s.grid, h->stream));
        }
        HIP_TRY(hipEventRecord(h->ev[1], h->stream));
        HIP_TRY(launch_block_reduce(h->d_val, h->d_steps, h->d_begin, nb, ns, d_rows + row * (j - R.block_begin),
                                    h->d_counter, h->stream, t.tree ? 0 : s.waves, d_lstats,
                                    launches == 0 ? 1 : 0));   // (the tree kernels keep no wave records)
        h->counter_zero = true;
        HIP_TRY(hipEventRecord(h->ev[2], h->stream));
        if (L > 0) {   // the combinations of the same per-walk values: one more read of d_val
            HIP_TRY(launch_block_combine(h->d_val, h->d_steps, h->d_begin, nb, ns, h->d_cweights, L,
                                         h->d_cstats + (size_t)crow * (j - R.block_begin), h->stream));
            HIP_TRY(hipEventRecord(h->ev[6], h->stream));
        }

        // copy out the per-walk results, and wait
        if (out.walk_values)
            HIP_TRY(hipMemcpyAsync(out.walk_values + walks_done * ns, h->d_val, sizeof(float) * count * ns,
                                   hipMemcpyDeviceToHost, h->stream));
        if (out.walk_steps)
            HIP_TRY(hipMemcpyAsync(out.walk_steps + walks_done, h->d_steps, sizeof(uint32_t) * count,
                                   hipMemcpyDeviceToHost, h->stream));
        if (out.records)
            HIP_TRY(hipMemcpyAsync(out.records + walks_done * rec_stride * kRecFloats, d_rec, (size_t)count * rec_walk_bytes,
                                   hipMemcpyDeviceToHost, h->stream));
        if (b.j2 >= R.block_end) {   // the last batch: the block sums ride the same wait
            HIP_TRY(hipMemcpyAsync(st.bstats, h->d_bstats, sizeof(double) * (kLstatsWords + row * R.nblk),
                                   hipMemcpyDeviceToHost, h->stream));
            if (L > 0)
                HIP_TRY(hipMemcpyAsync(st.cstats, h->d_cstats, sizeof(double) * (size_t)(crow * R.nblk),
                                       hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipEventRecord(h->ev[5], h->stream));
            HIP_TRY(hipEventSynchronize(h->ev[5]));
        } else {
            HIP_TRY(hipEventSynchronize(h->ev[L > 0 ? 6 : 2]));
        }
        float t0 = 0.f, t1 = 0.f;
        HIP_TRY(hipEventElapsedTime(&t0, h->ev[0], h->ev[1]));
        HIP_TRY(hipEventElapsedTime(&t1, h->ev[1], h->ev[2]));
        walk_ms += t0;
        red_ms += t1;
        if (L > 0) {
            float t2 = 0.f;
            HIP_TRY(hipEventElapsedTime(&t2, h->ev[2], h->ev[6]));
            comb_ms += t2;
        }
        ++launches;
        walks_done += count;
    }
    if ((rc = dump_tree_iter_stats(h, a, kc.blocks_per_cu)) != WOST_OK) return rc;
    if ((rc = dump_vote_stats(d_votes)) != WOST_OK) return rc;
    read_launch_stats(h, st.bstats);
    float tt = 0.f;
    HIP_TRY(hipEventElapsedTime(&tt, h->ev[4], h->ev[5]));

    const double* bs = st.bstats + kLstatsWords;   // (copied and waited for with the last batch)
    uint64_t steps_sum = 0;
    for (int64_t k = 0; k < R.nblk; ++k) {
        steps_sum += (uint64_t)bs[row * k + row - 1];
        if (out.point_stats) {
            const int64_t p = R.point_of(R.block_begin + k);
            for (int c = 0; c < row; ++c) out.point_stats[row * p + c] += bs[row * k + c];
        }
    }
    if (out.block_stats) std::memcpy(out.block_stats, bs, sizeof(double) * row * R.nblk);
    if (L > 0) {   // the combined rows: the same block order
        if (out.combined_point_stats)
            for (int64_t k = 0; k < R.nblk; ++k) {
                const int64_t p = R.point_of(R.block_begin + k);
                for (int c = 0; c < crow; ++c) out.combined_point_stats[crow * p + c] += st.cstats[crow * k + c];
            }
        if (out.combined_block_stats)
            std::memcpy(out.combined_block_stats, st.cstats, sizeof(double) * (size_t)(crow * R.nblk));
        h->combine_ms = comb_ms;
    }
    h->timing.walk_kernel_ms = walk_ms;
    h->timing.reduce_kernel_ms = red_ms;
    h->timing.total_ms = tt;
    h->timing.n_launches = launches;
    h->timing.total_steps = steps_sum;
    h->timing.total_walks = (uint64_t)R.walks_total;
    h->timing.jit_ms = kc.jit_ms;
    h->timing.jit = kc.jfn ? 1 : 0;
    h->timing.tree = t.tree ? 1 : 0;
    h->dtree_last = kc.jfn != nullptr && kc.shape.dtree;
    return WOST_OK;
}
