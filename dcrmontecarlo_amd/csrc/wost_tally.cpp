// wost_tally.cpp -- Green's function maps (wost_solve_range_tally), the part
// that needs no device: which grids are accepted, the cell rule and the fixed-point conversion
// restated for the host (wost_device.h tally_cell / tally_quantize: the kernels' own text), the
// deposit limit of a solve and the default scale.
#include <algorithm>

#include "wost_handle.h"

namespace wost {

// The grids for which tally_axis_cell's one correction step is proven (wost_device.h).
int tally_grid_check(const wost_tally_grid* g) {
    if (!g) return fail(WOST_ERR_INVALID_ARG, "NULL tally grid");
    const float lim = (float)WOST_TALLY_MAX_CELLS_1D;
    struct Axis { const char* name; float o, d; int32_t n; };
    for (const Axis& a : {Axis{"x", g->x0, g->dx, g->nx}, Axis{"y", g->y0, g->dy, g->ny}}) {
        if (a.n < 1 || a.n > WOST_TALLY_MAX_CELLS_1D)
            return fail(WOST_ERR_INVALID_ARG, "tally grid: n%s = %d, need 1..%d cells", a.name, (int)a.n,
                        (int)WOST_TALLY_MAX_CELLS_1D);
        if (!std::isfinite(a.o) || !(a.d >= 0x1p-60f) || !(a.d <= 0x1p60f))
            return fail(WOST_ERR_INVALID_ARG, "tally grid: %s0 = %g, d%s = %g: need a finite origin and 2^-60 <= d%s <= 2^60",
                        a.name, (double)a.o, a.name, (double)a.d, a.name);
        const double end = (double)a.o + (double)a.n * (double)a.d;
        if (std::max(std::fabs((double)a.o), std::fabs(end)) > (double)lim * (double)a.d)
            return fail(WOST_ERR_INVALID_ARG,
                        "tally grid: its %s edges reach %g cell widths from 0, beyond the %d for which one correction "
                        "step finds the cell: move the origin or coarsen the grid", a.name,
                        std::max(std::fabs((double)a.o), std::fabs(end)) / (double)a.d, (int)WOST_TALLY_MAX_CELLS_1D);
    }
    if ((int64_t)g->nx * g->ny + 1 > WOST_TALLY_MAX_BYTES / 8)
        return fail(WOST_ERR_INVALID_ARG, "tally grid: %lld cells exceed a buffer of %lld bytes",
                    (long long)g->nx * g->ny, (long long)WOST_TALLY_MAX_BYTES);
    return WOST_OK;
}

// The most walks of [w0, w1) that one of R rows receives, and (optional) every row's count:
// walk i goes to row (i / WOST_BLOCK_WALKS) mod R.
int64_t tally_row_walks(int64_t w0, int64_t w1, int32_t R, int64_t* rows) {
    std::vector<int64_t> cnt((size_t)R, 0);
    const int64_t B = WOST_BLOCK_WALKS;
    if (w1 > w0) {
        const int64_t b0 = w0 / B, b1 = (w1 - 1) / B;   // first and last block touched
        // whole periods of R blocks between them give every row the same count
        const int64_t nb = b1 - b0 + 1, periods = nb / R;
        for (int32_t r = 0; r < R; ++r) cnt[(size_t)r] = periods * B;
        for (int64_t b = b0 + periods * R; b <= b1; ++b) cnt[(size_t)(b % R)] += B;
        // the two partial ends
        cnt[(size_t)(b0 % R)] -= w0 - b0 * B;
        cnt[(size_t)(b1 % R)] -= (b1 + 1) * B - w1;
    }
    if (rows) std::copy(cnt.begin(), cnt.end(), rows);
    return *std::max_element(cnt.begin(), cnt.end());
}

int tally_limit(int64_t W, int64_t w0, int64_t w1, int32_t R, int32_t max_steps, int64_t* limit) {
    if (R < 1) return fail(WOST_ERR_INVALID_ARG, "replicas must be >= 1 (got %d)", (int)R);
    if (W < 1 || w0 < 0 || w1 < w0 || w1 > W) return fail(WOST_ERR_INVALID_ARG, "bad walk range");
    const double n = std::max<double>(1.0, (double)tally_row_walks(w0, w1, R, nullptr)) * std::max<double>(1.0, max_steps);
    int64_t L = int64_t(1) << 62;
    while (L > 1 && n * (double)L >= 0x1p63) L >>= 1;
    if (n * (double)L >= 0x1p63) return fail(WOST_ERR_INVALID_ARG, "a tally row would sum 2^63 or more deposits");
    *limit = L;
    return WOST_OK;
}

// The weights of a channel-map solve, float [n_maps][n_channels]: every value finite, no
// row all zero (its map would be empty).
int tally_check_weights(const float* weights, int32_t n_maps, int32_t n_channels) {
    if (n_maps < 1 || n_maps > WOST_TALLY_MAX_MAPS)
        return fail(WOST_ERR_INVALID_ARG, "channel maps: n_maps = %d, need 1..%d", (int)n_maps, WOST_TALLY_MAX_MAPS);
    if (n_channels < 1 || n_channels > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "channel maps: %d channels, need 1..%d", (int)n_channels, WOST_MAX_SOURCES);
    if (!weights) return fail(WOST_ERR_INVALID_ARG, "channel maps: NULL weights");
    for (int32_t t = 0; t < n_maps; ++t) {
        bool any = false;
        for (int32_t c = 0; c < n_channels; ++c) {
            const float w = weights[(size_t)t * n_channels + c];
            if (!std::isfinite(w))
                return fail(WOST_ERR_INVALID_ARG, "channel maps: weight [%d][%d] is not finite", (int)t, (int)c);
            any = any || w != 0.0f;
        }
        if (!any) return fail(WOST_ERR_INVALID_ARG, "channel maps: row %d of the weights is all zero", (int)t);
    }
    return WOST_OK;
}

}  // namespace wost

using namespace wost;

extern "C" {

int wost_tally_cell(const wost_tally_grid* g, const float* points, int64_t n, int32_t* out) {
    if (int rc = tally_grid_check(g)) return rc;
    if (n < 0 || (n > 0 && (!points || !out))) return fail(WOST_ERR_INVALID_ARG, "bad points");
    const float ix = 1.0f / g->dx, iy = 1.0f / g->dy;
    for (int64_t i = 0; i < n; ++i)
        out[i] = tally_cell(points[2 * i], points[2 * i + 1], g->x0, g->y0, g->dx, g->dy, ix, iy, g->nx, g->ny);
    return WOST_OK;
}

int wost_tally_quantize(const float* d, int64_t n, int32_t scale_log2, int64_t limit, int64_t* out, uint8_t* ok) {
    if (n < 0 || (n > 0 && (!d || !out || !ok))) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    if (scale_log2 < -100 || scale_log2 > 100) return fail(WOST_ERR_INVALID_ARG, "scale_log2 must be in [-100, 100]");
    if (limit < 1 || limit > (int64_t(1) << 62) || (limit & (limit - 1)) != 0)
        return fail(WOST_ERR_INVALID_ARG, "limit must be a power of two in [1, 2^62]");
    const float scale = std::ldexp(1.0f, scale_log2);
    for (int64_t i = 0; i < n; ++i) {
        long long q;
        ok[i] = tally_quantize(d[i], scale, (float)limit, &q) ? 1 : 0;
        out[i] = q;
    }
    return WOST_OK;
}

int wost_tally_check_weights(const float* weights, int32_t n_maps, int32_t n_channels) {
    return tally_check_weights(weights, n_maps, n_channels);
}

int wost_tally_weighted(const float* d, int64_t n, int32_t n_channels, const float* weights, int32_t n_maps, float* out) {
    if (n < 0 || n_channels < 1 || n_maps < 1 || !weights || (n > 0 && (!d || !out)))
        return fail(WOST_ERR_INVALID_ARG, "bad argument");
    for (int64_t i = 0; i < n; ++i)
        for (int32_t t = 0; t < n_maps; ++t)
            out[i * n_maps + t] = tally_weighted(weights + (size_t)t * n_channels, d + i * n_channels, n_channels);
    return WOST_OK;
}

int wost_tally_map_row(int64_t n_points, int32_t replicas, int32_t n_maps, int64_t bins, int64_t point, int64_t walk,
                       int32_t map, int64_t* entry) {
    if (!entry) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    if (n_points < 1 || replicas < 1 || n_maps < 1 || bins < 1 || point < 0 || point >= n_points || walk < 0 ||
        walk >= (int64_t(1) << 43) || map < 0 || map >= n_maps)
        return fail(WOST_ERR_INVALID_ARG, "bad tally shape or index");
    const int64_t cap = WOST_TALLY_MAX_BYTES / 8;
    if (bins > cap || n_maps > cap / bins || replicas > cap / bins / n_maps || n_points > cap / bins / n_maps / replicas)
        return fail(WOST_ERR_INVALID_ARG, "a tally of %lld points x %d replicas x %d maps x %lld bins exceeds %lld bytes",
                    (long long)n_points, (int)replicas, (int)n_maps, (long long)bins, (long long)WOST_TALLY_MAX_BYTES);
    const uint32_t base = tally_maps_row((uint64_t)walk, (uint32_t)point, (uint32_t)replicas, (uint32_t)n_maps, (uint32_t)bins);
    *entry = (int64_t)(base + (uint32_t)map * (uint32_t)bins);
    return WOST_OK;
}

int wost_tally_limit(int64_t W, int64_t w0, int64_t w1, int32_t R, int32_t max_steps, int64_t* limit) {
    if (!limit) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    return tally_limit(W, w0, w1, R, max_steps, limit);
}

int wost_tally_default_scale(const wost_handle* h, int64_t W, int64_t w0, int64_t w1, int32_t R, int32_t max_steps,
                             int32_t* scale_log2) {
    if (!h || !scale_log2) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    int64_t L;
    if (int rc = tally_limit(W, w0, w1, R, max_steps, &L)) return rc;
    double bound;
    if (h->delta) {
        Program built;   // (the handle's own program unless a setter has changed a field since its last solve)
        if (h->prog_dirty) build_program(h->fields, h->sigma_bar, built, &h->model_fields);
        const Program& prog = h->prog_dirty ? built : h->prog;
        bound = 1.0 / (std::max(h->sigma_bar, 1e-30) * estimate_alpha_min(h->dverts, h->nverts, prog));
    } else {
        Box b;
        grow_box(b, h->dverts);
        const double ex = (double)b.x1 - b.x0, ey = (double)b.y1 - b.y0;
        bound = (ex * ex + ey * ey) / 4.0;
    }
    if (!(bound > 0.0) || !std::isfinite(bound)) bound = 1.0;
    // the largest s with 2^16 * bound * 2^s <= L: the collision weights of a sigma_bar below
    // sigma' (signed, or above 1 where sigma' < 0) multiply up along a walk, so the head room
    // above the bound is generous; what is left below it, L / 2^16 quanta per bound (2^27 at
    // 4096 walks x 200 steps per row), still resolves a float32 deposit
    const int s = (int)std::floor(std::log2((double)L / (65536.0 * bound)));
    *scale_log2 = std::max(-100, std::min(100, s));
    return WOST_OK;
}

}  // extern "C"
