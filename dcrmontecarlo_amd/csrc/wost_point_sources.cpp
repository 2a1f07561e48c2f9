// wost_point_sources.cpp -- point sources: the host's geometry (which Neumann segment a
// point lies on, which side of it is the domain), wost_set_point_sources and its checks,
// and the closed forms the tests pin the kernels to.
#include <algorithm>

#include "wost_handle.h"

namespace wost {

// The Neumann segment(s) the point lies on: up to two (a vertex), -1 for none. "On" is
// within 2^-21 of the summed coordinate magnitudes (a couple of float32 ulps).
void segments_at(const float* nv, int nn, float x, float y, int32_t* s0, int32_t* s1) {
    *s0 = *s1 = -1;
    for (int i = 0; i + 1 < nn; ++i) {
        const double ax = nv[2 * i], ay = nv[2 * i + 1], bx = nv[2 * i + 2], by = nv[2 * i + 3];
        const double ux = bx - ax, uy = by - ay, uu = ux * ux + uy * uy;
        double t = uu > 0.0 ? ((x - ax) * ux + (y - ay) * uy) / uu : 0.0;
        t = std::min(1.0, std::max(0.0, t));
        const double dx = x - (ax + t * ux), dy = y - (ay + t * uy);
        const double tol = 0x1p-21 * (std::fabs(x) + std::fabs(y) + std::fabs(ax) + std::fabs(ay) + std::fabs(bx) +
                                      std::fabs(by));
        if (std::sqrt(dx * dx + dy * dy) <= tol) {
            if (*s0 < 0) *s0 = i;
            else if (*s1 < 0) *s1 = i;
        }
    }
}

namespace {

// Even-odd test of (x, y) against the closed curve the Dirichlet and Neumann polylines form.
bool inside_domain(const wost_handle* h, double x, double y) {
    bool in = false;
    auto scan = [&](const std::vector<float>& v) {
        for (size_t i = 0; i + 3 < v.size(); i += 2) {
            const double ax = v[i], ay = v[i + 1], bx = v[i + 2], by = v[i + 3];
            if ((ay > y) != (by > y) && x < ax + (y - ay) * (bx - ax) / (by - ay)) in = !in;
        }
    };
    scan(h->dverts);
    scan(h->nverts);
    return in;
}

// FNV-1a 64 of the charges and their source count.
uint64_t charges_checksum(const wost_handle* h) {
    if (h->charges.empty()) return 0;
    Fnv1a sum;
    const int32_t ns = h->n_sources;
    sum.eat(&ns, sizeof(ns));
    for (const wost_point_charge& c : h->charges) {
        sum.eat(&c.x, sizeof(float)); sum.eat(&c.y, sizeof(float)); sum.eat(&c.strength, sizeof(float));
        sum.eat(&c.source, sizeof(int32_t));
    }
    return sum.h;
}

}  // namespace

// boundary_code of a point on Neumann segment seg: which of its normals points into the
// domain, from even-odd tests a thousandth of its length off its midpoint. 0 when the two
// sides do not differ (the polylines do not close the domain).
int32_t code_of_segment(const wost_handle* h, int seg) {
    const double ax = h->nverts[2 * seg], ay = h->nverts[2 * seg + 1];
    const double bx = h->nverts[2 * seg + 2], by = h->nverts[2 * seg + 3];
    const double mx = 0.5 * (ax + bx), my = 0.5 * (ay + by), d = 1e-3;
    const double lx = -(by - ay) * d, ly = (bx - ax) * d;   // the left normal, scaled
    const bool left = inside_domain(h, mx + lx, my + ly), right = inside_domain(h, mx - lx, my - ly);
    if (left == right) return 0;
    return boundary_code(seg, right);
}

// wost_set_point_sources' argument checks (shared with wost_kernel_source_points, which has
// counts only: charges == nullptr skips the per-charge checks).
int check_point_sources(const wost_handle* h, const wost_point_charge* charges, int32_t n, int32_t n_sources) {
    if (h->compat != WOST_COMPAT_FIXED)
        return fail(WOST_ERR_UNSUPPORTED,
                    "point sources need compat=\"fixed\": the reference estimator ties the source sample to the step's "
                    "direction (Q13) and draws it without the Jacobian (Q3), so it has no exact counterpart");
    if (n > WOST_MAX_POINT_CHARGES)
        return fail(WOST_ERR_INVALID_ARG, "%d point charges exceed %d per launch", n, WOST_MAX_POINT_CHARGES);
    if (n_sources < 1 || n_sources > n)
        return fail(WOST_ERR_INVALID_ARG, "need 1 <= n_sources <= n (every source has a charge), got %d sources of %d "
                                          "charges", n_sources, n);
    if (h->n_models >= 2)
        return fail(WOST_ERR_UNSUPPORTED, "point sources cannot be combined with several models (wost_set_models; the "
                                          "charge buffer holds one alpha per charge): clear the models first");
    const int nk = h->n_wavenumbers > 0 ? h->n_wavenumbers : 1;
    if ((int64_t)n_sources * nk > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "%d sources x %d wavenumbers exceed %d channels", n_sources, nk, WOST_MAX_SOURCES);
    if (h->fields[SLOT_F].present)
        return fail(WOST_ERR_INVALID_ARG, "the handle has a source field: point sources cannot be mixed with it "
                                          "(create the solver without a source)");
    if (!charges) return WOST_OK;
    std::vector<int> count((size_t)n_sources, 0);
    for (int p = 0; p < n; ++p) {
        const wost_point_charge& c = charges[p];
        if (!std::isfinite(c.x) || !std::isfinite(c.y) || !std::isfinite(c.strength))
            return fail(WOST_ERR_INVALID_ARG, "point charge %d has a non-finite position or strength", p);
        if (c.source < 0 || c.source >= n_sources)
            return fail(WOST_ERR_INVALID_ARG, "point charge %d: source %d outside [0, %d)", p, c.source, n_sources);
        ++count[(size_t)c.source];
    }
    for (int s = 0; s < n_sources; ++s)
        if (count[(size_t)s] == 0) return fail(WOST_ERR_INVALID_ARG, "source %d has no point charge", s);
    return WOST_OK;
}

}  // namespace wost

using namespace wost;

extern "C" {

int wost_set_point_sources(wost_handle* h, const wost_point_charge* charges, int32_t n, int32_t n_sources) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (n < 0 || (n > 0 && !charges)) return fail(WOST_ERR_INVALID_ARG, "need n >= 0 point charges");
    if (n == 0) {
        if (!h->charges.empty()) h->n_sources = 1;
        h->charges.clear();
        h->charge_seg.clear();
        return WOST_OK;
    }
    if (int rc = check_point_sources(h, charges, n, n_sources)) return rc;
    std::vector<int32_t> seg(2 * (size_t)n, -1);
    const int nn = (int)(h->nverts.size() / 2);
    for (int p = 0; p < n; ++p) segments_at(h->nverts.data(), nn, charges[p].x, charges[p].y, &seg[2 * p], &seg[2 * p + 1]);
    const std::vector<wost_point_charge> old_charges = h->charges;
    const std::vector<int32_t> old_seg = h->charge_seg;
    h->charges.assign(charges, charges + n);
    h->charge_seg = seg;
    if (int rc = upload_charges(h)) {   // (a refused set changes nothing)
        h->charges = old_charges;
        h->charge_seg = old_seg;
        return rc;
    }
    for (int k = SLOT_EXTRA; k < N_FIELDS; ++k) h->fields[k] = HostField();
    h->n_sources = n_sources;
    h->prog_dirty = true;
    return upload_program(h);
}

int wost_point_sources_info(const wost_handle* h, int32_t* n, uint64_t* checksum) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (n) *n = (int32_t)h->charges.size();
    if (checksum) *checksum = charges_checksum(h);
    return WOST_OK;
}

int wost_ball_greens(double sigma_bar, const float* r, const float* R, int64_t n, float* out) {
    if (!(sigma_bar >= 0.0) || !std::isfinite(sigma_bar) || n < 0 || (n > 0 && (!r || !R || !out)))
        return fail(WOST_ERR_INVALID_ARG, "need a finite sigma_bar >= 0 and n >= 0 radii");
    const float sqrt_sb = (float)std::sqrt(sigma_bar);   // the kernels' constant (build_program)
    for (int64_t i = 0; i < n; ++i)
        out[i] = sigma_bar > 0.0 ? ball_greens_screened(r[i], R[i], sqrt_sb) : ball_greens(r[i], R[i]);
    return WOST_OK;
}

int wost_point_visible(const wost_polyline* neumann, const float* points, const int32_t* point_segments,
                       const float* charges, int64_t n, uint8_t* out) {
    if (!neumann || !neumann->xy || neumann->n_vertices < 2) return fail(WOST_ERR_INVALID_ARG, "bad polyline");
    if (n < 0 || (n > 0 && (!points || !charges || !out))) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    const int nv = neumann->n_vertices;
    const float2* v = reinterpret_cast<const float2*>(neumann->xy);
    auto nearest = [&](float ox, float oy, float ex, float ey, float len) {
        return intersect_polylines_ray(v, nv, ox, oy, ex, ey, len);
    };
    for (int64_t i = 0; i < n; ++i) {
        const int32_t code = point_segments ? point_segments[i] : 0;
        if ((code < 0 ? -(int64_t)code : (int64_t)code) > nv - 1)
            return fail(WOST_ERR_INVALID_ARG, "point %lld: segment code %d outside the polyline", (long long)i, code);
        int32_t z0, z1;
        segments_at(neumann->xy, nv, charges[2 * i], charges[2 * i + 1], &z0, &z1);
        out[i] = point_visible(v, points[2 * i], points[2 * i + 1], code, charges[2 * i], charges[2 * i + 1], z0, z1,
                               nearest) ? 1 : 0;
    }
    return WOST_OK;
}

}  // extern "C"
