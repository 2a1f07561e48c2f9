// wost_program.cpp -- the device-free part of libwost's host half: wost_field -> HostField,
// the flattened program, sigma_bar, the model fields and the segment angles. No handle and
// no HIP call: its index arithmetic on the caller's arrays runs under the sanitizers
// (tests/native/sanitize_program.cpp).
#define WOST_PROGRAM_ONLY
#include "wost_handle.h"

#include <algorithm>

namespace wost {

int convert_field(const wost_field* in, HostField& out, const char* name) {
    out = HostField();
    if (!in) return WOST_OK;
    if (in->n_terms < 0 || in->n_factors < 0 || (in->n_terms > 0 && !in->terms) ||
        (in->n_factors > 0 && !in->factors))
        return fail(WOST_ERR_INVALID_ARG, "field %s: bad term/factor arrays", name);
    if (in->n_terms > 4096 || in->n_factors > 16384)
        return fail(WOST_ERR_INVALID_ARG, "field %s: too many terms/factors", name);
    if (in->n_grid < 0 || in->n_grid > WOST_MAX_GRID_VALUES || (in->n_grid > 0 && !in->grid))
        return fail(WOST_ERR_INVALID_ARG, "field %s: bad grid array (%lld values)", name, (long long)in->n_grid);
    out.present = true;
    out.flags = in->flags;
    for (int i = 0; i < in->n_factors; ++i) {
        const wost_factor& f = in->factors[i];
        if (f.kind < WOST_FK_MONO || f.kind > WOST_FK_GRID)
            return fail(WOST_ERR_INVALID_ARG, "field %s: factor %d has unknown kind %d", name, i, f.kind);
        if (f.kind == WOST_FK_GRID) {
            const float nx = f.p[4], ny = f.p[5], off = f.p[6];
            const bool ints = nx == std::floor(nx) && ny == std::floor(ny) && off == std::floor(off);
            if (!ints || !(nx >= 2.f && ny >= 2.f && off >= 0.f) ||
                (double)off + (double)nx * (double)ny > (double)in->n_grid)
                return fail(WOST_ERR_INVALID_ARG, "field %s: grid factor %d (%g x %g at %g) exceeds the %lld grid values",
                            name, i, nx, ny, off, (long long)in->n_grid);
            if (!(std::isfinite(f.p[0]) && std::isfinite(f.p[1]) && f.p[2] > 0.f && f.p[3] > 0.f &&
                  std::isfinite(f.p[2]) && std::isfinite(f.p[3])))
                return fail(WOST_ERR_INVALID_ARG, "field %s: grid factor %d has a bad origin or spacing", name, i);
        }
        if (f.kind == WOST_FK_MONO) {
            for (int q = 0; q < 2; ++q) {
                float e = f.p[q];
                if (!(e >= 0.f && e <= 15.f) || e != std::floor(e))
                    return fail(WOST_ERR_INVALID_ARG, "field %s: monomial exponent %g not an integer in [0,15]", name, e);
            }
        }
        DFactor d{};
        d.kind = f.kind;
        for (int q = 0; q < 8; ++q) d.p[q] = f.p[q];
        out.factors.push_back(d);
    }
    for (int t = 0; t < in->n_terms; ++t) {
        const wost_term& tm = in->terms[t];
        if (tm.n_factors < 0 || tm.first_factor < 0 || tm.first_factor + tm.n_factors > in->n_factors)
            return fail(WOST_ERR_INVALID_ARG, "field %s: term %d references factors out of range", name, t);
        DTerm d{};
        d.coef = tm.coef;
        d.first = tm.first_factor;
        d.nf = tm.n_factors;
        out.terms.push_back(d);
    }
    if (in->n_grid > 0) out.grid.assign(in->grid, in->grid + in->n_grid);
    return WOST_OK;
}

void build_program(const HostField* f, double sigma_bar, Program& out, const std::vector<HostField>* extra) {
    DProgram hdr{};
    std::vector<DTerm> terms;
    std::vector<DFactor> factors;
    std::vector<float> grid;
    auto add = [&](const HostField& hf, DField& d_) {
        d_.present = hf.present ? 1 : 0;
        d_.flags = hf.flags;
        d_.first_term = (int)terms.size();
        d_.n_terms = (int)hf.terms.size();
        const int fbase = (int)factors.size();
        const float gbase = (float)grid.size();   // exact: < 2^24 per field, checked on input
        for (DTerm t : hf.terms) {
            t.first += fbase;
            terms.push_back(t);
        }
        for (DFactor d : hf.factors) {
            if (d.kind == WOST_FK_GRID) d.p[6] += gbase;
            factors.push_back(d);
        }
        grid.insert(grid.end(), hf.grid.begin(), hf.grid.end());
    };
    for (int s = 0; s < N_FIELDS; ++s) add(f[s], hdr.field[s]);
    out.models.assign(extra ? extra->size() : 0, DField{});
    for (size_t s = 0; s < out.models.size(); ++s) add((*extra)[s], out.models[s]);
    hdr.sigma_bar = (float)sigma_bar;
    hdr.sqrt_sigma_bar = (float)std::sqrt(sigma_bar > 0 ? sigma_bar : 0.0);
    hdr.inv_sigma_bar = sigma_bar > 0 ? (float)(1.0 / sigma_bar) : 0.f;
    hdr.n_terms_total = (int)terms.size();
    hdr.n_factors_total = (int)factors.size();
    hdr.n_grid_total = (int)grid.size();
    const size_t goff = program_grid_offset(hdr.n_terms_total, hdr.n_factors_total);
    out.bytes.assign(goff + sizeof(float) * grid.size(), 0);
    std::memcpy(out.bytes.data(), &hdr, sizeof(hdr));
    if (!terms.empty())
        std::memcpy(out.bytes.data() + sizeof(DProgram), terms.data(), sizeof(DTerm) * terms.size());
    if (!factors.empty())
        std::memcpy(out.bytes.data() + sizeof(DProgram) + sizeof(DTerm) * terms.size(), factors.data(),
                    sizeof(DFactor) * factors.size());
    if (!grid.empty()) std::memcpy(out.bytes.data() + goff, grid.data(), sizeof(float) * grid.size());
}

namespace {
// torch.linspace(start, end, steps) in float32 (ATen CPU kernel: the first half
// counts up from start, the second half down from end).
std::vector<float> torch_linspace(float start, float end, int steps) {
    std::vector<float> v(steps);
    if (steps == 1) { v[0] = start; return v; }
    const float step = (end - start) / (float)(steps - 1);
    const int half = steps / 2;
    for (int i = 0; i < steps; ++i)
        v[i] = i < half ? start + step * (float)i : end - step * (float)(steps - i - 1);
    return v;
}
}  // namespace

// buildModifiedSigma's sigma_bar (solvers/WoStSolver.py:129-136 with
// utils.py:65-120): max - min of sigma' on a 50x50 ij-grid over the bounding
// box of all boundary vertices; NaN/inf samples skipped; a range <= 0 or
// > 1e3 falls back to 10.0 (quirk Q8).
double estimate_sigma_bar(const std::vector<float>& dverts, const std::vector<float>& nverts, const Program& prog) {
    Box box;
    grow_box(box, dverts);
    grow_box(box, nverts);
    const std::vector<float> gx = torch_linspace(box.x0, box.x1, 50), gy = torch_linspace(box.y0, box.y1, 50);
    const DProgram* hd = prog.hdr();
    const DField& fa = hd->field[SLOT_ALPHA];
    const DField& fs = hd->field[SLOT_SIGMA];
    const bool detached = (fa.flags & WOST_FIELD_DETACHED) != 0;
    bool any = false;
    float lo = INFINITY, hi = -INFINITY;
    for (float x : gx) {
        for (float y : gy) {
            Jet aj = field_jet(fa, prog.terms(), prog.factors(), prog.grid(), x, y);
            float sg = fs.present ? field_value(fs, prog.terms(), prog.factors(), prog.grid(), x, y) : 0.f;
            float sp = sigma_prime_from(aj, sg, detached);
            if (std::isnan(sp) || std::isinf(sp)) continue;
            any = true;
            lo = std::min(lo, sp);
            hi = std::max(hi, sp);
        }
    }
    if (!any) return NAN;
    double sb = (double)hi - (double)lo;
    if (sb <= 0.0 || sb > 1e3) sb = 10.0;
    return sb;
}

// The smallest finite positive alpha on the grid estimate_sigma_bar samples (1 without an
// alpha field or without such a sample), over the handle's alpha and those of the models
// after it (Program::models): the tally's default scale bounds a deposit with it.
double estimate_alpha_min(const std::vector<float>& dverts, const std::vector<float>& nverts, const Program& prog) {
    std::vector<const DField*> alphas;
    if (prog.hdr()->field[SLOT_ALPHA].present) alphas.push_back(&prog.hdr()->field[SLOT_ALPHA]);
    for (size_t s = 1; s < prog.models.size(); s += 2)   // (sigma, alpha) pairs of models 1..
        if (prog.models[s].present) alphas.push_back(&prog.models[s]);
    if (alphas.empty()) return 1.0;
    Box box;
    grow_box(box, dverts);
    grow_box(box, nverts);
    const std::vector<float> gx = torch_linspace(box.x0, box.x1, 50), gy = torch_linspace(box.y0, box.y1, 50);
    double lo = INFINITY;
    for (float x : gx)
        for (float y : gy)
            for (const DField* fa : alphas) {
                const float a = field_value(*fa, prog.terms(), prog.factors(), prog.grid(), x, y);
                if (std::isfinite(a) && a > 0.0f) lo = std::min(lo, (double)a);
            }
    return std::isfinite(lo) ? lo : 1.0;
}

// ---- conductivity models (wost_set_models, wost_kernel_source_models) ----

// models[0..n) converted with wost_problem's NULL rules (sigma NULL: 0; alpha NULL: the
// detached constant 1, as create_host): out[2 m] sigma, out[2 m + 1] alpha.
int convert_models(const wost_model* models, int32_t n, std::vector<HostField>* out) {
    out->assign(2 * (size_t)n, HostField());
    for (int m = 0; m < n; ++m) {
        if (!models[m].sigma && !models[m].alpha)
            return fail(WOST_ERR_INVALID_ARG, "model %d has neither sigma nor alpha", m);
        char name[40];
        HostField& sg = (*out)[2 * (size_t)m];
        HostField& al = (*out)[2 * (size_t)m + 1];
        std::snprintf(name, sizeof(name), "models[%d].sigma", m);
        if (int rc = convert_field(models[m].sigma, sg, name)) return rc;
        std::snprintf(name, sizeof(name), "models[%d].alpha", m);
        if (int rc = convert_field(models[m].alpha, al, name)) return rc;
        if (!al.present) {
            al.present = true;
            al.flags = WOST_FIELD_DETACHED;
            al.terms.push_back(DTerm{1.0f, 0, 0, 0});
        }
        if (!sg.present) {
            sg.present = true;
            sg.terms.push_back(DTerm{0.0f, 0, 0, 0});
        }
    }
    return WOST_OK;
}

// FNV-1a 64 of the converted fields: the count, then per field its flags, terms (coef,
// first, nf), factors (kind, p) and grid values. Padding never enters.
uint64_t models_checksum(const std::vector<HostField>& f) {
    if (f.empty()) return 0;
    Fnv1a sum;
    const int32_t n = (int32_t)(f.size() / 2);
    sum.eat(&n, sizeof(n));
    for (const HostField& hf : f) {
        const int32_t head[4] = {hf.flags, (int32_t)hf.terms.size(), (int32_t)hf.factors.size(), (int32_t)hf.grid.size()};
        sum.eat(head, sizeof(head));
        for (const DTerm& t : hf.terms) { sum.eat(&t.coef, 4); sum.eat(&t.first, 4); sum.eat(&t.nf, 4); }
        for (const DFactor& d : hf.factors) { sum.eat(&d.kind, 4); sum.eat(d.p, sizeof(d.p)); }
        if (!hf.grid.empty()) sum.eat(hf.grid.data(), sizeof(float) * hf.grid.size());
    }
    return sum.h;
}

// atan2 of each Neumann segment's left normal (:227-228, quirk Q2) on the host: the C
// library's atan2f is what torch.atan2 of the reference's 0-d tensors calls, and
// the device's atan2f differs from it on ~half of the C5 topography's segments
// (tools/r05/trig_compare.py), each a different direction after a Neumann hit
std::vector<float> segment_angles(const std::vector<float>& nverts) {
    const int nn = (int)(nverts.size() / 2);
    std::vector<float> phi(nn > 1 ? nn - 1 : 0);
    for (int i = 0; i + 1 < nn; ++i) {
        const float2 a{nverts[2 * i], nverts[2 * i + 1]}, b{nverts[2 * i + 2], nverts[2 * i + 3]};
        const float2 n = segment_left_normal(a, b);
        phi[i] = std::atan2(n.y, n.x);
    }
    return phi;
}

}  // namespace wost
