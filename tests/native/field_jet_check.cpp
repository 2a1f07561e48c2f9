// TEST HARNESS -- a host build of the field interpreter (wost_device.h field_value,
// field_jet, sigma_prime_from and the sat_* predicates), called per point. Built and run by
// tests/test_field_zoo.py, which fills the records from Field.pack() and compares the
// results with a float64 autograd reference (tests/field_zoo.py).
#include <cstdint>

#include "../../dcrmontecarlo_amd/csrc/wost_device.h"

namespace {

// One factor's saturation predicate, chosen as wost_jit.cpp's sat_call chooses it:
// 0 / 1 the predicate, + 2 when a radial factor reports its centre, -1 for a kind that has
// none (the indicators count as saturated everywhere, the others never).
float factor_sat(const wost::DFactor& f, float x, float y) {
    const float* p = f.p;
    switch (f.kind) {
    case WOST_FK_SIGMOID_RADIAL: {
        bool centre = false;
        const bool s = wost::sat_sigmoid_radial(x, y, p[0], p[1], p[2], p[3], centre);
        return (s ? 1.0f : 0.0f) + (centre ? 2.0f : 0.0f);
    }
    case WOST_FK_SIGMOID_LIN: return wost::sat_sigmoid_lin(x, y, p[0], p[1], p[2]) ? 1.0f : 0.0f;
    case WOST_FK_EXP_QUAD:
        return (wost::exp_quad_is_diag(p) ? wost::sat_exp_quad_diag(x, y, p[0], p[1], p[2], p[3])
                                          : wost::sat_exp_quad(x, y, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]))
                   ? 1.0f
                   : 0.0f;
    default: return -1.0f;
    }
}

}  // namespace

// fields[0]: the field (mode 2: alpha), fields[1]: sigma of mode 2 (present = 0: sigma = 0);
// both index into terms / factors, whose grid factors index into grid.
// mode 0: out[i]      = field_value
//      1: out[4 i ..] = field_jet (v, gx, gy, lap)
//      2: out[i]      = sigma_prime_from(field_jet(alpha), field_value(sigma), alpha detached)
//      3: out[nf i + j] = factor_sat of factor j of the field, in term order (nf: the sum
//                         of its terms' factor counts)
//      4: out[0..2]   = sizeof(DTerm), sizeof(DFactor), sizeof(DField)
extern "C" int field_jet_check(const wost::DTerm* terms, const wost::DFactor* factors, const float* grid,
                               const wost::DField* fields, const float* pts, int64_t n, int mode, float* out) {
    if (mode == 4) {
        out[0] = (float)sizeof(wost::DTerm);
        out[1] = (float)sizeof(wost::DFactor);
        out[2] = (float)sizeof(wost::DField);
        return 0;
    }
    if (mode < 0 || mode > 4) return 1;
    const wost::DField fd = fields[0];
    int nf = 0;
    for (int t = 0; t < fd.n_terms; ++t) nf += terms[fd.first_term + t].nf;
    for (int64_t i = 0; i < n; ++i) {
        const float x = pts[2 * i], y = pts[2 * i + 1];
        if (mode == 0) {
            out[i] = wost::field_value(fd, terms, factors, grid, x, y);
        } else if (mode == 1) {
            const wost::Jet j = wost::field_jet(fd, terms, factors, grid, x, y);
            out[4 * i] = j.v;
            out[4 * i + 1] = j.gx;
            out[4 * i + 2] = j.gy;
            out[4 * i + 3] = j.lap;
        } else if (mode == 2) {
            const wost::Jet a = wost::field_jet(fd, terms, factors, grid, x, y);
            const float s = fields[1].present ? wost::field_value(fields[1], terms, factors, grid, x, y) : 0.0f;
            out[i] = wost::sigma_prime_from(a, s, (fd.flags & WOST_FIELD_DETACHED) != 0);
        } else {
            int j = 0;
            for (int t = 0; t < fd.n_terms; ++t) {
                const wost::DTerm tm = terms[fd.first_term + t];
                for (int k = 0; k < tm.nf; ++k) out[(int64_t)nf * i + j++] = factor_sat(factors[tm.first + k], x, y);
            }
        }
    }
    return 0;
}
