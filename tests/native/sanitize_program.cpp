// TEST HARNESS -- AddressSanitizer / UndefinedBehaviorSanitizer run of the device-free part
// of libwost's host half (wost_program.cpp: convert_field, build_program,
// estimate_sigma_bar, convert_models, models_checksum, segment_angles), built by
// tests/test_sanitizers.py with -fsanitize=address,undefined -fno-sanitize-recover. These
// functions take pointers and counts from outside the library and do index arithmetic on
// them. Every input array is a heap block of exactly its stated size, so a read past it is
// a finding. Links neither the HIP runtime nor hiprtc. Exits non-zero on a failed check (a
// sanitizer finding aborts the process by itself).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define WOST_PROGRAM_ONLY
#include "../../dcrmontecarlo_amd/csrc/wost_handle.h"

using namespace wost;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "check failed: %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

// A wost_field over arrays of exactly the stated sizes.
struct Field {
    std::vector<wost_term> terms;
    std::vector<wost_factor> factors;
    std::vector<float> grid;
    int flags = 0;
    wost_field view() const {
        wost_field f{};
        f.terms = terms.empty() ? nullptr : terms.data();
        f.n_terms = (int32_t)terms.size();
        f.factors = factors.empty() ? nullptr : factors.data();
        f.n_factors = (int32_t)factors.size();
        f.flags = flags;
        f.grid = grid.empty() ? nullptr : grid.data();
        f.n_grid = (int64_t)grid.size();
        return f;
    }
};

static wost_factor mono(float px, float py) {
    wost_factor f{};
    f.kind = WOST_FK_MONO;
    f.p[0] = px;
    f.p[1] = py;
    return f;
}

// an nx x ny grid factor on [0, 1]^2 whose values start at `off`
static wost_factor grid_factor(int nx, int ny, int off) {
    wost_factor f{};
    f.kind = WOST_FK_GRID;
    f.p[0] = 0.f;
    f.p[1] = 0.f;
    f.p[2] = (float)(nx - 1);
    f.p[3] = (float)(ny - 1);
    f.p[4] = (float)nx;
    f.p[5] = (float)ny;
    f.p[6] = (float)off;
    return f;
}

// 1 + x y^2
static Field monomial_field() {
    Field f;
    f.factors = {mono(1.f, 2.f)};
    f.terms = {wost_term{1.f, 0, 0}, wost_term{1.f, 0, 1}};
    return f;
}

// scale * (a 2 x 2 grid, the smallest legal one, after `off` unused values)
static Field grid_field(int off, float scale) {
    Field f;
    f.factors = {grid_factor(2, 2, off)};
    f.terms = {wost_term{scale, 0, 1}};
    f.grid.assign((size_t)off + 4, -7.f);
    for (int i = 0; i < 4; ++i) f.grid[(size_t)off + i] = 1.f + 0.25f * (float)i;
    return f;
}

// Reads everything the program's header promises.
static void check_layout(const Program& p, int n_terms, int n_factors, int n_grid) {
    const DProgram* hd = p.hdr();
    CHECK(hd->n_terms_total == n_terms);
    CHECK(hd->n_factors_total == n_factors);
    CHECK(hd->n_grid_total == n_grid);
    CHECK(p.bytes.size() == program_grid_offset(n_terms, n_factors) + sizeof(float) * (size_t)n_grid);
    auto field = [&](const DField& d) {
        CHECK(d.first_term >= 0 && d.n_terms >= 0 && d.first_term + d.n_terms <= n_terms);
        for (int t = d.first_term; t < d.first_term + d.n_terms; ++t) {
            const DTerm& tm = p.terms()[t];
            CHECK(tm.first >= 0 && tm.nf >= 0 && tm.first + tm.nf <= n_factors);
            for (int k = tm.first; k < tm.first + tm.nf; ++k) {
                const DFactor& f = p.factors()[k];
                if (f.kind != WOST_FK_GRID) continue;
                const int off = (int)f.p[6], cells = (int)f.p[4] * (int)f.p[5];
                CHECK(off >= 0 && off + cells <= n_grid);
                for (int i = 0; i < cells; ++i) CHECK(p.grid()[off + i] >= 1.f);   // (never the unused -7)
            }
        }
    };
    for (int s = 0; s < N_FIELDS; ++s) field(hd->field[s]);
    for (const DField& d : p.models) field(d);
}

int main() {
    HostField hf;
    // --- convert_field
    CHECK(convert_field(nullptr, hf, "absent") == WOST_OK && !hf.present);
    {
        const wost_field f = Field().view();   // 0 terms
        CHECK(convert_field(&f, hf, "empty") == WOST_OK);
        CHECK(hf.present && hf.terms.empty() && hf.factors.empty() && hf.grid.empty());
    }
    {
        const Field m = monomial_field();
        const wost_field f = m.view();
        CHECK(convert_field(&f, hf, "monomial") == WOST_OK);
        CHECK(hf.terms.size() == 2 && hf.factors.size() == 1 && hf.terms[1].first == 0 && hf.terms[1].nf == 1);
    }
    {
        const Field g = grid_field(3, 2.f);   // 2 x 2 at offset 3 of 7 values
        const wost_field f = g.view();
        CHECK(convert_field(&f, hf, "grid") == WOST_OK);
        CHECK(hf.grid.size() == 7 && hf.factors[0].p[6] == 3.f);
        Field shortg = g;   // offset + nx ny exceeds n_grid by one
        shortg.grid.pop_back();
        shortg.grid.shrink_to_fit();
        const wost_field f1 = shortg.view();
        g_err.clear();
        CHECK(convert_field(&f1, hf, "grid-1") == WOST_ERR_INVALID_ARG && !g_err.empty());
        CHECK(!hf.present || hf.grid.empty());
    }
    {
        Field m = monomial_field();   // a term whose factors end one past n_factors
        m.terms[1].n_factors = 2;
        const wost_field f = m.view();
        g_err.clear();
        CHECK(convert_field(&f, hf, "term+1") == WOST_ERR_INVALID_ARG && !g_err.empty());
        m.terms[1] = wost_term{1.f, 1, 1};
        const wost_field f1 = m.view();
        CHECK(convert_field(&f1, hf, "term+1") == WOST_ERR_INVALID_ARG);
    }

    // --- build_program: g monomial, f and sigma tabulated (offsets 3 and 0), alpha detached
    // constant; then two models after them
    const Field fm = monomial_field(), fg = grid_field(3, 2.f), fs = grid_field(0, 0.5f);
    Field fa;
    fa.terms = {wost_term{1.5f, 0, 0}};
    fa.flags = WOST_FIELD_DETACHED;
    std::vector<HostField> fields(N_FIELDS);
    const wost_field vg = fm.view(), vf = fg.view(), vs = fs.view(), va = fa.view();
    CHECK(convert_field(&vg, fields[SLOT_G], "g") == WOST_OK);
    CHECK(convert_field(&vf, fields[SLOT_F], "f") == WOST_OK);
    CHECK(convert_field(&vs, fields[SLOT_SIGMA], "sigma") == WOST_OK);
    CHECK(convert_field(&va, fields[SLOT_ALPHA], "alpha") == WOST_OK);
    Program prog;
    build_program(fields.data(), 2.25, prog);
    check_layout(prog, 2 + 1 + 1 + 1, 1 + 1 + 1, 7 + 4);
    CHECK(prog.models.empty());
    CHECK(prog.hdr()->sigma_bar == 2.25f && prog.hdr()->sqrt_sigma_bar == 1.5f);
    CHECK(prog.hdr()->field[SLOT_F].first_term == 2 && prog.hdr()->field[SLOT_SIGMA].first_term == 3);
    CHECK(prog.factors()[1].p[6] == 3.f && prog.factors()[2].p[6] == 7.f);   // (sigma's grid after f's 7 values)
    build_program(fields.data(), 0.0, prog);
    CHECK(prog.hdr()->inv_sigma_bar == 0.f);

    const Field m1s = grid_field(2, 1.f);
    const wost_field v1s = m1s.view();
    const wost_model models[2] = {{&vs, &va}, {&v1s, nullptr}};   // (model 1's alpha: the default 1)
    std::vector<HostField> conv;
    CHECK(convert_models(models, 2, &conv) == WOST_OK && conv.size() == 4);
    CHECK(conv[3].present && conv[3].flags == WOST_FIELD_DETACHED && conv[3].terms.size() == 1);
    const uint64_t sum = models_checksum(conv);
    CHECK(sum != 0 && sum == models_checksum(conv) && models_checksum({}) == 0);
    fields[SLOT_SIGMA] = conv[0];
    fields[SLOT_ALPHA] = conv[1];
    const std::vector<HostField> extra(conv.begin() + 2, conv.end());
    build_program(fields.data(), 2.25, prog, &extra);
    check_layout(prog, 5 + 1 + 1, 3 + 1, 11 + 6);
    CHECK(prog.models.size() == 2 && prog.models[0].first_term == 5 && prog.models[1].first_term == 6);
    CHECK(prog.factors()[3].p[6] == 11.f + 2.f);   // (model 1's sigma: its own offset 2, rebased by 11)
    const wost_model none[1] = {{nullptr, nullptr}};
    CHECK(convert_models(none, 1, &conv) == WOST_ERR_INVALID_ARG);

    // --- estimate_sigma_bar over polylines of 2 vertices (and no Neumann polyline)
    const std::vector<float> dv = {0.f, 0.f, 1.f, 1.f}, nv = {1.f, 0.f, 0.f, 1.f}, no_nv;
    for (const std::vector<float>* n : {&nv, &no_nv}) {
        const double sb = estimate_sigma_bar(dv, *n, prog);
        CHECK(std::isfinite(sb) && sb > 0.0);
    }
    CHECK(segment_angles(nv).size() == 1 && std::isfinite(segment_angles(nv)[0]));
    CHECK(segment_angles(no_nv).empty());

    std::printf("%d failed checks\n", fails);
    return fails ? 1 : 0;
}
