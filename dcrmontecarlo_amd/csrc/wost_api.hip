// wost_api.hip -- host side of libwost.so: the C ABI of include/wost.h (with the units
// wost_handle.h lists).
//
// Mirrors the control flow around the reference's hot loop:
//   wost_create  <- WostSolver_2D.__init__ / buildModifiedSigma (solvers/WoStSolver.py:22-138)
//   wost_solve   <- WostSolver_2D.solve / _solveUnified        (solvers/WoStSolver.py:162-353)
// Here: the handle's creation and destruction, the field, source, model, wavenumber and
// option setters, the getters and the stand-alone device queries.
#include <algorithm>
#include <cstdlib>

#include "wost_handle.h"
#include "wost_tables.h"

using namespace wost;

namespace {

int check_polyline(const wost_polyline& p, const char* name, bool required, std::vector<float>& out) {
    out.clear();
    if (!p.xy || p.n_vertices == 0) {
        if (required) return fail(WOST_ERR_INVALID_ARG, "%s polyline is required", name);
        return WOST_OK;
    }
    if (p.n_vertices < 2) return fail(WOST_ERR_INVALID_ARG, "%s polyline needs >= 2 vertices (got %d)", name, p.n_vertices);
    out.assign(p.xy, p.xy + 2 * (size_t)p.n_vertices);
    for (float v : out)
        if (!std::isfinite(v)) return fail(WOST_ERR_INVALID_ARG, "%s polyline has a non-finite coordinate", name);
    return WOST_OK;
}

// A device buffer of v's size, filled with v.
template <class T, class V>
hipError_t upload(DeviceBuffer<T>& buf, const std::vector<V>& v) {
    const hipError_t e = buf.reserve(sizeof(V) * v.size() / sizeof(T));
    return e != hipSuccess ? e : hipMemcpy(buf, v.data(), sizeof(V) * v.size(), hipMemcpyHostToDevice);
}

}  // namespace

namespace wost {

// The host half of wost_create: validation, field conversion, sigma_bar. No
// HIP call; the handle's device is -1 until wost_create takes a device.
int create_host(const wost_problem* pb, HandlePtr* out) {
    out->reset();
    if (pb->compat != WOST_COMPAT_REFERENCE && pb->compat != WOST_COMPAT_FIXED)
        return fail(WOST_ERR_INVALID_ARG, "unknown compat %d", pb->compat);
    HandlePtr h(new wost_handle());
    h->device = -1;
    int rc;
    if ((rc = check_polyline(pb->dirichlet, "dirichlet", true, h->dverts)) != WOST_OK ||
        (rc = check_polyline(pb->neumann, "neumann", false, h->nverts)) != WOST_OK ||
        (rc = convert_field(pb->boundary, h->fields[SLOT_G], "boundary")) != WOST_OK ||
        (rc = convert_field(pb->source, h->fields[SLOT_F], "source")) != WOST_OK ||
        (rc = convert_field(pb->sigma, h->fields[SLOT_SIGMA], "sigma")) != WOST_OK ||
        (rc = convert_field(pb->alpha, h->fields[SLOT_ALPHA], "alpha")) != WOST_OK)
        return rc;
    h->compat = pb->compat;
    h->dtree_usable = dirichlet_tree_usable(h->dverts.data(), (int)(h->dverts.size() / 2));
#if defined(WOST_STUDY)
    // study builds only: the tools' A/B environment (the product library reads none of it;
    // wost_set_jit / wost_set_trig / wost_set_segment_tree / wost_set_option instead)
    if (const char* e = std::getenv("WOST_JIT")) h->jit_enabled = std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("WOST_TREE_MIN_SEGMENTS")) h->tree_min_segments = std::atoi(e);
    if (const char* e = std::getenv("WOST_TRIG"))
        h->trig_mode = std::strcmp(e, "exact") == 0 ? WOST_TRIG_EXACT : std::strcmp(e, "fast") == 0 ? WOST_TRIG_FAST
                                                                                                   : WOST_TRIG_AUTO;
    if (const char* e = std::getenv("WOST_TREE_LEAF")) h->tree_leaf = std::min(32, std::max(1, std::atoi(e)));
#endif
    options_from_study_env(h->opt);
    // solvers/WoStSolver.py:54-64: any of sigma/alpha turns on delta tracking,
    // the missing one defaults to sigma = 0 / alpha = 1 (constant => Q9 fallback).
    h->delta = h->fields[SLOT_SIGMA].present || h->fields[SLOT_ALPHA].present;
    if (h->delta) {
        if (!h->fields[SLOT_ALPHA].present) {
            HostField& a = h->fields[SLOT_ALPHA];
            a.present = true;
            a.flags = WOST_FIELD_DETACHED;
            a.terms.push_back(DTerm{1.0f, 0, 0, 0});
        }
        if (!h->fields[SLOT_SIGMA].present) {
            HostField& s = h->fields[SLOT_SIGMA];
            s.present = true;
            s.terms.push_back(DTerm{0.0f, 0, 0, 0});
        }
        if (pb->sigma_bar_override > 0.0) {
            h->sigma_bar = pb->sigma_bar_override;
        } else {
            Program tmp;
            build_program(h->fields, 1.0, tmp);
            h->sigma_bar = estimate_sigma_bar(h->dverts, h->nverts, tmp);
            if (!(h->sigma_bar > 0.0))
                return fail(WOST_ERR_INVALID_ARG,
                            "sigma' could not be evaluated at any grid point (reference raises ValueError, utils.py:108-109)");
        }
    }
    *out = std::move(h);
    return WOST_OK;
}

// The handle's fields with sources[0..n) in the source slots (wost_set_sources' conversion
// and checks).
int fields_with_sources(const wost_handle* h, const wost_field* const* sources, int32_t n, HostField* out) {
    if (n < 1 || n > WOST_MAX_SOURCES || !sources)
        return fail(WOST_ERR_INVALID_ARG, "need 1..%d sources (got %d)", WOST_MAX_SOURCES, n);
    std::vector<HostField> conv(n);
    int64_t grid = 0;
    for (int s = 0; s < n; ++s) {
        if (!sources[s]) return fail(WOST_ERR_INVALID_ARG, "source %d is NULL", s);
        char name[32];
        std::snprintf(name, sizeof(name), "source[%d]", s);
        int rc = convert_field(sources[s], conv[s], name);
        if (rc != WOST_OK) return rc;
        grid += (int64_t)conv[s].grid.size();
    }
    for (int s = 0; s < N_SLOTS; ++s)
        if (s != SLOT_F) grid += (int64_t)h->fields[s].grid.size();
    for (const HostField& mf : h->model_fields) grid += (int64_t)mf.grid.size();
    if (grid >= (int64_t(1) << 24))
        return fail(WOST_ERR_INVALID_ARG, "tabulated fields hold %lld values together (limit 2^24)", (long long)grid);
    if ((int64_t)n * std::max(h->n_wavenumbers, 1) * std::max(h->n_models, 1) > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "%d sources x %d wavenumbers x %d models exceed %d channels", n,
                    std::max(h->n_wavenumbers, 1), std::max(h->n_models, 1), WOST_MAX_SOURCES);
    for (int s = 0; s < N_FIELDS; ++s) out[s] = h->fields[s];
    out[SLOT_F] = conv[0];
    for (int s = 1; s < WOST_MAX_SOURCES; ++s) out[SLOT_EXTRA + s - 1] = s < n ? conv[s] : HostField();
    return WOST_OK;
}

// The checks a model set must pass on this handle (no device).
int check_models(const wost_handle* h, int32_t n, const std::vector<HostField>& conv) {
    if (!h->delta)
        return fail(WOST_ERR_UNSUPPORTED,
                    "models need delta tracking (the conductivity enters through the walk's weights only there): "
                    "create the solver with sigma or alpha");
    if ((int64_t)n * std::max(h->n_wavenumbers, 1) * h->n_sources > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "%d models x %d wavenumbers x %d sources exceed %d channels", n,
                    std::max(h->n_wavenumbers, 1), h->n_sources, WOST_MAX_SOURCES);
    if (n >= 2 && !h->charges.empty())
        return fail(WOST_ERR_UNSUPPORTED, "several models cannot be combined with point sources (the charge buffer "
                                          "holds one alpha per charge): clear them first");
    int64_t grid = 0;
    for (const HostField& hf : conv) grid += (int64_t)hf.grid.size();
    for (int s = 0; s < N_FIELDS; ++s)
        if (s != SLOT_SIGMA && s != SLOT_ALPHA) grid += (int64_t)h->fields[s].grid.size();
    if (grid >= (int64_t(1) << 24))
        return fail(WOST_ERR_INVALID_ARG, "tabulated fields hold %lld values together (limit 2^24)", (long long)grid);
    return WOST_OK;
}

// Puts the converted models (2 n fields; n = 0: none) into the handle: model 0 into the
// program's SLOT_SIGMA / SLOT_ALPHA, the rest after the extra sources.
void install_models(wost_handle* h, int32_t n, std::vector<HostField>& conv) {
    if (h->n_models == 0) {   // keep the problem's own pair
        h->own_fields[0] = h->fields[SLOT_SIGMA];
        h->own_fields[1] = h->fields[SLOT_ALPHA];
    }
    if (n == 0) {
        h->fields[SLOT_SIGMA] = h->own_fields[0];
        h->fields[SLOT_ALPHA] = h->own_fields[1];
        h->model_fields.clear();
        h->models_sum = 0;
    } else {
        h->models_sum = models_checksum(conv);
        h->fields[SLOT_SIGMA] = std::move(conv[0]);
        h->fields[SLOT_ALPHA] = std::move(conv[1]);
        h->model_fields.assign(std::make_move_iterator(conv.begin() + 2), std::make_move_iterator(conv.end()));
    }
    h->n_models = n;
    h->prog_dirty = true;
}

}  // namespace wost

extern "C" {

int wost_version(void) { return WOST_ABI_VERSION; }

const char* wost_last_error(void) { return g_err.c_str(); }

int wost_device_count(int32_t* count) {
    if (!count) return fail(WOST_ERR_INVALID_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(WOST_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return WOST_OK;
}

int64_t wost_num_blocks(int64_t n_points, int64_t walks_per_point) {
    if (n_points <= 0 || walks_per_point <= 0) return 0;
    return n_points * ((walks_per_point + WOST_BLOCK_WALKS - 1) / WOST_BLOCK_WALKS);
}

// (also HandlePtr's deleter: a device-less handle holds no event, stream or buffer)
void wost_destroy(wost_handle* h) {
    if (!h) return;
    if (h->device >= 0) (void)hipSetDevice(h->device);
    for (hipEvent_t& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;   // (its buffers free themselves)
}

int wost_create(const wost_problem* pb, wost_handle** out) {
    if (!pb || !out) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    jit_start_identity_probe();   // (the compile helper's start, in the background)
    HandlePtr h;
    int rc = create_host(pb, &h);
    if (rc != WOST_OK) return rc;
    *out = nullptr;
    if (h->fields[SLOT_F].present || h->delta)   // the first solve's sampler nodes, meanwhile
        sampler_nodes_prefetch(sampler_kind(h.get()), h->sigma_bar);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(WOST_ERR_NO_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    if (pb->device < 0 || pb->device >= ndev)
        return fail(WOST_ERR_INVALID_ARG, "device %d out of range [0,%d)", pb->device, ndev);
    h->device = pb->device;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, h->device));
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) == hipSuccess && khz > 0)
            h->tick_khz = (double)khz;
    }
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t& ev : h->ev) HIP_TRY(hipEventCreate(&ev));
    HIP_TRY(h->d_counter.reserve(ctl_words(8192)));   // 8,192 waves: 256 CUs x 32
    HIP_TRY(hipMemset(h->d_counter, 0, sizeof(unsigned long long) * h->d_counter.capacity()));
    HIP_TRY(upload(h->d_dverts, h->dverts));
    if (!h->nverts.empty()) {
        HIP_TRY(upload(h->d_nverts, h->nverts));
        HIP_TRY(upload(h->d_seg_phi, segment_angles(h->nverts)));
    }
    if ((rc = upload_program(h.get())) != WOST_OK) return rc;
    *out = h.release();
    return WOST_OK;
}

int wost_set_field(wost_handle* h, int32_t slot, const wost_field* field) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    int s;
    if (slot == WOST_SLOT_BOUNDARY) s = SLOT_G;
    else if (slot == WOST_SLOT_SOURCE) s = SLOT_F;
    else return fail(WOST_ERR_INVALID_ARG, "unknown field slot %d", slot);
    HostField hf;
    int rc = convert_field(field, hf, s == SLOT_G ? "boundary" : "source");
    if (rc != WOST_OK) return rc;
    if (s == SLOT_F && !h->charges.empty()) {   // point sources: no source field beside them
        if (hf.present)
            return fail(WOST_ERR_INVALID_ARG, "the handle has point sources (wost_set_point_sources): clear them "
                                              "before setting a source field");
        return WOST_OK;
    }
    h->fields[s] = hf;
    if (s == SLOT_F) {   // setSourceTerm: back to a single source
        for (int k = SLOT_EXTRA; k < N_FIELDS; ++k) h->fields[k] = HostField();
        h->n_sources = 1;
    }
    h->prog_dirty = true;
    HIP_TRY(hipSetDevice(h->device));
    return upload_program(h);
}

int wost_get_info(const wost_handle* h, double* sigma_bar, int32_t* use_delta) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (sigma_bar) *sigma_bar = h->sigma_bar;
    if (use_delta) *use_delta = h->delta ? 1 : 0;
    return WOST_OK;
}

int wost_sampler_table(const wost_handle* hc, float* out, int32_t n) {
    wost_handle* h = const_cast<wost_handle*>(hc);
    if (!h || !out || n != WOST_SAMPLER_TABLE_N)
        return fail(WOST_ERR_INVALID_ARG, "need a handle and a %d-float buffer", WOST_SAMPLER_TABLE_N);
    HIP_TRY(hipSetDevice(h->device));
    int rc = ensure_table(h);
    if (rc != WOST_OK) return rc;
    std::memcpy(out, h->table.data(), sizeof(float) * WOST_SAMPLER_TABLE_N);
    return WOST_OK;
}

int wost_greens_norm(double sigma_bar, const float* radii, int64_t n, float* out) {
    if (!(sigma_bar > 0.0) || n < 0 || (n > 0 && (!radii || !out)))
        return fail(WOST_ERR_INVALID_ARG, "need sigma_bar > 0 and n >= 0 radii");
    std::vector<float4> cells(kGnormCells);
    greens_norm_cells(reinterpret_cast<float*>(cells.data()), kGnormCells, (double)kGnormCells / kGnormInvH);
    // the kernels' constants (build_program)
    const float sqrt_sb = (float)std::sqrt(sigma_bar), inv_sb = (float)(1.0 / sigma_bar);
    for (int64_t i = 0; i < n; ++i) {
        const float r = radii[i];
        out[i] = greens_norm_from_table(cells.data(), r * sqrt_sb, r, inv_sb);
    }
    return WOST_OK;
}

int wost_screened_sample_fixed(const float* s, const float* u, int64_t n, float* rho) {
    if (n < 0 || (n > 0 && (!s || !u || !rho))) return fail(WOST_ERR_INVALID_ARG, "need n >= 0 and buffers");
    const std::vector<float>& t = fixed_screened_table();
    for (int64_t i = 0; i < n; ++i) rho[i] = sample_rho_screened_fixed(t.data(), u[i], s[i]);
    return WOST_OK;
}

int wost_screened_cdf_fixed(double s, const double* rho, int64_t n, double* cdf) {
    if (!(s >= 0.0) || n < 0 || (n > 0 && (!rho || !cdf))) return fail(WOST_ERR_INVALID_ARG, "need s >= 0, n >= 0");
    for (int64_t i = 0; i < n; ++i) cdf[i] = screened_fixed_cdf(rho[i], s);
    return WOST_OK;
}

int wost_num_sources(const wost_handle* h, int32_t* n_sources) {
    if (!h || !n_sources) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    *n_sources = h->n_sources;
    return WOST_OK;
}

int wost_last_timing(const wost_handle* h, wost_timing* out) {
    if (!h || !out) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    *out = h->timing;
    return WOST_OK;
}

int wost_set_sources(wost_handle* h, const wost_field* const* sources, int32_t n) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (!h->charges.empty())
        return fail(WOST_ERR_INVALID_ARG, "the handle has point sources (wost_set_point_sources): clear them before "
                                          "setting source fields");
    std::vector<HostField> f(N_FIELDS);
    int rc = fields_with_sources(h, sources, n, f.data());
    if (rc != WOST_OK) return rc;
    for (int s = 0; s < N_FIELDS; ++s) h->fields[s] = std::move(f[s]);
    h->n_sources = n;
    h->prog_dirty = true;
    HIP_TRY(hipSetDevice(h->device));
    return upload_program(h);
}

int wost_set_models(wost_handle* h, const wost_model* models, int32_t n) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (n < 0 || (n > 0 && !models)) return fail(WOST_ERR_INVALID_ARG, "need n >= 0 models");
    std::vector<HostField> conv;
    if (n > 0) {
        if (n > WOST_MAX_SOURCES) return fail(WOST_ERR_INVALID_ARG, "%d models exceed %d channels", n, WOST_MAX_SOURCES);
        if (int rc = convert_models(models, n, &conv)) return rc;
        if (int rc = check_models(h, n, conv)) return rc;
    } else if (h->n_models == 0) {
        return WOST_OK;
    }
    // (a refused set changes nothing: the handle's state is put back when the upload fails)
    const int old_n = h->n_models;
    const uint64_t old_sum = h->models_sum;
    HostField old_pair[2] = {h->fields[SLOT_SIGMA], h->fields[SLOT_ALPHA]};
    HostField old_own[2] = {h->own_fields[0], h->own_fields[1]};
    std::vector<HostField> old_models = h->model_fields;
    install_models(h, n, conv);
    const hipError_t e = hipSetDevice(h->device);
    int rc = e == hipSuccess ? upload_program(h) : fail(WOST_ERR_HIP, "hipSetDevice failed: %s", hipGetErrorString(e));
    if (rc != WOST_OK) {
        h->n_models = old_n;
        h->models_sum = old_sum;
        h->fields[SLOT_SIGMA] = std::move(old_pair[0]);
        h->fields[SLOT_ALPHA] = std::move(old_pair[1]);
        h->own_fields[0] = std::move(old_own[0]);
        h->own_fields[1] = std::move(old_own[1]);
        h->model_fields = std::move(old_models);
        h->prog_dirty = true;   // (the next solve uploads the old program again)
    }
    return rc;
}

int wost_models_info(const wost_handle* h, int32_t* n, uint64_t* checksum) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (n) *n = h->n_models;
    if (checksum) *checksum = h->n_models > 0 ? h->models_sum : 0;
    return WOST_OK;
}

int wost_set_wavenumbers(wost_handle* h, const double* k2, int32_t n) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (n < 0 || (n > 0 && !k2)) return fail(WOST_ERR_INVALID_ARG, "need n >= 0 wavenumbers");
    if (n == 0) {
        h->n_wavenumbers = 0;
        std::fill(h->k2, h->k2 + WOST_MAX_SOURCES, 0.0f);
        return WOST_OK;
    }
    if (!h->delta)
        return fail(WOST_ERR_UNSUPPORTED,
                    "wavenumbers need delta tracking (the screening k^2 alpha enters through the collision weight): "
                    "create the solver with sigma or alpha -- a constant alpha is enough");
    if ((int64_t)n * h->n_sources * std::max(h->n_models, 1) > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "%d wavenumbers x %d sources x %d models exceed %d channels", n, h->n_sources,
                    std::max(h->n_models, 1), WOST_MAX_SOURCES);
    float v[WOST_MAX_SOURCES] = {};
    for (int j = 0; j < n; ++j) {
        if (!(k2[j] >= 0.0) || !std::isfinite(k2[j]) || !std::isfinite((float)k2[j]))
            return fail(WOST_ERR_INVALID_ARG, "k2[%d] = %g must be finite and >= 0", j, k2[j]);
        v[j] = (float)k2[j];
    }
    std::copy(v, v + WOST_MAX_SOURCES, h->k2);
    h->n_wavenumbers = n;
    return WOST_OK;
}

int wost_num_channels(const wost_handle* h, int32_t* n_channels) {
    if (!h || !n_channels) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    *n_channels = h->channels();
    return WOST_OK;
}

int wost_jit_compile(const char* source, const char* arch, int32_t in_process, uint8_t* out, int64_t capacity,
                     int64_t* length, int32_t* used_helper) {
    if (!source || !arch || !*arch || !length) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    Options opt;   // a new handle's compile options
    opt.jit_process = in_process ? 0 : 1;
    std::vector<char> code;
    std::string err;
    bool helper = false;
    if (!jit_compile_host(opt, source, arch, &code, &err, &helper))
        return fail(WOST_ERR_UNSUPPORTED, "%s", err.c_str());
    if (used_helper) *used_helper = helper ? 1 : 0;
    *length = (int64_t)code.size();
    if (out && capacity < (int64_t)code.size())
        return fail(WOST_ERR_INVALID_ARG, "capacity %lld < the code object's %lld bytes", (long long)capacity,
                    (long long)code.size());
    if (out) std::memcpy(out, code.data(), code.size());
    return WOST_OK;
}

int wost_set_segment_tree(wost_handle* h, int32_t min_segments, int32_t leaf_segments) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (leaf_segments < 0 || leaf_segments > 32) return fail(WOST_ERR_INVALID_ARG, "leaf_segments must be in [0, 32]");
    h->tree_min_segments = min_segments;
    if (leaf_segments > 0 && leaf_segments != h->tree_leaf) {
        h->tree_leaf = leaf_segments;
        h->tree_ready = false;
    }
    return WOST_OK;
}

int wost_set_dirichlet_tree(wost_handle* h, int32_t min_segments, int32_t leaf_segments) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (leaf_segments < 0 || leaf_segments > 32) return fail(WOST_ERR_INVALID_ARG, "leaf_segments must be in [0, 32]");
    h->dtree_min_segments = min_segments;
    if (leaf_segments > 0 && leaf_segments != h->dtree_leaf) {
        h->dtree_leaf = leaf_segments;
        h->dtree_ready = false;
    }
    return WOST_OK;
}

int wost_dirichlet_tree_info(const wost_handle* h, int32_t* min_segments, int32_t* leaf_segments, int32_t* usable,
                             int32_t* last_solve) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (min_segments) *min_segments = h->dtree_min_segments;
    if (leaf_segments) *leaf_segments = h->dtree_leaf;
    if (usable) *usable = h->dtree_usable ? 1 : 0;
    if (last_solve) *last_solve = h->dtree_last ? 1 : 0;
    return WOST_OK;
}

int wost_set_trig(wost_handle* h, int32_t mode) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (mode != WOST_TRIG_AUTO && mode != WOST_TRIG_EXACT && mode != WOST_TRIG_FAST)
        return fail(WOST_ERR_INVALID_ARG, "trig mode must be WOST_TRIG_AUTO, _EXACT or _FAST");
    h->trig_mode = mode;
    h->jit_fn = nullptr;
    h->jit_variant.reset();
    return WOST_OK;
}

int wost_set_fixed_step_check(wost_handle* h, int32_t enable) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    h->fixed_step_check = enable != 0;
    return WOST_OK;
}

int wost_set_jit(wost_handle* h, int32_t enable) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    h->jit_enabled = enable != 0;
    h->jit_fn = nullptr;
    h->jit_variant.reset();
    return WOST_OK;
}

int wost_set_option(wost_handle* h, const char* name, double value) {
    if (!h || !name) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    bool kernel = false;
    const int rc = options_set(h->opt, name, value, &kernel);
    if (rc == -1) return fail(WOST_ERR_INVALID_ARG, "unknown option \"%s\" (wost_options.h)", name);
    if (rc == -2) return fail(WOST_ERR_INVALID_ARG, "option \"%s\": value %g out of range", name, value);
    if (rc == -3)
        return fail(WOST_ERR_UNSUPPORTED, "option \"%s\" exists in study builds only (make study)", name);
    if (kernel) {   // the generated source changes: rebuild the handle's kernel
        h->jit_fn = nullptr;
        h->jit_variant.reset();
    }
    return WOST_OK;
}

int wost_get_option(const wost_handle* h, const char* name, double* value) {
    if (!h || !name || !value) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    if (options_get(h->opt, name, value) != 0) return fail(WOST_ERR_INVALID_ARG, "unknown option \"%s\"", name);
    return WOST_OK;
}

int wost_options_report(const wost_handle* h, char* out, int64_t capacity, int64_t* length) {
    if (!length) return fail(WOST_ERR_INVALID_ARG, "NULL length");
    Options fresh;   // without a handle: what a new handle gets (study builds: from the environment)
    options_from_study_env(fresh);
    copy_text(options_report(h ? h->opt : fresh), out, capacity, length);
    return WOST_OK;
}

int wost_eval_field(wost_handle* h, int32_t which, const float* points, int64_t n, float* out) {
    if (!h || (n > 0 && (!points || !out))) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    if (which < 0 || which > 4) return fail(WOST_ERR_INVALID_ARG, "which must be 0..4");
    if (n == 0) return WOST_OK;
    HIP_TRY(hipSetDevice(h->device));
    int rc = upload_program(h);
    if (rc != WOST_OK) return rc;
    DeviceBuffer<float2> dp;
    DeviceBuffer<float4> dout;
    HIP_TRY(dp.reserve((size_t)n));
    hipError_t e = dout.reserve((size_t)n);
    if (e == hipSuccess) e = hipMemcpyAsync(dp, points, sizeof(float2) * n, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = launch_eval_field(h->d_prog, which, dp, n, dout, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, sizeof(float4) * n, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(WOST_ERR_HIP, "wost_eval_field: %s", hipGetErrorString(e));
    return WOST_OK;
}

int wost_geometry_query(int32_t device, int32_t op, const wost_polyline* poly, const float* points,
                        const float* dirs, const float* radii, int64_t n, float* out_f, uint8_t* out_mask) {
    if (!poly || !poly->xy || poly->n_vertices < 1) return fail(WOST_ERR_INVALID_ARG, "bad polyline");
    const bool tree = (op & WOST_GEOM_TREE) != 0;
    op &= ~WOST_GEOM_TREE;
    if (op < WOST_GEOM_DISTANCE || op > WOST_GEOM_INTERSECT_POLYLINES) return fail(WOST_ERR_INVALID_ARG, "unknown op %d", op);
    if (tree && op != WOST_GEOM_DISTANCE && op != WOST_GEOM_SILHOUETTE_DISTANCE && op != WOST_GEOM_INTERSECT_POLYLINES)
        return fail(WOST_ERR_INVALID_ARG,
                    "the segment tree answers distance, silhouetteDistance and intersectPolylines only");
    const int nv = poly->n_vertices;
    if (tree && nv < 3) return fail(WOST_ERR_INVALID_ARG, "the segment tree needs >= 2 segments");
    if (tree && op == WOST_GEOM_DISTANCE && !dirichlet_tree_usable(poly->xy, nv))
        return fail(WOST_ERR_INVALID_ARG, "the distance through the segment tree needs segments of nonzero length and "
                                          "finite coordinates up to 2^60 (wost_set_dirichlet_tree)");
    if ((op == WOST_GEOM_DISTANCE || op == WOST_GEOM_RAY_INTERSECTION || op == WOST_GEOM_INTERSECT_POLYLINES) && nv < 2)
        return fail(WOST_ERR_INVALID_ARG, "op %d needs a polyline with >= 2 vertices", op);
    if (n < 0 || (n > 0 && !points)) return fail(WOST_ERR_INVALID_ARG, "bad points");
    const bool need_dirs = op == WOST_GEOM_RAY_INTERSECTION || op == WOST_GEOM_INTERSECT_POLYLINES;
    if (need_dirs && n > 0 && !dirs) return fail(WOST_ERR_INVALID_ARG, "directions required");
    if (op == WOST_GEOM_INTERSECT_POLYLINES && n > 0 && !radii) return fail(WOST_ERR_INVALID_ARG, "radii required");
    const int64_t nf_out = op == WOST_GEOM_RAY_INTERSECTION ? n * (nv - 1)
                         : op == WOST_GEOM_INTERSECT_POLYLINES ? 5 * n
                         : op == WOST_GEOM_IS_SILHOUETTE ? 0 : n;
    const int64_t nm_out = op == WOST_GEOM_IS_SILHOUETTE ? n * std::max(0, nv - 2) : 0;
    if ((nf_out > 0 && !out_f) || (nm_out > 0 && !out_mask)) return fail(WOST_ERR_INVALID_ARG, "output buffer missing");
    if (n == 0) return WOST_OK;
    SegmentTreeHost th;
    const int leaf = op == WOST_GEOM_DISTANCE ? WOST_DTREE_LEAF_DEFAULT : WOST_TREE_LEAF_DEFAULT;
    if (tree && !build_segment_tree(poly->xy, nv, leaf, &th) &&
        !build_segment_tree(poly->xy, nv, 32, &th))
        return fail(WOST_ERR_INVALID_ARG, "no segment tree for this polyline (degenerate or too long)");
    HIP_TRY(hipSetDevice(device));
    DeviceBuffer<float> drec;
    if (tree) {
        HIP_TRY(drec.reserve(std::max<size_t>(th.rec.size(), 4)));
        const hipError_t e0 = hipMemcpy(drec, th.rec.data(), sizeof(float) * th.rec.size(), hipMemcpyHostToDevice);
        if (e0 != hipSuccess) return fail(WOST_ERR_HIP, "wost_geometry_query: %s", hipGetErrorString(e0));
    }
    DeviceBuffer<float2> dv, dp, dd;
    DeviceBuffer<float> dr, df;
    DeviceBuffer<uint8_t> dm;
    hipError_t e = dv.reserve((size_t)nv);
    if (e == hipSuccess) e = dp.reserve((size_t)n);
    if (e == hipSuccess && need_dirs) e = dd.reserve((size_t)n);
    if (e == hipSuccess && op == WOST_GEOM_INTERSECT_POLYLINES) e = dr.reserve((size_t)n);
    if (e == hipSuccess) e = df.reserve((size_t)nf_out);
    if (e == hipSuccess) e = dm.reserve((size_t)nm_out);
    if (e == hipSuccess) e = hipMemcpy(dv, poly->xy, sizeof(float2) * nv, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dp, points, sizeof(float2) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && dd) e = hipMemcpy(dd, dirs, sizeof(float2) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && dr) e = hipMemcpy(dr, radii, sizeof(float) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const float* const rec = drec;
        e = tree ? launch_geometry_tree_query(op, dv, nv, reinterpret_cast<const float4*>(rec), th.first_leaf, th.depth,
                                              th.leaf, th.tol, th.kmax, dp, dd, dr, n, df, nullptr)
                 : launch_geometry_query(op, dv, nv, dp, dd, dr, n, df, dm, nullptr);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && df) e = hipMemcpy(out_f, df, sizeof(float) * nf_out, hipMemcpyDeviceToHost);
    if (e == hipSuccess && dm) e = hipMemcpy(out_mask, dm, nm_out, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(WOST_ERR_HIP, "wost_geometry_query: %s", hipGetErrorString(e));
    return WOST_OK;
}

}  // extern "C"
