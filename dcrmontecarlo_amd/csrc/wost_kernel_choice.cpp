// wost_kernel_choice.cpp -- which walk kernel a solve launches: the field-specialised
// kernel's variant and source, its lookup or compile, the occupancy fallback of what the
// segment tree stages, and the entry points that hand out or prepare a kernel's source
// (wost_kernel_source*, wost_prepare_sources).
#include <algorithm>
#include <cstdlib>
#include <mutex>

#include "wost_handle.h"

namespace wost {

namespace {

// Above this many bytes of staged polylines per workgroup (4 workgroups of 256 on a
// 160 KiB CU, 4 waves per SIMD) the field-specialised kernel reads the polylines from
// global memory instead (wost_walk.h GL): long Dirichlet polylines, and long Neumann
// polylines under compat="fixed" (which scans them), work at any length.
constexpr size_t kGlobalPolylineLdsBytes = 40 * 1024;

// The source of the field-specialised kernel `v` with the program `prog` (the handle's own,
// or wost_prepare_sources' with other sources) and the handle's polylines and options.
// seg_phi: the segment angles a compiled-in Neumann polyline carries; null: the device's.
int jit_source(const wost_handle* h, const Program& prog, const KernelVariant& v, const float* seg_phi,
               std::string* src) {
    const int nn = (int)(h->nverts.size() / 2);
    std::vector<float> phi;
    if (!seg_phi && jit_const_neumann(h->opt, v.traits, nn) && nn >= 2) {
        phi.resize(nn - 1);
        HIP_TRY(hipMemcpy(phi.data(), h->d_seg_phi, sizeof(float) * phi.size(), hipMemcpyDeviceToHost));
        seg_phi = phi.data();
    }
    *src = jit_generate(h->opt, v,
                        ProgramView{prog.hdr(), prog.terms(), prog.factors(),
                                    prog.models.empty() ? nullptr : prog.models.data()},
                        PolylineView{h->dverts.data(), (int)(h->dverts.size() / 2), h->nverts.data(), nn, seg_phi});
    return WOST_OK;
}

// The field-specialised kernel `v` of the handle's program, or nullptr when it is disabled
// or could not be built (the precompiled kernel is used then; same results). *compile_ms
// grows by the host time of a compile.
hipFunction_t jit_kernel(wost_handle* h, const KernelVariant& v, double* compile_ms) {
    if (!h->jit_enabled) return nullptr;
    if (h->jit_cached(v)) return h->jit_fn;
    h->jit_fn = nullptr;
    h->jit_alpha_fn = nullptr;
    h->jit_variant = v;
    h->jit_version = h->prog_version;
    std::string src;
    if (jit_source(h, h->prog, v, nullptr, &src) != WOST_OK) return nullptr;
    std::string err;
    hipFunction_t fn = nullptr;
    hipFunction_t afn = nullptr;
    double cms = 0.0;
    const bool ok = jit_get_kernel(h->opt, h->device, src, &fn, &err, &afn, &cms);
    *compile_ms += cms;
    if (!ok) {
        h->jit_error = err;
        std::fprintf(stderr, "libwost: field-specialised kernel unavailable, using the precompiled one: %s\n",
                     err.c_str());
        return nullptr;
    }
    if (v.traits.delta && !afn) {
        h->jit_error = "the specialised module has no wost_point_alpha_jit";
        return nullptr;
    }
    h->jit_fn = fn;
    h->jit_alpha_fn = afn;
    return fn;
}

// What of the segment tree the field-specialised kernels stage in LDS, by level:
// 2 = its records and the Neumann vertices (one kTreeStageVertsBlock-thread workgroup
// per CU), 1 = its records (two kTreeStageBlock-thread workgroups per CU), 0 = nothing
// (256-thread workgroups, records and vertices through L1/L2). The option tree_lds caps
// the level (A/B; the results are the same bits at every level). Returns the records to
// stage and sets the workgroup size and the vertices to stage.
constexpr size_t kTreeLdsMaxBytes = 64 * 1024;
int tree_lds_records(const wost_handle* h, const WalkTraits& t, int level, int* block, int* verts) {
    *block = kWalkBlock;
    *verts = 0;
    if (!t.tree || !h->tree_ready) return 0;
    level = std::min(level, h->opt.tree_lds);
    const int n = h->tree.first_leaf;
    if (level <= 0 || n <= 0 || (size_t)n * 8 * sizeof(float4) > kTreeLdsMaxBytes) return 0;
    if (level >= 2) {
        *block = kTreeStageVertsBlock;
        *verts = (int)(h->nverts.size() / 2);
        return n;
    }
    *block = h->opt.tree_lds_block;
    return n;
}

// LDS bytes per workgroup of the chosen kernel
size_t lds_of(const wost_handle* h, const WalkTraits& t, const KernelChoice& kc) {
    const int nd_ = (int)(h->dverts.size() / 2);
    const bool jit = kc.jfn != nullptr;
    // option lds_pad_bytes (occupancy studies): extra bytes of LDS per workgroup
    return walk_lds_bytes({.traits = t, .nd = nd_, .nn = (int)(h->nverts.size() / 2), .tree_lds = kc.shape.tree_lds,
                           .tree_verts = kc.shape.tree_verts, .const_d = jit && jit_const_dirichlet(h->opt, nd_),
                           .global_polylines = jit && kc.shape.gpoly, .block = kc.shape.block,
                           .dirichlet_tree = jit && kc.shape.dtree}) +
           (size_t)h->opt.lds_pad_bytes;
}

std::mutex g_prepare_mu;   // wost_prepare_sources: one segment-tree build per handle

}  // namespace

// jit_kernel without blocking on a compile (option jit_race): kReady with the handle's
// kernel set, kStarted when its compile began now in the background (ticket), else kWait.
JitTry jit_kernel_try(wost_handle* h, const KernelVariant& v, JitTicket* ticket) {
    if (!h->jit_enabled) return JitTry::kWait;
    if (h->jit_cached(v) && h->jit_fn) return JitTry::kReady;
    std::string src, err;
    if (jit_source(h, h->prog, v, nullptr, &src) != WOST_OK) return JitTry::kWait;
    hipFunction_t fn = nullptr, afn = nullptr;
    const JitTry r = jit_try_kernel(h->opt, h->device, src, &fn, &afn, ticket, &err);
    if (r == JitTry::kReady && (!v.traits.delta || afn)) {
        h->jit_variant = v;
        h->jit_version = h->prog_version;
        h->jit_fn = fn;
        h->jit_alpha_fn = afn;
    }
    return r;
}

// The field-specialised kernel of that shape for walks with traits `t` that score n_sources
// sources: the one place that reads the rest of the variant off the handle.
KernelVariant kernel_variant(const wost_handle* h, const WalkTraits& t, const KernelShape& ks, bool record,
                             int n_sources, bool point_list, bool tally, int tally_maps) {
    return KernelVariant{.traits = t, .record = record, .n_sources = n_sources,
                         .n_wavenumbers = t.delta ? h->n_wavenumbers : 0,   // (0: the kernel without the k2 read)
                         .n_charges = (int)h->charges.size(), .n_models = t.delta ? h->n_models : 0,
                         .block = ks.block, .global_polylines = ks.gpoly,
                         .tree_stage = ks.stage(), .exact_trig = exact_trig_of(h), .dirichlet_tree = ks.dtree,
                         .point_list = point_list, .tally = tally, .tally_maps = tally_maps};
}

int first_kernel_shape(const wost_handle* h, const WalkTraits& t, KernelShape* ks) {
    *ks = KernelShape{};
    ks->tree_lds = h->jit_enabled ? tree_lds_records(h, t, ks->tree_level, &ks->block, &ks->tree_verts) : 0;
    // option walk_block: the workgroup of the field-specialised scan kernels (a multiple of
    // 64 up to 1024): larger workgroups share one LDS copy of the sampler and G_norm tables,
    // so more waves fit a CU than 256-thread workgroups allow (results are the same bits)
    if (h->jit_enabled && !t.tree && h->opt.walk_block > 0) ks->block = h->opt.walk_block;
    const int nd_ = (int)(h->dverts.size() / 2), nn_ = (int)(h->nverts.size() / 2);
    const Options& O = h->opt;
    // polylines whose LDS copy would cost the walk kernel its occupancy are read from
    // global memory instead (field-specialised kernels; the precompiled ones stage them)
    // (the staged tree records have their own budget, kTreeLdsMaxBytes)
    // the Dirichlet tree (field-specialised kernels): no Dirichlet vertex is staged, so a long
    // Dirichlet polyline no longer counts against the budget below
    ks->dtree = use_dtree(h);
    WalkLds lds{.traits = t, .nd = nd_, .nn = nn_, .const_d = jit_const_dirichlet(O, nd_)};
    lds.dirichlet_tree = ks->dtree;
    ks->gpoly = h->jit_enabled && walk_lds_bytes(lds) > kGlobalPolylineLdsBytes;
    // the brute-force scan of a long Neumann polyline (neumann_scan_both) reads every vertex
    // at every step: staged in LDS with one 1024-thread workgroup per CU when it fits (a
    // broadcast LDS read per vertex), else from global memory
    if (ks->gpoly && h->jit_enabled && jit_fused_neumann_scan(O, t, nn_)) {
        int cap = 0;
        HIP_TRY(hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, h->device));
        lds.block = kTreeStageVertsBlock;
        if (walk_lds_bytes(lds) <= (size_t)cap) {
            ks->gpoly = false;
            ks->block = kTreeStageVertsBlock;
        }
    }
    return WOST_OK;
}

// The kernel of a solve with the handle's fields: the field-specialised one of
// first_kernel_shape, staging less of the segment tree while what it stages costs the CU
// its waves; the precompiled one when that is disabled or could not be built.
int choose_kernel(wost_handle* h, const WalkTraits& t, bool record, int n_src, int ns, KernelChoice* kc,
                  bool point_list, bool tally, int tally_maps) {
    *kc = KernelChoice{};
    KernelShape& ks = kc->shape;
    int rc;
    if ((rc = first_kernel_shape(h, t, &ks)) != WOST_OK) return rc;
    int lds_cap = -1;
    // looks ks up and measures its occupancy
    auto lookup = [&]() -> int {
        kc->jfn = jit_kernel(h, kernel_variant(h, t, ks, record, n_src, point_list, tally, tally_maps), &kc->jit_ms);
        if (!kc->jfn) {   // the precompiled kernels run 256-thread workgroups, no staged tree, one channel
            if (tally || tally_maps > 0)   // (... and tally nothing)
                return fail(WOST_ERR_UNSUPPORTED, "a tally needs the field-specialised kernel%s%s",
                            h->jit_enabled ? ": " : " (disabled by wost_set_jit)", h->jit_error.c_str());
            if (point_list)   // (... and read no point list)
                return fail(WOST_ERR_UNSUPPORTED, "a point list needs the field-specialised kernel%s%s",
                            h->jit_enabled ? ": " : " (disabled by wost_set_jit)", h->jit_error.c_str());
            if (!h->charges.empty())
                return fail(WOST_ERR_UNSUPPORTED, "point sources need the field-specialised kernel%s%s",
                            h->jit_enabled ? ": " : " (disabled by wost_set_jit)", h->jit_error.c_str());
            if (ns > 1)
                return fail(WOST_ERR_UNSUPPORTED,
                            "multi-source, multi-wavenumber and multi-model solves need the field-specialised kernel%s%s",
                            h->jit_enabled ? ": " : " (disabled by wost_set_jit)", h->jit_error.c_str());
            ks.block = kWalkBlock;
            ks.tree_lds = ks.tree_verts = 0;
            ks.dtree = false;   // (the precompiled kernels scan the Dirichlet polyline)
        }
        kc->lds = lds_of(h, t, *kc);
        kc->blocks_per_cu = 0;
        if (lds_cap < 0)
            HIP_TRY(hipDeviceGetAttribute(&lds_cap, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, h->device));
        // a workgroup whose LDS exceeds the CU's never fits: checked here, not left to the
        // occupancy query
        if (kc->jfn && kc->lds <= (size_t)lds_cap)
            HIP_TRY(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&kc->blocks_per_cu, kc->jfn, ks.block, kc->lds));
        return WOST_OK;
    };
    if ((rc = lookup()) != WOST_OK) return rc;
    while (kc->jfn && ks.tree_lds > 0 && kc->blocks_per_cu * (ks.block / 64) < 16) {
        // what the tree stages leaves fewer than 16 waves per CU (or does not fit at all):
        // stage less (the vertices, then the records), down to reading both through L1/L2
        // from 256-thread workgroups
        ks.tree_level = ks.tree_verts > 0 ? 1 : 0;
        ks.tree_lds = tree_lds_records(h, t, ks.tree_level, &ks.block, &ks.tree_verts);
        if ((rc = lookup()) != WOST_OK) return rc;
    }
    if (!kc->jfn)
        HIP_TRY(walk_occupancy(t, (int)(h->dverts.size() / 2), (int)(h->nverts.size() / 2), &kc->blocks_per_cu));
    if (kc->blocks_per_cu < 1)
        return fail(WOST_ERR_UNSUPPORTED, "walk kernel does not fit on a CU (polylines too large for LDS: %zu bytes)",
                    kc->lds);
    return WOST_OK;
}

namespace {

// wost_kernel_source_channels, and with n_charges > 0 wost_kernel_source_points (n_sources is
// then the charges' source count, sources NULL).
int kernel_source_impl(const wost_problem* pb, const wost_field* const* sources, int32_t n_sources,
                       int32_t n_wavenumbers, int32_t n_charges, char* out, int64_t capacity, int64_t* length,
                       const wost_model* models = nullptr, int32_t n_models = 0, const char* const* opt_names = nullptr,
                       const double* opt_values = nullptr, int32_t n_options = 0, const int32_t* dtree = nullptr,
                       bool point_list = false, bool tally = false, int tally_maps = 0) {
    if (!pb || !length) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    if (n_options < 0 || (n_options > 0 && (!opt_names || !opt_values)))
        return fail(WOST_ERR_INVALID_ARG, "need n_options >= 0 names and values");
    if (n_models < 0 || n_models > WOST_MAX_SOURCES || (n_models > 0 && !models))
        return fail(WOST_ERR_INVALID_ARG, "need 0..%d models", WOST_MAX_SOURCES);
    if (n_sources < 0 || n_sources > WOST_MAX_SOURCES || (n_charges == 0 && n_sources > 0 && !sources))
        return fail(WOST_ERR_INVALID_ARG, "need 0..%d sources", WOST_MAX_SOURCES);
    if (n_wavenumbers < 0 || n_wavenumbers * std::max(n_sources, 1) > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "need sources x wavenumbers <= %d channels", WOST_MAX_SOURCES);
    HandlePtr owner;
    int rc = create_host(pb, &owner);
    if (rc != WOST_OK) return rc;
    wost_handle* h = owner.get();
    if (dtree && (rc = wost_set_dirichlet_tree(h, dtree[0], dtree[1])) != WOST_OK) return rc;
    for (int i = 0; i < n_options; ++i)   // wost_set_option, without a device
        if ((rc = wost_set_option(h, opt_names[i], opt_values[i])) != WOST_OK) return rc;
    if (n_wavenumbers > 0 && !h->delta)
        return fail(WOST_ERR_UNSUPPORTED, "wavenumbers need delta tracking: give sigma or alpha (a constant alpha is enough)");
    h->n_wavenumbers = n_wavenumbers;
    int ns = 1;
    if (n_charges > 0) {   // wost_set_point_sources' checks and counts, without a device
        if ((rc = check_point_sources(h, nullptr, n_charges, n_sources)) != WOST_OK) return rc;
        h->charges.assign((size_t)n_charges, wost_point_charge{0.f, 0.f, 0.f, 0});
        h->n_sources = ns = n_sources;
    } else if (n_sources >= 1) {   // wost_set_sources' fields, without a device
        for (int k = 0; k < n_sources; ++k) {
            HostField hf;
            if (!sources[k]) return fail(WOST_ERR_INVALID_ARG, "source %d is NULL", k);
            if ((rc = convert_field(sources[k], hf, "source")) != WOST_OK) return rc;
            h->fields[k == 0 ? SLOT_F : SLOT_EXTRA + k - 1] = hf;
        }
        ns = n_sources;
    }
    if (n_models > 0) {   // wost_set_models' fields, without a device
        h->n_sources = ns;
        std::vector<HostField> conv;
        if ((rc = convert_models(models, n_models, &conv)) != WOST_OK || (rc = check_models(h, n_models, conv)) != WOST_OK)
            return rc;
        install_models(h, n_models, conv);
    }
    build_program(h->fields, h->sigma_bar, h->prog, &h->model_fields);
    const WalkTraits t = walk_traits(h);
    // no device here: the segment angles of a compiled-in Neumann polyline come from the
    // host's atan2f (the kernels use the device's bits; this source is for offline study)
    const std::vector<float> phi = segment_angles(h->nverts);
    // the first solve's kernel without a device: 256 threads, nothing of the tree staged
    KernelShape ks0;
    ks0.dtree = use_dtree(h);
    if (tally_maps != 0 && (tally_maps < 1 || tally_maps > WOST_TALLY_MAX_MAPS))
        return fail(WOST_ERR_INVALID_ARG, "channel maps: n_maps = %d, need 1..%d", (int)tally_maps, WOST_TALLY_MAX_MAPS);
    if (tally || tally_maps > 0) {   // wost_solve_range_tally's (_channels') refusals that need no device
        if (h->compat != WOST_COMPAT_FIXED)
            return fail(WOST_ERR_UNSUPPORTED, "a tally needs compat=\"fixed\": the reference's source sample does not "
                                              "estimate the integral of G f (quirks Q3, Q13)");
        if (!h->fields[SLOT_F].present) return fail(WOST_ERR_INVALID_ARG, "a tally needs a source field on the handle");
    }
    KernelVariant v = kernel_variant(h, t, ks0, false, ns, point_list, tally, tally_maps);
    // study builds: offline study of the tree kernels' LDS staging (tools/jit_isa.py --stage):
    // the source of staging level WOST_KERNEL_SOURCE_STAGE (2: records and vertices, 1:
    // records, with the tree_lds_block workgroup) instead
#if defined(WOST_STUDY)
    if (const char* e = std::getenv("WOST_KERNEL_SOURCE_STAGE"); e && t.tree) {
        v.tree_stage = std::max(0, std::min(2, std::atoi(e)));
        v.block = v.tree_stage == 2 ? kTreeStageVertsBlock : v.tree_stage == 1 ? h->opt.tree_lds_block : kWalkBlock;
    }
#endif
    std::string src;
    if ((rc = jit_source(h, h->prog, v, phi.empty() ? nullptr : phi.data(), &src)) != WOST_OK) return rc;
    copy_text(src, out, capacity, length);
    return WOST_OK;
}

}  // namespace
}  // namespace wost

using namespace wost;

extern "C" {

int wost_kernel_source_channels(const wost_problem* pb, const wost_field* const* sources, int32_t n_sources,
                                int32_t n_wavenumbers, char* out, int64_t capacity, int64_t* length) {
    return kernel_source_impl(pb, sources, n_sources, n_wavenumbers, 0, out, capacity, length);
}

int wost_kernel_source_points(const wost_problem* pb, int32_t n_charges, int32_t n_sources, int32_t n_wavenumbers,
                              char* out, int64_t capacity, int64_t* length) {
    if (n_charges < 1) return fail(WOST_ERR_INVALID_ARG, "need n_charges >= 1");
    return kernel_source_impl(pb, nullptr, n_sources, n_wavenumbers, n_charges, out, capacity, length);
}

int wost_kernel_source_models(const wost_problem* pb, const wost_model* models, int32_t n_models,
                              const wost_field* const* sources, int32_t n_sources, int32_t n_wavenumbers, char* out,
                              int64_t capacity, int64_t* length) {
    return kernel_source_impl(pb, sources, n_sources, n_wavenumbers, 0, out, capacity, length, models, n_models);
}

int wost_kernel_source_point_list(const wost_problem* pb, const wost_model* models, int32_t n_models,
                                  const wost_field* const* sources, int32_t n_sources, int32_t n_wavenumbers,
                                  char* out, int64_t capacity, int64_t* length) {
    return kernel_source_impl(pb, sources, n_sources, n_wavenumbers, 0, out, capacity, length, models, n_models, nullptr,
                              nullptr, 0, nullptr, true);
}

int wost_kernel_source_tally(const wost_problem* pb, char* out, int64_t capacity, int64_t* length) {
    return kernel_source_impl(pb, nullptr, 0, 0, 0, out, capacity, length, nullptr, 0, nullptr, nullptr, 0, nullptr, false,
                              true);
}

int wost_kernel_source_tally_channels(const wost_problem* pb, const wost_model* models, int32_t n_models,
                                      int32_t n_wavenumbers, int32_t n_maps, char* out, int64_t capacity,
                                      int64_t* length) {
    if (n_maps < 1 || n_maps > WOST_TALLY_MAX_MAPS)
        return fail(WOST_ERR_INVALID_ARG, "channel maps: n_maps = %d, need 1..%d", (int)n_maps, WOST_TALLY_MAX_MAPS);
    return kernel_source_impl(pb, nullptr, 0, n_wavenumbers, 0, out, capacity, length, models, n_models, nullptr, nullptr,
                              0, nullptr, false, false, n_maps);
}

int wost_kernel_source_options(const wost_problem* pb, const char* const* names, const double* values,
                               int32_t n_options, char* out, int64_t capacity, int64_t* length) {
    return kernel_source_impl(pb, nullptr, 0, 0, 0, out, capacity, length, nullptr, 0, names, values, n_options);
}

int wost_kernel_source_dirichlet_tree(const wost_problem* pb, int32_t min_segments, int32_t leaf_segments,
                                      int32_t n_charges, int32_t n_sources, char* out, int64_t capacity,
                                      int64_t* length) {
    if (n_charges < 0) return fail(WOST_ERR_INVALID_ARG, "need n_charges >= 0");
    const int32_t dtree[2] = {min_segments, leaf_segments};
    return kernel_source_impl(pb, nullptr, n_charges > 0 ? n_sources : 0, 0, n_charges, out, capacity, length, nullptr, 0,
                              nullptr, nullptr, 0, dtree);
}

int wost_kernel_source_sources(const wost_problem* pb, const wost_field* const* sources, int32_t n_sources,
                               char* out, int64_t capacity, int64_t* length) {
    return wost_kernel_source_channels(pb, sources, n_sources, 0, out, capacity, length);
}

int wost_kernel_source(const wost_problem* pb, char* out, int64_t capacity, int64_t* length) {
    return wost_kernel_source_sources(pb, nullptr, 0, out, capacity, length);
}

int wost_prepare_sources(wost_handle* h, const wost_field* const* sources, int32_t n, int64_t n_points) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (n_points < 1) return fail(WOST_ERR_INVALID_ARG, "n_points must be >= 1 (got %lld)", (long long)n_points);
    if (!h->charges.empty())
        return fail(WOST_ERR_INVALID_ARG, "the handle has point sources (wost_set_point_sources): clear them first");
    std::vector<HostField> f(N_FIELDS);
    int rc = fields_with_sources(h, sources, n, f.data());
    if (rc != WOST_OK) return rc;
    if (!h->jit_enabled)
        return fail(WOST_ERR_UNSUPPORTED, "multi-source solves need the field-specialised kernel (disabled by wost_set_jit)");
    Program prog;
    build_program(f.data(), h->sigma_bar, prog, &h->model_fields);
    const WalkTraits t = walk_traits(h, f[SLOT_F].present);
    HIP_TRY(hipSetDevice(h->device));
    if (t.tree) {   // the staging choice depends on the tree's size
        std::lock_guard<std::mutex> lock(g_prepare_mu);
        if ((rc = ensure_tree(h)) != WOST_OK) return rc;
    }
    KernelShape ks;
    if ((rc = first_kernel_shape(h, t, &ks)) != WOST_OK) return rc;
    std::string src, err;
    if ((rc = jit_source(h, prog, kernel_variant(h, t, ks, false, n), nullptr, &src)) != WOST_OK) return rc;
    hipFunction_t fn = nullptr;
    if (!jit_get_kernel(h->opt, h->device, src, &fn, &err, nullptr, nullptr))
        return fail(WOST_ERR_UNSUPPORTED, "field-specialised kernel unavailable: %s", err.c_str());
    return WOST_OK;
}

}  // extern "C"
