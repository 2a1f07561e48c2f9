// wost_api.hip -- host side of libwost.so: the C ABI of include/wost.h.
//
// Mirrors the control flow around the reference's hot loop:
//   wost_create  <- WostSolver_2D.__init__ / buildModifiedSigma (solvers/WoStSolver.py:22-138)
//   wost_solve   <- WostSolver_2D.solve / _solveUnified        (solvers/WoStSolver.py:162-353)
// and owns the device state: geometry, field programs, sampler table,
// per-walk workspace and the walk/reduce launches on a private HIP stream.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <map>
#include <thread>
#include <set>
#include <mutex>
#include <optional>
#include <string>
#include <vector>

#include "wost_device.h"
#include "wost_internal.h"
#include "wost_jit.h"
#include "wost_launch.h"
#include "wost_options.h"
#include "wost_tables.h"
#include "wost_tree.h"

using namespace wost;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(WOST_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

struct HostField {
    bool present = false;
    int flags = 0;
    std::vector<DTerm> terms;      // first = index into this field's factors
    std::vector<DFactor> factors;
    std::vector<float> grid;       // FK_GRID values; p6 = offset into this field's grid
};

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

// Flattened program for the device (and for host-side evaluation).
struct Program {
    std::vector<unsigned char> bytes;
    // the (sigma, alpha) descriptors of models 1.. (wost_set_models, n >= 2): host only, read by
    // the generator (wost_jit.h ProgramView::models); their terms, factors and grid values
    // follow the N_FIELDS fields' in `bytes`
    std::vector<DField> models;
    const DProgram* hdr() const { return reinterpret_cast<const DProgram*>(bytes.data()); }
    const DTerm* terms() const { return reinterpret_cast<const DTerm*>(bytes.data() + sizeof(DProgram)); }
    const DFactor* factors() const {
        return reinterpret_cast<const DFactor*>(bytes.data() + sizeof(DProgram) +
                                                sizeof(DTerm) * hdr()->n_terms_total);
    }
    const float* grid() const {
        return reinterpret_cast<const float*>(bytes.data() +
                                              program_grid_offset(hdr()->n_terms_total, hdr()->n_factors_total));
    }
};

// f: N_FIELDS fields (absent ones empty); extra: the model fields after them (Program::models)
void build_program(const HostField* f, double sigma_bar, Program& out, const std::vector<HostField>* extra = nullptr) {
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

struct wost_handle {
    int device = 0;
    int compat = WOST_COMPAT_REFERENCE;
    int num_cus = 0;
    std::vector<float> dverts, nverts;
    HostField fields[N_FIELDS];   // N_SLOTS problem fields, then sources 1.. of wost_set_sources
    int n_sources = 1;
    // 2.5-D wavenumbers (wost_set_wavenumbers): k^2 per wavenumber, 0 = none set; a solve
    // scores channels() = max(1, n_wavenumbers) * n_sources values per walk
    int n_wavenumbers = 0;
    float k2[WOST_MAX_SOURCES] = {};
    // conductivity models (wost_set_models): 0 = none set. Model 0's (sigma, alpha) sit in
    // SLOT_SIGMA / SLOT_ALPHA (the problem's own are kept in own_fields meanwhile), models 1..
    // in model_fields[2 (m - 1)], [2 (m - 1) + 1]
    int n_models = 0;
    std::vector<HostField> model_fields;
    HostField own_fields[2];
    uint64_t models_sum = 0;   // FNV-1a 64 of the converted model fields (0: none)
    int channels() const {
        return (n_models > 0 ? n_models : 1) * (n_wavenumbers > 0 ? n_wavenumbers : 1) * n_sources;
    }
    // point sources (wost_set_point_sources): the charges (n_sources counts their source
    // channels then), the Neumann segment(s) each lies on ([2 n], -1: none) and their device
    // image (WalkArgs::charges, kChargeWords words)
    std::vector<wost_point_charge> charges;
    std::vector<int32_t> charge_seg;
    float* d_charges = nullptr;
    int32_t* d_point_code = nullptr;   // boundary_code of the query points (WalkArgs::point_code)
    int64_t point_code_cap = 0;
    bool has_source() const { return fields[SLOT_F].present || !charges.empty(); }
    bool delta = false;
    double sigma_bar = 0.0;
    Program prog;
    std::vector<float> table;   // sampler nodes (built on first use)
    bool table_ready = false;
    bool prog_dirty = true;
    uint64_t prog_version = 0;  // bumped whenever the program is rebuilt

    // compat="fixed" delta tracking: refuse solves whose walks would all hit maxSteps
    bool fixed_step_check = true;
    int trig_mode = WOST_TRIG_AUTO;       // wost_set_trig

    // kernel and launch options (wost_set_option; study builds: also the A/B environment)
    Options opt;

    // field-specialised walk kernel (wost_jit.cpp)
    bool jit_enabled = true;
    hipFunction_t jit_fn = nullptr;
    hipFunction_t jit_alpha_fn = nullptr;   // the same module's wost_point_alpha_jit (delta tracking)
    std::optional<KernelVariant> jit_variant;   // the variant jit_fn was looked up for (empty: none)
    uint64_t jit_version = ~0ull;               // ... and the program's version then
    bool jit_cached(const KernelVariant& v) const { return jit_variant == v && jit_version == prog_version; }
    std::string jit_error;

    // Neumann segment tree (wost_tree.h): used when the Neumann polyline has at
    // least tree_min_segments segments (< 0: never)
    int tree_min_segments = WOST_TREE_MIN_SEGMENTS_DEFAULT;
    int tree_leaf = WOST_TREE_LEAF_DEFAULT;
    bool tree_ready = false;
    SegmentTreeHost tree;
    float* d_tree = nullptr;

    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};
    float2* d_dverts = nullptr;
    float2* d_nverts = nullptr;
    float* d_seg_phi = nullptr;
    float* d_table = nullptr;
    char* d_prog = nullptr;
    size_t d_prog_cap = 0;
    unsigned long long* d_counter = nullptr;   // the walk launches' control words (wost_walk.h kCtlWords)
    int64_t ctl_cap = 0;                       // ... words allocated
    float* d_val = nullptr;
    uint32_t* d_steps = nullptr;
    int64_t ws_cap = 0, ws_val_cap = 0;
    int64_t* d_begin = nullptr;       // (d_points and d_begin point into d_stage)
    char* d_stage = nullptr;          // device image of the pinned staging's [points | block ranges]
    size_t stage_cap = 0;
    double* d_bstats = nullptr;
    int64_t bstats_cap = 0;
    float2* d_points = nullptr;
    float* d_point_alpha = nullptr;   // alpha at the query points (delta tracking)
    int64_t point_alpha_cap = 0;
    uint32_t* d_pool = nullptr;       // walk pools of the tree kernels' workgroups (WalkArgs::pool)
    int64_t pool_cap = 0;
    double tick_khz = 100000.0;       // the device wall clock (hipDeviceAttributeWallClockRate)
    // pinned host staging of a solve's small copies (points, block ranges, block sums):
    // a pageable hipMemcpyAsync costs ~9 us of host time each (profiles/r05_ab/host_path/)
    char* h_pin = nullptr;
    size_t pin_cap = 0;
    bool counter_zero = false;        // d_counter is 0 (the block reduce resets it after each walk launch)
    Batch batch;                      // the current launch's plan (wost_launch.h; its block list is reused)
    wost_timing timing{};
};

namespace {

constexpr int64_t kMaxBatchWalks = int64_t(1) << 26;   // 64 Mi walks = 512 MiB of per-walk results
// Above this many bytes of staged polylines per workgroup (4 workgroups of 256 on a
// 160 KiB CU, 4 waves per SIMD) the field-specialised kernel reads the polylines from
// global memory instead (wost_walk.h GL): long Dirichlet polylines, and long Neumann
// polylines under compat="fixed" (which scans them), work at any length.
constexpr size_t kGlobalPolylineLdsBytes = 40 * 1024;

// The solve's launch statistics (the walk kernel's per-wave records, wost_block_reduce)
// ride in front of the block sums in d_bstats, so that one copy brings both to the host.
constexpr int64_t kLstatsWords = 8;

int upload_program(wost_handle* h) {
    if (!h->prog_dirty) return WOST_OK;
    build_program(h->fields, h->sigma_bar, h->prog, &h->model_fields);
    if (h->prog.bytes.size() > h->d_prog_cap) {
        if (h->d_prog) (void)hipFree(h->d_prog);
        h->d_prog = nullptr;
        HIP_TRY(hipMalloc(&h->d_prog, h->prog.bytes.size()));
        h->d_prog_cap = h->prog.bytes.size();
    }
    HIP_TRY(hipMemcpy(h->d_prog, h->prog.bytes.data(), h->prog.bytes.size(), hipMemcpyHostToDevice));
    h->prog_dirty = false;
    ++h->prog_version;
    return WOST_OK;
}

// wost_set_trig's choice for this handle: WOST_TRIG_AUTO is exact for a Neumann polyline
// of >= 3 segments (a curved boundary, where a direction's last ulp decides where the
// walk goes), the hardware's sin/cos otherwise
bool exact_trig_of(const wost_handle* h) {
    if (h->trig_mode != WOST_TRIG_AUTO) return h->trig_mode == WOST_TRIG_EXACT;
    return (int)(h->nverts.size() / 2) - 1 >= 3;
}

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

// The corrected screened sampler's nodes do not depend on sigma_bar (only on the
// shape s = R sqrt(sigma_bar)): built once per process (~0.5 s of Bessel series).
const std::vector<float>& fixed_screened_table() {
    static const std::vector<float> t = [] {
        std::vector<float> v((size_t)kFixTableFloats);
        screened_fixed_nodes(v.data(), kFixRows, kFixCols, kFixXMax);
        return v;
    }();
    return t;
}

// The radial sampler's nodes depend only on the sampler and (screened) sigma_bar: each
// table is computed once per process (8-14 ms of host time, which every fresh handle's
// first solve paid; a survey's handles share one sigma_bar). kind 0: Green's, 1: the
// Jacobian-corrected Green's (compat fixed), 2: screened.
// (the cache and its lock are never destroyed: a prefetch thread may outlive the statics)
struct NodeCache {
    std::mutex mu;
    std::condition_variable cv;
    std::map<std::pair<int, uint64_t>, std::vector<float>> done;
    std::set<std::pair<int, uint64_t>> running;
};
NodeCache& node_cache() {
    static NodeCache* c = new NodeCache;
    return *c;
}

std::pair<int, uint64_t> node_key(int kind, double sigma_bar) {
    uint64_t bits = 0;
    if (kind == 2) std::memcpy(&bits, &sigma_bar, sizeof(bits));
    return std::make_pair(kind, bits);
}

void compute_nodes(int kind, double sigma_bar, std::vector<float>& v) {
    v.resize(WOST_SAMPLER_TABLE_N);
    if (kind == 2) screened_sampler_nodes(v.data(), WOST_SAMPLER_TABLE_N, sigma_bar);
    else if (kind == 1) greens_sampler_nodes_jacobian(v.data(), WOST_SAMPLER_TABLE_N);
    else greens_sampler_nodes(v.data(), WOST_SAMPLER_TABLE_N);
}

void store_nodes(const std::pair<int, uint64_t>& key, std::vector<float>&& v) {
    NodeCache& c = node_cache();
    std::lock_guard<std::mutex> lock(c.mu);
    if (c.done.size() >= 64) c.done.clear();
    c.done.emplace(key, std::move(v));
    c.running.erase(key);
    c.cv.notify_all();
}

void sampler_nodes_once(int kind, double sigma_bar, float* out) {
    NodeCache& c = node_cache();
    const auto key = node_key(kind, sigma_bar);
    {
        std::unique_lock<std::mutex> lock(c.mu);
        c.cv.wait(lock, [&] { return !c.running.count(key); });   // (a prefetch computing them)
        auto it = c.done.find(key);
        if (it != c.done.end()) {
            std::memcpy(out, it->second.data(), sizeof(float) * WOST_SAMPLER_TABLE_N);
            return;
        }
        c.running.insert(key);
    }
    std::vector<float> v;
    compute_nodes(kind, sigma_bar, v);
    std::memcpy(out, v.data(), sizeof(float) * WOST_SAMPLER_TABLE_N);
    store_nodes(key, std::move(v));
}

// wost_create: the nodes a first solve of this handle needs, computed in the background
// while the handle's device setup runs (a fresh process's first HIP calls take ~0.1 s).
void sampler_nodes_prefetch(int kind, double sigma_bar) {
    NodeCache& c = node_cache();
    const auto key = node_key(kind, sigma_bar);
    {
        std::lock_guard<std::mutex> lock(c.mu);
        if (c.running.count(key) || c.done.count(key)) return;
        c.running.insert(key);
    }
    try {
        std::thread([kind, sigma_bar, key]() {
            std::vector<float> v;
            compute_nodes(kind, sigma_bar, v);
            store_nodes(key, std::move(v));
        }).detach();
    } catch (...) {
        std::vector<float> v;
        compute_nodes(kind, sigma_bar, v);
        store_nodes(key, std::move(v));
    }
}

// The sampler kind ensure_table builds for a handle.
int sampler_kind(const wost_handle* h) {
    if (h->delta && h->compat == WOST_COMPAT_FIXED) return 1;
    if (h->delta) return 2;
    return h->compat == WOST_COMPAT_FIXED ? 1 : 0;
}

int ensure_table(wost_handle* h) {
    if (h->table_ready) return WOST_OK;
    // sampler nodes, then (delta tracking) the G_norm cells (wost_device.h), then
    // (compat="fixed" delta tracking) the corrected screened sampler's nodes
    const bool fix_delta = h->delta && h->compat == WOST_COMPAT_FIXED;
    const size_t n = table_floats(h->delta, fix_delta);
    h->table.assign(n, 0.f);
    if (fix_delta) {
        sampler_nodes_once(sampler_kind(h), 0.0, h->table.data());   // staged, unused
        greens_norm_cells(h->table.data() + kSamplerFloatsPadded, kGnormCells, (double)kGnormCells / kGnormInvH);
        const std::vector<float>& fx = fixed_screened_table();
        std::memcpy(h->table.data() + kFixTableOffset, fx.data(), sizeof(float) * fx.size());
    } else if (h->delta) {
        sampler_nodes_once(2, h->sigma_bar, h->table.data());
        greens_norm_cells(h->table.data() + kSamplerFloatsPadded, kGnormCells, (double)kGnormCells / kGnormInvH);
    } else if (h->compat == WOST_COMPAT_FIXED) {
        sampler_nodes_once(1, 0.0, h->table.data());
    } else {
        sampler_nodes_once(0, 0.0, h->table.data());
    }
    if (!h->d_table) HIP_TRY(hipMalloc(&h->d_table, sizeof(float) * std::max(n, table_floats(true))));
    HIP_TRY(hipMemcpy(h->d_table, h->table.data(), sizeof(float) * n, hipMemcpyHostToDevice));
    h->table_ready = true;
    return WOST_OK;
}

// buildModifiedSigma's sigma_bar (solvers/WoStSolver.py:129-136 with
// utils.py:65-120): max - min of sigma' on a 50x50 ij-grid over the bounding
// box of all boundary vertices; NaN/inf samples skipped; a range <= 0 or
// > 1e3 falls back to 10.0 (quirk Q8).
double estimate_sigma_bar(const wost_handle* h, const Program& prog) {
    float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    auto scan = [&](const std::vector<float>& v) {
        for (size_t i = 0; i + 1 < v.size(); i += 2) {
            xmin = std::min(xmin, v[i]); xmax = std::max(xmax, v[i]);
            ymin = std::min(ymin, v[i + 1]); ymax = std::max(ymax, v[i + 1]);
        }
    };
    scan(h->dverts);
    scan(h->nverts);
    const std::vector<float> gx = torch_linspace(xmin, xmax, 50), gy = torch_linspace(ymin, ymax, 50);
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

// What of the segment tree the field-specialised kernels stage in LDS, by level:
// 2 = its records and the Neumann vertices (one kTreeStageVertsBlock-thread workgroup
// per CU), 1 = its records (two kTreeStageBlock-thread workgroups per CU), 0 = nothing
// (256-thread workgroups, records and vertices through L1/L2). The option tree_lds caps
// the level (A/B; the results are the same bits at every level). Returns the records to
// stage and sets the workgroup size and the vertices to stage.
constexpr size_t kTreeLdsMaxBytes = 64 * 1024;
constexpr int kTreeLdsDefaultLevel = 2;
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

bool use_tree(const wost_handle* h) {
    const int nseg = (int)(h->nverts.size() / 2) - 1;
    return nseg >= 1 && h->tree_min_segments >= 0 && nseg >= h->tree_min_segments;
}

// The traits of the handle's walks with a source term or not (delta tracking needs one:
// check_request refuses the solve without).
WalkTraits walk_traits(const wost_handle* h, bool src) {
    const bool neu = !h->nverts.empty();
    return WalkTraits{.neu = neu, .src = src || h->delta, .delta = h->delta, .tree = neu && use_tree(h),
                      .fix = h->compat == WOST_COMPAT_FIXED};
}

WalkTraits walk_traits(const wost_handle* h) { return walk_traits(h, h->has_source()); }

int ensure_tree(wost_handle* h) {
    if (h->tree_ready) return WOST_OK;
    const int nv = (int)(h->nverts.size() / 2);
    // a polyline too long for kTreeMaxDepth levels at the chosen leaf size takes 32 per leaf
    if (!build_segment_tree(h->nverts.data(), nv, h->tree_leaf, &h->tree) &&
        !build_segment_tree(h->nverts.data(), nv, 32, &h->tree))
        return fail(WOST_ERR_UNSUPPORTED, "cannot build the Neumann segment tree of %d segments (at most %d levels "
                    "of 32-segment leaves)", nv - 1, kTreeMaxDepth);
    if (h->d_tree) (void)hipFree(h->d_tree);
    h->d_tree = nullptr;
    const size_t n = std::max<size_t>(h->tree.rec.size(), 16);
    HIP_TRY(hipMalloc(&h->d_tree, sizeof(float) * n));
    if (!h->tree.rec.empty())
        HIP_TRY(hipMemcpy(h->d_tree, h->tree.rec.data(), sizeof(float) * h->tree.rec.size(), hipMemcpyHostToDevice));
    h->tree_ready = true;
    return WOST_OK;
}

template <class T>
int ensure_cap(T*& p, int64_t& cap, int64_t need) {
    if (need <= cap) return WOST_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, sizeof(T) * (size_t)need);
    if (e != hipSuccess) return fail(WOST_ERR_OOM, "hipMalloc(%lld bytes): %s", (long long)(sizeof(T) * need), hipGetErrorString(e));
    cap = need;
    return WOST_OK;
}

// pinned host staging of at least `need` bytes
int ensure_pin(wost_handle* h, size_t need) {
    if (need <= h->pin_cap) return WOST_OK;
    if (h->h_pin) {   // (a solve that failed mid-way may have left copies from it queued)
        (void)hipStreamSynchronize(h->stream);
        (void)hipHostFree(h->h_pin);
    }
    h->h_pin = nullptr;
    h->pin_cap = 0;
    need = std::max<size_t>(need, 4096);
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h->h_pin), need, hipHostMallocDefault);
    if (e != hipSuccess) return fail(WOST_ERR_OOM, "hipHostMalloc(%zu bytes): %s", need, hipGetErrorString(e));
    h->pin_cap = need;
    return WOST_OK;
}

// per-walk value and step buffers, always of equal capacity
// Per-walk results of `need` walks with `ns` values each.
int ensure_workspace(wost_handle* h, int64_t need, int ns = 1) {
    if (need <= h->ws_cap && need * ns <= h->ws_val_cap && h->d_val && h->d_steps) return WOST_OK;
    if (h->d_val) (void)hipFree(h->d_val);
    if (h->d_steps) (void)hipFree(h->d_steps);
    h->d_val = nullptr;
    h->d_steps = nullptr;
    h->ws_cap = h->ws_val_cap = 0;
    hipError_t e = hipMalloc(&h->d_val, sizeof(float) * (size_t)need * (size_t)ns);
    if (e == hipSuccess) e = hipMalloc(&h->d_steps, sizeof(uint32_t) * (size_t)need);
    if (e != hipSuccess) return fail(WOST_ERR_OOM, "per-walk workspace of %lld walks: %s", (long long)need, hipGetErrorString(e));
    h->ws_cap = need;
    h->ws_val_cap = need * ns;
    return WOST_OK;
}

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

}  // namespace

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

void wost_destroy(wost_handle* h) {
    if (!h) return;
    if (h->device >= 0) (void)hipSetDevice(h->device);
    void* ptrs[] = {h->d_dverts, h->d_nverts, h->d_table, h->d_prog, h->d_counter, h->d_val,
                    h->d_steps, h->d_stage, h->d_bstats, h->d_tree, h->d_seg_phi, h->d_point_alpha, h->d_pool,
                    h->d_charges, h->d_point_code};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (h->h_pin) (void)hipHostFree(h->h_pin);
    for (hipEvent_t& e : h->ev)
        if (e) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

}  // extern "C"

namespace {

// The host half of wost_create: validation, field conversion, sigma_bar. No
// HIP call; the handle's device is -1 until wost_create takes a device.
int create_host(const wost_problem* pb, wost_handle** out) {
    *out = nullptr;
    if (pb->compat != WOST_COMPAT_REFERENCE && pb->compat != WOST_COMPAT_FIXED)
        return fail(WOST_ERR_INVALID_ARG, "unknown compat %d", pb->compat);
    wost_handle* h = new wost_handle();
    h->device = -1;
    int rc;
    if ((rc = check_polyline(pb->dirichlet, "dirichlet", true, h->dverts)) != WOST_OK ||
        (rc = check_polyline(pb->neumann, "neumann", false, h->nverts)) != WOST_OK ||
        (rc = convert_field(pb->boundary, h->fields[SLOT_G], "boundary")) != WOST_OK ||
        (rc = convert_field(pb->source, h->fields[SLOT_F], "source")) != WOST_OK ||
        (rc = convert_field(pb->sigma, h->fields[SLOT_SIGMA], "sigma")) != WOST_OK ||
        (rc = convert_field(pb->alpha, h->fields[SLOT_ALPHA], "alpha")) != WOST_OK) {
        delete h;
        return rc;
    }
    h->compat = pb->compat;
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
            h->sigma_bar = estimate_sigma_bar(h, tmp);
            if (!(h->sigma_bar > 0.0)) {
                delete h;
                return fail(WOST_ERR_INVALID_ARG,
                            "sigma' could not be evaluated at any grid point (reference raises ValueError, utils.py:108-109)");
            }
        }
    }
    *out = h;
    return WOST_OK;
}

}  // namespace

extern "C" {

int wost_create(const wost_problem* pb, wost_handle** out) {
    if (!pb || !out) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    jit_start_identity_probe();   // (the compile helper's start, in the background)
    wost_handle* h = nullptr;
    int rc = create_host(pb, &h);
    if (rc != WOST_OK) return rc;
    *out = nullptr;
    if (h->fields[SLOT_F].present || h->delta)   // the first solve's sampler nodes, meanwhile
        sampler_nodes_prefetch(sampler_kind(h), h->sigma_bar);

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        wost_destroy(h);
        return fail(WOST_ERR_NO_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    }
    if (pb->device < 0 || pb->device >= ndev) {
        wost_destroy(h);
        return fail(WOST_ERR_INVALID_ARG, "device %d out of range [0,%d)", pb->device, ndev);
    }
    h->device = pb->device;
#define CREATE_TRY(expr)                                              \
    do {                                                              \
        hipError_t e_ = (expr);                                       \
        if (e_ != hipSuccess) {                                       \
            int rc_ = fail(WOST_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
            wost_destroy(h);                                          \
            return rc_;                                               \
        }                                                             \
    } while (0)
    CREATE_TRY(hipSetDevice(h->device));
    CREATE_TRY(hipDeviceGetAttribute(&h->num_cus, hipDeviceAttributeMultiprocessorCount, h->device));
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) == hipSuccess && khz > 0)
            h->tick_khz = (double)khz;
    }
    CREATE_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    for (hipEvent_t& ev : h->ev) CREATE_TRY(hipEventCreate(&ev));
    h->ctl_cap = (int64_t)ctl_words(8192);   // 8,192 waves: 256 CUs x 32
    CREATE_TRY(hipMalloc(&h->d_counter, sizeof(unsigned long long) * (size_t)h->ctl_cap));
    CREATE_TRY(hipMemset(h->d_counter, 0, sizeof(unsigned long long) * (size_t)h->ctl_cap));
    CREATE_TRY(hipMalloc(&h->d_dverts, sizeof(float) * h->dverts.size()));
    CREATE_TRY(hipMemcpy(h->d_dverts, h->dverts.data(), sizeof(float) * h->dverts.size(), hipMemcpyHostToDevice));
    if (!h->nverts.empty()) {
        CREATE_TRY(hipMalloc(&h->d_nverts, sizeof(float) * h->nverts.size()));
        CREATE_TRY(hipMemcpy(h->d_nverts, h->nverts.data(), sizeof(float) * h->nverts.size(), hipMemcpyHostToDevice));
        // atan2 of each segment's left normal (:227-228, quirk Q2) on the host: the C
        // library's atan2f is what torch.atan2 of the reference's 0-d tensors calls, and
        // the device's atan2f differs from it on ~half of the C5 topography's segments
        // (tools/r05/trig_compare.py), each a different direction after a Neumann hit
        const int nseg = (int)(h->nverts.size() / 2) - 1;
        std::vector<float> phi((size_t)std::max(nseg, 1), 0.0f);
        for (int i = 0; i < nseg; ++i) {
            const float2 a{h->nverts[2 * i], h->nverts[2 * i + 1]}, b{h->nverts[2 * i + 2], h->nverts[2 * i + 3]};
            const float2 n = segment_left_normal(a, b);
            phi[i] = std::atan2(n.y, n.x);
        }
        CREATE_TRY(hipMalloc(&h->d_seg_phi, sizeof(float) * phi.size()));
        CREATE_TRY(hipMemcpy(h->d_seg_phi, phi.data(), sizeof(float) * phi.size(), hipMemcpyHostToDevice));
    }
#undef CREATE_TRY
    if ((rc = upload_program(h)) != WOST_OK) {
        wost_destroy(h);
        return rc;
    }
    *out = h;
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

}  // extern "C"

namespace {

constexpr int64_t kMaxRecordBatchBytes = int64_t(1) << 30;   // device buffer of the walk recorder

// What a solve computes: W walks of each point, of which either blocks [block_begin,
// block_end) or (wost_solve_range) walks [walk_begin, walk_end) of every point
// (wost_launch.h SolveRanges). multi: the caller takes channels() values per walk.
struct SolveRequest {
    const float* points = nullptr;
    int64_t n_points = 0, W = 0;
    int32_t max_steps = 0;
    float eps = 0.f;
    uint64_t seed = 0;
    bool multi = false;
    int64_t block_begin = 0, block_end = 0;
    int64_t walk_begin = 0, walk_end = -1;   // (-1: W)
};

// Where its results go on the host (each may be null): rows of 2 * channels + 1 doubles per
// block and per point, per-walk values and steps, and with `records` the walk recorder's
// (wost_solve_history) records[walk][max_steps + 1][kRecFloats].
struct SolveOutputs {
    double* block_stats = nullptr;
    double* point_stats = nullptr;
    float* walk_values = nullptr;
    uint32_t* walk_steps = nullptr;
    float* records = nullptr;
};

SolveRequest whole_request(const float* points, int64_t n_points, int64_t W, int32_t max_steps, float eps,
                           uint64_t seed) {
    SolveRequest rq;
    rq.points = points;
    rq.n_points = n_points;
    rq.W = W;
    rq.max_steps = max_steps;
    rq.eps = eps;
    rq.seed = seed;
    rq.block_end = wost_num_blocks(n_points, W);
    return rq;
}

// The kernel a solve launches first (its occupancy fallback may then stage
// less): the workgroup, the segment tree's staging, and whether the polylines are read
// from global memory. Shared by choose_kernel, solve_race and wost_prepare_sources, so that
// a raced or prepared kernel is the one the solve looks up.
struct KernelShape {
    int block = kWalkBlock, tree_verts = 0, tree_level = kTreeLdsDefaultLevel, tree_lds = 0;
    bool gpoly = false;
    // the staging level compiled into the kernel (tree_lds_records)
    int stage() const { return tree_lds > 0 ? (tree_verts > 0 ? 2 : 1) : 0; }
};

// The field-specialised kernel of that shape for walks with traits `t` that score n_sources
// sources: the one place that reads the rest of the variant off the handle.
KernelVariant kernel_variant(const wost_handle* h, const WalkTraits& t, const KernelShape& ks, bool record,
                             int n_sources) {
    return KernelVariant{.traits = t, .record = record, .n_sources = n_sources,
                         .n_wavenumbers = t.delta ? h->n_wavenumbers : 0,   // (0: the kernel without the k2 read)
                         .n_charges = (int)h->charges.size(), .n_models = t.delta ? h->n_models : 0,
                         .block = ks.block, .global_polylines = ks.gpoly,
                         .tree_stage = ks.stage(), .exact_trig = exact_trig_of(h)};
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
    WalkLds lds{.traits = t, .nd = nd_, .nn = nn_, .const_d = jit_const_dirichlet(O, nd_)};
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

// The kernel a solve launches and how it fits a CU.
struct KernelChoice {
    hipFunction_t jfn = nullptr;   // the field-specialised kernel; null: the precompiled one
    KernelShape shape;             // (of the precompiled one: 256 threads, nothing of the tree staged)
    size_t lds = 0;                // dynamic LDS of a workgroup
    int blocks_per_cu = 0;
    double jit_ms = 0.0;           // host time spent compiling
};

// LDS bytes per workgroup of the chosen kernel
size_t lds_of(const wost_handle* h, const WalkTraits& t, const KernelChoice& kc) {
    const int nd_ = (int)(h->dverts.size() / 2);
    const bool jit = kc.jfn != nullptr;
    // option lds_pad_bytes (occupancy studies): extra bytes of LDS per workgroup
    return walk_lds_bytes({.traits = t, .nd = nd_, .nn = (int)(h->nverts.size() / 2), .tree_lds = kc.shape.tree_lds,
                           .tree_verts = kc.shape.tree_verts, .const_d = jit && jit_const_dirichlet(h->opt, nd_),
                           .global_polylines = jit && kc.shape.gpoly, .block = kc.shape.block}) +
           (size_t)h->opt.lds_pad_bytes;
}

// The kernel of a solve with the handle's fields: the field-specialised one of
// first_kernel_shape, staging less of the segment tree while what it stages costs the CU
// its waves; the precompiled one when that is disabled or could not be built.
int choose_kernel(wost_handle* h, const WalkTraits& t, bool record, int n_src, int ns, KernelChoice* kc) {
    *kc = KernelChoice{};
    KernelShape& ks = kc->shape;
    int rc;
    if ((rc = first_kernel_shape(h, t, &ks)) != WOST_OK) return rc;
    int lds_cap = -1;
    // looks ks up and measures its occupancy
    auto lookup = [&]() -> int {
        kc->jfn = jit_kernel(h, kernel_variant(h, t, ks, record, n_src), &kc->jit_ms);
        if (!kc->jfn) {   // the precompiled kernels run 256-thread workgroups, no staged tree, one channel
            if (!h->charges.empty())
                return fail(WOST_ERR_UNSUPPORTED, "point sources need the field-specialised kernel%s%s",
                            h->jit_enabled ? ": " : " (disabled by wost_set_jit)", h->jit_error.c_str());
            if (ns > 1)
                return fail(WOST_ERR_UNSUPPORTED,
                            "multi-source, multi-wavenumber and multi-model solves need the field-specialised kernel%s%s",
                            h->jit_enabled ? ": " : " (disabled by wost_set_jit)", h->jit_error.c_str());
            ks.block = kWalkBlock;
            ks.tree_lds = ks.tree_verts = 0;
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
    if (int rc = plan_ranges(n_points, W, rq.block_begin, rq.block_end, rq.walk_begin, rq.walk_end, ranges, msg,
                             sizeof(msg)))
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

// Pinned staging: [points | one batch's block ranges | the block sums], 64-byte aligned;
// the device holds the first two parts in one buffer of the same layout (h->d_points,
// h->d_begin), so that one copy brings the points and the first batch's block ranges (C2: a
// copy and its ~6 us gap less)
struct Staging {
    float* points = nullptr;
    int64_t* begin = nullptr;
    double* bstats = nullptr;
    size_t pts_bytes = 0, beg_bytes = 0, bs_bytes = 0;
};

int stage_buffers(wost_handle* h, int64_t n_points, int64_t nblk, int row, Staging* st) {
    auto al64 = [](size_t b) { return (b + 63) / 64 * 64; };
    st->pts_bytes = al64(sizeof(float2) * (size_t)std::max<int64_t>(n_points, 1));
    st->beg_bytes = al64(sizeof(int64_t) * (size_t)(nblk + 1));
    st->bs_bytes = al64(sizeof(double) * (size_t)(kLstatsWords + row * nblk));
    const size_t dev_bytes = st->pts_bytes + st->beg_bytes;
    if (int rc = ensure_pin(h, dev_bytes + st->bs_bytes)) return rc;
    if (dev_bytes > h->stage_cap) {
        if (h->d_stage) (void)hipFree(h->d_stage);
        h->d_stage = nullptr;
        h->stage_cap = 0;
        const hipError_t e = hipMalloc(&h->d_stage, dev_bytes);
        if (e != hipSuccess) return fail(WOST_ERR_OOM, "hipMalloc(%zu bytes): %s", dev_bytes, hipGetErrorString(e));
        h->stage_cap = dev_bytes;
    }
    h->d_points = reinterpret_cast<float2*>(h->d_stage);
    h->d_begin = reinterpret_cast<int64_t*>(h->d_stage + st->pts_bytes);
    st->points = reinterpret_cast<float*>(h->h_pin);
    st->begin = reinterpret_cast<int64_t*>(h->h_pin + st->pts_bytes);
    st->bstats = reinterpret_cast<double*>(h->h_pin + dev_bytes);
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
        a.tree = reinterpret_cast<const float4*>(h->d_tree);
        a.tree_first_leaf = h->tree.first_leaf;
        a.tree_leaf = h->tree.leaf;
        a.tree_tol = h->tree.tol;
        a.tree_stop2 = silhouette_stop2(a.rmin);
        a.tree_kmax = h->tree.kmax;
        a.tree_lds_records = kc.shape.tree_lds;
        a.tree_lds_verts = kc.shape.tree_verts;
        a.tree_depth = h->tree.depth;
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
    float x0 = h->nverts[0], x1 = x0, y0 = h->nverts[1], y1 = y0;
    for (size_t i = 2; i + 1 < h->nverts.size(); i += 2) {
        x0 = std::min(x0, h->nverts[i]); x1 = std::max(x1, h->nverts[i]);
        y0 = std::min(y0, h->nverts[i + 1]); y1 = std::max(y1, h->nverts[i + 1]);
    }
    const float m = (float)O.pool_near * std::max(x1 - x0, y1 - y0);
    // (study builds, tree_iter_stats: 16 counter words after each workgroup's pools)
    const int64_t words = (int64_t)pool_wg_words(n_src, O.pool_slots) + (O.tree_iter_stats ? 16 : 0);
    if (int rc = ensure_cap(h->d_pool, h->pool_cap, words * (int64_t)blocks_per_cu * h->num_cus)) return rc;
    a->pool = h->d_pool;
    a->pool_slots = O.pool_slots;
    a->pool_wg_words = (int32_t)words;
    a->pool_box = make_float4(x0 - m, y0 - m, x1 + m, y1 + m);
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
    if (int rc = ensure_cap(h->d_point_alpha, h->point_alpha_cap, nm * n_points)) return rc;
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

// ---- point sources: the host's geometry (wost_set_point_sources, setup_point_sources) ----

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

// The device image of the handle's charges (WalkArgs::charges), alpha left at 1.
int upload_charges(wost_handle* h) {
    std::vector<float> w((size_t)kChargeWords, 0.0f);
    for (size_t p = 0; p < h->charges.size(); ++p) {
        const wost_point_charge& c = h->charges[p];
        w[CHG_XY + 2 * p] = c.x;
        w[CHG_XY + 2 * p + 1] = c.y;
        w[CHG_Q + p] = c.strength;
        w[CHG_ALPHA + p] = 1.0f;
        std::memcpy(&w[CHG_SOURCE + p], &c.source, sizeof(int32_t));
        std::memcpy(&w[CHG_SEG0 + p], &h->charge_seg[2 * p], sizeof(int32_t));
        std::memcpy(&w[CHG_SEG1 + p], &h->charge_seg[2 * p + 1], sizeof(int32_t));
    }
    HIP_TRY(hipSetDevice(h->device));
    if (!h->d_charges) HIP_TRY(hipMalloc(&h->d_charges, sizeof(float) * (size_t)kChargeWords));
    HIP_TRY(hipMemcpy(h->d_charges, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice));
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
    if (int rc = ensure_cap(h->d_point_code, h->point_code_cap, rq.n_points)) return rc;
    HIP_TRY(hipMemcpy(h->d_point_code, code.data(), sizeof(int32_t) * code.size(), hipMemcpyHostToDevice));
    a->point_code = h->d_point_code;
    return WOST_OK;
}

// FNV-1a 64 of the charges and their source count.
uint64_t charges_checksum(const wost_handle* h) {
    if (h->charges.empty()) return 0;
    uint64_t hsh = 1469598103934665603ull;
    auto eat = [&](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) hsh = (hsh ^ b[i]) * 1099511628211ull;
    };
    const int32_t ns = h->n_sources;
    eat(&ns, sizeof(ns));
    for (const wost_point_charge& c : h->charges) {
        eat(&c.x, sizeof(float)); eat(&c.y, sizeof(float)); eat(&c.strength, sizeof(float)); eat(&c.source, sizeof(int32_t));
    }
    return hsh;
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
    if ((int64_t)ctl_words(waves) <= h->ctl_cap) return WOST_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    (void)hipFree(h->d_counter);
    h->d_counter = nullptr;
    h->ctl_cap = 0;
    HIP_TRY(hipMalloc(&h->d_counter, sizeof(unsigned long long) * ctl_words(waves)));
    HIP_TRY(hipMemset(h->d_counter, 0, sizeof(unsigned long long) * ctl_words(waves)));   // synchronous
    h->ctl_cap = (int64_t)ctl_words(waves);
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

// Every solve: checks, the kernel, then one walk launch and one block reduce per batch of
// the plan (wost_launch.h), all on the handle's stream.
int solve_impl(wost_handle* h, const SolveRequest& rq, const SolveOutputs& out) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    SolveRanges R;
    int rc;
    if ((rc = check_request(h, rq, &R)) != WOST_OK) return rc;
    const int n_src = h->n_sources;
    const int ns = h->channels();
    const int row = 2 * ns + 1;   // doubles per block / point row
    const int64_t n_points = rq.n_points;
    const WalkTraits t = walk_traits(h);

    HIP_TRY(hipSetDevice(h->device));
    if ((rc = upload_program(h)) != WOST_OK) return rc;
    if (h->has_source() && (rc = ensure_table(h)) != WOST_OK) return rc;
    if (t.tree && (rc = ensure_tree(h)) != WOST_OK) return rc;
    if (out.records && !h->charges.empty())
        return fail(WOST_ERR_UNSUPPORTED, "wost_solve_history does not record point sources (a step scores every "
                                          "charge in its ball: there is no sample point)");

    h->timing = wost_timing{};
    if (out.point_stats) std::fill(out.point_stats, out.point_stats + row * n_points, 0.0);
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
    if ((rc = stage_buffers(h, n_points, R.nblk, row, &st)) != WOST_OK) return rc;
    std::memcpy(st.points, rq.points, sizeof(float2) * (size_t)n_points);
    // the points go with the first batch's block ranges, unless the query points' alpha
    // (delta tracking) needs them first
    bool points_pending = true;
    if (t.delta && n_points > 0) {
        HIP_TRY(hipMemcpyAsync(h->d_points, st.points, sizeof(float2) * n_points, hipMemcpyHostToDevice, h->stream));
        points_pending = false;
    }
    if ((rc = ensure_workspace(h, std::min<int64_t>(R.walks_total, batch_limit), ns)) != WOST_OK) return rc;
    if ((rc = ensure_cap(h->d_bstats, h->bstats_cap, kLstatsWords + R.nblk * row)) != WOST_OK) return rc;
    // (the launch statistics in front of the block sums: one copy brings both)
    unsigned long long* const d_lstats = reinterpret_cast<unsigned long long*>(h->d_bstats);
    double* const d_rows = h->d_bstats + kLstatsWords;
    float* d_rec = nullptr;
    struct RecFree {
        float*& p;
        ~RecFree() { if (p) (void)hipFree(p); }
    } rec_free{d_rec};
    if (out.records)
        HIP_TRY(hipMalloc(&d_rec, (size_t)std::min<int64_t>(R.walks_total, batch_limit) * rec_walk_bytes));

    KernelChoice kc;
    if ((rc = choose_kernel(h, t, out.records != nullptr, n_src, ns, &kc)) != WOST_OK) return rc;
    const int block = kc.shape.block;
    WalkArgs a = fill_walk_args(h, rq, t, kc, d_rec);
    if ((rc = setup_pools(h, t, n_src, kc.blocks_per_cu, &a)) != WOST_OK) return rc;
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
    double walk_ms = 0.0, red_ms = 0.0;
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
            HIP_TRY(hipEventRecord(h->ev[5], h->stream));
            HIP_TRY(hipEventSynchronize(h->ev[5]));
        } else {
            HIP_TRY(hipEventSynchronize(h->ev[2]));
        }
        float t0 = 0.f, t1 = 0.f;
        HIP_TRY(hipEventElapsedTime(&t0, h->ev[0], h->ev[1]));
        HIP_TRY(hipEventElapsedTime(&t1, h->ev[1], h->ev[2]));
        walk_ms += t0;
        red_ms += t1;
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
    h->timing.walk_kernel_ms = walk_ms;
    h->timing.reduce_kernel_ms = red_ms;
    h->timing.total_ms = tt;
    h->timing.n_launches = launches;
    h->timing.total_steps = steps_sum;
    h->timing.total_walks = (uint64_t)R.walks_total;
    h->timing.jit_ms = kc.jit_ms;
    h->timing.jit = kc.jfn ? 1 : 0;
    h->timing.tree = t.tree ? 1 : 0;
    return WOST_OK;
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

// A solve of walks [w_begin, w_begin + Wr) of every point that takes several solves of
// block-aligned sub-ranges (wost_solve_range beyond one launch per point, solve_race): each
// piece's block rows, values and steps are scattered into the whole range's layout, so the
// block sums, their order and every output are those of one solve.
struct Stitch {
    SolveRequest rq;       // the whole solve (its ranges set per piece)
    SolveOutputs out;
    int ns = 1;            // values per walk
    int64_t w_begin = 0, Wr = 0, nbr = 0;
    std::vector<double> all, part;   // block rows of the range / of a piece
    std::vector<float> pv;
    std::vector<uint32_t> ps;
    wost_timing acc{};
    double solve_ms = 0.0;   // host time of the last piece's solve

    Stitch(const SolveRequest& whole, const SolveOutputs& o, int ns_, int64_t w0, int64_t w1)
        : rq(whole), out(o), ns(ns_), w_begin(w0), Wr(w1 - w0), nbr((w1 - w0 + WOST_BLOCK_WALKS - 1) / WOST_BLOCK_WALKS),
          all((size_t)whole.n_points * nbr * (2 * ns_ + 1)) {}
};

// Solves walks [c0, c1) of every point into the stitched solve's outputs and timing.
int solve_piece(wost_handle* h, Stitch& s, int64_t c0, int64_t c1) {
    const int row = 2 * s.ns + 1;
    const int64_t n_points = s.rq.n_points;
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
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = solve_impl(h, s.rq, piece);
    s.solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != WOST_OK) return rc;
    for (int64_t p = 0; p < n_points; ++p) {
        std::memcpy(&s.all[((size_t)p * s.nbr + boff) * row], &s.part[(size_t)p * nbc * row], sizeof(double) * nbc * row);
        if (s.out.walk_values)
            std::memcpy(s.out.walk_values + ((size_t)p * s.Wr + woff) * s.ns, &s.pv[(size_t)p * wc * s.ns],
                        sizeof(float) * wc * s.ns);
        if (s.out.walk_steps)
            std::memcpy(s.out.walk_steps + (size_t)p * s.Wr + woff, &s.ps[(size_t)p * wc], sizeof(uint32_t) * wc);
    }
    add_timing(s.acc, h->timing);
    return WOST_OK;
}

// The stitched solve's block rows and point sums (in the range's block order) to the caller.
void stitched_stats(const Stitch& s) {
    const int row = 2 * s.ns + 1;
    if (s.out.block_stats) std::memcpy(s.out.block_stats, s.all.data(), sizeof(double) * s.all.size());
    if (!s.out.point_stats) return;
    std::fill(s.out.point_stats, s.out.point_stats + (size_t)row * s.rq.n_points, 0.0);
    for (int64_t p = 0; p < s.rq.n_points; ++p)
        for (int64_t k = 0; k < s.nbr; ++k)
            for (int c = 0; c < row; ++c) s.out.point_stats[(size_t)row * p + c] += s.all[((size_t)p * s.nbr + k) * row + c];
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


// The handle's fields with sources[0..n) in the source slots (wost_set_sources' conversion).
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
    for (int s = 0; s < N_FIELDS; ++s) out[s] = h->fields[s];
    out[SLOT_F] = conv[0];
    for (int s = 1; s < WOST_MAX_SOURCES; ++s) out[SLOT_EXTRA + s - 1] = s < n ? conv[s] : HostField();
    return WOST_OK;
}

std::mutex g_prepare_mu;   // wost_prepare_sources: one segment-tree build per handle

}  // namespace

extern "C" {

int wost_solve(wost_handle* h, const float* points, int64_t n_points, int64_t W,
               int64_t block_begin, int64_t block_end, int32_t max_steps, float eps, uint64_t seed,
               double* block_stats, double* point_stats, float* walk_values, uint32_t* walk_steps) {
    SolveRequest rq = whole_request(points, n_points, W, max_steps, eps, seed);
    SolveOutputs out;
    out.block_stats = block_stats; out.point_stats = point_stats;
    out.walk_values = walk_values; out.walk_steps = walk_steps;
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
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    SolveRequest rq = whole_request(points, n_points, W, max_steps, eps, seed);
    rq.multi = true;
    SolveOutputs out;
    out.block_stats = block_stats; out.point_stats = point_stats;
    out.walk_values = walk_values; out.walk_steps = walk_steps;
    if (walk_begin == 0 && walk_end == W) return solve_impl(h, rq, out);   // the whole range: an ordinary solve
    const int ns = h->channels();
    const int64_t chunk = (kMaxBatchWalks / ns) / WOST_BLOCK_WALKS * WOST_BLOCK_WALKS;   // walks of a point per launch
    if (walk_end - walk_begin <= chunk || walk_begin < 0 || walk_end <= walk_begin || n_points <= 0) {
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
    return WOST_OK;
}

int wost_solve_history(wost_handle* h, const float* points, int64_t n_points, int64_t W, int32_t max_steps,
                       float eps, uint64_t seed, double* point_stats, float* walk_values, uint32_t* walk_steps,
                       float* records) {
    if (!records) return fail(WOST_ERR_INVALID_ARG, "NULL records");
    SolveOutputs out;
    out.point_stats = point_stats;
    out.walk_values = walk_values;
    out.walk_steps = walk_steps;
    out.records = records;
    return solve_impl(h, whole_request(points, n_points, W, max_steps, eps, seed), out);
}

int wost_solve_multi(wost_handle* h, const float* points, int64_t n_points, int64_t W, int64_t block_begin,
                     int64_t block_end, int32_t max_steps, float eps, uint64_t seed, double* block_stats,
                     double* point_stats, float* walk_values, uint32_t* walk_steps) {
    SolveRequest rq = whole_request(points, n_points, W, max_steps, eps, seed);
    rq.multi = true;
    rq.block_begin = block_begin;
    rq.block_end = block_end;
    SolveOutputs out;
    out.block_stats = block_stats; out.point_stats = point_stats;
    out.walk_values = walk_values; out.walk_steps = walk_steps;
    return solve_impl(h, rq, out);
}


int wost_set_sources(wost_handle* h, const wost_field* const* sources, int32_t n) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (!h->charges.empty())
        return fail(WOST_ERR_INVALID_ARG, "the handle has point sources (wost_set_point_sources): clear them before "
                                          "setting source fields");
    std::vector<HostField> f(N_FIELDS);
    int rc = fields_with_sources(h, sources, n, f.data());
    if (rc != WOST_OK) return rc;
    if ((int64_t)n * std::max(h->n_wavenumbers, 1) * std::max(h->n_models, 1) > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "%d sources x %d wavenumbers x %d models exceed %d channels", n,
                    std::max(h->n_wavenumbers, 1), std::max(h->n_models, 1), WOST_MAX_SOURCES);
    for (int s = 0; s < N_FIELDS; ++s) h->fields[s] = std::move(f[s]);
    h->n_sources = n;
    h->prog_dirty = true;
    HIP_TRY(hipSetDevice(h->device));
    return upload_program(h);
}

int wost_prepare_sources(wost_handle* h, const wost_field* const* sources, int32_t n, int64_t n_points) {
    if (!h) return fail(WOST_ERR_INVALID_ARG, "NULL handle");
    if (n_points < 1) return fail(WOST_ERR_INVALID_ARG, "n_points must be >= 1 (got %lld)", (long long)n_points);
    if (!h->charges.empty())
        return fail(WOST_ERR_INVALID_ARG, "the handle has point sources (wost_set_point_sources): clear them first");
    std::vector<HostField> f(N_FIELDS);
    int rc = fields_with_sources(h, sources, n, f.data());
    if (rc != WOST_OK) return rc;
    if ((int64_t)n * std::max(h->n_wavenumbers, 1) * std::max(h->n_models, 1) > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "%d sources x %d wavenumbers x %d models exceed %d channels", n,
                    std::max(h->n_wavenumbers, 1), std::max(h->n_models, 1), WOST_MAX_SOURCES);
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

namespace {
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
    uint64_t hsh = 1469598103934665603ull;
    auto eat = [&](const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) hsh = (hsh ^ b[i]) * 1099511628211ull;
    };
    const int32_t n = (int32_t)(f.size() / 2);
    eat(&n, sizeof(n));
    for (const HostField& hf : f) {
        const int32_t head[4] = {hf.flags, (int32_t)hf.terms.size(), (int32_t)hf.factors.size(), (int32_t)hf.grid.size()};
        eat(head, sizeof(head));
        for (const DTerm& t : hf.terms) { eat(&t.coef, 4); eat(&t.first, 4); eat(&t.nf, 4); }
        for (const DFactor& d : hf.factors) { eat(&d.kind, 4); eat(d.p, sizeof(d.p)); }
        if (!hf.grid.empty()) eat(hf.grid.data(), sizeof(float) * hf.grid.size());
    }
    return hsh;
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

// wost_kernel_source_channels, and with n_charges > 0 wost_kernel_source_points (n_sources is
// then the charges' source count, sources NULL).
int kernel_source_impl(const wost_problem* pb, const wost_field* const* sources, int32_t n_sources,
                       int32_t n_wavenumbers, int32_t n_charges, char* out, int64_t capacity, int64_t* length,
                       const wost_model* models = nullptr, int32_t n_models = 0) {
    if (!pb || !length) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    if (n_models < 0 || n_models > WOST_MAX_SOURCES || (n_models > 0 && !models))
        return fail(WOST_ERR_INVALID_ARG, "need 0..%d models", WOST_MAX_SOURCES);
    if (n_sources < 0 || n_sources > WOST_MAX_SOURCES || (n_charges == 0 && n_sources > 0 && !sources))
        return fail(WOST_ERR_INVALID_ARG, "need 0..%d sources", WOST_MAX_SOURCES);
    if (n_wavenumbers < 0 || n_wavenumbers * std::max(n_sources, 1) > WOST_MAX_SOURCES)
        return fail(WOST_ERR_INVALID_ARG, "need sources x wavenumbers <= %d channels", WOST_MAX_SOURCES);
    wost_handle* h = nullptr;
    int rc = create_host(pb, &h);
    if (rc != WOST_OK) return rc;
    if (n_wavenumbers > 0 && !h->delta) {
        delete h;
        return fail(WOST_ERR_UNSUPPORTED, "wavenumbers need delta tracking: give sigma or alpha (a constant alpha is enough)");
    }
    h->n_wavenumbers = n_wavenumbers;
    int ns = 1;
    if (n_charges > 0) {   // wost_set_point_sources' checks and counts, without a device
        if ((rc = check_point_sources(h, nullptr, n_charges, n_sources)) != WOST_OK) {
            delete h;
            return rc;
        }
        h->charges.assign((size_t)n_charges, wost_point_charge{0.f, 0.f, 0.f, 0});
        h->n_sources = ns = n_sources;
    } else if (n_sources >= 1) {   // wost_set_sources' fields, without a device
        for (int k = 0; k < n_sources; ++k) {
            HostField hf;
            if (!sources[k] || (rc = convert_field(sources[k], hf, "source")) != WOST_OK) {
                delete h;
                return rc != WOST_OK ? rc : fail(WOST_ERR_INVALID_ARG, "source %d is NULL", k);
            }
            h->fields[k == 0 ? SLOT_F : SLOT_EXTRA + k - 1] = hf;
        }
        ns = n_sources;
    }
    if (n_models > 0) {   // wost_set_models' fields, without a device
        h->n_sources = ns;
        std::vector<HostField> conv;
        if ((rc = convert_models(models, n_models, &conv)) != WOST_OK || (rc = check_models(h, n_models, conv)) != WOST_OK) {
            delete h;
            return rc;
        }
        install_models(h, n_models, conv);
    }
    build_program(h->fields, h->sigma_bar, h->prog, &h->model_fields);
    const WalkTraits t = walk_traits(h);
    // no device here: the segment angles of a compiled-in Neumann polyline come from the
    // host's atan2f (the kernels use the device's bits; this source is for offline study)
    const int nn = (int)(h->nverts.size() / 2);
    std::vector<float> phi(nn > 1 ? nn - 1 : 0);
    for (int i = 0; i + 1 < nn; ++i) {
        const float2 a{h->nverts[2 * i], h->nverts[2 * i + 1]}, b{h->nverts[2 * i + 2], h->nverts[2 * i + 3]};
        const float2 n = segment_left_normal(a, b);
        phi[i] = std::atan2(n.y, n.x);
    }
    // the first solve's kernel without a device: 256 threads, nothing of the tree staged
    KernelVariant v = kernel_variant(h, t, KernelShape{}, false, ns);
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
    rc = jit_source(h, h->prog, v, phi.empty() ? nullptr : phi.data(), &src);
    delete h;
    if (rc != WOST_OK) return rc;
    *length = (int64_t)src.size();
    if (out && capacity > 0) {
        const size_t n = std::min<size_t>(src.size(), (size_t)capacity - 1);
        std::memcpy(out, src.data(), n);
        out[n] = '\0';
    }
    return WOST_OK;
}
}  // namespace

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

int wost_kernel_source_sources(const wost_problem* pb, const wost_field* const* sources, int32_t n_sources,
                               char* out, int64_t capacity, int64_t* length) {
    return wost_kernel_source_channels(pb, sources, n_sources, 0, out, capacity, length);
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

int wost_kernel_source(const wost_problem* pb, char* out, int64_t capacity, int64_t* length) {
    return wost_kernel_source_sources(pb, nullptr, 0, out, capacity, length);
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
    const std::string r = options_report(h ? h->opt : fresh);
    *length = (int64_t)r.size();
    if (out && capacity > 0) {
        const size_t n = std::min<size_t>(r.size(), (size_t)capacity - 1);
        std::memcpy(out, r.data(), n);
        out[n] = '\0';
    }
    return WOST_OK;
}

int wost_eval_field(wost_handle* h, int32_t which, const float* points, int64_t n, float* out) {
    if (!h || (n > 0 && (!points || !out))) return fail(WOST_ERR_INVALID_ARG, "NULL argument");
    if (which < 0 || which > 4) return fail(WOST_ERR_INVALID_ARG, "which must be 0..4");
    if (n == 0) return WOST_OK;
    HIP_TRY(hipSetDevice(h->device));
    int rc = upload_program(h);
    if (rc != WOST_OK) return rc;
    float2* dp = nullptr;
    float4* dout = nullptr;
    HIP_TRY(hipMalloc(&dp, sizeof(float2) * n));
    hipError_t e = hipMalloc(&dout, sizeof(float4) * n);
    if (e == hipSuccess) e = hipMemcpyAsync(dp, points, sizeof(float2) * n, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = launch_eval_field(h->d_prog, which, dp, n, dout, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, sizeof(float4) * n, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    (void)hipFree(dp);
    if (dout) (void)hipFree(dout);
    if (e != hipSuccess) return fail(WOST_ERR_HIP, "wost_eval_field: %s", hipGetErrorString(e));
    return WOST_OK;
}

int wost_geometry_query(int32_t device, int32_t op, const wost_polyline* poly, const float* points,
                        const float* dirs, const float* radii, int64_t n, float* out_f, uint8_t* out_mask) {
    if (!poly || !poly->xy || poly->n_vertices < 1) return fail(WOST_ERR_INVALID_ARG, "bad polyline");
    const bool tree = (op & WOST_GEOM_TREE) != 0;
    op &= ~WOST_GEOM_TREE;
    if (op < WOST_GEOM_DISTANCE || op > WOST_GEOM_INTERSECT_POLYLINES) return fail(WOST_ERR_INVALID_ARG, "unknown op %d", op);
    if (tree && op != WOST_GEOM_SILHOUETTE_DISTANCE && op != WOST_GEOM_INTERSECT_POLYLINES)
        return fail(WOST_ERR_INVALID_ARG, "the segment tree answers silhouetteDistance and intersectPolylines only");
    const int nv = poly->n_vertices;
    if (tree && nv < 3) return fail(WOST_ERR_INVALID_ARG, "the segment tree needs >= 2 segments");
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
    if (tree && !build_segment_tree(poly->xy, nv, WOST_TREE_LEAF_DEFAULT, &th) &&
        !build_segment_tree(poly->xy, nv, 32, &th))
        return fail(WOST_ERR_INVALID_ARG, "no segment tree for this polyline (degenerate or too long)");
    HIP_TRY(hipSetDevice(device));
    float4* drec = nullptr;
    if (tree) {
        HIP_TRY(hipMalloc(&drec, sizeof(float) * std::max<size_t>(th.rec.size(), 4)));
        const hipError_t e0 = hipMemcpy(drec, th.rec.data(), sizeof(float) * th.rec.size(), hipMemcpyHostToDevice);
        if (e0 != hipSuccess) {
            (void)hipFree(drec);
            return fail(WOST_ERR_HIP, "wost_geometry_query: %s", hipGetErrorString(e0));
        }
    }
    float2 *dv = nullptr, *dp = nullptr, *dd = nullptr;
    float *dr = nullptr, *df = nullptr;
    uint8_t* dm = nullptr;
    hipError_t e = hipMalloc(&dv, sizeof(float2) * nv);
    if (e == hipSuccess) e = hipMalloc(&dp, sizeof(float2) * n);
    if (e == hipSuccess && need_dirs) e = hipMalloc(&dd, sizeof(float2) * n);
    if (e == hipSuccess && op == WOST_GEOM_INTERSECT_POLYLINES) e = hipMalloc(&dr, sizeof(float) * n);
    if (e == hipSuccess && nf_out > 0) e = hipMalloc(&df, sizeof(float) * nf_out);
    if (e == hipSuccess && nm_out > 0) e = hipMalloc(&dm, nm_out);
    if (e == hipSuccess) e = hipMemcpy(dv, poly->xy, sizeof(float2) * nv, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dp, points, sizeof(float2) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && dd) e = hipMemcpy(dd, dirs, sizeof(float2) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess && dr) e = hipMemcpy(dr, radii, sizeof(float) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = tree ? launch_geometry_tree_query(op, dv, nv, drec, th.first_leaf, th.depth, th.leaf, th.tol, th.kmax, dp,
                                              dd, dr, n, df, nullptr)
                 : launch_geometry_query(op, dv, nv, dp, dd, dr, n, df, dm, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && df) e = hipMemcpy(out_f, df, sizeof(float) * nf_out, hipMemcpyDeviceToHost);
    if (e == hipSuccess && dm) e = hipMemcpy(out_mask, dm, nm_out, hipMemcpyDeviceToHost);
    void* all[] = {dv, dp, dd, dr, df, dm, drec};
    for (void* p : all)
        if (p) (void)hipFree(p);
    if (e != hipSuccess) return fail(WOST_ERR_HIP, "wost_geometry_query: %s", hipGetErrorString(e));
    return WOST_OK;
}

}  // extern "C"
