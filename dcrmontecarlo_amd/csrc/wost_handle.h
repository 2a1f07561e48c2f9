// wost_handle.h -- what the units of libwost's host half share: the error message, the
// converted fields and their device program, the owning device / pinned buffers, the
// handle, and the functions that cross units. Not part of the public ABI.
//   wost_program.cpp        field conversion and program layout (no handle, no HIP call)
//   wost_resources.cpp      sampler-node cache, table, segment tree, program and charge uploads
//   wost_kernel_choice.cpp  the kernel of a solve, its occupancy fallback, wost_kernel_source*
//   wost_solve.cpp          the per-solve steps and solve_impl
//   wost_solve_stitch.cpp   the wost_solve* entry points, the stitched and raced solves
//   wost_point_sources.cpp  point-source geometry and setters
//   wost_combine.cpp        weighted channel combinations on the host (wost_combine.h; no HIP)
//   wost_api.hip            create / destroy, the setters, the stand-alone device queries
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "wost_device.h"

namespace wost {

inline thread_local std::string g_err;   // wost_last_error

inline int fail(int code, const char* fmt, ...) {
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

// The bounding box of the vertices xy[2 n], grown from `b`.
struct Box {
    float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
};
inline void grow_box(Box& b, const std::vector<float>& xy) {
    for (size_t i = 0; i + 1 < xy.size(); i += 2) {
        b.x0 = std::min(b.x0, xy[i]); b.x1 = std::max(b.x1, xy[i]);
        b.y0 = std::min(b.y0, xy[i + 1]); b.y1 = std::max(b.y1, xy[i + 1]);
    }
}

// FNV-1a 64.
struct Fnv1a {
    uint64_t h = 1469598103934665603ull;
    void eat(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    }
};

// A text to the caller's (out, capacity): its length, and as much as fits, terminated.
inline void copy_text(const std::string& s, char* out, int64_t capacity, int64_t* length) {
    *length = (int64_t)s.size();
    if (out && capacity > 0) {
        const size_t n = std::min<size_t>(s.size(), (size_t)capacity - 1);
        std::memcpy(out, s.data(), n);
        out[n] = '\0';
    }
}

// ---- wost_program.cpp ----
int convert_field(const wost_field* in, HostField& out, const char* name);
// f: N_FIELDS fields (absent ones empty); extra: the model fields after them (Program::models)
void build_program(const HostField* f, double sigma_bar, Program& out, const std::vector<HostField>* extra = nullptr);
double estimate_sigma_bar(const std::vector<float>& dverts, const std::vector<float>& nverts, const Program& prog);
double estimate_alpha_min(const std::vector<float>& dverts, const std::vector<float>& nverts, const Program& prog);
int convert_models(const wost_model* models, int32_t n, std::vector<HostField>* out);
uint64_t models_checksum(const std::vector<HostField>& f);
std::vector<float> segment_angles(const std::vector<float>& nverts);

}  // namespace wost

// (wost_program.cpp sees the part above only: it is built without the kernels' headers)
#if !defined(WOST_PROGRAM_ONLY)

#include <memory>
#include <optional>

#include "wost_internal.h"
#include "wost_jit.h"
#include "wost_launch.h"
#include "wost_options.h"
#include "wost_tree.h"

namespace wost {

// Device memory of `capacity()` elements (kPinned: pinned host memory): move-only, freed
// with the buffer. reserve(n) only grows (no HIP call when the capacity suffices; the
// contents are not kept across a growth) and returns HIP's error for the caller to report.
template <class T, bool kPinned = false>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~DeviceBuffer() { release(); }
    hipError_t reserve(size_t n) {
        if (n <= cap_) return hipSuccess;
        release();
        void* p = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&p, sizeof(T) * n, hipHostMallocDefault) : hipMalloc(&p, sizeof(T) * n);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }
    size_t capacity() const { return cap_; }
    operator T*() const { return p_; }

private:
    void release() {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    T* p_ = nullptr;
    size_t cap_ = 0;
};
using PinnedBuffer = DeviceBuffer<char, true>;

}  // namespace wost

struct wost_handle {
    int device = 0;
    int compat = WOST_COMPAT_REFERENCE;
    int num_cus = 0;
    std::vector<float> dverts, nverts;
    wost::HostField fields[wost::N_FIELDS];   // N_SLOTS problem fields, then sources 1.. of wost_set_sources
    int n_sources = 1;
    // 2.5-D wavenumbers (wost_set_wavenumbers): k^2 per wavenumber, 0 = none set; a solve
    // scores channels() = max(1, n_wavenumbers) * n_sources values per walk
    int n_wavenumbers = 0;
    float k2[WOST_MAX_SOURCES] = {};
    // conductivity models (wost_set_models): 0 = none set. Model 0's (sigma, alpha) sit in
    // SLOT_SIGMA / SLOT_ALPHA (the problem's own are kept in own_fields meanwhile), models 1..
    // in model_fields[2 (m - 1)], [2 (m - 1) + 1]
    int n_models = 0;
    std::vector<wost::HostField> model_fields;
    wost::HostField own_fields[2];
    uint64_t models_sum = 0;   // FNV-1a 64 of the converted model fields (0: none)
    int channels() const {
        return (n_models > 0 ? n_models : 1) * (n_wavenumbers > 0 ? n_wavenumbers : 1) * n_sources;
    }
    // point sources (wost_set_point_sources): the charges (n_sources counts their source
    // channels then), the Neumann segment(s) each lies on ([2 n], -1: none) and their device
    // image (WalkArgs::charges, kChargeWords words)
    std::vector<wost_point_charge> charges;
    std::vector<int32_t> charge_seg;
    wost::DeviceBuffer<float> d_charges;
    wost::DeviceBuffer<int32_t> d_point_code;   // boundary_code of the query points (WalkArgs::point_code)
    wost::DeviceBuffer<int32_t> d_point_list;   // the point list of a solve (WalkArgs::point_list)
    // Green's function map of a solve (wost_solve_range_tally): the int64 sums
    // [n_points][replicas][cells + 1] and the flag word (WalkArgs::tally, tally_flag)
    wost::DeviceBuffer<long long> d_tally;
    wost::DeviceBuffer<uint32_t> d_tally_flag;
    // ... and of a channel-map solve (wost_solve_range_tally_channels) the combination weights
    // float [n_maps][channels] (WalkArgs::tally_weights), uploaded per solve
    wost::DeviceBuffer<float> d_tally_weights;
    bool has_source() const { return fields[wost::SLOT_F].present || !charges.empty(); }
    bool delta = false;
    double sigma_bar = 0.0;
    wost::Program prog;
    std::vector<float> table;   // sampler nodes (built on first use)
    bool table_ready = false;
    bool prog_dirty = true;
    uint64_t prog_version = 0;  // bumped whenever the program is rebuilt

    // compat="fixed" delta tracking: refuse solves whose walks would all hit maxSteps
    bool fixed_step_check = true;
    int trig_mode = WOST_TRIG_AUTO;       // wost_set_trig

    // kernel and launch options (wost_set_option; study builds: also the A/B environment)
    wost::Options opt;

    // field-specialised walk kernel (wost_jit.cpp)
    bool jit_enabled = true;
    hipFunction_t jit_fn = nullptr;
    hipFunction_t jit_alpha_fn = nullptr;   // the same module's wost_point_alpha_jit (delta tracking)
    std::optional<wost::KernelVariant> jit_variant;   // the variant jit_fn was looked up for (empty: none)
    uint64_t jit_version = ~0ull;                     // ... and the program's version then
    bool jit_cached(const wost::KernelVariant& v) const { return jit_variant == v && jit_version == prog_version; }
    std::string jit_error;

    // Neumann segment tree (wost_tree.h): used when the Neumann polyline has at
    // least tree_min_segments segments (< 0: never)
    int tree_min_segments = WOST_TREE_MIN_SEGMENTS_DEFAULT;
    int tree_leaf = WOST_TREE_LEAF_DEFAULT;
    bool tree_ready = false;
    wost::SegmentTreeHost tree;
    wost::DeviceBuffer<float> d_tree;
    // Dirichlet segment tree (wost_set_dirichlet_tree): the field-specialised kernel's
    // Dirichlet distance goes through it when the polyline admits it (dtree_usable, decided
    // once at creation: wost_tree.h dirichlet_tree_usable), has at least dtree_min_segments
    // segments (< 0: never) and is not compiled into the kernel
    int dtree_min_segments = WOST_DTREE_MIN_SEGMENTS_DEFAULT;
    int dtree_leaf = WOST_DTREE_LEAF_DEFAULT;
    bool dtree_usable = false;
    bool dtree_ready = false;
    bool dtree_last = false;   // the last solve's walk kernel used it
    wost::SegmentTreeHost dtree;
    wost::DeviceBuffer<float> d_dtree;

    hipStream_t stream = nullptr;
    hipEvent_t ev[7] = {};
    wost::DeviceBuffer<float2> d_dverts, d_nverts;
    wost::DeviceBuffer<float> d_seg_phi;
    wost::DeviceBuffer<float> d_table;
    wost::DeviceBuffer<char> d_prog;
    wost::DeviceBuffer<unsigned long long> d_counter;   // the walk launches' control words (wost_walk.h kCtlWords)
    wost::DeviceBuffer<float> d_val;                    // per-walk values and steps
    wost::DeviceBuffer<uint32_t> d_steps;
    wost::DeviceBuffer<char> d_stage;   // device image of the pinned staging's [points | block ranges]
    float2* d_points = nullptr;         // (d_points and d_begin point into d_stage)
    int64_t* d_begin = nullptr;
    wost::DeviceBuffer<double> d_bstats;
    // weighted channel combinations (wost_solve_range_combined): the weights [L][C] and the
    // combined block rows [blocks][2L+1] of a solve, and the HIP-event time of its combine kernels
    wost::DeviceBuffer<double> d_cweights, d_cstats;
    double combine_ms = 0.0;
    wost::DeviceBuffer<float> d_point_alpha;   // alpha at the query points (delta tracking)
    wost::DeviceBuffer<uint32_t> d_pool;       // walk pools of the tree kernels' workgroups (WalkArgs::pool)
    double tick_khz = 100000.0;       // the device wall clock (hipDeviceAttributeWallClockRate)
    // pinned host staging of a solve's small copies (points, block ranges, block sums):
    // a pageable hipMemcpyAsync costs ~9 us of host time each (profiles/r05_ab/host_path/)
    wost::PinnedBuffer h_pin;
    bool counter_zero = false;        // d_counter is 0 (the block reduce resets it after each walk launch)
    wost::Batch batch;                // the current launch's plan (wost_launch.h; its block list is reused)
    wost_timing timing{};
};

namespace wost {

// A handle's owner: wost_destroy, which also takes the device-less handles of create_host.
struct HandleDeleter {
    void operator()(wost_handle* h) const { wost_destroy(h); }
};
using HandlePtr = std::unique_ptr<wost_handle, HandleDeleter>;

// ---- the handle's small questions, inline: the per-solve path asks them ----

// The sampler kind ensure_table builds for a handle. kind 0: Green's, 1: the
// Jacobian-corrected Green's (compat fixed), 2: screened.
inline int sampler_kind(const wost_handle* h) {
    if (h->compat == WOST_COMPAT_FIXED) return 1;
    return h->delta ? 2 : 0;
}

// wost_set_trig's choice for this handle: WOST_TRIG_AUTO is exact for a Neumann polyline
// of >= 3 segments (a curved boundary, where a direction's last ulp decides where the
// walk goes), the hardware's sin/cos otherwise
inline bool exact_trig_of(const wost_handle* h) {
    if (h->trig_mode != WOST_TRIG_AUTO) return h->trig_mode == WOST_TRIG_EXACT;
    return (int)(h->nverts.size() / 2) - 1 >= 3;
}

inline bool use_tree(const wost_handle* h) {
    const int nseg = (int)(h->nverts.size() / 2) - 1;
    return nseg >= 1 && h->tree_min_segments >= 0 && nseg >= h->tree_min_segments;
}

// Whether the handle's field-specialised kernels find the Dirichlet distance through the
// Dirichlet tree (a polyline short enough to be compiled in keeps poly_distance_const).
inline bool use_dtree(const wost_handle* h) {
    const int nd = (int)(h->dverts.size() / 2);
    return h->jit_enabled && h->dtree_usable && h->dtree_min_segments >= 0 && nd - 1 >= h->dtree_min_segments &&
           !jit_const_dirichlet(h->opt, nd);
}

// The traits of the handle's walks with a source term or not (delta tracking needs one:
// check_request refuses the solve without).
inline WalkTraits walk_traits(const wost_handle* h, bool src) {
    const bool neu = !h->nverts.empty();
    return WalkTraits{.neu = neu, .src = src || h->delta, .delta = h->delta, .tree = neu && use_tree(h),
                      .fix = h->compat == WOST_COMPAT_FIXED};
}
inline WalkTraits walk_traits(const wost_handle* h) { return walk_traits(h, h->has_source()); }

// ---- wost_resources.cpp ----
void sampler_nodes_prefetch(int kind, double sigma_bar);
const std::vector<float>& fixed_screened_table();
int ensure_table(wost_handle* h);
int ensure_tree(wost_handle* h);
int ensure_dtree(wost_handle* h);
int upload_program(wost_handle* h);
int upload_charges(wost_handle* h);

// ---- wost_kernel_choice.cpp ----
constexpr int kTreeLdsDefaultLevel = 2;
// The kernel a solve launches first (its occupancy fallback may then stage
// less): the workgroup, the segment tree's staging, and whether the polylines are read
// from global memory. Shared by choose_kernel, solve_race and wost_prepare_sources, so that
// a raced or prepared kernel is the one the solve looks up.
struct KernelShape {
    int block = kWalkBlock, tree_verts = 0, tree_level = kTreeLdsDefaultLevel, tree_lds = 0;
    bool gpoly = false;
    bool dtree = false;   // the Dirichlet distance through the Dirichlet tree (no Dirichlet vertex staged)
    // the staging level compiled into the kernel (tree_lds_records)
    int stage() const { return tree_lds > 0 ? (tree_verts > 0 ? 2 : 1) : 0; }
};
// The kernel a solve launches and how it fits a CU.
struct KernelChoice {
    hipFunction_t jfn = nullptr;   // the field-specialised kernel; null: the precompiled one
    KernelShape shape;             // (of the precompiled one: 256 threads, nothing of the tree staged)
    size_t lds = 0;                // dynamic LDS of a workgroup
    int blocks_per_cu = 0;
    double jit_ms = 0.0;           // host time spent compiling
};
KernelVariant kernel_variant(const wost_handle* h, const WalkTraits& t, const KernelShape& ks, bool record,
                             int n_sources, bool point_list = false, bool tally = false, int tally_maps = 0);
int first_kernel_shape(const wost_handle* h, const WalkTraits& t, KernelShape* ks);
JitTry jit_kernel_try(wost_handle* h, const KernelVariant& v, JitTicket* ticket);
int choose_kernel(wost_handle* h, const WalkTraits& t, bool record, int n_src, int ns, KernelChoice* kc,
                  bool point_list = false, bool tally = false, int tally_maps = 0);

// ---- wost_solve.cpp ----
constexpr int64_t kMaxBatchWalks = int64_t(1) << 26;   // 64 Mi walks = 512 MiB of per-walk results
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
    // the point list of wost_solve_range_points (null: none): the walk range of these n_ids
    // points only; every output then has n_ids rows in list order
    const int32_t* point_ids = nullptr;
    int64_t n_ids = 0;
    int64_t rows() const { return point_ids ? n_ids : n_points; }   // point rows of the outputs
    // wost_solve_range_tally (null: none): the solve's launches add their deposits to the
    // handle's tally buffer, which the entry point has sized and zeroed and reads afterwards
    const struct TallyRequest* tally = nullptr;
};
// The tally of a solve: the grid (accepted: tally_grid_check), the rows per point, the scale
// 2^scale_log2 and the power of two a quantised deposit must stay below.
struct TallyRequest {
    wost_tally_grid grid{};
    int32_t replicas = 1;
    int32_t scale_log2 = 0;
    int64_t limit = 1;
    // channel maps (wost_solve_range_tally_channels; 0: the one-channel tally): the maps kept and
    // their weights [n_maps][channels] on the host (checked: tally_check_weights)
    int32_t n_maps = 0;
    const float* weights = nullptr;
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
    // weighted channel combinations (wost_combine.h; null / 0: none): n_combinations rows of
    // weights [L][channels], reduced on the device into rows of 2L+1 doubles per block and
    // per point (the point rows added in block order, like point_stats)
    const double* weights = nullptr;
    int32_t n_combinations = 0;
    double* combined_block_stats = nullptr;
    double* combined_point_stats = nullptr;
};
int solve_impl(wost_handle* h, const SolveRequest& rq, const SolveOutputs& out);

// ---- wost_tally.cpp ----
int tally_grid_check(const wost_tally_grid* g);
int64_t tally_row_walks(int64_t w0, int64_t w1, int32_t R, int64_t* rows);
int tally_limit(int64_t W, int64_t w0, int64_t w1, int32_t R, int32_t max_steps, int64_t* limit);
int tally_check_weights(const float* weights, int32_t n_maps, int32_t n_channels);

// ---- wost_point_sources.cpp ----
void segments_at(const float* nv, int nn, float x, float y, int32_t* s0, int32_t* s1);
int32_t code_of_segment(const wost_handle* h, int seg);
int check_point_sources(const wost_handle* h, const wost_point_charge* charges, int32_t n, int32_t n_sources);

// ---- wost_api.hip ----
int create_host(const wost_problem* pb, HandlePtr* out);
int fields_with_sources(const wost_handle* h, const wost_field* const* sources, int32_t n, HostField* out);
int check_models(const wost_handle* h, int32_t n, const std::vector<HostField>& conv);
void install_models(wost_handle* h, int32_t n, std::vector<HostField>& conv);

}  // namespace wost

#endif  // !WOST_PROGRAM_ONLY
