// wost_walk.h -- the walk loop of WostSolver_2D._solveUnified
// (reference: solvers/WoStSolver.py:182-311) as a device function template,
// instantiated by the precompiled kernels (wost_kernels.hip, fields read from
// a program buffer) and by the hiprtc-specialised kernels (wost_jit.cpp,
// fields compiled in). Compiled by hipcc and by hiprtc: no system headers.
//
// One walk per lane:
//  * persistent waves; each lane holds one walk's state in registers;
//  * when walks finish, the wave re-fills those lanes by __ballot / __popcll
//    rank from a chunk of walk ids it dequeued with one atomic (active-mask
//    compaction, so short walks never idle a lane for long);
//  * polyline vertices, the sampler's inverse-CDF table and (up to 1024) query
//    points staged in LDS; the segment loops are wave-uniform (LDS broadcasts);
//  * Philox4x32-10 counters derived from (seed, walk id, step): no RNG state.
#pragma once

#include "wost_device.h"
#if !defined(__HIPCC_RTC__)
#include "wost_variant.h"   // (host side only: WalkLds below)
#endif

namespace wost {

// Arguments of the walk kernel, passed by value in the kernarg segment.
struct WalkArgs {
    const float2* points;        // [n_points] query points
    const float2* dverts;        // Dirichlet polyline vertices
    const float2* nverts;        // Neumann polyline vertices (may be null)
    const float* table;          // sampler inverse-CDF nodes (may be null)
    const char* prog;            // DProgram + terms + factors (interpreted fields)
    float* out_val;              // [count] per-walk estimate
    uint32_t* out_steps;         // [count] per-walk step count
    unsigned long long* counter; // the launch's control words (kCtlWords, zeroed before launch): [0] the
                                 // work-queue head; the per-wave launch statistics after them
    int64_t wid_begin;           // global id of local walk 0
    int64_t count;               // walks in this launch
    int64_t walks_per_point;     // W: point of global walk g is g / W
    int32_t nd, nn;              // vertex counts
    int32_t max_steps;
    float eps;
    float rmin;                  // eps / 2 (solvers/WoStSolver.py:167)
    uint32_t key0, key1;         // Philox key = seed
    int32_t chunk;               // walks claimed per work-queue dequeue
    int32_t n_points;            // query points
    double inv_walks_per_point;  // 1/W for the point index of a walk id
    const float* seg_phi;        // [nn-1] atan2 of each Neumann segment's left normal
    float* rec;                  // walk recorder (return_history), or null: kRecFloats floats per
                                 // record, rec_stride records per local walk
    int32_t rec_stride;          // max_steps + 1
    const float4* tree;          // Neumann segment tree (TREE kernels; wost_device.h SegTree)
    int32_t tree_first_leaf;
    int32_t tree_leaf;
    float tree_tol;
    float tree_stop2;            // largest float whose sqrtf is <= rmin (< 0: none); silhouette_distance_tree
    float tree_kmax;             // SegmentTreeHost::kmax
    int32_t tree_lds_records;    // records staged in LDS (the first ones, 128 B each; field-specialised
                                 // kernels with kTreeStageBlock-thread workgroups), or 0: read through L1/L2
    int32_t tree_depth;          // level of the tree's leaves
    int32_t tree_lds_verts;      // Neumann vertices staged in LDS after the records (kTreeStageVertsBlock
                                 // workgroups, WOST_TREE_VSTAGED kernels), or 0
    // walk-range batches (wost_solve_range): when range_walks > 0, local walk l is walk
    // range_offset + l % range_walks of point range_point0 + l / range_walks, i.e. global
    // id (range_point0 + l / range_walks) * walks_per_point + range_offset + l % range_walks
    int64_t range_walks;
    int64_t range_offset;
    int64_t range_point0;
    double inv_range_walks;
    // delta tracking: alpha at each query point (point_alpha_body, same fields and
    // arithmetic as the walk's own alpha), read at a walk's start instead of
    // evaluating the field there
    const float* point_alpha;
    // 32-bit point index of a walk (the refill's quotient): wid_begin = base_pid * W +
    // base_off, and when base_off + count < 2^31 (small32) the quotient of base_off +
    // local index by W is taken in 32 bits (a double estimate and one correction)
    int64_t base_pid;
    uint32_t base_off;
    int32_t small32;
    // walk pools (TREE kernels, WOST_TREE_POOL; null: none): pool_wg_words words per
    // workgroup, a 4-word header (lock, walks parked near, walks parked far) and then
    // per class pool_slots parked walks of pool_fields(NS) words each (field-major);
    // a walk is "near" while its point lies in pool_box (x0, y0, x1, y1)
    uint32_t* pool;
    int32_t pool_slots;
    int32_t pool_wg_words;
    float4 pool_box;
    int32_t pool_near_waves;     // the workgroup's first pool_near_waves waves take the near walks
                                 // (0: each wave takes the class most of its walks are in)
    int32_t exact_trig;          // precompiled kernels: the direction's cos/sin correctly rounded
                                 // (wost_set_trig; the field-specialised kernels fix it at compile time)
    // the work queue's static first fill: wave v of the grid starts with local walks
    // [v * chunk0, (v + 1) * chunk0) (clamped to count) without touching the counter, and
    // the counter's dequeues start at queue_base = waves * chunk0 (>= count: none)
    int32_t chunk0;
    int64_t queue_base;
    // adaptive dequeues (chunk_share > 0; walk_body's refill): a wave's dynamic dequeue takes
    // at least the walks that keep the whole grid below ~4e7 dequeues per second at the
    // grid's walk completion rate as this wave measures it -- the walks it has completed
    // since it started, over the wall-clock ticks, times the grid's `waves` -- and at most
    // chunk_share (count / (waves * 4): a quarter of a wave's even share). The launch shape
    // is thus a function of this call alone, never of an earlier one.
    uint32_t chunk_share;
    uint32_t waves;
    // 2.5-D wavenumbers (wost_set_wavenumbers; delta tracking): channel j of a walk weights a
    // collision by 1 - (sigma' + k2[j]) / sigma_bar. Read at run time (wave-uniform scalar
    // loads), so one kernel per (problem, NS, NK) serves every wavenumber set; all 0 when none
    // is set, and only kernels built with WOST_WAVENUMBERS read it.
    float k2[WOST_MAX_SOURCES];
    // point sources (wost_set_point_sources; read only by kernels built with a charge count
    // PC > 0): kChargeWords words, arrays of WOST_MAX_POINT_CHARGES entries each (ChargeWord).
    // Read at run time (wave-uniform scalar loads), so one kernel per (problem, PC, NS, NK)
    // serves every electrode set.
    const float* charges;
    // ... and boundary_code (wost_device.h) of each query point: a walk that starts on the
    // Neumann polyline starts as a walk that has just hit it there (PC > 0 kernels only)
    const int32_t* point_code;
    // Dirichlet segment tree (wost_set_dirichlet_tree; read only by kernels built with
    // WOST_DIRICHLET_TREE, through GenFields::dirichlet_distance): its records and the
    // scalars of SegTree; null / 0 otherwise
    const float4* dtree;
    int32_t dtree_first_leaf;
    int32_t dtree_depth;
    int32_t dtree_leaf;
    float dtree_kmax;
    // point list (wost_solve_range_points; read only by kernels built with WOST_POINT_LIST, in
    // walk-range batches): the n_sel ascending ids of the points solved. range_point0 and the
    // quotient l / range_walks then index this list, and the walk's point -- its id, its
    // Philox stream, its entry of points, point_alpha and point_code, all full-size arrays --
    // is point_list[range_point0 + l / range_walks]. Outputs stay indexed by the local walk.
    // Every launch can carry the list: the walk pools keep running with it (a parked walk
    // holds its own id and state, never its point), and so would the recorder (indexed by the
    // local walk), though no entry point records a list solve (solve_impl refuses). Null
    // otherwise.
    const int32_t* point_list;
    // Green's function map (wost_solve_range_tally; read only by kernels built with WOST_TALLY):
    // tally is [n_points][tally_replicas][tally_nx * tally_ny + 1] int64 sums of fixed-point
    // deposits (the last entry of a row: the outside bin), tally_flag one word that a deposit
    // beyond tally_limit raises (tally_deposit: to its exponent field + 1, by an atomic max). The grid as tally_cell (wost_device.h) takes it; tally_scale is
    // 2^s and tally_limit the power of two a quantised deposit must stay below. Null / 0 otherwise.
    long long* tally;
    uint32_t* tally_flag;
    float tally_x0, tally_y0, tally_dx, tally_dy, tally_inv_dx, tally_inv_dy;
    int32_t tally_nx, tally_ny;
    int32_t tally_replicas;
    float tally_scale, tally_limit;
    // channel maps (wost_solve_range_tally_channels; read only by kernels built with
    // WOST_TALLY_MAPS T): tally is then [n_points][tally_replicas][T][bins] and tally_weights the
    // float [T][C] combination weights of the launch's C channels, tally_n_weights = T * C of
    // them. Run-time data behind a pointer (wave-uniform scalar loads through the constant
    // address space), so one kernel per (problem, channels, T) serves every combination. Null /
    // 0 otherwise.
    const float* tally_weights;
    int32_t tally_n_weights;
};

// The Dirichlet polyline's tree as poly_distance_tree reads it (records and vertices through
// global loads; the line-test tolerance is the ray query's and unused).
__device__ __forceinline__ SegTree dirichlet_seg_tree(const WalkArgs& A) {
    return SegTree{A.dtree, A.dverts, A.nd, A.dtree_first_leaf, A.dtree_depth, A.dtree_leaf, 0.0f, A.dtree_kmax};
}

// Offsets of the per-charge arrays in WalkArgs::charges: position (x, y interleaved),
// strength, alpha at the charge (delta tracking: point_alpha_body's bits), and as ints the
// source channel and the Neumann segment(s) the charge lies on (-1: none; two at a vertex).
enum ChargeWord : int {
    CHG_XY = 0,
    CHG_Q = 2 * WOST_MAX_POINT_CHARGES,
    CHG_ALPHA = 3 * WOST_MAX_POINT_CHARGES,
    CHG_SOURCE = 4 * WOST_MAX_POINT_CHARGES,
    CHG_SEG0 = 5 * WOST_MAX_POINT_CHARGES,
    CHG_SEG1 = 6 * WOST_MAX_POINT_CHARGES
};
constexpr int kChargeWords = 7 * WOST_MAX_POINT_CHARGES;
// word i of the charge buffer, as a scalar load from constant memory
__device__ __forceinline__ float charge_float(const float* c, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const __attribute__((address_space(4))) float*)c)[i];
#else
    return c[i];
#endif
}
__device__ __forceinline__ int charge_int(const float* c, int i) {
    return __builtin_bit_cast(int, charge_float(c, i));
}

// The refill's id arithmetic: local walk `lid` of the launch `A` -> its global walk id `wid`
// and its point index `pid` (uint64_t lvalues). Integer quotients without a 64-bit division:
// a double estimate (exact operands below 2^53) and one correction. Three paths, chosen by
// the launch (wost_launch.h next_batch): walk-range batches (local index < 2^26, one launch:
// a 32-bit quotient), 32-bit offsets (small32), and 64 bits.
// A statement macro and not a function: walk_body expands it, and walk_of_local below wraps
// the same text for the host check (tests/native/walk_ids_check.cpp). As a forced-inline
// function called from walk_body it changed the register allocation of the segment-tree
// kernels; expanded in place their code is instruction for instruction what it was.
// WOST_WALK_ID_CORRECTED(path, dir): the host check's counter of the corrections that fire
// (path 0 range, 1 small32, 2 64-bit; dir -1 / +1); nothing in the kernels.
// WOST_POINT_LIST (default 0; wost_jit.cpp defines it for a KernelVariant with point_list): a
// fourth way to place a walk -- the range path's quotient indexes WalkArgs::point_list, and
// the list's entry is the point. Compile-time for the reason above: a data-driven branch on
// the list pointer in every kernel would change the kernels that never see a list.
#ifndef WOST_WALK_ID_CORRECTED
#define WOST_WALK_ID_CORRECTED(path, dir)
#endif
#ifndef WOST_POINT_LIST
#define WOST_POINT_LIST 0
#endif
#if WOST_POINT_LIST
#define WOST_RANGE_POINT(A, q) ((uint64_t)(uint32_t)A.point_list[(uint64_t)A.range_point0 + q])
#else
#define WOST_RANGE_POINT(A, q) ((uint64_t)A.range_point0 + q)
#endif
#define WOST_WALK_OF_LOCAL(A, lid, wid, pid) \
    if (A.range_walks > 0) { \
        const uint32_t l32 = (uint32_t)lid, rw = (uint32_t)A.range_walks; \
        uint32_t q = (uint32_t)((double)l32 * A.inv_range_walks); \
        int32_t rem = (int32_t)(l32 - q * rw); \
        if (rem < 0) { --q; rem += (int32_t)rw; WOST_WALK_ID_CORRECTED(0, -1) } \
        else if (rem >= (int32_t)rw) { ++q; rem -= (int32_t)rw; WOST_WALK_ID_CORRECTED(0, +1) } \
        pid = WOST_RANGE_POINT(A, q); \
        wid = pid * (uint64_t)A.walks_per_point + (uint64_t)A.range_offset + (uint64_t)rem; \
    } else if (A.small32) { \
        const uint32_t local = A.base_off + (uint32_t)lid, w32 = (uint32_t)A.walks_per_point; \
        uint32_t q = (uint32_t)((double)local * A.inv_walks_per_point); \
        const int32_t rem = (int32_t)(local - q * w32); \
        if (rem < 0) { --q; WOST_WALK_ID_CORRECTED(1, -1) } \
        else if (rem >= (int32_t)w32) { ++q; WOST_WALK_ID_CORRECTED(1, +1) } \
        pid = (uint64_t)A.base_pid + q; \
        wid = (uint64_t)A.wid_begin + lid; \
    } else { \
        wid = (uint64_t)A.wid_begin + lid; \
        pid = (uint64_t)((double)wid * A.inv_walks_per_point); \
        const int64_t rem = (int64_t)(wid - pid * (uint64_t)A.walks_per_point); \
        if (rem < 0) { --pid; WOST_WALK_ID_CORRECTED(2, -1) } \
        else if (rem >= A.walks_per_point) { ++pid; WOST_WALK_ID_CORRECTED(2, +1) } \
    }

// WOST_WALK_OF_LOCAL as a function: the point index of local walk lid, its global id in *wid.
WOST_HD uint64_t walk_of_local(const WalkArgs& A, uint64_t lid, uint64_t* wid) {
    uint64_t pid, g;
    WOST_WALK_OF_LOCAL(A, lid, g, pid)
    *wid = g;
    return pid;
}

// The walk launch's control words (WalkArgs::counter): [0] the work-queue head, [1] the
// block reduce's finished-workgroup count, [2] its longest walk (kernels without wave
// records), [3] unused; then per wave two uint4 of launch statistics: {start tick low, high,
// last dequeue - start, end - start} and {loop iterations, longest walk, 0, 0} (wave index
// as in the static chunks). Derived from the
// queue's own pointer so that the walk loop keeps no extra pointer live.
constexpr int kCtlWords = 4;
WOST_HD constexpr size_t ctl_words(int64_t waves) { return (size_t)kCtlWords + 4 * (size_t)waves; }

// words of one parked walk: global id (2), local index (2), x, y, dD, step | onB << 31,
// phi, w, alpha(x), then the NS source totals
WOST_HD constexpr int pool_fields(int ns) { return 11 + ns; }
WOST_HD constexpr int pool_wg_words(int ns, int slots) { return 4 + 2 * pool_fields(ns) * slots; }

// The GPU's constant-rate wall clock (s_memrealtime, 100 MHz on gfx950: hipDeviceAttribute-
// WallClockRate), low 32 bits: differences are exact for launches shorter than ~42 s.
__device__ __forceinline__ uint64_t wall_ticks64() {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__builtin_amdgcn_s_memrealtime();
#else
    return 0ull;
#endif
}
__device__ __forceinline__ uint32_t wall_ticks() { return (uint32_t)wall_ticks64(); }
// the grid's dequeue budget (~4e7 per second) per tick of the 100 MHz wall clock, inverted
constexpr float kDequeuesPerTickInv = 1.0e8f / 4.0e7f;
// The scan kernels' adaptive dequeues and launch statistics (walk_body). The segment-tree
// kernels compile neither: their registers are full (96 VGPRs at 5 waves per SIMD, with
// spills), their long walks take the host's 16-walk chunks, and the wave state they need
// cost the C5 kernel ~4% (profiles/r06_ab/).
#ifndef WOST_ADAPTIVE_DEQ
#define WOST_ADAPTIVE_DEQ 1
#endif
#ifndef WOST_WAVE_STATS
#define WOST_WAVE_STATS 1
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define WOST_KEEP_VGPR(v) __asm__ volatile("" : "+v"(v))
#else
#define WOST_KEEP_VGPR(v) ((void)0)
#endif

// Sum over the wave's lanes (every lane active), as a wave-uniform value.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// alpha at the query points with the walk kernel's own Fields policy (the same
// function the walk would evaluate at its start point, hence the same bits).
template <class F>
__device__ __forceinline__ void point_alpha_body(const float2* pts, int64_t n, float* out, const F& fld) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float2 q = pts[i];
        out[i] = fld.alpha(q.x, q.y);
    }
}
// ... of every model of a model-batched kernel (NM > 1): out[m * n + i] = alpha_m(pts[i])
template <int NM, class F>
__device__ __forceinline__ void point_alpha_multi_body(const float2* pts, int64_t n, float* out, const F& fld) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float2 q = pts[i];
        float a[NM];
        fld.alpha_multi(q.x, q.y, a);
#pragma unroll
        for (int m = 0; m < NM; ++m) out[(int64_t)m * n + i] = a[m];
    }
}

constexpr int kWalkBlock = 256;
// workgroup of the field-specialised tree kernels that stage the tree's records in LDS:
// 8 waves, two per SIMD, so two workgroups per CU place 4 waves on every SIMD (a
// 640-thread workgroup places 3-3-2-2 and a second one no longer fits 5 per SIMD:
// profiles/r03_tree/tree_lds_block_ab.log; WOST_TREE_LDS_BLOCK for A/B)
constexpr int kTreeStageBlock = 512;
// ... and of those that stage the polyline's vertices as well: one 16-wave workgroup per CU
constexpr int kTreeStageVertsBlock = 1024;

// Walk recorder (solvers/WoStSolver.py:197-309, return_history). Record k < steps
// of a walk is its step k: the pre-step point and its distances (:218-222), the
// source sample point after clipping and its contribution (:261-266).
// Record `steps` is the end: final point (REC_X, REC_Y), boundary contribution
// (REC_C) and the walk's total (REC_AUX) (:301-306). A step record's REC_AUX is
// 1 when the step sampled the source.
constexpr int kRecFloats = WOST_REC_FLOATS;   // include/wost.h, wost_solve_history
enum RecField { REC_X = 0, REC_Y, REC_DD, REC_DN, REC_SX, REC_SY, REC_C, REC_AUX };

WOST_HD size_t align16(size_t b) { return (b + 15) & ~size_t(15); }

// LDS scratch of one wave for the cooperative tree queries (below): the hand-out
// slots and one result slot per owner lane
struct TreeWaveScratch {
    uint32_t task[64];             // owner | level << 6 | position << 10
    unsigned long long slot[64];   // silhouette: float bits of the squared distance; ray: s bits << 32 | segment
};
constexpr size_t kTreeWaveScratchBytes = sizeof(TreeWaveScratch);

// Bytes of dynamic LDS a walk-kernel workgroup needs, in layout order:
//  * G_norm cells (delta tracking; else a 16-byte pad): sample_rho_tail reads the
//    word before the sampler's tail;
//  * the sampler's nodes 1..N-1 (node 0 is a kernel argument);
//  * the Dirichlet vertices, unless the Fields policy has them compiled in;
//  * the Neumann vertices and segment angles (scan kernels), also when compiled in
//    (walk_body kStageN);
//  * with the segment tree, its first tree_lds records (128 B each), the tree_verts
//    staged Neumann vertices, then one TreeWaveScratch per wave (the cooperative
//    tree queries) of the `block`-thread workgroup.
// Query points are read from global memory (once per walk, at refill).
#if !defined(__HIPCC_RTC__)   // the host sizes the launch; a run-time-compiled source never does
struct WalkLds {
    WalkTraits traits;
    int nd = 0, nn = 0;              // vertex counts
    int tree_lds = 0;                // records of the segment tree staged
    int tree_verts = 0;              // Neumann vertices staged after them
    bool const_d = false;            // the Dirichlet polyline is compiled in (field-specialised kernels)
    bool global_polylines = false;   // nothing of the polylines is staged (wost_walk.h GL)
    int block = kWalkBlock;          // threads per workgroup
    bool dirichlet_tree = false;     // the Dirichlet distance through its tree: no Dirichlet vertex staged
};
WOST_HD size_t walk_lds_bytes(const WalkLds& k) {
    const WalkTraits& t = k.traits;
    size_t b = 0;
    if (t.src) b += t.delta ? sizeof(float4) * (size_t)kGnormCells : 16;
    if (t.src) b += sizeof(float) * (size_t)kSamplerTailFloats;
    b = align16(b);
    if (!k.const_d && !k.global_polylines && !k.dirichlet_tree) b += align16(sizeof(float2) * (size_t)k.nd);
    if (t.neu && !t.tree && !k.global_polylines)
        b += align16(sizeof(float2) * (size_t)k.nn) + align16(sizeof(float) * (size_t)(k.nn > 1 ? k.nn - 1 : 0));
    if (t.tree)
        b += 8 * sizeof(float4) * (size_t)k.tree_lds + align16(sizeof(float2) * (size_t)k.tree_verts) +
             kTreeWaveScratchBytes * (size_t)((k.block + 63) / 64);
    return b;
}
#endif

// ---------------------------------------------------------------------------
// Wave-cooperative segment-tree queries (TREE kernels; compat="fixed" too, its ray
// query keyed by the nearest crossing's (t, segment)). The records and, when they
// fit, the vertices are read from LDS (WOST_TREE_STAGED / WOST_TREE_VSTAGED kernels).
//
// silhouette_distance_tree / intersect_polylines_tree run one query per lane, and a
// wave iterates until its slowest lane is done: at C5's walk positions ~89% of the
// queries end after one or two record visits while the few near the surface need
// 20-40, so a tree instruction ran on ~12-19% of the lanes. Here the lanes of a wave
// share the work: when at most WOST_TREE_SHARE lanes still search, the searching
// lanes hand the subtrees pending in their traversal state (pend bits: the children
// of an ancestor still to visit) to idle lanes, which search them for the same query
// (the owner's registers, read with a lane shuffle) and leave their result in the
// owner's LDS slot. Both queries are minima that do not depend on the visiting order
// (the silhouette query's squared distance, the ray query's lexicographic (s, segment)
// -- the scan's first argmin), so the answer is bit for bit the per-lane search's.
// Shared bounds only prune more: at each hand-out the silhouette searches of one
// owner take the smallest squared distance found so far by any of them.
// Every lane of the wave calls these together (no lane may have left the loop body).
// ---------------------------------------------------------------------------
#ifndef WOST_TREE_SHARE   // hand out pending subtrees when at most this many lanes search
#define WOST_TREE_SHARE 32
#endif
#ifndef WOST_TREE_SHARE_DESCENT   // also at every level of the descent (else once per leaf round)
#define WOST_TREE_SHARE_DESCENT 1
#endif
#ifndef WOST_TREE_SHARE_MIN   // ... and at least this many subtrees are pending
#define WOST_TREE_SHARE_MIN 1
#endif
#ifndef WOST_TREE_BATCH   // children of a record whose words are loaded together (1, 2 or 4)
#define WOST_TREE_BATCH 4
#endif

// the LDS writes of the wave's lanes visible to its other lanes (a wave's LDS
// operations complete in order; this keeps the compiler from moving them)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The pending subtrees of the wave: per bit b of each lane's count n < 32 of pend
// bits, the ballot of that bit (so the total is scalar work and a lane's prefix
// offset is taken only when a hand-out happens).
struct PendCount {
    uint64_t m[5];
    uint32_t total;
};
__device__ __forceinline__ PendCount wave_pend_count(uint32_t n) {
    PendCount c;
    c.total = 0u;
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        c.m[b] = __ballot((n >> b) & 1u);
        c.total += (uint32_t)__popcll(c.m[b]) << b;
    }
    return c;
}

// Hand out pending subtrees: searching lanes (`live`, n = popcount(pend)) list their
// pend bits (the shallowest levels, i.e. the largest subtrees, first) into the idle
// lanes' slots; an idle lane that receives one becomes a helper: *owner, d, pos of the
// subtree's root, pend = 0. Returns true on the lanes that became helpers.
__device__ __forceinline__ bool tree_hand_out(TreeWaveScratch* ws, uint64_t live_mask, bool live, uint32_t n,
                                              const PendCount& pc, uint64_t lanes_below, int& owner, int& d, int& pos,
                                              uint32_t& pend) {
    const uint64_t idle = ~live_mask;
    const uint32_t nidle = (uint32_t)__popcll(idle);
    uint32_t off = 0u;   // exclusive prefix sum of n over the lanes below
#pragma unroll
    for (int b = 0; b < 5; ++b) off += (uint32_t)__popcll(pc.m[b] & lanes_below) << b;
    if (live && off < nidle) {
        const uint32_t give = n < nidle - off ? n : nidle - off;
        for (uint32_t i = 0; i < give; ++i) {
            const int b = lowest_bit(pend);
            pend &= pend - 1u;
            const int p = b >> 2, child = 4 * (pos >> (2 * (d - p))) + (b & 3);
            ws->task[off + i] = (uint32_t)owner | (uint32_t)(p + 1) << 6 | (uint32_t)child << 10;
        }
    }
    wave_lds_sync();
    const uint32_t rank = (uint32_t)__popcll(idle & lanes_below);
    const bool helper = !live && rank < (pc.total < nidle ? pc.total : nidle);
    if (helper) {
        const uint32_t tk = ws->task[rank];
        owner = (int)(tk & 63u);
        d = (int)((tk >> 6) & 15u);
        pos = (int)(tk >> 10);
        pend = 0u;
    }
    return helper;
}

// silhouette_distance_tree (wost_device.h), the wave's lanes sharing the search;
// `want`: this lane has a query. Same use contract (exact below dd and above rmin).
// (ic: loop counters of a WOST_TREE_ITER_STATS study build, else null and compiled away)
__device__ __forceinline__ float silhouette_distance_tree_wave(const SegTree& t, float px, float py, float dd,
                                                               float stop2, bool want, TreeWaveScratch* ws,
                                                               int lane, uint32_t* ic = nullptr) {
#pragma clang fp contract(off)
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    const int nv = t.nv, nseg = nv - 1;
    const float Town = (dd * dd) * 1.002f;
    ws->slot[lane] = (unsigned long long)__builtin_bit_cast(uint32_t, WOST_INF);
    // the query this lane searches for (its own, or its owner's as a helper)
    float qx = px, qy = py, T = Town;
    // its rounding scales (silhouette_child_keep_q, WOST_TREE_QMARGIN)
    auto qscale = [&]() { return ((fabsf(qx) + fabsf(qy)) + t.kmax) * 1.001f; };
    float qsl = 9.5367431640625e-07f * qscale(), qmc = kConeMargin * qscale();   // 2^-20 W, 1e-5 W
    int owner = lane;
    float best = WOST_INF;
    bool live = want && nv >= 3;
    int d = 0, pos = 0;
    uint32_t pend = 0u;
    float plb0 = WOST_INF, plb1 = WOST_INF, plb2 = WOST_INF, plb3 = WOST_INF, plb4 = WOST_INF;
    auto plb_get = [&](int l) {
        float v = -WOST_INF;
        v = l == 0 ? plb0 : v; v = l == 1 ? plb1 : v; v = l == 2 ? plb2 : v;
        v = l == 3 ? plb3 : v; v = l == 4 ? plb4 : v;
        return v;
    };
    auto plb_set = [&](int l, float x) {
        plb0 = l == 0 ? x : plb0; plb1 = l == 1 ? x : plb1; plb2 = l == 2 ? x : plb2;
        plb3 = l == 3 ? x : plb3; plb4 = l == 4 ? x : plb4;
    };
    auto visit = [&](int lvl, int at, uint32_t cand, int& nj, float& nb2) {
        if (ic) {
            ic[3] += 1u;                                                     // lane-visits
            if (lane == (int)__builtin_ctzll(__ballot(1))) ic[15] += 1u;    // the wave's visit issues
        }
        const int k = tree_level_offset(lvl) + at;
        const float bound = best < T ? best : T;
        uint32_t kept = 0u;
        float nb = WOST_INF;
        nb2 = WOST_INF;
        nj = 0;
        // the children's words loaded WOST_TREE_BATCH children at a time before any test
        // (one round trip per batch; tested one by one the loads waited in turn)
#pragma unroll
        for (int j0 = 0; j0 < 4; j0 += WOST_TREE_BATCH) {
            float4 w[2 * WOST_TREE_BATCH];
#pragma unroll
            for (int i = 0; i < 2 * WOST_TREE_BATCH; ++i) w[i] = t.word(k, 2 * j0 + i);
#pragma unroll
            for (int u = 0; u < WOST_TREE_BATCH; ++u) {
                const int j = j0 + u;
                float lb;
#if WOST_TREE_QMARGIN
                const bool keep = silhouette_child_keep_q(w[2 * u], w[2 * u + 1], qx, qy, bound, qsl, qmc, &lb);
#else
                const bool keep = silhouette_child_keep(w[2 * u], w[2 * u + 1], qx, qy, bound, &lb);
#endif
                if (((cand >> j) & 1u) && keep) {
                    kept |= 1u << j;
                    if (lb < nb) { nb2 = nb; nb = lb; nj = j; }
                    else if (lb < nb2) nb2 = lb;
                }
            }
        }
        return kept;
    };
    auto resume = [&]() {
        while (pend != 0u) {
            const int p = highest_bit(pend) >> 2;
            const uint32_t m = (pend >> (4 * p)) & 15u;
            pend &= ~(15u << (4 * p));
            const float bound = best < T ? best : T;
            if (plb_get(p) > bound) continue;
            const int anc = pos >> (2 * (d - p));
            int nj;
            float nb2;
            const uint32_t kept = visit(p, anc, m, nj, nb2);
            if (kept) {
                pend |= (kept & ~(1u << nj)) << (4 * p);
                plb_set(p, nb2);
                pos = 4 * anc + nj;
                d = p + 1;
                return true;
            }
        }
        return false;
    };
    // hand out pending subtrees when few lanes still search (a uniform branch)
    auto share = [&](uint64_t L) {
        if (!(__popcll(L) <= WOST_TREE_SHARE) || __ballot(live && pend != 0u) == 0ull) return;
        const uint32_t n = live ? (uint32_t)__popcll(pend) : 0u;
        const PendCount pc = wave_pend_count(n);
        if (WOST_TREE_SHARE_MIN > 1 && pc.total < WOST_TREE_SHARE_MIN) return;
        if (ic) ic[4] += 1u;
        // every lane leaves what it found in its owner's slot, then takes the owner's
        // best so far as its bound
        if (best < WOST_INF) atomicMin(&ws->slot[owner], (unsigned long long)__builtin_bit_cast(uint32_t, best));
        if (tree_hand_out(ws, L, live, n, pc, lanes_below, owner, d, pos, pend)) {
            live = true;
            best = WOST_INF;
            plb0 = plb1 = plb2 = plb3 = plb4 = WOST_INF;
        }
        qx = __shfl(px, owner);
        qy = __shfl(py, owner);
        T = __shfl(Town, owner);
        qsl = 9.5367431640625e-07f * qscale();
        qmc = kConeMargin * qscale();
        const float sb = __builtin_bit_cast(float, (uint32_t)ws->slot[owner]);
        best = sb < best ? sb : best;
        if (live && best <= stop2) { live = false; pend = 0u; }
    };
    if (ic) ic[0] += 1u;
    wave_lds_sync();
    for (;;) {
        const uint64_t L = __ballot(live);
        if (L == 0ull) break;
        if (ic) ic[1] += 1u;
        share(L);
#if WOST_TREE_SHARE_DESCENT
        // the descent as a uniform loop, so that a hand-out can run at every level
        for (;;) {
            const bool down = live && d < t.depth;
            if (!__any(down)) break;
            if (ic) ic[2] += 1u;
            if (down) {
#else
        {
            while (live && d < t.depth) {
#endif
                int nj;
                float nb2;
                const uint32_t kept = visit(d, pos, 15u, nj, nb2);
                if (kept) {
                    pend |= (kept & ~(1u << nj)) << (4 * d);
                    plb_set(d, nb2);
                    pos = 4 * pos + nj;
                    ++d;
                } else {
                    live = resume();
                }
            }
#if WOST_TREE_SHARE_DESCENT
            share(__ballot(live));
#endif
        }
        // (no `continue` in this loop: every lane must reach the next ballot)
        if (ic && __any(live)) ic[6] += 1u;
        if (live) {
            if (ic) ic[5] += 1u;
            const int s0 = pos * t.leaf;
            const int s1 = s0 + t.leaf < nseg ? s0 + t.leaf : nseg;
            const int j1 = s1 < nv - 2 ? s1 : nv - 2;
            bool stop = false;
            if (s0 + 1 <= j1) {
                const float2 va = t.vert(s0);
                float2 vb = t.vert(s0 + 1);
                float cprev = (vb.x - va.x) * (qy - va.y) - (vb.y - va.y) * (qx - va.x);
                // vertices loaded four at a time (indices clamped in range), then scanned
                for (int j0 = s0 + 1; j0 <= j1; j0 += 4) {
                    float2 vcs[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) vcs[u] = t.vert(j0 + 1 + u < nv ? j0 + 1 + u : nv - 1);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (j0 + u <= j1) {
                            const float2 vc = vcs[u];
                            const float bpx = qx - vb.x, bpy = qy - vb.y;
                            const float ccur = (vc.x - vb.x) * bpy - (vc.y - vb.y) * bpx;
                            if (cprev * ccur < 0.0f) {
                                const float d2 = bpx * bpx + bpy * bpy;
                                best = d2 < best ? d2 : best;
                            }
                            cprev = ccur;
                            vb = vc;
                        }
                    }
                }
                stop = best <= stop2;
            }
            if (stop) {
                live = false;
                pend = 0u;
            } else {
                live = resume();
            }
        }
    }
    if (best < WOST_INF) atomicMin(&ws->slot[owner], (unsigned long long)__builtin_bit_cast(uint32_t, best));
    wave_lds_sync();
    const float res = __builtin_bit_cast(float, (uint32_t)ws->slot[lane]);
    wave_lds_sync();   // the slots are rewritten by the next query
    return res == WOST_INF ? res : sqrt_rn(res);
}

// intersect_polylines_tree<NORMAL> (wost_device.h, reference mode), the wave's lanes
// sharing the search; `want`: this lane has a query.
// NEAREST (compat="fixed"): the nearest crossing of intersect_polylines_tree<.., true>,
// the lexicographic minimum of (t, segment), t > 0.
template <bool NORMAL = true, bool NEAREST = false>
__device__ __forceinline__ Hit intersect_polylines_tree_wave(const SegTree& t, float px, float py, float dxi,
                                                             float dyi, float r, bool want, TreeWaveScratch* ws,
                                                             int lane, uint32_t* ic = nullptr) {
#pragma clang fp contract(off)
    const uint64_t lanes_below = (1ull << lane) - 1ull;
    float dn, dx, dy;
    unit_direction(dxi, dyi, dn, dx, dy);
    const bool degenerate = dn < 1e-10f;
    const float qx0 = px + 1e-6f * dx, qy0 = py + 1e-6f * dy;
    const float tol0 = t.tol + 7.62939453125e-06f * (fabsf(qx0) + fabsf(qy0));   // + 2^-17 |q|_1
    const int nseg = t.nv - 1;
    ws->slot[lane] = ~0ull;
    float qx = qx0, qy = qy0, ddx = dx, ddy = dy, tol = tol0;
    int owner = lane;
    float best = WOST_INF;
    int bi = -1;
    bool live = want && !degenerate;
    // the pruning of intersect_polylines_tree's keep()
    auto keep = [&](float4 cu, float4 ab) {
        if (ab.x < 0.0f) return false;
        const float cx = cu.x - qx, cy = cu.y - qy;
        const float cr = ddx * cu.w - ddy * cu.z, dt = ddx * cu.z + ddy * cu.w;
        if (fabsf(ddx * cy - ddy * cx) > (ab.x * fabsf(cr) + ab.y * fabsf(dt)) + tol) return false;
#if !defined(WOST_NO_TREE_BEHIND)
        if (ab.z == 3.0f) return true;
        const float ahead = (ddx * cx + ddy * cy) + (ab.x * fabsf(dt) + ab.y * fabsf(cr));
        if (!(ahead < -(512.0f * tol + 1e-2f * ((fabsf(cx) + fabsf(cy)) + (ab.x + ab.y))))) return true;
        if (ab.z == 2.0f) return false;
        return !(ab.z * fabsf(cr) - ab.w * fabsf(dt) > 1e-3f);
#else
        return true;
#endif
    };
    int d = 0, pos = 0;
    uint32_t pend = 0u;
    auto resume = [&]() {
        if (pend == 0u) return false;
        const int p = highest_bit(pend) >> 2;
        const int j = lowest_bit((pend >> (4 * p)) & 15u);
        pend &= ~(1u << (4 * p + j));
        pos = 4 * (pos >> (2 * (d - p))) + j;
        d = p + 1;
        return true;
    };
    // (s, segment) as one 64-bit key: s >= 0 here, so its bits order like the floats
    // (s + 0 makes a -0 the +0 it ties with, leaving the segment index to decide)
    auto deposit = [&]() {
        if (bi >= 0)
            atomicMin(&ws->slot[owner], (unsigned long long)__builtin_bit_cast(uint32_t, best + 0.0f) << 32 |
                                            (unsigned long long)(uint32_t)bi);
    };
    auto share = [&](uint64_t L) {
        if (!(__popcll(L) <= WOST_TREE_SHARE) || __ballot(live && pend != 0u) == 0ull) return;
        const uint32_t n = live ? (uint32_t)__popcll(pend) : 0u;
        const PendCount pc = wave_pend_count(n);
        if (WOST_TREE_SHARE_MIN > 1 && pc.total < WOST_TREE_SHARE_MIN) return;
        if (ic) ic[11] += 1u;
        deposit();
        if (tree_hand_out(ws, L, live, n, pc, lanes_below, owner, d, pos, pend)) {
            live = true;
            best = WOST_INF;
            bi = -1;
        }
        qx = __shfl(qx0, owner);
        qy = __shfl(qy0, owner);
        ddx = __shfl(dx, owner);
        ddy = __shfl(dy, owner);
        tol = __shfl(tol0, owner);
    };
    if (ic) ic[7] += 1u;
    wave_lds_sync();
    for (;;) {
        const uint64_t L = __ballot(live);
        if (L == 0ull) break;
        if (ic) ic[8] += 1u;
        share(L);
#if WOST_TREE_SHARE_DESCENT
        for (;;) {
            const bool down = live && d < t.depth;
            if (!__any(down)) break;
            if (ic) ic[9] += 1u;
            if (down) {
#else
        {
            while (live && d < t.depth) {
#endif
                if (ic) ic[10] += 1u;
                const int k = tree_level_offset(d) + pos;
                uint32_t kept = 0u;
#pragma unroll
                for (int j0 = 0; j0 < 4; j0 += WOST_TREE_BATCH) {
                    float4 w[2 * WOST_TREE_BATCH];
#pragma unroll
                    for (int i = 0; i < 2 * WOST_TREE_BATCH; ++i) w[i] = t.word(k, 2 * j0 + i);
#pragma unroll
                    for (int u = 0; u < WOST_TREE_BATCH; ++u)
                        if (keep(w[2 * u], w[2 * u + 1])) kept |= 1u << (j0 + u);
                }
                if (kept) {
                    const int j = lowest_bit(kept);
                    pend |= (kept & ~(1u << j)) << (4 * d);
                    pos = 4 * pos + j;
                    ++d;
                } else {
                    live = resume();
                }
            }
#if WOST_TREE_SHARE_DESCENT
            share(__ballot(live));
#endif
        }
        const int s0 = pos * t.leaf;
        const int s1 = s0 + t.leaf < nseg ? s0 + t.leaf : nseg;
        if (ic && __any(live && s0 < s1)) ic[13] += 1u;
        if (ic && live && s0 < s1) ic[12] += 1u;
        if (NEAREST && live && s0 < s1) {
            float2 a = t.vert(s0);
            for (int i0 = s0; i0 < s1; i0 += 4) {   // vertices loaded four at a time
                float2 bs[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) bs[u] = t.vert(i0 + 1 + u <= nseg ? i0 + 1 + u : nseg);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (i0 + u < s1) {
                        const int i = i0 + u;
                        // t <= best (ties too: the lower segment index wins them)
                        const float bq = best < WOST_INF ? bits_to_float(__builtin_bit_cast(int32_t, best) + 1) : best;
                        const float tt = ray_segment_nearest_t(a, bs[u], qx, qy, ddx, ddy, bq);
                        if (tt < best || (tt == best && i < bi)) { best = tt; bi = i; }
                        a = bs[u];
                    }
                }
            }
        } else if (live && s0 < s1) {
            const float S = 2.0f * tol;
            const float m = fmaf(ddx, qy, -(ddy * qx));
            const float hi = m + S, lo = m - S;     // the thresholds of intersect_polylines_lines
            const float2 a = t.vert(s0);
            const float ca = fmaf(ddx, a.y, -(ddy * a.x));
            bool aprev = ca > hi, bprev = ca < lo;   // the filter of intersect_polylines_lines
            uint32_t cand = 0u;
            for (int i0 = s0; i0 < s1; i0 += 4) {   // vertices loaded four at a time
                float2 bs[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) bs[u] = t.vert(i0 + 1 + u <= nseg ? i0 + 1 + u : nseg);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (i0 + u < s1) {
                        const float cb = fmaf(ddx, bs[u].y, -(ddy * bs[u].x));
                        const bool ab = cb > hi, bb = cb < lo;
                        if (!((aprev && ab) || (bprev && bb))) cand |= 1u << (i0 + u - s0);
                        aprev = ab;
                        bprev = bb;
                    }
                }
            }
            while (cand != 0u) {
                const int i = s0 + lowest_bit(cand);
                cand &= cand - 1u;
                const float s = ray_segment_time_filtered(t.vert(i), t.vert(i + 1), qx, qy, ddx, ddy);
                if (s < best || (s == best && i < bi)) { best = s; bi = i; }
            }
        }
        if (live) live = resume();
    }
    deposit();
    wave_lds_sync();
    const unsigned long long key = ws->slot[lane];
    wave_lds_sync();   // the slots are rewritten by the next query
    if (degenerate) {
        Hit h;
        h.x = px; h.y = py; h.nx = 1.f; h.ny = 0.f; h.hit = false; h.seg = -1;
        return h;
    }
    const int wbi = key == ~0ull ? -1 : (int)(uint32_t)key;
    const float wbest = key == ~0ull ? WOST_INF : __builtin_bit_cast(float, (uint32_t)(key >> 32));
    if (NEAREST) return ray_nearest_finish(wbi, wbest, px, py, dx, dy, qx0, qy0, r);
    return intersect_finish<NORMAL>(t.v, wbi, wbest, px, py, dx, dy, qx0, qy0, r);
}

// The Fields policy F provides: has_g(), g(x,y), f(x,y), sigma(x,y),
// alpha(x,y), alpha_jet(x,y), detached(), sigma_bar(), sqrt_sigma_bar(),
// inv_sigma_bar(), and the polyline scans dirichlet_distance(sD,
// nd, x, y), neumann_silhouette_distance(sN, nn, x, y), neumann_intersect(sN,
// nn, x, y, dx, dy, r), neumann_intersect_nearest(...) (compat="fixed"),
// neumann_phi(sPhi, seg) (the interpreted kernels scan the
// staged vertices; the specialised ones may have them compiled in:
// F::kConstDirichlet / F::kConstNeumann, and then nothing is staged for them). TREE: Neumann queries through
// the segment tree. REC: the kernel can record walks (A.rec).
// NS > 1 (multi-source batching): the walk scores NS source
// fields at once -- the walk itself does not depend on the source, so every
// source's total is bit for bit what a single-source solve of it gives. The
// Fields policy then provides f_multi(x, y, float out[NS]); per-walk values go
// to out_val[local walk * NS + k].
// FIX (compat="fixed"): the estimator with the reference's quirks corrected
// (SURVEY 8a):
//  Q7/Q12 the walk stops when the CURRENT point's Dirichlet distance is <= eps
//         (no extra step inside the eps-shell; eps >= 1 no longer skips walks);
//  Q1     the Neumann ray query takes the nearest crossing along the ray;
//  Q2     after a Neumann hit the direction is uniform on the hemisphere of the
//         INWARD normal (the side the ray came from);
//  Q3     the source radius follows the Green's density with its Jacobian,
//         rho ln(1/rho) (the host builds that sampler table);
//  Q13    (Laplace / Poisson / mixed) the source sample takes its own direction
//         (Philox word w) and counts only if it is visible from x (no Neumann
//         crossing before it); on a Neumann boundary point that direction, like
//         the step's, is uniform on the inward hemisphere (the star-shaped region
//         is then a half-ball: the full ball's radial law over a half-circle of
//         directions gives the factor 2 of the boundary representation);
//  Q4/Q5  delta tracking draws the sample from the ball's screened Green's
//         function of THIS radius (shape s = R sqrt(sigma_bar), Jacobian
//         included, no clipped envelope; sample_rho_screened_fixed).
//  Delta tracking with Neumann boundaries needs more than the reference's
//  collision rule: along a ray that meets the boundary at distance d < R, the
//  screened Poisson kernel's weight there is t (K1(t) + c I1(t)) (t = d
//  sqrt(sigma_bar)), not 1/I0(R sqrt(sigma_bar)) -- per direction, the
//  no-collision probability must be 1 - sigma_bar |G| F_s(d / R). FIX draws the
//  sample on the step's ray and collides only when mu <= sigma_bar |G| AND the
//  sample lies before the ray's boundary point (probability F_s(d / R)), which is
//  exactly that, with the collision point from the truncated law; otherwise the
//  walk moves to the ray's point with weight 1. A collision leaves the Neumann
//  boundary, and its weight 1 - sigma'/sigma_bar is kept signed (unbiased for
//  any sigma_bar; the reference's max(., 0) at solvers/WoStSolver.py:282 is
//  biased wherever sigma' > sigma_bar).
// GL: the polylines (and segment angles) are read from global memory instead of being
// staged in LDS -- field-specialised kernels for polylines too long for the LDS budget
// (wost_api.hip kGlobalPolylineLdsBytes).
// NK > 1 (2.5-D wavenumber batching): under delta tracking a walk's path depends
// only on sigma_bar -- the step, the collision test and the sampler never read sigma' --
// and sigma' enters through the collision weight alone. The screened problem of wavenumber
// k has sigma'_k = sigma' + k^2 (A.k2[j]), so one walk carries NK attenuations w[j] and
// scores NK * NS channels, channel c = j * NS + s (wavenumber major): per-walk values go to
// out_val[local walk * NK * NS + c], and every channel's total is bit for bit that of a
// single solve of (k2[j], source s). Kernels built with WOST_WAVENUMBERS 1 read A.k2 (the
// precompiled ones, NK = 1, and the specialised ones of a handle with wavenumbers set); the
// others compile the add out, so a handle without wavenumbers runs the kernel it always ran.
// NK > 1 tree kernels run without walk pools (a parked walk holds one w).
// NM > 1 (shared-path model batching): the same argument for the whole (sigma,
// alpha) pair. The step, the collision test, the sampler and the Green's norm read sigma_bar
// and the geometry only; the conductivity enters through alpha_jet(y) and sigma(y) (the
// collision weight), alpha(next) / alpha(x) (the factor sqrt(a_new / alpha(x))), the source
// score's rsq(alpha(y) alpha(x)) and alpha(x0). One walk carries NW = NM * NK weights
// w[m * NK + j] and ax[NM], and scores NM * NK * NS channels, c = (m * NK + j) * NS + s (model
// major): each bit for bit the single solve of model m on this sigma_bar. The Fields policy
// then provides alpha_multi(x, y, float[NM]), alpha_jet_multi(x, y, Jet[NM]), sigma_multi(x,
// y, float[NM]) and detached_multi(m); A.point_alpha is [NM][n_points]. Field-specialised
// kernels only, no walk pools, no point charges.
// PC > 0 (point sources, FIX only): the handle's source is PC point charges
// q_p delta(z_p), charge p belonging to source channel s(p) (A.charges, run-time data). A
// step scores each charge inside its ball and visible from x with q_p G_B(x, z_p)
// (ball_greens / ball_greens_screened, point_visible) instead of sampling a point y and
// evaluating f(y); under delta tracking the sample still drives the collision, without
// it nothing is sampled. A query point on the Neumann polyline starts as a walk that has
// just hit it there (A.point_code). No walk pools (a parked walk holds no xcode). Kernels
// with PC == 0 compile none of this: their code is what it was.
#ifndef WOST_WAVENUMBERS
#define WOST_WAVENUMBERS 0
#endif
// WOST_FLAT_SIGMA_PRIME 1 (generated kernels whose sigma is the constant 0, option
// flat_sigma_prime): the Fields policy also provides alpha_jet(x, y, bool& flat), and the
// delta update skips sigma' where every colliding lane's weight is exactly 1
// (wost_device.h flat_alpha_min). The other kernels compile none of it.
#ifndef WOST_FLAT_SIGMA_PRIME
#define WOST_FLAT_SIGMA_PRIME 0
#endif
// WOST_DIRICHLET_TREE 1 (generated kernels of a handle whose Dirichlet distance goes through
// the Dirichlet polyline's segment tree, wost_set_dirichlet_tree): the Fields policy holds
// the kernel's arguments and its dirichlet_distance calls poly_distance_tree; walk_body
// stages no Dirichlet vertex. The other kernels compile none of it.
#ifndef WOST_DIRICHLET_TREE
#define WOST_DIRICHLET_TREE 0
#endif
// WOST_TALLY 1 (generated kernels of wost_solve_range_tally, KernelVariant::tally; one channel,
// no point charges, no recorder, no walk pools): the refill finds the walk's row of
// WalkArgs::tally, and the source sample of every step that is not clipped adds the deposit a
// source f == 1 would score there to the row's cell of the sample (tally_deposit). The walks,
// their values and steps are untouched. The other kernels compile none of it.
#ifndef WOST_TALLY
#define WOST_TALLY 0
#endif
// The first entry of walk wid's tally row, wid a walk of point pid: row (i / WOST_BLOCK_WALKS)
// mod replicas of the point, i the walk's index in the point (a function of the walk id
// alone). The buffer holds fewer than 2^27 entries (WOST_TALLY_MAX_BYTES) and i /
// WOST_BLOCK_WALKS is below 2^31 (walks_per_point < 2^43): 32 bits.
WOST_HD uint32_t tally_row_base(const WalkArgs& A, uint64_t wid, uint64_t pid) {
    const uint64_t i = wid - pid * (uint64_t)A.walks_per_point;
    const uint32_t row = (uint32_t)(i / (uint64_t)WOST_BLOCK_WALKS) % (uint32_t)A.tally_replicas;
    return ((uint32_t)pid * (uint32_t)A.tally_replicas + row) * (uint32_t)(A.tally_nx * A.tally_ny + 1);
}
// One deposit d at the sample (yx, yy) (tally_deposit; tally_add: at an entry already found):
// a no-return 64-bit integer add at device scope to the
// sample's bin of the row that starts at entry `base`, so that the sums do not depend on the
// order of arrival. A deposit that does not fit (tally_quantize) is not added and sets the
// flag word (q is 0 then): the host then fails the solve. The word keeps the largest E + 1
// seen, E the float32 exponent field of the scaled deposit (|d * scale| < 2^(E - 126); 255:
// infinite or NaN), so that the host can name a quantum under which every deposit fits.
__device__ __forceinline__ void tally_add(const WalkArgs& A, size_t entry, float d) {
    long long q;
    const bool bad = !tally_quantize(d, A.tally_scale, A.tally_limit, &q);
    if (WOST_ANY(bad)) {
        if (bad) atomicMax(A.tally_flag, ((__builtin_bit_cast(uint32_t, d * A.tally_scale) >> 23) & 0xffu) + 1u);
    }
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_add(A.tally + entry, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    A.tally[entry] += q;
#endif
}
__device__ __forceinline__ void tally_deposit(const WalkArgs& A, uint32_t base, float yx, float yy, float d) {
    const int cell = tally_cell(yx, yy, A.tally_x0, A.tally_y0, A.tally_dx, A.tally_dy, A.tally_inv_dx,
                                A.tally_inv_dy, A.tally_nx, A.tally_ny);
    tally_add(A, (size_t)base + (size_t)cell, d);
}
// WOST_TALLY_MAPS T (1..WOST_TALLY_MAX_MAPS; generated kernels of
// wost_solve_range_tally_channels, KernelVariant::tally_maps): the tally of a launch with NM *
// NK channels (one source, no point charges, no recorder, no walk pools). The refill finds the
// first of the walk's T sub-rows; a step that is not clipped forms, per map, the weighted
// combination of the deposits a source f == 1 would score on each channel (tally_weighted,
// WalkArgs::tally_weights) and adds it to the sample's bin of that map's sub-row: one cell
// computation, T quantisations, T adds. WOST_TALLY stays the one-channel tally; not both.
#ifndef WOST_TALLY_MAPS
#define WOST_TALLY_MAPS 0
#endif
// (row t of the weights, as scalar loads from constant memory)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) float* TallyWeightRow;
#else
typedef const float* TallyWeightRow;
#endif
template <int T, int C>
__device__ __forceinline__ void tally_deposit_maps(const WalkArgs& A, uint32_t base, float yx, float yy,
                                                   const float (&d)[C]) {
    const int cell = tally_cell(yx, yy, A.tally_x0, A.tally_y0, A.tally_dx, A.tally_dy, A.tally_inv_dx,
                                A.tally_inv_dy, A.tally_nx, A.tally_ny);
    const uint32_t bins = (uint32_t)(A.tally_nx * A.tally_ny + 1);
#pragma unroll
    for (int t = 0; t < T; ++t)
        tally_add(A, (size_t)(base + (uint32_t)t * bins) + (size_t)cell,
                  tally_weighted((TallyWeightRow)A.tally_weights + t * C, d, C));
}
// Walk pools (TREE kernels): see the exchange in walk_body. WOST_TREE_POOL 0 compiles
// them out; WOST_POOL_MIN_PUSH: fewest mismatched walks a wave parks at once.
#ifndef WOST_TREE_POOL
#define WOST_TREE_POOL 1
#endif
#ifndef WOST_POOL_MIN_PUSH
#define WOST_POOL_MIN_PUSH 1
#endif
// the lanes whose walk is inside the near box, as a wave mask (wost_device.h WaveMask)
__device__ __forceinline__ WaveMask pool_near_lanes(float4 b, float x, float y) {
    return wm_and(wm_and(wm_ge(x, b.x), wm_le(x, b.z)), wm_and(wm_ge(y, b.y), wm_le(y, b.w)));
}
// walks parked in class c (header word 1 + c), read with an atomic load so that every
// read goes to memory (under the lock: exact; outside it: a hint)
// A pool count as a wave-uniform value: the first active lane's load, broadcast. The
// callers branch on it around pool_lock/pool_unlock, which must run with the whole wave
// (lane 0 takes the lock for it), so no lane may see a different count.
__device__ __forceinline__ uint32_t pool_count(uint32_t* pool, int c) {
    return (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)__hip_atomic_load(pool + 1 + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
// the pool lock (header word 0), taken by the wave's first lane for the whole wave; the
// fences order the wave's slot reads and writes inside it
__device__ __forceinline__ void pool_lock(uint32_t* pool, int lane) {
    if (lane == 0) {
        while (__hip_atomic_exchange(pool, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0u)
            __builtin_amdgcn_s_sleep(1);
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ void pool_unlock(uint32_t* pool, int lane, uint32_t n_near, uint32_t n_far) {
    if (lane == 0) {
        __hip_atomic_store(pool + 1, n_near, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_store(pool + 2, n_far, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) __hip_atomic_store(pool, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Phase markers of the walk step for the offline ISA budget (tools/r05/phase_isa.py,
// WOST_PHASE_MARKS builds only): an assembly comment, which also bounds the instruction
// scheduler's regions, so the marked kernel is a study build, never the one that runs.
#if defined(WOST_PHASE_MARKS)
#define WOST_PHASE(name) asm volatile("; @phase " name)
#else
#define WOST_PHASE(name)
#endif

// Study builds (tools/r05/phase_dup.sh; WOST_EXP_FLAGS bits 2^18 and up, A/B only): a
// phase of the walk step computed a second time from opaque copies of its inputs and
// merged so that it cannot be removed yet changes no bit (x | (y & opaque 0)), so the
// walks are the same walks and the dynamic VALU counter grows by that phase's cost plus
// the merge's ~3 instructions. 1 Dirichlet distance, 2 Philox draw, 4 direction cos/sin,
// 8 Neumann ray query (scan kernels), 16 radial sampler, 32 screened G_norm, 64 alpha jet
// at the sample (NM > 1: model 0's), 128 alpha at the ray's point, 256 the source f, 512 sigma'.
#ifndef WOST_ABL_DUP
#define WOST_ABL_DUP 0
#endif
__device__ __forceinline__ float dup_opq(float v) {
    __asm__ volatile("" : "+v"(v));
    return v;
}
__device__ __forceinline__ uint32_t dup_zero() {
    uint32_t z = 0u;
    __asm__ volatile("" : "+v"(z));
    return z;
}
__device__ __forceinline__ float dup_merge(float a, float b) {   // a, depending on b
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, a) | (__builtin_bit_cast(uint32_t, b) & dup_zero()));
}

// The direction's cos and sin (wost_set_trig): correctly rounded (sincos_rn, the
// reference's values but for its own ulp errors; double-precision arithmetic) or the
// hardware's v_sin/v_cos (a few ulps, tens near the zeros). The field-specialised kernels
// fix the choice at compile time (WOST_JIT_TRIG_EXACT 1 / 0), the precompiled ones take
// it per launch (a uniform branch).
__device__ __forceinline__ void walk_sincos(float theta, float& sn, float& cs, bool exact) {
#if defined(WOST_JIT_TRIG_EXACT)
    exact = WOST_JIT_TRIG_EXACT != 0;
#endif
    if (exact) {
        sincos_rn(theta, sn, cs);
    } else {
        cs = f_cos(theta);
        sn = f_sin(theta);
    }
}

#ifndef WOST_REFILL_MIN   // idle lanes that trigger a refill (tools/ab_refill.sh; 1 = every iteration)
#define WOST_REFILL_MIN 4
#endif
// Philox one step ahead: step k's random words are drawn during step k - 1 (at the
// refill for step 0), right after that step's direction, where the ten dependent
// multiply rounds can overlap the step's geometry and field arithmetic instead of
// heading the next step's dependency chain. The words depend only on (seed, walk id,
// step), so the bits are unchanged.
// (1: where the compiler puts it -- it sinks the draw to the loop latch; 2: pinned
// right after the direction; 3: pinned before the source sample's clip test)
#ifndef WOST_PHILOX_AHEAD
#define WOST_PHILOX_AHEAD 0
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define WOST_PIN_U4(u) __asm__ volatile("" : "+v"((u).x), "+v"((u).y), "+v"((u).z), "+v"((u).w))
#else
#define WOST_PIN_U4(u) ((void)0)
#endif
template <bool NEU, bool SRC, bool DELTA, bool TREE, bool REC, int NS = 1, bool FIX = false, bool GL = false,
          int NK = 1, int PC = 0, int NM = 1, class F>
__device__ __forceinline__ void walk_body(const WalkArgs& A, const F& fld, unsigned char* smem) {
    // the walk's position updates round op by op like the reference (torch CPU
    // has no FMA contraction); the field math it calls keeps its own setting
#pragma clang fp contract(off)
    static_assert(NS >= 1 && (NS == 1 || SRC) && (NS == 1 || !REC), "multi-source walks need a source, no recorder");
    static_assert(NK >= 1 && (NK == 1 || (DELTA && !REC && WOST_WAVENUMBERS)) && NK * NS <= WOST_MAX_SOURCES,
                  "wavenumber channels need delta tracking, no recorder, at most WOST_MAX_SOURCES channels");
    static_assert(NM >= 1 && (NM == 1 || (DELTA && !REC && PC == 0)) && NM * NK * NS <= WOST_MAX_SOURCES,
                  "model channels need delta tracking, no recorder, no point charges, at most WOST_MAX_SOURCES channels");
    static_assert(PC >= 0 && PC <= WOST_MAX_POINT_CHARGES && (PC == 0 || (FIX && SRC && !REC)),
                  "point sources need compat=\"fixed\", a source mode, no recorder, at most WOST_MAX_POINT_CHARGES charges");
    static_assert(!WOST_TALLY || (SRC && NS == 1 && NK == 1 && NM == 1 && PC == 0 && !REC),
                  "a tally needs a source mode, one channel, no point charges, no recorder");
    static_assert(!WOST_TALLY_MAPS || (SRC && NS == 1 && PC == 0 && !REC && !WOST_TALLY && WOST_TALLY_MAPS >= 1 &&
                                       WOST_TALLY_MAPS <= WOST_TALLY_MAX_MAPS),
                  "channel maps need a source mode, one source, no point charges, no recorder, at most "
                  "WOST_TALLY_MAX_MAPS maps and no WOST_TALLY beside them");
    constexpr int NW = NM * NK;   // weights: wc = m * NK + j
    constexpr int NC = NW * NS;   // channels: c = (m * NK + j) * NS + s
    // (a Dirichlet-tree kernel reads the vertices it needs through global loads)
    constexpr bool kStageD = !F::kConstDirichlet && !GL && !WOST_DIRICHLET_TREE;
    // the Neumann polyline is staged also when compiled in (FIX scans sN itself; a few
    // hundred bytes otherwise)
    constexpr bool kStageN = NEU && !TREE && !GL;
    unsigned char* lds = smem;
    float4* sG = reinterpret_cast<float4*>(lds);                          // G_norm cells
    float* sT = reinterpret_cast<float*>(lds + (DELTA ? sizeof(float4) * (size_t)kGnormCells : 16));  // sampler tail
    lds += SRC ? align16((DELTA ? sizeof(float4) * (size_t)kGnormCells : 16) + sizeof(float) * kSamplerTailFloats) : 0;
    float2* sD = reinterpret_cast<float2*>(lds);
    lds += kStageD ? align16(sizeof(float2) * (size_t)A.nd) : 0;
    float2* sN = reinterpret_cast<float2*>(lds);
    lds += kStageN ? align16(sizeof(float2) * (size_t)A.nn) : 0;
    float* sPhi = reinterpret_cast<float*>(lds);
    lds += kStageN ? align16(sizeof(float) * (size_t)(A.nn > 1 ? A.nn - 1 : 0)) : 0;
    // the cooperative tree queries (the silhouette and the step's ray query; compat="fixed"
    // keeps the per-lane search for the source sample's visibility)
    constexpr bool kWaveTree = TREE;
    float4* const sRec = reinterpret_cast<float4*>(lds);   // staged tree records (TREE, tree_lds_records > 0)
    const int n_rec = TREE ? A.tree_lds_records : 0;
    lds += 8 * sizeof(float4) * (size_t)n_rec;
    float2* const sVert = reinterpret_cast<float2*>(lds);  // staged Neumann vertices (TREE, tree_lds_verts > 0)
    const int n_vert = TREE ? A.tree_lds_verts : 0;
    lds += align16(sizeof(float2) * (size_t)n_vert);
    TreeWaveScratch* const tws = reinterpret_cast<TreeWaveScratch*>(lds) + (threadIdx.x >> 6);
    for (int i = threadIdx.x; i < 8 * n_rec; i += blockDim.x) sRec[i] = A.tree[i];
    for (int i = threadIdx.x; i < n_vert; i += blockDim.x) sVert[i] = A.nverts[i];

    if (kStageD)
        for (int i = threadIdx.x; i < A.nd; i += blockDim.x) sD[i] = A.dverts[i];
    if (kStageN) {
        for (int i = threadIdx.x; i < A.nn; i += blockDim.x) sN[i] = A.nverts[i];
        for (int i = threadIdx.x; i < A.nn - 1; i += blockDim.x) sPhi[i] = A.seg_phi[i];
    }
    // the polylines the queries read: the LDS copies, or (GL) global memory
    const float2* const dP = (GL || WOST_DIRICHLET_TREE) ? A.dverts : sD;
    const float2* const nP = GL ? A.nverts : sN;
    const float* const phiP = GL ? A.seg_phi : sPhi;
    const SegTree tree{A.tree, A.nverts, A.nn, A.tree_first_leaf, A.tree_depth, A.tree_leaf, A.tree_tol, A.tree_kmax,
                       sRec, n_rec, sVert};
    float node0 = 0.0f;
    if (SRC) {
        node0 = A.table[0];
        for (int i = threadIdx.x; i < kSamplerTailFloats; i += blockDim.x) sT[i] = A.table[i + 1];
    }
    if (DELTA) {
        const float4* g = reinterpret_cast<const float4*>(A.table + kSamplerFloatsPadded);
        for (int i = threadIdx.x; i < kGnormCells; i += blockDim.x) sG[i] = g[i];
    }
    // this workgroup's walk pools (header: lock, walks parked near, walks parked far)
    // (a parked walk holds no tally row: tally kernels run without pools)
    uint32_t* const pool = (TREE && WOST_TREE_POOL && !WOST_TALLY && !WOST_TALLY_MAPS && NK == 1 && PC == 0 && NM == 1 && A.pool != nullptr)
                               ? A.pool + (size_t)blockIdx.x * (size_t)A.pool_wg_words : nullptr;
    if (pool != nullptr && threadIdx.x < 4) pool[threadIdx.x] = 0u;
    __syncthreads();

    const float sigma_bar = fld.sigma_bar();
    const float inv_sb = fld.inv_sigma_bar();
    const float sqrt_sb = fld.sqrt_sigma_bar();
    // sigma' shortcut of the sigma = 0 kernels (wost_device.h flat_alpha_min): the generator
    // defines WOST_FLAT_SIGMA_PRIME and gives alpha_jet the `flat` out-parameter
    constexpr bool kFlatSigmaPrime = WOST_FLAT_SIGMA_PRIME && DELTA && NM == 1 && NK == 1 && !WOST_WAVENUMBERS;
    const float flat_amin = kFlatSigmaPrime ? flat_alpha_min(inv_sb) : 0.0f;

    const int lane = threadIdx.x & 63;
    const uint64_t lanes_below = (1ull << lane) - 1ull;
#if defined(WOST_VOTE_STATS)   // study build: the wave votes' counters (wost_device.h WOST_VOTE)
    vote_begin();
#endif

    // wave-uniform work-queue state
    uint64_t c_next = 0, c_end = 0;
    bool exhausted = false;
    // the wave's own measurements (adaptive dequeues, launch statistics): its start and
    // last dequeue on the wall clock and its loop iterations (wave-uniform values kept in
    // VGPRs: the SGPR file is full, and a uniform scalar here would spill into VGPR lanes
    // through v_writelane / v_readlane inside the loop)
    constexpr bool kAdaptive = WOST_ADAPTIVE_DEQ && !TREE;
    constexpr bool kWaveStats = WOST_WAVE_STATS && !TREE;
    uint32_t q_t0 = (kAdaptive || kWaveStats) ? wall_ticks() : 0u;
    WOST_KEEP_VGPR(q_t0);
    uint32_t q_tdeq = q_t0;   // (WOST_WAVE_STATS)
    uint32_t q_iters = 0u;
    WOST_KEEP_VGPR(q_iters);
    uint32_t q_taken = 0u;   // walks this wave took from its static chunk and the queue (kAdaptive)
    WOST_KEEP_VGPR(q_taken);
    uint32_t my_kmax = 0u;   // the longest walk this lane finished (kWaveStats)
    {   // the wave's static first chunk (no atomic at the launch's start, when every wave
        // would hit the one counter at once)
        const uint64_t wv = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        const uint64_t cnt = (uint64_t)A.count;
        c_next = min(wv * (uint64_t)A.chunk0, cnt);
        c_end = min(c_next + (uint64_t)A.chunk0, cnt);
    }

    // the lanes that hold a walk, as a wave mask in scalar registers (wost_device.h
    // WaveMask): the votes below test it directly, a lane reads its own bit with wm_lane,
    // and it changes only where the whole wave is present (after the termination, at a
    // refill round, at a pool exchange), from the masks of the lanes that end or start there
    WaveMask live = wm_none();
    // per-lane walk state (solvers/WoStSolver.py:188-195)
    uint64_t wid = 0;           // global walk id: the Philox subsequence
    PhiloxWalk pw{0u, 0u, 0u, 0u};   // its per-walk Philox words (philox_walk)
    uint64_t lid = 0;           // local walk index: the output slot
    float px = 0.f, py = 0.f;
    float dD = 1.0f;            // dDirichlet seeded with 1.0 (:190, quirk Q12)
    int k = 0;                  // step_count
    bool onB = false;           // onBoundary
    float phi = 0.f;            // atan2 of currentNormal (:228), set when onB
    int xcode = 0;              // (PC > 0) boundary_code of the current point: its segment and inward side
#if WOST_TALLY || WOST_TALLY_MAPS
    uint32_t trow = 0u;         // first entry of this walk's tally row (tally_row_base; tally_maps_row)
#endif
    float ax[NM];               // alpha(current_point), cached (one per model)
#pragma unroll
    for (int m = 0; m < NM; ++m) ax[m] = 1.f;
    float w[NW];                // attenuation_coef (one per model and wavenumber)
#pragma unroll
    for (int j = 0; j < NW; ++j) w[j] = 1.f;
    U4 rn_ahead{0u, 0u, 0u, 0u};   // (WOST_PHILOX_AHEAD) the words of this walk's step k
    float total[NC];            // this walk's contributions (one per channel)
#pragma unroll
    for (int c = 0; c < NC; ++c) total[c] = 0.f;
#if defined(WOST_TREE_ITER_STATS)   // study build: the tree queries' loop counters (WOST_IC)
    uint32_t ic_arr[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) ic_arr[i] = 0u;
#define WOST_IC (TREE ? ic_arr : nullptr)
#else
#define WOST_IC nullptr
#endif

    // Tree kernels (long walks) also defer a finished walk's end record and output
    // into the refill batch: it idles until WOST_REFILL_MIN lanes are finished or
    // idle, or no lane is still stepping (C5 +4%; C3 and Laplace -2%, C4 neutral:
    // profiles/r02_ab/termination_batch.log). Its state does not change meanwhile,
    // so neither do its bits.
    constexpr bool kBatchEnd = TREE;
    for (;;) {
        // (the compiler carries the mask round this loop as a per-lane value, since the refill's
        // lane-dependent branches end where the loop's paths merge: read back as a scalar, what is
        // formed from it in this iteration stays in scalar registers)
        live = wm_scalar(live);
        const WaveMask done_m = wm_andn(live, wm_and(wm_lt_i(k, A.max_steps), wm_gt(dD, A.eps)));
        const bool done = wm_lane(done_m);
        bool batch = true;
        if (kBatchEnd)
            batch = __popcll(wm_ballot(wm_or(done_m, wm_not(live)))) >= WOST_REFILL_MIN || !wm_any(wm_andn(live, done_m));
        // --- walk termination: while-condition of :206, boundary term :295-298
        if (batch && done) {
            const float g0 = fld.has_g() ? fld.g(px, py) : 0.0f;
            float g = g0;
            if (DELTA) g = g0 * w[0];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const float gj = (DELTA && j > 0) ? g0 * w[j] : g;
#pragma unroll
                for (int s = 0; s < NS; ++s) total[j * NS + s] = total[j * NS + s] + gj;
            }
            const int64_t li = (int64_t)lid;
            if (REC && A.rec != nullptr) {
                float* rr = A.rec + ((size_t)li * (size_t)A.rec_stride + (size_t)k) * kRecFloats;
                rr[REC_X] = px; rr[REC_Y] = py; rr[REC_C] = g; rr[REC_AUX] = total[0];   // end record
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) A.out_val[li * NC + c] = total[c];
            A.out_steps[li] = (uint32_t)k;
            if (kWaveStats) my_kmax = (uint32_t)k > my_kmax ? (uint32_t)k : my_kmax;
        }
        if (batch) live = wm_andn(live, done_m);   // the finished lanes are idle

        // --- refill idle lanes from the wave's chunk (active-mask compaction), in
        // batches: the refill runs on the few lanes it starts while the wave's other
        // lanes wait, so finished lanes idle until WOST_REFILL_MIN of them (or all
        // the wave's live ones) can start together. Each walk's result depends only
        // on its id, so the batching changes no bits.
        // --- walk pools (TREE kernels): a wave pays its slowest lane's tree queries, and the
        // lanes whose walks are near the Neumann polyline are the slow ones (C5: ~5% of the
        // positions within 30 units of the topography cost ~5x the others). A wave whose
        // walks are mostly far parks its near walks in the workgroup's near pool, and one
        // whose walks are mostly near parks its far ones; freed lanes take parked walks of
        // the wave's own class first, then new walks from the queue. A walk's state moves
        // with it whole and its result depends only on its id: the bits do not change.
        if (pool != nullptr && batch) {
            const uint64_t act = wm_ballot(live);
            const uint64_t nm = wm_ballot(wm_and(live, pool_near_lanes(A.pool_box, px, py)));
            const int nact = __popcll(act), nnear = __popcll(nm);
            const uint32_t hn = pool_count(pool, 0), hf = pool_count(pool, 1);
            // (the wave's index as a scalar: the exchange below updates `live`, which must stay uniform)
            const int wave_in_group = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
            const int role = A.pool_near_waves > 0 ? (wave_in_group < A.pool_near_waves ? 0 : 1)
                             : nact > 0 ? (2 * nnear > nact ? 0 : 1) : (hn >= hf ? 0 : 1);
            uint64_t mis = role == 0 ? (act & ~nm) : nm;
            if (exhausted || __popcll(mis) < WOST_POOL_MIN_PUSH) mis = 0ull;
            if (mis != 0ull || (act != ~0ull && (role == 0 ? hn : hf) > 0u)) {
                pool_lock(pool, lane);
                uint32_t cnt[2] = {pool_count(pool, 0), pool_count(pool, 1)};
                const int cm = 1 - role;
                const uint32_t npush = min((uint32_t)__popcll(mis), (uint32_t)A.pool_slots - cnt[cm]);
                const uint32_t rk = (uint32_t)__popcll(mis & lanes_below);
                const WaveMask pushed = wm_and(mis, wm_lt_u(rk, npush));
                if (wm_lane(pushed)) {
                    uint32_t* const r = pool + 4 + (size_t)cm * pool_fields(NS) * A.pool_slots + cnt[cm] + rk;
                    const int P = A.pool_slots;
                    r[0 * P] = (uint32_t)wid; r[1 * P] = (uint32_t)(wid >> 32);
                    r[2 * P] = (uint32_t)lid; r[3 * P] = (uint32_t)(lid >> 32);
                    r[4 * P] = __builtin_bit_cast(uint32_t, px); r[5 * P] = __builtin_bit_cast(uint32_t, py);
                    r[6 * P] = __builtin_bit_cast(uint32_t, dD);
                    r[7 * P] = (uint32_t)k | (onB ? 0x80000000u : 0u);
                    r[8 * P] = __builtin_bit_cast(uint32_t, phi); r[9 * P] = __builtin_bit_cast(uint32_t, w[0]);
                    r[10 * P] = __builtin_bit_cast(uint32_t, ax[0]);
#pragma unroll
                    for (int s = 0; s < NS; ++s) r[(11 + s) * P] = __builtin_bit_cast(uint32_t, total[s]);
                }
                // (wm_scalar here and below: after a lane-dependent branch the compiler takes the
                // masks merged at its end for per-lane values)
                live = wm_scalar(wm_andn(live, pushed));
                cnt[cm] += npush;
                const uint64_t fr = wm_ballot(wm_not(live));
                const uint32_t npull = min((uint32_t)__popcll(fr), cnt[role]);
                const uint32_t rf = (uint32_t)__popcll(fr & lanes_below);
                const WaveMask pulled = wm_and(fr, wm_lt_u(rf, npull));
                if (wm_lane(pulled)) {
                    const uint32_t* const r =
                        pool + 4 + (size_t)role * pool_fields(NS) * A.pool_slots + (cnt[role] - npull) + rf;
                    const int P = A.pool_slots;
                    wid = (uint64_t)r[0 * P] | (uint64_t)r[1 * P] << 32;
                    lid = (uint64_t)r[2 * P] | (uint64_t)r[3 * P] << 32;
                    px = __builtin_bit_cast(float, r[4 * P]); py = __builtin_bit_cast(float, r[5 * P]);
                    dD = __builtin_bit_cast(float, r[6 * P]);
                    const uint32_t kb = r[7 * P];
                    k = (int)(kb & 0x7fffffffu); onB = (kb >> 31) != 0u;
                    phi = __builtin_bit_cast(float, r[8 * P]); w[0] = __builtin_bit_cast(float, r[9 * P]);
                    ax[0] = __builtin_bit_cast(float, r[10 * P]);
#pragma unroll
                    for (int s = 0; s < NS; ++s) total[s] = __builtin_bit_cast(float, r[(11 + s) * P]);
                    pw = philox_walk(wid, A.key0, A.key1);
                    if (WOST_PHILOX_AHEAD) rn_ahead = philox_draw(pw, (uint32_t)k, A.key0, A.key1);
                }
                live = wm_scalar(wm_or(live, pulled));
                cnt[role] -= npull;
                pool_unlock(pool, lane, cnt[0], cnt[1]);
            }
        }
        uint64_t need = batch ? wm_ballot(wm_not(live)) : 0ull;
        if (!kBatchEnd && __popcll(need) < WOST_REFILL_MIN && wm_any(live)) need = 0ull;
        while (need != 0ull && !exhausted) {
            if (c_next >= c_end) {
                if (A.queue_base >= A.count) {   // the static chunks covered every walk
                    exhausted = true;
                    break;
                }
                // the dequeue's size: the host's (WalkArgs::chunk), raised (adaptive) to
                // keep the grid below ~4e7 dequeues per second at the walk completion rate
                // seen so far (cheap short walks: a counter dequeue per 64 walks would set
                // the pace, 2.1e11 -> 7.0e10 walk-steps/s on Laplace), within chunk_share
                uint32_t chunk = (uint32_t)A.chunk;
                const uint32_t now = (kAdaptive || kWaveStats) ? wall_ticks() : 0u;
                if (kAdaptive && A.chunk_share > 0u) {
                    // the walks this wave completed: taken, less its lanes still walking
                    const float done = (float)(q_taken - (64u - (uint32_t)__popcll(need)));
                    // grid walks per second / 4e7 per second, at the 100 MHz wall clock
                    const float lo = fminf((float)A.chunk_share, ceilf(done * (float)A.waves * kDequeuesPerTickInv /
                                                                       ((float)(now - q_t0) + 1.0f)));
                    chunk = (uint32_t)__builtin_amdgcn_readfirstlane((int)fmaxf(lo, (float)chunk));
                }
                unsigned long long c = 0;
                if (lane == 0) c = atomicAdd(A.counter, (unsigned long long)chunk);
                c += (unsigned long long)A.queue_base;
                // lane 0's value as a scalar (every lane runs the refill): the queue
                // state stays in SGPRs and the refill loop's control flow uniform
                c = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(c >> 32)) << 32) |
                    (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)c);
                if (c >= (unsigned long long)A.count) {
                    exhausted = true;
                    break;
                }
                if (kWaveStats) {
                    q_tdeq = now;
                    WOST_KEEP_VGPR(q_tdeq);
                }
                c_next = c;
                c_end = c + (uint64_t)chunk;
                if (c_end > (uint64_t)A.count) c_end = (uint64_t)A.count;
            }
            const uint64_t avail = c_end - c_next;
            const uint32_t n = (uint32_t)__popcll(need);
            const uint32_t take = avail < (uint64_t)n ? (uint32_t)avail : n;
            const uint32_t rank = (uint32_t)__popcll(need & lanes_below);
            const WaveMask got = wm_and(need, wm_lt_u(rank, take));   // the lanes that start a walk
            if (wm_lane(got)) {
                lid = c_next + rank;
                uint64_t pid;
                WOST_WALK_OF_LOCAL(A, lid, wid, pid)
                pw = philox_walk(wid, A.key0, A.key1);
                if (WOST_PHILOX_AHEAD) rn_ahead = philox_draw(pw, 0u, A.key0, A.key1);
#if WOST_TALLY
                trow = tally_row_base(A, wid, pid);
#elif WOST_TALLY_MAPS
                trow = tally_maps_row(wid - pid * (uint64_t)A.walks_per_point, (uint32_t)pid, (uint32_t)A.tally_replicas,
                                      (uint32_t)WOST_TALLY_MAPS, (uint32_t)(A.tally_nx * A.tally_ny + 1));
#endif
                const float2 q = A.points[pid];
                px = q.x; py = q.y;
                k = 0; dD = FIX ? WOST_INF : 1.0f; onB = false; phi = 0.f;
                if constexpr (PC > 0 && NEU) {   // a query point on the Neumann polyline: as after a hit there
                    xcode = A.point_code[pid];
                    if (xcode != 0) {
                        const int sg = (xcode < 0 ? -xcode : xcode) - 1;
                        onB = true;
                        phi = TREE ? A.seg_phi[sg] : fld.neumann_phi(phiP, sg);
                        if (xcode < 0) phi = phi + kPiF;
                    }
                }
#pragma unroll
                for (int j = 0; j < NW; ++j) w[j] = 1.f;
#pragma unroll
                for (int c = 0; c < NC; ++c) total[c] = 0.f;
                if (DELTA) ax[0] = A.point_alpha[pid];             // alpha(x0), precomputed per point
                if constexpr (NM > 1) {                            // ... and per model: [NM][n_points]
#pragma unroll
                    for (int m = 1; m < NM; ++m) ax[m] = A.point_alpha[(size_t)m * (size_t)A.n_points + pid];
                }
            }
            live = wm_or(live, got);
            c_next += take;
            if (kAdaptive) {
                q_taken += take;
                WOST_KEEP_VGPR(q_taken);
            }
            need = wm_ballot(wm_andn(need, got));   // (need was every idle lane: the loop runs only then)
        }
        // the queue is exhausted: idle lanes take parked walks of either class, and the
        // wave ends only when both pools are empty (a wave parks walks only while the
        // queue is not exhausted for it, and drains the pools itself before it ends)
        if (pool != nullptr && exhausted && batch && wm_any(wm_not(live)) &&
            (!wm_any(live) || pool_count(pool, 0) + pool_count(pool, 1) > 0u)) {
            pool_lock(pool, lane);
            uint32_t cnt[2] = {pool_count(pool, 0), pool_count(pool, 1)};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint64_t fr = wm_ballot(wm_not(live));
                const uint32_t npull = min((uint32_t)__popcll(fr), cnt[c]);
                const uint32_t rf = (uint32_t)__popcll(fr & lanes_below);
                const WaveMask pulled = wm_and(fr, wm_lt_u(rf, npull));
                if (wm_lane(pulled)) {
                    const uint32_t* const r =
                        pool + 4 + (size_t)c * pool_fields(NS) * A.pool_slots + (cnt[c] - npull) + rf;
                    const int P = A.pool_slots;
                    wid = (uint64_t)r[0 * P] | (uint64_t)r[1 * P] << 32;
                    lid = (uint64_t)r[2 * P] | (uint64_t)r[3 * P] << 32;
                    px = __builtin_bit_cast(float, r[4 * P]); py = __builtin_bit_cast(float, r[5 * P]);
                    dD = __builtin_bit_cast(float, r[6 * P]);
                    const uint32_t kb = r[7 * P];
                    k = (int)(kb & 0x7fffffffu); onB = (kb >> 31) != 0u;
                    phi = __builtin_bit_cast(float, r[8 * P]); w[0] = __builtin_bit_cast(float, r[9 * P]);
                    ax[0] = __builtin_bit_cast(float, r[10 * P]);
#pragma unroll
                    for (int s = 0; s < NS; ++s) total[s] = __builtin_bit_cast(float, r[(11 + s) * P]);
                    pw = philox_walk(wid, A.key0, A.key1);
                    if (WOST_PHILOX_AHEAD) rn_ahead = philox_draw(pw, (uint32_t)k, A.key0, A.key1);
                }
                live = wm_scalar(wm_or(live, pulled));
                cnt[c] -= npull;
            }
            pool_unlock(pool, lane, cnt[0], cnt[1]);
        }
        if (!wm_any(live)) break;
        if (kWaveStats) {
            q_iters += 1u;
            WOST_KEEP_VGPR(q_iters);
        }
        // a freshly refilled walk may already fail the while-condition (eps >= 1,
        // maxSteps == 0): it takes no step and is finished at the next iteration
        bool stepping;
        // the cooperative tree queries need every lane of the wave: the others run the
        // step's pure arithmetic up to the ray query with them and leave after it
        if constexpr (kWaveTree) {
            const WaveMask step_m = wm_and(live, wm_and(wm_lt_i(k, A.max_steps), wm_gt(dD, A.eps)));
            stepping = wm_lane(step_m);
            if (!wm_any(step_m)) continue;
        } else {
            stepping = wm_lane(live) && (k < A.max_steps) && (dD > A.eps);
            if (!stepping) continue;
        }

        // --- one walk-step (:206-291)
#if defined(WOST_TREE_ITER_STATS)
        ic_arr[14] += 1u;
#endif
        WOST_VOTE(0, stepping);
        WOST_PHASE("dirichlet_distance");
        float dd = fld.dirichlet_distance(dP, A.nd, px, py);        // :208
        if (WOST_ABL_DUP & 1) dd = dup_merge(dd, fld.dirichlet_distance(dP, A.nd, dup_opq(px), py));
        if (FIX && stepping && !(dd > A.eps)) {   // Q7/Q12 fixed: stop here, g at this point
            dD = dd;
            if (!kWaveTree) continue;
            stepping = false;   // (it only helps the wave's tree queries)
        }
        // the step's random words and direction (:226-232)
        U4 rn;
        float cs = 0.f, sn = 0.f;
        bool onB0 = false;                                           // the current point's, for FIX's
        float phi0 = 0.f;                                            // source direction
        auto draw_direction = [&]() {
#if defined(WOST_ABL_NO_PHILOX)   // ablation (timing only): a cheap hash
            const uint32_t hh = (pw.b ^ (uint32_t)k * 0x9E3779B9u) * 0x85EBCA6Bu;
            rn = U4{hh, hh * 0xC2B2AE35u, (hh ^ pw.d) * 0x27D4EB2Fu, hh ^ pw.c};
#else
            // the key enters each step opaque, so its round schedule (key + r * W) is
            // formed by scalar adds here instead of 16 loop-invariant SGPRs, which the
            // register allocator would otherwise spill to VGPR lanes (a v_readlane each)
            if (WOST_PHILOX_AHEAD) {
                rn = rn_ahead;                                       // drawn during the previous step
            } else {
                uint32_t key0 = A.key0, key1 = A.key1;
                WOST_OPAQUE_SGPR(key0);
                WOST_OPAQUE_SGPR(key1);
                rn = philox_draw(pw, (uint32_t)k, key0, key1);       // philox4x32_10({k, 0, wid})
                if (WOST_ABL_DUP & 2) {
                    const U4 r2 = philox_draw(pw, (uint32_t)k | dup_zero(), key0, key1);
                    rn.x |= (r2.x ^ r2.y ^ r2.z ^ r2.w) & dup_zero();
                }
            }
#endif
            float theta = (u01(rn.x) * 2.0f) * kPiF;                 // :226
            // :227-228 (quirk Q2): atan2(normal) is a property of the segment that
            // was hit, precomputed per segment on the host (the C library's atan2f)
            if (NEU && onB) theta = FIX ? theta / 2.0f + (phi - kPiF / 2.0f) : theta / 2.0f + phi;
            onB0 = onB;
            phi0 = phi;
            walk_sincos(theta, sn, cs, A.exact_trig != 0);           // :230-232
            if (WOST_ABL_DUP & 4) {
                float s2, c2;
                walk_sincos(dup_opq(theta), s2, c2, A.exact_trig != 0);
                sn = dup_merge(sn, s2);
                cs = dup_merge(cs, c2);
            }
        };
        float r;
        float dnv = WOST_NAN;                                        // recorder: None without Neumann
        // a long polyline's brute-force scans in one pass (neumann_scan_both): the direction
        // first, the ray query's finish after r
#if defined(WOST_ABL_NO_SILHOUETTE)   // (the ablation skips the fused scan, which draws the direction)
        constexpr bool kFused = false;
#else
        constexpr bool kFused = NEU && !TREE && !FIX && F::kFusedNeumann;
#endif
        ScanBoth sb{};
        WOST_PHASE("silhouette");
        if (NEU) {
#if defined(WOST_ABL_NO_SILHOUETTE)   // ablation (timing only)
            const float dn = WOST_INF;
#else
            float dn;
            if constexpr (kFused) {
                draw_direction();
                sb = fld.neumann_scan_both(nP, A.nn, px, py, cs, sn);
                dn = scan_both_silhouette(sb);                        // :211
            } else {
                dn = kWaveTree ? silhouette_distance_tree_wave(tree, px, py, dd, A.tree_stop2, stepping, tws, lane,
                                                               WOST_IC)
                     : TREE    ? silhouette_distance_tree(tree, px, py, dd, A.tree_stop2)
                               : fld.neumann_silhouette_distance(nP, A.nn, px, py);  // :211
            }
#endif
            dnv = dn;
            const float m = dn < dd ? dn : dd;                       // Python min()
            r = m > A.rmin ? m : A.rmin;                             // Python max() (:212)
        } else {
            r = dd > A.rmin ? dd : A.rmin;                           // :215
        }
        if constexpr (PC > 0 && NEU) {   // a walker on a Neumann segment: its half-ball ends at a re-entrant corner
            if (onB) {
                const float rc = boundary_corner_radius(TREE ? A.nverts : nP, A.nn, px, py, xcode, r);
                r = rc > A.rmin ? rc : A.rmin;
            }
        }
        WOST_PHASE("philox_direction");
        if (!kFused) draw_direction();
#if !defined(WOST_ABL_NO_PHILOX)
        if (WOST_PHILOX_AHEAD) {   // the next step's words, overlapping this step's arithmetic
            uint32_t key0 = A.key0, key1 = A.key1;
            WOST_OPAQUE_SGPR(key0);
            WOST_OPAQUE_SGPR(key1);
            rn_ahead = philox_draw(pw, (uint32_t)(k + 1), key0, key1);
            if (WOST_PHILOX_AHEAD == 2) WOST_PIN_U4(rn_ahead);
        }
#endif

        float xnx, xny;
        const int xcode0 = xcode;                                    // the current point's, like onB0
        WOST_PHASE("ray_query");
        if (NEU) {                                                   // :235-236
#if defined(WOST_ABL_NO_RAY)
            Hit h; h.x = px + r * cs; h.y = py + r * sn; h.hit = false; h.seg = -1;
#else
            Hit h = kFused    ? scan_both_finish(nP, sb, px, py, r)
                    : kWaveTree ? intersect_polylines_tree_wave<false, FIX>(tree, px, py, cs, sn, r, stepping, tws,
                                                                            lane, WOST_IC)
                    : FIX       ? fld.neumann_intersect_nearest(nP, A.nn, px, py, cs, sn, r)
                                : fld.neumann_intersect(nP, A.nn, px, py, cs, sn, r);
            if ((WOST_ABL_DUP & 8) && !kWaveTree && !FIX && !kFused) {
                const Hit h2 = fld.neumann_intersect(nP, A.nn, dup_opq(px), py, cs, sn, r);
                h.x = dup_merge(h.x, h2.x);
                h.y = dup_merge(h.y, h2.y);
                h.seg |= h2.seg & (int)dup_zero();
                h.hit = h.hit || (h2.hit && dup_zero() != 0u);
            }
#endif
            if (kWaveTree && !stepping) continue;   // the lanes that only helped
            xnx = h.x; xny = h.y; onB = h.hit;
            if (h.hit) phi = TREE ? A.seg_phi[h.seg] : fld.neumann_phi(phiP, h.seg);
            if (FIX && h.hit) {
                // inward normal: the left normal when the ray crossed the segment from
                // its left side, i.e. cross(d, u) > 0 (then dot(left normal, d) < 0)
                const float2* const sv = TREE ? A.nverts : nP;   // the tree kernels stage none
                const float2 a = sv[h.seg], b = sv[h.seg + 1];
                const bool right_inward = !(cs * (b.y - a.y) - sn * (b.x - a.x) > 0.0f);
                if (right_inward) phi = phi + kPiF;
                if constexpr (PC > 0) xcode = boundary_code(h.seg, right_inward);
            } else if constexpr (PC > 0) {
                xcode = 0;
            }
        } else {                                                     // :238-239
            xnx = px + r * cs;
            xny = py + r * sn;
        }

        float yx = xnx, yy = xny;
        float cv = 0.0f;                                             // recorder: source contribution
        bool clipped = false;
        float gnorm = 0.f;
        Jet aj{0.f, 0.f, 0.f, 0.f};
        Jet ajm[NM];                                                 // (NM > 1) every model's jet at y; ajm[0] = aj
        bool aj_flat = false;                                        // (kFlatSigmaPrime) aj is {v, 0, 0, 0}
        WOST_PHASE("sample_and_clip");
        if (SRC) {                                                   // :242-258
            float rs;
            if constexpr (FIX && DELTA)                              // Q4/Q5 fixed: this ball's law
                rs = sample_rho_screened_fixed(A.table + kFixTableOffset, u01(rn.y), r * sqrt_sb) * r;
            else if constexpr (PC == 0)                              // (point sources: nothing is sampled)
                rs = sample_rho_tail(sT, node0, u01(rn.y)) * r;      // :244 (sampler, quirks Q3-Q5)
            if (WOST_ABL_DUP & 16) rs = dup_merge(rs, sample_rho_tail(sT, node0, u01(rn.y | dup_zero())) * r);
            if constexpr (FIX && !DELTA && PC > 0) {
                // point sources without delta tracking: the charges are scored below, exactly;
                // no source sample, no direction of its own, no visibility query for it
            } else if constexpr (FIX && !DELTA) {                    // Q13 fixed: own direction
                float ts = (u01(rn.w) * 2.0f) * kPiF;
                if (NEU && onB0) ts = ts / 2.0f + (phi0 - kPiF / 2.0f);   // the inward hemisphere
                float cs2, sn2;
                walk_sincos(ts, sn2, cs2, A.exact_trig != 0);
                yx = px + rs * cs2;
                yy = py + rs * sn2;
                if (NEU)   // not visible
                    clipped = TREE ? intersect_polylines_tree<false, true>(tree, px, py, cs2, sn2, rs).hit
                                   : fld.neumann_intersect_nearest(nP, A.nn, px, py, cs2, sn2, rs).hit;
            } else {
                // :245 (quirk Q13). FIX delta keeps the sample on the step's ray: with the
                // nearest crossing (Q1) the clip below is exactly "y is in the star-shaped
                // region", and a collision is taken only there, so it lands at a radius
                // drawn from the Green's law truncated at the ray's boundary point
                yx = px + rs * cs;
                yy = py + rs * sn;
                const float e1x = yx - px, e1y = yy - py;
                const float e2x = xnx - px, e2y = xny - py;
                // :248 compares the two norms. a2 > b2 is not rare: a Neumann "hit" is any
                // ray whose line crosses a segment (Q1), its point within ~1 of x while the
                // sample radius is of order r, so a2 > b2 on 13.9% of C4's lane-steps (2.1%
                // of C3's) and some lane of nearly every wave-step has it. The ratio decides
                // all of them without a square root; only the ~2^-19 wide band above b2
                // (no lane-step of either sample) evaluates the reference's comparison.
                const float a2 = e1x * e1x + e1y * e1y, b2 = e2x * e2x + e2y * e2y;
                if (WOST_PHILOX_AHEAD == 3) WOST_PIN_U4(rn_ahead);
                clipped = norm_greater(a2, b2);
                if (clipped) { yx = xnx; yy = xny; }
            }
            if (DELTA) {
                WOST_PHASE("greens_norm");
                gnorm = greens_norm_from_table(sG, r * sqrt_sb, r, inv_sb);   // solvers/utils.py:29-44
                if (WOST_ABL_DUP & 32) gnorm = dup_merge(gnorm, greens_norm_from_table(sG, dup_opq(r) * sqrt_sb, r, inv_sb));
                WOST_PHASE("alpha_jet");
                if constexpr (NM > 1) {
                    fld.alpha_jet_multi(yx, yy, ajm);
                    aj = ajm[0];
                } else if constexpr (kFlatSigmaPrime) {
                    aj = fld.alpha_jet(yx, yy, aj_flat);
                } else {
                    aj = fld.alpha_jet(yx, yy);
                }
                if (WOST_ABL_DUP & 64) {
                    const Jet a2 = fld.alpha_jet(dup_opq(yx), yy);
                    aj.v = dup_merge(aj.v, a2.v);
                    aj.gx = dup_merge(aj.gx, a2.gx);
                    aj.gy = dup_merge(aj.gy, a2.gy);
                    aj.lap = dup_merge(aj.lap, a2.lap);
                    if constexpr (NM > 1) ajm[0] = aj;   // (the score and sigma' read model 0's jet from ajm)
                }
            }
            WOST_PHASE("source_contribution");
            if constexpr (PC > 0) {
                // Point sources: every charge inside the step's ball and visible from x scores
                // q G_B(x, z), the sampled estimator's f G_norm with the sample integrated out
                // (under delta tracking its rsq(alpha(y) alpha(x)) at y = z). On a Neumann
                // boundary point the star-shaped region is a half-ball, whose Green's function
                // at a boundary pole is twice the ball's: the factor 2 of the sampled estimator.
                // The in-ball test is per lane; visibility and the Bessel evaluation run only
                // when a lane of the wave needs them. The per-source sums are formed first, in
                // charge order, so that a source's value does not depend on the other sources.
                float cq[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) cq[s] = 0.0f;
                const float r2 = r * r;
                auto nearest = [&](float ox, float oy, float ex, float ey, float len) {
                    if constexpr (TREE) return intersect_polylines_tree<false, true>(tree, ox, oy, ex, ey, len);
                    else return fld.neumann_intersect_nearest(nP, A.nn, ox, oy, ex, ey, len);
                };
#pragma unroll 1
                for (int p = 0; p < PC; ++p) {
                    const float zx = charge_float(A.charges, CHG_XY + 2 * p);
                    const float zy = charge_float(A.charges, CHG_XY + 2 * p + 1);
                    const float ex = zx - px, ey = zy - py;
                    const float d2 = ex * ex + ey * ey;
                    // (delta tracking: beyond t = r_p sqrt(sigma_bar) = 88 the function is below
                    // float32's smallest normal, exp(-88) = 6e-39: such a charge scores nothing)
                    const bool in = d2 < r2 && (!DELTA || d2 * sigma_bar < 7744.0f);
                    if (WOST_ANY(in)) {
                        WOST_NO_SPECULATION();
                        if (in) {
                            bool vis = true;
                            if constexpr (NEU)
                                vis = point_visible(TREE ? A.nverts : nP, px, py, xcode0, zx, zy,
                                                    charge_int(A.charges, CHG_SEG0 + p),
                                                    charge_int(A.charges, CHG_SEG1 + p), nearest);
                            if (vis) {
                                // r_p clamped at rmin: the potential of an electrode of radius eps / 2
                                // (a query point that is itself a charge stays finite)
                                float rp = f_sqrt(d2);
                                rp = rp > A.rmin ? rp : A.rmin;
                                const float q = charge_float(A.charges, CHG_Q + p);
                                float v;
                                if constexpr (DELTA)
                                    v = (q * ball_greens_screened(rp, r, sqrt_sb)) *
                                        f_rsq(charge_float(A.charges, CHG_ALPHA + p) * ax[0]);
                                else
                                    v = q * ball_greens(rp, r);
                                const int sp = charge_int(A.charges, CHG_SOURCE + p);
#pragma unroll
                                for (int s = 0; s < NS; ++s) cq[s] = sp == s ? cq[s] + v : cq[s];
                            }
                        }
                    }
                }
                const float bf = (NEU && onB0) ? 2.0f : 1.0f;
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const float c = cq[s] * bf;
#pragma unroll
                    for (int j = 0; j < NK; ++j) total[j * NS + s] = total[j * NS + s] + (DELTA ? c * w[j] : c);
                }
            } else if constexpr (NC == 1) {
                float c = 0.0f;
                if (!clipped) {
                    float f = fld.f(yx, yy);
                    if (WOST_ABL_DUP & 256) f = dup_merge(f, fld.f(dup_opq(yx), yy));
                    if (DELTA)
                        c = (f * gnorm) * f_rsq(aj.v * ax[0]) * w[0];  // :253-254
                    else
                        c = f * ((r * r) / 4.0f);                        // :256, utils.py:61
#if WOST_TALLY   // what f == 1.0f scores here: (1.0f * gnorm) is gnorm, 1.0f * (r * r / 4) is r * r / 4
                    tally_deposit(A, trow, yx, yy, DELTA ? (gnorm * f_rsq(aj.v * ax[0])) * w[0] : (r * r) / 4.0f);
#elif WOST_TALLY_MAPS   // one channel (one wavenumber, no models): the same deposit, T weights of it
                    const float td[1] = {DELTA ? (gnorm * f_rsq(aj.v * ax[0])) * w[0] : (r * r) / 4.0f};
                    tally_deposit_maps<WOST_TALLY_MAPS, 1>(A, trow, yx, yy, td);
#endif
                }
                total[0] = total[0] + c;                                 // :258
                cv = c;
            } else if (!clipped) {                                       // the same per channel
                float fv[NS];
                if constexpr (NS == 1) fv[0] = fld.f(yx, yy);
                else fld.f_multi(yx, yy, fv);
                const float q = DELTA ? 0.0f : ((r * r) / 4.0f);
#if WOST_TALLY_MAPS   // what f == 1.0f scores on channel m * NK + j: (1.0f * gnorm) is gnorm
                float td[NW];
#endif
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    const float sa = DELTA ? f_rsq((NM > 1 ? ajm[m].v : aj.v) * ax[m]) : 0.0f;
#if WOST_TALLY_MAPS
#pragma unroll
                    for (int j = 0; j < NK; ++j) td[m * NK + j] = DELTA ? (gnorm * sa) * w[m * NK + j] : q;
#endif
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const float fg = DELTA ? ((fv[s] * gnorm) * sa) : fv[s] * q;
#pragma unroll
                        for (int j = 0; j < NK; ++j) {
                            const float c = DELTA ? fg * w[m * NK + j] : fg;
                            total[(m * NK + j) * NS + s] = total[(m * NK + j) * NS + s] + c;
                        }
                    }
                }
#if WOST_TALLY_MAPS
                tally_deposit_maps<WOST_TALLY_MAPS, NW>(A, trow, yx, yy, td);
#endif
            } else {
#pragma unroll
                for (int c = 0; c < NC; ++c) total[c] = total[c] + 0.0f;
            }
        }
        if (REC && A.rec != nullptr) {                               // :218-222, :261-266
            // the tree's silhouette distance is exact only below dD: recompute it
            if (TREE) dnv = silhouette_distance_tree(tree, px, py, WOST_INF);
            const int64_t li = (int64_t)lid;
            float4* rr = reinterpret_cast<float4*>(A.rec + ((size_t)li * (size_t)A.rec_stride + (size_t)k) * kRecFloats);
            rr[0] = float4{px, py, dd, dnv};
            rr[1] = float4{yx, yy, cv, SRC ? 1.0f : 0.0f};
        }

        WOST_PHASE("delta_update");
        if (DELTA && FIX) {
            const float mu = u01(rn.z);
            // collision: mu <= sigma_bar |G| and the sample before the ray's boundary point
            const bool collide = !(mu > sigma_bar * gnorm) && !clipped;
            float anew[NM];                                          // a collision, or a clipped sample (y = z)
            anew[0] = aj.v;
            if constexpr (NM > 1) {
#pragma unroll
                for (int m = 1; m < NM; ++m) anew[m] = ajm[m].v;
            }
            if (!collide && !clipped) {
                if constexpr (NM > 1) fld.alpha_multi(xnx, xny, anew);
                else anew[0] = fld.alpha(xnx, xny);
            }
            float sc[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) sc[j] = 1.0f;
            // sigma = 0 kernels: a colliding lane whose jet is flat and whose alpha clears the
            // bound has sc == 1.0f exactly (flat_alpha_min); the wave runs sigma' only when
            // some colliding lane is not such a lane, and then for all of them as ever
            bool sp_wave = true;
            if constexpr (kFlatSigmaPrime) {
                const bool full = collide && !flat_sigma_trivial(aj_flat, aj.v, flat_amin);
                WOST_VOTE(13, full);
                sp_wave = WOST_ANY(full);
            }
            if (sp_wave && collide) {
                if constexpr (kFlatSigmaPrime) WOST_NO_SPECULATION();
                float spv[NM];
                if constexpr (NM > 1) {
                    float sg[NM];
                    fld.sigma_multi(yx, yy, sg);
#pragma unroll
                    for (int m = 0; m < NM; ++m) spv[m] = sigma_prime_from(ajm[m], sg[m], fld.detached_multi(m));
                } else {
                    spv[0] = sigma_prime_from(aj, fld.sigma(yx, yy), fld.detached());
                }
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int j = 0; j < NK; ++j) {
                        if constexpr (WOST_WAVENUMBERS) sc[m * NK + j] = 1.0f - (spv[m] + A.k2[j]) * inv_sb;   // kept signed
                        else sc[m * NK + j] = 1.0f - spv[m] * inv_sb;
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const float wr = f_sqrt(f_div(anew[m], ax[m]));      // shared by the wavenumbers
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    const float wt = w[m * NK + j] * wr;
                    w[m * NK + j] = collide ? wt * sc[m * NK + j] : wt;
                }
                ax[m] = anew[m];
            }
            px = collide ? yx : xnx;
            py = collide ? yy : xny;
            onB = collide ? false : onB;                             // a collision point is interior
            if constexpr (PC > 0) xcode = collide ? 0 : xcode;
        } else if (DELTA) {                                          // :271-284
            const float mu = u01(rn.z);
            const bool accept = mu > sigma_bar * gnorm;              // :273-275
            // the two branches share the weight update w * sqrt(a_new / alpha(x));
            // only the field evaluations stay divergent
            float anew[NM];                                          // collision, or a clipped accept
            anew[0] = aj.v;
            if constexpr (NM > 1) {
#pragma unroll
                for (int m = 1; m < NM; ++m) anew[m] = ajm[m].v;
            }
#if !defined(WOST_ABL_NO_ALPHA_Z)
            if (accept && !clipped) {
                if constexpr (NM > 1) {
                    fld.alpha_multi(xnx, xny, anew);
                } else {
                    anew[0] = fld.alpha(xnx, xny);                   // :277
                    if (WOST_ABL_DUP & 128) anew[0] = dup_merge(anew[0], fld.alpha(dup_opq(xnx), xny));
                }
            }
#endif
            float sc[NW];
#pragma unroll
            for (int j = 0; j < NW; ++j) sc[j] = 1.0f;
            bool sp_wave = true;                                     // (see the FIX branch above)
            if constexpr (kFlatSigmaPrime) {
                const WaveMask full =
                    wm_andn(wm_not(wm_gt(mu, sigma_bar * gnorm)), flat_sigma_trivial_lanes(aj_flat, aj.v, flat_amin));
                WOST_VOTE(13, wm_lane(full));
                sp_wave = wm_any(full);
            }
#if defined(WOST_ABL_NO_SIGMA_PRIME)
            if (false) {
#else
            if (sp_wave && !accept) {
#endif
                if constexpr (kFlatSigmaPrime) WOST_NO_SPECULATION();
                float spv[NM];
                if constexpr (NM > 1) {
                    float sg[NM];
                    fld.sigma_multi(yx, yy, sg);
#pragma unroll
                    for (int m = 0; m < NM; ++m) spv[m] = sigma_prime_from(ajm[m], sg[m], fld.detached_multi(m));
                } else {
                    spv[0] = sigma_prime_from(aj, fld.sigma(yx, yy), fld.detached());  // :281
                    if (WOST_ABL_DUP & 512)
                        spv[0] = dup_merge(spv[0], sigma_prime_from(Jet{dup_opq(aj.v), aj.gx, aj.gy, aj.lap},
                                                                    fld.sigma(dup_opq(yx), yy), fld.detached()));
                }
#pragma unroll
                for (int m = 0; m < NM; ++m) {
#pragma unroll
                    for (int j = 0; j < NK; ++j) {
                        float scj;
                        if constexpr (WOST_WAVENUMBERS) scj = 1.0f - (spv[m] + A.k2[j]) * inv_sb;
                        else scj = 1.0f - spv[m] * inv_sb;
                        sc[m * NK + j] = (0.0f > scj) ? 0.0f : scj;  // Python max(., 0.0) (:282)
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const float wr = f_sqrt(f_div(anew[m], ax[m]));      // :277 / :283, shared by the wavenumbers
#pragma unroll
                for (int j = 0; j < NK; ++j) {
                    const float wt = w[m * NK + j] * wr;
                    w[m * NK + j] = accept ? wt : wt * sc[m * NK + j];
                }
                ax[m] = anew[m];
            }
            px = accept ? xnx : yx;
            py = accept ? xny : yy;
        } else {
            px = xnx; py = xny;                                      // :287
        }
        k += 1;                                                      // :291
        dD = dd;   // the loop tests the distance of the pre-step point (quirk Q7)
        WOST_PHASE("loop_head");
    }
#if defined(WOST_VOTE_STATS)
    vote_end();   // (every lane is here)
#endif
    if (kWaveStats) {   // the wave's longest walk (every lane is here)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)my_kmax, o);
            my_kmax = other > my_kmax ? other : my_kmax;
        }
    }
    if (kWaveStats && lane == 0) {   // the launch statistics (wost_block_reduce sums them up)
        uint4* const wave_stats = reinterpret_cast<uint4*>(A.counter + kCtlWords);
        const uint64_t wv = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        const uint64_t end = wall_ticks64();
        const uint32_t dur = (uint32_t)end - q_t0;
        const uint64_t start = end - dur;                   // the start's high word, from the end's
        wave_stats[2 * wv] = uint4{(uint32_t)start, (uint32_t)(start >> 32), q_tdeq - q_t0, dur};
        wave_stats[2 * wv + 1] = uint4{q_iters, my_kmax, 0u, 0u};
    }
#if defined(WOST_TREE_ITER_STATS)
    // each lane's counters into the workgroup's study words after its pools (the host
    // sizes A.pool for them when WOST_TREE_ITER_STATS is set)
    if (pool != nullptr) {
        uint32_t* const st = pool + 4 + 2 * (size_t)pool_fields(NS) * A.pool_slots;
#pragma unroll
        for (int i = 0; i < 16; ++i) atomicAdd(st + i, ic_arr[i]);
    }
#endif
#undef WOST_IC
}

}  // namespace wost
