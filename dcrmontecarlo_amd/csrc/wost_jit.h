// wost_jit.h -- field-specialised walk kernels compiled at run time (hiprtc).
//
// The precompiled walk kernel interprets each handle's coefficient fields
// from a program buffer (a term/factor loop with a kind switch per factor).
// For a given handle and kernel variant, libwost instead generates HIP source
// in which the fields are straight-line calls to the same per-kind functions
// (wost_device.h) with their parameters as literals, compiles it for the
// device's gfx target with hiprtc, caches the code object (in memory and on
// disk) and launches it with the same WalkArgs. Results are identical to the
// interpreted kernel; the interpretation overhead disappears.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "wost_device.h"
#include "wost_options.h"
#include "wost_variant.h"

namespace wost {

// Which polylines a specialised kernel with traits `t` compiles in (at most
// Options::const_vertices vertices, default kJitMaxConstVertices; a compiled-in
// Dirichlet polyline is not staged in LDS).
bool jit_const_dirichlet(const Options& o, int nd);
bool jit_const_neumann(const Options& o, const WalkTraits& t, int nn);
// a long Neumann polyline scanned without the segment tree (the brute-force kernel, reference
// mode): both queries of a step in one pass (wost_device.h neumann_scan_both)
bool jit_fused_neumann_scan(const Options& o, const WalkTraits& t, int nn);

// The fields a kernel compiles in: the program's header, terms and factors.
// models: the (sigma, alpha) field pairs of models 1.. of a model-batched kernel (variant
// n_models >= 2; model 0 is the header's SLOT_SIGMA / SLOT_ALPHA): 2 * (n_models - 1)
// descriptors into the same terms and factors, in slots after the extra sources. Only
// generated code reads them, so they stay on the host: the header the device reads is
// unchanged. Null otherwise.
struct ProgramView {
    const DProgram* hdr;
    const DTerm* terms;
    const DFactor* factors;
    const DField* models = nullptr;
};
// The polylines (Dirichlet dverts[2*nd], Neumann nverts[2*nn]; short ones are compiled in)
// and seg_phi: the device's per-segment normal angles of a compiled-in Neumann polyline
// (nn - 1 floats, read back from the setup kernel so the constants carry its bits), or null.
struct PolylineView {
    const float* dverts;
    int nd;
    const float* nverts;
    int nn;
    const float* seg_phi;
};

// HIP source of the walk kernel named "wost_walk_jit" for the variant `v` (wost_variant.h:
// its traits, recorder, channel counts, workgroup, polyline placement, tree staging -- the
// caller's decision, independent of the workgroup size -- and trig choice) with the fields
// of `prog` and the short polylines of `poly` compiled in.
// `opt`: the handle's kernel options (wost_options.h).
std::string jit_generate(const Options& opt, const KernelVariant& v, const ProgramView& prog, const PolylineView& poly);

// Compiles (or fetches from the caches) the source for `device` and returns
// the kernel. On failure returns false and a message in *err.
// alpha_fn (optional): the source's wost_point_alpha_jit kernel (delta tracking), or null.
// opt: the compile options it selects (the SLP vectoriser; study builds: the scheduler).
// *compile_ms: host time of the hiprtc compile (0 when a cache had the code).
bool jit_get_kernel(const Options& opt, int device, const std::string& source, hipFunction_t* fn, std::string* err,
                    hipFunction_t* alpha_fn = nullptr, double* compile_ms = nullptr);

// Background compiles for a solve that can run on the precompiled kernel meanwhile
// (option jit_race, wost_api.hip solve_race): jit_try_kernel returns
//   kReady   -- *fn is the kernel (in memory, on disk, or a finished background compile);
//   kStarted -- it was nowhere and nothing compiled it: a compile started now in a helper
//               process (a detached thread waits for it and fills the disk cache); *ticket
//               says when it is done, and jit_get_kernel then loads it without compiling;
//   kWait    -- only a blocking jit_get_kernel gets it (a compile of it is already running,
//               or failed, or there is no helper).
enum class JitTry { kReady, kStarted, kWait };
struct JitTicket {
    const void* p = nullptr;
    bool done() const;
};
JitTry jit_try_kernel(const Options& opt, int device, const std::string& source, hipFunction_t* fn,
                      hipFunction_t* alpha_fn, JitTicket* ticket, std::string* err);

// A compile of `source` for `arch` with the options `opt` selects, without a device (the
// helper process wost_jitc when there is one and opt.jit_process is set, else in this
// process; *in_helper says which ran). For wost_jit_compile and the tests.
bool jit_compile_host(const Options& opt, const std::string& source, const std::string& arch,
                      std::vector<char>* code, std::string* err, bool* in_helper);
// Whether the compile helper is installed next to this library (and runs).
// Study builds (option vote_stats): the device address and size of a module-scope variable
// of the loaded module that `fn` belongs to; false when it has none of that name.
bool jit_kernel_global(hipFunction_t fn, const char* name, void** dptr, size_t* bytes);
bool jit_helper_available();
// Starts finding the helper's compiler in the background (once per process; wost_create),
// so that the first compile does not wait for the helper's start.
void jit_start_identity_probe();

}  // namespace wost
