// wost_combine.h -- the arithmetic of weighted channel combinations, one
// text for the device (wost_kernels.hip wost_block_combine) and the host
// (wost_combine.cpp): L combinations v_l = sum_c w[l][c] val[walk][c] of a launch's C
// channels per walk, and their (sum, sum^2) per block of walks in wost_block_reduce's
// order. Usable without HIP, like the host-callable parts of wost_device.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define WOST_CHD __host__ __device__ inline
#else
#define WOST_CHD inline
#endif

namespace wost {

constexpr int kCombineBlock = 256;     // threads of a workgroup: wost_block_reduce's kReduceBlock
constexpr int kCombineMax = 16;        // combinations and channels per launch (WOST_MAX_SOURCES)

// One product and one sum, each rounded on its own: never a fused multiply-add, whatever
// the contraction mode of the unit that includes this header. Under clang (the library's
// compiler, host and device) the pragma sees to it: plain operators under it carry no
// contraction flag. HIP's __dmul_rn / __dadd_rn do not serve: they come from the device
// library as a multiply and an add that the backend still fuses (v_fmac_f64 in
// wost_block_combine's ISA). Under GCC (the host checks of tests/native) the function is
// compiled with -ffp-contract=off.
#if defined(__GNUC__) && !defined(__clang__)
#define WOST_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define WOST_NO_CONTRACT
#endif
WOST_NO_CONTRACT WOST_CHD double combine_term(double acc, double w, double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = w * x;
    return acc + p;
}

// Combination l of one walk: v starts at 0.0, then for c ascending v = v + w[c] * x[c],
// a term whose weight is exactly 0.0 skipped (a sparse row costs what it uses, and a unit
// row is x[c] itself whatever the other channels hold, a NaN or an infinity included).
template <class X>
WOST_CHD double combine_walk(const X* x, const double* w, int C) {
    double v = 0.0;
    for (int c = 0; c < C; ++c)
        if (w[c] != 0.0) v = combine_term(v, w[c], (double)x[c]);
    return v;
}

// A thread's running (sum, sum^2), as wost_block_reduce's `s += v; q += v * v` compiles
// for gfx950: the sum a plain add, the square contracted into one fused multiply-add
// (v_fma_f64 in the kernel's ISA).
WOST_CHD void combine_accumulate(double& s, double& q, double v) {
    s = s + v;
    q = __builtin_fma(v, v, q);
}

// ---- wost_combine.cpp (host only) ----
// 0 when the L x C weights are usable, else a message: L in [1, kCombineMax], C in
// [1, kCombineMax], weights not NULL and finite.
int combine_check_weights(const double* weights, int32_t n_combinations, int32_t n_channels, char* msg,
                          size_t msg_cap);
// The rows [n_blocks][2L] of (sum_l, sumsq_l) of blocks b = walks [begin[b], begin[b+1]) of
// values [walks][C], op for op the device's: thread t of kCombineBlock takes walks lo + t,
// lo + t + kCombineBlock, ..., then the halving tree.
void combine_blocks_host(const float* values, const int64_t* begin, int64_t n_blocks, int32_t n_channels,
                         const double* weights, int32_t n_combinations, double* out);

}  // namespace wost
