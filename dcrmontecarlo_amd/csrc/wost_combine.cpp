// wost_combine.cpp -- weighted channel combinations on the host (wost_combine.h): the
// weights' checks and the block rows of wost_block_combine restated op for op. No HIP.
#include "wost_combine.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace wost {

int combine_check_weights(const double* weights, int32_t n_combinations, int32_t n_channels, char* msg,
                          size_t msg_cap) {
    if (n_combinations < 1 || n_combinations > kCombineMax) {
        std::snprintf(msg, msg_cap, "need 1..%d combinations (got %d)", kCombineMax, (int)n_combinations);
        return 1;
    }
    if (n_channels < 1 || n_channels > kCombineMax) {
        std::snprintf(msg, msg_cap, "need 1..%d channels (got %d)", kCombineMax, (int)n_channels);
        return 1;
    }
    if (!weights) {
        std::snprintf(msg, msg_cap, "NULL weights");
        return 1;
    }
    for (int32_t i = 0; i < n_combinations * n_channels; ++i)
        if (!std::isfinite(weights[i])) {
            std::snprintf(msg, msg_cap, "weight [%d][%d] is not finite", (int)(i / n_channels), (int)(i % n_channels));
            return 1;
        }
    return 0;
}

void combine_blocks_host(const float* values, const int64_t* begin, int64_t n_blocks, int32_t n_channels,
                         const double* weights, int32_t n_combinations, double* out) {
    const int C = n_channels, L = n_combinations;
    std::vector<double> sum((size_t)kCombineBlock), sq((size_t)kCombineBlock);
    for (int64_t b = 0; b < n_blocks; ++b) {
        const int64_t lo = begin[b], hi = begin[b + 1];
        for (int l = 0; l < L; ++l) {
            for (int t = 0; t < kCombineBlock; ++t) {
                double s = 0.0, q = 0.0;
                for (int64_t i = lo + t; i < hi; i += kCombineBlock)
                    combine_accumulate(s, q, combine_walk(values + i * C, weights + (size_t)l * C, C));
                sum[(size_t)t] = s;
                sq[(size_t)t] = q;
            }
            for (int h = kCombineBlock / 2; h > 0; h >>= 1)
                for (int t = 0; t < h; ++t) {
                    sum[(size_t)t] += sum[(size_t)(t + h)];
                    sq[(size_t)t] += sq[(size_t)(t + h)];
                }
            out[(size_t)b * 2 * L + 2 * l] = sum[0];
            out[(size_t)b * 2 * L + 2 * l + 1] = sq[0];
        }
    }
}

}  // namespace wost
