// fp64 forms of the fixed-order partial-row reductions of common.h, for the BatchNorm FORWARD statistics: sum x and sum x^2 are carried in
// double from the accumulators to the finalize kernels, which form var = sum x^2 / n - mean^2 - a difference that cancels |mean/std|^2 of
// the leading digits (fp32 sums leave nothing of the variance of a channel whose mean is 100 standard deviations from zero).
#pragma once
#include "common.h"

namespace mvs {

// out[j] = sum_p part[p * n + j] over fp64 partial rows (mvs_bn_stats: fp64 lane accumulators)
void launch_partials_reduce(const double* part, int nparts, int n, double* out, hipStream_t stream);

// launch_partials_reduce_grouped over fp32 partial rows (short fp32 chains: one block's rows each) added in double: the bf16 path
void launch_partials_reduce_grouped(const float* part, int bps, int nsamples, int groups, int C, double* out, hipStream_t stream);

}  // namespace mvs
