// The one home of the training BatchNorm arithmetic that train.hip (fp32 [B,C,N]) and bf16_train.hip (bf16 channel-last) share; included
// by those two files and by nothing of the eval path.  The kernels keep their own row walks and reduction trees (the summation order is
// part of the behaviour); what follows a reduction is written here, once.  Expression order and float / double types are the contract:
// with -ffp-contract=off the results are the bits the source spells.
#pragma once
#include "common.h"

namespace mvsbn {

// Sums of one (group, channel) -> the eval-style affine form and the saved statistics.  mean and var stay DOUBLE (var = s2/n - mean^2
// cancels |mean/std|^2 of the leading digits); shift is formed against the ROUNDED scale: x*scale + shift = (x - mean)*scale + beta.
__device__ __forceinline__ void finalize(double s1, double s2, double count, float gamma, float beta, float eps, float& scale, float& shift,
                                         float& mean_out, float& invstd, double& var) {
    const double mean = s1 / count;
    var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
    invstd = (float)(1.0 / sqrt(var + (double)eps));
    scale = gamma * invstd;
    shift = (float)((double)beta - mean * (double)scale);
    mean_out = (float)mean;
}

// One BatchNorm call's update of the running statistics (unbiased variance); a grouped BatchNorm applies it once per group IN ORDER.
__device__ __forceinline__ void running_update(float& rm, float& rv, float momentum, float mean, double var, double count) {
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    rm = (1.0f - momentum) * rm + momentum * mean;
    rv = (1.0f - momentum) * rv + momentum * (float)unbiased;
}

// Gradient through the ReLU after a BatchNorm: zero where x*scale + shift is not positive (NaN included).  scale and shift come as
// ADDRESSES, read only under `relu` as the callers' hand-written forms read them (by value the loads would become unconditional).
__device__ __forceinline__ float masked_grad(float g, float x, const float* scale, const float* shift, int relu) {
    if (relu && !(fmaf(x, *scale, *shift) > 0.0f)) g = 0.0f;
    return g;
}

// Sum of v over the block: xor-shuffle tree in a wavefront, then the wavefronts' values through red[] (blockDim.x / 64 entries) in order
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    T t = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
    return t;
}

}  // namespace mvsbn
