// AdamW over MANY parameter tensors in a few launches (the reference's optimizer, train.py:98 torch.optim.AdamW; decoupled weight
// decay, Loshchilov & Hutter):
//     p <- p * (1 - lr * wd);  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;
//     p <- p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps),        t = step + 1
// The cascade's hot path has ~190 parameter tensors with 1.2 M values: ATen's multi-tensor kernel gives every tensor (chunk of 64 K values)
// to ONE block, so a launch lasts as long as its largest tensor takes a single block - five launches of 40 us per step.  Here a block owns
// 2048 consecutive values of one tensor (block -> tensor through a table in the kernel arguments: by value, so a hipGraph captures it with
// the launch and nothing has to stay alive), ~650 blocks for the whole path; the step count lives on the device and is advanced by a
// one-thread launch after the updates (all of them read the old value).
//
// mvs_adamw_multi / mvs_grad_norm / mvs_grad_scale_ (below) are the forms for the reference's training RECIPE (train.py:78-100,
// trainer/mvsformer_trainer.py:39-45, 157-167): layer-wise parameter groups, a learning rate that changes every step, a GradScaler and
// global-norm clipping.  Everything that changes between steps - the groups' hyper-parameters, the step counts, the gradient multiplier
// (clip coefficient / loss scale) and the overflow flag - is read from DEVICE memory, so one captured hipGraph stays valid for a whole
// run; the tensors of ALL groups share the launches (an entry of the table names its group).
#include <math.h>

#include "common.h"

namespace {
constexpr int AD_GROUP = 88;                                  // tensors per launch (kernel arguments are limited to 4 KB)
constexpr int AD_BLOCK = 2048;                                // values per block

struct AdamGroup {
    int n;
    int start[AD_GROUP + 1];                                  // first block of tensor i
    MvsAdamTensor t[AD_GROUP];
};
static_assert(sizeof(AdamGroup) <= 3900, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(256) void adamw_kernel(const AdamGroup g, float lr, float beta1, float beta2, float eps, float wd, int maximize,
                                                    const float* __restrict__ step) {
    int lo = 0, hi = g.n - 1;                                 // the tensor of this block: binary search over the (block-uniform) table
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= g.start[mid]) lo = mid;
        else hi = mid - 1;
    }
    const MvsAdamTensor t = g.t[lo];
    const long long base = (long long)((int)blockIdx.x - g.start[lo]) * AD_BLOCK;
    const double tt = (double)step[0] + 1.0;
    const float bc1 = (float)(1.0 - pow((double)beta1, tt)), bc2s = sqrtf((float)(1.0 - pow((double)beta2, tt)));
    const float step_size = lr / bc1, decay = 1.0f - lr * wd;
#pragma unroll
    for (int k = 0; k < AD_BLOCK / 256; ++k) {
        const long long i = base + k * 256 + threadIdx.x;
        if (i >= t.n) break;
        const float gr = maximize ? -t.g[i] : t.g[i];
        const float m = beta1 * t.m[i] + (1.0f - beta1) * gr;
        const float v = beta2 * t.v[i] + (1.0f - beta2) * gr * gr;
        t.m[i] = m;
        t.v[i] = v;
        t.p[i] = t.p[i] * decay - step_size * (m / (sqrtf(v) / bc2s + eps));
    }
}

__global__ void adamw_advance_kernel(float* step) { step[0] += 1.0f; }

// ---------------------------------------------------------------------------------------------- the multi-group forms
constexpr int MT_GROUP = 74;                                  // entries per launch (48 B each + a block start)
constexpr int MT_MAX_GROUPS = 1024;

struct MultiTable {
    int n;
    int start[MT_GROUP + 1];                                  // first block of entry i
    MvsAdamEntry t[MT_GROUP];
};
static_assert(sizeof(MultiTable) <= 3900, "kernel arguments are limited to 4 KB");

struct GroupMask {
    unsigned w[MT_MAX_GROUPS / 32];                           // bit g: group g has a tensor in this step
};

__device__ __forceinline__ int entry_of_block(const MultiTable& g) {
    int lo = 0, hi = g.n - 1;                                 // binary search over the (block-uniform) table, as adamw_kernel
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= g.start[mid]) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

struct AdamConsts {
    float beta1, beta2, eps, step_size, decay, bc2s, gmul;
    int maximize;
};

// adamw_kernel's arithmetic, operation for operation (the gradient is multiplied by gmul first: x * 1.0f keeps x's bits)
__device__ __forceinline__ void adam_one(const AdamConsts& c, float g, float& p, float& m, float& v) {
    g *= c.gmul;
    const float gr = c.maximize ? -g : g;
    m = c.beta1 * m + (1.0f - c.beta1) * gr;
    v = c.beta2 * v + (1.0f - c.beta2) * gr * gr;
    p = p * c.decay - c.step_size * (m / (sqrtf(v) / c.bc2s + c.eps));
}

// hyper[group][MVS_ADAM_HYPER_STRIDE] = lr, weight_decay, beta1, beta2, eps, maximize (0 / 1), 0, 0
__global__ __launch_bounds__(256) void adamw_multi_kernel(const MultiTable g, const float* __restrict__ hyper, const float* __restrict__ step,
                                                          const float* __restrict__ grad_mul, const int* __restrict__ skip) {
    if (skip && skip[0]) return;                              // overflow / non-finite norm: nothing is written
    const int e = entry_of_block(g);
    const MvsAdamEntry t = g.t[e];
    const long long base = (long long)((int)blockIdx.x - g.start[e]) * AD_BLOCK;
    const float* h = hyper + (size_t)t.group * MVS_ADAM_HYPER_STRIDE;
    const float lr = h[0], wd = h[1], beta1 = h[2], beta2 = h[3];
    const double tt = (double)step[t.group] + 1.0;
    const float bc1 = (float)(1.0 - pow((double)beta1, tt));
    AdamConsts c;
    c.beta1 = beta1;
    c.beta2 = beta2;
    c.eps = h[4];
    c.maximize = h[5] != 0.0f;
    c.bc2s = sqrtf((float)(1.0 - pow((double)beta2, tt)));
    c.step_size = lr / bc1;
    c.decay = 1.0f - lr * wd;
    c.gmul = grad_mul ? grad_mul[0] : 1.0f;
    if (aligned16(t.p, t.g, t.m, t.v)) {                      // 16-byte accesses; the last (n % 4) values of a tensor one by one
#pragma unroll
        for (int k = 0; k < AD_BLOCK / 1024; ++k) {
            const long long i = base + (long long)(k * 256 + (int)threadIdx.x) * 4;
            if (i + 3 < t.n) {
                const float4 gv = *reinterpret_cast<const float4*>(t.g + i);
                float4 pv = *reinterpret_cast<const float4*>(t.p + i);
                float4 mv = *reinterpret_cast<const float4*>(t.m + i);
                float4 vv = *reinterpret_cast<const float4*>(t.v + i);
                adam_one(c, gv.x, pv.x, mv.x, vv.x);
                adam_one(c, gv.y, pv.y, mv.y, vv.y);
                adam_one(c, gv.z, pv.z, mv.z, vv.z);
                adam_one(c, gv.w, pv.w, mv.w, vv.w);
                *reinterpret_cast<float4*>(t.m + i) = mv;
                *reinterpret_cast<float4*>(t.v + i) = vv;
                *reinterpret_cast<float4*>(t.p + i) = pv;
            } else {
                for (long long j = i; j < t.n; ++j) adam_one(c, t.g[j], t.p[j], t.m[j], t.v[j]);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < AD_BLOCK / 256; ++k) {
            const long long i = base + k * 256 + threadIdx.x;
            if (i >= t.n) break;
            adam_one(c, t.g[i], t.p[i], t.m[i], t.v[i]);
        }
    }
}

// after the updates: the counts of the groups that had a tensor advance, unless the step was skipped (then skipped_steps does)
__global__ void adamw_multi_advance_kernel(const GroupMask mask, int ngroups, float* step, const int* __restrict__ skip, int* skipped_steps) {
    const int gi = blockIdx.x * blockDim.x + threadIdx.x;
    const bool sk = skip && skip[0];
    if (gi == 0 && sk && skipped_steps) skipped_steps[0] += 1;
    if (gi < ngroups && !sk && ((mask.w[gi >> 5] >> (gi & 31)) & 1u)) step[gi] += 1.0f;
}

// sum over the 256 threads of a block in a fixed order (xor tree inside a wave, then the four waves in index order); valid in thread 0
__device__ __forceinline__ double block_sum_256(double acc) {
    __shared__ double wave_sum[4];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// pass 1 of the global gradient norm: partial[first_block + blockIdx.x] = sum of g^2 over this block's 2048 values, in double
__global__ __launch_bounds__(256) void grad_sq_kernel(const MultiTable g, double* __restrict__ partial) {
    const int e = entry_of_block(g);
    const MvsAdamEntry t = g.t[e];
    const long long base = (long long)((int)blockIdx.x - g.start[e]) * AD_BLOCK;
    double acc = 0.0;
    if (aligned16(t.g)) {
#pragma unroll
        for (int k = 0; k < AD_BLOCK / 1024; ++k) {
            const long long i = base + (long long)(k * 256 + (int)threadIdx.x) * 4;
            if (i + 3 < t.n) {
                const float4 gv = *reinterpret_cast<const float4*>(t.g + i);
                acc += (double)gv.x * (double)gv.x;
                acc += (double)gv.y * (double)gv.y;
                acc += (double)gv.z * (double)gv.z;
                acc += (double)gv.w * (double)gv.w;
            } else {
                for (long long j = i; j < t.n; ++j) acc += (double)t.g[j] * (double)t.g[j];
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < AD_BLOCK / 256; ++k) {
            const long long i = base + k * 256 + threadIdx.x;
            if (i >= t.n) break;
            acc += (double)t.g[i] * (double)t.g[i];
        }
    }
    acc = block_sum_256(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// pass 2: one block adds the partials (thread i takes i, i + 256, ...; then the block tree: a fixed order) and writes the three scalars
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ partial, long long nparts, float max_norm,
                                                              const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                              float* norm, float* grad_mul, int* skip) {
    double acc = 0.0;
    for (long long i = threadIdx.x; i < nparts; i += 256) acc += partial[i];
    acc = block_sum_256(acc);
    if (threadIdx.x != 0) return;
    const float scale = grad_scale ? grad_scale[0] : 1.0f;
    const float total = (float)(sqrt(acc) / (double)scale);   // the norm of the UNSCALED gradients
    float coef = 1.0f;
    if (max_norm > 0.0f && max_norm < INFINITY) {             // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
        coef = max_norm / (total + 1e-6f);
        if (coef > 1.0f) coef = 1.0f;                         // a NaN stays a NaN, as torch's clamp keeps it
    }
    norm[0] = total;
    grad_mul[0] = grad_scale ? coef / scale : coef;
    if (skip) skip[0] = ((found_inf && found_inf[0] != 0.0f) || !isfinite(total)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const MultiTable g, const float* __restrict__ grad_mul) {
    const int e = entry_of_block(g);
    const MvsAdamEntry t = g.t[e];
    const long long base = (long long)((int)blockIdx.x - g.start[e]) * AD_BLOCK;
    const float mul = grad_mul[0];
    if (aligned16(t.g)) {
#pragma unroll
        for (int k = 0; k < AD_BLOCK / 1024; ++k) {
            const long long i = base + (long long)(k * 256 + (int)threadIdx.x) * 4;
            if (i + 3 < t.n) {
                float4 gv = *reinterpret_cast<const float4*>(t.g + i);
                gv.x *= mul;
                gv.y *= mul;
                gv.z *= mul;
                gv.w *= mul;
                *reinterpret_cast<float4*>(t.g + i) = gv;
            } else {
                for (long long j = i; j < t.n; ++j) t.g[j] *= mul;
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < AD_BLOCK / 256; ++k) {
            const long long i = base + k * 256 + threadIdx.x;
            if (i >= t.n) break;
            t.g[i] *= mul;
        }
    }
}

// Cuts the host table into launches of MT_GROUP entries and calls launch(table, first block of this launch over the whole table).
// `all_pointers`: p, m, v are required too (the norm and the scaling touch g alone).
template <class Launch>
int for_each_launch(const char* who, const MvsAdamEntry* tensors, int ntensors, int ngroups, bool all_pointers, Launch launch) {
    long long first_block = 0;
    for (int first = 0; first < ntensors; first += MT_GROUP) {
        MultiTable g{};
        g.n = ntensors - first < MT_GROUP ? ntensors - first : MT_GROUP;
        for (int i = 0; i < g.n; ++i) {
            const MvsAdamEntry& t = tensors[first + i];
            MVS_REQUIRE(t.g && t.n >= 1 && t.n < ((int64_t)1 << 40) && (!all_pointers || (t.p && t.m && t.v)),
                        "%s: tensor %d: null pointer or bad size", who, first + i);
            MVS_REQUIRE(t.group >= 0 && t.group < ngroups, "%s: tensor %d: group %d of %d", who, first + i, t.group, ngroups);
            g.t[i] = t;
            const int64_t blocks = (t.n + AD_BLOCK - 1) / AD_BLOCK;
            MVS_REQUIRE(g.start[i] + blocks < ((int64_t)1 << 31), "%s: too many blocks", who);
            g.start[i + 1] = g.start[i] + (int)blocks;
        }
        launch(g, first_block);
        if (int rc = mvs::finish_launch(who)) return rc;
        first_block += g.start[g.n];
    }
    return MVS_OK;
}
}  // namespace

extern "C" int mvs_adamw_step(const MvsAdamTensor* tensors, int ntensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                              int maximize, float* step, mvs_stream_t stream) {
    MVS_REQUIRE(tensors && ntensors >= 1 && ntensors <= 1 << 20 && step, "mvs_adamw_step: bad arguments (ntensors=%d)", ntensors);
    MVS_REQUIRE(lr >= 0.0f && beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f && eps >= 0.0f && weight_decay >= 0.0f,
                "mvs_adamw_step: lr %g, betas (%g, %g), eps %g, weight_decay %g out of range", lr, beta1, beta2, eps, weight_decay);
    hipStream_t s = MVS_STREAM(stream);
    for (int first = 0; first < ntensors; first += AD_GROUP) {
        AdamGroup g{};
        g.n = ntensors - first < AD_GROUP ? ntensors - first : AD_GROUP;
        for (int i = 0; i < g.n; ++i) {
            const MvsAdamTensor& t = tensors[first + i];
            MVS_REQUIRE(t.p && t.g && t.m && t.v && t.n >= 1 && t.n < ((int64_t)1 << 40), "mvs_adamw_step: tensor %d: null pointer or bad size", first + i);
            g.t[i] = t;
            const int64_t blocks = (t.n + AD_BLOCK - 1) / AD_BLOCK;
            MVS_REQUIRE(g.start[i] + blocks < ((int64_t)1 << 31), "mvs_adamw_step: too many blocks");
            g.start[i + 1] = g.start[i] + (int)blocks;
        }
        hipLaunchKernelGGL(adamw_kernel, dim3(g.start[g.n]), dim3(256), 0, s, g, lr, beta1, beta2, eps, weight_decay, maximize, step);
        if (int rc = mvs::finish_launch("mvs_adamw_step")) return rc;
    }
    hipLaunchKernelGGL(adamw_advance_kernel, dim3(1), dim3(1), 0, s, step);
    return mvs::finish_launch("mvs_adamw_step");
}

extern "C" int mvs_adamw_multi(const MvsAdamEntry* tensors, int ntensors, const float* hyper, int ngroups, float* step, const float* grad_mul,
                               const int* skip, int* skipped_steps, mvs_stream_t stream) {
    MVS_REQUIRE(tensors && ntensors >= 1 && ntensors <= 1 << 20 && hyper && step && ngroups >= 1 && ngroups <= MT_MAX_GROUPS,
                "mvs_adamw_multi: bad arguments (ntensors=%d, ngroups=%d, at most %d groups)", ntensors, ngroups, MT_MAX_GROUPS);
    hipStream_t s = MVS_STREAM(stream);
    GroupMask mask{};
    for (int i = 0; i < ntensors; ++i)
        if (tensors[i].group >= 0 && tensors[i].group < ngroups) mask.w[tensors[i].group >> 5] |= 1u << (tensors[i].group & 31);
    if (int rc = for_each_launch("mvs_adamw_multi", tensors, ntensors, ngroups, true, [&](const MultiTable& g, long long) {
            hipLaunchKernelGGL(adamw_multi_kernel, dim3(g.start[g.n]), dim3(256), 0, s, g, hyper, step, grad_mul, skip);
        }))
        return rc;
    hipLaunchKernelGGL(adamw_multi_advance_kernel, dim3((ngroups + 63) / 64), dim3(64), 0, s, mask, ngroups, step, skip, skipped_steps);
    return mvs::finish_launch("mvs_adamw_multi");
}

extern "C" int64_t mvs_grad_norm_workspace_bytes(const MvsAdamEntry* tensors, int ntensors) {
    if (!tensors || ntensors < 1 || ntensors > 1 << 20) return -1;
    int64_t blocks = 0;
    for (int i = 0; i < ntensors; ++i) {
        if (tensors[i].n < 1 || tensors[i].n >= ((int64_t)1 << 40)) return -1;
        blocks += (tensors[i].n + AD_BLOCK - 1) / AD_BLOCK;
    }
    return blocks * (int64_t)sizeof(double);
}

extern "C" int mvs_grad_norm(const MvsAdamEntry* tensors, int ntensors, float max_norm, const float* grad_scale, const float* found_inf,
                             void* workspace, float* norm, float* grad_mul, int* skip, mvs_stream_t stream) {
    MVS_REQUIRE(tensors && ntensors >= 1 && ntensors <= 1 << 20 && workspace && norm && grad_mul && ((uintptr_t)workspace & 7) == 0,
                "mvs_grad_norm: bad arguments (ntensors=%d)", ntensors);
    MVS_REQUIRE(max_norm == max_norm, "mvs_grad_norm: max_norm is NaN");
    hipStream_t s = MVS_STREAM(stream);
    double* partial = static_cast<double*>(workspace);
    long long nparts = 0;
    if (int rc = for_each_launch("mvs_grad_norm", tensors, ntensors, 1 << 30, false, [&](const MultiTable& g, long long first_block) {
            hipLaunchKernelGGL(grad_sq_kernel, dim3(g.start[g.n]), dim3(256), 0, s, g, partial + first_block);
            nparts = first_block + g.start[g.n];
        }))
        return rc;
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, s, partial, nparts, max_norm, grad_scale, found_inf, norm, grad_mul, skip);
    return mvs::finish_launch("mvs_grad_norm");
}

extern "C" int mvs_grad_scale_(const MvsAdamEntry* tensors, int ntensors, const float* grad_mul, mvs_stream_t stream) {
    MVS_REQUIRE(tensors && ntensors >= 1 && ntensors <= 1 << 20 && grad_mul, "mvs_grad_scale_: bad arguments (ntensors=%d)", ntensors);
    hipStream_t s = MVS_STREAM(stream);
    return for_each_launch("mvs_grad_scale_", tensors, ntensors, 1 << 30, false, [&](const MultiTable& g, long long) {
        hipLaunchKernelGGL(grad_scale_kernel, dim3(g.start[g.n]), dim3(256), 0, s, g, grad_mul);
    });
}
