// Training mode of the DINO ViT-small feature branch (models/vision_transformer.py:104-154,194-214,324-451 under autograd, as
// models/mvsformer_model.py:216-219 runs it with "fix": false): the pieces of the backward that are not matrix products.  Every matrix
// product of the forward and the backward - the linear layers' data and weight gradients, Q K^T, P V and the four products of the attention
// backward - is mvs_gemm_x3 (csrc/vit.hip, three-term split form, fp32-equivalent; a_mode 3 reads dY^T for dW = dY^T X).
//
//   mvs_layernorm_stats       LayerNorm forward that also writes each row's mean and 1 / std (what the backward reads)
//   mvs_layernorm_bwd         dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) with g = dy * gamma, plus an optional residual gradient
//   mvs_colsum                column sums of dy (a bias gradient) or of (dy * xhat, dy) (LayerNorm's dgamma / dbeta): per-chunk partial
//                             rows, then mvs::launch_partials_reduce in a fixed order - no atomics, bitwise reproducible
//   mvs_gelu_fwd / _bwd       GELU(erf) on the saved fc1 pre-activation and its derivative
//   mvs_attention_softmax_bwd dS = scale * P * (dP + dA - rowsum(P * (dP + dA))) per attention row (dA: the gradient of the returned attention
//                             matrix - its CLS row only, or all rows)
//   mvs_bicubic_resize_bwd    the adjoint of mvs_bicubic_resize in gather form (two separable passes, each output element sums its own taps
//                             in a fixed order)
#include "common.h"
#include "prims.h"

namespace {
using mvsprim::cc1;
using mvsprim::cc2;

// ---------------------------------------------------------------------------------------------------------------- LayerNorm
// One wavefront per row (C <= 1024), the arithmetic of csrc/vit.hip layernorm_kernel.
__global__ __launch_bounds__(256) void layernorm_stats_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ b,
                                                              float* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                              int rows, int C, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float* xr = x + (size_t)row * C;
    float v[16];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + i * 64;
        v[i] = c < C ? xr[c] : 0.0f;
        s += v[i];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    const float mean = s / (float)C;
    float q = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + i * 64;
        const float d = c < C ? v[i] - mean : 0.0f;
        q = fmaf(d, d, q);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) q += __shfl_xor(q, m, 64);
    const float rstd = 1.0f / sqrtf(q / (float)C + eps);
    float* yr = y + (size_t)row * C;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + i * 64;
        if (c < C) yr[c] = fmaf((v[i] - mean) * rstd, g[c], b[c]);
    }
    if (lane == 0) mean_out[row] = mean, rstd_out[row] = rstd;
}

__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, const float* __restrict__ g, const float* __restrict__ res,
                                                            float* __restrict__ dx, int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const size_t o = (size_t)row * C;
    const float mu = mean[row], rs = rstd[row];
    float gv[16], xh[16];
    float sa = 0.0f, sb = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + i * 64;
        gv[i] = c < C ? dy[o + c] * g[c] : 0.0f;
        xh[i] = c < C ? (x[o + c] - mu) * rs : 0.0f;
        sa += gv[i];
        sb = fmaf(gv[i], xh[i], sb);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sa += __shfl_xor(sa, m, 64), sb += __shfl_xor(sb, m, 64);
    const float a = sa / (float)C, bm = sb / (float)C;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + i * 64;
        if (c < C) {
            float v = rs * (gv[i] - a - xh[i] * bm);
            if (res) v += res[o + c];
            dx[o + c] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- column sums
constexpr int COLSUM_ROWS = 64;                              // rows per partial

// part[chunk][c] = sum over the chunk's rows of dy (x == NULL), or part[chunk][c] = sum dy * xhat, part[chunk][C + c] = sum dy
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ rstd, int64_t rows, int64_t C, float* __restrict__ part) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int64_t r0 = (int64_t)blockIdx.y * COLSUM_ROWS, r1 = r0 + COLSUM_ROWS < rows ? r0 + COLSUM_ROWS : rows;
    float s = 0.0f, sg = 0.0f;
    for (int64_t r = r0; r < r1; ++r) {
        const float d = dy[r * C + c];
        sg += d;
        if (x) s = fmaf(d, (x[r * C + c] - mean[r]) * rstd[r], s);
    }
    if (x) {
        part[(int64_t)blockIdx.y * 2 * C + c] = s;
        part[(int64_t)blockIdx.y * 2 * C + C + c] = sg;
    } else {
        part[(int64_t)blockIdx.y * C + c] = sg;
    }
}

// ---------------------------------------------------------------------------------------------------------------- GELU(erf)
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    y[i] = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));     // = csrc/vit.hip gelu_erf (the GEMM epilogue's act 1)
}

__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * v * v) * 0.39894228040143267794f;
    dx[i] = dy[i] * fmaf(v, pdf, cdf);
}

// ---------------------------------------------------------------------------------------------------------------- softmax backward
// One block per attention row (N <= 8192, 32 values per thread in registers), the row sum in a fixed order (xor-shuffle tree, then the four
// waves in order).  Row i of head bh: g = dP + dA (dA row: da_rows == N -> row i, da_rows == 1 -> only i == 0 has one).
__global__ __launch_bounds__(256) void attention_softmax_bwd_kernel(const float* __restrict__ P, const float* __restrict__ dP, const float* __restrict__ dA,
                                                                    int da_rows, float* __restrict__ dS, int N, float scale) {
    __shared__ float red[4];
    const size_t row = blockIdx.x;
    const int bh = (int)(row / N), i = (int)(row % N);
    const float* pr = P + row * N;
    const float* dr = dP + row * N;
    const float* ar = nullptr;
    if (dA && (da_rows == N || i == 0)) ar = dA + ((size_t)bh * da_rows + (da_rows == N ? i : 0)) * N;
    float p[32], g[32];
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int c = threadIdx.x + k * 256;
        p[k] = c < N ? pr[c] : 0.0f;
        g[k] = c < N ? dr[c] + (ar ? ar[c] : 0.0f) : 0.0f;
        s = fmaf(p[k], g[k], s);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float delta = (red[0] + red[1]) + (red[2] + red[3]);
    float* out = dS + row * N;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int c = threadIdx.x + k * 256;
        if (c < N) out[c] = scale * p[k] * (g[k] - delta);
    }
}

// ---------------------------------------------------------------------------------------------------------------- bicubic adjoint
// The forward's taps (csrc/vit.hip bicubic_kernel): output o reads inputs clamp(floor(s) - 1 + t, 0, In - 1), t = 0..3, s = (o + 0.5) * r - 0.5,
// weights cubic_coeffs(s - floor(s)).  An interior input i is read only by outputs with floor(s) in [i - 2, i + 1]; the edge inputs also
// receive the clamped taps, so their range runs to the end of the axis.  Each output of the adjoint sums its contributions in order of o.

// weight of input i in output o along one axis
__device__ __forceinline__ float tap_weight(int o, int i, float r, int In) {
    const float s = ((float)o + 0.5f) * r - 0.5f, f = floorf(s), t = s - f;
    const float c[4] = {cc2(t + 1.0f), cc1(t), cc1(1.0f - t), cc2(2.0f - t)};
    const int f0 = (int)f;
    float w = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a)
        if (min(max(f0 - 1 + a, 0), In - 1) == i) w += c[a];
    return w;
}

__device__ __forceinline__ void out_range(int i, float r, int In, int Out, int& lo, int& hi) {
    lo = i == 0 ? 0 : max(0, (int)floorf(((float)i - 1.5f) / r - 0.5f) - 2);
    hi = i == In - 1 ? Out - 1 : min(Out - 1, (int)ceilf(((float)i + 2.5f) / r - 0.5f) + 2);
}

// pass 1, along x: tmp[p][oy][ix] = sum_ox w_x(ox, ix) * dout[p][oy][ox]
__global__ __launch_bounds__(256) void bicubic_bwd_x_kernel(const float* __restrict__ dout, float* __restrict__ tmp, int W, int Ho, int Wo, float rw) {
    const int ix = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y;
    if (ix >= W) return;
    const float* src = dout + ((size_t)blockIdx.z * Ho + oy) * Wo;
    int lo, hi;
    out_range(ix, rw, W, Wo, lo, hi);
    float s = 0.0f;
    for (int ox = lo; ox <= hi; ++ox) {
        const float w = tap_weight(ox, ix, rw, W);
        if (w != 0.0f) s = fmaf(w, src[ox], s);
    }
    tmp[((size_t)blockIdx.z * Ho + oy) * W + ix] = s;
}

// pass 2, along y: din[p][iy][ix] = sum_oy w_y(oy, iy) * tmp[p][oy][ix]
__global__ __launch_bounds__(256) void bicubic_bwd_y_kernel(const float* __restrict__ tmp, float* __restrict__ din, int H, int W, int Ho, float rh) {
    const int ix = blockIdx.x * 256 + threadIdx.x, iy = blockIdx.y;
    if (ix >= W) return;
    const float* src = tmp + (size_t)blockIdx.z * Ho * W + ix;
    int lo, hi;
    out_range(iy, rh, H, Ho, lo, hi);
    float s = 0.0f;
    for (int oy = lo; oy <= hi; ++oy) {
        const float w = tap_weight(oy, iy, rh, H);
        if (w != 0.0f) s = fmaf(w, src[(size_t)oy * W], s);
    }
    din[((size_t)blockIdx.z * H + iy) * W + ix] = s;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int mvs_layernorm_stats(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows, int C,
                                   float eps, mvs_stream_t stream) {
    MVS_REQUIRE(x && gamma && beta && y && mean && rstd && rows >= 1 && rows < ((int64_t)1 << 31) && C >= 1 && C <= 1024,
                "mvs_layernorm_stats: rows >= 1, 1 <= C <= 1024 (got %d)", C);
    hipLaunchKernelGGL(layernorm_stats_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, MVS_STREAM(stream), x, gamma, beta, y, mean, rstd,
                       (int)rows, C, eps);
    return mvs::finish_launch("mvs_layernorm_stats");
}

extern "C" int mvs_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* res, float* dx,
                                 int64_t rows, int C, mvs_stream_t stream) {
    MVS_REQUIRE(dy && x && mean && rstd && gamma && dx && rows >= 1 && rows < ((int64_t)1 << 31) && C >= 1 && C <= 1024,
                "mvs_layernorm_bwd: rows >= 1, 1 <= C <= 1024 (got %d)", C);
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, MVS_STREAM(stream), dy, x, mean, rstd, gamma, res, dx,
                       (int)rows, C);
    return mvs::finish_launch("mvs_layernorm_bwd");
}

extern "C" int64_t mvs_colsum_workspace_floats(int64_t rows, int64_t C, int with_x) {
    if (rows < 1 || C < 1) return -1;
    return ((rows + COLSUM_ROWS - 1) / COLSUM_ROWS) * C * (with_x ? 2 : 1);
}

extern "C" int mvs_colsum(const float* dy, const float* x, const float* mean, const float* rstd, int64_t rows, int64_t C, float* out, float* workspace,
                          mvs_stream_t stream) {
    MVS_REQUIRE(dy && out && workspace && rows >= 1 && C >= 1 && (!x || (mean && rstd)), "mvs_colsum: bad arguments");
    const int64_t chunks = (rows + COLSUM_ROWS - 1) / COLSUM_ROWS, width = C * (x ? 2 : 1);
    MVS_REQUIRE(chunks <= 65535 && (C + 255) / 256 < ((int64_t)1 << 31) && width < ((int64_t)1 << 31) && chunks * width < ((int64_t)1 << 31),
                "mvs_colsum: %lld rows x %lld columns is too large", (long long)rows, (long long)C);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(blocks_of(C), (unsigned)chunks), dim3(256), 0, MVS_STREAM(stream), dy, x, mean, rstd, rows, C,
                       workspace);
    mvs::launch_partials_reduce(workspace, (int)chunks, (int)width, out, MVS_STREAM(stream));
    return mvs::finish_launch("mvs_colsum");
}

extern "C" int mvs_gelu_fwd(const float* x, float* y, int64_t n, mvs_stream_t stream) {
    MVS_REQUIRE(x && y && n >= 1 && n < ((int64_t)1 << 40), "mvs_gelu_fwd: bad arguments");
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3(blocks_of(n)), dim3(256), 0, MVS_STREAM(stream), x, y, n);
    return mvs::finish_launch("mvs_gelu_fwd");
}

extern "C" int mvs_gelu_bwd(const float* dy, const float* x, float* dx, int64_t n, mvs_stream_t stream) {
    MVS_REQUIRE(dy && x && dx && n >= 1 && n < ((int64_t)1 << 40), "mvs_gelu_bwd: bad arguments");
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(blocks_of(n)), dim3(256), 0, MVS_STREAM(stream), dy, x, dx, n);
    return mvs::finish_launch("mvs_gelu_bwd");
}

extern "C" int mvs_attention_softmax_bwd(const float* P, const float* dP, const float* dA, int da_rows, float* dS, int64_t BH, int N, float scale,
                                         mvs_stream_t stream) {
    MVS_REQUIRE(P && dP && dS && BH >= 1 && N >= 1 && N <= 8192 && BH * N < ((int64_t)1 << 31), "mvs_attention_softmax_bwd: 1 <= N <= 8192 (got %d)", N);
    MVS_REQUIRE(!dA || da_rows == 1 || da_rows == N, "mvs_attention_softmax_bwd: dA holds 1 (the CLS row) or N rows per head (got %d)", da_rows);
    hipLaunchKernelGGL(attention_softmax_bwd_kernel, dim3((unsigned)(BH * N)), dim3(256), 0, MVS_STREAM(stream), P, dP, dA, da_rows, dS, N, scale);
    return mvs::finish_launch("mvs_attention_softmax_bwd");
}

extern "C" int mvs_bicubic_resize_bwd(const float* dout, float* din, float* tmp, int planes, int H, int W, int Ho, int Wo, float rscale_h,
                                      float rscale_w, mvs_stream_t stream) {
    MVS_REQUIRE(dout && din && tmp && planes >= 1 && planes <= 65535 && H >= 1 && H <= 65535 && W >= 1 && Ho >= 1 && Ho <= 65535 && Wo >= 1 &&
                rscale_h > 0.0f && rscale_w > 0.0f, "mvs_bicubic_resize_bwd: bad shape");
    hipLaunchKernelGGL(bicubic_bwd_x_kernel, dim3(blocks_of(W), Ho, planes), dim3(256), 0, MVS_STREAM(stream), dout, tmp, W, Ho, Wo, rscale_w);
    hipLaunchKernelGGL(bicubic_bwd_y_kernel, dim3(blocks_of(W), H, planes), dim3(256), 0, MVS_STREAM(stream), tmp, din, H, W, Ho, rscale_h);
    return mvs::finish_launch("mvs_bicubic_resize_bwd");
}
