// Training heads of depth_type 'mixup_ce' and the regression types (models/mvsformer_model.py:126-146): softmax over the depth axis, the
// head's depth and confidence, and the backward through head + softmax - one launch forward, one backward.  One lane per pixel column over
// the flattened H*W plane (the heads have no spatial structure), reductions over d in registers: deterministic, no atomics.  DT > 0: the
// cascade's depth counts, every logit / hypothesis of the column requested before the first is consumed (as head_reg_kernel of head.hip);
// DT = 0: any D, the column re-read from memory per sweep.
#include "common.h"

namespace {

// A column of a [B,D,plane] tensor: registers (DT > 0) or memory (DT = 0)
template <int DT>
struct Column {
    float r[DT ? DT : 1];
    const float* p;
    size_t plane;
    __device__ __forceinline__ void load(const float* base, size_t pl) {
        p = base;
        plane = pl;
        if (DT) {
#pragma unroll
            for (int d = 0; d < DT; ++d) r[d] = base[(size_t)d * pl];
        }
    }
    __device__ __forceinline__ float operator[](int d) const { return DT ? r[DT ? d : 0] : p[(size_t)d * plane]; }
};

// softmax of the column `l` -> prob (written), returns nothing; the probabilities are re-read through `pcol` by the caller
template <int DT>
__device__ __forceinline__ void softmax_column(const Column<DT>& l, int D, float* __restrict__ prob, size_t plane, float* pr) {
    float m = -INFINITY;
#pragma unroll
    for (int d = 0; d < D; ++d) m = fmaxf(m, l[d]);
    float s = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) s += expf(l[d] - m);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float p = expf(l[d] - m) / s;
        prob[(size_t)d * plane] = p;
        if (DT) pr[DT ? d : 0] = p;
    }
}

// mvsformer_model.py:111,138,146: prob = softmax(pre), depth = sum_d prob*hyp, conf = max_d prob (conf may be NULL)
template <int DT>
__global__ __launch_bounds__(256) void reg_head_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ hyp, int Drt, size_t plane,
                                                           float* __restrict__ prob, float* __restrict__ depth, float* __restrict__ conf) {
    const int D = DT ? DT : Drt;
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (pix >= plane) return;
    const size_t base = b * D * plane + pix;
    Column<DT> l, h;
    l.load(pre + base, plane);
    h.load(hyp + base, plane);
    float pr[DT ? DT : 1];
    softmax_column<DT>(l, D, prob + base, plane, pr);
    float acc = 0.0f, pmax = -INFINITY;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float p = DT ? pr[DT ? d : 0] : prob[base + (size_t)d * plane];
        acc = acc + p * h[d];
        pmax = fmaxf(pmax, p);
    }
    depth[b * plane + pix] = acc;
    if (conf) conf[b * plane + pix] = pmax;
}

// g_d = dprob_d + extra_d -> dpre_d = prob_d * (g_d - sum_k prob_k g_k); `extra(d)` is the head's own path from ddepth to prob_d
template <int DT, class Extra>
__device__ __forceinline__ void softmax_bwd_column(const Column<DT>& p, const float* __restrict__ dprob, int D, size_t plane, Extra extra,
                                                   float* __restrict__ dpre) {
    float g[DT ? DT : 1];
    float dot = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float gd = (dprob ? dprob[(size_t)d * plane] : 0.0f) + extra(d);
        if (DT) g[DT ? d : 0] = gd;
        dot = fmaf(p[d], gd, dot);
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const float gd = DT ? g[DT ? d : 0] : (dprob ? dprob[(size_t)d * plane] : 0.0f) + extra(d);
        dpre[(size_t)d * plane] = p[d] * (gd - dot);
    }
}

template <int DT>
__global__ __launch_bounds__(256) void reg_head_bwd_kernel(const float* __restrict__ prob, const float* __restrict__ hyp,
                                                           const float* __restrict__ dprob, const float* __restrict__ ddepth, int Drt, size_t plane,
                                                           float* __restrict__ dpre) {
    const int D = DT ? DT : Drt;
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (pix >= plane) return;
    const size_t base = b * D * plane + pix;
    Column<DT> p, h;
    p.load(prob + base, plane);
    h.load(hyp + base, plane);
    const float dd = ddepth ? ddepth[b * plane + pix] : 0.0f;
    // the softmax backward does not see a constant added to every g_d: hypotheses relative to the column's first one keep the
    // hundreds of millimetres they share out of the cancellation g_d - sum_k prob_k g_k
    const float h0 = h[0];
    softmax_bwd_column<DT>(p, dprob ? dprob + base : nullptr, D, plane, [&](int d) { return dd * (h[d] - h0); }, dpre + base);
}

// The best adjacent pair of a probability column as mvs_mixup_head finds it (first maximum of p[d] + p[d+1]) and the pair's mixed depth
// (mvsformer_model.py:127-136: two divisions, two products, one sum)
struct MixPair { int idx; float best, norm, hl, hr, depth; };
template <int DT>
__device__ __forceinline__ MixPair mix_pair(const Column<DT>& p, const Column<DT>& h, int D) {
    float left = p[0], best = -1.0f, bl = 0.0f, br = 0.0f;
    int idx = 0;
#pragma unroll
    for (int d = 0; d + 1 < D; ++d) {
        const float right = p[d + 1];
        const float s = left + right;
        if (s > best) { best = s; idx = d; bl = left; br = right; }
        left = right;
    }
    MixPair r;
    r.idx = idx;
    r.best = best;
    r.norm = (bl + br) + 1e-7f;
    r.hl = h[DT ? 0 : idx];
    r.hr = h[DT ? 1 : idx + 1];
    if (DT) {                                                // registers: select, no dynamic index
#pragma unroll
        for (int d = 1; d + 1 < D; ++d) {
            r.hl = idx == d ? h[d] : r.hl;
            r.hr = idx == d ? h[d + 1] : r.hr;
        }
    }
    r.depth = r.hl * (bl / r.norm) + r.hr * (br / r.norm);
    return r;
}

template <int DT>
__global__ __launch_bounds__(256) void mixup_train_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ hyp, int Drt, size_t plane,
                                                              float* __restrict__ prob, float* __restrict__ depth, float* __restrict__ conf,
                                                              int* __restrict__ pair) {
    const int D = DT ? DT : Drt;
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (pix >= plane) return;
    const size_t base = b * D * plane + pix;
    Column<DT> l, h, p;
    l.load(pre + base, plane);
    h.load(hyp + base, plane);
    softmax_column<DT>(l, D, prob + base, plane, p.r);
    p.p = prob + base;                                       // DT = 0: this lane's own stores, read back in program order
    p.plane = plane;
    const MixPair m = mix_pair<DT>(p, h, D);
    depth[b * plane + pix] = m.depth;
    conf[b * plane + pix] = m.best;
    pair[b * plane + pix] = m.idx;
}

// ddepth reaches only prob[idx] and prob[idx+1]: with s = p_l + p_r + 1e-7, d(depth)/d(p_l) = (h_l - depth)/s, likewise for p_r
template <int DT>
__global__ __launch_bounds__(256) void mixup_train_bwd_kernel(const float* __restrict__ prob, const float* __restrict__ hyp, const int* __restrict__ pair,
                                                              const float* __restrict__ dprob, const float* __restrict__ ddepth, int Drt, size_t plane,
                                                              float* __restrict__ dpre) {
    const int D = DT ? DT : Drt;
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (pix >= plane) return;
    const size_t base = b * D * plane + pix;
    Column<DT> p, h;
    p.load(prob + base, plane);
    h.load(hyp + base, plane);
    int idx = pair[b * plane + pix];
    idx = idx < 0 ? 0 : (idx > D - 2 ? D - 2 : idx);        // the saved index is the forward's own; the clamp keeps a foreign one inside the column
    float pl = p[DT ? 0 : idx], pr = p[DT ? 1 : idx + 1], hl = h[DT ? 0 : idx], hr = h[DT ? 1 : idx + 1];
    if (DT) {                                                // registers: select, no dynamic index
#pragma unroll
        for (int d = 1; d + 1 < D; ++d) {
            pl = idx == d ? p[d] : pl;
            pr = idx == d ? p[d + 1] : pr;
            hl = idx == d ? h[d] : hl;
            hr = idx == d ? h[d + 1] : hr;
        }
    }
    const float norm = (pl + pr) + 1e-7f;
    const float dd = ddepth ? ddepth[b * plane + pix] : 0.0f;
    // (h_l - depth)/s with depth = (h_l p_l + h_r p_r)/s written out: h_l - depth = (1e-7 h_l - (h_r - h_l) p_r)/s, h_r - depth =
    // (1e-7 h_r + (h_r - h_l) p_l)/s.  The same value without the cancellation against a depth of hundreds of millimetres rounded to fp32
    // (which left 1e-5 of the gradient's scale where one of the pair holds nearly all of its probability).
    const float gap = hr - hl;
    const float gl = dd * (((1e-7f * hl - gap * pr) / norm) / norm), gr = dd * (((1e-7f * hr + gap * pl) / norm) / norm);
    softmax_bwd_column<DT>(p, dprob ? dprob + base : nullptr, D, plane,
                           [&](int d) { return d == idx ? gl : (d == idx + 1 ? gr : 0.0f); }, dpre + base);
}

bool head_train_shape_ok(int B, int D, int H, int W) { return B >= 1 && D >= 2 && H >= 1 && W >= 1 && B <= 65535; }

}  // namespace

// the register-resident form at the cascade's depth counts, the generic form otherwise
#define MVS_HEAD_TRAIN_LAUNCH(KERNEL, ...)                                                                      \
    do {                                                                                                        \
        const size_t plane = (size_t)H * W;                                                                     \
        dim3 grid((unsigned)((plane + 255) / 256), B), block(256);                                              \
        hipStream_t s = MVS_STREAM(stream);                                                                     \
        if (D == 4) hipLaunchKernelGGL(KERNEL<4>, grid, block, 0, s, __VA_ARGS__);                              \
        else if (D == 8) hipLaunchKernelGGL(KERNEL<8>, grid, block, 0, s, __VA_ARGS__);                         \
        else if (D == 16) hipLaunchKernelGGL(KERNEL<16>, grid, block, 0, s, __VA_ARGS__);                       \
        else if (D == 32) hipLaunchKernelGGL(KERNEL<32>, grid, block, 0, s, __VA_ARGS__);                       \
        else hipLaunchKernelGGL(KERNEL<0>, grid, block, 0, s, __VA_ARGS__);                                     \
    } while (0)

extern "C" int mvs_reg_head_fwd(const float* pre, const float* depth_values, int B, int D, int H, int W, float* prob_volume, float* depth,
                                float* conf, mvs_stream_t stream) {
    MVS_REQUIRE(pre && depth_values && prob_volume && depth, "mvs_reg_head_fwd: null pointer");
    MVS_REQUIRE(head_train_shape_ok(B, D, H, W), "mvs_reg_head_fwd: bad shape B=%d D=%d H=%d W=%d (needs D >= 2)", B, D, H, W);
    MVS_HEAD_TRAIN_LAUNCH(reg_head_fwd_kernel, pre, depth_values, D, plane, prob_volume, depth, conf);
    return mvs::finish_launch("mvs_reg_head_fwd");
}

extern "C" int mvs_reg_head_bwd(const float* prob_volume, const float* depth_values, const float* dprob, const float* ddepth, int B, int D,
                                int H, int W, float* dpre, mvs_stream_t stream) {
    MVS_REQUIRE(prob_volume && depth_values && dpre, "mvs_reg_head_bwd: null pointer");
    MVS_REQUIRE(head_train_shape_ok(B, D, H, W), "mvs_reg_head_bwd: bad shape B=%d D=%d H=%d W=%d (needs D >= 2)", B, D, H, W);
    MVS_HEAD_TRAIN_LAUNCH(reg_head_bwd_kernel, prob_volume, depth_values, dprob, ddepth, D, plane, dpre);
    return mvs::finish_launch("mvs_reg_head_bwd");
}

extern "C" int mvs_mixup_train_fwd(const float* pre, const float* depth_values, int B, int D, int H, int W, float* prob_volume, float* depth,
                                   float* conf, int* pair, mvs_stream_t stream) {
    MVS_REQUIRE(pre && depth_values && prob_volume && depth && conf && pair, "mvs_mixup_train_fwd: null pointer");
    MVS_REQUIRE(head_train_shape_ok(B, D, H, W), "mvs_mixup_train_fwd: bad shape B=%d D=%d H=%d W=%d (needs D >= 2)", B, D, H, W);
    MVS_HEAD_TRAIN_LAUNCH(mixup_train_fwd_kernel, pre, depth_values, D, plane, prob_volume, depth, conf, pair);
    return mvs::finish_launch("mvs_mixup_train_fwd");
}

extern "C" int mvs_mixup_train_bwd(const float* prob_volume, const float* depth_values, const int* pair, const float* dprob, const float* ddepth,
                                   int B, int D, int H, int W, float* dpre, mvs_stream_t stream) {
    MVS_REQUIRE(prob_volume && depth_values && pair && dpre, "mvs_mixup_train_bwd: null pointer");
    MVS_REQUIRE(head_train_shape_ok(B, D, H, W), "mvs_mixup_train_bwd: bad shape B=%d D=%d H=%d W=%d (needs D >= 2)", B, D, H, W);
    MVS_HEAD_TRAIN_LAUNCH(mixup_train_bwd_kernel, prob_volume, depth_values, pair, dprob, ddepth, D, plane, dpre);
    return mvs::finish_launch("mvs_mixup_train_bwd");
}
