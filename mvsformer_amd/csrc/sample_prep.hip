// Sample preparation between "decoded bytes" and the network's input tensors: the arithmetic of the reference's
// datasets/dtu_dataset_ms.py:173-247,296-367 (pre_resize, final_crop, the crop retry loop, generate_stage_depth, the projection matrices
// and depth_values), datasets/color_jittor.py:53-83 over PIL's ImageEnhance / HSV conversion, ToTensor / RandomGamma / Normalize
// (dtu_dataset_ms.py:18-37,341-349) and datasets/general_eval.py:108-128 (read_img's edge padding, scale_mvs_input).
//
// All kernels are one lane per output element, bandwidth-bound and integer-exact where the reference is.  Everything that changes per
// sample (resized sizes, offsets, candidate offsets, jitter order and factors) is read from small device tables, so no launch geometry
// depends on it and a captured graph replays with new tables.  Every source index is clamped into its image: a table with nonsense in it
// gives nonsense pixels, never an access outside a tensor.
#include "block_ops.h"

namespace {

constexpr int PREP_THREADS = 256;
constexpr int PT = MVS_PREP_VIEW_INTS, JT = MVS_PREP_JITTER_INTS;
constexpr int AREA_MAX_TAPS = 8;

// ---------------------------------------------------------------------------------------------------------------- tables
struct ViewGeom {
    int rw, rh, ox, oy;            // resized size, crop offset inside the resized image
};

__device__ __forceinline__ ViewGeom view_geom(const int32_t* __restrict__ ptab, const int32_t* __restrict__ chosen, int b, int v, int V,
                                               int H0, int W0, int h, int w) {
    const int32_t* p = ptab + ((size_t)b * V + v) * PT;
    ViewGeom g;
    g.rw = min(max(p[0], 1), W0);
    g.rh = min(max(p[1], 1), H0);
    const bool ref = p[4] != 0;
    g.ox = ref ? chosen[b * 4 + 1] : p[2];
    g.oy = ref ? chosen[b * 4 + 0] : p[3];
    g.ox = min(max(g.ox, 0), max(g.rw - w, 0));
    g.oy = min(max(g.oy, 0), max(g.rh - h, 0));
    return g;
}

// cv2.INTER_NEAREST: source index of destination index d, the product taken in double
__device__ __forceinline__ int nn_index(int d, int src, int dst) {
    const int s = (int)floor((double)d * ((double)src / (double)dst));
    return min(max(s, 0), src - 1);
}

// crop pixel (y, x) of the resized reference image -> index into the H0 x W0 source map
__device__ __forceinline__ size_t nn_source(const ViewGeom& g, int y, int x, int H0, int W0) {
    const int ry = min(g.oy + y, g.rh - 1), rx = min(g.ox + x, g.rw - 1);
    const int sy = g.rh == H0 ? ry : nn_index(ry, H0, g.rh);
    const int sx = g.rw == W0 ? rx : nn_index(rx, W0, g.rw);
    return (size_t)sy * W0 + sx;
}

// ---------------------------------------------------------------------------------------------------------------- crop acceptance
// One block per sample: the first of K candidate offsets whose stage-1 mask (nearest neighbour, h/8 x w/8 of the crop) has a positive
// pixel; the last one with accepted = 0 when none has.  require_positive = 0 (val / test): candidate 0 is taken as it is.
__global__ __launch_bounds__(PREP_THREADS) void prep_accept_kernel(const uint8_t* __restrict__ mask_raw, const int32_t* __restrict__ ptab,
                                                                   const int32_t* __restrict__ cand, int V, int H0, int W0, int h, int w, int K,
                                                                   int require_positive, int32_t* __restrict__ chosen) {
    const int b = blockIdx.x;
    const int32_t* p = ptab + (size_t)b * V * PT;
    ViewGeom g;
    g.rw = min(max(p[0], 1), W0);
    g.rh = min(max(p[1], 1), H0);
    const int h1 = h / 8, w1 = w / 8;
    const uint8_t* m = mask_raw + (size_t)b * H0 * W0;
    int pick = K - 1, ok = 0;
    for (int k = 0; k < K; ++k) {
        g.oy = min(max(cand[((size_t)b * K + k) * 2 + 0], 0), max(g.rh - h, 0));
        g.ox = min(max(cand[((size_t)b * K + k) * 2 + 1], 0), max(g.rw - w, 0));
        int any = 0;
        if (require_positive) {
            for (int i = threadIdx.x; i < h1 * w1; i += PREP_THREADS) {
                const int y = nn_index(i / w1, h, h1), x = nn_index(i % w1, w, w1);
                any |= m[nn_source(g, y, x, H0, W0)] > 10;
            }
            any = __syncthreads_or(any);                          // block-uniform: every lane leaves the loop together
        } else {
            any = 1;
        }
        if (any) {
            pick = k, ok = 1;
            break;
        }
    }
    if (threadIdx.x == 0) {
        chosen[b * 4 + 0] = min(max(cand[((size_t)b * K + pick) * 2 + 0], 0), max(g.rh - h, 0));
        chosen[b * 4 + 1] = min(max(cand[((size_t)b * K + pick) * 2 + 1], 0), max(g.rw - w, 0));
        chosen[b * 4 + 2] = ok;
        chosen[b * 4 + 3] = pick;
    }
}

// ---------------------------------------------------------------------------------------------------------------- ground-truth pyramid
// depth and mask of stages 4..1, each [B][hs][ws], stage s at pyr + B * (pixels of the stages before it).  Stage 4 is the crop of the
// nearest-neighbour resize; stages 3, 2, 1 are nearest-neighbour resizes OF that crop to (h/2, w/2), (h/4, w/4), (h/8, w/8).
__global__ __launch_bounds__(PREP_THREADS) void prep_pyramid_kernel(const float* __restrict__ depth_hr, const uint8_t* __restrict__ mask_raw,
                                                                    const int32_t* __restrict__ ptab, const int32_t* __restrict__ chosen, int B, int V,
                                                                    int H0, int W0, int h, int w, float* __restrict__ depth_pyr,
                                                                    float* __restrict__ mask_pyr) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * PREP_THREADS + threadIdx.x;
    long long base = 0, local = i;
    int hs = h, ws = w, found = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int hh = h >> s, ww = w >> s;
        const long long n = (long long)hh * ww;
        if (!found) {
            if (local < n) {
                hs = hh, ws = ww, found = 1;
            } else {
                local -= n;
                base += n * B;
            }
        }
    }
    if (!found) return;
    const int ys = (int)(local / ws), xs = (int)(local % ws);
    const int y = hs == h ? ys : nn_index(ys, h, hs), x = ws == w ? xs : nn_index(xs, w, ws);
    const ViewGeom g = view_geom(ptab, chosen, b, 0, V, H0, W0, h, w);
    const size_t src = (size_t)b * H0 * W0 + nn_source(g, y, x, H0, W0);
    const size_t dst = (size_t)base + (size_t)b * hs * ws + (size_t)local;
    depth_pyr[dst] = depth_hr[src];
    mask_pyr[dst] = mask_raw[src] > 10 ? 1.0f : 0.0f;
}

// projection matrices of the four stages [4][B][V][2][4][4] (stage 1 first) and depth_values [B][L]
__global__ __launch_bounds__(PREP_THREADS) void prep_proj_kernel(const float* __restrict__ intr, const float* __restrict__ extr,
                                                                 const double* __restrict__ drange, const int32_t* __restrict__ ptab,
                                                                 const int32_t* __restrict__ chosen, int B, int V, int H0, int W0, int h, int w, int L,
                                                                 float* __restrict__ proj, float* __restrict__ depth_values) {
    const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (i < B * V) {
        const int b = i / V, v = i % V;
        const ViewGeom g = view_geom(ptab, chosen, b, v, V, H0, W0, h, w);
        const int32_t* p = ptab + (size_t)i * PT;
        const float rs = __int_as_float(p[5]);
        float K[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) K[j] = intr[(size_t)i * 9 + j];
        if (p[6]) {                                               // pre_resize ran (resize_scale != 1.0): rows 0 and 1 in fp32
#pragma unroll
            for (int j = 0; j < 6; ++j) K[j] = K[j] * rs;
        }
        K[2] = K[2] - (float)g.ox;                                // final_crop
        K[5] = K[5] - (float)g.oy;
        const float mul[4] = {0.125f, 0.25f, 0.5f, 1.0f};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float* o = proj + ((size_t)s * B * V + i) * 32;
#pragma unroll
            for (int j = 0; j < 16; ++j) o[j] = extr[(size_t)i * 16 + j];
#pragma unroll
            for (int j = 0; j < 16; ++j) o[16 + j] = 0.0f;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) o[16 + r * 4 + c] = r < 2 && s < 3 ? K[r * 3 + c] * mul[s] : K[r * 3 + c];
        }
    }
    if (i < B * L) {
        // np.arange(start, stop, step, dtype=float32): the first two elements are start and start + step formed in double and rounded;
        // the rest is numpy's fill loop in the ARRAY's type: first + i * (second - first), fp32 throughout
        const int b = i / L, k = i % L;
        const double start = drange[b * 2 + 0], step = drange[b * 2 + 1];
        const float f0 = (float)start, f1 = (float)(start + step);
        const float delta = f1 - f0;
        depth_values[i] = k == 0 ? f0 : (k == 1 ? f1 : f0 + (float)k * delta);
    }
}

// ---------------------------------------------------------------------------------------------------------------- INTER_AREA + crop
// OpenCV's area table of one axis for destination index D: taps (source index, weight).  The cell is [D * scale, D * scale + scale)
// clipped to the source; weights are covered length / min(scale, ssize - D * scale), formed in double and rounded to fp32; a partial
// pixel narrower than 1e-3 is dropped, as computeResizeAreaTab drops it.
__device__ __forceinline__ int area_taps(int D, int ssize, double scale, int* first, float* wgt) {
    const double fsx1 = (double)D * scale, fsx2 = fsx1 + scale;
    const double cell = fmin(scale, (double)ssize - fsx1);
    int sx1 = (int)ceil(fsx1), sx2 = (int)floor(fsx2);
    sx2 = min(sx2, ssize - 1);
    sx1 = min(sx1, sx2);
    int n = 0;
    *first = sx1;
    if ((double)sx1 - fsx1 > 1e-3) {
        *first = sx1 - 1;
        wgt[n++] = (float)(((double)sx1 - fsx1) / cell);
    }
    for (int sx = sx1; sx < sx2 && n < AREA_MAX_TAPS - 1; ++sx) wgt[n++] = (float)(1.0 / cell);
    if (fsx2 - (double)sx2 > 1e-3 && n < AREA_MAX_TAPS) wgt[n++] = (float)(fmin(fmin(fsx2 - (double)sx2, 1.0), cell) / cell);
    return n;
}

__device__ __forceinline__ uint8_t round_sat_u8(float v) {
    const float r = rintf(v);                                     // to nearest, ties to even
    return (uint8_t)fminf(fmaxf(r, 0.0f), 255.0f);
}

__global__ __launch_bounds__(PREP_THREADS) void prep_area_crop_kernel(const uint8_t* __restrict__ imgs, const int32_t* __restrict__ ptab,
                                                                      const int32_t* __restrict__ chosen, int V, int H0, int W0, int h, int w,
                                                                      uint8_t* __restrict__ out) {
    const int bv = blockIdx.y, b = bv / V, v = bv % V;
    const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (i >= h * w) return;
    const int y = i / w, x = i % w;
    const ViewGeom g = view_geom(ptab, chosen, b, v, V, H0, W0, h, w);
    const int ry = min(g.oy + y, g.rh - 1), rx = min(g.ox + x, g.rw - 1);
    const uint8_t* src = imgs + (size_t)bv * H0 * W0 * 3;
    uint8_t* o = out + ((size_t)bv * h * w + i) * 3;
    if (g.rw == W0 && g.rh == H0) {                               // a scale of 1: a copy
        const uint8_t* s = src + ((size_t)ry * W0 + rx) * 3;
        o[0] = s[0], o[1] = s[1], o[2] = s[2];
        return;
    }
    if (W0 == 2 * g.rw && H0 == 2 * g.rh) {                       // exact 2:1: OpenCV's integer path
        const uint8_t* s0 = src + ((size_t)(2 * ry) * W0 + 2 * rx) * 3;
        const uint8_t* s1 = s0 + (size_t)W0 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (uint8_t)(((int)s0[c] + (int)s0[3 + c] + (int)s1[c] + (int)s1[3 + c] + 2) >> 2);
        return;
    }
    int x0, y0;
    float ax[AREA_MAX_TAPS], ay[AREA_MAX_TAPS];
    const int nx = area_taps(rx, W0, (double)W0 / (double)g.rw, &x0, ax);
    const int ny = area_taps(ry, H0, (double)H0 / (double)g.rh, &y0, ay);
    float sum[3] = {0.0f, 0.0f, 0.0f};
    for (int j = 0; j < ny; ++j) {
        const int sy = min(max(y0 + j, 0), H0 - 1);
        float buf[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < nx; ++k) {                            // horizontal pass first
            const int sx = min(max(x0 + k, 0), W0 - 1);
            const uint8_t* s = src + ((size_t)sy * W0 + sx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) buf[c] = buf[c] + (float)s[c] * ax[k];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = sum[c] + ay[j] * buf[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = round_sat_u8(sum[c]);
}

// ---------------------------------------------------------------------------------------------------------------- colour jitter (PIL)
struct Rgb {
    int r, g, b;
};

// Image.blend(degenerate, image, factor) of one channel: ImagingBlend's two branches, in C float arithmetic
__device__ __forceinline__ int pil_blend(int d, int s, float alpha) {
    const float t = (float)d + alpha * (float)(s - d);
    if (alpha >= 0.0f && alpha <= 1.0f) return (int)t & 0xff;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int pil_luma(const Rgb& p) { return (p.r * 19595 + p.g * 38470 + p.b * 7471 + 0x8000) >> 16; }

// convert('HSV'), h += shift (uint8 wrap-around), convert('RGB'): PIL's rgb2hsv_row / hsv2rgb, which follow colorsys in C float / double
__device__ __forceinline__ Rgb pil_hue(const Rgb& p, int shift) {
    const int maxc = max(p.r, max(p.g, p.b)), minc = min(p.r, min(p.g, p.b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = cr / (float)maxc;
        const float rc = (float)(maxc - p.r) / cr, gc = (float)(maxc - p.g) / cr, bc = (float)(maxc - p.b) / cr;
        float hh;
        if (p.r == maxc) hh = bc - gc;
        else if (p.g == maxc) hh = (float)(2.0 + (double)rc - (double)bc);
        else hh = (float)(4.0 + (double)gc - (double)rc);
        hh = (float)fmod((double)hh / 6.0 + 1.0, 1.0);
        uh = min(max((int)((double)hh * 255.0), 0), 255);
        us = min(max((int)((double)s * 255.0), 0), 255);
    }
    uh = (uh + shift) & 0xff;
    Rgb o;
    if (us == 0) {
        o.r = o.g = o.b = uv;
        return o;
    }
    const double h6 = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const float f = (float)(h6 - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const double vv = (double)(float)uv;
    const int pp = min(max((int)round(vv * (1.0 - (double)fs)), 0), 255);
    const int qq = min(max((int)round(vv * (1.0 - (double)fs * (double)f)), 0), 255);
    const int tt = min(max((int)round(vv * (1.0 - (double)fs * (1.0 - (double)f))), 0), 255);
    switch (i % 6) {
        case 0: o.r = uv, o.g = tt, o.b = pp; break;
        case 1: o.r = qq, o.g = uv, o.b = pp; break;
        case 2: o.r = pp, o.g = uv, o.b = tt; break;
        case 3: o.r = pp, o.g = qq, o.b = uv; break;
        case 4: o.r = tt, o.g = pp, o.b = uv; break;
        default: o.r = uv, o.g = pp, o.b = qq; break;
    }
    return o;
}

// the operations of jt in fn_idx order; stop_at_contrast: only those before contrast's turn (the image whose mean(L) contrast blends with)
__device__ __forceinline__ Rgb jitter_chain(Rgb p, const int32_t* __restrict__ jt, int grey, bool stop_at_contrast) {
    const int enable = jt[4];
    for (int k = 0; k < 4; ++k) {
        const int op = jt[k];
        if (op < 0 || op > 3 || !((enable >> op) & 1)) continue;
        if (op == 0) {
            const float a = __int_as_float(jt[8]);
            p.r = pil_blend(0, p.r, a), p.g = pil_blend(0, p.g, a), p.b = pil_blend(0, p.b, a);
        } else if (op == 1) {
            if (stop_at_contrast) return p;
            const float a = __int_as_float(jt[9]);
            p.r = pil_blend(grey, p.r, a), p.g = pil_blend(grey, p.g, a), p.b = pil_blend(grey, p.b, a);
        } else if (op == 2) {
            const float a = __int_as_float(jt[10]);
            const int l = pil_luma(p);
            p.r = pil_blend(l, p.r, a), p.g = pil_blend(l, p.g, a), p.b = pil_blend(l, p.b, a);
        } else {
            p = pil_hue(p, jt[6]);
        }
    }
    return p;
}

__global__ __launch_bounds__(PREP_THREADS) void prep_zero_kernel(unsigned long long* __restrict__ p, int n) {
    const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (i < n) p[i] = 0ull;
}

// first launch: sum of L, per image, of the image as it stands when contrast's turn comes (64-bit integer: exact and order-free)
__global__ __launch_bounds__(PREP_THREADS) void prep_jitter_stats_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ jtab, int V,
                                                                         int hw, unsigned long long* __restrict__ lsum) {
    __shared__ unsigned int sred[PREP_THREADS / 64];
    const int bv = blockIdx.y, b = bv / V;
    const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
    unsigned int l = 0;
    if (i < hw) {
        const uint8_t* s = img + ((size_t)bv * hw + i) * 3;
        Rgb p{s[0], s[1], s[2]};
        p = jitter_chain(p, jtab + (size_t)b * JT, 0, true);
        l = (unsigned int)pil_luma(p);
    }
    l = blk::block_sum(l, sred);
    if (threadIdx.x == 0) atomicAdd(lsum + bv, (unsigned long long)l);
}

// second launch: the whole chain, then ToTensor, RandomGamma (clip_image=True) and Normalize into NCHW fp32
__global__ __launch_bounds__(PREP_THREADS) void prep_jitter_tail_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ jtab, int V,
                                                                        int hw, const unsigned long long* __restrict__ lsum, int augment,
                                                                        float* __restrict__ out, uint8_t* __restrict__ out_u8) {
    const int bv = blockIdx.y, b = bv / V;
    const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (i >= hw) return;
    const uint8_t* s = img + ((size_t)bv * hw + i) * 3;
    Rgb p{s[0], s[1], s[2]};
    const int32_t* jt = jtab + (size_t)b * JT;
    bool gamma_on = false;
    float gamma = 1.0f;
    if (augment) {
        int grey = 0;
        if (lsum) grey = (int)((double)lsum[bv] / (double)hw + 0.5);          // int(ImageStat.Stat(L).mean[0] + 0.5)
        p = jitter_chain(p, jt, grey, false);
        gamma_on = jt[5] != 0;
        gamma = __int_as_float(jt[11]);
    }
    if (out_u8) {
        uint8_t* o = out_u8 + ((size_t)bv * hw + i) * 3;
        o[0] = (uint8_t)p.r, o[1] = (uint8_t)p.g, o[2] = (uint8_t)p.b;
    }
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const int c3[3] = {p.r, p.g, p.b};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = (float)c3[c] / 255.0f;
        if (gamma_on) t = fminf(fmaxf(powf(t, gamma), 0.0f), 1.0f);
        out[((size_t)bv * 3 + c) * hw + i] = (t - mean[c]) / stdv[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------- INTER_LINEAR (uint8)
// OpenCV's fixed-point bilinear resize of 8-bit images: coefficients round(w * 2048), horizontal pass in integers, vertical pass
// (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2.  pad rows of edge padding above and below the source (read_img's 'tt').
__device__ __forceinline__ void linear_coef(int d, double scale, int ssize, int* s0, int* a0, int* a1) {
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int sx = (int)floorf(fx);
    fx -= (float)sx;
    if (sx < 0) fx = 0.0f, sx = 0;
    if (sx >= ssize - 1) fx = 0.0f, sx = ssize - 1;
    *s0 = sx;
    *a0 = (int)rintf((1.0f - fx) * 2048.0f);
    *a1 = (int)rintf(fx * 2048.0f);
}

__global__ __launch_bounds__(PREP_THREADS) void prep_eval_resize_kernel(const uint8_t* __restrict__ src, int H0, int W0, int H, int W, int pad,
                                                                        uint8_t* __restrict__ out_u8, float* __restrict__ out) {
    const int v = blockIdx.y;
    const int i = blockIdx.x * PREP_THREADS + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i % W;
    const int Hp = H0 + 2 * pad;
    const uint8_t* img = src + (size_t)v * H0 * W0 * 3;
    int res[3];
    if (W0 == 2 * W && Hp == 2 * H) {                             // cv2.resize turns an exact 2:1 INTER_LINEAR into INTER_AREA
        const int ya = min(max(2 * y - pad, 0), H0 - 1), yb = min(max(2 * y + 1 - pad, 0), H0 - 1);
        const uint8_t* s0 = img + ((size_t)ya * W0 + 2 * x) * 3;
        const uint8_t* s1 = img + ((size_t)yb * W0 + 2 * x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) res[c] = ((int)s0[c] + (int)s0[3 + c] + (int)s1[c] + (int)s1[3 + c] + 2) >> 2;
    } else {
        int sx, ax0, ax1, sy, by0, by1;
        linear_coef(x, (double)W0 / (double)W, W0, &sx, &ax0, &ax1);
        linear_coef(y, (double)Hp / (double)H, Hp, &sy, &by0, &by1);
        const int sx1 = min(sx + 1, W0 - 1);
        const int ya = min(max(sy - pad, 0), H0 - 1), yb = min(max(min(sy + 1, Hp - 1) - pad, 0), H0 - 1);
        const uint8_t* r0 = img + (size_t)ya * W0 * 3;
        const uint8_t* r1 = img + (size_t)yb * W0 * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int h0 = (int)r0[sx * 3 + c] * ax0 + (int)r0[sx1 * 3 + c] * ax1;
            const int h1 = (int)r1[sx * 3 + c] * ax0 + (int)r1[sx1 * 3 + c] * ax1;
            res[c] = min(max((((by0 * (h0 >> 4)) >> 16) + ((by1 * (h1 >> 4)) >> 16) + 2) >> 2, 0), 255);
        }
    }
    if (out_u8) {
        uint8_t* o = out_u8 + ((size_t)v * H * W + i) * 3;
        o[0] = (uint8_t)res[0], o[1] = (uint8_t)res[1], o[2] = (uint8_t)res[2];
    }
    if (out) {
        const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
        for (int c = 0; c < 3; ++c) out[((size_t)v * 3 + c) * H * W + i] = ((float)res[c] / 255.0f - mean[c]) / stdv[c];
    }
}

bool prep_shape_ok(int B, int V, int H0, int W0, int h, int w) {
    return B >= 1 && V >= 1 && (long long)B * V <= 65535 && H0 >= 1 && W0 >= 1 && h >= 1 && w >= 1 && h <= H0 && w <= W0 &&
           (long long)H0 * W0 * 3 <= INT32_MAX;
}

}  // namespace

extern "C" int64_t mvs_prep_pyramid_floats(int B, int h, int w) {
    if (B < 1 || h < 8 || w < 8) return -1;
    int64_t n = 0;
    for (int s = 0; s < 4; ++s) n += (int64_t)(h >> s) * (w >> s);
    return n * B;
}

extern "C" int mvs_prep_accept(const uint8_t* mask_raw, const int32_t* ptab, const int32_t* cand, int B, int V, int H0, int W0, int h, int w, int K,
                               int require_positive, int32_t* chosen, mvs_stream_t stream) {
    MVS_REQUIRE(prep_shape_ok(B, V, H0, W0, h, w) && h >= 8 && w >= 8 && K >= 1, "mvs_prep_accept: bad shape B=%d V=%d %dx%d crop %dx%d K=%d", B, V,
                H0, W0, h, w, K);
    MVS_REQUIRE(mask_raw && ptab && cand && chosen, "mvs_prep_accept: null pointer");
    hipLaunchKernelGGL(prep_accept_kernel, dim3((unsigned)B), dim3(PREP_THREADS), 0, MVS_STREAM(stream), mask_raw, ptab, cand, V, H0, W0, h, w, K,
                       require_positive, chosen);
    return mvs::finish_launch("mvs_prep_accept");
}

extern "C" int mvs_prep_geometry(const float* depth_hr, const uint8_t* mask_raw, const int32_t* ptab, const int32_t* chosen, const float* intrinsics,
                                 const float* extrinsics, const double* depth_range, int B, int V, int H0, int W0, int h, int w, int L,
                                 float* depth_pyr, float* mask_pyr, float* proj, float* depth_values, mvs_stream_t stream) {
    MVS_REQUIRE(prep_shape_ok(B, V, H0, W0, h, w) && h >= 8 && w >= 8 && L >= 1 && (long long)B * L <= INT32_MAX,
                "mvs_prep_geometry: bad shape B=%d V=%d %dx%d crop %dx%d L=%d", B, V, H0, W0, h, w, L);
    MVS_REQUIRE(depth_hr && mask_raw && ptab && chosen && intrinsics && extrinsics && depth_range && depth_pyr && mask_pyr && proj && depth_values,
                "mvs_prep_geometry: null pointer");
    MVS_REQUIRE(((uintptr_t)depth_range & 7) == 0, "mvs_prep_geometry: depth_range must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    const long long per = mvs_prep_pyramid_floats(1, h, w);
    hipLaunchKernelGGL(prep_pyramid_kernel, dim3((unsigned)mvs::ceil_div(per, (long long)PREP_THREADS), (unsigned)B), dim3(PREP_THREADS), 0, s,
                       depth_hr, mask_raw, ptab, chosen, B, V, H0, W0, h, w, depth_pyr, mask_pyr);
    const int n = B * V > B * L ? B * V : B * L;
    hipLaunchKernelGGL(prep_proj_kernel, dim3((unsigned)mvs::ceil_div(n, PREP_THREADS)), dim3(PREP_THREADS), 0, s, intrinsics, extrinsics, depth_range,
                       ptab, chosen, B, V, H0, W0, h, w, L, proj, depth_values);
    return mvs::finish_launch("mvs_prep_geometry");
}

extern "C" int mvs_prep_area_crop(const uint8_t* imgs, const int32_t* ptab, const int32_t* chosen, int B, int V, int H0, int W0, int h, int w,
                                  uint8_t* out, mvs_stream_t stream) {
    MVS_REQUIRE(prep_shape_ok(B, V, H0, W0, h, w), "mvs_prep_area_crop: bad shape B=%d V=%d %dx%d crop %dx%d", B, V, H0, W0, h, w);
    MVS_REQUIRE(imgs && ptab && chosen && out, "mvs_prep_area_crop: null pointer");
    hipLaunchKernelGGL(prep_area_crop_kernel, dim3((unsigned)mvs::ceil_div(h * w, PREP_THREADS), (unsigned)(B * V)), dim3(PREP_THREADS), 0,
                       MVS_STREAM(stream), imgs, ptab, chosen, V, H0, W0, h, w, out);
    return mvs::finish_launch("mvs_prep_area_crop");
}

extern "C" int mvs_prep_jitter_tail(const uint8_t* img, const int32_t* jtab, int B, int V, int h, int w, int augment, int has_contrast,
                                    uint64_t* lsum, float* out, uint8_t* out_u8, mvs_stream_t stream) {
    MVS_REQUIRE(B >= 1 && V >= 1 && (long long)B * V <= 65535 && h >= 1 && w >= 1 && (long long)h * w * 3 <= INT32_MAX,
                "mvs_prep_jitter_tail: bad shape B=%d V=%d %dx%d", B, V, h, w);
    MVS_REQUIRE(img && out && (!augment || jtab) && (!(augment && has_contrast) || lsum), "mvs_prep_jitter_tail: null pointer");
    MVS_REQUIRE(((uintptr_t)lsum & 7) == 0, "mvs_prep_jitter_tail: lsum must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    const int hw = h * w;
    dim3 grid((unsigned)mvs::ceil_div(hw, PREP_THREADS), (unsigned)(B * V));
    unsigned long long* ls = augment && has_contrast ? reinterpret_cast<unsigned long long*>(lsum) : nullptr;
    if (ls) {
        hipLaunchKernelGGL(prep_zero_kernel, dim3((unsigned)mvs::ceil_div(B * V, PREP_THREADS)), dim3(PREP_THREADS), 0, s, ls, B * V);
        hipLaunchKernelGGL(prep_jitter_stats_kernel, grid, dim3(PREP_THREADS), 0, s, img, jtab, V, hw, ls);
    }
    hipLaunchKernelGGL(prep_jitter_tail_kernel, grid, dim3(PREP_THREADS), 0, s, img, jtab, V, hw, ls, augment, out, out_u8);
    return mvs::finish_launch("mvs_prep_jitter_tail");
}

extern "C" int mvs_prep_eval_resize(const uint8_t* src, int V, int H0, int W0, int H, int W, int pad_rows, uint8_t* out_u8, float* out,
                                    mvs_stream_t stream) {
    MVS_REQUIRE(V >= 1 && V <= 65535 && H0 >= 1 && W0 >= 1 && H >= 1 && W >= 1 && pad_rows >= 0 && pad_rows <= 64 &&
                    (long long)(H0 + 2 * pad_rows) * W0 * 3 <= INT32_MAX && (long long)H * W * 3 <= INT32_MAX,
                "mvs_prep_eval_resize: bad shape V=%d %dx%d -> %dx%d pad=%d", V, H0, W0, H, W, pad_rows);
    MVS_REQUIRE(src && (out_u8 || out), "mvs_prep_eval_resize: null pointer");
    hipLaunchKernelGGL(prep_eval_resize_kernel, dim3((unsigned)mvs::ceil_div(H * W, PREP_THREADS), (unsigned)V), dim3(PREP_THREADS), 0,
                       MVS_STREAM(stream), src, H0, W0, H, W, pad_rows, out_u8, out);
    return mvs::finish_launch("mvs_prep_eval_resize");
}
