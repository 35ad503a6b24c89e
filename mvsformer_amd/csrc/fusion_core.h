// Per-pixel arithmetic of the depth-map consistency filter, shared by the per-sample kernels of fusion.hip and the
// job-table ("scene") kernels of pointcloud.hip: both call the SAME functions, so a reference pixel filtered through
// either entry point gets bit-identical masks, averaged depth and fused point.
//
// Conventions kept from the reference (misc/fusion.py): pixel centres at +0.5 (get_pixel_grids), homogeneous divides by
// (w + 1e-9), warp coordinates normalized as x/width*2-1, clamped to [-1.1, 1.1], sampled with align_corners=True, zeros
// padding.
#pragma once
#include "common.h"

namespace {

struct ViewXf {            // per (reference, source) pair: 84 floats
    float r2s[16];         // E_src * inv(E_ref)
    float s2r[16];         // E_ref * inv(E_src)
    float Kr[9], Kri[9], Ks[9], Ksi[9];
    float Eri[16];         // inv(E_ref), for the fused world point
};

__device__ void inv4d(const double* A, double* inv) {
    double a[4][8];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { a[i][j] = A[i * 4 + j]; a[i][4 + j] = (i == j) ? 1.0 : 0.0; }
    for (int c = 0; c < 4; ++c) {
        int p = c;
        double best = fabs(a[c][c]);
        for (int r = c + 1; r < 4; ++r) if (fabs(a[r][c]) > best) { best = fabs(a[r][c]); p = r; }
        if (p != c) for (int j = 0; j < 8; ++j) { double t = a[c][j]; a[c][j] = a[p][j]; a[p][j] = t; }
        const double piv = 1.0 / a[c][c];
        for (int j = 0; j < 8; ++j) a[c][j] *= piv;
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = a[r][c];
            for (int j = 0; j < 8; ++j) a[r][j] -= f * a[c][j];
        }
    }
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) inv[i * 4 + j] = a[i][4 + j];
}

__device__ void inv3d(const float* K, float* out) {     // K is [4,4] row-major, upper-left 3x3 used
    double m[16] = {0}, mi[16];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) m[i * 4 + j] = K[i * 4 + j];
    m[15] = 1.0;
    inv4d(m, mi);
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) out[i * 3 + j] = (float)mi[i * 4 + j];
}

// camera algebra of one (reference, source) pair; rc, sc are [2,4,4] (E, K); fp64 inverses
__device__ void prep_view(const float* __restrict__ rc, const float* __restrict__ sc, ViewXf& o) {
    double Er[16], Es[16], Eri[16], Esi[16];
    for (int i = 0; i < 16; ++i) { Er[i] = rc[i]; Es[i] = sc[i]; }
    inv4d(Er, Eri);
    inv4d(Es, Esi);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double a = 0.0, b = 0.0;
            for (int k = 0; k < 4; ++k) { a += Es[i * 4 + k] * Eri[k * 4 + j]; b += Er[i * 4 + k] * Esi[k * 4 + j]; }
            o.r2s[i * 4 + j] = (float)a;
            o.s2r[i * 4 + j] = (float)b;
            o.Eri[i * 4 + j] = (float)Eri[i * 4 + j];
        }
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) { o.Kr[i * 3 + j] = rc[16 + i * 4 + j]; o.Ks[i * 3 + j] = sc[16 + i * 4 + j]; }
    inv3d(rc + 16, o.Kri);
    inv3d(sc + 16, o.Ksi);
}

struct V3 { float x, y, z; };

// 1/x: v_rcp_f32 (1 ulp) + one Newton step, ~0.5 ulp; shared by the three components of each homogeneous divide
// (the IEEE division sequence per component made the kernel VALU-bound: ~45 divides per pixel per view)
__device__ __forceinline__ float recip(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return fmaf(fmaf(-x, r, 1.0f), r, r);
}

// pixel (px,py) with depth d in camera A (Kinv) -> camera B coordinates (via M = E_B * inv(E_A)); homogeneous
// divides by (w + 1e-9) kept where the reference has them
__device__ __forceinline__ V3 pix_to_cam(const float* Kinv, const float* M, float px, float py, float d) {
    float cx = Kinv[0] * px + Kinv[1] * py + Kinv[2];
    float cy = Kinv[3] * px + Kinv[4] * py + Kinv[5];
    float cz = Kinv[6] * px + Kinv[7] * py + Kinv[8];
    const float sc = recip(cz + 1e-9f) * d;
    cx *= sc; cy *= sc; cz *= sc;
    float X = M[0] * cx + M[1] * cy + M[2] * cz + M[3];
    float Y = M[4] * cx + M[5] * cy + M[6] * cz + M[7];
    float Z = M[8] * cx + M[9] * cy + M[10] * cz + M[11];
    const float Wh = M[12] * cx + M[13] * cy + M[14] * cz + M[15];
    // idx_cam2world divides by (w+1e-9), idx_world2cam again: both are divisions by ~1
    const float w1 = recip(Wh + 1e-9f);
    X *= w1; Y *= w1; Z *= w1;
    return V3{X, Y, Z};
}

__device__ __forceinline__ V3 cam_to_img(const float* K, V3 c) {      // idx_cam2img: K * c, divided by (z + 1e-9)
    const float ix = K[0] * c.x + K[1] * c.y + K[2] * c.z;
    const float iy = K[3] * c.x + K[4] * c.y + K[5] * c.z;
    const float iz = K[6] * c.x + K[7] * c.y + K[8] * c.z;
    const float den = iz + 1e-9f, zz = recip(den);
    // quotient with one residual correction: correctly rounded in all but rare cases.  A prob-filtered (depth 0) source
    // pixel lands at |x| ~ 1e4 px where a 1-ulp quotient error is already 1e-3 px in the blended coordinate.
    float qx = ix * zz, qy = iy * zz;
    qx = fmaf(fmaf(-den, qx, ix), zz, qx);
    qy = fmaf(fmaf(-den, qy, iy), zz, qy);
    return V3{qx, qy, iz * zz};
}

// One source view of get_reproj (fusion.py:80-98) + vis_filter (fusion.py:101-109) for the reference pixel (px, py) with
// depth dref: the reprojected (x, y, depth), the in-range flag and the 0/1 consistency mask of this view.
struct GeoView { float rx, ry, rd, inr, m; };

__device__ __forceinline__ GeoView geo_view(const ViewXf& t, const float* __restrict__ sd, int H, int W, float px, float py, float dref,
                                            float dist_thresh, float depth_thresh) {
    // project_img(dst = reference): reference pixel -> source image coordinates
    const V3 cs = pix_to_cam(t.Kri, t.r2s, px, py, dref);
    const V3 q = cam_to_img(t.Ks, cs);
    float wx = q.x / (float)W * 2.0f - 1.0f, wy = q.y / (float)H * 2.0f - 1.0f;
    // clamp(-1.1, 1.1).  Non-finite depths: fmaxf / fminf return their other operand for a NaN, so a NaN coordinate (a NaN or infinite
    // reference depth) becomes -1.1 where torch.clamp keeps the NaN.  Either way the pixel is out of range and its mask is 0, which is the
    // contract: in_range = 0 and m = 0 for a non-finite reference depth, m = 0 for every pixel whose blend reads a non-finite source depth
    // (NaN compares false), pixels that read no such value are untouched.  The reprojected triple of an affected pixel is unspecified: here
    // it is the blend at the -1.1 corner (for W or H <= 20 that still reaches tap row / column 0), in the reference whatever grid_sample
    // makes of a NaN coordinate.  The tap index is bounds-checked below, so nothing is read outside the map in any case.
    wx = fminf(fmaxf(wx, -1.1f), 1.1f);
    wy = fminf(fmaxf(wy, -1.1f), 1.1f);
    GeoView o;
    o.inr = (-1.0f <= wx && wx <= 1.0f && -1.0f <= wy && wy <= 1.0f) ? 1.0f : 0.0f;
    // grid_sample(align_corners=True, zeros) of the source-grid image srcs2ref_xyd, evaluated tap by tap
    const float ix = ((wx + 1.0f) / 2.0f) * (float)(W - 1), iy = ((wy + 1.0f) / 2.0f) * (float)(H - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float fx1 = ix - x0f, fx0 = (x0f + 1.0f) - ix, fy1 = iy - y0f, fy0 = (y0f + 1.0f) - iy;   // ATen's tap weights
    float rx = 0.0f, ry = 0.0f, rd = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xs = x0f + (float)(k & 1), ys = y0f + (float)(k >> 1);
        const float wgt = ((k & 1) ? fx1 : fx0) * ((k >> 1) ? fy1 : fy0);
        if (xs >= 0.0f && xs <= (float)(W - 1) && ys >= 0.0f && ys <= (float)(H - 1)) {
            const float ds = sd[(size_t)ys * W + (size_t)xs];
            const V3 cr = pix_to_cam(t.Ksi, t.s2r, xs + 0.5f, ys + 0.5f, ds);
            const V3 im = cam_to_img(t.Kr, cr);
            rx = fmaf(im.x, wgt, rx);
            ry = fmaf(im.y, wgt, ry);
            rd = fmaf(cr.z, wgt, rd);
        }
    }
    o.rx = rx; o.ry = ry; o.rd = rd;
    // vis_filter
    const float ddx = rx - px, ddy = ry - py;
    const float distm = (sqrtf(ddx * ddx + ddy * ddy) < dist_thresh) ? 1.0f : 0.0f;
    const float depm = (fabsf(dref - rd) < fmaxf(dref, rd) * depth_thresh) ? 1.0f : 0.0f;
    o.m = fminf(o.inr, fminf(distm, depm));
    return o;
}

// idx_img2cam(pixel, ave, ref_cam) -> idx_cam2world(ref_cam): world = inv(E_ref) * cam   (test.py:432-434); t is any
// ViewXf of the reference view (Kri and Eri depend on the reference camera only)
__device__ __forceinline__ V3 fused_point(const ViewXf& t, float px, float py, float ave) {
    float cx = t.Kri[0] * px + t.Kri[1] * py + t.Kri[2], cy = t.Kri[3] * px + t.Kri[4] * py + t.Kri[5];
    float cz = t.Kri[6] * px + t.Kri[7] * py + t.Kri[8];
    const float sc = recip(cz + 1e-9f) * ave;
    cx *= sc; cy *= sc; cz *= sc;
    const float* M = t.Eri;
    const float wh = recip(M[12] * cx + M[13] * cy + M[14] * cz + M[15] + 1e-9f);
    return V3{(M[0] * cx + M[1] * cy + M[2] * cz + M[3]) * wh, (M[4] * cx + M[5] * cy + M[6] * cz + M[7]) * wh,
              (M[8] * cx + M[9] * cy + M[10] * cz + M[11]) * wh};
}

// ---------------------------------------------------------------------------------------------------------------
// Dynamic consistency (fusion.py:116-165 get_reproj_dynamic / vis_filter_dynamic, test.py:475-514): the reference pixel
// is projected into the source view, the SOURCE depth is sampled there (index = pixel coordinate, align_corners=True,
// no clamp), that sample is back-projected into the reference camera.  A view passes at level k in [2, v] when
// dist < k/dist_base and |d_ref - d|/d_ref < k/rel_diff_base; the pixel is kept if for some k at least k views pass.
// Thresholds grow with k, so a view is summarized by the first level it passes (kmin) and the [n,v,v-1,h,w] mask stack
// of the reference is only written on request.
constexpr int kMaxDynViews = 16;

__device__ __forceinline__ int first_level(float rx, float ry, float rd, float px, float py, float dref, int V, float dist_base,
                                           float rel_base) {
    const float ddx = rx - px, ddy = ry - py;
    const float cd = sqrtf(ddx * ddx + ddy * ddy);
    const float dd = fabsf(dref - rd) / dref;
    int kmin = V + 1;
    for (int k = V; k >= 2; --k) {
        const bool ok = (cd < (float)k / dist_base) && (dd < (float)k / rel_base);
        kmin = ok ? k : kmin;
    }
    return kmin;
}

struct DynAcc {
    int cnt[kMaxDynViews + 1];
    float msum, dsum;
    __device__ void init() {
#pragma unroll
        for (int k = 0; k <= kMaxDynViews; ++k) cnt[k] = 0;
        msum = 0.0f;
        dsum = 0.0f;
    }
    __device__ void add(int kmin, float rd, int V) {
#pragma unroll
        for (int k = 2; k <= kMaxDynViews; ++k) cnt[k] += (k >= kmin) ? 1 : 0;
        if (kmin <= V) { msum += 1.0f; dsum += rd; }
    }
    __device__ bool keep(int V) const {
        bool g = false;
#pragma unroll
        for (int k = 2; k <= kMaxDynViews; ++k) g = g || (k <= V && cnt[k] >= k);
        return g;
    }
};

// One source view of get_reproj_dynamic for the reference pixel (px, py) with depth dref -> (x, y) in the reference image
// and the depth in the reference camera of the source sample.
__device__ __forceinline__ V3 dyn_view(const ViewXf& t, const float* __restrict__ sd, int H, int W, float px, float py, float dref) {
    const float hx = (float)(W - 1) / 2.0f, hy = (float)(H - 1) / 2.0f;
    const V3 q = cam_to_img(t.Ks, pix_to_cam(t.Kri, t.r2s, px, py, dref));
    // grid = q/((w-1)/2) - 1, unnormalized by ATen as ((g+1)/2)*(w-1): the sample index is q itself (up to rounding)
    const float ix = ((q.x / hx - 1.0f + 1.0f) / 2.0f) * (float)(W - 1), iy = ((q.y / hy - 1.0f + 1.0f) / 2.0f) * (float)(H - 1);
    const float x0f = floorf(ix), y0f = floorf(iy);
    const float fx1 = ix - x0f, fx0 = (x0f + 1.0f) - ix, fy1 = iy - y0f, fy0 = (y0f + 1.0f) - iy;
    float ds = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float xs = x0f + (float)(k & 1), ys = y0f + (float)(k >> 1);
        if (xs >= 0.0f && xs <= (float)(W - 1) && ys >= 0.0f && ys <= (float)(H - 1))
            ds = fmaf(sd[(size_t)ys * W + (size_t)xs], ((k & 1) ? fx1 : fx0) * ((k >> 1) ? fy1 : fy0), ds);
    }
    const V3 cr = pix_to_cam(t.Ksi, t.s2r, q.x, q.y, ds);
    const V3 im = cam_to_img(t.Kr, cr);
    return V3{im.x, im.y, cr.z};
}

// ---------------------------------------------------------------------------------------------------------------
// The filter kernels, written once over a view-addressing policy `Views`: which reference and source maps a grid row
// (blockIdx.z) filters, where their ViewXf sit, and whether per-view outputs exist.
//   SampleViews (fusion.hip):   row n = sample n, views = rows n*V + v of src_depth / xf / the cameras [n,2,4,4], [n,v,2,4,4];
//                               per-view outputs of the dynamic filter on request (the per-sample geo filter: see fusion.hip).
//   JobViews (pointcloud.hip):  row r = job (ref_idx[r]; src_idx[r, 0..n_src[r])) into stacks of Nv maps and cameras; a row
//                               whose table entries are inconsistent writes "nothing kept"; no per-view outputs.
struct SampleViews {
    static constexpr bool kChecked = false, kPerView = true;
    int V;
    float* reproj /*[n,v,3,h,w]*/;
    uint8_t *level_masks /*[n,v,v-1,h,w]*/, *vis /*[n,v,h,w]*/;
    __device__ int count(int, int) const { return V; }
    __device__ int ref(int n) const { return n; }
    __device__ int slot(int n, int v) const { return n * V + v; }         // the pair's ViewXf
    __device__ int src(int n, int v) const { return n * V + v; }          // the pair's source map
    __device__ bool cams(int idx, const float* ref_cam, const float* src_cam, const float*& rc, const float*& sc) const {
        rc = ref_cam + (size_t)(idx / V) * 32;
        sc = src_cam + (size_t)idx * 32;
        return true;
    }
};

struct JobViews {
    static constexpr bool kChecked = true, kPerView = false;
    int Nv;
    const int32_t *ref_idx /*[R]*/, *src_idx /*[R,Vmax]*/, *n_src /*[R]*/;
    int Vmax;
    // a job's source count as the kernels use it; 0 = the job table is inconsistent and the job writes "nothing kept"
    __device__ int count(int r, int vmin) const {
        const int V = n_src[r];
        if ((unsigned)ref_idx[r] >= (unsigned)Nv || V < vmin || V > Vmax) return 0;
        for (int v = 0; v < V; ++v)
            if ((unsigned)src_idx[r * Vmax + v] >= (unsigned)Nv) return 0;
        return V;
    }
    __device__ int ref(int r) const { return ref_idx[r]; }
    __device__ int slot(int r, int v) const { return r * Vmax + v; }
    __device__ int src(int r, int v) const { return src_idx[r * Vmax + v]; }
    __device__ bool cams(int idx, const float* ref_cam, const float* src_cam, const float*& rc, const float*& sc) const {
        const int r = idx / Vmax, v = idx % Vmax;
        const int ref = ref_idx[r], s = src_idx[idx];
        if (v >= n_src[r] || (unsigned)ref >= (unsigned)Nv || (unsigned)s >= (unsigned)Nv) return false;      // padding (-1) or a bad entry
        rc = ref_cam + (size_t)ref * 32;
        sc = src_cam + (size_t)s * 32;
        return true;
    }
};

// the end of every filter kernel: keep mask, averaged depth and (points_out != null: t = the row's first ViewXf) the fused point of row n
__device__ __forceinline__ void write_fused(uint8_t* mask_out, float* ave_out, float* points_out, size_t n, size_t HW, size_t pix, bool keep,
                                            float ave, const ViewXf* t, float px, float py) {
    if (mask_out) mask_out[n * HW + pix] = keep ? 1 : 0;
    if (ave_out) ave_out[n * HW + pix] = ave;
    if (points_out) {
        const V3 p = fused_point(*t, px, py, ave);
        points_out[(n * 3 + 0) * HW + pix] = p.x;
        points_out[(n * 3 + 1) * HW + pix] = p.y;
        points_out[(n * 3 + 2) * HW + pix] = p.z;
    }
}

// a row whose job table is inconsistent: nothing kept
__device__ __forceinline__ void write_nothing(uint8_t* mask_out, float* ave_out, float* points_out, size_t n, size_t HW, size_t pix) {
    if (mask_out) mask_out[n * HW + pix] = 0;
    if (ave_out) ave_out[n * HW + pix] = 0.0f;
    if (points_out)
        for (int c = 0; c < 3; ++c) points_out[(n * 3 + c) * HW + pix] = 0.0f;
}

// the per-level masks of one view of the dynamic filter (level k passes iff k >= kmin) and its "some level passes" flag
__device__ __forceinline__ void write_levels(uint8_t* masks_out, uint8_t* vis_out, size_t nv, size_t HW, size_t pix, int kmin, int V) {
    if (masks_out)
        for (int k = 2; k <= V; ++k) masks_out[(nv * (V - 1) + (k - 2)) * HW + pix] = (k >= kmin) ? 1 : 0;
    if (vis_out) vis_out[nv * HW + pix] = (kmin <= V) ? 1 : 0;
}

// camera algebra, one thread per (row, view) slot
template <class Views>
__global__ void prep_kernel(Views vw, const float* __restrict__ ref_cam, const float* __restrict__ src_cam, int slots, ViewXf* __restrict__ xf) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= slots) return;
    const float *rc, *sc;
    if (vw.cams(idx, ref_cam, src_cam, rc, sc)) prep_view(rc, sc, xf[idx]);
}

template <class Views>
__global__ __launch_bounds__(256) void geo_filter_kernel(Views vw, const float* __restrict__ ref_depth, const float* __restrict__ src_depth,
                                                         const ViewXf* __restrict__ xf, int H, int W, float dist_thresh, float depth_thresh,
                                                         float vthresh, uint8_t* __restrict__ mask_out, float* __restrict__ ave_out,
                                                         float* __restrict__ points_out /*[rows,3,h,w]*/) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
    if (x >= W || y >= H) return;
    const size_t HW = (size_t)H * W, pix = (size_t)y * W + x;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const int V = vw.count(n, 1);
    if constexpr (Views::kChecked)
        if (V == 0) { write_nothing(mask_out, ave_out, points_out, n, HW, pix); return; }
    const float dref = ref_depth[(size_t)vw.ref(n) * HW + pix];
    float msum = 0.0f, dsum = 0.0f;
    for (int v = 0; v < V; ++v) {
        const GeoView g = geo_view(xf[vw.slot(n, v)], src_depth + (size_t)vw.src(n, v) * HW, H, W, px, py, dref, dist_thresh, depth_thresh);
        msum += g.m;
        dsum += g.rd * g.m;
    }
    write_fused(mask_out, ave_out, points_out, n, HW, pix, msum >= vthresh - 1.1f, (dsum + dref) / (msum + 1.0f), &xf[vw.slot(n, 0)], px, py);
}

template <class Views>
__global__ __launch_bounds__(256) void geo_filter_dynamic_kernel(const float* __restrict__ ref_depth, const float* __restrict__ src_depth,
                                                                 Views vw, const ViewXf* __restrict__ xf, int H, int W, float dist_base,
                                                                 float rel_base, uint8_t* __restrict__ geo_out, float* __restrict__ ave_out,
                                                                 float* __restrict__ points_out) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
    if (x >= W || y >= H) return;
    const size_t HW = (size_t)H * W, pix = (size_t)y * W + x;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const int V = vw.count(n, 2);                                            // a job's dy_range = n_src[r] + 1 (test.py:485)
    if constexpr (Views::kChecked)
        if (V == 0) { write_nothing(geo_out, ave_out, points_out, n, HW, pix); return; }
    const float dref = ref_depth[(size_t)vw.ref(n) * HW + pix];
    DynAcc acc;
    acc.init();
    for (int v = 0; v < V; ++v) {
        const V3 r = dyn_view(xf[vw.slot(n, v)], src_depth + (size_t)vw.src(n, v) * HW, H, W, px, py, dref);
        const int kmin = first_level(r.x, r.y, r.z, px, py, dref, V, dist_base, rel_base);
        if constexpr (Views::kPerView) {
            if (vw.reproj) {
                const size_t o3 = ((size_t)vw.src(n, v) * 3) * HW + pix;
                vw.reproj[o3] = r.x; vw.reproj[o3 + HW] = r.y; vw.reproj[o3 + 2 * HW] = r.z;
            }
            write_levels(vw.level_masks, vw.vis, (size_t)vw.src(n, v), HW, pix, kmin, V);
        }
        acc.add(kmin, r.z, V);
    }
    write_fused(geo_out, ave_out, points_out, n, HW, pix, acc.keep(V), (acc.dsum + dref) / (acc.msum + 1.0f), &xf[vw.slot(n, 0)], px, py);
}

}  // namespace
