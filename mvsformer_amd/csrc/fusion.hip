// Depth-map geometric consistency filtering — SURVEY.md §8(f2), the step right after the path: reference
// misc/fusion.py:79-122 (get_reproj -> project_img, vis_filter, ave_fusion) as used by test.py:404-438 (filter_depth).
//
// The reference materializes, per source view, a 3-channel "src pixel -> (x_ref, y_ref, depth_ref)" image, then warps it
// into the reference view with grid_sample, through ~20 [n,h,w,4,1] temporaries and 6 batched 4x4 inverses.  Here one
// lane owns one reference pixel and walks the source views: reference pixel -> source image (with the reference depth),
// the 4 bilinear taps there are back-projected on the fly with THEIR source depths into the reference camera, blended,
// compared against the pixel itself; masks, the averaged depth and the fused 3-D point fall out of the same pass.
// Traffic: (V+1) depth maps read (taps hit L1/L2), outputs written once.  Camera algebra is hoisted into a prep kernel
// (fp64 inverses, one thread per view).
//
// Conventions kept from the reference: pixel centres at +0.5 (get_pixel_grids), homogeneous divides by (w + 1e-9),
// warp coordinates normalized as x/width*2-1, clamped to [-1.1, 1.1], sampled with align_corners=True, zeros padding.
// The per-pixel arithmetic lives in fusion_core.h, shared with the job-table kernels of pointcloud.hip.
#include "fusion_core.h"

namespace {

// prep_kernel / geo_filter_dynamic_kernel: the templates of fusion_core.h over SampleViews.  The per-sample geo filter keeps its own body:
// as an instance of geo_filter_kernel<> it gives the same bits but spills 3 SGPRs where this form spills 1 (it sits at the SGPR limit).
__global__ __launch_bounds__(256) void geo_filter_sample_kernel(const float* __restrict__ ref_depth, const float* __restrict__ src_depth,
                                                         const float* __restrict__ ref_cam, const ViewXf* __restrict__ xf, int V, int H,
                                                         int W, float dist_thresh, float depth_thresh, float vthresh,
                                                         float* __restrict__ reproj /*[n,v,3,h,w]*/, float* __restrict__ in_range_out,
                                                         float* __restrict__ masks_out /*[n,v,h,w]*/, uint8_t* __restrict__ mask_out,
                                                         float* __restrict__ ave_out, float* __restrict__ points_out /*[n,3,h,w]*/) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, n = blockIdx.z;
    if (x >= W || y >= H) return;
    const size_t HW = (size_t)H * W, pix = (size_t)y * W + x;
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    const float dref = ref_depth[(size_t)n * HW + pix];
    float msum = 0.0f, dsum = 0.0f;
    for (int v = 0; v < V; ++v) {
        const GeoView g = geo_view(xf[n * V + v], src_depth + (size_t)(n * V + v) * HW, H, W, px, py, dref, dist_thresh, depth_thresh);
        const size_t o3 = ((size_t)(n * V + v) * 3) * HW + pix;
        if (reproj) { reproj[o3] = g.rx; reproj[o3 + HW] = g.ry; reproj[o3 + 2 * HW] = g.rd; }
        if (in_range_out) in_range_out[(size_t)(n * V + v) * HW + pix] = g.inr;
        if (masks_out) masks_out[(size_t)(n * V + v) * HW + pix] = g.m;
        msum += g.m;
        dsum += g.rd * g.m;
    }
    const float ave = (dsum + dref) / (msum + 1.0f);
    if (mask_out) mask_out[(size_t)n * HW + pix] = (msum >= vthresh - 1.1f) ? 1 : 0;
    if (ave_out) ave_out[(size_t)n * HW + pix] = ave;
    if (points_out) {
        const V3 p = fused_point(xf[n * V], px, py, ave);
        points_out[((size_t)n * 3 + 0) * HW + pix] = p.x;
        points_out[((size_t)n * 3 + 1) * HW + pix] = p.y;
        points_out[((size_t)n * 3 + 2) * HW + pix] = p.z;
    }
}

// vis_filter (+ ave_fusion) on an already materialized reproj_xyd — the op-level form of fusion.py:101-114.
// masks_in != null: use them (ave_fusion alone); else compute them from in_range and the two thresholds.
__global__ __launch_bounds__(256) void vis_filter_kernel(const float* __restrict__ ref_depth, const float* __restrict__ reproj,
                                                         const float* __restrict__ in_range, const float* __restrict__ masks_in, int V,
                                                         int H, int W, float dist_thresh, float depth_thresh, float vthresh,
                                                         float* __restrict__ masks_out, uint8_t* __restrict__ mask_out,
                                                         float* __restrict__ ave_out) {
    const size_t HW = (size_t)H * W;
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (pix >= HW) return;
    const float px = (float)(pix % W) + 0.5f, py = (float)(pix / W) + 0.5f;
    const float dref = ref_depth[(size_t)n * HW + pix];
    float msum = 0.0f, dsum = 0.0f;
    for (int v = 0; v < V; ++v) {
        const size_t o1 = (size_t)(n * V + v) * HW + pix, o3 = (size_t)(n * V + v) * 3 * HW + pix;
        const float rd = reproj[o3 + 2 * HW];
        float m;
        if (masks_in) {
            m = masks_in[o1];
        } else {
            const float ddx = reproj[o3] - px, ddy = reproj[o3 + HW] - py;
            const float distm = (sqrtf(ddx * ddx + ddy * ddy) < dist_thresh) ? 1.0f : 0.0f;
            const float depm = (fabsf(dref - rd) < fmaxf(dref, rd) * depth_thresh) ? 1.0f : 0.0f;
            m = fminf(in_range[o1], fminf(distm, depm));
        }
        if (masks_out) masks_out[o1] = m;
        msum += m;
        dsum += rd * m;
    }
    write_fused(mask_out, ave_out, nullptr, n, HW, pix, msum >= vthresh - 1.1f, (dsum + dref) / (msum + 1.0f), nullptr, px, py);
}

// ---------------------------------------------------------------------------------------------------------------
// Dynamic consistency (fusion.py:116-165, test.py:475-514); first_level / DynAcc / dyn_view are in fusion_core.h.
// op-level vis_filter_dynamic (fusion.py:153-165) on a materialized reproj_xyd, plus the reduction of test.py:503-511
__global__ __launch_bounds__(256) void vis_filter_dynamic_kernel(const float* __restrict__ ref_depth, const float* __restrict__ reproj, int V,
                                                                 int H, int W, float dist_base, float rel_base,
                                                                 uint8_t* __restrict__ masks_out, uint8_t* __restrict__ vis_out,
                                                                 uint8_t* __restrict__ geo_out, float* __restrict__ ave_out) {
    const size_t HW = (size_t)H * W;
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (pix >= HW) return;
    const float px = (float)(pix % W) + 0.5f, py = (float)(pix / W) + 0.5f;
    const float dref = ref_depth[(size_t)n * HW + pix];
    DynAcc acc;
    acc.init();
    for (int v = 0; v < V; ++v) {
        const size_t o3 = (size_t)(n * V + v) * 3 * HW + pix;
        const float rd = reproj[o3 + 2 * HW];
        const int kmin = first_level(reproj[o3], reproj[o3 + HW], rd, px, py, dref, V, dist_base, rel_base);
        write_levels(masks_out, vis_out, (size_t)(n * V + v), HW, pix, kmin, V);
        acc.add(kmin, rd, V);
    }
    write_fused(geo_out, ave_out, nullptr, n, HW, pix, acc.keep(V), (acc.dsum + dref) / (acc.msum + 1.0f), nullptr, px, py);
}

// prob_filter, fusion.py:69-77: AND over the C confidence channels of (conf[:, i] > thresh[i]); optionally zeroes a
// depth map in place where the test fails (test.py:414-418, `src_depths[:, ids] *= mask`).
__global__ __launch_bounds__(256) void prob_filter_kernel(const float* __restrict__ conf, int C, size_t HW, float t0, float t1, float t2,
                                                          float t3, uint8_t* __restrict__ mask, float* __restrict__ depth) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int n = blockIdx.y;
    if (pix >= HW) return;
    const float th[4] = {t0, t1, t2, t3};
    bool keep = true;
    for (int c = 0; c < C; ++c) keep = keep && (conf[((size_t)n * C + c) * HW + pix] > th[c]);
    if (mask) mask[(size_t)n * HW + pix] = keep ? 1 : 0;
    if (depth) depth[(size_t)n * HW + pix] *= keep ? 1.0f : 0.0f;
}

}  // namespace

extern "C" int mvs_vis_filter_fwd(const float* ref_depth, const float* reproj_xyd, const float* in_range, const float* masks_in, int n,
                                  int v, int H, int W, float img_dist_thresh, float depth_thresh, float vthresh, float* masks,
                                  uint8_t* mask, float* ref_depth_ave, mvs_stream_t stream) {
    MVS_REQUIRE(ref_depth && reproj_xyd && (in_range || masks_in), "mvs_vis_filter_fwd: null pointer");
    MVS_REQUIRE(n >= 1 && n <= 65535 && v >= 1 && H >= 1 && W >= 1, "mvs_vis_filter_fwd: bad shape n=%d v=%d H=%d W=%d", n, v, H, W);
    dim3 grid((unsigned)mvs::ceil_div((long long)H * W, 256LL), n);
    hipLaunchKernelGGL(vis_filter_kernel, grid, dim3(256), 0, MVS_STREAM(stream), ref_depth, reproj_xyd, in_range, masks_in, v, H, W,
                       img_dist_thresh, depth_thresh, vthresh, masks, mask, ref_depth_ave);
    return mvs::finish_launch("mvs_vis_filter_fwd");
}

extern "C" int mvs_prob_filter(const float* conf, int n, int C, int64_t HW, const float* thresh_host, uint8_t* mask, float* depth_inplace,
                               mvs_stream_t stream) {
    MVS_REQUIRE(conf && thresh_host && (mask || depth_inplace), "mvs_prob_filter: null pointer");
    MVS_REQUIRE(n >= 1 && n <= 65535 && C >= 1 && C <= 4 && HW >= 1, "mvs_prob_filter: bad shape n=%d C=%d HW=%lld", n, C, (long long)HW);
    float t[4] = {0, 0, 0, 0};
    for (int c = 0; c < C; ++c) t[c] = thresh_host[c];
    dim3 grid((unsigned)mvs::ceil_div((long long)HW, 256LL), n);
    hipLaunchKernelGGL(prob_filter_kernel, grid, dim3(256), 0, MVS_STREAM(stream), conf, C, (size_t)HW, t[0], t[1], t[2], t[3], mask,
                       depth_inplace);
    return mvs::finish_launch("mvs_prob_filter");
}

extern "C" int mvs_geo_filter_dynamic_fwd(const float* ref_depth, const float* src_depths, const float* ref_cam, const float* src_cams,
                                          int n, int v, int H, int W, float dist_base, float rel_diff_base, void* workspace,
                                          float* reproj_xyd, uint8_t* masks, uint8_t* vis_mask, uint8_t* geo_mask, float* ref_depth_ave,
                                          float* points, mvs_stream_t stream) {
    MVS_REQUIRE(ref_depth && src_depths && ref_cam && src_cams && workspace, "mvs_geo_filter_dynamic_fwd: null pointer");
    MVS_REQUIRE(n >= 1 && n <= 65535 && v >= 2 && v <= kMaxDynViews && H >= 2 && W >= 2,
                "mvs_geo_filter_dynamic_fwd: bad shape n=%d v=%d (2..%d) H=%d W=%d", n, v, kMaxDynViews, H, W);
    MVS_REQUIRE(dist_base > 0.0f && rel_diff_base > 0.0f, "mvs_geo_filter_dynamic_fwd: bases must be positive");
    hipStream_t s = MVS_STREAM(stream);
    ViewXf* xf = reinterpret_cast<ViewXf*>(workspace);
    const SampleViews vw{v, reproj_xyd, masks, vis_mask};
    hipLaunchKernelGGL(prep_kernel<SampleViews>, dim3(mvs::ceil_div(n * v, 64)), dim3(64), 0, s, vw, ref_cam, src_cams, n * v, xf);
    dim3 grid(mvs::ceil_div(W, 64), mvs::ceil_div(H, 4), n), block(64, 4);
    hipLaunchKernelGGL(geo_filter_dynamic_kernel<SampleViews>, grid, block, 0, s, ref_depth, src_depths, vw, xf, H, W, dist_base,
                       rel_diff_base, geo_mask, ref_depth_ave, points);
    return mvs::finish_launch("mvs_geo_filter_dynamic_fwd");
}

extern "C" int mvs_vis_filter_dynamic_fwd(const float* ref_depth, const float* reproj_xyd, int n, int v, int H, int W, float dist_base,
                                          float rel_diff_base, uint8_t* masks, uint8_t* vis_mask, uint8_t* geo_mask, float* ref_depth_ave,
                                          mvs_stream_t stream) {
    MVS_REQUIRE(ref_depth && reproj_xyd, "mvs_vis_filter_dynamic_fwd: null pointer");
    MVS_REQUIRE(n >= 1 && n <= 65535 && v >= 2 && v <= kMaxDynViews && H >= 1 && W >= 1,
                "mvs_vis_filter_dynamic_fwd: bad shape n=%d v=%d (2..%d) H=%d W=%d", n, v, kMaxDynViews, H, W);
    MVS_REQUIRE(dist_base > 0.0f && rel_diff_base > 0.0f, "mvs_vis_filter_dynamic_fwd: bases must be positive");
    dim3 grid((unsigned)mvs::ceil_div((long long)H * W, 256LL), n);
    hipLaunchKernelGGL(vis_filter_dynamic_kernel, grid, dim3(256), 0, MVS_STREAM(stream), ref_depth, reproj_xyd, v, H, W, dist_base,
                       rel_diff_base, masks, vis_mask, geo_mask, ref_depth_ave);
    return mvs::finish_launch("mvs_vis_filter_dynamic_fwd");
}

extern "C" int64_t mvs_geo_filter_workspace_bytes(int n, int v) { return (int64_t)n * v * (int64_t)sizeof(ViewXf); }

extern "C" int mvs_geo_filter_fwd(const float* ref_depth, const float* src_depths, const float* ref_cam, const float* src_cams, int n,
                                  int v, int H, int W, float img_dist_thresh, float depth_thresh, float vthresh, void* workspace,
                                  float* reproj_xyd, float* in_range, float* masks, uint8_t* mask, float* ref_depth_ave, float* points,
                                  mvs_stream_t stream) {
    MVS_REQUIRE(ref_depth && src_depths && ref_cam && src_cams && workspace, "mvs_geo_filter_fwd: null pointer");
    MVS_REQUIRE(n >= 1 && n <= 65535 && v >= 1 && H >= 2 && W >= 2, "mvs_geo_filter_fwd: bad shape n=%d v=%d H=%d W=%d", n, v, H, W);
    hipStream_t s = MVS_STREAM(stream);
    ViewXf* xf = reinterpret_cast<ViewXf*>(workspace);
    hipLaunchKernelGGL(prep_kernel<SampleViews>, dim3(mvs::ceil_div(n * v, 64)), dim3(64), 0, s, SampleViews{v, nullptr, nullptr, nullptr},
                       ref_cam, src_cams, n * v, xf);
    dim3 grid(mvs::ceil_div(W, 64), mvs::ceil_div(H, 4), n), block(64, 4);
    hipLaunchKernelGGL(geo_filter_sample_kernel, grid, block, 0, s, ref_depth, src_depths, ref_cam, xf, v, H, W, img_dist_thresh, depth_thresh,
                       vthresh, reproj_xyd, in_range, masks, mask, ref_depth_ave, points);
    return mvs::finish_launch("mvs_geo_filter_fwd");
}
