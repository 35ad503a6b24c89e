// Scene-resident depth-map fusion — the end of the reference's inference script (test.py:404-549, filter_depth /
// dynamic_filter_depth): every view of a scan sits on the device once, all reference views are filtered against their
// source views through a job table, and the surviving points + colours are compacted, in the reference's order, straight
// into the 15-byte vertex records of the PLY file.
//
//   1. mvs_geo_filter_scene_fwd / mvs_geo_filter_dynamic_scene_fwd: job r = (ref_idx[r]; src_idx[r, 0..n_src[r])) indexes
//      the view stacks depth_ref / depth_src [Nv,H,W] and cams [Nv,2,4,4]; grid z = job.  The per-pixel arithmetic is
//      fusion_core.h, the same functions the per-sample kernels of fusion.hip call: bit-identical results.
//   2. mvs_pointcloud_count: keep = photo[ref_idx[r]] & geo[r]; per 256-pixel block the number kept (__ballot + popcount
//      per wavefront), per job the integer sums photo / geo / kept (integer atomics: exact, order-free); then ONE block
//      scans the block counts into 64-bit exclusive offsets (block_ops.h: 8192-element tiles with a running carry).
//   3. mvs_pointcloud_scatter (after the host has read the total and allocated): lane rank = mbcnt of the ballot + the
//      wavefront's offset + the block's offset; records are staged in LDS and stored as aligned dwords.
// No block ever waits on another block: the phases are separate launches on one stream.
//
// Output order = numpy boolean indexing per job (row-major over y, x), jobs concatenated (test.py:445-448, :459).
#include "block_ops.h"
#include "fusion_core.h"

namespace {

constexpr int kBlock = 256;            // pixels per compaction block (4 wavefronts)
constexpr int kRec = 15;               // bytes per vertex: x y z float32 little-endian, r g b uint8

// the filter kernels are the templates of fusion_core.h over JobViews: row r is job (ref_idx[r]; src_idx[r, 0..n_src[r]))

// ------------------------------------------------------------------------------------------------ compaction
// workspace: offsets int64 [N + 1] (exclusive scan of the block counts, offsets[N] = total), then counts uint32 [N], N = R * nb
__host__ __device__ inline long long pc_blocks(long long HW) { return (HW + kBlock - 1) / kBlock; }

__global__ __launch_bounds__(kBlock) void pc_count_kernel(const uint8_t* __restrict__ photo /*[Nv,HW]*/, const uint8_t* __restrict__ geo /*[R,HW]*/,
                                                          const int32_t* __restrict__ ref_idx, int Nv, size_t HW, uint32_t* __restrict__ counts,
                                                          unsigned long long* __restrict__ stats /*[R,3]*/) {
    const int r = blockIdx.y, ref = ref_idx[r];
    const size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x;
    bool p = false, g = false;
    if (pix < HW && (unsigned)ref < (unsigned)Nv) {
        p = photo[(size_t)ref * HW + pix] != 0;
        g = geo[(size_t)r * HW + pix] != 0;
    }
    __shared__ uint32_t part[3][kBlock / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t cp = blk::ballot_count(p), cg = blk::ballot_count(g), ck = blk::ballot_count(p && g);
    if (lane == 0) { part[0][wave] = cp; part[1][wave] = cg; part[2][wave] = ck; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const uint32_t s = blk::sum4(part[threadIdx.x]);
        if (threadIdx.x == 2) counts[(size_t)r * gridDim.x + blockIdx.x] = s;
        if (s) atomicAdd(&stats[r * 3 + threadIdx.x], (unsigned long long)s);
    }
}

__device__ __forceinline__ uint8_t colour_byte(const void* img, bool is_float, size_t i) {
    if (!img) return 0;
    if (!is_float) return reinterpret_cast<const uint8_t*>(img)[i];
    // the reference holds uint8/255. in fp32 and writes (c * 255).astype(uint8): one IEEE multiply, truncation toward zero
    const float c = reinterpret_cast<const float*>(img)[i] * 255.0f;
    return (uint8_t)min(__float2uint_rz(c), 255u);
}

__global__ __launch_bounds__(kBlock) void pc_scatter_kernel(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ geo,
                                                            const int32_t* __restrict__ ref_idx, int Nv, size_t HW,
                                                            const float* __restrict__ points /*[R,3,HW]*/, const void* __restrict__ img /*[Nv,3,HW]*/,
                                                            int img_is_float, const long long* __restrict__ offsets, long long total,
                                                            uint8_t* __restrict__ records, float* __restrict__ xyz, uint8_t* __restrict__ rgb) {
    const int r = blockIdx.y, ref = ref_idx[r];
    const size_t pix = (size_t)blockIdx.x * kBlock + threadIdx.x;
    bool keep = false;
    if (pix < HW && (unsigned)ref < (unsigned)Nv) keep = photo[(size_t)ref * HW + pix] != 0 && geo[(size_t)r * HW + pix] != 0;
    __shared__ uint32_t wcnt[kBlock / 64];
    __shared__ uint32_t stage[(kBlock * kRec + 4 + 3) / 4];
    uint32_t wave_cnt, cnt;
    const uint32_t rank = blk::ballot_rank(keep, wave_cnt);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = wave_cnt;
    __syncthreads();
    const uint32_t woff = blk::block_rank_offset(wcnt, cnt);
    if (cnt == 0) return;                                                     // uniform over the block
    const long long off = offsets[(size_t)r * gridDim.x + blockIdx.x];
    // never write past what the host allocated, whatever the offsets say
    if (off < 0 || off + (long long)cnt > total) return;
    const uint32_t k = woff + rank;
    const uint32_t sh = (uint32_t)((15ull * (unsigned long long)off) & 3ull);   // LDS bytes are laid out with the alignment of their destination
    uint8_t* sb = reinterpret_cast<uint8_t*>(stage);
    if (keep) {
        uint32_t u[3];
        uint8_t c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            u[a] = __float_as_uint(points[((size_t)r * 3 + a) * HW + pix]);
            c[a] = colour_byte(img, img_is_float != 0, ((size_t)ref * 3 + a) * HW + pix);
        }
        const long long m = off + (long long)k;
        if (xyz) { xyz[3 * m] = __uint_as_float(u[0]); xyz[3 * m + 1] = __uint_as_float(u[1]); xyz[3 * m + 2] = __uint_as_float(u[2]); }
        if (rgb) { rgb[3 * m] = c[0]; rgb[3 * m + 1] = c[1]; rgb[3 * m + 2] = c[2]; }
        if (records) {
            uint8_t* d = sb + sh + kRec * k;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int i = 0; i < 4; ++i) d[4 * a + i] = (uint8_t)(u[a] >> (8 * i));
                d[12 + a] = c[a];
            }
        }
    }
    if (!records) return;
    __syncthreads();
    // the block's bytes [sh, sh + len) of the staging area go to records + 15 * off - sh + the same index: whole dwords
    // inside the range as aligned dword stores, the <= 3 head and tail bytes one by one
    const uint32_t end = sh + kRec * cnt;
    uint8_t* gbase = records + (15ull * (unsigned long long)off - sh);
    for (uint32_t w = threadIdx.x; 4 * w < end; w += kBlock) {
        const uint32_t lo = 4 * w, hi = 4 * w + 4;
        if (lo >= sh && hi <= end) {
            *reinterpret_cast<uint32_t*>(gbase + lo) = stage[w];
        } else {
            for (uint32_t i = max(lo, sh); i < min(hi, end); ++i) gbase[i] = sb[i];
        }
    }
}

int check_scene(const char* what, const void* a, const void* b, const void* c, const void* t0, const void* t1, const void* t2, const void* ws,
                int Nv, int R, int Vmax, int H, int W) {
    MVS_REQUIRE(a && b && c && t0 && t1 && t2 && ws, "%s: null pointer", what);
    MVS_REQUIRE(Nv >= 1 && R >= 1 && R <= 65535 && Vmax >= 1 && H >= 2 && W >= 2 && (long long)R * Vmax <= (1LL << 24),
                "%s: bad shape Nv=%d R=%d Vmax=%d H=%d W=%d", what, Nv, R, Vmax, H, W);
    return 0;
}

}  // namespace

extern "C" int64_t mvs_geo_filter_scene_workspace_bytes(int R, int Vmax) {
    if (R < 1 || Vmax < 1) return -1;
    return (int64_t)R * Vmax * (int64_t)sizeof(ViewXf);
}

extern "C" int mvs_geo_filter_scene_fwd(const float* depth_ref, const float* depth_src, const float* cams, int Nv, const int32_t* ref_idx,
                                        const int32_t* src_idx, const int32_t* n_src, int R, int Vmax, int H, int W, float img_dist_thresh,
                                        float depth_thresh, float vthresh, void* workspace, uint8_t* mask, float* ref_depth_ave,
                                        float* points, mvs_stream_t stream) {
    if (int rc = check_scene("mvs_geo_filter_scene_fwd", depth_ref, depth_src, cams, ref_idx, src_idx, n_src, workspace, Nv, R, Vmax, H, W))
        return rc;
    hipStream_t s = MVS_STREAM(stream);
    ViewXf* xf = reinterpret_cast<ViewXf*>(workspace);
    const JobViews vw{Nv, ref_idx, src_idx, n_src, Vmax};
    hipLaunchKernelGGL(prep_kernel<JobViews>, dim3(mvs::ceil_div(R * Vmax, 64)), dim3(64), 0, s, vw, cams, cams, R * Vmax, xf);
    dim3 grid(mvs::ceil_div(W, 64), mvs::ceil_div(H, 4), R), block(64, 4);
    hipLaunchKernelGGL(geo_filter_kernel<JobViews>, grid, block, 0, s, vw, depth_ref, depth_src, xf, H, W, img_dist_thresh, depth_thresh,
                       vthresh, mask, ref_depth_ave, points);
    return mvs::finish_launch("mvs_geo_filter_scene_fwd");
}

extern "C" int mvs_geo_filter_dynamic_scene_fwd(const float* depth_ref, const float* depth_src, const float* cams, int Nv,
                                                const int32_t* ref_idx, const int32_t* src_idx, const int32_t* n_src, int R, int Vmax,
                                                int H, int W, float dist_base, float rel_diff_base, void* workspace, uint8_t* geo_mask,
                                                float* ref_depth_ave, float* points, mvs_stream_t stream) {
    if (int rc = check_scene("mvs_geo_filter_dynamic_scene_fwd", depth_ref, depth_src, cams, ref_idx, src_idx, n_src, workspace, Nv, R, Vmax,
                             H, W))
        return rc;
    MVS_REQUIRE(Vmax >= 2 && Vmax <= kMaxDynViews, "mvs_geo_filter_dynamic_scene_fwd: Vmax=%d, a job takes 2..%d source views", Vmax,
                kMaxDynViews);
    MVS_REQUIRE(dist_base > 0.0f && rel_diff_base > 0.0f, "mvs_geo_filter_dynamic_scene_fwd: bases must be positive");
    hipStream_t s = MVS_STREAM(stream);
    ViewXf* xf = reinterpret_cast<ViewXf*>(workspace);
    const JobViews vw{Nv, ref_idx, src_idx, n_src, Vmax};
    hipLaunchKernelGGL(prep_kernel<JobViews>, dim3(mvs::ceil_div(R * Vmax, 64)), dim3(64), 0, s, vw, cams, cams, R * Vmax, xf);
    dim3 grid(mvs::ceil_div(W, 64), mvs::ceil_div(H, 4), R), block(64, 4);
    hipLaunchKernelGGL(geo_filter_dynamic_kernel<JobViews>, grid, block, 0, s, depth_ref, depth_src, vw, xf, H, W, dist_base, rel_diff_base,
                       geo_mask, ref_depth_ave, points);
    return mvs::finish_launch("mvs_geo_filter_dynamic_scene_fwd");
}

extern "C" int64_t mvs_pointcloud_workspace_bytes(int R, int H, int W) {
    if (R < 1 || H < 1 || W < 1) return -1;
    const long long N = (long long)R * pc_blocks((long long)H * W);
    return (int64_t)((N + 1) * 8 + N * 4);
}

extern "C" int64_t mvs_pointcloud_record_offset(int64_t point_index) { return (int64_t)kRec * point_index; }

extern "C" int mvs_pointcloud_count(const uint8_t* photo_mask, const uint8_t* geo_mask, const int32_t* ref_idx, int Nv, int R, int H, int W,
                                    void* workspace, int64_t* stats, int64_t* total, mvs_stream_t stream) {
    MVS_REQUIRE(photo_mask && geo_mask && ref_idx && workspace && stats && total, "mvs_pointcloud_count: null pointer");
    MVS_REQUIRE(Nv >= 1 && R >= 1 && R <= 65535 && H >= 1 && W >= 1, "mvs_pointcloud_count: bad shape Nv=%d R=%d H=%d W=%d", Nv, R, H, W);
    MVS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mvs_pointcloud_count: workspace must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    const long long HW = (long long)H * W, nb = pc_blocks(HW), N = nb * R;
    long long* offsets = reinterpret_cast<long long*>(workspace);
    uint32_t* counts = reinterpret_cast<uint32_t*>(offsets + N + 1);
    if (hipMemsetAsync(stats, 0, sizeof(int64_t) * 3 * (size_t)R, s) != hipSuccess) return mvs::finish_launch("mvs_pointcloud_count(memset)");
    hipLaunchKernelGGL(pc_count_kernel, dim3((unsigned)nb, R), dim3(kBlock), 0, s, photo_mask, geo_mask, ref_idx, Nv, (size_t)HW, counts,
                       reinterpret_cast<unsigned long long*>(stats));
    blk::launch_exclusive_scan_u32(counts, N, offsets, reinterpret_cast<long long*>(total), s);
    return mvs::finish_launch("mvs_pointcloud_count");
}

extern "C" int mvs_pointcloud_scatter(const uint8_t* photo_mask, const uint8_t* geo_mask, const int32_t* ref_idx, int Nv, int R, int H, int W,
                                      const float* points, const void* images, int images_are_float, const void* workspace, int64_t total,
                                      uint8_t* records, float* xyz, uint8_t* rgb, mvs_stream_t stream) {
    MVS_REQUIRE(photo_mask && geo_mask && ref_idx && points && workspace, "mvs_pointcloud_scatter: null pointer");
    MVS_REQUIRE(records || xyz || rgb, "mvs_pointcloud_scatter: no output requested");
    MVS_REQUIRE(Nv >= 1 && R >= 1 && R <= 65535 && H >= 1 && W >= 1 && total >= 1,
                "mvs_pointcloud_scatter: bad shape Nv=%d R=%d H=%d W=%d total=%lld (an empty cloud needs no launch)", Nv, R, H, W,
                (long long)total);
    MVS_REQUIRE(total <= (long long)R * H * W, "mvs_pointcloud_scatter: total=%lld exceeds R*H*W", (long long)total);
    MVS_REQUIRE((reinterpret_cast<uintptr_t>(records) & 3) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                "mvs_pointcloud_scatter: records must be 4-byte and workspace 8-byte aligned");
    const long long HW = (long long)H * W, nb = pc_blocks(HW);
    hipLaunchKernelGGL(pc_scatter_kernel, dim3((unsigned)nb, R), dim3(kBlock), 0, MVS_STREAM(stream), photo_mask, geo_mask, ref_idx, Nv,
                       (size_t)HW, points, images, images_are_float, reinterpret_cast<const long long*>(workspace), (long long)total, records,
                       xyz, rgb);
    return mvs::finish_launch("mvs_pointcloud_scatter");
}
