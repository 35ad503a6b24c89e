// Gipuma-style sequential depth-map fusion (the reference's default `--filter_method gipuma`, misc/gipuma.py -> the external
// `fusibile` binary).  The rule is RESTATED in include/mvs_hip.h (parity with the binary is unverified); this file is that text.
//
// One launch per reference view, enqueued in job order on one stream: a kept pixel marks the source pixels that supported it in
// `used`, and a later launch skips its own used pixels.  Launch k reads used[ref] and writes used[s], s != ref, only: no
// read-after-write race inside a launch, and racing writers all store the same byte.
//
// Layout of the work: a 16 x 16 block, i.e. a wavefront = 16 x 4 pixels, so that the 64 lanes of a gather land in a compact
// patch of the source view (4 short row segments) instead of along one 64-pixel row.  The source loop runs over a wave-uniform
// index, so the pair tables A / b / fb are read with scalar loads and live in scalar registers; ineligible pixels (zeroed by the
// probability filter, or already used) leave before the loop.
//
// A thread cannot hold (ix, iy) of every consistent source (Tanks-and-Temples scans have 300+ views).  It keeps a 64-bit mask of
// the LAST 64 sources' verdicts and, once the pixel is kept, walks the sources again: sources under the mask only recompute the
// projection (same instructions, same bits), earlier ones (S > 64) repeat the whole test.  The verdicts cannot differ: the depth
// stack is read-only during the launch.
#include "common.h"

namespace {

struct GipParams {
    float disp_thresh, num_consistent, depth_min, depth_max;
};

// steps 3a/3b of the rule: q = (A (x, y, 1)) d + b, z = q_2 > 0, (fx, fy) = floor(q_xy / z + 0.5) inside the image, compared as floats
__device__ __forceinline__ bool gip_project(const float* __restrict__ A, const float* __restrict__ b, float x, float y, float d, int H, int W,
                                            float& fx, float& fy, float& z) {
    const float q0 = ((A[0] * x + A[1] * y) + A[2]) * d + b[0];
    const float q1 = ((A[3] * x + A[4] * y) + A[5]) * d + b[1];
    z = ((A[6] * x + A[7] * y) + A[8]) * d + b[2];
    if (!(z > 0.0f)) return false;
    fx = floorf(q0 / z + 0.5f);
    fy = floorf(q1 / z + 0.5f);
    return fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H;
}

// the whole of step 3 for one source: on true, (fx, fy) is the source pixel and ds its depth
__device__ __forceinline__ bool gip_consistent(const float* __restrict__ A, const float* __restrict__ b, float fb,
                                               const float* __restrict__ depth_s, float x, float y, float d, int H, int W, const GipParams& p,
                                               float& fx, float& fy, float& ds) {
    float z;
    if (!gip_project(A, b, x, y, d, H, W, fx, fy, z)) return false;
    ds = depth_s[(size_t)(int)fy * W + (int)fx];
    if (!(ds > p.depth_min && ds < p.depth_max)) return false;
    return fabsf(fb / z - fb / ds) < p.disp_thresh;
}

// X_i = ((B[i][0] x + B[i][1] y) + B[i][2]) d + c[i]
__device__ __forceinline__ float gip_world(const float* __restrict__ B, const float* __restrict__ c, int i, float x, float y, float d) {
    return ((B[3 * i] * x + B[3 * i + 1] * y) + B[3 * i + 2]) * d + c[i];
}

// job k's row: the reference view and S source views; S = 0 = the row is inconsistent (nothing kept, nothing marked)
__device__ __forceinline__ int gip_row(const int32_t* __restrict__ ref_idx, const int32_t* __restrict__ src_idx, const int32_t* __restrict__ n_src,
                                       int k, int Vmax, int Nv, int& ref) {
    if (!ref_idx) { ref = k; return Nv - 1; }
    ref = ref_idx[k];
    const int S = n_src[k];
    if ((unsigned)ref >= (unsigned)Nv || S < 1 || S > Vmax) return 0;
    for (int j = 0; j < S; ++j) {
        const int s = src_idx[(size_t)k * Vmax + j];
        if ((unsigned)s >= (unsigned)Nv || s == ref) return 0;
    }
    return S;
}

__global__ __launch_bounds__(256) void gipuma_fuse_kernel(const float* __restrict__ depth, const float* __restrict__ Bt, const float* __restrict__ ct,
                                                          const float* __restrict__ At, const float* __restrict__ bt, const float* __restrict__ fbt,
                                                          int Nv, const int32_t* __restrict__ ref_idx, const int32_t* __restrict__ src_idx,
                                                          const int32_t* __restrict__ n_src, int k, int Vmax, int H, int W, GipParams p,
                                                          uint8_t* used, uint8_t* __restrict__ keep, uint8_t* __restrict__ count,
                                                          float* __restrict__ points) {
    const int xi = blockIdx.x * 16 + threadIdx.x, yi = blockIdx.y * 16 + threadIdx.y;
    if (xi >= W || yi >= H) return;
    const size_t HW = (size_t)H * W, pix = (size_t)yi * W + xi;
    int ref;
    const int S = gip_row(ref_idx, src_idx, n_src, k, Vmax, Nv, ref);
    const float d = S ? depth[(size_t)ref * HW + pix] : 0.0f;
    const bool eligible = S && d > p.depth_min && d < p.depth_max && used[(size_t)ref * HW + pix] == 0;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    int n = 0;
    bool kept = false;
    unsigned long long mask = 0;
    const int last = S ? ((S - 1) / 64) * 64 : 0;                  // the mask covers sources [last, S)
    const float x = (float)xi, y = (float)yi;
    const float* Ar = At + (size_t)ref * Nv * 9;
    const float* br = bt + (size_t)ref * Nv * 3;
    const float* fr = fbt + (size_t)ref * Nv;
    if (eligible) {
#pragma unroll
        for (int i = 0; i < 3; ++i) sum[i] = gip_world(Bt + (size_t)ref * 9, ct + (size_t)ref * 3, i, x, y, d);
        for (int j = 0; j < S; ++j) {
            const int s = ref_idx ? src_idx[(size_t)k * Vmax + j] : j + (j >= ref);
            float fx, fy, ds;
            if (!gip_consistent(Ar + (size_t)s * 9, br + (size_t)s * 3, fr[s], depth + (size_t)s * HW, x, y, d, H, W, p, fx, fy, ds)) continue;
#pragma unroll
            for (int i = 0; i < 3; ++i) sum[i] += gip_world(Bt + (size_t)s * 9, ct + (size_t)s * 3, i, fx, fy, ds);
            ++n;
            if (j >= last) mask |= 1ull << (j - last);
        }
        kept = (float)n >= p.num_consistent;
    }
    keep[(size_t)k * HW + pix] = kept ? 1 : 0;
    if (count) count[(size_t)k * HW + pix] = (uint8_t)min(n, 255);
    const float div = (float)(n + 1);
#pragma unroll
    for (int i = 0; i < 3; ++i) points[((size_t)k * 3 + i) * HW + pix] = kept ? sum[i] / div : 0.0f;
    if (!kept) return;
    for (int j = 0; j < S; ++j) {
        const int s = ref_idx ? src_idx[(size_t)k * Vmax + j] : j + (j >= ref);
        float fx, fy, t;
        if (j >= last) {
            if (!((mask >> (j - last)) & 1ull)) continue;
            if (!gip_project(Ar + (size_t)s * 9, br + (size_t)s * 3, x, y, d, H, W, fx, fy, t)) continue;     // cannot happen: it passed above
        } else if (!gip_consistent(Ar + (size_t)s * 9, br + (size_t)s * 3, fr[s], depth + (size_t)s * HW, x, y, d, H, W, p, fx, fy, t)) {
            continue;
        }
        used[(size_t)s * HW + (size_t)(int)fy * W + (int)fx] = 1;   // s != ref (gip_row), 0 <= fx < W, 0 <= fy < H (gip_project)
    }
}

}  // namespace

extern "C" int mvs_gipuma_fuse_scene(const float* depth, const float* B, const float* c, const float* A, const float* b, const float* fb, int Nv,
                                     const int32_t* ref_idx, const int32_t* src_idx, const int32_t* n_src, int R, int Vmax, int H, int W,
                                     float disp_thresh, float num_consistent, float depth_min, float depth_max, uint8_t* used, uint8_t* keep,
                                     uint8_t* count, float* points, mvs_stream_t stream) {
    MVS_REQUIRE(depth && B && c && A && b && fb && used && keep && points, "mvs_gipuma_fuse_scene: null pointer");
    MVS_REQUIRE(Nv >= 2 && Nv <= 32768 && H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24),
                "mvs_gipuma_fuse_scene: bad shape Nv=%d H=%d W=%d (at least two views, pixel coordinates exact in float32)", Nv, H, W);
    const bool table = ref_idx || src_idx || n_src;
    MVS_REQUIRE(!table || (ref_idx && src_idx && n_src), "mvs_gipuma_fuse_scene: the job table is ref_idx, src_idx and n_src, or none of them");
    if (table)
        MVS_REQUIRE(R >= 1 && R <= 65535 && Vmax >= 1 && Vmax < Nv, "mvs_gipuma_fuse_scene: bad job table R=%d Vmax=%d for %d views", R, Vmax, Nv);
    else
        MVS_REQUIRE(R == Nv && Vmax == Nv - 1, "mvs_gipuma_fuse_scene: without a job table R = Nv and Vmax = Nv - 1, got R=%d Vmax=%d Nv=%d", R,
                    Vmax, Nv);
    MVS_REQUIRE(disp_thresh == disp_thresh && num_consistent == num_consistent && depth_min == depth_min && depth_max == depth_max,
                "mvs_gipuma_fuse_scene: a threshold is NaN");
    const dim3 grid(mvs::ceil_div(W, 16), mvs::ceil_div(H, 16)), block(16, 16);
    MVS_REQUIRE(grid.y <= 65535u, "mvs_gipuma_fuse_scene: H=%d needs more than 65535 block rows", H);
    hipStream_t s = MVS_STREAM(stream);
    const size_t HW = (size_t)H * W;
    if (hipMemsetAsync(used, 0, (size_t)Nv * HW, s) != hipSuccess) return mvs::finish_launch("mvs_gipuma_fuse_scene(memset)");
    const GipParams p{disp_thresh, num_consistent, depth_min, depth_max};
    for (int k = 0; k < R; ++k)
        hipLaunchKernelGGL(gipuma_fuse_kernel, grid, block, 0, s, depth, B, c, A, b, fb, Nv, ref_idx, src_idx, n_src, k, Vmax, H, W, p, used, keep,
                           count, points);
    return mvs::finish_launch("mvs_gipuma_fuse_scene");
}
