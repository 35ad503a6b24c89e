// The full-resolution tail of FPNDecoderV2 (models/module.py:299-300) as ONE kernel, channel-last in and out:
//
//     out4 = Swish(BN4(conv3x3( ReLU(BN3(ConvTranspose2d_{4,2,1}(out3))) + conv01 )))        out3 [N,h,w,16], conv01 [N,2h,2w,8] -> out4 [N,2h,2w,8]
//
// The ReLU sits between the two linear maps, so they cannot be composed (csrc/fpn_cp.hip's contraction-first form does not apply); what can be
// saved is the traffic: the 8-channel full-resolution up map lives in LDS only.  Per block, a fine tile of TW x TH = 30 x 14 output pixels:
//   1. the coarse window (17 x 9 pixels x 16 channels) that the tile's up map + its one-pixel halo reads -> LDS (range-checked 16-byte loads,
//      pixels outside the image are 0: a transposed convolution's missing taps contribute nothing);
//   2. the up map of the 32 x 16 fine positions (tile + halo): ReLU(convT * scale + shift) + conv01 -> LDS.  Positions OUTSIDE the image are the
//      3x3 convolution's zero padding and are written as 0, not as ReLU(shift) + skip.  Wave k works on output-parity class k (its 2x2 taps of
//      the 4x4 kernel, K = 64): 16 x 8 positions per class = two full rounds of 64 lanes, the class's weights wave-uniform;
//   3. the 3x3 convolution (K = 72) from LDS, + shift, Swish, two 16-byte stores per pixel.
// Arithmetic: fp32 FMAs, every weight a wave-uniform scalar operand read from the prepared table (both BatchNorm scales folded into the weights).
// Both contractions have N = 8: a 16x16x32 bf16 MFMA in three-term split form would run half empty and pay a per-pixel split of the up map,
// so the fp32 vector form is the one built; it is fp32 by construction (DESIGN.md §8 has its measured error and time).
// LDS: 12,240 B (coarse, pixel stride 20 dwords) + 24,576 B (up map, pixel stride 12 dwords: 16-byte aligned, conflict-free ds_read_b128
// within a 16-lane group) = 36.8 KB per block, four blocks per CU.
#include "conv_common.h"

namespace {

using mvsprim::f32x4;
using mvsprim::rsrc_t;
using mvsprim::OOB;
using mvsprim::make_rsrc;
using mvsprim::buf_load4;
using mvsprim::swish;
using mvsconv::xcd_block_coords;

constexpr int CI = 16, CM = 8, CO = 8;              // out3 channels -> up map channels -> out4 channels
constexpr int TW = 30, TH = 14;                     // fine output tile
constexpr int UW = TW + 2, UH = TH + 2;             // up map with halo: 32 x 16, 16 x 8 positions per parity class
constexpr int CW = UW / 2 + 1, CH = UH / 2 + 1;     // coarse window: 17 x 9
constexpr int CS = 20, US = 12;                     // LDS pixel strides in dwords
constexpr int WT_FLOATS = 4 * 4 * CI * CM;          // [class][tap a*2+b][cin][cmid]
constexpr int W3_FLOATS = 9 * CM * CO;              // [tap ky*3+kx][cmid][cout]

// wt [16,8,4,4] (ConvTranspose2d: [Cin,Cout,ky,kx]) * scale_up[cout], w3 [8,8,3,3] * scale_out[cout] -> the two tables above.
// Class (py, px) = output parity; its window row a = 0 | 1 is input row (i-1 | i) for py = 0 with ky = 3 | 1, (i | i+1) for py = 1 with ky = 2 | 0.
__global__ void fpn_v2_tail_prepare_kernel(const float* __restrict__ wt, const float* __restrict__ scale_up, const float* __restrict__ w3,
                                           const float* __restrict__ scale_out, float* __restrict__ prep) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < WT_FLOATS) {
        const int o = i % CM, c = (i / CM) % CI, t = (i / (CM * CI)) % 4, cls = i / (CM * CI * 4);
        const int py = cls >> 1, px = cls & 1, a = t >> 1, b = t & 1;
        const int ky = py == 0 ? (a ? 1 : 3) : (a ? 0 : 2), kx = px == 0 ? (b ? 1 : 3) : (b ? 0 : 2);
        prep[i] = wt[((c * CM + o) * 4 + ky) * 4 + kx] * scale_up[o];
    } else if (i < WT_FLOATS + W3_FLOATS) {
        const int j = i - WT_FLOATS;
        const int o = j % CO, c = (j / CO) % CM, tap = j / (CO * CM);
        prep[i] = w3[(o * CM + c) * 9 + tap] * scale_out[o];
    }
}

__global__ __launch_bounds__(256) void fpn_v2_tail_kernel(const float* __restrict__ out3, const float* __restrict__ lat,
                                                          const float* __restrict__ prep, const float* __restrict__ shift_up,
                                                          const float* __restrict__ shift_out, int h, int w, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_c[CH * CW * CS];
    __shared__ __attribute__((aligned(16))) float s_u[UH * UW * US];
    unsigned bx, by, bz;
    xcd_block_coords(bx, by, bz);
    const int H = 2 * h, W = 2 * w;
    const int x0 = (int)bx * TW, y0 = (int)by * TH;      // both even: a parity class is the same set of LDS positions in every tile
    const int tid = threadIdx.x, lane = tid & 63;
    const rsrc_t rc = make_rsrc(out3 + (size_t)bz * h * w * CI, (unsigned)(h * w * CI * 4));
    const rsrc_t rl = make_rsrc(lat + (size_t)bz * H * W * CM, (unsigned)(H * W * CM * 4));

    // ---- 1. coarse window -> LDS
    const int r0 = y0 / 2 - 1, c0 = x0 / 2 - 1;
    for (int i = tid; i < CH * CW * 4; i += 256) {
        const int p = i >> 2, q = i & 3;
        const int cy = p / CW, cx = p - cy * CW;
        const int gy = r0 + cy, gx = c0 + cx;
        const bool in = gy >= 0 && gy < h && gx >= 0 && gx < w;
        const f32x4 v = buf_load4(rc, in ? (unsigned)(((gy * w + gx) * CI + q * 4) * 4) : OOB);
        *reinterpret_cast<f32x4*>(&s_c[p * CS + q * 4]) = v;
    }
    __syncthreads();

    // ---- 2. up map + lateral for the tile and its halo -> LDS; wave = parity class
    {
        const int cls = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int py = cls >> 1, px = cls & 1;
        const float* __restrict__ wc = prep + cls * (4 * CI * CM);
#pragma unroll 1
        for (int r = 0; r < 2; ++r) {
            const int p = lane + 64 * r;
            const int cyi = p >> 4, cxi = p & 15;
            const int uy = 2 * cyi + (1 - py), ux = 2 * cxi + (1 - px);
            const int gy = y0 - 1 + uy, gx = x0 - 1 + ux;
            const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const unsigned off = in ? (unsigned)((gy * W + gx) * CM * 4) : OOB;
            const f32x4 l0 = buf_load4(rl, off), l1 = buf_load4(rl, in ? off + 16u : OOB);
            float acc[CM];
#pragma unroll
            for (int o = 0; o < CM; ++o) acc[o] = 0.0f;
#pragma unroll 1
            for (int g = 0; g < 8; ++g) {                      // (tap, channel half): 64 weights in scalar registers at a time
                const int t = g >> 1, c8 = (g & 1) * 8;
                const float* src = &s_c[((cyi + (t >> 1)) * CW + cxi + (t & 1)) * CS + c8];
                const float* __restrict__ wg = wc + (t * CI + c8) * CM;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(src + q * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int o = 0; o < CM; ++o) acc[o] = fmaf(v[e], wg[(q * 4 + e) * CM + o], acc[o]);
                }
            }
            f32x4 u0, u1;
#pragma unroll
            for (int o = 0; o < 4; ++o) {                      // outside the image: the 3x3's zero padding
                u0[o] = in ? fmaxf(acc[o] + shift_up[o], 0.0f) + l0[o] : 0.0f;
                u1[o] = in ? fmaxf(acc[4 + o] + shift_up[4 + o], 0.0f) + l1[o] : 0.0f;
            }
            float* dst = &s_u[(uy * UW + ux) * US];
            *reinterpret_cast<f32x4*>(dst) = u0;
            *reinterpret_cast<f32x4*>(dst + 4) = u1;
        }
    }
    __syncthreads();

    // ---- 3. 3x3 convolution from LDS, shift, Swish, 32-byte store per pixel
    const float* __restrict__ w3 = prep + WT_FLOATS;
    float* img_o = out + (size_t)bz * H * W * CO;
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
        const int t = tid + 256 * r;
        if (t >= TW * TH) break;
        const int oy = t / TW, ox = t - oy * TW;
        const int gy = y0 + oy, gx = x0 + ox;
        float acc[CO];
#pragma unroll
        for (int o = 0; o < CO; ++o) acc[o] = 0.0f;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {                    // 64 weights in scalar registers at a time
            const float* src = &s_u[((oy + tap / 3) * UW + ox + tap % 3) * US];
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
            for (int c = 0; c < CM; ++c) {
                const float x = c < 4 ? v0[c & 3] : v1[c & 3];
#pragma unroll
                for (int o = 0; o < CO; ++o) acc[o] = fmaf(x, w3[(tap * CM + c) * CO + o], acc[o]);
            }
        }
        if (gy < H && gx < W) {
            f32x4 o0, o1;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                o0[o] = swish(acc[o] + shift_out[o]);
                o1[o] = swish(acc[4 + o] + shift_out[4 + o]);
            }
            float* dst = img_o + ((size_t)gy * W + gx) * CO;
            *reinterpret_cast<f32x4*>(dst) = o0;
            *reinterpret_cast<f32x4*>(dst + 4) = o1;
        }
    }
}

bool tail_channels_ok(int Cin, int Cmid, int Cout) { return Cin == CI && Cmid == CM && Cout == CO; }

}  // namespace

extern "C" int64_t mvs_fpn_v2_tail_prepared_bytes(int Cin, int Cmid, int Cout) {
    return tail_channels_ok(Cin, Cmid, Cout) ? (int64_t)(WT_FLOATS + W3_FLOATS) * 4 : -1;
}

extern "C" int mvs_fpn_v2_tail_prepare(const float* wt, const float* scale_up, const float* w3, const float* scale_out, int Cin, int Cmid,
                                       int Cout, void* prepared, mvs_stream_t stream) {
    MVS_REQUIRE(wt && scale_up && w3 && scale_out && prepared, "mvs_fpn_v2_tail_prepare: null pointer");
    MVS_REQUIRE(tail_channels_ok(Cin, Cmid, Cout), "mvs_fpn_v2_tail_prepare: built for 16 -> 8 -> 8 channels (got %d -> %d -> %d)", Cin, Cmid, Cout);
    constexpr int total = WT_FLOATS + W3_FLOATS;
    hipLaunchKernelGGL(fpn_v2_tail_prepare_kernel, dim3(mvs::ceil_div(total, 256)), dim3(256), 0, MVS_STREAM(stream), wt, scale_up, w3, scale_out,
                       static_cast<float*>(prepared));
    return mvs::finish_launch("mvs_fpn_v2_tail_prepare");
}

extern "C" int mvs_fpn_v2_tail(const float* out3, const float* conv01, const void* prepared, const float* shift_up, const float* shift_out, int N,
                               int Cin, int Cmid, int Cout, int h, int w, float* out, mvs_stream_t stream) {
    MVS_REQUIRE(out3 && conv01 && prepared && shift_up && shift_out && out, "mvs_fpn_v2_tail: null pointer");
    MVS_REQUIRE(tail_channels_ok(Cin, Cmid, Cout), "mvs_fpn_v2_tail: built for 16 -> 8 -> 8 channels (got %d -> %d -> %d)", Cin, Cmid, Cout);
    MVS_REQUIRE(N >= 1 && h >= 1 && w >= 1, "mvs_fpn_v2_tail: bad shape N=%d h=%d w=%d", N, h, w);
    MVS_REQUIRE((int64_t)CM * 4 * h * w * 4 < ((int64_t)1 << 31), "mvs_fpn_v2_tail: one image's full-resolution map exceeds 2 GiB");
    const int ntx = mvs::ceil_div(2 * w, TW), nty = mvs::ceil_div(2 * h, TH);
    MVS_REQUIRE(nty <= 65535 && N <= 65535, "mvs_fpn_v2_tail: grid too large (%d row tiles, %d images)", nty, N);
    hipLaunchKernelGGL(fpn_v2_tail_kernel, dim3(ntx, nty, N), dim3(256), 0, MVS_STREAM(stream), out3, conv01, static_cast<const float*>(prepared),
                       shift_up, shift_out, h, w, out);
    return mvs::finish_launch("mvs_fpn_v2_tail");
}
