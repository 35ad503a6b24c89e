// The work plan of a bf16 training convolution (bf16_conv_kernel of bf16_train.hip) in ONE place: output dims, work items, the K-split
// decision, the statistics rows its epilogue writes and the workspace that holds them - the kernel writes block_rows (or items) rows of
// 2*Cout floats into a workspace sized by conv_rows_workspace_bytes, so the formulas must agree exactly (tests/bf16_conv_plan_check.cpp
// sweeps them on the host).  Host code only.
#pragma once
#include "common.h"

namespace mvsplan {

inline bool chan_ok(int c) { return c == 8 || c == 16 || c == 32 || c == 64; }

// K split over a block's wavefronts (see bf16_conv_kernel): 32 / 64 input channels (27 / 54 steps per wavefront) while the launch has
// at most ~3 work items per CU.  Every block streams the whole packed weight image (221 KB at 64 -> 64) from L2, and with one 64-voxel item
// per block that traffic is what bounds a larger launch: measured per call (tools/exp_small_conv.py, 64 -> 64 stride 1), split / not split:
// 256 items 14 / 37 us, 512 items 28 / 39 us, 1024 items 53 / 41 us (32 -> 64 stride (1,2,2): 11 / 21, 21 / 22, 41 / 24 us).
inline bool conv_ksplit(int cin, int items, int taps) {
    static const int lim = mvs::env_int("MVS_BF16_KSPLIT_ITEMS", 768);
    return taps == 27 && cin >= 32 && items <= lim;
}

struct ConvPlan {
    int Do, Ho, Wo;
    bool wpar;                          // ConvTranspose3d, column stride 2: a work item = ONE column parity of a 128-voxel chunk of a row
    int nwchunks;                       // chunks per output row: 64 voxels, or 128 (two items) when wpar
    int64_t items_per_sample, items;    // work items (64 output voxels of a row), sample-major; callers require items < 2^30
    bool ksplit;                        // a block's four wavefronts share ONE work item (else they take four consecutive ones)
    int64_t block_rows;                 // blocks that hold work = the statistics rows of the block-row form (ConvArgs::stats_rows)
    int samples;                        // statistics samples: B, or 1 when every row is one group's anyway (B == 1 or groups == 1)
    int64_t rows_per_sample;            // block rows of one of them (* samples == block_rows); -1: a block would straddle two samples
};                                      // of different groups (items_per_sample no multiple of 4, no K split)

// gather: 0 = Conv3d (out = (in - 1)/stride + 1, stride 1 | 2), 1 = ConvTranspose3d k3 p1 op(stride-1) (out = in*stride); groups: of the
// statistics, sample b in group b % groups.  Total (no division by an argument): callers may plan first and check the shape after.
inline ConvPlan conv_plan(int B, int Cin, int Di, int Hi, int Wi, int gather, int sd, int shw, int taps, int groups) {
    ConvPlan p;
    if (gather == 0) p.Do = sd == 2 ? (Di - 1) / 2 + 1 : Di, p.Ho = shw == 2 ? (Hi - 1) / 2 + 1 : Hi, p.Wo = shw == 2 ? (Wi - 1) / 2 + 1 : Wi;
    else p.Do = Di * sd, p.Ho = Hi * shw, p.Wo = Wi * shw;
    p.wpar = gather == 1 && shw == 2;
    p.nwchunks = p.wpar ? (p.Wo + 127) / 128 : (p.Wo + 63) / 64;
    p.items_per_sample = (int64_t)p.Do * p.Ho * p.nwchunks * (p.wpar ? 2 : 1);
    p.items = p.items_per_sample * B;
    p.ksplit = p.items < ((int64_t)1 << 30) && conv_ksplit(Cin, (int)p.items, taps);
    p.block_rows = p.ksplit ? p.items : (p.items + 3) / 4;
    p.samples = (B == 1 || groups == 1) ? 1 : B;
    p.rows_per_sample = p.samples == 1 ? p.block_rows : p.ksplit ? p.items_per_sample : p.items_per_sample % 4 == 0 ? p.items_per_sample / 4 : -1;
    return p;
}

// Bytes of the statistics rows of either form (a row of 2*Cout floats per work item, or per block), from the OUTPUT dims alone: two
// items per 128-voxel chunk bound one per 64-voxel chunk.  -1: bad shape.
inline int64_t conv_rows_workspace_bytes(int B, int Cout, int Do, int Ho, int Wo) {
    if (!chan_ok(Cout) || B < 1 || Do < 1 || Ho < 1 || Wo < 1) return -1;
    return (int64_t)B * Do * Ho * ((Wo + 127) / 128) * 2 * 2 * Cout * (int64_t)sizeof(float);
}

}  // namespace mvsplan
