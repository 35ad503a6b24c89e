// The work plan of a bf16 training convolution (bf16_conv_kernel of bf16_train.hip) in ONE place: output dims, work items, the K-split
// decision, the statistics rows its epilogue writes and the workspace that holds them - the kernel writes block_rows (or items) rows of
// 2*Cout floats into a workspace sized by conv_rows_workspace_bytes, so the formulas must agree exactly (tests/bf16_conv_plan_check.cpp
// sweeps them on the host) - and the work plan of the bf16 weight gradient (bf16_wgrad_kernel): patches, depth segments, blocks and LDS bytes, which
// the two workspace queries and the launch read (tests/conv_plan_tool.cpp sweeps it).  Host code only.
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

// ---- the bf16 weight gradient (bf16_wgrad_kernel): a work item = a patch of PH x WG_PW voxels of A over a depth segment -------------------
constexpr int WG_PW = 16;                                   // patch columns
struct WgradPlan { int PH, npr, npc, npatch, dseg, nseg, TA, TB, gy, blocks; size_t lds; };
constexpr size_t WG_RING_B = 56 * 1024;                      // budget of the 4-plane Bt ring (bytes)
inline int wgrad_nseg(int columns, int Dp, int target) {            // depth segments per column: enough work items, >= 2 depths each
    int nseg = (target + columns - 1) / columns;
    const int cap = Dp / 2 > 1 ? Dp / 2 : 1;
    if (nseg > cap) nseg = cap;
    return nseg < 1 ? 1 : nseg;
}
// grouped: a job of a GROUP launch - the jobs fill the chip together, so each takes fewer blocks (= slabs the reduce reads back) than a
// launch of its own needs: 256 for the single-tile instance, 128 for the others (measured on config 3's step, kernel time per step of
// the instances <1,1> / <2,2> / <1,4> / <2,1> at 512: 0.46 / 0.30 / 0.16 / 0.13 ms, at 256: 0.41 / 0.23 / 0.10 / 0.10, at 128: 0.42 / 0.15 /
// 0.11 / <0.09, at 64: 0.71 / 0.13 / 0.15 / 0.11; block counts proportional to the jobs' patch x depth steps were slower than either).
inline WgradPlan wgrad_plan(int nbatch, int CA, int CB, int Dp, int Hp, int Wp, int shw, bool grouped = false) {
    WgradPlan p;
    const int nA = (CA + 15) / 16, nB = (CB + 15) / 16;
    p.TB = nB;                                               // one block sees all of CB (nB <= 4)
    p.TA = nA < 4 / nB ? nA : 4 / nB;
    if (p.TA > 2) p.TA = 2;                                  // the A tile is staged as two 16-byte pieces per thread: 32 channels at most
    if (p.TA < 1) p.TA = 1;                                  // (64 x <=16 channels - no layer of the networks - runs as two channel groups)
    p.gy = (nA + p.TA - 1) / p.TA;
    const int b_row = CB < p.TB * 16 ? CB : p.TB * 16, a_row = CA < p.TA * 16 ? CA : p.TA * 16;
    p.PH = 8;
    while (p.PH > 2 && (size_t)4 * (p.PH * shw + 2) * (WG_PW * shw + 2) * b_row * 2 > WG_RING_B) p.PH >>= 1;
    p.npr = (Hp + p.PH - 1) / p.PH;
    p.npc = (Wp + WG_PW - 1) / WG_PW;
    // two resident blocks per CU over all channel groups (three for the single-tile instance was measured: no faster, and every block
    // writes a slab the reduce kernel reads back)
    static const int gblocks = mvs::env_int("MVS_WGRAD_GROUP_BLOCKS", 0);       // diagnostics
    const int target = (grouped ? (gblocks > 0 ? gblocks : p.TA * p.TB == 1 ? 256 : 128) : 512) / p.gy;
    p.nseg = wgrad_nseg(nbatch * p.npr * p.npc, Dp, target);
    p.dseg = (Dp + p.nseg - 1) / p.nseg;
    p.nseg = (Dp + p.dseg - 1) / p.dseg;
    p.npatch = nbatch * p.npr * p.npc * p.nseg;
    // the slab (= block) count must not depend on the stride (the workspace is sized without it): the count at PH = 8
    const int col8 = nbatch * ((Hp + 7) / 8) * p.npc;
    const int seg8 = wgrad_nseg(col8, Dp, target), d8 = (Dp + seg8 - 1) / seg8;
    const int least = col8 * ((Dp + d8 - 1) / d8);
    p.blocks = target < least ? target : least;
    if (p.blocks < 1) p.blocks = 1;
    p.lds = ((size_t)p.PH * WG_PW * a_row + 64 + (size_t)4 * (p.PH * shw + 2) * (WG_PW * shw + 2) * b_row + 64) * 2;
    return p;
}

}  // namespace mvsplan
