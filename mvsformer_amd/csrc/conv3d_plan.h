// The work plans of the fp32 training convolutions in ONE place: conv3d_kernel (conv3d_fwd.hip), deconv3d_kernel (conv3d.hip),
// wino_conv3d_kernel (conv3d_wino.hip), wgrad_tiled_kernel and wgrad_kernel (wgrad.hip) - tile form, channels per chunk, LDS bytes, grid
// and work items.  The launchers launch what a plan says, and tests/conv_plan_tool.cpp prints the same plans for the edge tests, so a case
// table asserts facts about the code that runs.  Pure functions: none reads the environment (the launcher passes the value of a switch
// in), each is total over its arguments (callers may plan first and check the shape after).  Host code only; what a kernel template
// needs as well (pick_cc, lds_bytes, the tile of a form, TH / SEG of the weight gradient) is constexpr.
#pragma once
#include <string.h>

#include "conv_common.h"

namespace mvsconv {

// ---- conv3d_kernel ---------------------------------------------------------------------------------------------------------------------
// A block computes TD x TH output rows x 16*MT voxels along W x NT 16-channel tiles, CC input channels per LDS chunk.
enum class ConvForm { F22, F42, F22S64, F22S };          // 2x2x64 all channels | 4x2x64 all channels | 2x2x64 channels split | 2x2x32 channels split
struct ConvTile { int TD, TH, MT; };
constexpr ConvTile conv_tile(ConvForm f) {
    return f == ConvForm::F42 ? ConvTile{4, 2, 4} : f == ConvForm::F22S ? ConvTile{2, 2, 2} : ConvTile{2, 2, 4};
}
inline const char* conv_form_name(ConvForm f) {
    return f == ConvForm::F22 ? "22" : f == ConvForm::F42 ? "42" : f == ConvForm::F22S64 ? "22s64" : "22s";
}

// input channels per chunk: 8 if tile + weights fit in ~96 KiB of LDS, else 4
constexpr int tile_cs(int SD, int SHW, int TD, int TH, int MT) {
    return pad_cs(((TD - 1) * SD + 3) * ((TH - 1) * SHW + 3) * ((16 * MT - 1) * SHW + 3), SHW);
}
constexpr int pick_cc(int NP, int SD, int SHW, int TD, int TH, int MT) {
    return (8 * tile_cs(SD, SHW, TD, TH, MT) + 2 * 27 * 4 * NP) * 4 <= 96 * 1024 ? 8 : 4;
}
constexpr size_t lds_bytes(int NP, int SD, int SHW, int TD, int TH, int MT) {
    const int cc = pick_cc(NP, SD, SHW, TD, TH, MT);
    return (size_t)(cc * tile_cs(SD, SHW, TD, TH, MT) + (cc / 4) * 27 * 4 * NP) * 4;
}

struct Conv3dPlan {
    ConvForm form;
    int NT;                     // 16-channel N tiles per block: all of Cout, or 1 when the output channels are split over blocks
    int TD, TH, MT;             // conv_tile(form)
    int CC, NP;                 // input channels per chunk; packed weight row length (of the layer's full Cout)
    int nsplit;                 // blocks along x that share one output tile, each with NT of the channel tiles
    int Do, Ho, Wo;
    unsigned gx, gy, gz;        // grid
    size_t lds;                 // dynamic LDS bytes
    int chunks;                 // LDS chunks of CC input channels
};

// Tile choice (measured with tools/bench_conv.py on config-2 shapes, profiles/r01_conv_layers_*.txt):
//   * NTF == 1 (Cout 8/16) on large volumes: 4x2-row tiles, one block per CU — the weight fragment is reused by 8 MFMAs
//     and the halo re-read drops from 4.1x to 2.3x (2x faster for the stride-(1,2,2) conv1);
//   * NTF >= 2: 2x2-row tiles at 2 blocks per CU are as fast or faster;
//   * small volumes (deep U-Net levels of the coarse stages, < 256 blocks): 32-voxel tiles and one 16-channel N tile per
//     block, so a 64->64 layer on 4x18x24 voxels becomes 72 short blocks instead of 18 long ones.
// force: what MVS_CONV_TILE holds (tuning knob for tools/bench_conv.py: 42 | 22 | 22s), or null.
inline Conv3dPlan conv3d_plan(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int shw, const char* force) {
    Conv3dPlan p;
    p.Do = sd == 2 ? (Di - 1) / 2 + 1 : Di, p.Ho = shw == 2 ? (Hi - 1) / 2 + 1 : Hi, p.Wo = shw == 2 ? (Wi - 1) / 2 + 1 : Wi;
    const int NTF = nt_of(Cout);
    p.NP = np_of(NTF);
    const int NP = p.NP;
    auto blocks = [&](int td, int th, int tw) {
        return (long)mvs::ceil_div(p.Wo, tw) * mvs::ceil_div(p.Ho, th) * mvs::ceil_div(p.Do, td) * B;
    };
    int pick = 0;
    if (force) {
        if (sd == 1 && !strcmp(force, "42") && p.Do >= 3) pick = 2;
        else if (!strcmp(force, "22")) pick = 1;
        else if (!strcmp(force, "22s")) pick = 4;
    }
    if (!pick) {
        // cost model: the matrix pipe of a CU is the shared resource, so time ~ (blocks per CU, rounded up) x (MFMA cycles
        // per block + per-chunk staging overhead, which is exposed when only one block fits on the CU)
        auto model = [&](int td, int th, int mt, int ntb, size_t lds, int cc) {
            const double chunks = mvs::ceil_div(Cin, cc);
            const double mfma = 27.0 * (cc / 4) * (td * th / 4) * mt * ntb * 32.0;
            const double ovh = (lds > 80 * 1024) ? 3500.0 : 1200.0;
            const long nb = blocks(td, th, 16 * mt) * mvs::ceil_div(NTF, ntb);
            return (double)((nb + 255) / 256) * chunks * (mfma + ovh);
        };
        double best = 1e300;
        pick = 1;
        {   // 1: 2x2 rows, 64 voxels, all channels
            const double c = model(2, 2, 4, NTF, lds_bytes(NP, sd, shw, 2, 2, 4), pick_cc(NP, sd, shw, 2, 2, 4));
            if (c < best) { best = c; pick = 1; }
        }
        if (NTF == 1 && sd == 1 && p.Do >= 3) {   // 2: 4x2 rows
            const double c = model(4, 2, 4, NTF, lds_bytes(NP, sd, shw, 4, 2, 4), pick_cc(NP, sd, shw, 4, 2, 4)) * (shw == 2 ? 0.6 : 0.95);
            if (c < best) { best = c; pick = 2; }
        }
        if (NTF > 1) {   // 3: channels split over blocks, 64 voxels
            const double c = model(2, 2, 4, 1, lds_bytes(NP, sd, shw, 2, 2, 4), pick_cc(NP, sd, shw, 2, 2, 4)) * 1.1;
            if (c < best) { best = c; pick = 3; }
        }
        {   // 4: channels split, 32 voxels
            const double c = model(2, 2, 2, 1, lds_bytes(NP, sd, shw, 2, 2, 2), pick_cc(NP, sd, shw, 2, 2, 2)) * 1.15;
            if (c < best || p.Wo <= 32) { best = c; pick = 4; }
        }
    }
    p.form = pick == 4 ? ConvForm::F22S : pick == 3 ? ConvForm::F22S64 : pick == 2 ? ConvForm::F42 : ConvForm::F22;
    const ConvTile t = conv_tile(p.form);
    p.TD = t.TD, p.TH = t.TH, p.MT = t.MT;
    p.NT = (p.form == ConvForm::F22 || p.form == ConvForm::F42) ? NTF : 1;
    p.CC = pick_cc(NP, sd, shw, t.TD, t.TH, t.MT);
    p.lds = lds_bytes(NP, sd, shw, t.TD, t.TH, t.MT);
    p.nsplit = mvs::ceil_div(NTF, p.NT);
    p.gx = (unsigned)(mvs::ceil_div(p.Wo, 16 * t.MT) * p.nsplit), p.gy = (unsigned)mvs::ceil_div(p.Ho, t.TH);
    p.gz = (unsigned)(B * mvs::ceil_div(p.Do, t.TD));
    p.chunks = mvs::ceil_div(Cin, p.CC);
    return p;
}

// ---- deconv3d_kernel -------------------------------------------------------------------------------------------------------------------
constexpr int CC_DECONV = 8;                                                  // input channels per LDS chunk
constexpr int DECONV_IWI = 32, DECONV_IHI = 2;                                // input columns (+1 halo) and rows (+1) per block
constexpr int deconv_id(int SD) { return SD == 1 ? 4 : 2; }                   // input depths staged per block
constexpr size_t deconv_lds_bytes(int NT, int SD) {
    return (size_t)(CC_DECONV * pad_cs(deconv_id(SD) * (DECONV_IHI + 1) * (DECONV_IWI + 1), 1) + (CC_DECONV / 4) * 27 * 4 * np_of(NT)) * sizeof(float);
}
// the layers of the split-form kernel of deconv3d_s1.hip under stride-1 depth; mvs_deconv3d_fwd routes by this and refuses a layer that
// deconv_s1_supported (the packing side, deconv3d_s1.hip) does not know
inline bool deconv_s1_cout(int Cout) { return Cout == 8 || Cout == 16; }

struct Deconv3dPlan {
    bool s1;                    // stride-1 depth with 8 / 16 output channels: deconv3d_s1.hip, else deconv3d_kernel
    int NT;
    int TWI, THI, TDI;          // a block covers TWI input columns, THI input rows and TDI input depths (sd == 1: = 2 output depths)
    int Do, Ho, Wo;
    unsigned gx, gy, gz;
    size_t lds;
    int chunks;
};

inline Deconv3dPlan deconv3d_plan(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd) {
    Deconv3dPlan p;
    p.s1 = sd == 1 && deconv_s1_cout(Cout);
    p.NT = nt_of(Cout);
    p.TWI = DECONV_IWI, p.THI = DECONV_IHI, p.TDI = sd == 1 ? 2 : 1;
    p.Do = Di * sd, p.Ho = Hi * 2, p.Wo = Wi * 2;
    p.gx = (unsigned)mvs::ceil_div(Wi, DECONV_IWI), p.gy = (unsigned)mvs::ceil_div(Hi, DECONV_IHI);
    p.gz = (unsigned)(B * ((sd == 1) ? mvs::ceil_div(Di, 2) : Di));
    p.lds = deconv_lds_bytes(p.NT, sd == 1 ? 1 : 2);
    p.chunks = mvs::ceil_div(Cin, CC_DECONV);
    return p;
}

// ---- wino_conv3d_kernel ----------------------------------------------------------------------------------------------------------------
constexpr int WTY = 4;                       // tile rows per block = wavefronts

inline bool wino_supported(int Cin, int Cout, int D, int H, int W) {
    return Cin >= 4 && Cin % 4 == 0 && Cout >= 16 && Cout % 16 == 0 && Cout <= 64 && D >= 1 && H >= 1 && W >= 4 && W % 4 == 0 &&
           (int64_t)4 * D * H * W * 4 < ((int64_t)1 << 31);
}

struct WinoPlan {
    bool supported;
    int NT;                     // all output channels in one block up to 32 (128 accumulator registers); 48/64 channels split over blocks
    int ngroups;                // channel groups of 16 NT
    unsigned gx, gy, gz;        // a block = WTY tile rows (2 WTY output rows) x 32 output columns of one depth plane x 16 NT channels
    int chunks;                 // of 4 input channels
};

inline WinoPlan wino_plan(int B, int Cin, int Cout, int D, int H, int W, int env_nt) {      // env_nt: MVS_WINO_NT, 0 when unset
    WinoPlan p;
    p.supported = wino_supported(Cin, Cout, D, H, W);
    p.NT = (env_nt == 2 && Cout % 32 == 0) ? 2 : 1;
    p.ngroups = Cout / (16 * p.NT);
    p.gx = (unsigned)(D * p.ngroups), p.gy = (unsigned)mvs::ceil_div(W, 32), p.gz = (unsigned)(mvs::ceil_div(H, 2 * WTY) * B);
    p.chunks = Cin / 4;
    return p;
}

// ---- wgrad_tiled_kernel, wgrad_kernel --------------------------------------------------------------------------------------------------
//   SHW = 1: TH x SEG = 8x64 (MT=1), 4x64 (MT=2), 2x64 (MT=3,4)        SHW = 2: 4x32
constexpr int wg_seg(int SHW) { return SHW == 1 ? 64 : 32; }
inline int wg_mt(int CA) { const int mt = mvs::ceil_div(CA, 16); return mt >= 1 && mt <= 3 ? mt : 4; }      // 16-channel tiles of A (CA <= 64)
constexpr int wg_th(int MT, int SHW) { return SHW == 2 ? 4 : (MT == 1 ? 8 : (MT == 2 ? 4 : 2)); }

struct WgradTiledPlan {
    int MT, TH, SEG;            // 16-channel tiles of A; output tile = TH rows x SEG voxels of one (batch, depth)
    int nchunk;                 // chunks of 4 Bt channels = grid.x
    int hblocks, wblocks;
    long long ntiles;           // block y walks tiles y, y + gy, ..
    long long gy;
};

inline WgradTiledPlan wgrad_tiled_plan(int nbatch, int CA, int CB, int Dp, int Hp, int Wp, int shw) {
    WgradTiledPlan p;
    p.MT = wg_mt(CA);
    p.TH = wg_th(p.MT, shw), p.SEG = wg_seg(shw);
    p.nchunk = mvs::ceil_div(CB, 4);
    p.hblocks = mvs::ceil_div(Hp, p.TH), p.wblocks = mvs::ceil_div(Wp, p.SEG);
    p.ntiles = (long long)nbatch * Dp * p.hblocks * p.wblocks;
    p.gy = mvs::ceil_div(512, p.nchunk < 1 ? 1 : p.nchunk);          // ~2 blocks per CU in total: few adders per dW address (256: slower)
    if (p.gy > p.ntiles) p.gy = p.ntiles;
    if (p.gy < 1) p.gy = 1;
    return p;
}

struct WgradV1Plan { int MT, nchunk, rows, gy; };      // wgrad_kernel: a wavefront walks rows (batch, depth, row) y*4 + wave, + 4 gy, ..

inline WgradV1Plan wgrad_v1_plan(int nbatch, int CA, int CB, int Dp, int Hp) {
    WgradV1Plan p;
    p.MT = wg_mt(CA);
    p.nchunk = mvs::ceil_div(CB, 4);
    p.rows = nbatch * Dp * Hp;
    p.gy = mvs::ceil_div(1024, p.nchunk < 1 ? 1 : p.nchunk);
    if (p.gy > mvs::ceil_div(p.rows, NWAVES)) p.gy = mvs::ceil_div(p.rows, NWAVES);
    if (p.gy < 1) p.gy = 1;
    return p;
}

}  // namespace mvsconv
