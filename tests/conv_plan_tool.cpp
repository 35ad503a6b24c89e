// Stand-alone host program over the two plan headers of the training convolutions, csrc/conv3d_plan.h (fp32: conv3d_kernel,
// deconv3d_kernel, wino_conv3d_kernel, wgrad_tiled_kernel, wgrad_kernel) and csrc/bf16_conv_plan.h (bf16_conv_kernel, bf16_wgrad_kernel).
// Not part of the library; host code only.
//
//   no argument   check mode: every plan against the launch arithmetic it replaced - dispatch_tile / launch of conv3d_fwd.hip, launch_deconv
//                 of conv3d.hip, mvs_conv3d_wino_fwd, launch_wgrad_tiled and mvs_conv3d_wgrad of wgrad.hip, wgrad_plan of bf16_train.hip - kept
//                 here verbatim as the oracle, field by field over the tile edges.  Prints "ok" and exits 0 when every case agrees
//                 (tests/test_abi.py builds it with AddressSanitizer and UBSan on the host side and runs it).
//   "print"       print mode: one request per line on stdin - a kind and its arguments - one line of name=value fields per request on
//                 stdout.  This is how the edge tests (tests/conv_plan_reader.py) learn what the launchers do.
//                     conv B Cin Cout Di Hi Wi sd shw force          force: what MVS_CONV_TILE holds, "-" when unset
//                     conv_tile form                                 form: 22 | 42 | 22s64 | 22s
//                     deconv B Cin Cout Di Hi Wi sd
//                     wino B Cin Cout D H W env_nt                   env_nt: MVS_WINO_NT, 0 when unset
//                     wgrad nbatch CA CB Dp Hp Wp shw
//                     wgrad_v1 nbatch CA CB Dp Hp
//                     bf16_conv B Cin Di Hi Wi gather sd shw taps groups
//                     bf16_wgrad nbatch CA CB Dp Hp Wp shw grouped
//                     bf16_consts
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../mvsformer_amd/csrc/bf16_conv_plan.h"
#include "../mvsformer_amd/csrc/conv3d_plan.h"

using namespace mvsconv;

// ---- the parent's formulas, verbatim ---------------------------------------------------------------------------------------------------
namespace old {
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
struct ConvArgs { int B, Cin, Cout, Do, Ho, Wo; };
struct Launch { int NT, NP, TD, TH, MT, CC; size_t lds; unsigned gx, gy, gz; };

template <int NT, int NP, int SD, int SHW, int TD, int TH, int MT>
Launch launch(const ConvArgs& a) {
    constexpr size_t lds = lds_bytes(NP, SD, SHW, TD, TH, MT);
    static_assert(lds <= 160 * 1024, "tile does not fit in LDS");
    const int nsplit = mvs::ceil_div(nt_of(a.Cout), NT);
    dim3 grid(mvs::ceil_div(a.Wo, 16 * MT) * nsplit, mvs::ceil_div(a.Ho, TH), a.B * mvs::ceil_div(a.Do, TD));
    return Launch{NT, NP, TD, TH, MT, pick_cc(NP, SD, SHW, TD, TH, MT), lds, grid.x, grid.y, grid.z};
}

template <int NTF, int SD, int SHW>
Launch dispatch_tile(const ConvArgs& a, const char* force) {
    constexpr int NP = np_of(NTF);
    auto blocks = [&](int td, int th, int tw) {
        return (long)mvs::ceil_div(a.Wo, tw) * mvs::ceil_div(a.Ho, th) * mvs::ceil_div(a.Do, td) * a.B;
    };
    if (force) {
        if constexpr (SD == 1) { if (!strcmp(force, "42") && a.Do >= 3) return launch<NTF, NP, SD, SHW, 4, 2, 4>(a); }
        if (!strcmp(force, "22")) return launch<NTF, NP, SD, SHW, 2, 2, 4>(a);
        if (!strcmp(force, "22s")) return launch<1, NP, SD, SHW, 2, 2, 2>(a);
    }
    auto model = [&](int td, int th, int mt, int ntb, size_t lds, int cc) {
        const double chunks = mvs::ceil_div(a.Cin, cc);
        const double mfma = 27.0 * (cc / 4) * (td * th / 4) * mt * ntb * 32.0;
        const double ovh = (lds > 80 * 1024) ? 3500.0 : 1200.0;
        const long nb = blocks(td, th, 16 * mt) * mvs::ceil_div(NTF, ntb);
        return (double)((nb + 255) / 256) * chunks * (mfma + ovh);
    };
    double best = 1e300;
    int pick = 1;
    {   // 1: 2x2 rows, 64 voxels, all channels
        const double c = model(2, 2, 4, NTF, lds_bytes(NP, SD, SHW, 2, 2, 4), pick_cc(NP, SD, SHW, 2, 2, 4));
        if (c < best) { best = c; pick = 1; }
    }
    if constexpr (NTF == 1 && SD == 1) {
        if (a.Do >= 3) {   // 2: 4x2 rows
            const double c = model(4, 2, 4, NTF, lds_bytes(NP, SD, SHW, 4, 2, 4), pick_cc(NP, SD, SHW, 4, 2, 4)) * (SHW == 2 ? 0.6 : 0.95);
            if (c < best) { best = c; pick = 2; }
        }
    }
    if constexpr (NTF > 1) {   // 3: channels split over blocks, 64 voxels
        const double c = model(2, 2, 4, 1, lds_bytes(NP, SD, SHW, 2, 2, 4), pick_cc(NP, SD, SHW, 2, 2, 4)) * 1.1;
        if (c < best) { best = c; pick = 3; }
    }
    {   // 4: channels split, 32 voxels
        const double c = model(2, 2, 2, 1, lds_bytes(NP, SD, SHW, 2, 2, 2), pick_cc(NP, SD, SHW, 2, 2, 2)) * 1.15;
        if (c < best || a.Wo <= 32) { best = c; pick = 4; }
    }
    if (pick == 4) return launch<1, NP, SD, SHW, 2, 2, 2>(a);
    if constexpr (NTF > 1) { if (pick == 3) return launch<1, NP, SD, SHW, 2, 2, 4>(a); }
    if constexpr (NTF == 1 && SD == 1) { if (pick == 2) return launch<NTF, NP, SD, SHW, 4, 2, 4>(a); }
    return launch<NTF, NP, SD, SHW, 2, 2, 4>(a);
}

Launch conv3d_fwd(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int shw, const char* force) {
    ConvArgs a{B, Cin, Cout, (Di - 1) / sd + 1, (Hi - 1) / shw + 1, (Wi - 1) / shw + 1};
    const int nt = nt_of(Cout);
#define MVS_CONV(NTV)                                                     \
    if (sd == 1 && shw == 1) return dispatch_tile<NTV, 1, 1>(a, force);   \
    if (sd == 2) return dispatch_tile<NTV, 2, 2>(a, force);               \
    return dispatch_tile<NTV, 1, 2>(a, force)
    if (nt == 1) { MVS_CONV(1); }
    if (nt == 2) { MVS_CONV(2); }
    MVS_CONV(4);
#undef MVS_CONV
}

constexpr int CC_DECONV = 8;
template <int NT, int SD>
size_t deconv_lds_bytes() {
    constexpr int ID = (SD == 1) ? 4 : 2, IW = 32 + 1;
    return (size_t)(CC_DECONV * pad_cs(ID * 3 * IW, 1) + (CC_DECONV / 4) * 27 * 4 * np_of(NT)) * sizeof(float);
}
template <int NT, int SD>
Launch launch_deconv(int B, int Di, int Hi, int Wi) {
    const size_t lds = deconv_lds_bytes<NT, SD>();
    dim3 grid(mvs::ceil_div(Wi, 32), mvs::ceil_div(Hi, 2), B * ((SD == 1) ? mvs::ceil_div(Di, 2) : Di));
    return Launch{NT, np_of(NT), 0, 0, 0, CC_DECONV, lds, grid.x, grid.y, grid.z};
}
bool deconv_s1_supported(int Cout) { return Cout == 8 || Cout == 16; }       // deconv3d_s1.hip
Launch deconv3d_fwd(int B, int Cout, int Di, int Hi, int Wi, int sd, bool* s1) {
    *s1 = sd == 1 && deconv_s1_supported(Cout);
    const int nt = nt_of(Cout);
#define MVS_DECONV(NTV)                                             \
    if (sd == 1) return launch_deconv<NTV, 1>(B, Di, Hi, Wi);       \
    return launch_deconv<NTV, 2>(B, Di, Hi, Wi)
    if (nt == 1) { MVS_DECONV(1); }
    if (nt == 2) { MVS_DECONV(2); }
    MVS_DECONV(4);
#undef MVS_DECONV
}

constexpr int WTY = 4;
int wino_supported(int Cin, int Cout, int D, int H, int W) {
    return Cin >= 4 && Cin % 4 == 0 && Cout >= 16 && Cout % 16 == 0 && Cout <= 64 && D >= 1 && H >= 1 && W >= 4 && W % 4 == 0 &&
           (int64_t)4 * D * H * W * 4 < ((int64_t)1 << 31);
}
Launch wino_fwd(int B, int Cout, int D, int H, int W, int env_nt) {
    const int nt = (env_nt == 2 && Cout % 32 == 0) ? 2 : 1;
    const int ngroups = Cout / (16 * nt);
    dim3 grid(D * ngroups, mvs::ceil_div(W, 32), mvs::ceil_div(H, 2 * WTY) * B);
    return Launch{nt, ngroups, 0, 0, 0, 0, 0, grid.x, grid.y, grid.z};
}

template <int MT, int SHW>
struct WgTile {
    static constexpr int SEG = SHW == 1 ? 64 : 32;
    static constexpr int TH = SHW == 2 ? 4 : (MT == 1 ? 8 : (MT == 2 ? 4 : 2));
};
struct WgLaunch { int MT, TH, SEG, nchunk; long long ntiles, gy; };
template <int MT, int SHW>
WgLaunch launch_wgrad_tiled(int nbatch, int CB, int Dp, int Hp, int Wp) {
    using T = WgTile<MT, SHW>;
    const int nchunk = mvs::ceil_div(CB, 4);
    const long long ntiles = (long long)nbatch * Dp * mvs::ceil_div(Hp, T::TH) * mvs::ceil_div(Wp, T::SEG);
    long long gy = mvs::ceil_div(512, nchunk);
    if (gy > ntiles) gy = ntiles;
    if (gy < 1) gy = 1;
    return WgLaunch{MT, T::TH, T::SEG, nchunk, ntiles, gy};
}
WgLaunch conv3d_wgrad(int nbatch, int CA, int CB, int Dp, int Hp, int Wp, int shw) {
    const int mt2 = mvs::ceil_div(CA, 16);
#define MVS_WGT(M)                                                          \
    if (shw == 1) return launch_wgrad_tiled<M, 1>(nbatch, CB, Dp, Hp, Wp);  \
    else return launch_wgrad_tiled<M, 2>(nbatch, CB, Dp, Hp, Wp)
    switch (mt2) {
        case 1: MVS_WGT(1);
        case 2: MVS_WGT(2);
        case 3: MVS_WGT(3);
        default: MVS_WGT(4);
    }
#undef MVS_WGT
}
WgLaunch conv3d_wgrad_v1(int nbatch, int CA, int CB, int Dp, int Hp) {
    const int nchunk = mvs::ceil_div(CB, 4);
    const int rows = nbatch * Dp * Hp;
    int gy = mvs::ceil_div(1024, nchunk);
    if (gy > mvs::ceil_div(rows, mvsconv::NWAVES)) gy = mvs::ceil_div(rows, mvsconv::NWAVES);
    if (gy < 1) gy = 1;
    const int mt = mvs::ceil_div(CA, 16);
    return WgLaunch{mt >= 1 && mt <= 3 ? mt : 4, 0, 0, nchunk, rows, gy};
}

// bf16_train.hip
constexpr int WG_PW = 16;
struct WgradPlan { int PH, npr, npc, npatch, dseg, nseg, TA, TB, gy, blocks; size_t lds; };
constexpr size_t WG_RING_B{56 * 1024};
int wgrad_nseg(int columns, int Dp, int target) {
    int nseg = (target + columns - 1) / columns;
    const int cap = Dp / 2 > 1 ? Dp / 2 : 1;
    if (nseg > cap) nseg = cap;
    return nseg < 1 ? 1 : nseg;
}
WgradPlan wgrad_plan(int nbatch, int CA, int CB, int Dp, int Hp, int Wp, int shw, bool grouped = false) {
    WgradPlan p;
    const int nA = (CA + 15) / 16, nB = (CB + 15) / 16;
    p.TB = nB;
    p.TA = nA < 4 / nB ? nA : 4 / nB;
    if (p.TA > 2) p.TA = 2;
    if (p.TA < 1) p.TA = 1;
    p.gy = (nA + p.TA - 1) / p.TA;
    const int b_row = CB < p.TB * 16 ? CB : p.TB * 16, a_row = CA < p.TA * 16 ? CA : p.TA * 16;
    p.PH = 8;
    while (p.PH > 2 && (size_t)4 * (p.PH * shw + 2) * (WG_PW * shw + 2) * b_row * 2 > WG_RING_B) p.PH >>= 1;
    p.npr = (Hp + p.PH - 1) / p.PH;
    p.npc = (Wp + WG_PW - 1) / WG_PW;
    static const int gblocks = mvs::env_int("MVS_WGRAD_GROUP_BLOCKS", 0);
    const int target = (grouped ? (gblocks > 0 ? gblocks : p.TA * p.TB == 1 ? 256 : 128) : 512) / p.gy;
    p.nseg = wgrad_nseg(nbatch * p.npr * p.npc, Dp, target);
    p.dseg = (Dp + p.nseg - 1) / p.nseg;
    p.nseg = (Dp + p.dseg - 1) / p.dseg;
    p.npatch = nbatch * p.npr * p.npc * p.nseg;
    const int col8 = nbatch * ((Hp + 7) / 8) * p.npc;
    const int seg8 = wgrad_nseg(col8, Dp, target), d8 = (Dp + seg8 - 1) / seg8;
    const int least = col8 * ((Dp + d8 - 1) / d8);
    p.blocks = target < least ? target : least;
    if (p.blocks < 1) p.blocks = 1;
    p.lds = ((size_t)p.PH * WG_PW * a_row + 64 + (size_t)4 * (p.PH * shw + 2) * (WG_PW * shw + 2) * b_row + 64) * 2;
    return p;
}
}  // namespace old

// ---- check mode ------------------------------------------------------------------------------------------------------------------------
static long bad = 0, cases = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond) && ++bad <= 20) {                                       \
            printf("FAILED %s:", #cond);                                    \
            printf(" " __VA_ARGS__);                                        \
            printf("\n");                                                   \
        }                                                                   \
    } while (0)

static int check() {
    const int strides[3][2] = {{1, 1}, {1, 2}, {2, 2}};
    const int edges[12] = {15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129};
    const char* forces[5] = {nullptr, "22", "42", "22s", "64"};
    // conv3d_kernel: Cin across the chunk sizes, Cout across the NT boundaries (16 | 32, 48 -> 4 | 64), every force value
    for (const auto& st : strides)
    for (const char* force : forces)
    for (int B : {1, 2})
    for (int Cin : {4, 8, 12, 16, 64})
    for (int Cout : {8, 16, 24, 32, 40, 48, 64})
    for (int Di = 1; Di <= 5; ++Di)
    for (int Hi : edges)
    for (int Wi : edges) {
        const int sd = st[0], shw = st[1];
        ++cases;
        const Conv3dPlan p = conv3d_plan(B, Cin, Cout, Di, Hi, Wi, sd, shw, force);
        const old::Launch o = old::conv3d_fwd(B, Cin, Cout, Di, Hi, Wi, sd, shw, force);
#define WHERE "conv B=%d Cin=%d Cout=%d in=[%d,%d,%d] stride=(%d,%d) force=%s", B, Cin, Cout, Di, Hi, Wi, sd, shw, force ? force : "-"
        CHECK(p.NT == o.NT && p.NP == o.NP && p.TD == o.TD && p.TH == o.TH && p.MT == o.MT && p.CC == o.CC, WHERE);
        CHECK(p.lds == o.lds && p.gx == o.gx && p.gy == o.gy && p.gz == o.gz, WHERE);
        CHECK(p.Do == (Di - 1) / sd + 1 && p.Ho == (Hi - 1) / shw + 1 && p.Wo == (Wi - 1) / shw + 1, WHERE);
        CHECK(p.nsplit == mvs::ceil_div(nt_of(Cout), o.NT) && p.chunks == (Cin + o.CC - 1) / o.CC, WHERE);
        const ConvTile t = conv_tile(p.form);
        CHECK(t.TD == o.TD && t.TH == o.TH && t.MT == o.MT && ((p.form == ConvForm::F22 || p.form == ConvForm::F42) ? o.NT == nt_of(Cout) : o.NT == 1), WHERE);
        CHECK(p.form != ConvForm::F42 || sd == 1, WHERE);                      // the 4x2-row form is built for stride-1 depth only
#undef WHERE
    }
    // deconv3d_kernel: input widths around the 32-column block, every depth / row parity
    for (int sd : {1, 2})
    for (int B : {1, 2, 3})
    for (int Cin : {4, 8, 12, 16, 24, 64})
    for (int Cout : {8, 16, 24, 32, 40, 48, 64})
    for (int Di = 1; Di <= 5; ++Di)
    for (int Hi : {1, 2, 3, 4, 5, 15, 16, 17})
    for (int Wi : {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129}) {
        ++cases;
        const Deconv3dPlan p = deconv3d_plan(B, Cin, Cout, Di, Hi, Wi, sd);
        bool s1;
        const old::Launch o = old::deconv3d_fwd(B, Cout, Di, Hi, Wi, sd, &s1);
#define WHERE "deconv B=%d Cin=%d Cout=%d in=[%d,%d,%d] sd=%d", B, Cin, Cout, Di, Hi, Wi, sd
        CHECK(p.s1 == s1 && p.NT == o.NT && p.lds == o.lds && p.gx == o.gx && p.gy == o.gy && p.gz == o.gz, WHERE);
        CHECK(p.Do == Di * sd && p.Ho == Hi * 2 && p.Wo == Wi * 2 && p.chunks == (Cin + old::CC_DECONV - 1) / old::CC_DECONV, WHERE);
        CHECK(p.TWI == 32 && p.THI == 2 && p.TDI == (sd == 1 ? 2 : 1), WHERE);
#undef WHERE
    }
    // wino_conv3d_kernel: the predicate on both sides of each of its terms, MVS_WINO_NT unset / 1 / 2 / 3
    for (int env_nt : {0, 1, 2, 3})
    for (int B : {1, 3})
    for (int Cin : {0, 2, 4, 6, 8, 12, 64})
    for (int Cout : {8, 16, 24, 32, 48, 64, 80})
    for (int D : {0, 1, 3})
    for (int H : {0, 1, 2, 7, 8, 9, 16, 17})
    for (int W : {0, 2, 4, 6, 28, 31, 32, 33, 36, 64, 68, 128, 132}) {
        ++cases;
        const WinoPlan p = wino_plan(B, Cin, Cout, D, H, W, env_nt);
#define WHERE "wino B=%d Cin=%d Cout=%d [%d,%d,%d] env_nt=%d", B, Cin, Cout, D, H, W, env_nt
        CHECK(p.supported == (old::wino_supported(Cin, Cout, D, H, W) != 0) && wino_supported(Cin, Cout, D, H, W) == p.supported, WHERE);
        if (!p.supported) continue;
        const old::Launch o = old::wino_fwd(B, Cout, D, H, W, env_nt);
        CHECK(p.NT == o.NT && p.ngroups == o.NP && p.gx == o.gx && p.gy == o.gy && p.gz == o.gz && p.chunks == Cin / 4, WHERE);
#undef WHERE
    }
    CHECK(!wino_supported(4, 16, 1024, 1024, 128) && wino_supported(4, 16, 1024, 1024, 124), "wino: the 2 GiB window");
    // wgrad_tiled_kernel / wgrad_kernel: CA across MT, widths around SEG, heights around TH
    for (int shw : {1, 2})
    for (int nbatch : {1, 2, 3})
    for (int CA : {1, 8, 16, 17, 24, 32, 33, 40, 48, 49, 64})
    for (int CB : {1, 3, 4, 5, 8, 64, 256})
    for (int Dp = 1; Dp <= 5; ++Dp)
    for (int Hp : {1, 2, 3, 4, 5, 7, 8, 9, 13, 17})
    for (int Wp : {1, 8, 31, 32, 33, 36, 63, 64, 65, 68, 127, 128, 129}) {
        ++cases;
        const WgradTiledPlan p = wgrad_tiled_plan(nbatch, CA, CB, Dp, Hp, Wp, shw);
        const old::WgLaunch o = old::conv3d_wgrad(nbatch, CA, CB, Dp, Hp, Wp, shw);
#define WHERE "wgrad n=%d CA=%d CB=%d [%d,%d,%d] shw=%d", nbatch, CA, CB, Dp, Hp, Wp, shw
        CHECK(p.MT == o.MT && p.TH == o.TH && p.SEG == o.SEG && p.nchunk == o.nchunk && p.ntiles == o.ntiles && p.gy == o.gy, WHERE);
        CHECK(p.hblocks == (Hp + o.TH - 1) / o.TH && p.wblocks == (Wp + o.SEG - 1) / o.SEG, WHERE);
        const WgradV1Plan v = wgrad_v1_plan(nbatch, CA, CB, Dp, Hp);
        const old::WgLaunch w = old::conv3d_wgrad_v1(nbatch, CA, CB, Dp, Hp);
        CHECK(v.MT == w.MT && v.nchunk == w.nchunk && v.rows == w.ntiles && v.gy == w.gy, WHERE);
#undef WHERE
    }
    // bf16_wgrad_kernel: the channel counts the library takes, heights around PH, widths around the 16-column patch, alone and grouped
    for (int grouped = 0; grouped <= 1; ++grouped)
    for (int shw : {1, 2})
    for (int nbatch : {1, 2, 3})
    for (int CA : {8, 16, 32, 64})
    for (int CB : {8, 16, 32, 64})
    for (int Dp : {1, 2, 3, 4, 5, 8, 32})
    for (int Hp : {1, 2, 3, 4, 5, 7, 8, 9, 17, 40})
    for (int Wp : {1, 15, 16, 17, 33, 64, 208}) {
        ++cases;
        const mvsplan::WgradPlan p = mvsplan::wgrad_plan(nbatch, CA, CB, Dp, Hp, Wp, shw, grouped != 0);
        const old::WgradPlan o = old::wgrad_plan(nbatch, CA, CB, Dp, Hp, Wp, shw, grouped != 0);
#define WHERE "bf16 wgrad n=%d CA=%d CB=%d [%d,%d,%d] shw=%d grouped=%d", nbatch, CA, CB, Dp, Hp, Wp, shw, grouped
        CHECK(p.PH == o.PH && p.npr == o.npr && p.npc == o.npc && p.npatch == o.npatch && p.dseg == o.dseg && p.nseg == o.nseg, WHERE);
        CHECK(p.TA == o.TA && p.TB == o.TB && p.gy == o.gy && p.blocks == o.blocks && p.lds == o.lds, WHERE);
        CHECK(p.blocks == mvsplan::wgrad_plan(nbatch, CA, CB, Dp, Hp, Wp, 1, grouped != 0).blocks, WHERE);      // the workspace is sized without the stride
#undef WHERE
    }
    CHECK(mvsplan::WG_PW == old::WG_PW && mvsplan::WG_RING_B == old::WG_RING_B, "bf16 wgrad constants");
    if (cases < 10000) { printf("only %ld cases swept\n", cases); ++bad; }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

// ---- print mode ------------------------------------------------------------------------------------------------------------------------
static int print_plans() {
    char line[512], kind[32], word[32];
    int a[10];
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%31s", kind) != 1) continue;
        const char* rest = line + (strstr(line, kind) - line) + strlen(kind);
        if (!strcmp(kind, "conv") && sscanf(rest, "%d %d %d %d %d %d %d %d %31s", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, word) == 9) {
            const Conv3dPlan p = conv3d_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], strcmp(word, "-") ? word : nullptr);
            printf("form=%s NT=%d TD=%d TH=%d MT=%d TW=%d CC=%d NP=%d nsplit=%d Do=%d Ho=%d Wo=%d grid=%u,%u,%u nblocks=%lld chunks=%d lds=%zu\n",
                   conv_form_name(p.form), p.NT, p.TD, p.TH, p.MT, 16 * p.MT, p.CC, p.NP, p.nsplit, p.Do, p.Ho, p.Wo, p.gx, p.gy, p.gz,
                   (long long)p.gx * p.gy * p.gz, p.chunks, p.lds);
        } else if (!strcmp(kind, "conv_tile") && sscanf(rest, "%31s", word) == 1) {
            bool known = false;
            for (ConvForm f : {ConvForm::F22, ConvForm::F42, ConvForm::F22S64, ConvForm::F22S})
                if (!strcmp(word, conv_form_name(f))) {
                    const ConvTile t = conv_tile(f);
                    printf("form=%s TD=%d TH=%d MT=%d TW=%d\n", word, t.TD, t.TH, t.MT, 16 * t.MT);
                    known = true;
                }
            if (!known) printf("error=form\n");
        } else if (!strcmp(kind, "deconv") && sscanf(rest, "%d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6) == 7) {
            const Deconv3dPlan p = deconv3d_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
            printf("route=%s NT=%d TWI=%d THI=%d TDI=%d Do=%d Ho=%d Wo=%d grid=%u,%u,%u chunks=%d lds=%zu\n", p.s1 ? "s1" : "deconv3d_kernel", p.NT,
                   p.TWI, p.THI, p.TDI, p.Do, p.Ho, p.Wo, p.gx, p.gy, p.gz, p.chunks, p.lds);
        } else if (!strcmp(kind, "wino") && sscanf(rest, "%d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6) == 7) {
            const WinoPlan p = wino_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
            printf("supported=%s NT=%d ngroups=%d grid=%u,%u,%u chunks=%d\n", p.supported ? "true" : "false", p.NT, p.ngroups, p.gx, p.gy, p.gz, p.chunks);
        } else if (!strcmp(kind, "wgrad") && sscanf(rest, "%d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6) == 7) {
            const WgradTiledPlan p = wgrad_tiled_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
            printf("MT=%d SHW=%d TH=%d SEG=%d nchunk=%d hblocks=%d wblocks=%d ntiles=%lld gy=%lld\n", p.MT, a[6], p.TH, p.SEG, p.nchunk, p.hblocks,
                   p.wblocks, p.ntiles, p.gy);
        } else if (!strcmp(kind, "wgrad_v1") && sscanf(rest, "%d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4) == 5) {
            const WgradV1Plan p = wgrad_v1_plan(a[0], a[1], a[2], a[3], a[4]);
            printf("MT=%d nchunk=%d rows=%d gy=%d\n", p.MT, p.nchunk, p.rows, p.gy);
        } else if (!strcmp(kind, "bf16_conv") &&
                   sscanf(rest, "%d %d %d %d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8, a + 9) == 10) {
            const mvsplan::ConvPlan p = mvsplan::conv_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]);
            printf("Do=%d Ho=%d Wo=%d wpar=%s nwchunks=%d items_per_sample=%lld items=%lld ksplit=%s block_rows=%lld samples=%d rows_per_sample=%lld\n",
                   p.Do, p.Ho, p.Wo, p.wpar ? "true" : "false", p.nwchunks, (long long)p.items_per_sample, (long long)p.items,
                   p.ksplit ? "true" : "false", (long long)p.block_rows, p.samples, (long long)p.rows_per_sample);
        } else if (!strcmp(kind, "bf16_wgrad") &&
                   sscanf(rest, "%d %d %d %d %d %d %d %d", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7) == 8) {
            const mvsplan::WgradPlan p = mvsplan::wgrad_plan(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7] != 0);
            printf("PH=%d npr=%d npc=%d npatch=%d dseg=%d nseg=%d TA=%d TB=%d gy=%d blocks=%d lds=%zu\n", p.PH, p.npr, p.npc, p.npatch, p.dseg,
                   p.nseg, p.TA, p.TB, p.gy, p.blocks, p.lds);
        } else if (!strcmp(kind, "bf16_consts")) {
            int ksplit_items = 0;                                  // the largest launch that still splits K: what MVS_BF16_KSPLIT_ITEMS holds here
            while (ksplit_items < (1 << 20) && mvsplan::conv_ksplit(32, ksplit_items + 1, 27)) ++ksplit_items;
            printf("KSPLIT_ITEMS=%d WG_PW=%d WG_RING_B=%zu\n", ksplit_items, mvsplan::WG_PW, mvsplan::WG_RING_B);
        } else {
            printf("error=request\n");
        }
        fflush(stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return check();
    if (argc == 2 && !strcmp(argv[1], "print")) return print_plans();
    fprintf(stderr, "usage: %s [print]\n", argv[0]);
    return 2;
}
