// Stand-alone host check of mvsplan::conv_plan / conv_rows_workspace_bytes (csrc/bf16_conv_plan.h) against the three hand-copied formula
// sets they replaced - bf16_conv3d_impl, mvs_bf16_conv3d_bn_fwd and mvs_bf16_conv3d_bnbwd of csrc/bf16_train.hip, and the two
// *_workspace_bytes functions - kept here verbatim as the oracle.  The convolution kernel writes block_rows (or items) rows of 2*Cout floats
// into a workspace sized by the other formula, so a disagreement is an out-of-bounds write on the device: this is checked on the host, over
// every tile edge of the plan.  Built with AddressSanitizer and UBSan on the host side (there is no device code here) and run by
// tests/test_abi.py; exits 0 when every case agrees.  Not part of the library.
#include <stdint.h>
#include <stdio.h>

#include "../mvsformer_amd/csrc/bf16_conv_plan.h"

// ---- the parent's formulas, verbatim -------------------------------------------------------------------------------------------------
static bool old_conv_ksplit(int cin, int items, int taps) {
    static const int lim = mvs::env_int("MVS_BF16_KSPLIT_ITEMS", 768);
    return taps == 27 && cin >= 32 && items <= lim;
}
struct OldImpl { int Do, Ho, Wo, nwchunks, items, stats_rows, rows_per_sample_reduce; bool wpar, launch_ks; };
static OldImpl old_impl(int B, int Cin, int Di, int Hi, int Wi, int gather, int sd, int shw, int taps) {
    OldImpl a;
    if (gather == 0) a.Do = (Di - 1) / sd + 1, a.Ho = (Hi - 1) / shw + 1, a.Wo = (Wi - 1) / shw + 1;
    else a.Do = Di * sd, a.Ho = Hi * shw, a.Wo = Wi * shw;
    const bool wpar = gather == 1 && shw == 2;
    a.nwchunks = wpar ? (a.Wo + 127) / 128 : (a.Wo + 63) / 64;
    const int64_t items = (int64_t)B * a.Do * a.Ho * a.nwchunks * (wpar ? 2 : 1);
    a.items = (int)items;
    a.stats_rows = (int)(old_conv_ksplit(Cin, (int)items, taps) ? items : (items + 3) / 4);      // one row per BLOCK
    a.launch_ks = taps == 27 && old_conv_ksplit(Cin, a.items, 27);                                 // launch_conv (the taps = 9 launch never splits)
    a.rows_per_sample_reduce = (int)(items / B);                                                   // launch_partials_reduce_grouped
    a.wpar = wpar;
    return a;
}
struct OldRows { int Do, Ho, Wo, nrows, rps, samples; int64_t ips; bool ks, accepted; };
static OldRows old_bn_fwd(int B, int Cin, int Di, int Hi, int Wi, int gather, int sd, int shw, int taps, int groups) {
    OldRows r;
    int Do, Ho, Wo;
    if (gather == 0) Do = (Di - 1) / sd + 1, Ho = (Hi - 1) / shw + 1, Wo = (Wi - 1) / shw + 1;
    else Do = Di * sd, Ho = Hi * shw, Wo = Wi * shw;
    const int64_t ips = (gather == 1 && shw == 2) ? (int64_t)Do * Ho * ((Wo + 127) / 128) * 2 : (int64_t)Do * Ho * ((Wo + 63) / 64);   // work items per sample
    const bool ks = old_conv_ksplit(Cin, (int)(ips * B), taps);
    r.accepted = B == 1 || groups == 1 || ks || ips % 4 == 0;
    const bool one = B == 1 || groups == 1;                                  // all rows are one group's
    const int nrows = ks ? (int)(ips * B) : (int)((ips * B + 3) / 4), rps = one ? nrows : (int)(ks ? ips : ips / 4);
    r.Do = Do, r.Ho = Ho, r.Wo = Wo, r.ips = ips, r.ks = ks, r.nrows = nrows, r.rps = rps, r.samples = one ? 1 : B;
    return r;
}
static OldRows old_bnbwd(int B, int Cin, int Di, int Hi, int Wi, int gather, int sd, int shw, int taps) {
    OldRows r;
    int Do, Ho, Wo;
    if (gather == 0) Do = (Di - 1) / sd + 1, Ho = (Hi - 1) / shw + 1, Wo = (Wi - 1) / shw + 1;
    else Do = Di * sd, Ho = Hi * shw, Wo = Wi * shw;
    const int64_t ips = (gather == 1 && shw == 2) ? (int64_t)Do * Ho * ((Wo + 127) / 128) * 2 : (int64_t)Do * Ho * ((Wo + 63) / 64);
    const bool ks = old_conv_ksplit(Cin, (int)(ips * B), taps);
    r.accepted = B == 1 || ks || ips % 4 == 0;
    const int nrows = ks ? (int)(ips * B) : (int)((ips * B + 3) / 4), rps = B == 1 ? nrows : (int)(ks ? ips : ips / 4);
    r.Do = Do, r.Ho = Ho, r.Wo = Wo, r.ips = ips, r.ks = ks, r.nrows = nrows, r.rps = rps, r.samples = B;
    return r;
}
static int64_t old_stats_workspace_bytes(int B, int Cout, int Do, int Ho, int Wo) {
    if (!mvsplan::chan_ok(Cout) || B < 1 || Do < 1 || Ho < 1 || Wo < 1) return -1;
    return (int64_t)B * Do * Ho * ((Wo + 127) / 128) * 2 * 2 * Cout * (int64_t)sizeof(float);      // >= the work items of either form
}
static int64_t old_bn_fwd_workspace_bytes(int B, int Cout, int Do, int Ho, int Wo) {
    if (!mvsplan::chan_ok(Cout) || B < 1 || Do < 1 || Ho < 1 || Wo < 1) return -1;
    const int64_t items = (int64_t)B * Do * Ho * ((Wo + 127) / 128) * 2;           // >= the work items of either form (see bf16_conv3d_impl)
    return items * 2 * Cout * (int64_t)sizeof(float);      // one row per block: up to one block per work item (the K-split form)
}

// ---- the sweep -----------------------------------------------------------------------------------------------------------------------
static long bad = 0, cases = 0;
#define CHECK(cond)                                                                                                                          \
    do {                                                                                                                                     \
        if (!(cond)) {                                                                                                                       \
            if (++bad <= 20)                                                                                                                 \
                printf("FAILED %s: B=%d Cin=%d in=[%d,%d,%d] gather=%d stride=(%d,%d) taps=%d groups=%d\n", #cond, B, Cin, Di, Hi, Wi, gather, sd, \
                       shw, taps, groups);                                                                                                   \
        }                                                                                                                                    \
    } while (0)

int main() {
    const int strides[3][2] = {{1, 1}, {1, 2}, {2, 2}}, wis[10] = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129}, dhs[3] = {1, 2, 5};
    for (int gather = 0; gather <= 1; ++gather)
    for (const auto& st : strides)
    for (int taps : {27, 9})
    for (int Cin : {8, 16, 32, 64})
    for (int B : {1, 2, 4, 6})
    for (int groups : {1, 2})
    for (int Di : dhs)
    for (int Hi : dhs)
    for (int Wi : wis) {
        const int sd = st[0], shw = st[1];
        if (taps == 9 && !(gather == 0 && sd == 1 && shw == 1 && Cin <= 16)) continue;      // where the 2-D kernel is built
        if (B % groups) continue;                                                           // every entry point requires it
        ++cases;
        const mvsplan::ConvPlan p = mvsplan::conv_plan(B, Cin, Di, Hi, Wi, gather, sd, shw, taps, groups);
        // (a) field by field against each old copy
        const OldImpl a = old_impl(B, Cin, Di, Hi, Wi, gather, sd, shw, taps);
        CHECK(p.Do == a.Do && p.Ho == a.Ho && p.Wo == a.Wo && p.wpar == a.wpar && p.nwchunks == a.nwchunks);
        CHECK(p.items == a.items && p.block_rows == a.stats_rows && p.ksplit == a.launch_ks && p.items_per_sample == a.rows_per_sample_reduce);
        CHECK(p.ksplit == mvsplan::conv_ksplit(Cin, (int)p.items, taps));
        const OldRows f = old_bn_fwd(B, Cin, Di, Hi, Wi, gather, sd, shw, taps, groups);
        CHECK(p.Do == f.Do && p.Ho == f.Ho && p.Wo == f.Wo && p.items_per_sample == f.ips && p.ksplit == f.ks && p.block_rows == f.nrows);
        // (c) the forward accepts exactly the shapes it accepted, with the same rows per sample and samples
        CHECK((p.rows_per_sample >= 0) == f.accepted);
        if (f.accepted) CHECK(p.rows_per_sample == f.rps && p.samples == f.samples && p.rows_per_sample * p.samples == p.block_rows);
        // ... and so does the backward form where its old copy accepted (that copy's own, stricter test, written with the plan's fields; the
        // entry point has since taken the forward's test, rows_per_sample >= 0: a one-group batch whose blocks straddle samples runs).  Its old
        // copy walked a one-group batch as B samples of rps rows; the plan walks it as ONE sample of B * rps rows: bf16_rows_reduce_kernel
        // visits row (i / rps) * rps + i % rps = i for i < B * rps either way, so only the pair (rps, samples) differs, not the rows or their order.
        const OldRows w = old_bnbwd(B, Cin, Di, Hi, Wi, gather, sd, shw, taps);
        CHECK(p.items_per_sample == w.ips && p.ksplit == w.ks && p.block_rows == w.nrows);
        CHECK(!w.accepted || p.rows_per_sample >= 0);      // what the entry point tests now (= the forward's f.accepted above) includes the old set
        CHECK(w.accepted || p.rows_per_sample < 0 || (groups == 1 && B > 1));      // ... and adds only one-group batches
        if (w.accepted) {
            CHECK(p.rows_per_sample >= 0 && p.rows_per_sample * p.samples == p.block_rows && (int64_t)w.rps * w.samples == p.block_rows);
            if (groups > 1 || B == 1) CHECK(p.rows_per_sample == w.rps && p.samples == w.samples);
            else CHECK(p.samples == 1 && p.rows_per_sample == (int64_t)w.rps * B);
        }
        // (b) the rows the kernel writes fit the workspace the callers allocate, in both forms
        for (int Cout : {8, 16, 32, 64}) {
            const int64_t ws = mvsplan::conv_rows_workspace_bytes(B, Cout, p.Do, p.Ho, p.Wo);
            CHECK(ws == old_stats_workspace_bytes(B, Cout, p.Do, p.Ho, p.Wo) && ws == old_bn_fwd_workspace_bytes(B, Cout, p.Do, p.Ho, p.Wo));
            CHECK(p.block_rows * 2 * Cout * 4 <= ws);      // one row per block (bn_fwd / bnbwd)
            CHECK(p.items * 2 * Cout * 4 <= ws);           // one row per work item (stats)
        }
    }
    // bad shapes are refused by the size query as before
    bad += mvsplan::conv_rows_workspace_bytes(0, 8, 1, 1, 1) != -1 || mvsplan::conv_rows_workspace_bytes(1, 12, 1, 1, 1) != -1 ||
           mvsplan::conv_rows_workspace_bytes(1, 8, 1, 0, 1) != -1 || mvsplan::conv_rows_workspace_bytes(1, 8, 1, 1, 1) != 2 * 2 * 8 * 4;
    if (cases < 10000) { printf("only %ld cases swept\n", cases); ++bad; }
    printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
