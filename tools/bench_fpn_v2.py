#!/usr/bin/env python
"""The fused full-resolution tail of FPNDecoderV2 (csrc/fpn_v2_tail.hip) against the GEMM route (MVS_FPN_V2_TAIL=0), both in one process on
the same inputs: (a) the tail alone, (b) the whole ``FPNDecoderV2.forward``, (c) images -> depth with ``multi_scale=True`` beside
``multi_scale=False``.  Warm-up, then the median (and the spread) of repeated timed regions of several launches each.  One JSON line.

    python tools/bench_fpn_v2.py [--views 5] [--height 1152] [--width 1536] [--regions 9] [--iters 10] [--no-e2e]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvsformer_amd as m  # noqa: E402
from mvsformer_amd import fpn, ops, synth, vit  # noqa: E402
from mvsformer_amd.cascade import randomize_bn_  # noqa: E402


def regions(fn, n_regions, iters, warmup=3):
    """ms per call: [median, min, max] over ``n_regions`` event-timed regions of ``iters`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n_regions):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def model_args(multi_scale):
    return dict(fix=True, depth_type="ce", fusion_type="cnn", inverse_depth=True, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
                depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=multi_scale,
                vit_args=dict(twin=False, rescale=0.5, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                              att_fusion=True, nhead=6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--height", type=int, default=1152)
    ap.add_argument("--width", type=int, default=1536)
    ap.add_argument("--regions", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W = a.views, a.height, a.width
    h, w = H // 2, W // 2
    torch.manual_seed(0)
    res = dict(device=torch.cuda.get_device_name(0), N=N, h=h, w=w, unit="ms per call: [median, min, max] of %d regions x %d calls" % (a.regions, a.iters))

    dec = m.FPNDecoderV2([8, 16, 32, 64]).eval()
    randomize_bn_(dec, seed=1)
    dec = dec.to(dev)
    # (a) the tail alone
    out3 = torch.randn(N, h, w, 16, device=dev)
    c01 = torch.randn(N, H, W, 8, device=dev)
    fold_up, fold_out = vit._fold(dec.upsample3[0], dec.upsample3[1]), vit._fold(dec.out4[0], dec.out4[1])
    prep = ops.fpn_v2_tail_prepare(vit._f(dec.upsample3[0].weight), fold_up, vit._f(dec.out4[0].weight), fold_out)
    wm, w3 = vit._convT_matrices(dec.upsample3[0].weight), vit._conv3_matrix(dec.out4[0].weight, 8)

    def gemm_route():
        up = vit.VITDecoderStage4Single._up(out3, wm, fold_up, fpn.ACT_RELU_GEMM)
        return fpn.FPNDecoderV2._conv3(up.add_(c01), w3, fold_out)
    diff = (ops.fpn_v2_tail(out3, c01, *prep) - gemm_route()).abs().max().item()
    res["a_tail_fused"] = regions(lambda: ops.fpn_v2_tail(out3, c01, *prep), a.regions, a.iters)
    res["a_tail_gemm_route"] = regions(gemm_route, a.regions, a.iters)
    res["a_max_abs_difference"] = diff
    res["a_fused_GBps_at_20_floats_per_pixel"] = round(20 * 4 * N * H * W / (res["a_tail_fused"][0] * 1e-3) / 1e9, 1)
    del out3

    # (b) the whole decoder
    c = [8, 16, 32, 64]
    convs = [c01.permute(0, 3, 1, 2)] + [torch.randn(N, c[i], H >> i, W >> i, device=dev) for i in range(1, 4)]
    vits = [torch.randn(N, c[3 - i], (H >> 3) << i, (W >> 3) << i, device=dev) for i in range(3)]
    for v in ("1", "0"):
        os.environ["MVS_FPN_V2_TAIL"] = v
        res["b_decoder_v2_tail=%s" % v] = regions(lambda: dec(*convs, *vits), a.regions, max(2, a.iters // 2))
    os.environ.pop("MVS_FPN_V2_TAIL")
    del convs, vits, c01, dec
    torch.cuda.empty_cache()

    # (c) images -> depth, single stream
    if not a.no_e2e:
        _, proj, dv, _ = synth.make_inputs(N, H, W, seed=0, device=dev)
        imgs = synth.render_features(synth.make_scene(N, H, W, 0), 1, 3, noise=0.02, device=dev, dtype=torch.float32)
        tmp = [5.0, 5.0, 5.0, 1.0]
        for ms in (False, True):
            net = m.DINOMVSNet(model_args(ms)).eval()
            randomize_bn_(net, seed=1)
            net = net.to(dev)
            res["c_images_to_depth_multi_scale=%s" % ms] = regions(lambda: net(imgs, proj, dv, tmp=tmp), 5, 3, warmup=2)
            if ms:
                res["c_extract_features_multi_scale=True"] = regions(lambda: net.extract_features(imgs), 5, 3, warmup=1)
            del net
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
