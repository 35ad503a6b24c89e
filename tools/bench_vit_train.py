#!/usr/bin/env python
"""Cost of fine-tuning the DINO ViT ("fix": false) at 640 x 512, 5 views (the ViT sees 320 x 256: 321 tokens per view): the ViT's training
forward and forward + backward (mvsformer_amd/vit.py ``_ViTTrainFn``), and one DINOMVSNet training step (forward, ce_loss_stage4, backward)
with fix=False against fix=True, and ``vit_train_peak_mb``: the peak device memory of one ViT forward + backward.  ``MVS_VIT_TRAIN_FLASH=0``
selects the materialized attention, so one run per setting is the A/B.  Median of --steps timed repetitions after --warmup; prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--vit-only", action="store_true", help="skip the two DINOMVSNet steps")
    args = ap.parse_args()
    import mvsformer_amd as m
    from mvsformer_amd import losses, synth
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    V, H, W = args.views, args.height, args.width
    vit = m.vit_small(patch_size=16, qk_scale="default").to(dev).train()
    x = torch.rand(V, 3, H // 2, W // 2, device=dev)
    params = list(vit.parameters())

    def vit_fwd():
        with torch.no_grad():
            vit.forward_with_cls_att(x)

    def vit_fwd_bwd():
        tok, att = vit.forward_with_cls_att(x)
        torch.autograd.grad(tok.sum() + att.sum(), params)

    # MVS_VIT_TRAIN_FLASH=0: the materialized attention (P saved); unset / 1: the flash pair (mvsformer_amd/vit.py reads it per call)
    res = {"views": V, "height": H, "width": W, "tokens_per_view": (H // 32) * (W // 32) + 1,
           "vit_train_flash": os.environ.get("MVS_VIT_TRAIN_FLASH", "1") != "0"}
    res["vit_train_fwd_ms"] = _time(vit_fwd, args.steps, args.warmup)
    res["vit_train_fwd_bwd_ms"] = _time(vit_fwd_bwd, args.steps, args.warmup)
    # peak of one forward + backward over the level before it (the saved activations + the backward's transients)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    vit_fwd_bwd()
    torch.cuda.synchronize()
    res["vit_train_peak_mb"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    res["vit_bwd_over_fwd"] = (res["vit_train_fwd_bwd_ms"] - res["vit_train_fwd_ms"]) / res["vit_train_fwd_ms"]
    if args.vit_only:
        print(json.dumps(res))
        return
    _, proj, dv, scene = synth.make_inputs(V, H, W, seed=1)
    proj = {k: v.to(dev) for k, v in proj.items()}
    dv = dv.to(dev)
    imgs = torch.rand(1, V, 3, H, W, device=dev)
    gts = {"stage%d" % (i + 1): synth.plane_depth(scene, s).to(torch.float32).unsqueeze(0).to(dev) for i, s in enumerate((8, 4, 2, 1))}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}
    for fix in (True, False):
        net = m.DINOMVSNet(dict(fix=fix, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4],
                                feat_chs=[8, 16, 32, 64], depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
                                vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384,
                                              out_ch=64, att_fusion=True, nhead=6, vit_path="")))
        net = net.to(dev).train()
        ps = [p for p in net.parameters()]

        def step():
            out = net(imgs, proj, dv, tmp=[5.0, 5.0, 5.0, 1.0])
            ls = losses.ce_loss_stage4(out, gts, masks, [1.0, 1.0, 1.0, 1.0], inverse_depth=True)
            torch.autograd.grad(sum(ls.values()), [p for p in ps if p.requires_grad], allow_unused=True)

        res["step_fix_%s_ms" % str(fix).lower()] = _time(step, args.steps, args.warmup)
        del net
    res["step_fix_false_minus_true_ms"] = res["step_fix_false_ms"] - res["step_fix_true_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
