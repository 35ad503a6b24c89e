#!/usr/bin/env python
"""Depth inference over a whole scan with every image through the FPN and the ViT once (``mvsformer_amd.scene.SceneInference``):

    python tools/infer_scan.py --scan SCAN_FOLDER --checkpoint model_best.pth [--config config.json] [--num_view 5] [--numdepth 192]
        [--interval_scale 1.06] [--tmp 5,5,5,1] [--out OUT_FOLDER] [--ply cloud.ply] [--prob_threshold 0.5,0.5,0.5,0.5] [--method pcd]
        [--gt_depth DIR --gt_mask DIR] [--max_h 864 --max_w 1152]

``SCAN_FOLDER`` holds ``images/%08d.jpg|png``, ``cams/%08d_cam.txt`` and ``pair.txt`` (the layout ``general_eval.py`` reads).  ``--out`` gets
the files the reference's ``save_depth`` writes (``depth_est/``, ``confidence/``, ``cams/``, ``images/``: ``tools/fuse_scan.py`` and the
reference's own filter step consume them); ``--ply`` fuses the scan on the device with no file in between.  Without ``--max_h`` /
``--max_w`` images are used as they are: their size must be a multiple of 64 and the intrinsics in the camera files must belong to that
size.  With either flag (the other takes the reference's default, 864 / 1152; both multiples of 64) every image goes through
``scale_mvs_input`` on the device (``mvsformer_amd.sample_prep.prepare_eval_views``: the 8-bit ``INTER_LINEAR`` resize to
``max_w x max_h``, intrinsics rows 0-1 times ``max_w / w`` and ``max_h / h``), so a 1600x1200 DTU scan is accepted and the written
``cams/`` carry the scaled intrinsics, as ``test.py`` writes them.  ``--gt_depth`` / ``--gt_mask`` (with ``--out``): ground truth per reference view, ``DIR/%08d.pfm`` and
``DIR/%08d.png`` (or DTU's ``depth_map_%04d.pfm`` / ``depth_visual_%04d.png``; a mask pixel is valid above 10, as the reference's loader
reads it), already at the images' size - ``OUT_FOLDER/depth_metric.txt`` then holds test.py's seven accuracy entries.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvsformer_amd as m  # noqa: E402
from mvsformer_amd import data_io, metrics, sample_prep  # noqa: E402
from mvsformer_amd.scene import IMAGENET_MEAN, IMAGENET_STD  # noqa: E402

DEFAULT_ARGS = dict(fix=True, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
                    depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
                    vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                                  att_fusion=True, nhead=6))


def depth_values(cam_file, numdepth, interval_scale):
    """general_eval.py:91-104,220: ``depth_min`` / ``depth_interval`` from line 11 of the camera file -> the hypothesis range."""
    with open(cam_file) as f:
        lines = [ln.rstrip() for ln in f.readlines()]
    tok = lines[11].split()
    depth_min, interval = float(tok[0]), float(tok[1])
    if len(tok) >= 3:
        depth_max = depth_min + int(float(tok[2])) * interval
        interval = (depth_max - depth_min) / numdepth
    interval *= interval_scale
    return np.arange(depth_min, interval * (numdepth - 0.5) + depth_min, interval, dtype=np.float32)


def load_gt(depth_dir, mask_dir, vid, dev):
    """-> ``(depth [H,W] fp32, mask [H,W] bool)`` of view ``vid`` on ``dev``."""
    def first(folder, patterns):
        for pat in patterns:
            path = os.path.join(folder, pat.format(vid))
            if os.path.exists(path):
                return path
        raise SystemExit("no ground truth for view %d in %s (%s)" % (vid, folder, " or ".join(p.format(vid) for p in patterns)))
    depth, _ = data_io.read_pfm(first(depth_dir, ("{:0>8}.pfm", "depth_map_{:0>4}.pfm")))
    mask = data_io.read_img(first(mask_dir, ("{:0>8}.png", "depth_visual_{:0>4}.png")))[..., 0] > 10
    return torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(mask)).to(dev)


def scaled_camera(cam_file, src_hw, out_hw):
    """-> the ``[2,4,4]`` camera of ``cam_file`` for an image of ``src_hw`` resized to ``out_hw`` (None: as it is)."""
    cam = data_io._cam_2x4x4(cam_file)
    if out_hw is not None:
        cam[1, :3, :3] = sample_prep.scale_intrinsics(cam[1, :3, :3], src_hw, out_hw)
    return cam


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", required=True)
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--config", default=None, help="the reference's config json (arch.args); default: MVSFormer-P, with multi_scale / att_fusion from the checkpoint's own config")
    ap.add_argument("--num_view", type=int, default=5)
    ap.add_argument("--numdepth", type=int, default=192)
    ap.add_argument("--interval_scale", type=float, default=1.06)
    ap.add_argument("--tmp", default="5,5,5,1")
    ap.add_argument("--out", default=None)
    ap.add_argument("--ply", default=None)
    ap.add_argument("--prob_threshold", default="0.5,0.5,0.5,0.5")
    ap.add_argument("--method", default="pcd", choices=["pcd", "dypcd"])
    ap.add_argument("--combine_conf", action="store_true")
    ap.add_argument("--capacity_views", type=int, default=None)
    ap.add_argument("--max_bank_mb", type=float, default=16384.0)
    ap.add_argument("--extract_batch", type=int, default=4)
    ap.add_argument("--gt_depth", default=None, help="folder of ground-truth depth maps (PFM) at the images' size; with --gt_mask and --out: depth_metric.txt")
    ap.add_argument("--gt_mask", default=None, help="folder of validity masks (PNG, valid above 10)")
    ap.add_argument("--max_h", type=int, default=None, help="resize every image to max_w x max_h as scale_mvs_input does (default with --max_w: 864)")
    ap.add_argument("--max_w", type=int, default=None, help="default with --max_h: 1152")
    a = ap.parse_args(argv)
    if a.max_h is not None or a.max_w is not None:
        a.max_h, a.max_w = a.max_h or 864, a.max_w or 1152
        if a.max_h % 64 or a.max_w % 64 or a.max_h < 64 or a.max_w < 64:
            raise SystemExit("--max_h %d --max_w %d: both must be multiples of 64" % (a.max_h, a.max_w))
    if not a.out and not a.ply:
        raise SystemExit("nothing to do: give --out and / or --ply")
    if bool(a.gt_depth) != bool(a.gt_mask) or (a.gt_depth and not a.out):
        raise SystemExit("--gt_depth and --gt_mask go together and need --out (depth_metric.txt is written there)")
    return a


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("infer_scan.py runs the MI355X path: no GPU")
    dev = torch.device("cuda:0")
    args = json.load(open(a.config))["arch"]["args"] if a.config else dict(DEFAULT_ARGS, vit_args=dict(DEFAULT_ARGS["vit_args"]))
    sd = torch.load(a.checkpoint, map_location="cpu")
    if not a.config:
        # the reference's trainer stores its config in the checkpoint: the flags that change the model's modules and its hypothesis
        # sampling come from there (absent ones as the reference's own constructor reads them, mvsformer_model.py:169-170)
        try:
            ck = sd["config"]["arch"]["args"]
        except (KeyError, TypeError, IndexError):
            ck = None
        if ck is not None:
            args["multi_scale"] = bool(ck.get("multi_scale", False))
            args["inverse_depth"] = bool(ck.get("inverse_depth", False))
            for k in ("att_fusion", "multi_scale_decoder"):
                if k in ck.get("vit_args", {}):
                    args["vit_args"][k] = ck["vit_args"][k]
    net = m.DINOMVSNet(args)
    sd = sd.get("state_dict", sd)
    net.load_state_dict({k[len("module."):] if k.startswith("module.") else k: v for k, v in sd.items()}, strict=True)
    net = net.to(dev).eval()
    pairs = data_io.read_pair_file(os.path.join(a.scan, "pair.txt"))
    ids = []
    for r, srcs in pairs:
        for v in [r] + srcs:
            if v not in ids:
                ids.append(v)
    si = m.SceneInference(net, capacity_views=a.capacity_views, max_bank_mb=a.max_bank_mb, extract_batch=a.extract_batch, combine_conf=a.combine_conf)
    mean, std = np.array(IMAGENET_MEAN, np.float32), np.array(IMAGENET_STD, np.float32)
    t0 = time.perf_counter()
    for v in ids:
        path = data_io._image_path(a.scan, v)
        if path is None:
            raise SystemExit("no images/{:0>8}.jpg (or .png) in {}".format(v, a.scan))
        img = data_io.read_img(path)
        cam_file = os.path.join(a.scan, "cams/{:0>8}_cam.txt".format(v))
        if a.max_h is not None:
            x, _ = sample_prep.prepare_eval_views(torch.from_numpy(np.ascontiguousarray(img)).to(dev)[None], None, a.max_h, a.max_w)
            x, cam = x[0], scaled_camera(cam_file, img.shape[:2], (a.max_h, a.max_w))
        else:
            if img.shape[0] % 64 or img.shape[1] % 64:
                raise SystemExit("%s is %dx%d: H and W must be multiples of 64 (give --max_h / --max_w to resize)" % (path, img.shape[0], img.shape[1]))
            x = torch.from_numpy(np.ascontiguousarray(((img.astype(np.float32) / 255.0 - mean) / std).transpose(2, 0, 1))).to(dev)
            cam = data_io._cam_2x4x4(cam_file)
        si.add_image(v, x, torch.from_numpy(cam).to(dev), torch.from_numpy(depth_values(cam_file, a.numdepth, a.interval_scale)).to(dev))
    si.set_pairs(pairs, num_views=a.num_view)
    th = [float(x) for x in a.prob_threshold.split(",")]
    fusion = m.SceneFusion(a.method, th, combine_conf=a.combine_conf, device="cuda:0") if a.ply else None
    gt = {r: load_gt(a.gt_depth, a.gt_mask, r, dev) for r, _ in pairs} if a.gt_depth else None
    t1 = time.perf_counter()
    si.run(tmp=[float(x) for x in a.tmp.split(",")], fusion=fusion, save_to=a.out, gt=gt)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = dict(views=len(ids), samples=len(pairs), seconds=dict(load=t1 - t0, infer=t2 - t1), bank=si.stats)
    if gt is not None:
        means = si.depth_meter.mean()                        # the scan's one device-to-host copy of the metrics
        os.makedirs(a.out, exist_ok=True)
        metrics.write_depth_metric_txt(os.path.join(a.out, "depth_metric.txt"), means)
        res.update(depth_metrics=means)
    if fusion is not None:
        out = fusion.fuse(want=("records",))
        data_io.write_ply_records(a.ply, out["records"], out["n_points"])
        res.update(n_points=out["n_points"], ply=a.ply)
        res["seconds"]["fuse"] = time.perf_counter() - t2
    print(json.dumps(res))


if __name__ == "__main__":
    main()
