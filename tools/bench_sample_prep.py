#!/usr/bin/env python
"""Sample preparation of one config-3 training batch, device against host, phase by phase (needs the GPU):

    python tools/bench_sample_prep.py [--repeats 5] [--threads 16] [--out profiles/sample_prep_bench.json]

B = 1, V = 5, 1600x1200 sources, a 640x512 crop, augmentation on, K = 4 crop candidates: the batch the captured training step of
BASELINE configs[2] consumes.  The device side is timed per C entry of csrc/sample_prep.hip (host clock with a synchronisation on both
sides; the jitter entry is its zero / statistics / tail launches together), the table upload, and ``prepare_train_batch`` as a whole.
The host side is the reference's pipeline on the same bytes and the same drawn parameters: PIL for the four colour steps, the numpy
restatements of tests/sample_prep_util.py for the rest (area resize, nearest resize, pyramid, matrices, tail), the views spread over
``--threads`` threads.  The two sides alternate, repeat by repeat, and every repeat is kept.  The uploaded decoded bytes (28.8 MB of
images) are not part of either side's time: both start from the decoder's output where it lies.
"""
import argparse
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import sample_prep_util as u  # noqa: E402
from mvsformer_amd import ops, sample_prep as sp  # noqa: E402

AUG = dict(brightness=0.2, contrast=0.1, saturation=0.1, hue=0.05, min_gamma=0.7, max_gamma=1.5)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def host_view(img, rs, off, crop, p):
    H0, W0 = img.shape[:2]
    rh, rw = (int(H0 * rs), int(W0 * rs)) if rs != 1.0 else (H0, W0)
    c = u.area_resize(img, rh, rw)[off[0]:off[0] + crop[0], off[1]:off[1] + crop[1]]
    return u.tail(u.jitter_pil(np.ascontiguousarray(c), p.fn_idx, p.factors, p.enabled), p.gamma)


def host_batch(inp, p, crop, dmin, dint, nd, pool):
    imgs, depth, mask, intr, extr = inp
    t = {}
    t0 = time.perf_counter()
    oy, ox, ok, _ = u.accept(mask[0], p.resize_scales[0], p.candidates, *crop)
    offs = [(oy, ox)] + [(oy, ox) if o is None else o for o in p.src_offsets]
    t["accept"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    d, m = u.crop_maps(depth[0], mask[0], p.resize_scales[0], oy, ox, *crop)
    proj = u.proj_matrices(intr[0], extr[0], p.resize_scales, offs)
    dv = u.depth_values(dmin, dint, nd)
    t["geometry"] = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    views = list(pool.map(lambda v: host_view(imgs[0, v], p.resize_scales[v], offs[v], crop, p), range(imgs.shape[1])))
    t["images_resize_crop_jitter_tail"] = 1e3 * (time.perf_counter() - t0)
    t["total"] = sum(t.values())
    return dict(imgs=np.stack(views), depth=d, mask=m, proj=proj, dv=dv), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--src", default="1200,1600")
    ap.add_argument("--crop", default="512,640")
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample_prep_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_prep.py runs the MI355X path: no GPU")
    dev = torch.device("cuda:0")
    hw, crop = tuple(int(x) for x in a.src.split(",")), tuple(int(x) for x in a.crop.split(","))
    V, K, nd, dmin, dint = a.views, 4, 192, 425.0, 2.5 * 1.06
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:hw[0], 0:hw[1]]
    base = (128 + 90 * np.sin(xx / 37.0) * np.cos(yy / 23.0)).astype(np.float32)
    imgs = np.clip(base[None, None, ..., None] + rng.normal(0, 25, (1, V) + hw + (3,)), 0, 255).astype(np.uint8)
    depth = rng.uniform(450, 900, (1,) + hw).astype(np.float32)
    mask = ((yy - hw[0] / 2) ** 2 + (xx - hw[1] / 2) ** 2 < (0.45 * hw[0]) ** 2).astype(np.uint8)[None] * 255
    intr = np.tile(np.array([[2892.33, 0, 823.205], [0, 2883.18, 619.071], [0, 0, 1]], np.float32), (1, V, 1, 1))
    extr = np.tile(np.eye(4, dtype=np.float32), (1, V, 1, 1))
    inp = (imgs, depth, mask, intr, extr)
    dev_in = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in inp]
    L = sp.arange_length(dmin, dint, nd)
    tb = sp.TrainTables(1, V, K, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), B=1, V=V, src_hw=list(hw), crop_hw=list(crop), K=K, threads=a.threads, repeats=[],
               note="ms per repeat, host clock; device and host alternate; the upload of the decoded bytes is in neither")
    pool = ThreadPoolExecutor(a.threads)
    torch.set_num_threads(a.threads)
    for r in range(a.repeats + 1):                                # repeat 0 warms both sides up and is kept, marked
        random.seed(r), np.random.seed(r), torch.manual_seed(r)
        p = sp.draw_train_params(0, list(range(1, 11)), V, crop, src_hw=hw, augment=True, aug_args=AUG, resize_range=(1.0, 1.2), K=K)
        ms = {}
        _, ms["tables_fill_and_copy"] = timed(lambda: tb.write([p], hw, [dmin], [dint]))
        chosen, ms["mvs_prep_accept"] = timed(lambda: ops.prep_accept(dev_in[2], tb.ptab, tb.cand, crop, chosen=tb.chosen))
        _, ms["mvs_prep_geometry"] = timed(lambda: ops.prep_geometry(dev_in[1], dev_in[2], tb.ptab, chosen, dev_in[3], dev_in[4], tb.drange, crop, L))
        u8, ms["mvs_prep_area_crop"] = timed(lambda: ops.prep_area_crop(dev_in[0], tb.ptab, chosen, crop))
        _, ms["mvs_prep_jitter_tail"] = timed(lambda: ops.prep_jitter_tail(u8, tb.jtab, has_contrast=tb.enabled[1]))
        batch, ms["prepare_train_batch"] = timed(lambda: sp.prepare_train_batch(*dev_in, tb, crop, L, augment=True))
        want, host_ms = host_batch(inp, p, crop, dmin, dint, nd, pool)
        got = batch["imgs"][0].cpu().numpy()
        rep = dict(repeat=r, warmup=r == 0, resize_scales=p.resize_scales, device_ms=ms, host_ms=host_ms,
                   max_abs_image_difference=float(np.abs(got.astype(np.float64) - want["imgs"]).max()),
                   maps_equal=bool(all(np.array_equal(batch["depth"][s][0].cpu().numpy(), want["depth"][s]) and
                                       np.array_equal(batch["proj_matrices"][s][0].cpu().numpy(), want["proj"][s]) for s in want["proj"])))
        res["repeats"].append(rep)
        print(json.dumps(rep))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
