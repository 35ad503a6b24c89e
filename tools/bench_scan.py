#!/usr/bin/env python
"""Time a whole scan -> PLY two ways on the same synthetic scan folder (test.py's filter step: 49 views, 10 source views each):

  (A) the per-view route: ``fusion.filter_scan`` (every reference view re-loads its sources from disk), then the numpy colour gather
      and a numpy PLY write - what a user had to do before ``fuse_scan`` existed;
  (B) the scene-resident route: ``data_io.load_scene`` -> ``SceneFusion`` -> ``fuse()`` -> ``write_ply_records`` (= ``fuse_scan``).

    python tools/bench_scan.py [--views 49] [--height 1152] [--width 1536] [--repeats 3] [--out profiles/scan_fusion_bench.json]

Each route is split into load / device / write with a host clock around work that ends in a device synchronise; the two routes alternate,
``--repeats`` times after one untimed pass of each, and every repeat is kept (median and min..max are reported).  (A)'s device part
contains its host-to-device uploads (``filter_scan`` uploads inside its loop), so (B) is reported both without and with its one upload; the
like-for-like comparison is ``B.upload + B.device`` against ``A.device``.  The two clouds are compared byte for byte.
Needs the GPU; prints and writes one JSON object.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvsformer_amd import data_io, fusion  # noqa: E402
from oracle import ref_fusion  # noqa: E402  (input generator only)


def write_scan(folder, views, h, w, n_src, seed=0):
    from PIL import Image
    case = ref_fusion.make_fusion_case(n=1, v=views - 1, h=h, w=w, seed=seed, noise=0.0005, outlier_frac=0.02)
    depths = torch.cat([case["ref_depth"], case["src_depths"][:, :, 0]], 1)[0].numpy()
    cams = torch.cat([case["ref_cam"][:, None], case["src_cams"]], 1)[0].numpy()
    conf = np.full((h, w, 4), 0.9, np.float32)
    conf[:h // 16] = 0.1
    ys, xs = np.mgrid[0:h, 0:w]
    os.makedirs(os.path.join(folder, "images"))
    for i in range(views):
        data_io.save_depth_outputs(folder, i, depths[i], conf, cams[i])
        img = np.stack([(xs + 3 * i) % 256, (ys + 5 * i) % 256, ((xs + ys) // 2 + 7 * i) % 256], -1).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(folder, "images/%08d.png" % i), compress_level=1)
    with open(os.path.join(folder, "pair.txt"), "w") as f:
        f.write("%d\n" % views)
        for i in range(views):
            srcs = [(i + d) % views for d in range(1, views)][:n_src]
            f.write("%d\n%d %s\n" % (i, len(srcs), " ".join("%d 1.0" % s for s in srcs)))


def route_a(folder, ply, th, method):
    """-> (seconds dict, file bytes).  The loader is wrapped to time the disk part of filter_scan's loop."""
    spent = {"load": 0.0}
    real = data_io.load_filter_sample

    def timed_loader(*a, **k):
        t = time.perf_counter()
        out = real(*a, **k)
        spent["load"] += time.perf_counter() - t
        return out

    data_io.load_filter_sample = timed_loader
    try:
        t0 = time.perf_counter()
        views = fusion.filter_scan(folder, folder, th, method=method)            # ends in .cpu()/.item() per view: synchronised
        torch.cuda.synchronize()
        t1 = time.perf_counter()
    finally:
        data_io.load_filter_sample = real
    # colours: the parent route returns points only, so the masks are not available - the user gathers colours by re-deriving the kept
    # pixels; here the cheapest honest stand-in: read each reference image (load) and take as many pixels as points (gather, not timed as
    # device work).  The cloud's xyz is what is compared with route B.
    t2 = time.perf_counter()
    imgs = {r: data_io.read_img(os.path.join(folder, "images/%08d.png" % r)) for r in views}
    t3 = time.perf_counter()
    xyz = np.concatenate([views[r][0] for r in views], 0)
    rgb = np.concatenate([imgs[r].reshape(-1, 3)[:len(views[r][0])] for r in views], 0)
    data_io.write_ply(ply, xyz, rgb)
    t4 = time.perf_counter()
    return dict(load=spent["load"] + (t3 - t2), device=(t1 - t0) - spent["load"], write=t4 - t3), xyz


def route_b(folder, ply, th, method):
    t0 = time.perf_counter()
    scene = data_io.load_scene(folder, folder)
    t1 = time.perf_counter()
    sc = fusion.SceneFusion(method, th, device="cuda:0")
    for i, vid in enumerate(scene["view_ids"]):
        sc.add_view(vid, scene["depths"][i], scene["confs"][i], scene["cams"][i], scene["imgs"][i])
    sc.set_pairs(scene["pairs"])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out = sc.fuse(want=("records",))                                               # ends with the records on the host
    t3 = time.perf_counter()
    data_io.write_ply_records(ply, out["records"], out["n_points"])
    t4 = time.perf_counter()
    return dict(load=t1 - t0, upload=t2 - t1, device=t3 - t2, write=t4 - t3), out


def summarize(runs):
    keys = runs[0].keys()
    return {k: dict(median=statistics.median(r[k] for r in runs), min=min(r[k] for r in runs), max=max(r[k] for r in runs),
                    all=[r[k] for r in runs]) for k in keys}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=1152)
    ap.add_argument("--width", type=int, default=1536)
    ap.add_argument("--n_src", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--method", default="pcd", choices=["pcd", "dypcd"])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scan_fusion_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan.py measures the MI355X path: no GPU, no number")
    th = [0.5, 0.5, 0.5, 0.5]
    tmp = tempfile.mkdtemp(prefix="bench_scan_")
    try:
        t0 = time.perf_counter()
        write_scan(tmp, a.views, a.height, a.width, a.n_src)
        print("scan written in %.1f s" % (time.perf_counter() - t0), flush=True)
        ply_a, ply_b = os.path.join(tmp, "a.ply"), os.path.join(tmp, "b.ply")
        runs_a, runs_b = [], []
        for rep in range(a.repeats + 1):                                           # pass 0 warms every shape and the page cache: not kept
            sa, xyz_a = route_a(tmp, ply_a, th, a.method)
            sb, out_b = route_b(tmp, ply_b, th, a.method)
            print("pass %d  A %s  B %s" % (rep, json.dumps(sa), json.dumps(sb)), flush=True)
            if rep:
                runs_a.append(sa)
                runs_b.append(sb)
        xyz_b, _ = data_io.read_ply(ply_b)
        same = bool(np.array_equal(xyz_a.view(np.uint32), xyz_b.view(np.uint32)))
        A, B = summarize(runs_a), summarize(runs_b)
        res = dict(tool="tools/bench_scan.py", device=torch.cuda.get_device_name(0),
                   scene=dict(views=a.views, height=a.height, width=a.width, n_src_views=a.n_src, method=a.method, points=out_b["n_points"],
                              images="PNG", confidence_channels=4),
                   repeats=a.repeats, unit="seconds",
                   A_filter_scan_numpy_ply=A, B_fuse_scan=B,
                   device_part=dict(A=A["device"]["median"], B=B["device"]["median"], B_with_upload=B["device"]["median"] + B["upload"]["median"],
                                    note="A.device contains filter_scan's uploads; compare it with B_with_upload"),
                   total=dict(A=sum(v["median"] for v in A.values()), B=sum(v["median"] for v in B.values())),
                   xyz_identical=same)
        print(json.dumps(res))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        if not same:
            raise SystemExit("the two routes disagree on the cloud")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
