#!/usr/bin/env python
"""Time depth inference over a whole scan two ways on the same synthetic scan (49 views, 5 per sample, random-weight ``DINOMVSNet`` with
``randomize_bn_``):

  (A) the per-sample route: ``DINOMVSNet.forward`` once per reference view - the 2-D networks see N*V images;
  (B) the scene route: ``scene.SceneInference`` - every image through the FPN and the ViT once into a feature bank, the cascade over the bank.

    python tools/bench_scan_infer.py [--views 49] [--num_views 5] [--sizes 1152x1536,512x640] [--repeats 3] [--out profiles/scan_inference_bench.json]

Each route is split into extract (2-D networks; for (B) including the copy into the bank) / cascade / total: extract and cascade are HIP-event
brackets on the one stream both routes use, total is a host clock around the whole scan ending in a device synchronise (it contains the launch
gaps the brackets do not).  The routes alternate, ``--repeats`` times after one untimed pass of each, and every repeat is kept (median and
min..max are reported).  Also reported: the bank's bytes, how many images each route extracted, and the largest depth difference between the
routes.  Needs the GPU; prints and writes one JSON object.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mvsformer_amd as m  # noqa: E402
from mvsformer_amd import synth  # noqa: E402

TMP = [5.0, 5.0, 5.0, 1.0]
ARGS = dict(fix=True, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
            depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
            vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                          att_fusion=True, nhead=6))


def make_scan(views, num_views, h, w, dev):
    sc = synth.make_scene(views, h, w, seed=4)
    imgs = torch.cat([synth.render_features(synth.make_scene(1, h, w, seed=10 + i), 1, 3, noise=0.02, device=dev, dtype=torch.float32)[0]
                      for i in range(views)])                                        # [views,3,h,w], one texture per view
    cams = torch.zeros(views, 2, 4, 4, dtype=torch.float64)
    cams[:, 0] = sc.E
    cams[:, 1, :3, :3] = sc.K
    cams[:, 1, 3, 3] = 1.0
    pairs = [(i, [(i + d) % views for d in (1, views - 1, 2, views - 2, 3, views - 3, 4, views - 4, 5, views - 5)]) for i in range(views)]
    return imgs, cams.to(device=dev, dtype=torch.float32), synth.depth_range(1, device=dev)[0].contiguous(), pairs


def route_a(net, imgs, cams, dr, pairs, num_views):
    """DINOMVSNet.forward per reference view, as the code stood before the scene route: extract_features + the cascade, bracketed apart."""
    from mvsformer_amd import scene
    from mvsformer_amd.cascade import CascadeMVS
    per_view = [scene.stage_cams(c) for c in cams]
    ev = {"extract": [], "cascade": []}
    depths = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for r, srcs in pairs:
            views = [r] + srcs[:num_views - 1]
            proj = {"stage%d" % (k + 1): torch.stack([per_view[v][k] for v in views])[None] for k in range(4)}
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            feats = net.extract_features(imgs[views][None])
            e[1].record()
            out = CascadeMVS.forward(net, feats, proj, dr[None], tmp=TMP)
            e[2].record()
            ev["extract"].append((e[0], e[1]))
            ev["cascade"].append((e[1], e[2]))
            depths[r] = out["refined_depth"][0]
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    return dict(extract=sum(a.elapsed_time(b) for a, b in ev["extract"]), cascade=sum(a.elapsed_time(b) for a, b in ev["cascade"]), total=total), depths


def route_b(net, imgs, cams, dr, pairs, num_views, extract_batch, capacity):
    si = m.SceneInference(net, capacity_views=capacity, max_bank_mb=65536, extract_batch=extract_batch)
    for v in range(imgs.shape[0]):
        si.add_image(v, imgs[v], cams[v], dr)
    si.set_pairs(pairs, num_views=num_views)
    si.timing = True
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = si.run(tmp=TMP)
    torch.cuda.synchronize()
    total = (time.perf_counter() - t0) * 1e3
    return dict(si.timings(), total=total), {r: o["depth"] for r, o in out.items()}, dict(si.stats)


def summarize(runs):
    return {k: dict(median=statistics.median(r[k] for r in runs), min=min(r[k] for r in runs), max=max(r[k] for r in runs), all=[r[k] for r in runs])
            for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--num_views", type=int, default=5)
    ap.add_argument("--sizes", default="1152x1536,512x640")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--extract_batch", type=int, default=4)
    ap.add_argument("--capacity_views", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scan_inference_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scan_infer.py measures the MI355X path: no GPU, no number")
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    net = m.DINOMVSNet(ARGS).eval()
    m.cascade.randomize_bn_(net, seed=2)
    net = net.to(dev)
    res = dict(tool="tools/bench_scan_infer.py", device=torch.cuda.get_device_name(0), repeats=a.repeats, unit="milliseconds per scan",
               scan=dict(views=a.views, views_per_sample=a.num_views, extract_batch=a.extract_batch, capacity_views=a.capacity_views), sizes={})
    for size in a.sizes.split(","):
        h, w = (int(x) for x in size.split("x"))
        imgs, cams, dr, pairs = make_scan(a.views, a.num_views, h, w, dev)
        runs_a, runs_b = [], []
        for rep in range(a.repeats + 1):                                            # pass 0 warms every shape and the weight caches: not kept
            ta, da = route_a(net, imgs, cams, dr, pairs, a.num_views)
            tb, db, stats = route_b(net, imgs, cams, dr, pairs, a.num_views, a.extract_batch, a.capacity_views)
            print("%s pass %d  A %s  B %s" % (size, rep, json.dumps(ta), json.dumps(tb)), flush=True)
            if rep:
                runs_a.append(ta)
                runs_b.append(tb)
        worst = max(((db[r] - da[r]).abs() / da[r].abs()).max().item() for r in da)
        bitwise = all(torch.equal(db[r], da[r]) for r in da)
        A, B = summarize(runs_a), summarize(runs_b)
        n = len(pairs)
        res["sizes"][size] = dict(
            A_per_sample=A, B_scene=B,
            per_depth_map_ms=dict(A=A["total"]["median"] / n, B=B["total"]["median"] / n),
            images_extracted=dict(A=n * a.num_views, B=stats["extracted"], B_passes=stats["extract_passes"]),
            extract_ratio_A_over_B=A["extract"]["median"] / B["extract"]["median"],
            cascade_ratio_B_over_A=B["cascade"]["median"] / A["cascade"]["median"],
            B_extract_share_of_device_time=B["extract"]["median"] / (B["extract"]["median"] + B["cascade"]["median"]),
            speedup_total=A["total"]["median"] / B["total"]["median"],
            bank_bytes=stats["bank_bytes"], view_bytes=stats["view_bytes"], capacity_views=stats["capacity_views"],
            max_rel_depth_diff=worst, depth_bitwise_equal=bitwise)
        del imgs
        torch.cuda.empty_cache()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
