#!/usr/bin/env python
"""Time the gipuma-style sequential fusion (``mvs_gipuma_fuse_scene``) on a DTU-sized synthetic scan: 49 views at 1152x864, every view
against all others, default thresholds.

    python tools/bench_gipuma_fuse.py [--views 49] [--iters 5] [--host] [--out profiles/gipuma_fuse_bench.json]

Records total and per-launch device time (one launch per reference view; launch k cannot be replayed without the ``used`` history of
the launches before it, so its time is the difference of two prefix runs, jobs 0..k and 0..k-1, for a few k), the points kept,
(pixel, source) gathers per second beside the measured gather ceiling of profiles/gather_bound.json, the same scan through
``SceneFusion("pcd")`` with 10 sources for scale, and with ``--host`` the numpy restatement's time on a quarter-size scan.
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from mvsformer_amd import fusion, ops  # noqa: E402
from oracle import ref_fusion  # noqa: E402  (input generator only)


def scene(nv, h, w, seed=0):
    case = ref_fusion.make_fusion_case(n=1, v=nv - 1, h=h, w=w, seed=seed, noise=0.0005, outlier_frac=0.02)
    depths = torch.cat([case["ref_depth"], case["src_depths"][:, :, 0]], 1)[0].contiguous()
    cams = torch.cat([case["ref_cam"][:, None], case["src_cams"]], 1)[0].contiguous()
    return depths, cams


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--height", type=int, default=864)
    ap.add_argument("--width", type=int, default=1152)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gipuma_fuse_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    nv, h, w = a.views, a.height, a.width
    depths, cams = scene(nv, h, w)
    tables = tuple(torch.from_numpy(t).to(dev) for t in fusion.gipuma_tables(cams))
    d = depths.to(dev)
    jobs = [(r, [s for s in range(nv) if s != r]) for r in range(nv)]
    out = ops.gipuma_fuse_scene(d, tables, want_count=True)
    torch.cuda.synchronize()
    keep = out["keep"]
    kept_per_view = keep.view(nv, -1).sum(1).cpu().tolist()
    eligible = ((d > 0.001) & (d < 100000.0)).view(nv, -1).sum(1).cpu().tolist()
    total_ms = timed(lambda: ops.gipuma_fuse_scene(d, tables), a.iters)
    # launch k alone cannot be replayed without the history of `used`: time the prefixes 0..k and take differences (a few of them)
    probe = sorted({0, 1, 2, nv // 2, nv - 1})
    prefix = {}
    for k in sorted({p for q in probe for p in (q, q + 1) if p > 0}):
        table = ops.JobTable(jobs[:k], nv, dev)
        prefix[k] = timed(lambda: ops.gipuma_fuse_scene(d, tables, table), a.iters)
    prefix[0] = 0.0
    per_launch = {str(k): prefix[k + 1] - prefix[k] for k in probe}
    pairs_all = float(nv) * (nv - 1) * h * w
    # pairs that are really gathered: eligible, unused pixels x sources; from the count of pixels that entered the loop
    entered = [int(((out["count"][k] > 0) | keep[k]).sum()) for k in range(nv)]
    line = dict(metric="gipuma_fuse_scan_ms", value=total_ms, unit="ms per scan",
                config=dict(workload="%d views %dx%d, all-others sources, disp 0.2, 3 consistent" % (nv, w, h)),
                total_ms=total_ms, per_launch_ms=per_launch, mean_launch_ms=total_ms / nv,
                points_kept=int(sum(kept_per_view)), kept_per_view=kept_per_view[:4] + ["..."] + kept_per_view[-2:],
                kept_fraction_view0=kept_per_view[0] / float(h * w), pixels_valid_per_view=eligible[:2],
                pixels_with_a_consistent_source_or_kept=entered[:4], dtype="f32")
    gb = os.path.join(REPO, "profiles", "gather_bound.json")
    first_ms = per_launch["0"]
    pairs_first = float(eligible[0]) * (nv - 1)                 # launch 0: nothing is used yet, every valid pixel walks every source
    line["gathers"] = dict(pairs_nominal=pairs_all, nominal_pairs_per_s=pairs_all / total_ms * 1e3,
                           launch0_pairs=pairs_first, launch0_pairs_per_s=pairs_first / first_ms * 1e3,
                           launch0_gathered_TBps=pairs_first * 4.0 / first_ms * 1e3 / 1e12)
    if os.path.exists(gb):
        rows = json.load(open(gb))["rows"]
        tb = [r["gather_regs_TBps"] for r in rows if "gather_regs_TBps" in r]
        line["gathers"]["gather_ceiling_TBps"] = dict(min=min(tb), max=max(tb), source="profiles/gather_bound.json (gather_regs)")
        line["gathers"]["launch0_frac_of_ceiling"] = line["gathers"]["launch0_gathered_TBps"] / min(tb)
    # the same scan through the pcd filter with 10 sources
    confs = torch.ones(nv, 1, h, w)
    sc = fusion.SceneFusion("pcd", [0.5], thres_view=2, device=dev)
    for i in range(nv):
        sc.add_view(i, d[i], confs[i].to(dev), cams[i].to(dev))
    sc.set_pairs([(r, [(r + j) % nv for j in range(1, 11)]) for r in range(nv)])
    table = ops.JobTable([(r, [(r + j) % nv for j in range(1, 11)]) for r in range(nv)], nv, dev)
    cams_d = cams.to(dev)
    pcd_ms = timed(lambda: ops.geo_filter_scene(table, d, d, cams_d, 1.0, 0.01, 2.0, want=("mask", "points")), a.iters)
    pcd_points = sc.fuse(want=("xyz",))["n_points"]
    line["pcd_10_sources"] = dict(filter_ms=pcd_ms, points=pcd_points, pairs_per_s=float(nv) * 10 * h * w / pcd_ms * 1e3,
                                  taps_per_pair=4, gathered_TBps=float(nv) * 10 * h * w * 16.0 / pcd_ms * 1e3 / 1e12)
    g = fusion.GipumaFusion([0.5], device=dev)
    for i in range(nv):
        g.add_view(i, d[i], confs[i].to(dev), cams_d[i])
    t0 = time.perf_counter()
    res = g.fuse(want=("records",), on_device=True)
    torch.cuda.synchronize()
    line["fuse_end_to_end_ms"] = (time.perf_counter() - t0) * 1e3
    assert res["n_points"] == line["points_kept"], (res["n_points"], line["points_kept"])
    if a.host:
        import gipuma_fuse_util as gu
        hd, hc = scene(nv, h // 2, w // 2)
        t0 = time.time()
        gu.gipuma_rule(hd.numpy(), fusion.gipuma_tables(hc))
        dt = time.time() - t0
        line["host_numpy"] = dict(seconds=dt, sample="%d views at %dx%d (a quarter of the pixels)" % (nv, w // 2, h // 2),
                                  scaled_to_full_s=dt * 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
