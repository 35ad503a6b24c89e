#!/usr/bin/env python
"""Point-cloud evaluation phase by phase (needs the GPU):

    python tools/bench_cloud_eval.py [--sizes 2000000,20000000] [--repeats 3] [--out profiles/cloud_eval_bench.json]

Two synthetic surface clouds per size - a "ground truth" of three large noisy patches and a "reconstruction" of the same surface with more
noise, 2 % far outliers and a missing strip - the larger size of the order of a fused DTU scan.  Timed separately, host clock with a
synchronisation on both sides, every repeat kept: the index build of each cloud (bounds, keys, ``torch.sort``, table), both queries
(query keys, sort, walk), the thinning of the reconstruction, the score reduction, and ``evaluate`` as a whole.  Beside them, where
``scipy`` imports, the same distances from ``scipy.spatial.cKDTree(...).query(..., distance_upper_bound=max_dist, workers=16)`` (build
and query; one repeat at the larger size) and the largest difference between the two routes' distances.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvsformer_amd import cloud_eval, ops  # noqa: E402


def surface(n, seed, noise, outliers=0.0, gap=False, dev="cuda:0"):
    """Three 400 x 400 patches (a floor and two tilted walls), ``noise`` mm of Gaussian noise, a share of uniform outliers."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand(n, 2, device=dev, generator=g) * 400.0 - 200.0
    which = torch.randint(0, 3, (n,), device=dev, generator=g)
    z = torch.where(which == 0, 0.2 * u[:, 0], torch.where(which == 1, 150.0 + 0.5 * u[:, 1], -100.0 - 0.3 * u[:, 0] + 0.1 * u[:, 1]))
    p = torch.stack([u[:, 0], u[:, 1], z], 1) + noise * torch.randn(n, 3, device=dev, generator=g)
    if gap:
        p = p[(u[:, 0] < 40.0) | (u[:, 0] > 70.0)]
    k = int(outliers * p.shape[0])
    if k:
        p[:k] = torch.rand(k, 3, device=dev, generator=g) * 800.0 - 400.0
    return p.contiguous()


def timed(fn, repeats):
    out, ms = None, []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000000,20000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max_dist", type=float, default=20.0)
    ap.add_argument("--voxel", type=float, default=0.2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cloud_eval_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_eval.py runs the MI355X path: no GPU")
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        cKDTree = None
    md, taus = a.max_dist, (1.0, 2.0)
    res = dict(device=torch.cuda.get_device_name(0), max_dist=md, taus=list(taus), voxel=a.voxel, scipy=cKDTree is not None, cases=[])
    for n in [int(s) for s in a.sizes.split(",")]:
        gt, pred = surface(n, 1, 0.05), surface(n, 2, 0.4, outliers=0.02, gap=True)
        case = dict(n_gt=int(gt.shape[0]), n_pred=int(pred.shape[0]), ms={})
        index_gt, case["ms"]["index_gt"] = timed(lambda: cloud_eval._Index(gt, None, md), a.repeats)
        index_pred, case["ms"]["index_pred"] = timed(lambda: cloud_eval._Index(pred, None, md), a.repeats)
        case["cell"] = dict(gt=index_gt.cell, pred=index_pred.cell)
        (d_pg, _), case["ms"]["query_pred_to_gt"] = timed(lambda: index_gt.query(pred, md), a.repeats)
        (d_gp, _), case["ms"]["query_gt_to_pred"] = timed(lambda: index_pred.query(gt, md), a.repeats)
        thin, case["ms"]["voxel_downsample_pred"] = timed(lambda: cloud_eval.voxel_downsample(pred, a.voxel), a.repeats)
        case["n_pred_thinned"] = int(thin.shape[0])
        rec, case["ms"]["score_both"] = timed(lambda: (ops.cloud_score(d_pg, md, taus), ops.cloud_score(d_gp, md, taus)), a.repeats)
        scores, case["ms"]["evaluate"] = timed(lambda: cloud_eval.evaluate(pred, gt, md, taus), a.repeats)
        case["scores"] = {k: scores[k] for k in ("accuracy", "completeness", "overall", "precision", "recall", "fscore")}
        if cKDTree is not None:
            reps = a.repeats if n <= 4000000 else 1
            hp, hg = pred.cpu().numpy().astype(np.float64), gt.cpu().numpy().astype(np.float64)
            kd = {"build_gt": [], "build_pred": [], "query_pred_to_gt": [], "query_gt_to_pred": []}
            for _ in range(reps):
                t0 = time.perf_counter(); tg = cKDTree(hg); t1 = time.perf_counter(); tp = cKDTree(hp); t2 = time.perf_counter()      # noqa: E702
                kpg = tg.query(hp, distance_upper_bound=md, workers=16)[0]; t3 = time.perf_counter()                                    # noqa: E702
                kgp = tp.query(hg, distance_upper_bound=md, workers=16)[0]; t4 = time.perf_counter()                                    # noqa: E702
                for k, v in zip(kd, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                    kd[k].append(1e3 * v)
            case["ms_scipy_ckdtree_workers16"] = kd
            worst = 0.0
            for mine, theirs in ((d_pg, kpg), (d_gp, kgp)):
                theirs = np.where(np.isfinite(theirs), theirs, md)
                worst = max(worst, float(np.abs(mine.cpu().numpy().astype(np.float64) - theirs).max()))
            case["largest_distance_difference"] = worst
            del hp, hg, tg, tp
        res["cases"].append(case)
        print(json.dumps(case))
        del gt, pred, index_gt, index_pred, d_pg, d_gp, thin
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
