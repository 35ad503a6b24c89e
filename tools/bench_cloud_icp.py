#!/usr/bin/env python
"""One iteration of scaled point-to-point ICP phase by phase (needs the GPU):

    python tools/bench_cloud_icp.py [--sizes 4000000,20000000] [--repeats 3] [--threshold 1.0] [--host-max 8000000] \\
        [--out profiles/cloud_icp_bench.json]

Two synthetic surface clouds per size (tools/bench_cloud_eval.py's three noisy patches, two different samplings), the source moved off by a
small similarity.  Timed separately, host clock with a synchronisation on both sides, every repeat kept: the target's index (built once per
registration), then per iteration the transform of the source, the nearest-neighbour query, the pair sums with their one record read, and the
host solve (``cloud_eval.umeyama``); then ``cloud_eval.icp`` as a whole (``--iters`` iterations, tolerances 0).  Beside them, where
``scipy`` imports, the host route on the same clouds (sizes up to ``--host-max``): ``cKDTree`` build, one capped query with 16 workers,
and the sums in numpy.
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
from bench_cloud_eval import surface, timed  # noqa: E402


def host_iteration(src, dst, threshold):
    """-> ms of ``(tree build, capped query, sums + solve)`` on the host."""
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(dst)
    t1 = time.perf_counter()
    dist, idx = tree.query(src, k=1, distance_upper_bound=threshold, workers=16)
    t2 = time.perf_counter()
    ok = idx < len(dst)
    o = 0.5 * (dst.min(0) + dst.max(0)).astype(np.float64)
    p, q = src[ok].astype(np.float64) - o, dst[idx[ok]].astype(np.float64) - o
    cloud_eval.umeyama(cloud_eval.PairSums(int(ok.sum()), len(src), p.sum(0), q.sum(0), q.T @ p, (p * p).sum(), (q * q).sum(), (dist[ok] ** 2).sum(), o))
    t3 = time.perf_counter()
    return 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000000,20000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=8000000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cloud_icp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_icp.py runs the MI355X path: no GPU")
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    res = dict(device=torch.cuda.get_device_name(0), threshold=a.threshold, scipy=have_scipy, cases=[])
    off = np.eye(4)
    off[:3, :3] *= 1.0005
    off[:3, 3] = [0.2, -0.1, 0.15]
    for n in [int(s) for s in a.sizes.split(",")]:
        dst, src = surface(n, 2, 0.05), cloud_eval.transform(surface(n, 3, 0.05), off)
        case = dict(n=n, ms={})
        index, case["ms"]["index_build_once"] = timed(lambda: cloud_eval._Index(dst, None, a.threshold), a.repeats)
        origin = [0.5 * (index.bounds[k] + index.bounds[3 + k]) for k in range(3)]
        srt = list(np.eye(3).reshape(-1)) + [0.0, 0.0, 0.0]
        moved, case["ms"]["transform"] = timed(lambda: ops.align_transform(src, srt), a.repeats)
        (dist, idx), case["ms"]["query"] = timed(lambda: index.query(moved, a.threshold), a.repeats)
        sums, case["ms"]["pair_sums_and_read"] = timed(lambda: cloud_eval.PairSums.from_record(ops.align_pair_sums(moved, dst, idx, dist, origin), origin), a.repeats)
        _, case["ms"]["host_solve"] = timed(lambda: cloud_eval.umeyama(sums, True), a.repeats)
        case["pairs"], case["cell"] = sums.n, index.cell
        whole, case["ms"]["icp_%d_iterations" % a.iters] = timed(
            lambda: cloud_eval.icp(src, dst, a.threshold, max_iter=a.iters, fitness_tol=0.0, rmse_tol=0.0), a.repeats)
        case["fitness"], case["inlier_rmse"] = whole.fitness, whole.inlier_rmse
        print(json.dumps(case), flush=True)
        if have_scipy and n <= a.host_max:
            build, query, solve = host_iteration(moved.cpu().numpy(), dst.cpu().numpy(), a.threshold)
            case["ms_host_scipy_ckdtree_workers16"] = dict(tree_build_once=build, query=query, sums_and_solve=solve)
            print(json.dumps(case["ms_host_scipy_ckdtree_workers16"]), flush=True)
        res["cases"].append(case)
        del dst, src, moved, dist, idx, index
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
