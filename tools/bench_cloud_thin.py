#!/usr/bin/env python
"""DTU's greedy thinning phase by phase (needs the GPU):

    python tools/bench_cloud_thin.py [--sizes 4000000,20000000] [--repeats 3] [--dist D] [--seed 0] [--host-max 8000000] \\
        [--out profiles/cloud_thin_bench.json]

One synthetic surface cloud per size (tools/bench_cloud_eval.py's three noisy patches) and a radius at which a point has about two
neighbours, so that roughly half of the points survive (``--dist`` overrides it).  Timed separately, host clock with a synchronisation on
both sides, every repeat kept: the visiting order (``torch.randperm``), the index build (bounds, keys, ``torch.sort``, table), the rounds
(ranks, the rounds themselves with their counter reads, the keep mask; the number of rounds is reported) and the compaction
(``xyz[keep]``), then ``greedy_thin`` as a whole.  Beside them, where ``sklearn`` imports, the host pass on the same cloud and order:
``NearestNeighbors.radius_neighbors`` (kd-tree, 16 workers) and the sequential loop, and whether the two keep masks are equal (sizes up
to ``--host-max``; the larger size is of the order of a fused DTU scan).
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvsformer_amd import cloud_eval, ops  # noqa: E402
from bench_cloud_eval import surface, timed  # noqa: E402

AREA = 400.0 * 400.0 * (math.sqrt(1.04) + math.sqrt(1.25) + math.sqrt(1.10))   # the three patches of surface()


def host_pass(xyz, dist, order):
    """-> ``(keep, ms of the range search, ms of the loop)``: the rule on the host.  The kd-tree gives the candidates (fp64, radius widened
    by 1e-5); they are then held to the library's distance contract - ``(dx*dx + dy*dy) + dz*dz <= dist*dist`` in fp32 - so a pair at the
    radius to within rounding falls on the same side in both passes and the masks can be compared for equality."""
    from sklearn.neighbors import NearestNeighbors
    t0 = time.perf_counter()
    p = xyz.astype(np.float64)
    d32 = np.float32(dist)
    lists = NearestNeighbors(radius=float(d32) * (1.0 + 1e-5), algorithm="kd_tree", n_jobs=16).fit(p).radius_neighbors(p, return_distance=False)
    counts = np.fromiter((len(v) for v in lists), np.int64, len(lists))
    i, j = np.repeat(np.arange(len(p)), counts), np.concatenate(lists)
    d = xyz[i] - xyz[j]                                                      # float32 throughout
    near = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= d32 * d32
    i, j = i[near], j[near]                                                  # still grouped by i, i itself included
    start = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=len(p)))])
    t1 = time.perf_counter()
    state = np.zeros(len(p), np.int8)                                        # 0 unseen, 1 kept, -1 removed
    for k in order.tolist():
        if state[k] == 0:
            state[j[start[k]:start[k + 1]]] = -1
            state[k] = 1
    t2 = time.perf_counter()
    return state == 1, 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000000,20000000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dist", type=float, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--host-max", type=int, default=8000000)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cloud_thin_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cloud_thin.py runs the MI355X path: no GPU")
    try:
        import sklearn  # noqa: F401
        have_sklearn = True
    except ImportError:
        have_sklearn = False
    res = dict(device=torch.cuda.get_device_name(0), seed=a.seed, rounds_per_counter_read=ops.GREEDY_THIN_BATCH, sklearn=have_sklearn, cases=[])
    for n in [int(s) for s in a.sizes.split(",")]:
        xyz = surface(n, 2, 0.05)
        dist = a.dist if a.dist is not None else math.sqrt(2.0 * AREA / (math.pi * n))
        case = dict(n=n, dist=dist, ms={})
        order, case["ms"]["order_randperm"] = timed(lambda: cloud_eval._order(None, n, a.seed, xyz.device), a.repeats)

        def index():
            grid, bounds, n_bad = ops.cloud_bounds(xyz)
            cell = cloud_eval.thin_cell(bounds, dist)
            skeys, perm = torch.sort(ops.cloud_grid_keys(xyz, cell, grid, bounds, n_bad), stable=True)
            return (grid, cell, perm) + ops.cloud_grid_build(xyz, skeys, perm, grid, True)

        (grid, cell, perm, spts, cell_keys, cell_start), case["ms"]["index_build"] = timed(index, a.repeats)
        case["cell"], case["occupied_cells"] = cell, ops.cloud_voxel_count(grid)
        (keep, rounds), case["ms"]["rounds"] = timed(lambda: ops.greedy_thin(order, grid, dist, spts, perm, cell_keys, cell_start), a.repeats)
        case["rounds"] = rounds
        kept, case["ms"]["compaction"] = timed(lambda: xyz[keep], a.repeats)
        case["n_kept"], case["share_kept"] = int(kept.shape[0]), float(kept.shape[0]) / n
        whole, case["ms"]["greedy_thin"] = timed(lambda: cloud_eval.greedy_thin(xyz, dist, order=order), a.repeats)
        case["whole_equals_phases"] = bool(torch.equal(whole, kept))
        print(json.dumps(case), flush=True)
        if have_sklearn and n <= a.host_max:
            hk, ms_search, ms_loop = host_pass(xyz.cpu().numpy(), dist, order.cpu().numpy())
            case["ms_host_sklearn_kdtree_workers16"] = dict(radius_neighbors=ms_search, sequential_loop=ms_loop)
            mine = keep.cpu().numpy()
            case["host_n_kept"], case["masks_equal"], case["masks_differ_at"] = int(hk.sum()), bool(np.array_equal(hk, mine)), int((hk != mine).sum())
            print(json.dumps({k: case[k] for k in ("ms_host_sklearn_kdtree_workers16", "host_n_kept", "masks_equal", "masks_differ_at")}), flush=True)
        res["cases"].append(case)
        del xyz, order, grid, perm, spts, cell_keys, cell_start, keep, kept, whole
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
