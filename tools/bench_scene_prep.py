#!/usr/bin/env python
"""Time scene preparation (``mvsformer_amd.scene_prep``) on a synthetic scene of Tanks-and-Temples size: 300 views on a ring, 10^6
points, track lengths drawn around 6.

    python tools/bench_scene_prep.py [--views 300] [--points 1000000] [--iters 5] [--host_pairs 60] [--out profiles/scene_prep_bench.json]

Records the device time of each phase (visibility bitset, pair scores, ranking, depth ranges), ``prepare_scene`` end to end from device
arrays (wall clock, its one device-to-host copy included), and the numpy restatement of the pair loop (tests/scene_prep_util.py's
arithmetic on the common points of a pair, found with ``np.intersect1d``) on ``--host_pairs`` random pairs, scaled to all V (V - 1) / 2;
the same pairs are compared with the device's scores.  No pass threshold: a new capability, the file records what was measured.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from mvsformer_amd import scene_prep  # noqa: E402
import scene_prep_util as U  # noqa: E402


def scene(V, N, seed=0, track=6.0):
    """Cameras on a ring looking at a blob; a point's track is a run of neighbouring views (every 1st, 2nd or 3rd) from a random start."""
    rng = np.random.default_rng(seed)
    ang = np.arange(V) * (2.0 * np.pi / V)
    R, t = np.zeros((V, 3, 3)), np.zeros((V, 3))
    for v in range(V):
        R[v], t[v] = U.look_at((4.0 * np.cos(ang[v]), 4.0 * np.sin(ang[v]), rng.uniform(-0.3, 0.3)))
    xyz = rng.normal(0.0, 0.6, (N, 3)).astype(np.float32)
    lengths = np.minimum(rng.poisson(track, N), V // 3)
    start, stride = rng.integers(0, V, N), rng.integers(1, 4, N)
    obs_point = np.repeat(np.arange(N, dtype=np.int64), lengths)
    within = np.arange(len(obs_point)) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    obs_view = ((start[obs_point] + within * stride[obs_point]) % V).astype(np.int32)
    order = rng.permutation(len(obs_point))
    return xyz, obs_point[order], obs_view[order], R.astype(np.float32), t.astype(np.float32)


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


def host_pair(points_of, C, P, i, j):
    common = np.intersect1d(points_of[i], points_of[j], assume_unique=True)
    if not len(common):
        return 0.0, 0
    p = P[common]
    a, b = C[i] - p, C[j] - p
    c = np.cross(a, b)
    theta = np.arctan2(np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]), (a * b).sum(1)) * U.DEG
    d, s = theta - U.THETA0, np.where(theta <= U.THETA0, U.SIGMA1, U.SIGMA2)
    return float(np.exp(-(d * d) / (2.0 * s * s)).sum()), len(common)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=300)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host_pairs", type=int, default=60)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scene_prep_bench.json"))
    a = ap.parse_args()
    V, N = a.views, a.points
    dev = torch.device("cuda:0")
    xyz, obs_point, obs_view, R, t = scene(V, N)
    M = len(obs_point)
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(xyz=xyz, obs_point=obs_point, obs_view=obs_view, R=R, t=t).items()}
    bits, count, nonfinite = scene_prep.visibility(d["xyz"], d["obs_point"], d["obs_view"], V)
    S = scene_prep.pair_scores(bits, d["xyz"], d["R"], d["t"])
    phases = {
        "visibility_ms": timed(lambda: scene_prep.ops.scene_visibility(d["obs_point"], d["obs_view"], d["xyz"], V, wait=False), a.iters),
        "pair_scores_ms": timed(lambda: scene_prep.pair_scores(bits, d["xyz"], d["R"], d["t"]), a.iters),
        "rank_sources_ms": timed(lambda: scene_prep.rank_sources(S, 20), a.iters),
        "depth_ranges_ms": timed(lambda: scene_prep.depth_ranges(bits, count, d["xyz"], d["R"], d["t"], capacity=M), a.iters),
    }
    wall = []
    for _ in range(a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = scene_prep.prepare_scene(d["xyz"], d["obs_point"], d["obs_view"], d["R"], d["t"], num_views=20)
        wall.append((time.perf_counter() - t0) * 1e3)
    Sh = S.cpu().numpy()
    track = np.bincount(obs_point, minlength=N)                 # distinct views per point: L (L - 1) / 2 terms each
    common_terms = float((track * (track - 1) // 2).sum())
    line = dict(metric="scene_prep_ms", value=sorted(wall)[len(wall) // 2], unit="ms per scene (prepare_scene from device arrays, wall clock)",
                config=dict(workload="%d views on a ring, %d points, %d observations (track lengths ~ Poisson(6)), num_views 20" % (V, N, M)),
                phases_device_ms=phases, phases_sum_ms=sum(phases.values()), prepare_scene_wall_ms=sorted(wall),
                pairs=V * (V - 1) // 2, pair_terms=common_terms, bitset_MB=bits.numel() * 8 / 1e6,
                pair_scores=dict(bitset_bytes_read_per_run=float(V) * (V - 1) / 2 * 2 * bits.shape[1] * 8,
                                 read_TBps=float(V) * (V - 1) / 2 * 2 * bits.shape[1] * 8 / phases["pair_scores_ms"] * 1e3 / 1e12,
                                 terms_per_s=common_terms / phases["pair_scores_ms"] * 1e3),
                sources_per_view=[len(s) for _, s in res["pairs"]][:4], depth_range_view0=[float(res["depth_min"][0]), float(res["depth_max"][0])],
                n_nonfinite=nonfinite, dtype="f64 scores, f32 depths")
    if a.host_pairs > 0:
        rng = np.random.default_rng(1)
        order = np.argsort(obs_view, kind="stable")
        bounds = np.searchsorted(obs_view[order], np.arange(V + 1))
        points_of = [np.unique(obs_point[order[bounds[v]:bounds[v + 1]]]) for v in range(V)]
        C, P = U.centers_ref(R, t), xyz.astype(np.float64)
        near = [(int(i), int((i + k) % V)) for i, k in zip(rng.integers(0, V, a.host_pairs // 2), rng.integers(1, 12, a.host_pairs // 2))]
        far = [tuple(int(x) for x in rng.choice(V, 2, replace=False)) for _ in range(a.host_pairs - len(near))]
        t0 = time.perf_counter()
        got = [host_pair(points_of, C, P, i, j) for i, j in near + far]
        dt = time.perf_counter() - t0
        err = max(abs(s - Sh[i, j]) / max(Sh[i].max(), 1e-300) for (s, _), (i, j) in zip(got, near + far))
        line["host_numpy"] = dict(pairs=len(got), seconds=dt, scaled_to_all_pairs_s=dt / len(got) * (V * (V - 1) / 2),
                                  sample="half of the pairs within 12 ring positions, half random; view index lists prepared beforehand",
                                  common_points_mean=float(np.mean([n for _, n in got])), max_rel_diff_to_device=err,
                                  speedup_of_pair_scores=dt / len(got) * (V * (V - 1) / 2) * 1e3 / phases["pair_scores_ms"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(line, f, indent=1)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
