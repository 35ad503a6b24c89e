"""Scene preparation on the device: from a sparse reconstruction to ``pair.txt`` and a depth range per camera - the step BEFORE
``tools/infer_scan.py``.  The reference asks its users for it ("you should build a new pair.txt with 20 views as MVSNet") and leaves it
to MVSNet's ``colmap2mvsnet.py``, a Python double loop over view pairs and their common points.

The rule is RESTATED from memory of the published MVSNet script (its source is not part of the reference): every constant is an
argument, and parity with the original script is UNVERIFIED.  ``include/mvs_scene_prep.h`` ("Scene preparation") spells it out:

* two views score the sum, over the points both observe, of ``exp(-(theta - theta0)^2 / (2 sigma^2))`` with ``theta`` the angle in
  degrees between the rays from the point to the two camera centres and ``sigma = sigma1`` for ``theta <= theta0``, else ``sigma2``
  (the script: ``theta0 = 5, sigma1 = 1, sigma2 = 10``);
* a view's sources are the other views by descending score, equal scores in ascending index (a stable descending sort);
* a view's depth range is ``(sorted_z[int(n * lo)], sorted_z[int(n * hi)])`` over the camera-space depths ``z`` of the points it
  observes (the script: ``lo = 0.01, hi = 0.99``).

Inputs everywhere: ``xyz [N,3]`` fp32, one observation per track element ``(obs_point [M] int64, obs_view [M] int32)``, ``R [V,3,3]``
and ``t [V,3]`` fp32, world to camera.  numpy arrays and CPU tensors are uploaded; everything is computed by ``libmvs_hip.so``.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib, ops

__all__ = ["visibility", "pair_scores", "rank_sources", "depth_ranges", "prepare_scene", "write_scan"]


def _dev(a, dtype) -> torch.Tensor:
    """numpy array / CPU tensor / device tensor -> a contiguous tensor of ``dtype`` on the current device (values must survive the cast)."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=torch.device("cuda", torch.cuda.current_device()), dtype=dtype).contiguous()


def _scene(xyz, R, t):
    return _dev(xyz, torch.float32), _dev(R, torch.float32), _dev(t, torch.float32)


def visibility(xyz, obs_point, obs_view, num_views: int):
    """-> ``(bits [V, ceil(N/64)] int64 (the uint64 words), count [V] int32, number of non-finite points)``.  Bit ``p % 64`` of word
    ``p // 64`` of row ``v`` is set when view ``v`` observes point ``p``; duplicates collapse; a point with a non-finite coordinate is
    set in no row.  An observation that names a point or view out of range raises (checked on the device).  One host synchronisation."""
    bits, count, info = ops.scene_visibility(_dev(obs_point, torch.int64), _dev(obs_view, torch.int32), _dev(xyz, torch.float32), num_views)
    return bits, count, int(info[1].item())


def pair_scores(bits, xyz, R, t, theta0: float = 5.0, sigma1: float = 1.0, sigma2: float = 10.0) -> torch.Tensor:
    """-> ``S [V,V]`` fp64, symmetric with a zero diagonal; the same bits on every run."""
    return ops.scene_pair_scores(bits, *_scene(xyz, R, t), theta0=theta0, sigma1=sigma1, sigma2=sigma2)


def rank_sources(S, k: int):
    """-> ``(src [V,k] int32, score [V,k] fp64)``: descending score, ties to the lower view index; ``-1`` / ``0`` past ``V - 1`` sources."""
    return ops.scene_rank_sources(_dev(S, torch.float64), k)


def depth_ranges(bits, count, xyz, R, t, lo: float = 0.01, hi: float = 0.99, capacity=None):
    """-> ``(range [V,2] fp32, n [V] int32)``; a view that observes nothing gets ``(0, 0)`` and ``n = 0``."""
    return ops.scene_depth_ranges(bits, count, *_scene(xyz, R, t), lo=lo, hi=hi, capacity=capacity)


def write_scan(out_dir, result, R, t, K, num_depth: int = 192) -> None:
    """``out_dir/pair.txt`` and ``out_dir/cams/%08d_cam.txt`` (through ``data_io.write_pair_file`` / ``write_cam``) from what
    ``prepare_scene`` returned; the last row of a camera file is ``depth_min depth_interval num_depth depth_max``, MVSNet's layout."""
    import os
    from . import data_io
    os.makedirs(os.path.join(out_dir, "cams"), exist_ok=True)
    data_io.write_pair_file(os.path.join(out_dir, "pair.txt"), result["pairs"], result["scores"])
    for v in range(len(R)):
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0, :3, :3], cam[0, :3, 3], cam[0, 3, 3] = np.asarray(R[v]), np.asarray(t[v]), 1.0
        cam[1, :3, :3] = np.asarray(K[v])
        cam[1, 3] = result["depth_min"][v], result["depth_interval"][v], num_depth, result["depth_max"][v]
        data_io.write_cam(os.path.join(out_dir, "cams", "%08d_cam.txt" % v), cam)


def prepare_scene(xyz, obs_point, obs_view, R, t, num_views: int = 20, num_depth: int = 192, interval_scale: float = 1.0,
                  theta0: float = 5.0, sigma1: float = 1.0, sigma2: float = 10.0, lo: float = 0.01, hi: float = 0.99,
                  keep_zero: bool = False) -> Dict[str, object]:
    """The whole step -> ``{"pairs", "scores", "depth_min", "depth_interval", "depth_max", "n_points", "n_nonfinite"}``.

    ``pairs``: ``[(view, [source, ...])]`` in ``data_io.read_pair_file``'s form, at most ``num_views`` sources per view, best first;
    ``scores``: the matching list of score lists.  A source with score 0 shares no point with the view and is left out (``keep_zero=True``
    lists it): OUR choice - the script lists the top ``num_views`` whatever they score; a view left without sources keeps its (empty)
    entry here and is dropped by ``read_pair_file``, as the reference's reader does.
    ``depth_min``, ``depth_max`` float32 ``[V]``: the two order statistics; ``depth_interval = (depth_max - depth_min) / (num_depth - 1)
    / interval_scale`` in float64 - the PLAIN form (the script, as recalled, goes through an inverse-depth pixel step when no
    ``max_d`` is given; that branch is not restated).  ``n_points`` int ``[V]``: points behind each range (0: the range is (0, 0)).

    Four entry points enqueued back to back on the current stream and ONE device-to-host copy at the end; nothing waits in between.
    An observation that names a point or a view out of range raises after that copy (it was counted on the device, never written)."""
    xyz, R, t = _scene(xyz, R, t)
    obs_point, obs_view = _dev(obs_point, torch.int64), _dev(obs_view, torch.int32)
    V, k = R.shape[0], max(1, int(num_views))
    if int(num_depth) < 2 or not float(interval_scale) > 0.0:
        raise ValueError("prepare_scene: num_depth >= 2 and interval_scale > 0, got %r and %r" % (num_depth, interval_scale))
    bits, count, info = ops.scene_visibility(obs_point, obs_view, xyz, V, wait=False)
    S = ops.scene_pair_scores(bits, xyz, R, t, theta0=theta0, sigma1=sigma1, sigma2=sigma2)
    src, score = ops.scene_rank_sources(S, k)
    rng, n = ops.scene_depth_ranges(bits, count, xyz, R, t, lo=lo, hi=hi, capacity=obs_point.shape[0])
    f64 = torch.float64                                          # int32, float32 and the two counters (< 2^53) are exact in float64
    host = torch.cat([src.to(f64).reshape(-1), score.reshape(-1), rng.to(f64).reshape(-1), n.to(f64), info.to(f64)]).cpu().numpy()
    src_h, score_h = host[:V * k].reshape(V, k).astype(np.int64), host[V * k:2 * V * k].reshape(V, k)
    rng_h = host[2 * V * k:2 * V * k + 2 * V].reshape(V, 2).astype(np.float32)
    n_h = host[2 * V * k + 2 * V:2 * V * k + 3 * V].astype(np.int64)
    bad, nonfinite = int(host[-2]), int(host[-1])
    if bad:
        raise _lib.MvsHipError("prepare_scene: %d observations name a point outside [0, %d) or a view outside [0, %d)" % (bad, xyz.shape[0], V))
    if (n_h < 0).any():
        raise _lib.MvsHipError("prepare_scene: the depth workspace did not hold view(s) %s" % np.nonzero(n_h < 0)[0].tolist()[:8])
    pairs: List[Tuple[int, List[int]]] = []
    scores: List[List[float]] = []
    for v in range(V):
        keep = [c for c in range(k) if src_h[v, c] >= 0 and (keep_zero or score_h[v, c] > 0.0)]
        pairs.append((v, [int(src_h[v, c]) for c in keep]))
        scores.append([float(score_h[v, c]) for c in keep])
    dmin, dmax = rng_h[:, 0].copy(), rng_h[:, 1].copy()
    interval = (dmax.astype(np.float64) - dmin.astype(np.float64)) / (int(num_depth) - 1) / float(interval_scale)
    return {"pairs": pairs, "scores": scores, "depth_min": dmin, "depth_interval": interval, "depth_max": dmax, "n_points": n_h,
            "n_nonfinite": nonfinite}
