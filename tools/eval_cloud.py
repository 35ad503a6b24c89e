#!/usr/bin/env python
"""Score a reconstructed point cloud against a ground-truth cloud on the MI355X (needs the GPU):

    python tools/eval_cloud.py --pred fused.ply --gt stl.ply --max_dist 20 --tau 1,2 [--voxel 0.2 | --thin-dist 0.2 [--thin-seed 0]] \\
        [--box x0,y0,z0,x1,y1,z1] [--plane a,b,c,d] --out scores.json
    python tools/eval_cloud.py --pred Barn_fused.ply --gt Barn.ply --align Barn_trans.txt --crop Barn.json --icp 0.01 --out scores.json

Both files are read with ``data_io.read_ply`` (the layout ``write_ply`` / ``fuse_scan`` write).  ``--box`` keeps the points of BOTH clouds
inside the box, ``--plane`` those with ``a x + b y + c z + d > 0`` (DTU's bounding box and table plane).  The scores are
``mvsformer_amd.cloud_eval.evaluate``'s: accuracy / completeness / overall (DTU: means of the distances below ``--max_dist``) and, per
``--tau``, precision / recall / F-score (Tanks and Temples).  ``--voxel`` thins both clouds to one centroid per voxel first (the Open3D /
Tanks-and-Temples rule).  ``--thin-dist`` thins the PREDICTION only by DTU's rule (``cloud_eval.greedy_thin``: a greedy pass over a shuffle
of the points; a kept point removes every other point within the distance), after the box and the plane; the shuffle is a device
permutation seeded with ``--thin-seed``, not MATLAB's, so the scores are those of DTU's protocol under another shuffle.

Tanks and Temples (the second form): ``--align`` is the 4 x 4 that brings the prediction into the ground truth's frame (``*_trans.txt``),
``--crop`` Open3D's ``SelectionPolygonVolume`` json, ``--icp DTAU`` refines the alignment by the protocol's three scaled ICP stages
(``cloud_eval.register_tt``; the stage parameters are recalled from the toolbox, not checked against it) and scores with
``cloud_eval.evaluate_tt``: both clouds thinned to voxels of ``DTAU / 2``, precision / recall / F-score at ``DTAU`` (or at ``--tau``),
``--max_dist`` capping the means as before.  ``--no-icp`` with ``--align`` / ``--crop`` only applies them and scores as the first form
does.  The output then also holds the final transform, the per-stage fitness and inlier rmse and the point counts after the crop.  Without
these four flags the output is what it was before they existed.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvsformer_amd import cloud_eval, data_io  # noqa: E402


def floats(text, n=None):
    v = [float(t) for t in text.split(",") if t.strip()]
    if n is not None and len(v) != n:
        raise argparse.ArgumentTypeError("expected %d comma-separated numbers, got %r" % (n, text))
    return v


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pred", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--max_dist", type=float, required=True)
    ap.add_argument("--tau", type=floats, default=[])
    thin = ap.add_mutually_exclusive_group()
    thin.add_argument("--voxel", type=float, default=None)
    thin.add_argument("--thin-dist", type=float, default=None)
    ap.add_argument("--thin-seed", type=int, default=0)
    ap.add_argument("--box", type=lambda t: floats(t, 6), default=None)
    ap.add_argument("--plane", type=lambda t: floats(t, 4), default=None)
    ap.add_argument("--align", default=None, help="4x4 text file: prediction -> ground-truth frame")
    ap.add_argument("--crop", default=None, help="SelectionPolygonVolume json")
    icp = ap.add_mutually_exclusive_group()
    icp.add_argument("--icp", type=float, default=None, metavar="DTAU")
    icp.add_argument("--no-icp", action="store_true")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("eval_cloud.py runs the MI355X path: no GPU")
    dev = torch.device(a.device)
    t0 = time.perf_counter()
    aligned = a.align is not None or a.crop is not None or a.icp is not None
    if a.no_icp and not (a.align or a.crop):
        ap.error("--no-icp goes with --align and / or --crop")
    T = data_io.read_alignment(a.align) if a.align else None
    crop = data_io.read_crop_volume(a.crop) if a.crop else None
    extra = {}
    if a.icp is not None:
        if a.voxel is not None or a.thin_dist is not None or a.box is not None or a.plane is not None:
            ap.error("--icp scores by the Tanks-and-Temples protocol: no --voxel, --thin-dist, --box or --plane")
        clouds = [torch.from_numpy(data_io.read_ply(path)[0]).to(dev) for path in (a.pred, a.gt)]
        t1 = time.perf_counter()
        with torch.cuda.device(dev):
            scores = cloud_eval.evaluate_tt(clouds[0], clouds[1], torch.eye(4).tolist() if T is None else T, crop, a.icp, max_dist=a.max_dist,
                                            taus=a.tau or None)
        t2 = time.perf_counter()
        scores.update(pred=a.pred, gt=a.gt, max_dist=a.max_dist, dtau=a.icp, align=a.align, crop=a.crop, points_read=[int(c.shape[0]) for c in clouds],
                      seconds=dict(read=t1 - t0, evaluate=t2 - t1))
        return write(a.out, scores)
    clouds, masks = [], []
    for k, path in enumerate((a.pred, a.gt)):
        xyz = torch.from_numpy(data_io.read_ply(path)[0]).to(dev)
        if aligned:
            with torch.cuda.device(dev):
                if k == 0 and T is not None:
                    xyz = cloud_eval.transform(xyz, T)
                if crop is not None:
                    xyz = xyz[cloud_eval.crop_polygon(xyz, crop["orthogonal_axis"], crop["axis_min"], crop["axis_max"], crop["bounding_polygon"])]
            extra["n_pred_cropped" if k == 0 else "n_gt_cropped"] = int(xyz.shape[0])
        mask = None
        if a.box is not None:
            mask = cloud_eval.in_box(xyz, a.box[:3], a.box[3:])
        if a.plane is not None:
            up = cloud_eval.above_plane(xyz, a.plane)
            mask = up if mask is None else mask & up
        clouds.append(xyz)
        masks.append(mask)
    t1 = time.perf_counter()
    scores = cloud_eval.evaluate(clouds[0], clouds[1], a.max_dist, a.tau, voxel=a.voxel, pred_mask=masks[0], gt_mask=masks[1],
                                 greedy=a.thin_dist, greedy_seed=a.thin_seed)
    t2 = time.perf_counter()
    scores.update(pred=a.pred, gt=a.gt, max_dist=a.max_dist, voxel=a.voxel, thin_dist=a.thin_dist, thin_seed=a.thin_seed, box=a.box, plane=a.plane, points_read=[int(c.shape[0]) for c in clouds],
                  seconds=dict(read=t1 - t0, evaluate=t2 - t1))
    if aligned:
        scores.update(extra, align=a.align, crop=a.crop, T=None if T is None else T.tolist(), stages=[])
    return write(a.out, scores)


def write(out, scores):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(scores, f, indent=1)
    print(json.dumps(scores))
    return scores


if __name__ == "__main__":
    main()
