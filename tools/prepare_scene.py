#!/usr/bin/env python
"""From a COLMAP sparse model (text export, undistorted images) to what the pipeline reads: ``SCAN/pair.txt`` and
``SCAN/cams/%08d_cam.txt`` with a depth range per view - the step before ``tools/infer_scan.py``.

    python tools/prepare_scene.py --colmap MODEL_DIR --out SCAN [--num_views 20 --num_depth 192 --interval_scale 1.0
                                  --theta0 5 --sigma1 1 --sigma2 10 --lo 0.01 --hi 0.99 --keep_zero]

View selection and depth ranges run on the device (``mvsformer_amd.scene_prep``).  The rule is RESTATED from memory of MVSNet's
``colmap2mvsnet.py``; every constant is an argument and parity with the original script is UNVERIFIED (include/mvs_scene_prep.h, "Scene
preparation").  Views are numbered in ascending ``IMAGE_ID``; ``SCAN/images.txt`` lists ``view index, image name`` so that the images
can be copied to ``SCAN/images/%08d.jpg``.
"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mvsformer_amd import data_io, scene_prep  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--colmap", required=True, help="folder with cameras.txt, images.txt, points3D.txt")
    ap.add_argument("--out", required=True, help="scan folder to write")
    ap.add_argument("--num_views", type=int, default=20)
    ap.add_argument("--num_depth", type=int, default=192)
    ap.add_argument("--interval_scale", type=float, default=1.0)
    ap.add_argument("--theta0", type=float, default=5.0)
    ap.add_argument("--sigma1", type=float, default=1.0)
    ap.add_argument("--sigma2", type=float, default=10.0)
    ap.add_argument("--lo", type=float, default=0.01)
    ap.add_argument("--hi", type=float, default=0.99)
    ap.add_argument("--keep_zero", action="store_true", help="also list sources that share no point with the view")
    a = ap.parse_args(argv)
    m = data_io.read_colmap_text(a.colmap)
    res = scene_prep.prepare_scene(m["xyz"], m["obs_point"], m["obs_view"], m["R"], m["t"], num_views=a.num_views, num_depth=a.num_depth,
                                   interval_scale=a.interval_scale, theta0=a.theta0, sigma1=a.sigma1, sigma2=a.sigma2, lo=a.lo, hi=a.hi,
                                   keep_zero=a.keep_zero)
    scene_prep.write_scan(a.out, res, m["R"], m["t"], m["K"], num_depth=a.num_depth)
    with open(os.path.join(a.out, "images.txt"), "w") as f:
        f.write("".join("%d %s\n" % (v, name) for v, name in enumerate(m["names"])))
    empty = [v for v, n in enumerate(res["n_points"]) if n == 0]
    print("%d views, %d points (%d non-finite), %d observations -> %s; %d views without a point%s" % (
        len(m["R"]), len(m["xyz"]), res["n_nonfinite"], len(m["obs_point"]), a.out, len(empty), (": %s" % empty[:8]) if empty else ""))
    return res


if __name__ == "__main__":
    main()
