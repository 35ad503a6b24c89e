#!/usr/bin/env python
"""Depth maps of one scan -> one coloured point cloud (PLY): the reference's ``pcd_filter_worker`` (test.py:552-560) on the HIP path.

    python tools/fuse_scan.py --pair_folder <dir with pair.txt> --scan_folder <dir with depth_est/ confidence/ cams/ images/> \
        --ply out.ply --filter_method pcd --prob_threshold 0.5,0.5,0.5,0.5

Flag names follow the reference's test.py; ``--filter_method dpcd`` is its dynamic check (``dynamic_filter_depth``), ``--filter_method
gipuma`` the sequential disparity rule that stands where the reference runs the external ``fusibile`` binary (``--disp_threshold``,
``--num_consistent``; every view against all others in ascending id; the rule is restated, parity with the binary is unverified).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pair_folder", required=True)
    ap.add_argument("--scan_folder", required=True)
    ap.add_argument("--ply", required=True)
    ap.add_argument("--filter_method", default="pcd", choices=["pcd", "dpcd", "gipuma"])
    ap.add_argument("--prob_threshold", default="0.5,0.5,0.5,0.5")
    ap.add_argument("--thres_view", type=int, default=2)
    ap.add_argument("--thres_disp", type=float, default=1.0)
    ap.add_argument("--dist_base", type=float, default=4)
    ap.add_argument("--rel_diff_base", type=float, default=1300)
    ap.add_argument("--disp_threshold", type=float, default=0.2)
    ap.add_argument("--num_consistent", type=int, default=3)
    ap.add_argument("--combine_conf", action="store_true")
    ap.add_argument("--n_src_views", type=int, default=10)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    from mvsformer_amd import fusion
    if a.filter_method == "gipuma":
        out = fusion.gipuma_fuse_scan(a.pair_folder, a.scan_folder, a.ply, [float(p) for p in a.prob_threshold.split(",")],
                                      disp_threshold=a.disp_threshold, num_consistent=a.num_consistent, combine_conf=a.combine_conf,
                                      n_src_views=a.n_src_views, device=a.device)
    else:
        out = fusion.fuse_scan(a.pair_folder, a.scan_folder, a.ply, [float(p) for p in a.prob_threshold.split(",")],
                               method="pcd" if a.filter_method == "pcd" else "dypcd", thres_disp=a.thres_disp, thres_view=a.thres_view,
                               dist_base=a.dist_base, rel_diff_base=a.rel_diff_base, combine_conf=a.combine_conf, n_src_views=a.n_src_views,
                               device=a.device)
    for vid, st in out["stats"].items():
        print("ref-view{:0>2}, photo/geo/final-mask:{}/{}/{}".format(vid, st["photo"], st["geo"], st["final"]))
    print(json.dumps(dict(ply=a.ply, n_points=out["n_points"], seconds=out["seconds"])))


if __name__ == "__main__":
    main()
