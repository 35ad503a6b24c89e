"""TEST INFRASTRUCTURE - the gipuma-style fusion rule of include/mvs_hip.h (``mvs_gipuma_fuse_scene``) in numpy float32.

Every operation works on ``np.float32`` arrays (or scalars) and is rounded on its own, in the order the header writes it, so the device
result is reproduced bit for bit.  ``gipuma_rule`` is vectorised over the pixels of a reference view (the views and the sources of a view
are Python loops: the rule is sequential over them); ``gipuma_rule_pixelwise`` is the same rule as a plain loop over single pixels, the
form the header reads as.  ``make_scene`` stacks ``oracle.ref_fusion.make_fusion_case`` as tests/test_hip_pointcloud.py::_scene does.
"""
import numpy as np

F = np.float32
DEFAULTS = dict(disp_thresh=0.2, num_consistent=3, depth_min=0.001, depth_max=100000.0)


def make_scene(nv, h, w, seed):
    """-> depths [nv,h,w], confs [nv,3,h,w] (a low-confidence band per view), cams [nv,2,4,4], imgs [nv,3,h,w] uint8."""
    from oracle import ref_fusion
    import torch
    case = ref_fusion.make_fusion_case(n=1, v=nv - 1, h=h, w=w, seed=seed, noise=0.0005, outlier_frac=0.02)
    depths = torch.cat([case["ref_depth"], case["src_depths"][:, :, 0]], 1)[0].numpy()
    cams = torch.cat([case["ref_cam"][:, None], case["src_cams"]], 1)[0].numpy()
    confs = np.full((nv, 3, h, w), 0.9, np.float32)
    for v in range(nv):
        confs[v, v % 3, :3 + v % 4] = 0.1
    imgs = np.random.default_rng(seed).integers(0, 256, (nv, 3, h, w)).astype(np.uint8)
    return np.ascontiguousarray(depths, np.float32), confs, np.ascontiguousarray(cams, np.float32), imgs


def all_others(nv, order=None):
    order = list(range(nv)) if order is None else list(order)
    return [(r, [s for s in range(nv) if s != r]) for r in order]


def _world(B, c, x, y, d):
    return [((B[i, 0] * x + B[i, 1] * y) + B[i, 2]) * d + c[i] for i in range(3)]


def gipuma_rule(depth, tables, jobs=None, disp_thresh=0.2, num_consistent=3, depth_min=0.001, depth_max=100000.0):
    """-> dict: ``keep [R,H,W]`` bool, ``used [Nv,H,W]`` uint8, ``count [R,H,W]`` uint8, ``points [R,3,H,W]`` float32 (0 where not kept),
    ``eligible [R,H,W]`` bool, ``in_range [R,H,W]`` bool (eligible but for ``used``), ``consistent [R,Smax,H,W]`` bool and ``ddiff
    [R,Smax,H,W]`` float32 = |fb/z - fb/d_s| where the pair reached the disparity test, NaN elsewhere."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and all(t.dtype == np.float32 for t in tables)
    B, c, A, b, fb = tables
    nv, H, W = depth.shape
    jobs = all_others(nv) if jobs is None else jobs
    R, smax = len(jobs), max(len(s) for _, s in jobs)
    thr, ncons, dmin, dmax = F(disp_thresh), F(num_consistent), F(depth_min), F(depth_max)
    x = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    used = np.zeros((nv, H, W), np.uint8)
    keep = np.zeros((R, H, W), bool)
    eligible, in_range = np.zeros((R, H, W), bool), np.zeros((R, H, W), bool)
    count = np.zeros((R, H, W), np.uint8)
    points = np.zeros((R, 3, H, W), F)
    consistent = np.zeros((R, smax, H, W), bool)
    ddiff = np.full((R, smax, H, W), np.nan, F)
    with np.errstate(all="ignore"):
        for k, (r, srcs) in enumerate(jobs):
            assert r not in srcs
            d = depth[r]
            in_range[k] = (d > dmin) & (d < dmax)
            el = in_range[k] & (used[r] == 0)
            eligible[k] = el
            acc = _world(B[r], c[r], x, y, d)
            n = np.zeros((H, W), np.int32)
            marks = []
            for j, s in enumerate(srcs):
                q = [((A[r, s, i, 0] * x + A[r, s, i, 1] * y) + A[r, s, i, 2]) * d + b[r, s, i] for i in range(3)]
                z = q[2]
                ok = el & (z > F(0))
                fx = np.floor(q[0] / z + F(0.5))
                fy = np.floor(q[1] / z + F(0.5))
                ok = ok & (fx >= F(0)) & (fx < F(W)) & (fy >= F(0)) & (fy < F(H))
                ix = np.where(ok, fx, F(0)).astype(np.int64)
                iy = np.where(ok, fy, F(0)).astype(np.int64)
                ds = depth[s][iy, ix]
                ok = ok & (ds > dmin) & (ds < dmax)
                dd = np.abs(fb[r, s] / z - fb[r, s] / ds)
                ddiff[k, j] = np.where(ok, dd, F(np.nan))
                ok = ok & (dd < thr)
                xs = _world(B[s], c[s], fx, fy, ds)
                for i in range(3):
                    acc[i] = np.where(ok, acc[i] + xs[i], acc[i])
                n += ok
                consistent[k, j] = ok
                marks.append((s, iy, ix, ok))
            kp = el & (n.astype(F) >= ncons)
            keep[k] = kp
            count[k] = np.where(el, np.minimum(n, 255), 0).astype(np.uint8)
            div = (n + 1).astype(F)
            for i in range(3):
                points[k, i] = np.where(kp, acc[i] / div, F(0))
            for s, iy, ix, ok in marks:
                m = ok & kp
                used[s][iy[m], ix[m]] = 1
    return dict(keep=keep, used=used, count=count, points=points, eligible=eligible, in_range=in_range, consistent=consistent, ddiff=ddiff)


def gipuma_rule_pixelwise(depth, tables, jobs=None, disp_thresh=0.2, num_consistent=3, depth_min=0.001, depth_max=100000.0):
    """The same rule, one pixel at a time on ``np.float32`` scalars -> ``keep``, ``used``, ``count``, ``points`` as above."""
    B, c, A, b, fb = tables
    nv, H, W = depth.shape
    jobs = all_others(nv) if jobs is None else jobs
    thr, ncons, dmin, dmax = F(disp_thresh), F(num_consistent), F(depth_min), F(depth_max)
    used = np.zeros((nv, H, W), np.uint8)
    keep = np.zeros((len(jobs), H, W), bool)
    count = np.zeros((len(jobs), H, W), np.uint8)
    points = np.zeros((len(jobs), 3, H, W), F)
    with np.errstate(all="ignore"):
        for k, (r, srcs) in enumerate(jobs):
            for yi in range(H):
                for xi in range(W):
                    d = depth[r, yi, xi]
                    if not (dmin < d < dmax and used[r, yi, xi] == 0):
                        continue
                    x, y = F(xi), F(yi)
                    acc = _world(B[r], c[r], x, y, d)
                    n, marks = 0, []
                    for s in srcs:
                        q = [((A[r, s, i, 0] * x + A[r, s, i, 1] * y) + A[r, s, i, 2]) * d + b[r, s, i] for i in range(3)]
                        z = q[2]
                        if not z > F(0):
                            continue
                        fx, fy = np.floor(q[0] / z + F(0.5)), np.floor(q[1] / z + F(0.5))
                        if not (F(0) <= fx < F(W) and F(0) <= fy < F(H)):
                            continue
                        ix, iy = int(fx), int(fy)
                        ds = depth[s, iy, ix]
                        if not dmin < ds < dmax:
                            continue
                        if not np.abs(fb[r, s] / z - fb[r, s] / ds) < thr:
                            continue
                        xs = _world(B[s], c[s], fx, fy, ds)
                        acc = [acc[i] + xs[i] for i in range(3)]
                        n += 1
                        marks.append((s, iy, ix))
                    count[k, yi, xi] = min(n, 255)
                    if F(n) >= ncons:
                        keep[k, yi, xi] = True
                        for i in range(3):
                            points[k, i, yi, xi] = acc[i] / F(n + 1)
                        for s, iy, ix in marks:
                            used[s, iy, ix] = 1
    return dict(keep=keep, used=used, count=count, points=points)


def sequence_is_exercised(out, jobs, min_skipped=0.2, min_first=0.5):
    """What the issue asks of every scene, on the util's own output: the first job keeps at least ``min_first`` of its pixels, and in some
    later job at least ``min_skipped`` of the pixels that are in range were skipped because an earlier view had used them."""
    first = out["keep"][0].mean()
    skipped = [1.0 - out["eligible"][k].sum() / max(1, out["in_range"][k].sum()) for k in range(1, len(jobs))]
    return first >= min_first and max(skipped) >= min_skipped, (float(first), [float(s) for s in skipped])
