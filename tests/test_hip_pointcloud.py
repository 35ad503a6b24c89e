"""GPU tests of the scene-resident fusion (csrc/pointcloud.hip, ``fusion.SceneFusion`` / ``fuse_scan``): a whole scan -> one coloured
point cloud in the reference's order (test.py:404-549).

Bounds.  Against the per-view path (``fusion.filter_scan``) everything is exact: the scene kernels call the same device functions.
Against the CPU oracle the caps are those of tests/test_hip_fusion.py: keep-mask mismatch fraction < 2e-3 per job (a pixel within rounding
of a threshold may flip), points within 1e-5 * max|points| where both keep, colours equal.  ``stats`` are exact integer counts divided by
H*W in double; ``filter_scan`` reports the same fractions as float32 means, so the two agree as integers (round(fraction * H*W)) and
within one float32 ulp of a value <= 1 (2^-23).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
TH = [0.5, 0.5, 0.5]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _scene(nv, h, w, seed):
    """nv views of the slanted plane; a low-confidence band per view (its height differs from view to view), random uint8 images."""
    from oracle import ref_fusion
    case = ref_fusion.make_fusion_case(n=1, v=nv - 1, h=h, w=w, seed=seed, noise=0.0005, outlier_frac=0.02)
    depths = torch.cat([case["ref_depth"], case["src_depths"][:, :, 0]], 1)[0].numpy()
    cams = torch.cat([case["ref_cam"][:, None], case["src_cams"]], 1)[0].numpy()
    confs = np.full((nv, 3, h, w), 0.9, np.float32)
    for v in range(nv):
        confs[v, v % 3, :3 + v % 4] = 0.1
    imgs = np.random.default_rng(seed).integers(0, 256, (nv, 3, h, w)).astype(np.uint8)
    return depths, confs, cams, imgs


def _all_others(nv):
    return [(i, [j for j in range(nv) if j != i]) for i in range(nv)]


def _write(folder, depths, confs, cams, pairs, imgs=None):
    from mvsformer_amd import data_io
    from PIL import Image
    for i in range(len(depths)):
        data_io.save_depth_outputs(str(folder), i, depths[i], confs[i].transpose(1, 2, 0) if confs[i].ndim == 3 else confs[i], cams[i])
        if imgs is not None:
            os.makedirs(os.path.join(folder, "images"), exist_ok=True)
            Image.fromarray(imgs[i].transpose(1, 2, 0)).save(os.path.join(folder, "images/%08d.png" % i))
    with open(os.path.join(folder, "pair.txt"), "w") as f:
        f.write("%d\n" % len(pairs))
        for ref, srcs in pairs:
            f.write("%d\n%d %s\n" % (ref, len(srcs), " ".join("%d 1.0" % s for s in srcs)))


def _fusion(method, depths, confs, cams, imgs, pairs, dev, **kw):
    from mvsformer_amd import fusion
    kw.setdefault("prob_threshold", TH)
    sc = fusion.SceneFusion(method, thres_view=2, rel_diff_base=400, device=dev, **kw)
    for i in range(len(depths)):
        sc.add_view(i, depths[i], confs[i], cams[i], None if imgs is None else imgs[i])
    sc.set_pairs(pairs)
    return sc


PAIRS6 = {"pcd": [(0, [1, 2, 3, 4, 5]), (1, [0, 2]), (2, [5]), (3, [4, 5, 0, 1]), (5, [0, 1, 2])],
          "dypcd": [(0, [1, 2, 3, 4, 5]), (1, [0, 2]), (2, [5, 0]), (3, [4, 5, 0, 1]), (5, [0, 1, 2])]}


@pytest.mark.parametrize("method", ["pcd", "dypcd"])
@pytest.mark.parametrize("layout", ["all_others_5", "ragged_6"])
def test_same_answer_as_the_per_view_path(dev, tmp_path, method, layout):
    from mvsformer_amd import fusion
    nv = 5 if layout == "all_others_5" else 6
    h, w = 64, 80
    depths, confs, cams, imgs = _scene(nv, h, w, seed=2)
    pairs = _all_others(nv) if nv == 5 else PAIRS6[method]
    _write(tmp_path, depths, confs, cams, pairs)
    views = fusion.filter_scan(str(tmp_path), str(tmp_path), TH, method=method, thres_view=2, rel_diff_base=400)
    assert list(views) == [r for r, _ in pairs]
    got = _fusion(method, depths, confs, cams, imgs, pairs, dev).fuse()
    want_xyz = np.concatenate([views[r][0] for r, _ in pairs], 0)
    print("points", got["n_points"], "of", len(pairs) * h * w)
    assert got["xyz"].shape == want_xyz.shape and np.array_equal(got["xyz"].view(np.uint32), want_xyz.view(np.uint32))
    assert got["n_points"] == len(want_xyz) and got["counts_per_view"] == {r: len(views[r][0]) for r, _ in pairs}
    for r, _ in pairs:
        for k in ("photo", "geo", "final"):
            a, b = got["stats"][r][k], views[r][1][k]
            assert round(a * h * w) == round(b * h * w) and abs(a - b) <= 2.0 ** -23, (r, k, a, b)
        assert got["stats"][r]["final"] > 0.2


@pytest.mark.parametrize("method", ["pcd", "dypcd"])
def test_against_the_oracle(dev, method):
    from oracle import ref_fusion
    nv, h, w = 6, 64, 80
    depths, confs, cams, imgs = _scene(nv, h, w, seed=4)
    pairs = PAIRS6[method]
    got = _fusion(method, depths, confs, cams, imgs, pairs, dev).fuse(with_intermediates=True)
    T = torch.from_numpy
    photo = ref_fusion.prob_filter(T(confs), TH)[:, 0].numpy()                                  # [nv,h,w]
    ours_keep = (got["photo_mask"].cpu().numpy().astype(bool)[[r for r, _ in pairs]] & got["geo_mask"].cpu().numpy().astype(bool))
    ours_pts = got["points_dense"].cpu().numpy()
    assert np.array_equal(got["photo_mask"].cpu().numpy().astype(bool), photo)
    start = 0
    for i, (r, srcs) in enumerate(pairs):
        sd = T(depths[srcs])[None, :, None]
        if method == "pcd":
            sd = sd * T(photo[srcs])[None, :, None].float()
            want = ref_fusion.filter_depth_maps(T(depths[r])[None, None], sd, T(cams[r])[None], T(cams[srcs])[None], 1.0, 0.01, 2)
            geo = want["mask"][0, 0].numpy()
        else:
            want = ref_fusion.dynamic_filter_depth_maps(T(depths[r])[None, None], sd, T(cams[r])[None], T(cams[srcs])[None], 4, 400)
            geo = want["geo_mask"][0, 0].numpy()
        keep = photo[r] & geo
        wpts = want["points"][0].numpy()                                                         # [3,h,w]
        want_xyz = np.stack([wpts[k][keep] for k in range(3)], -1)                                # test.py:445-446
        want_rgb = np.stack([(imgs[r, k].astype(np.float32) / 255.)[keep] for k in range(3)], -1) * 255
        want_rgb = want_rgb.astype(np.uint8)                                                     # test.py:447-452
        mism = (ours_keep[i] != keep).mean()
        print("job", i, "ref", r, "kept", keep.mean(), "mask mismatch", mism)
        assert keep.mean() > 0.2 and ours_keep[i].mean() > 0.2
        assert mism < 2e-3
        n = int(ours_keep[i].sum())
        xyz, rgb = got["xyz"][start:start + n], got["rgb"][start:start + n]
        start += n
        # this job's slice of the cloud is numpy's boolean indexing of the job's own masks ...
        assert np.array_equal(xyz, np.stack([ours_pts[i, k][ours_keep[i]] for k in range(3)], -1))
        # ... and agrees with the oracle's cloud wherever both keep the pixel
        both_in_ours, both_in_want = keep[ours_keep[i]], ours_keep[i][keep]
        err = np.abs(xyz[both_in_ours] - want_xyz[both_in_want]).max()
        print("   max point error", err, "cap", 1e-5 * np.abs(wpts).max())
        assert err < 1e-5 * np.abs(wpts).max()
        assert np.array_equal(rgb[both_in_ours], want_rgb[both_in_want])
    assert start == got["n_points"] == len(got["xyz"])


def _expected(photo, geo, refs, points, imgs):
    keep = photo[refs] & geo
    xyz = np.concatenate([np.stack([points[i, k][keep[i]] for k in range(3)], -1) for i in range(len(refs))], 0)
    rgb = np.concatenate([np.stack([imgs[r, k][keep[i]] for k in range(3)], -1) for i, r in enumerate(refs)], 0)
    rec = np.empty(len(xyz), VERTEX)
    for i, k in enumerate(("x", "y", "z")):
        rec[k] = xyz[:, i]
    for i, k in enumerate(("red", "green", "blue")):
        rec[k] = rgb[:, i]
    stats = np.stack([photo[refs].reshape(len(refs), -1).sum(1), geo.reshape(len(refs), -1).sum(1), keep.reshape(len(refs), -1).sum(1)], 1)
    return xyz, rgb, rec.tobytes(), stats


@pytest.mark.parametrize("pattern", ["zeros", "ones", "last_pixel", "checker", "rand0.01", "rand0.5", "rand0.99"])
def test_compaction_alone(dev, tmp_path, pattern):
    from mvsformer_amd import data_io, ops
    R, h, w = 3, 37, 101                                          # 3737 pixels: not a multiple of the block (256) or the wavefront (64)
    refs = [2, 0, 1]
    rng = np.random.default_rng(11)
    photo = rng.random((3, h, w)) < 0.9
    if pattern == "zeros":
        geo = np.zeros((R, h, w), bool)
    elif pattern == "ones":
        geo, photo = np.ones((R, h, w), bool), np.ones((3, h, w), bool)
    elif pattern == "last_pixel":
        geo, photo = np.zeros((R, h, w), bool), np.ones((3, h, w), bool)
        geo[R - 1, h - 1, w - 1] = True
    elif pattern == "checker":
        geo = np.broadcast_to((np.add.outer(np.arange(h), np.arange(w)) % 2 == 0), (R, h, w)).copy()
    else:
        geo = rng.random((R, h, w)) < float(pattern[4:])
    points = rng.standard_normal((R, 3, h, w)).astype(np.float32)
    points[0, 0, 0, 0] = np.nan
    imgs = rng.integers(0, 256, (3, 3, h, w)).astype(np.uint8)
    xyz, rgb, rec, stats = _expected(photo, geo, refs, points, imgs)
    table = ops.JobTable([(r, [(r + 1) % 3]) for r in refs], 3, dev)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    args = (table, T(photo), T(geo), T(points), T(imgs))
    with ops.kernel_timer() as timer:
        a = ops.pointcloud_compact(*args)
    b = ops.pointcloud_compact(*args)
    print(pattern, "total", a["total"], "expected", len(xyz))
    assert a["total"] == len(xyz) and np.array_equal(a["stats"], stats)
    assert a["records"].cpu().numpy().tobytes() == rec
    assert np.array_equal(a["xyz"].cpu().numpy().view(np.uint32), xyz.view(np.uint32)) and np.array_equal(a["rgb"].cpu().numpy(), rgb)
    for k in ("records", "xyz", "rgb"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8))
    assert ("pointcloud_scatter" in timer.events) == (len(xyz) > 0)
    # records alone (what fuse_scan asks for) are the same bytes
    c = ops.pointcloud_compact(*args, want=("records",))
    assert c["records"].cpu().numpy().tobytes() == rec and "xyz" not in c
    path = str(tmp_path / "c.ply")
    data_io.write_ply_records(path, c["records"].cpu().numpy(), c["total"])
    gx, gc = data_io.read_ply(path)
    assert gx.shape == (len(xyz), 3) and np.array_equal(gx.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(gc, rgb)


@pytest.mark.parametrize("pattern", ["ones", "rand0.5"])
@pytest.mark.parametrize("nblocks", [1, 8191, 8192, 8193, 16385])
def test_compaction_at_the_scan_tile_edge(dev, nblocks, pattern):
    """One job whose 256-pixel blocks number 1, one below / at / one above the scan's 8192-count tile, and two tiles + 1: the running carry
    of the shared exclusive scan (csrc/block_ops.h) against numpy boolean indexing, exactly."""
    from mvsformer_amd import ops
    h, w = nblocks, 256
    rng = np.random.default_rng(100 + nblocks)
    photo = np.ones((1, h, w), bool)
    geo = np.ones((1, h, w), bool) if pattern == "ones" else rng.random((1, h, w)) < 0.5
    points = rng.standard_normal((1, 3, h, w)).astype(np.float32)
    imgs = rng.integers(0, 256, (1, 3, h, w)).astype(np.uint8)
    xyz, rgb, rec, stats = _expected(photo, geo, [0], points, imgs)
    table = ops.JobTable([(0, [0])], 1, dev)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    a = ops.pointcloud_compact(table, T(photo), T(geo), T(points), T(imgs))
    print(nblocks, pattern, "total", a["total"], "expected", len(xyz))
    assert a["total"] == len(xyz) and np.array_equal(a["stats"], stats)
    assert a["records"].cpu().numpy().tobytes() == rec
    assert np.array_equal(a["xyz"].cpu().numpy().view(np.uint32), xyz.view(np.uint32)) and np.array_equal(a["rgb"].cpu().numpy(), rgb)


def test_colours_all_levels(dev):
    from mvsformer_amd import ops
    k = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([k, 255 - k, k[::-1].copy()])[None]                                         # [1,3,16,16]
    imgf = img.astype(np.float32) / np.float32(255.)                                          # what the reference's read_img holds
    table = ops.JobTable([(0, [0])], 1, dev)
    ones = torch.ones(1, 16, 16, dtype=torch.bool, device=dev)
    pts = torch.zeros(1, 3, 16, 16, device=dev)
    want = img[0].reshape(3, 256).T
    for im in (img, imgf):
        out = ops.pointcloud_compact(table, ones, ones, pts, torch.from_numpy(np.ascontiguousarray(im)).to(dev))
        rgb = out["rgb"].cpu().numpy()
        assert np.array_equal(rgb[:, 0], np.arange(256)) and np.array_equal(rgb, want)
        assert np.array_equal(np.frombuffer(out["records"].cpu().numpy().tobytes(), VERTEX)["green"], 255 - np.arange(256))


@pytest.mark.parametrize("method", ["pcd", "dypcd"])
def test_fuse_scan_end_to_end(dev, tmp_path, method):
    from mvsformer_amd import data_io, fusion
    nv, h, w = 5, 64, 80
    depths, confs, cams, imgs = _scene(nv, h, w, seed=6)
    pairs = _all_others(nv)
    _write(tmp_path, depths, confs, cams, pairs, imgs)
    ply = str(tmp_path / "scan.ply")
    res = fusion.fuse_scan(str(tmp_path), str(tmp_path), ply, TH, method=method, thres_view=2, rel_diff_base=400)
    mem = _fusion(method, depths, confs, cams, imgs, pairs, dev).fuse()
    xyz, rgb = data_io.read_ply(ply)
    assert res["n_points"] == mem["n_points"] == len(xyz) > 0.2 * nv * h * w
    assert np.array_equal(xyz.view(np.uint32), mem["xyz"].view(np.uint32)) and np.array_equal(rgb, mem["rgb"])
    assert open(ply, "rb").read()[-15 * len(xyz):] == mem["records"].tobytes()
    assert res["stats"] == mem["stats"] and set(res["seconds"]) == {"load", "device", "write"}
    # float images in [0,1] (the reference's read_img) give the same bytes
    memf = _fusion(method, depths, confs, cams, imgs.astype(np.float32) / np.float32(255.), pairs, dev).fuse(want=("records",))
    assert memf["records"].tobytes() == mem["records"].tobytes()


def test_combine_conf(dev):
    """test.py:415-422: with --combine_conf the mask is ``conf > prob_threshold[0]`` on a single-channel confidence."""
    from mvsformer_amd import fusion
    nv, h, w = 5, 64, 80
    depths, confs, cams, imgs = _scene(nv, h, w, seed=8)
    conf1 = np.random.default_rng(3).random((nv, h, w)).astype(np.float32)
    pairs = _all_others(nv)
    got = _fusion("pcd", depths, conf1, cams, imgs, pairs, dev, prob_threshold=[0.3, 0.99, 0.99], combine_conf=True).fuse()
    photo = conf1 > np.float32(0.3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    xyz, rgb = [], []
    for r, srcs in pairs:
        sd = depths[srcs] * photo[srcs].astype(np.float32)                                      # test.py:416-419
        out = fusion.filter_depth_maps(T(depths[r])[None, None], T(sd)[None, :, None], T(cams[r])[None], T(cams[srcs])[None], 1.0, 0.01, 2)
        keep = photo[r] & out["mask"][0, 0].cpu().numpy()
        pts = out["points"][0].cpu().numpy()
        xyz.append(np.stack([pts[k][keep] for k in range(3)], -1))
        rgb.append(np.stack([imgs[r, k][keep] for k in range(3)], -1))
        assert got["stats"][r]["photo"] == photo[r].sum() / float(h * w) and got["counts_per_view"][r] == int(keep.sum())
    assert np.array_equal(got["xyz"].view(np.uint32), np.concatenate(xyz).view(np.uint32)) and np.array_equal(got["rgb"], np.concatenate(rgb))
    # further confidence channels are ignored under combine_conf
    conf3 = np.stack([conf1, np.zeros_like(conf1), np.zeros_like(conf1)], 1)
    got3 = _fusion("pcd", depths, conf3, cams, imgs, pairs, dev, prob_threshold=[0.3, 0.99, 0.99], combine_conf=True).fuse(want=("records",))
    assert got3["records"].tobytes() == got["records"].tobytes()


def test_errors_launch_nothing(dev):
    from oracle import ref_fusion
    from mvsformer_amd import fusion, ops
    from mvsformer_amd._lib import MvsHipError
    depths, confs, cams, imgs = _scene(3, 16, 16, seed=1)
    with ops.kernel_timer() as timer:
        sc = fusion.SceneFusion("pcd", TH, device=dev)
        with pytest.raises(MvsHipError):                                                          # CPU tensors
            sc.add_view(0, torch.from_numpy(depths[0]), torch.from_numpy(confs[0]), torch.from_numpy(cams[0]))
        sc.add_view(0, depths[0], confs[0], cams[0])
        with pytest.raises(MvsHipError):                                                          # H x W mismatch
            sc.add_view(1, depths[1][:, :8].copy(), confs[1][:, :, :8].copy(), cams[1])
        with pytest.raises(MvsHipError):
            sc.add_view(1, depths[1], confs[1], cams[1], imgs[1][:, :8])
        sc.add_view(1, depths[1], confs[1], cams[1])
        sc.set_pairs([(0, [1, 2])])
        with pytest.raises(ValueError):                                                           # view 2 was never added
            sc.fuse()
        big = ref_fusion.make_fusion_case(n=1, v=17, h=16, w=16)
        d = torch.cat([big["ref_depth"], big["src_depths"][:, :, 0]], 1)[0].numpy()
        c = torch.cat([big["ref_cam"][:, None], big["src_cams"]], 1)[0].numpy()
        dy = _fusion("dypcd", d, np.ones((18, 3, 16, 16), np.float32), c, None, [(0, list(range(1, 18))), (1, [0, 2])], dev)
        with pytest.raises(MvsHipError):                                                          # 17 sources in a dynamic job
            dy.fuse()
        dy.set_pairs([(0, [1]), (1, [0, 2])])
        with pytest.raises(MvsHipError):                                                          # and fewer than 2
            dy.fuse()
        with pytest.raises(ValueError):
            ops.JobTable([(0, [3])], 3, dev)
        with pytest.raises(MvsHipError):
            ops.pointcloud_compact(ops.JobTable([(0, [1])], 2, dev), torch.ones(2, 4, 4, dtype=torch.bool), torch.ones(1, 4, 4, dtype=torch.bool),
                                   torch.zeros(1, 3, 4, 4))
    assert not timer.events, list(timer.events)


def test_full_size_properties(dev):
    """11 views at 1536x1152, one job with 10 source views (test.py's n_src_views)."""
    h, w = 1152, 1536
    depths, confs, cams, imgs = _scene(11, h, w, seed=3)
    got = _fusion("pcd", depths, confs, cams, imgs, [(0, list(range(1, 11)))], dev).fuse(with_intermediates=True)
    keep = got["photo_mask"][0] & got["geo_mask"][0]
    n = int(keep.sum().item())
    print("full size: kept", n, "of", h * w)
    assert got["n_points"] == n == got["counts_per_view"][0] and n > 0.2 * h * w
    assert got["records"].shape == (15 * n,) and got["xyz"].shape == (n, 3) and got["rgb"].shape == (n, 3)
    rec = np.frombuffer(got["records"].tobytes(), VERTEX)
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], -1).view(np.uint32), got["xyz"].view(np.uint32))
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], -1), got["rgb"])
    keep_np = keep.cpu().numpy()
    pts = got["points_dense"][0].cpu().numpy()
    assert np.array_equal(got["xyz"], np.stack([pts[k][keep_np] for k in range(3)], -1))
    assert np.array_equal(got["rgb"], np.stack([imgs[0, k][keep_np] for k in range(3)], -1))
    nrm = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0])
    off = np.abs(got["xyz"].astype(np.float64) @ nrm - 600.0)
    assert np.quantile(off, 0.99) < 1.5
    assert got["stats"][0]["final"] == n / float(h * w)
