"""Point-cloud evaluation on the MI355X (csrc/cloud_eval.hip, mvsformer_amd/cloud_eval.py) against the fp64 brute force of
tests/cloud_eval_util.py.  tests/test_cloud_eval_refs.py checks on the CPU that the cases keep the premises used here: no nearest distance
within 8 fp32 ulp of a bound (so "capped or not" must match exactly), coordinates within +-2^10 and distinct targets more than 1e-3 apart
(so a wrong neighbour is always farther off than the tolerance)."""
import math

import numpy as np
import pytest
import torch

import cloud_eval_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_nn(case, ref, dev):
    from mvsformer_amd import cloud_eval
    want_d, want_i, raw = ref
    src, dst, md = case["src"], case["dst"], case["max_dist"]
    dist, idx = cloud_eval.nn_distance(_t(src, dev), _t(dst, dev), md, cell=case["cell"])
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and dist.shape == idx.shape == (len(src),)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert np.abs(src[np.isfinite(src)]).max(initial=0.0) <= 1024.0 and np.abs(dst[np.isfinite(dst)]).max(initial=0.0) <= 1024.0
    capped = want_i < 0
    assert ((idx < 0) == capped).all(), np.nonzero((idx < 0) != capped)[0][:8]
    assert (dist[capped] == np.float32(md)).all() and (idx[capped] == -1).all()
    hit = ~capped
    assert ((idx[hit] >= 0) & (idx[hit] < len(dst))).all()
    tol = U.ULPS * np.spacing(want_d[hit].astype(np.float32)).astype(np.float64)
    err = np.abs(dist[hit].astype(np.float64) - want_d[hit])
    assert (err <= tol).all(), (err.max(), tol[err.argmax()])
    again = np.linalg.norm(src[hit].astype(np.float64) - dst[idx[hit]].astype(np.float64), axis=1)          # the index names that neighbour
    assert (np.abs(again - dist[hit]) <= tol).all()
    if "exact" in case:
        assert idx[case["exact"][0]] == case["exact"][1]


@pytest.mark.parametrize("n", U.SIZES)
@pytest.mark.parametrize("m", U.SIZES)
def test_nn_distance_sizes(dev, m, n):
    case, ref = U.reference("size", (m, n))
    _check_nn(case, ref, dev)


@pytest.mark.parametrize("name", sorted(U.geometry_cases()))
def test_nn_distance_geometries(dev, name):
    case, ref = U.reference("geometry", name)
    _check_nn(case, ref, dev)


@pytest.mark.parametrize("n", [256 * 8192, 256 * 8192 + 1])
def test_index_at_the_scan_tile_edge(dev, n):
    """8192 and 8193 blocks of 256 points: the shared exclusive scan (csrc/block_ops.h) fills exactly one tile / starts a second one with a
    carry.  The number of occupied cells against numpy's fp32 cell rule, and every point finding itself."""
    from mvsformer_amd import cloud_eval
    r = np.random.default_rng(n)
    xyz = r.random((n, 3)) * 100.0
    xyz[:, 0] = r.permutation(n) * (100.0 / n)                    # 4.8e-5 apart, fp32 spacing below 100 is 7.6e-6: the points are distinct
    xyz = U.f32(xyz)
    assert len(np.unique(xyz[:, 0])) == n
    cell = 1.0                                                    # ~1e6 cells, about two points each
    c = U.cell_index(xyz, xyz.min(axis=0), cell)
    n_cells = len(np.unique(c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)))
    t = _t(xyz, dev)
    out = cloud_eval.voxel_downsample(t, cell)
    print(n, "voxels", out.shape[0], "expected", n_cells)
    assert out.shape[0] == n_cells
    dist, idx = cloud_eval.nn_distance(t, t, 0.5, cell=cell)
    assert torch.equal(idx, torch.arange(n, device=idx.device)) and int(torch.count_nonzero(dist)) == 0


def _voxel_clouds():
    r = np.random.default_rng(5)
    two = np.concatenate([r.uniform(0.0, 0.9, (129, 3)), r.uniform(0.0, 0.9, (128, 3)) + [1.0, 0.0, 0.0]])[r.permutation(257)]
    two[0] = 0.0                                                             # the origin: the split at x = 1 is then a voxel face
    nf = r.uniform(-3.0, 3.0, (300, 3))
    nf[::7, 2] = np.nan
    return {"random": (r.uniform(-6.0, 6.0, (5000, 3)), 0.75), "lattice": (r.integers(-8, 8, (1000, 3)) * 0.5, 0.5), "one_point": ([[1.5, -2.0, 3.0]], 0.2),
            "one_voxel": (r.uniform(2.0, 2.9, (300, 3)), 1.0), "two_voxels_257": (two, 1.0), "non_finite": (nf, 0.5)}


@pytest.mark.parametrize("name", sorted(_voxel_clouds()))
def test_voxel_downsample(dev, name):
    from mvsformer_amd import cloud_eval
    xyz, voxel = _voxel_clouds()[name]
    xyz = U.f32(xyz)
    rgb8 = np.random.default_rng(9).integers(0, 256, xyz.shape).astype(np.uint8)
    keys, (cen, col) = U.voxel_centroids(xyz, voxel, [rgb8.astype(np.float32)])
    got = cloud_eval.voxel_downsample(_t(xyz, dev), voxel)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(keys), 3)                 # the voxel set ...
    got = got.cpu().numpy()
    assert np.abs(got.astype(np.float64) - cen.astype(np.float32)).max() <= 1e-6 * voxel     # ... in the yardstick's order: centroid by centroid
    assert np.abs(got.astype(np.float64) - cen).max() <= 1e-6 * voxel                        # coordinates here stay within 16 voxels of zero
    if name == "two_voxels_257":
        assert len(keys) == 2 and keys.tolist() == [0, 1]
    if name in ("one_point", "one_voxel"):
        assert len(keys) == 1
    g2, c8 = cloud_eval.voxel_downsample(_t(xyz, dev), voxel, _t(rgb8, dev))
    assert torch.equal(g2.cpu(), torch.from_numpy(got)) and c8.dtype == torch.uint8
    assert np.abs(c8.cpu().numpy().astype(np.float64) - np.floor(col.astype(np.float32) + np.float32(0.5))).max() == 0
    _, cf = cloud_eval.voxel_downsample(_t(xyz, dev), voxel, _t(rgb8.astype(np.float32), dev))
    assert cf.dtype == torch.float32 and np.abs(cf.cpu().numpy().astype(np.float64) - col).max() <= 255 * 2.0 ** -23


def test_voxel_downsample_empty(dev):
    from mvsformer_amd import cloud_eval
    e = torch.empty(0, 3, device=dev)
    assert tuple(cloud_eval.voxel_downsample(e, 0.5).shape) == (0, 3)
    x, c = cloud_eval.voxel_downsample(e, 0.5, torch.empty(0, 3, dtype=torch.uint8, device=dev))
    assert tuple(x.shape) == (0, 3) and tuple(c.shape) == (0, 3) and c.dtype == torch.uint8
    assert tuple(cloud_eval.voxel_downsample(torch.full((5, 3), float("nan"), device=dev), 0.5).shape) == (0, 3)


def _check_scores(got, want):
    for k in ("n_pred", "n_gt", "pred_below_max", "gt_below_max", "pred_below_tau", "gt_below_tau"):
        assert got[k] == want[k], (k, got[k], want[k])
    flat = lambda r, k: r[k] if isinstance(r[k], list) else [r[k]]         # noqa: E731
    for k in ("accuracy", "completeness", "overall", "precision", "recall", "fscore"):
        for g, w in zip(flat(got, k), flat(want, k)):
            assert (math.isnan(g) and math.isnan(w)) or abs(g - w) <= 1e-6 * abs(w), (k, g, w)


@pytest.mark.parametrize("voxel", [None, 1.0])
@pytest.mark.parametrize("masks", [False, True])
@pytest.mark.parametrize("name", sorted(U.eval_clouds()))
def test_evaluate(dev, name, masks, voxel):
    from mvsformer_amd import cloud_eval
    pred, gt, md = U.eval_clouds()[name]
    taus = (0.5 * md, md)
    pm = gm = None
    if masks:
        lo, hi = gt.min(axis=0) + 2.0, gt.max(axis=0) - 1.0
        pm = cloud_eval.in_box(_t(pred, dev), lo.tolist(), hi.tolist())
        c = gt.mean(axis=0, dtype=np.float64)
        plane = [0.0, 0.6, 0.8, -(0.6 * float(c[1]) + 0.8 * float(c[2]))]        # through the centroid: about half of the points are above
        gm = cloud_eval.above_plane(_t(gt, dev), plane)
        assert (pm.cpu().numpy() == ((pred >= lo) & (pred <= hi)).all(axis=1)).all()
        assert (gm.cpu().numpy() == (gt.astype(np.float64) @ plane[:3] + plane[3] > 0)).sum() >= len(gt) - 2        # fp32 / fp64 at the plane
        pm_h, gm_h = pm.cpu().numpy(), gm.cpu().numpy()
        assert 0 < pm_h.sum() < len(pred) and 0 < gm_h.sum() < len(gt)
    want = U.evaluate_ref(pred, gt, md, taus, voxel, None if pm is None else pm_h, None if gm is None else gm_h)
    for t in taus:
        assert U.clear_of(want["all_dist"], t)
    got = cloud_eval.evaluate(_t(pred, dev), _t(gt, dev), md, taus, voxel=voxel, pred_mask=pm, gt_mask=gm)
    _check_scores(got, want)
    swapped = cloud_eval.evaluate(_t(gt, dev), _t(pred, dev), md, taus, voxel=voxel, pred_mask=gm, gt_mask=pm)             # the other direction
    assert swapped["accuracy"] == got["completeness"] and swapped["recall"] == got["precision"] and swapped["n_pred"] == got["n_gt"]


def test_evaluate_empty_sets_give_nan(dev):
    from mvsformer_amd import cloud_eval
    pred, gt, md = U.eval_clouds()["plane"]
    none = torch.zeros(len(pred), dtype=torch.bool, device=dev)
    r = cloud_eval.evaluate(_t(pred, dev), _t(gt, dev), md, (md,), pred_mask=none)
    _check_scores(r, U.evaluate_ref(pred, gt, md, (md,), pred_mask=np.zeros(len(pred), bool)))
    assert r["n_pred"] == 0 and math.isnan(r["accuracy"]) and math.isnan(r["completeness"]) and math.isnan(r["overall"])
    assert math.isnan(r["precision"][0]) and r["recall"] == [0.0] and math.isnan(r["fscore"][0])
    r = cloud_eval.evaluate(torch.empty(0, 3, device=dev), torch.empty(0, 3, device=dev), md, (md,))
    assert r["n_pred"] == r["n_gt"] == 0 and math.isnan(r["accuracy"]) and math.isnan(r["recall"][0])
    far = cloud_eval.evaluate(_t(pred, dev), _t(gt + np.float32(500.0), dev), md, (md,))          # nothing within max_dist: shares 0, F-score 0
    assert far["pred_below_max"] == 0 and math.isnan(far["accuracy"]) and far["precision"] == [0.0] and far["fscore"] == [0.0]


def test_in_volume(dev):
    from mvsformer_amd import cloud_eval
    occ = np.zeros((4, 5, 6), np.uint8)
    occ[1, 2, 3] = occ[3, 4, 5] = 1
    pts = np.array([[1.0, 2.0, 3.0], [1.2, 2.2, 2.8], [3.0, 4.0, 5.0], [0.0, 0.0, 0.0], [4.0, 4.0, 5.0], [-1.0, 2.0, 3.0], [np.nan, 2.0, 3.0]], np.float32)
    m = cloud_eval.in_volume(_t(pts * 0.5 + 10.0, dev), _t(occ, dev), [10.0, 10.0, 10.0], 0.5)
    assert m.cpu().tolist() == [True, True, True, False, False, False, False]


def test_two_calls_give_the_same_bits(dev):
    from mvsformer_amd import cloud_eval
    pred, gt, md = U.eval_clouds()["sphere"]
    p, g = _t(pred, dev), _t(gt, dev)
    a, b = cloud_eval.nn_distance(p, g, md), cloud_eval.nn_distance(p, g, md)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    rgb = torch.rand(len(gt), 3, device=dev)
    a, b = cloud_eval.voxel_downsample(g, 0.7, rgb), cloud_eval.voxel_downsample(g, 0.7, rgb)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = cloud_eval.evaluate(p, g, md, (0.5 * md, md), voxel=0.7), cloud_eval.evaluate(p, g, md, (0.5 * md, md), voxel=0.7)
    assert {k: str(v) for k, v in a.items()} == {k: str(v) for k, v in b.items()}             # str: nan equals nan


def test_bad_arguments_are_refused(dev):
    from mvsformer_amd import cloud_eval, ops
    from mvsformer_amd._lib import MvsHipError
    p = _t(U.plane_patch(100, 1), dev)
    with ops.kernel_timer() as timer:
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(MvsHipError):
                cloud_eval.nn_distance(p, p, 1.0, cell=bad)
            with pytest.raises(MvsHipError):
                cloud_eval.voxel_downsample(p, bad)
        for bad_md in (0.0, float("inf"), float("nan")):
            with pytest.raises(MvsHipError):
                cloud_eval.nn_distance(p, p, bad_md)
        with pytest.raises(MvsHipError):
            cloud_eval.evaluate(p, p, 1.0, taus=(0.5, 1.5))                   # a tau > max_dist
        with pytest.raises(MvsHipError):
            cloud_eval.evaluate(p, p, 1.0, taus=[0.1] * 9)
        with pytest.raises(MvsHipError):
            cloud_eval.nn_distance(p.view(-1, 2), p, 1.0)                    # not [*,3]
        with pytest.raises(MvsHipError):
            cloud_eval.nn_distance(p, p.view(-1), 1.0)
        with pytest.raises(MvsHipError):
            cloud_eval.nn_distance(p, p.cpu(), 1.0)
        with pytest.raises(MvsHipError):
            cloud_eval.nn_distance(p, p, 1.0, cell=1.0 / 40)                 # more shells than are walked
        assert timer.order == []                                             # none of these reached the library
        wide = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2097152.0 * 2.0 ** -12, 1.0]], device=dev)      # 2^21 cells of 2^-12 along y: at the limit
        with pytest.raises(MvsHipError, match="2\\^21"):
            cloud_eval.nn_distance(p, wide, 2.0 ** -10, cell=2.0 ** -12)
        # the bounds are a device result, so that launch ran; the key entry then refused on the host and launched nothing
        assert timer.order == ["cloud_bounds", "cloud_grid_keys"]
        below = torch.tensor([[0.0, 0.0, 0.0], [1.0, 2097151.0 * 2.0 ** -12, 1.0]], device=dev)     # one cell fewer: indexed
        d, i = cloud_eval.nn_distance(below, below, 2.0 ** -10, cell=2.0 ** -12)
        assert d.tolist() == [0.0, 0.0] and i.tolist() == [0, 1]
    # the library's own refusals surface as MvsHipError through the thin wrappers
    with pytest.raises(MvsHipError):
        ops.cloud_score(torch.zeros(4, device=dev), 1.0, taus=(2.0,))


def test_scene_fusion_output_is_scored_where_it_is(dev, tmp_path):
    """``SceneFusion.fuse(on_device=True)['xyz']`` goes into ``evaluate`` as it is; the scores equal those of the same points after a PLY
    round trip (tools/eval_cloud.py's route)."""
    from mvsformer_amd import cloud_eval, data_io
    from test_hip_pointcloud import _all_others, _fusion, _scene
    depths, confs, cams, imgs = _scene(4, 24, 32, 3)
    sc = _fusion("pcd", depths, confs, cams, imgs, _all_others(4), dev)
    out = sc.fuse(want=("xyz", "rgb"), on_device=True)
    xyz = out["xyz"]
    assert isinstance(xyz, torch.Tensor) and xyz.is_cuda and xyz.shape[0] == out["n_points"] > 50
    gt = xyz[::2] + 0.01
    ext = float((xyz.amax(0) - xyz.amin(0)).max())
    md = 0.05 * ext
    a = cloud_eval.evaluate(xyz, gt, md, (0.5 * md,))
    path = str(tmp_path / "pred.ply")
    data_io.write_ply(path, xyz.cpu().numpy(), out["rgb"].cpu().numpy())
    back, _ = data_io.read_ply(path)
    b = cloud_eval.evaluate(_t(back, dev), gt, md, (0.5 * md,))
    assert {k: str(v) for k, v in a.items()} == {k: str(v) for k, v in b.items()}
    _check_scores(a, U.evaluate_ref(xyz.cpu().numpy(), gt.cpu().numpy(), md, (0.5 * md,)))
    host = sc.fuse(want=("xyz",))["xyz"]                                     # the default still returns numpy
    assert isinstance(host, np.ndarray) and np.array_equal(host, xyz.cpu().numpy())
