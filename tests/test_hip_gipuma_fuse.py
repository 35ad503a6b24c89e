"""GPU tests of the gipuma-style sequential fusion (csrc/gipuma.hip, ``ops.gipuma_fuse_scene``, ``fusion.GipumaFusion`` / ``gipuma_fuse_scan``).

The bound is bit equality with tests/gipuma_fuse_util.py everywhere: ``keep``, ``used``, ``count`` and ``points``.  The rule's decisions feed
later decisions (a kept pixel marks source pixels as used, a later view skips them), so "a few flipped pixels" is not a bound that means
anything; the header states the rule in single float32 operations and numpy float32 repeats them.

Every scene must exercise the sequence, checked on the util's own output: view 0 keeps at least half of its pixels and some later view
skips at least 20 % of its in-range pixels because they were used.  Where no pixel can be kept at all (``num_consistent`` above the number
of sources: the two tiny shapes at ``num_consistent = 3``, and ``num_consistent = Nv``) the check that stands in is that nothing is kept
and nothing is used.
"""
import os

import numpy as np
import pytest
import torch

import gipuma_fuse_util as gu

pytestmark = pytest.mark.gpu

VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
TH = [0.5, 0.5, 0.5]
_scenes = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _scene(nv, h, w, seed=3):
    """Scene and host tables, built once per shape and never modified (tests copy what they change)."""
    from mvsformer_amd import fusion
    key = (nv, h, w, seed)
    if key not in _scenes:
        depths, confs, cams, imgs = gu.make_scene(nv, h, w, seed)
        _scenes[key] = (depths, confs, cams, imgs, fusion.gipuma_tables(cams))
    return _scenes[key]


def _run(dev, depths, tables, jobs=None, **kw):
    from mvsformer_amd import ops
    table = None if jobs is None else ops.JobTable(jobs, len(depths), dev)
    out = ops.gipuma_fuse_scene(torch.from_numpy(depths).to(dev), tuple(torch.from_numpy(t).to(dev) for t in tables), table,
                                want_count=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_equal(got, want, what=""):
    assert np.array_equal(got["keep"], want["keep"]), (what, "keep", int((got["keep"] != want["keep"]).sum()))
    assert np.array_equal(got["used"], want["used"]), (what, "used", int((got["used"] != want["used"]).sum()))
    assert np.array_equal(got["count"], want["count"]), (what, "count")
    assert np.array_equal(got["points"].view(np.uint32), want["points"].view(np.uint32)), (what, "points")


def _check(dev, depths, tables, jobs=None, exercised=True, **kw):
    want = gu.gipuma_rule(depths, tables, jobs, **kw)
    nv = len(depths)
    if exercised:
        ok, seen = gu.sequence_is_exercised(want, jobs or gu.all_others(nv))
        assert ok, seen
    got = _run(dev, depths, tables, jobs, **kw)
    _assert_equal(got, want, (depths.shape, kw))
    return got, want


@pytest.mark.parametrize("shape", [(5, 37, 53), (6, 48, 64), (3, 5, 1), (2, 1, 7)])
@pytest.mark.parametrize("disp_thresh", [0.2, 1.0])
@pytest.mark.parametrize("num_consistent", [1, 3])
def test_bit_equal_to_the_rule(dev, shape, disp_thresh, num_consistent):
    nv = shape[0]
    depths, _, _, _, tables = _scene(*shape)
    possible = num_consistent <= nv - 1
    got, want = _check(dev, depths, tables, exercised=possible, disp_thresh=disp_thresh, num_consistent=num_consistent)
    if not possible:
        assert not want["keep"].any() and not want["used"].any()
    else:
        assert want["keep"][0].mean() >= 0.5


@pytest.mark.parametrize("shape", [(5, 37, 53), (6, 48, 64), (3, 5, 1), (2, 1, 7)])
def test_num_consistent_zero_and_all_views(dev, shape):
    nv = shape[0]
    depths, _, _, _, tables = _scene(*shape)
    got, want = _check(dev, depths, tables, num_consistent=0)
    assert np.array_equal(want["keep"], want["eligible"])                     # no source needed: every eligible pixel is kept
    got, want = _check(dev, depths, tables, exercised=False, num_consistent=nv)
    assert not want["keep"].any() and not want["used"].any() and not got["points"].any() and want["count"].max() <= nv - 1


def test_reversed_view_order(dev):
    nv, h, w = 5, 37, 53
    depths, _, _, _, tables = _scene(nv, h, w)
    fwd, _ = _check(dev, depths, tables)
    jobs = gu.all_others(nv, order=range(nv - 1, -1, -1))
    rev, _ = _check(dev, depths, tables, jobs)
    assert not np.array_equal(rev["keep"][::-1], fwd["keep"])              # the same views, another order: another cloud
    assert rev["keep"][0].mean() >= 0.5 and fwd["keep"][nv - 1].mean() < 0.2


def test_job_table_sources(dev):
    """Rows with 1, 2 and Nv-1 sources in non-ascending order; views 2 and 5 are never a reference."""
    nv = 6
    depths, _, _, _, tables = _scene(nv, 48, 64)
    jobs = [(0, [5, 4, 3, 2, 1]), (3, [0]), (1, [4, 0]), (4, [2, 5, 0, 3, 1])]
    got, want = _check(dev, depths, tables, jobs, exercised=False, num_consistent=1)
    assert want["keep"][0].mean() >= 0.5 and want["keep"][1:].any()
    skipped = 1.0 - want["eligible"][1:].sum(axis=(1, 2)) / want["in_range"][1:].sum(axis=(1, 2))
    assert skipped.max() >= 0.2, skipped
    from mvsformer_amd import ops
    for bad in ([(0, [1, 0])], [(0, [1, 1])]):                               # the reference among its sources; a source twice
        with pytest.raises(ValueError):
            ops.gipuma_fuse_scene(torch.from_numpy(depths).to(dev), tuple(torch.from_numpy(t).to(dev) for t in tables),
                                  ops.JobTable(bad, nv, dev))


def test_bad_job_row_on_the_device_keeps_nothing(dev):
    """A row the host checks would have refused, written into the device table behind their back: the job keeps nothing and marks
    nothing, the other jobs are what the rule gives without it."""
    from mvsformer_amd import ops
    nv = 5
    depths, _, _, _, tables = _scene(nv, 37, 53)
    jobs = [(0, [1, 2, 3, 4]), (1, [0, 2, 3, 4]), (2, [0, 1, 3, 4])]
    want = gu.gipuma_rule(depths, tables, [jobs[0], jobs[2]])
    for col, value in ((1, 1), (0, nv), (3, -1)):                             # a source equal to the reference; indices out of range
        table = ops.JobTable(jobs, nv, dev)
        table.src_idx[1, col] = value
        out = ops.gipuma_fuse_scene(torch.from_numpy(depths).to(dev), tuple(torch.from_numpy(t).to(dev) for t in tables), table,
                                    want_count=True)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        assert not got["keep"][1].any() and not got["points"][1].any() and not got["count"][1].any()
        assert np.array_equal(got["keep"][[0, 2]], want["keep"]) and np.array_equal(got["used"], want["used"])
        assert np.array_equal(got["points"][[0, 2]].view(np.uint32), want["points"].view(np.uint32))


@pytest.mark.parametrize("nv", [35, 67])
def test_source_mask_crosses_a_word(dev, nv):
    """35 views: the per-thread source mask crosses bit 32.  67 views: 66 sources, the mask holds the last two, so the marking pass
    repeats the whole test for the first 64 - the result may not depend on which way a source is marked."""
    depths, _, _, _, tables = _scene(nv, 8, 9)
    got, want = _check(dev, depths, tables)
    assert want["count"].max() > 32
    if nv == 67:
        assert want["consistent"][0, :64].any() and want["consistent"][0, 64:].any()      # both ways of marking are taken


def test_exact_threshold(dev):
    nv, h, w = 5, 37, 53
    depths, _, _, _, tables = _scene(nv, h, w)
    base = gu.gipuma_rule(depths, tables)
    dd = np.where(base["consistent"][0], base["ddiff"][0], -1.0)
    j, y, x = np.unravel_index(np.argmax(dd), dd.shape)                       # the widest consistent pair of view 0
    delta = np.float32(dd[j, y, x])
    assert 0 < delta < 0.2
    got, want = _check(dev, depths, tables, disp_thresh=delta)
    assert not want["consistent"][0, j, y, x] and want["ddiff"][0, j, y, x] == delta
    up = np.nextafter(delta, np.float32(np.inf), dtype=np.float32)
    got2, want2 = _check(dev, depths, tables, disp_thresh=up)
    assert want2["consistent"][0, j, y, x] and got2["count"][0, y, x] == got["count"][0, y, x] + 1


def test_edges(dev):
    nv, h, w = 5, 37, 53
    depths, _, cams, _, tables = _scene(nv, h, w)
    from mvsformer_amd import fusion
    d = depths.copy()
    dmin, dmax = np.float32(1.0), np.float32(5000.0)
    d[0, 3, 4], d[0, 3, 5], d[1, 10, 10], d[1, 10, 11] = dmin, dmax, dmin, dmax             # exactly on a limit: not eligible, not a source
    d[2, 5:9, 7:30], d[3, 20:22, :], d[2, 30, 3] = np.nan, -600.0, np.inf
    got, want = _check(dev, d, tables, exercised=False, depth_min=dmin, depth_max=dmax)
    assert not want["eligible"][0, 3, 4] and not want["eligible"][0, 3, 5] and want["keep"][0].mean() > 0.5
    assert not got["keep"][2, 5:9, 7:30].any() and not got["keep"][3, 20:22].any()
    # view 1 turned to look away (z <= 0 for every pixel of every other view), view 2 moved far to the side (out of frame), view 4 a
    # duplicate of view 0's camera (fb = 0: consistent wherever both depths are valid)
    c = cams.copy()
    c[1, 0, :3, :3] = np.diag([1.0, -1.0, -1.0]).astype(np.float32) @ c[1, 0, :3, :3]
    c[1, 0, :3, 3] = np.diag([1.0, -1.0, -1.0]).astype(np.float32) @ c[1, 0, :3, 3]
    c[2, 0, 0, 3] += 5000.0
    c[4] = c[0]
    tabs = fusion.gipuma_tables(c)
    assert tabs[4][0, 4] == 0 and tabs[4][4, 0] == 0
    d2 = depths.copy()
    d2[4] = depths[0]
    got, want = _check(dev, d2, tabs, exercised=False, num_consistent=1)
    jobs = gu.all_others(nv)
    assert not want["consistent"][0, jobs[0][1].index(1)].any() and not want["consistent"][0, jobs[0][1].index(2)].any()
    both = want["in_range"][0]
    assert np.array_equal(want["consistent"][0, jobs[0][1].index(4)], both) and want["used"][4].sum() >= both.sum() * 0.99
    assert not want["eligible"][4][both].any()                                  # the duplicate finds every pixel used


def test_empty_scan(dev, monkeypatch):
    from mvsformer_amd import fusion, ops
    nv, h, w = 3, 6, 7
    _, confs, cams, imgs, tables = _scene(nv, h, w)
    zeros = np.zeros((nv, h, w), np.float32)
    got, want = _check(dev, zeros, tables, exercised=False)
    assert not got["keep"].any() and not got["used"].any() and not got["points"].any()
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    sc = fusion.GipumaFusion(TH, device=dev)
    for i in range(nv):
        sc.add_view(i, zeros[i], confs[i], cams[i], imgs[i])
    out = sc.fuse()
    assert out["n_points"] == 0 and out["xyz"].shape == (0, 3) and len(out["records"]) == 0
    assert "mvs_gipuma_fuse_scene" in calls and "mvs_pointcloud_count" in calls and "mvs_pointcloud_scatter" not in calls


def _write(folder, depths, confs, cams, imgs):
    from mvsformer_amd import data_io
    from PIL import Image
    nv = len(depths)
    os.makedirs(os.path.join(folder, "images"), exist_ok=True)
    for i in range(nv):
        data_io.save_depth_outputs(str(folder), i, depths[i], confs[i].transpose(1, 2, 0), cams[i])
        Image.fromarray(imgs[i].transpose(1, 2, 0)).save(os.path.join(folder, "images/%08d.png" % i))
    with open(os.path.join(folder, "pair.txt"), "w") as f:                       # listed out of order: the route sorts the view ids
        f.write("%d\n" % nv)
        for ref in list(range(nv))[::-1]:
            srcs = [s for s in range(nv) if s != ref][:2]
            f.write("%d\n%d %s\n" % (ref, len(srcs), " ".join("%d 1.0" % s for s in srcs)))


def test_fusion_class_and_scan_from_a_folder(dev, tmp_path):
    from mvsformer_amd import data_io, fusion
    from mvsformer_amd._lib import MvsHipError
    nv, h, w = 5, 37, 53
    depths, confs, cams, imgs, _ = _scene(nv, h, w)
    _write(tmp_path, depths, confs, cams, imgs)
    # what the files hold (the camera file is text: the tables come from the values read back)
    scene = data_io.load_scene(str(tmp_path), str(tmp_path))
    order = np.argsort(scene["view_ids"])
    assert [scene["view_ids"][i] for i in order] == list(range(nv))
    d, cf, cm = scene["depths"][order], scene["confs"][order], scene["cams"][order]
    assert np.array_equal(d, depths) and np.array_equal(cf, confs)
    photo = (cf > np.float32(0.5)).all(axis=1)
    want = gu.gipuma_rule(np.where(photo, d, np.float32(0)).astype(np.float32), fusion.gipuma_tables(cm))
    ok, seen = gu.sequence_is_exercised(want, gu.all_others(nv))
    assert ok, seen
    assert not (want["keep"] & ~photo).any()
    xyz = np.concatenate([np.stack([want["points"][k, i][want["keep"][k]] for i in range(3)], -1) for k in range(nv)], 0)
    rgb = np.concatenate([np.stack([imgs[k, i][want["keep"][k]] for i in range(3)], -1) for k in range(nv)], 0)
    rec = np.empty(len(xyz), VERTEX)
    for i, k in enumerate(("x", "y", "z")):
        rec[k] = xyz[:, i]
    for i, k in enumerate(("red", "green", "blue")):
        rec[k] = rgb[:, i]
    sc = fusion.GipumaFusion.from_folder(str(tmp_path), str(tmp_path), prob_threshold=TH, device=dev)
    out = sc.fuse(with_intermediates=True)
    assert out["view_ids"] == list(range(nv)) and out["n_points"] == len(xyz) > 0
    assert np.array_equal(out["records"], np.frombuffer(rec.tobytes(), np.uint8))
    assert np.array_equal(out["xyz"].view(np.uint32), xyz.view(np.uint32)) and np.array_equal(out["rgb"], rgb)
    assert np.array_equal(out["used"].cpu().numpy(), want["used"]) and np.array_equal(out["count"].cpu().numpy(), want["count"])
    assert out["counts_per_view"] == {k: int(want["keep"][k].sum()) for k in range(nv)}
    for k in range(nv):
        assert out["stats"][k] == dict(photo=photo[k].sum() / float(h * w), geo=want["keep"][k].sum() / float(h * w),
                                       final=want["keep"][k].sum() / float(h * w))
    # an explicit pair list: processing order and sources as given
    jobs = [(3, [1, 0]), (0, [4, 2, 1, 3])]
    sc.set_pairs(jobs)
    want2 = gu.gipuma_rule(np.where(photo, d, np.float32(0)).astype(np.float32), fusion.gipuma_tables(cm), jobs, num_consistent=3)
    out2 = sc.fuse(want=("xyz",))
    xyz2 = np.concatenate([np.stack([want2["points"][k, i][want2["keep"][k]] for i in range(3)], -1) for k in range(2)], 0)
    assert list(out2["counts_per_view"]) == [3, 0] and np.array_equal(out2["xyz"].view(np.uint32), xyz2.view(np.uint32))
    # the scan function: the same bytes, twice
    ply = [str(tmp_path / ("%d.ply" % i)) for i in range(2)]
    res = [fusion.gipuma_fuse_scan(str(tmp_path), str(tmp_path), p, TH) for p in ply]
    raw = [open(p, "rb").read() for p in ply]
    assert raw[0] == raw[1] and res[0]["n_points"] == len(xyz) and res[0]["counts_per_view"] == out["counts_per_view"]
    gx, gc = data_io.read_ply(ply[0])
    assert np.array_equal(gx.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(gc, rgb)
    assert set(res[0]["seconds"]) == {"load", "device", "write"}
    with pytest.raises(MvsHipError):
        fusion.GipumaFusion(TH, device=dev).add_view(0, torch.ones(h, w), torch.ones(3, h, w), torch.from_numpy(cams[0]))
