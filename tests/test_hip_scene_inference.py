"""GPU tests of scene-resident depth inference: the view-indexed sweeps against the dense sweeps (bit for bit), the bad-table guard,
``ops.conf_stack``, and ``SceneInference`` (each image through the FPN and the ViT once, the cascade over a feature bank) against
``DINOMVSNet.forward`` per reference view - depth and confidences, with eviction, through to the fused point cloud and through files."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TMP = [5.0, 5.0, 5.0, 1.0]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _sweep_inputs(dev, N, tables, C, h, w, D, seed):
    """A random bank [N,h,w,C], plausible cameras for every sample of ``tables`` ([B][V]) and inverse-depth hypotheses [B,D,h,w]."""
    from mvsformer_amd import ops, synth
    B, V = len(tables), len(tables[0])
    g = torch.Generator().manual_seed(seed)
    bank = torch.randn(N, h, w, C, generator=g).to(dev)
    _, proj, dv, _ = synth.make_inputs(V, 8 * h, 8 * w, seed=seed)
    p = proj["stage1"]                                       # [1,V,2,4,4] at 1/8 of (8h, 8w)
    proj_b = torch.cat([p[:, [0] + [1 + (j + b) % (V - 1) for j in range(V - 1)]] for b in range(B)]).contiguous().to(dev)
    rt = ops.proj_prepare(proj_b)
    hyp = ops.init_inverse_range(dv.expand(B, -1).contiguous().to(dev), D, h, w)
    hyp = (hyp * (1.0 + 0.01 * torch.rand(hyp.shape, generator=g).to(dev))).contiguous()      # per-pixel hypotheses, as the fine stages have
    return bank, rt, hyp


TABLES = {"distinct": [[4, 0, 6, 2, 5]], "repeated": [[3, 1, 3, 6, 1]], "batch2": [[4, 0, 6, 2, 5], [1, 5, 0, 0, 3]]}


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("case", list(TABLES))
@pytest.mark.parametrize("C,h,w,D", [(8, 24, 40, 4), (16, 24, 37, 8), (32, 16, 24, 16), (64, 8, 19, 32), (64, 16, 24, 32)])
def test_indexed_sweeps_equal_dense_sweeps_bitwise(dev, C, h, w, D, case, fast, monkeypatch):
    """``ops.cv_*_views(bank, idx, ...)`` == the dense op on ``bank[idx]`` copied contiguous: same arithmetic, only the base differs."""
    from mvsformer_amd import ops
    if fast:
        monkeypatch.setenv("MVS_CV_FAST", "1")
    tables = TABLES[case]
    N, G = 7, 8
    bank, rt, hyp = _sweep_inputs(dev, N, tables, C, h, w, D, seed=3 + C + D)
    dense = bank[torch.tensor(tables, device=dev)].contiguous()          # [B,V,h,w,C]
    B, V = len(tables), len(tables[0])
    ent0 = ops.cv_entropy(dense, rt, hyp, G)
    ent1 = ops.cv_entropy_views(bank, tables, rt, hyp, G)
    assert torch.equal(ent0, ent1)
    assert torch.isfinite(ent0).all() and ent0.abs().max() > 0
    weight = torch.rand(B, V - 1, h, w, generator=torch.Generator().manual_seed(1)).to(dev)
    for want_sim in (True, False):
        vol0, sim0 = ops.cv_aggregate(dense, rt, hyp, weight, G, want_sim_depth=want_sim)
        vol1, sim1 = ops.cv_aggregate_views(bank, tables, rt, hyp, weight, G, want_sim_depth=want_sim)
        assert torch.equal(vol0, vol1)
        assert (sim0 is None and sim1 is None) or torch.equal(sim0, sim1)
    assert vol0.abs().max() > 0
    if C >= 32:                                              # the stored-correlation route: whole image and a band of rows
        e0, s0 = ops.cv_corr(dense, rt, hyp, G)
        e1, s1 = ops.cv_corr_rows_views(bank, tables, rt, hyp, G, 0, h)
        assert torch.equal(e0, e1) and torch.equal(s0, s1) and torch.equal(e0, ent0)
        v0, d0 = ops.cv_merge(s0, hyp, weight, V, C, G, want_sim_depth=True)
        v1, d1 = ops.cv_merge(s1, hyp, weight, V, C, G, want_sim_depth=True)
        assert torch.equal(v0, v1) and torch.equal(d0, d1)
        y0, rows = 2, h - 5
        eb0, sb0 = ops.cv_corr_rows(dense, rt, hyp, G, y0, rows)
        eb1, sb1 = ops.cv_corr_rows_views(bank, tables, rt, hyp, G, y0, rows)
        assert torch.equal(eb0, eb1) and torch.equal(sb0, sb1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("C,h,w,D", [(32, 16, 24, 16), (64, 8, 19, 32)])
def test_banded_stored_correlation_over_a_bank_equals_dense_bitwise(dev, C, h, w, D):
    """The band form with a table that repeats a view: ``cv_corr_rows_views`` == ``cv_corr_rows`` on the gathered views (entropy and store) for
    the whole image as a band, an inner band and the last three rows, and ``cv_merge_rows`` builds the same rows of the volume from either
    store and leaves the other rows alone.  At C = 32 also ``cv_corr`` == ``cv_corr_rows(0, H)``: one body, two entries."""
    from mvsformer_amd import ops
    tables = TABLES["repeated"]
    N, G, B, V = 7, 8, 1, 5
    bank, rt, hyp = _sweep_inputs(dev, N, tables, C, h, w, D, seed=11 + C)
    dense = bank[torch.tensor(tables, device=dev)].contiguous()
    weight = torch.rand(B, V - 1, h, w, generator=torch.Generator().manual_seed(2)).to(dev)
    for y0, rows in ((0, h), (2, h - 4), (h - 3, 3)):
        e0, s0 = ops.cv_corr_rows(dense, rt, hyp, G, y0, rows)
        e1, s1 = ops.cv_corr_rows_views(bank, tables, rt, hyp, G, y0, rows)
        assert e0.shape == (B, V - 1, rows, w)
        assert torch.equal(e0, e1) and torch.equal(s0, s1), (y0, rows)
        assert torch.isfinite(e0).all() and e0.abs().max() > 0
        wb = weight[:, :, y0:y0 + rows].contiguous()
        merged = []
        for store in (s0, s1):
            vol, sim = torch.full((B, G, D, h, w), -7.0, device=dev), torch.full((B, h, w), -7.0, device=dev)
            ops.cv_merge_rows(store, hyp, wb, V, C, G, y0, 0, rows, vol, sim)
            merged.append((vol, sim))
        (v0, d0), (v1, d1) = merged
        assert torch.equal(v0, v1) and torch.equal(d0, d1), (y0, rows)
        inside = torch.zeros(h, dtype=torch.bool, device=dev)
        inside[y0:y0 + rows] = True
        assert (v0[:, :, :, ~inside] == -7).all() and (d0[:, ~inside] == -7).all()
        assert (d0[:, inside] != -7).all() and v0[:, :, :, inside].abs().max() > 0
    if C == 32:
        ew, sw = ops.cv_corr(dense, rt, hyp, G)
        er, sr = ops.cv_corr_rows(dense, rt, hyp, G, 0, h)
        assert torch.equal(ew, er) and torch.equal(sw, sr)
    torch.cuda.synchronize()


def test_bad_view_table_is_an_error_before_any_launch(dev):
    """An index of N or -1 (or a table too large to travel by value) is refused by the entry's host check: an error, no kernel."""
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    N, G = 7, 8
    bank, rt, hyp = _sweep_inputs(dev, N, [[0, 1, 2]], 32, 16, 24, 8, seed=5)
    weight = torch.rand(1, 2, 16, 24).to(dev)
    for bad in ([[0, 1, N]], [[-1, 1, 2]], [[0, N + 100, 2]]):
        with pytest.raises(MvsHipError, match="outside the bank"):
            ops.cv_entropy_views(bank, bad, rt, hyp, G)
        with pytest.raises(MvsHipError, match="outside the bank"):
            ops.cv_aggregate_views(bank, bad, rt, hyp, weight, G, want_sim_depth=True)
        with pytest.raises(MvsHipError, match="outside the bank"):
            ops.cv_corr_rows_views(bank, bad, rt, hyp, G, 0, 16)
    with pytest.raises(MvsHipError):
        ops.cv_entropy_views(bank, [[0, 1.5, 2]], rt, hyp, G)
    big = [[0] * 13 for _ in range(5)]                       # B*V = 65 > 64 slots
    with pytest.raises(MvsHipError, match="by-value table"):
        ops.cv_entropy_views(bank, big, torch.zeros(5, 12, 12, device=dev), hyp.expand(5, -1, -1, -1).contiguous(), G)
    with pytest.raises(MvsHipError):                         # a device table is not a host table
        ops.cv_entropy_views(bank, torch.tensor([[0, 1, 2]], device=dev), rt, hyp, G)
    torch.cuda.synchronize()
    assert torch.equal(ops.cv_entropy_views(bank, [[0, 1, 2]], rt, hyp, G), ops.cv_entropy(bank[:3][None].contiguous(), rt, hyp, G))


@pytest.mark.parametrize("H,W", [(64, 64), (128, 192), (72, 104)])
def test_conf_stack_equals_nearest_interpolation(dev, H, W):
    from mvsformer_amd import ops
    g = torch.Generator().manual_seed(H + W)
    confs = [torch.rand(1, H >> (3 - k), W >> (3 - k), generator=g).to(dev) for k in range(4)]
    want = torch.stack([F.interpolate(c[None], size=(H, W), mode="nearest")[0, 0] for c in confs])
    scene_wide = torch.full((3, 4, H, W), -1.0, device=dev)
    got = ops.conf_stack(confs, scene_wide[1])               # a slice of a scene-wide tensor
    assert torch.equal(got, want) and torch.equal(scene_wide[1], want)
    assert (scene_wide[0] == -1).all() and (scene_wide[2] == -1).all()
    assert torch.equal(ops.conf_stack([c[0] for c in confs]), want)


# ------------------------------------------------------------------------------------------------------- the scene
def _mvsformer_p_args():
    return dict(fix=True, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
                depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
                vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                              att_fusion=True, nhead=6))


NV, H, W = 6, 256, 320
PAIRS = [(i, [(i + 1) % NV, (i + 2) % NV, (i + 4) % NV]) for i in range(NV)]
NUM_VIEWS = 3


@pytest.fixture(scope="module")
def scan(dev):
    """A synthetic scan (6 views, 3 per sample, 256 x 320), a random-weight model, and the PER-SAMPLE route's results."""
    import mvsformer_amd as m
    from mvsformer_amd import synth
    torch.manual_seed(1)
    net = m.DINOMVSNet(_mvsformer_p_args()).eval()
    m.cascade.randomize_bn_(net, seed=2)
    net = net.to(dev)
    sc = synth.make_scene(NV, H, W, seed=4)
    imgs = synth.render_features(sc, 1, 3, noise=0.02, device=dev, dtype=torch.float32)[0]       # [NV,3,H,W]
    cams = torch.zeros(NV, 2, 4, 4, dtype=torch.float64)
    cams[:, 0] = sc.E
    cams[:, 1, :3, :3] = sc.K
    cams[:, 1, 3, 3] = 1.0
    dr = synth.depth_range(1, device=dev)                    # [1,192]
    per_sample = {}
    for r, srcs in PAIRS:
        views = [r] + srcs[:NUM_VIEWS - 1]
        proj = {}
        for k, s in enumerate(synth.STAGE_SCALES):
            pm = cams[views].clone()
            pm[:, 1, :3, :3] = torch.stack([synth.stage_intrinsics(sc.K, s)] * len(views))
            proj["stage%d" % (k + 1)] = pm[None].to(device=dev, dtype=torch.float32)
        out = net(imgs[views][None], proj, dr, tmp=TMP)
        conf4 = torch.stack([F.interpolate(out["stage%d" % (k + 1)]["photometric_confidence"][None], size=(H, W), mode="nearest")[0, 0]
                             for k in range(4)])
        per_sample[r] = {"depth": out["refined_depth"][0].clone(), "confidence": conf4, "combined": out["photometric_confidence"][0].clone()}
    torch.cuda.synchronize()
    return dict(net=net, imgs=imgs, cams=cams.to(device=dev, dtype=torch.float32), dr=dr[0].contiguous(), per_sample=per_sample)


def _scene(scan, **kw):
    import mvsformer_amd as m
    si = m.SceneInference(scan["net"], **kw)
    for v in range(NV):
        si.add_image(v, scan["imgs"][v], scan["cams"][v], scan["dr"])
    si.set_pairs(PAIRS, num_views=NUM_VIEWS)
    return si


@pytest.fixture(scope="module")
def full_run(scan):
    si = _scene(scan)
    out = si.run(tmp=TMP)
    torch.cuda.synchronize()
    return si, out


def test_scene_route_matches_per_sample_route(scan, full_run):
    """max |depth - depth0| / |depth0| <= 1e-3 (the project's parity bar) and the same absolute bar on the confidences.  The figures are
    printed: DESIGN.md records the largest difference seen and whether the result was bitwise equal (which this test does not require)."""
    si, out = full_run
    assert list(out) == [r for r, _ in PAIRS]
    assert si.stats["extracted"] == NV and si.stats["capacity_views"] == NV          # every image through the 2-D networks once
    worst_d = worst_c = 0.0
    bitwise = True
    for r, want in scan["per_sample"].items():
        got = out[r]
        assert got["depth"].shape == (H, W) and got["confidence"].shape == (4, H, W)
        assert torch.equal(got["cam"], scan["cams"][r])
        worst_d = max(worst_d, ((got["depth"] - want["depth"]).abs() / want["depth"].abs()).max().item())
        worst_c = max(worst_c, (got["confidence"] - want["confidence"]).abs().max().item())
        bitwise = bitwise and torch.equal(got["depth"], want["depth"]) and torch.equal(got["confidence"], want["confidence"])
    print("scene vs per-sample route: max rel depth diff %.3e, max abs confidence diff %.3e, bitwise equal: %s" % (worst_d, worst_c, bitwise))
    assert worst_d <= 1e-3, worst_d
    assert worst_c <= 1e-3, worst_c


def test_scene_route_combined_confidence(scan):
    si = _scene(scan, combine_conf=True)
    out = si.run(tmp=TMP)
    for r, want in scan["per_sample"].items():
        assert out[r]["confidence"].shape == (H, W)
        assert (out[r]["confidence"] - want["combined"]).abs().max().item() <= 1e-3


def test_eviction_changes_nothing(scan, full_run):
    """capacity_views = 3 (= the views of one sample: images are extracted again and again) gives the full-bank run's tensors exactly."""
    _, full = full_run
    si = _scene(scan, capacity_views=3, extract_batch=2)
    out = si.run(tmp=TMP)
    assert si.stats["capacity_views"] == 3 and si.stats["extracted"] > NV
    for r in full:
        assert torch.equal(out[r]["depth"], full[r]["depth"]), r
        assert torch.equal(out[r]["confidence"], full[r]["confidence"]), r


def test_scene_through_to_the_cloud(scan, tmp_path):
    """``run(fusion=...)`` + ``fuse()`` gives the ``records`` bytes of adding the PER-SAMPLE route's outputs by hand; with ``save_to`` the
    written files, read back through ``SceneFusion.from_folder``, give the same cloud (same points; colours from the JPEG files the folder
    holds, which are lossy)."""
    import mvsformer_amd as m
    from mvsformer_amd import data_io
    # loose thresholds: a random-weight model's confidences are near 1/D and its depth maps agree between views only by chance
    kw = dict(method="pcd", prob_threshold=(0.01, 0.01, 0.01, 0.01), thres_disp=1000.0, thres_view=1)
    si = _scene(scan)
    fusion = m.SceneFusion(**kw)
    folder = str(tmp_path / "scan")
    out = si.run(tmp=TMP, fusion=fusion, save_to=folder)
    got = fusion.fuse(want=("records",))
    mean = torch.tensor([0.485, 0.456, 0.406], device=scan["imgs"].device).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=scan["imgs"].device).view(3, 1, 1)
    by_hand = m.SceneFusion(**kw)
    for r, _ in PAIRS:
        img8 = ((scan["imgs"][r] * std + mean) * 255.0).round().clamp(0, 255).to(torch.uint8)
        by_hand.add_view(r, scan["per_sample"][r]["depth"], scan["per_sample"][r]["confidence"], scan["cams"][r], img8)
    by_hand.set_pairs(PAIRS)
    want = by_hand.fuse(want=("records",))
    print("fused cloud: %d points, per view %s" % (want["n_points"], want["stats"]))
    assert want["n_points"] > 100                            # the comparison is not about an empty cloud
    assert got["n_points"] == want["n_points"] and got["records"].tobytes() == want["records"].tobytes()
    # through files: pair.txt next to the folder save_to filled
    with open(os.path.join(folder, "pair.txt"), "w") as f:
        f.write("%d\n" % len(PAIRS))
        for r, srcs in PAIRS:
            f.write("%d\n%d %s\n" % (r, len(srcs), " ".join("%d 1.0" % v for v in srcs)))
    from_files = m.SceneFusion.from_folder(folder, folder, **kw)
    back = from_files.fuse(want=("records", "xyz"))
    assert back["n_points"] == got["n_points"]
    assert np.array_equal(back["xyz"], fusion.fuse(want=("xyz",))["xyz"])
    jpeg = m.SceneFusion(**kw)                               # the same views with the colours the folder holds (JPEG is lossy)
    for r, _ in PAIRS:
        img = data_io.read_img(os.path.join(folder, "images/{:0>8}.jpg".format(r))).transpose(2, 0, 1)
        jpeg.add_view(r, out[r]["depth"], out[r]["confidence"], scan["cams"][r], torch.from_numpy(np.ascontiguousarray(img)).to(scan["imgs"].device))
    jpeg.set_pairs(PAIRS)
    assert back["records"].tobytes() == jpeg.fuse(want=("records",))["records"].tobytes()
