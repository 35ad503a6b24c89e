"""GPU tests of the depth metrics (csrc/metrics.hip behind ``mvsformer_amd.metrics``) against the fp64 restatement of
tests/depth_metrics_util.py and the fixture recorded from the real ``utils.py``: every edge of the kernel's decomposition, views at a
storage offset, every K, the mask forms, strictness, the band, NaN / Inf, capture in a graph, the validation epoch and the scene route.

Pass criteria: integer counts equal the restatement's exactly; ratios and per-image abs errors within 2 fp32 ulp of it (the kernel adds in
double and rounds once); batch means within (B + 2) * 2^-24 relative; two runs bitwise equal."""
import os

import numpy as np
import pytest
import torch

import depth_metrics_util as du
from conftest import load_golden

pytestmark = pytest.mark.gpu

P = 1024                                                     # MVS_DEPTH_METRICS_BLOCK_PIXELS (test_block_pixels_constant checks it)
SHAPES = [(1, 1), (1, 63), (1, 64), (1, 65), (3, 85), (4, 64), (1, 257), (5, 51), (1, P - 1), (1, P), (1, P + 1), (1, 2 * P + 3), (37, 113)]
KS = [0, 1, 4, 6, 8]
MASKS = ["all", "half_f32", "half_bool", "last", "none1"]
THR8 = np.array([0.37, 0.94, 1.89, 3.77, 7.55, 13.2, 18.9, 0.0], dtype=np.float32)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return load_golden("depth_metrics.npz")


def _view(arr, dev, offset):
    """``arr`` on the device as a contiguous view that starts ``offset`` elements into its storage (``.contiguous()`` does not realign it)."""
    t = torch.from_numpy(np.ascontiguousarray(arr))
    base = torch.empty(t.numel() + offset + 5, dtype=t.dtype, device=dev)
    v = base[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == offset
    return v


def _run(dev, est, gt, mask, thr=None, band=None, offset=0, mask_f32=False):
    from mvsformer_amd import metrics
    m = mask.astype(np.float32) if mask_f32 else mask
    args = (_view(est, dev, offset), _view(gt, dev, offset), _view(m, dev, offset))
    t = None if thr is None else torch.from_numpy(np.ascontiguousarray(thr)).to(dev)
    out = metrics.depth_metrics(*args, t, band=band)
    again = metrics.depth_metrics(*args, t, band=band)
    for k in ("valid_count", "band_count", "exceed_count"):
        assert torch.equal(out[k], again[k]), k
    for k in ("per_image", "batch"):                           # bitwise: NaN payloads included
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), k
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _check(got, ref, B, what):
    assert np.array_equal(got["valid_count"], ref["n"]), what
    assert np.array_equal(got["band_count"], ref["n_band"]), what
    assert np.array_equal(got["exceed_count"], ref["above"]), what
    assert got["per_image"].dtype == np.float32 and got["batch"].dtype == np.float32
    assert np.array_equal(np.isnan(got["per_image"]), np.isnan(ref["per_image"])), what
    assert np.array_equal(np.isnan(got["batch"]), np.isnan(ref["batch"])), what
    u = du.ulps32(got["per_image"], ref["per_image"]).max()
    assert u <= 2.0, (what, u)
    ok = ~np.isnan(ref["batch"])
    err = np.abs(got["batch"][ok].astype(np.float64) - ref["batch"][ok])
    assert (err <= (B + 2) * 2.0 ** -24 * np.abs(ref["batch"][ok])).all(), (what, err)
    assert got[du.ABS_KEY] == got["batch"][0] or (np.isnan(got[du.ABS_KEY]) and np.isnan(got["batch"][0]))


def test_block_pixels_constant():
    from mvsformer_amd import _lib, ops
    assert _lib.load().mvs_depth_metrics_block_pixels() == P == ops.DEPTH_METRICS_BLOCK_PIXELS


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_views_masks_and_k(dev, H, W, B, offset):
    """Every edge shape, aligned and as views one and three elements into their storage, with every mask form; K walks 0, 1, 4, 6, 8 against
    the mask forms so that over the shapes every K meets every mask."""
    si = SHAPES.index((H, W))
    for mi, kind in enumerate(MASKS):
        K = KS[(mi + si) % len(KS)]
        est, gt, mask = du.make_case(B, H, W, seed=100 * si + 10 * B + mi, mask=kind.split("_")[0])
        thr = np.stack([np.roll(THR8, b)[:K] for b in range(B)]).astype(np.float32)              # per-image thresholds
        got = _run(dev, est, gt, mask, thr if K else None, offset=offset, mask_f32=kind == "half_f32")
        _check(got, du.np_metrics(est, gt, mask, thr), B, (H, W, B, offset, kind, K))
        if kind == "last":
            assert (got["valid_count"] == 1).all()


def test_more_than_eight_thresholds_are_refused(dev):
    from mvsformer_amd import metrics
    from mvsformer_amd._lib import MvsHipError
    x = torch.zeros(1, 4, 4, device=dev)
    with pytest.raises(MvsHipError, match="K=9"):
        metrics.depth_metrics(x, x, x > -1, torch.ones(1, 9, device=dev))
    assert metrics.depth_metrics(x, x, x > -1, torch.ones(8, device=dev))["exceed_count"].shape == (1, 8)      # [K] is broadcast over the batch


@pytest.mark.parametrize("H,W", [(5, 51), (1, 2 * P + 3)])
def test_threshold_is_strict_in_fp32(dev, H, W):
    """Integer-valued gt, est = gt + 2.0 on the first half of the map: at threshold 2.0 none of those pixels counts, at nextafter(2.0, 0)
    in fp32 all of them do."""
    est, gt, mask = du.make_case(3, H, W, seed=9, mask="all", integer=True, offset=2.0)
    half = (H * W + 1) // 2
    assert (np.abs(est - gt).reshape(3, -1)[:, :half] == 2.0).all()
    thr = np.array([[2.0, np.nextafter(np.float32(2.0), np.float32(0.0))]] * 3, dtype=np.float32)
    got = _run(dev, est, gt, mask, thr)
    _check(got, du.np_metrics(est, gt, mask, thr), 3, "strict")
    assert (got["exceed_count"][:, 0] == 0).all() and (got["exceed_count"][:, 1] == half).all()


def test_band_is_inclusive_and_empty_selections_give_zero(dev):
    est, gt, mask = du.make_case(3, 5, 51, seed=11, mask="half", integer=True, offset=0.0)
    e = est.reshape(3, -1)
    e[:, 0::4] += np.float32(1.0)                             # errors of exactly lo
    e[:, 1::4] += np.float32(3.0)                             # exactly hi
    e[:, 2::4] += np.float32(2.0)                             # inside; the rest 0: outside
    band = (1.0, 3.0)
    got = _run(dev, est, gt, mask, band=band, offset=1)
    ref = du.np_metrics(est, gt, mask, band=band)
    _check(got, ref, 3, "band")
    v = mask.reshape(3, -1)
    want = np.array([np.count_nonzero(v[b] & (np.abs(est - gt).reshape(3, -1)[b] >= 1.0)) for b in range(3)])
    assert np.array_equal(got["band_count"], want) and (want > 0).all()
    empty = _run(dev, est, gt, mask, band=(10.0, 20.0))
    assert (empty["band_count"] == 0).all() and (empty["per_image"][:, 0] == 0).all() and empty["batch"][0] == 0
    mask[1] = False                                           # band together with an empty mask: 0, not NaN
    got = _run(dev, est, gt, mask, band=band)
    _check(got, du.np_metrics(est, gt, mask, band=band), 3, "band + empty mask")
    assert got["per_image"][1, 0] == 0 and got["valid_count"][1] == 0 and np.isfinite(got["batch"][0])
    none = _run(dev, est, gt, mask)                           # without the band the same image is NaN, and so is the batch
    assert np.isnan(none["per_image"][1, 0]) and np.isnan(none["batch"][0]) and np.isfinite(none["per_image"][[0, 2], 0]).all()


@pytest.mark.parametrize("offset", [0, 3])
def test_nan_and_inf(dev, offset):
    """NaN / Inf in est and gt at invalid pixels change nothing (bitwise); a NaN at one valid pixel makes that image's abs error NaN, only
    that image's, and leaves its exceed counts as they are without the pixel."""
    B, H, W = 3, 7, 2 * P // 7 + 5
    clean = du.make_case(B, H, W, seed=21, mask="half")
    dirty = du.make_case(B, H, W, seed=21, mask="half", poison=True)
    assert np.array_equal(clean[2], dirty[2]) and np.isnan(dirty[0]).any() and np.isinf(dirty[1]).any()
    thr = np.broadcast_to(THR8, (B, 8)).copy()
    a, b = _run(dev, *clean, thr, offset=offset), _run(dev, *dirty, thr, offset=offset, mask_f32=True)
    for k in ("valid_count", "exceed_count", "per_image", "batch"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.isfinite(a["per_image"]).all()
    flat = int(np.flatnonzero(~clean[2].reshape(B, -1)[1])[5])        # an invalid pixel of image 1, made valid with a NaN in est
    est, gt, mask = du.make_case(B, H, W, seed=21, mask="half", nan_valid=(1, flat))
    got = _run(dev, est, gt, mask, thr, offset=offset)
    _check(got, du.np_metrics(est, gt, mask, thr), B, "nan at a valid pixel")
    assert np.isnan(got["per_image"][1, 0]) and np.isfinite(got["per_image"][[0, 2]]).all() and np.isnan(got["batch"][0])
    assert np.array_equal(got["exceed_count"], a["exceed_count"]) and got["valid_count"][1] == a["valid_count"][1] + 1
    assert np.isfinite(got["per_image"][1, 1:]).all()


@pytest.mark.parametrize("name", list(du.FIXTURE_CASES))
def test_fixture_cases_and_the_reference_interface(dev, golden, name):
    """The recorded cases: NaN exactly where the real ``utils.py`` has NaN, values within the reference's own fp32 error of it, and
    ``Thres_metrics`` / ``AbsDepthError_metrics`` return what ``depth_metrics`` returns for the same arguments (0-dim fp32)."""
    import mvsformer_amd as m
    est, gt, mask = golden[name + ".est"], golden[name + ".gt"], golden[name + ".mask"].astype(bool)
    B = est.shape[0]
    thr = np.array(du.FIXTURE_THRES, dtype=np.float32)
    got = _run(dev, est, gt, mask, np.broadcast_to(thr, (B, thr.size)).copy())
    ref = du.np_metrics(est, gt, mask, thr)
    _check(got, ref, B, name)
    assert np.array_equal(np.isnan(got["batch"][1:]), np.isnan(golden[name + ".thres"]))
    assert np.array_equal(np.isnan(got["per_image"][:, 1:]), np.isnan(golden[name + ".thres_img"]))
    assert np.isnan(got["batch"][0]) == np.isnan(golden[name + ".abs"][0])
    assert du.ulps32(got["per_image"][:, 1:], golden[name + ".thres_img"].astype(np.float64)).max() <= 1.0
    e, g, k = (torch.from_numpy(a).to(dev) for a in (est, gt, mask))
    for mk in (k, k.to(torch.float32)):
        for i, t in enumerate(du.FIXTURE_THRES):
            v = m.Thres_metrics(e, g, mk, t)
            assert v.dim() == 0 and v.dtype == torch.float32 and v.device.type == "cuda"
            assert np.array_equal(v.cpu().numpy(), got["batch"][1 + i], equal_nan=True), (name, t)
    for i, band in enumerate(du.FIXTURE_BANDS):
        v = m.AbsDepthError_metrics(e, g, k) if band is None else m.AbsDepthError_metrics(e, g, k, band)
        w = m.depth_metrics(e, g, k, band=band)[du.ABS_KEY]
        assert v.dim() == 0 and v.dtype == torch.float32 and np.array_equal(v.cpu().numpy(), w.cpu().numpy(), equal_nan=True)
        want, n = golden[name + ".abs"][i], int(ref["n"].max()) + B + 2
        assert np.isnan(want) == bool(torch.isnan(v))
        if not np.isnan(want):
            assert abs(v.item() - float(want)) <= n * 2.0 ** -24 * abs(float(want)), (name, band)
    # lower-precision inputs are converted to fp32 first
    h = m.AbsDepthError_metrics(e.half(), g.half(), k)
    w = m.AbsDepthError_metrics(e.half().float(), g.half().float(), k)
    assert np.array_equal(h.cpu().numpy(), w.cpu().numpy(), equal_nan=True)


def test_device_built_thresholds_and_names(dev):
    from mvsformer_amd import metrics
    est, gt, mask = du.make_case(3, 5, 51, seed=31, mask="half")
    itv = np.array([du.DTU_INTERVAL, 3.3, 0.7], dtype=np.float32)
    e, g, k, it = (torch.from_numpy(a).to(dev) for a in (est, gt, mask, itv))
    for per_sample in (False, True):
        out = metrics.depth_metrics(e, g, k, depth_interval=it, multipliers=du.TEST_MULT, per_sample_interval=per_sample)
        want = du.thresholds_host(itv, du.TEST_MULT, per_sample)
        want = want if per_sample else want[:1].repeat(3, 0)
        assert np.array_equal(out["thresholds"].cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert list(out)[:7] == [du.ABS_KEY] + ["thres%dmm_error" % x for x in du.TEST_MULT]
        ref = du.np_metrics(est, gt, mask, want)
        assert np.array_equal(out["exceed_count"].cpu().numpy(), ref["above"])


def test_offsets_past_2_31(dev):
    """B * HW > 2^31 elements (byte offsets past 2^33): image 1 is read where it lies.  Constant maps with three marked pixels, so the
    expected counts are known without a host pass over 2^31 pixels."""
    from mvsformer_amd import metrics
    HW = 2 ** 30 + 5
    gt = torch.full((2, 1, HW), 2.0, device=dev)
    est = torch.full((2, 1, HW), 3.0, device=dev)
    mask = torch.ones((2, 1, HW), dtype=torch.bool, device=dev)
    est[1, 0, HW - 1] = 7.0                                   # the very last pixel: error 5
    est[1, 0, 0] = 7.0
    mask[1, 0, 1] = False
    mask[0, 0, HW - 2] = False
    out = metrics.depth_metrics(est, gt, mask, torch.tensor([0.5, 1.0, 4.0], device=dev))
    assert out["valid_count"].tolist() == [HW - 1, HW - 1]
    assert out["exceed_count"].tolist() == [[HW - 1, 0, 0], [HW - 1, 2, 2]]
    want1 = (HW - 3 + 10.0) / (HW - 1)
    assert out["per_image"][0, 0].item() == 1.0 and out["per_image"][1, 0].item() == float(np.float32(want1))
    del est, gt, mask


def test_capture_in_one_graph(dev):
    """``depth_metrics`` with the meter update, thresholds built from the interval on the device, captured in one ``torch.cuda.graph`` on
    one stream (a linear chain), replayed three times with the inputs overwritten in place: the meter equals three eager updates exactly."""
    from mvsformer_amd import metrics
    B, H, W = 2, 37, 113
    names = [du.ABS_KEY] + metrics.threshold_names(du.VALID_MULT)
    cases = [du.make_case(B, H, W, seed=40 + i, mask="half") for i in range(3)]
    itvs = [np.array([du.DTU_INTERVAL * (1 + i), 1.0], dtype=np.float32) for i in range(3)]
    est, gt, mask, itv = (torch.empty(B, H, W, device=dev), torch.empty(B, H, W, device=dev), torch.empty(B, H, W, device=dev),
                          torch.empty(B, device=dev))

    def load(i):
        est.copy_(torch.from_numpy(cases[i][0])), gt.copy_(torch.from_numpy(cases[i][1]))
        mask.copy_(torch.from_numpy(cases[i][2].astype(np.float32))), itv.copy_(torch.from_numpy(itvs[i]))

    def step(meter):
        return metrics.depth_metrics(est, gt, mask, depth_interval=itv, multipliers=du.VALID_MULT, meter=meter)

    eager = metrics.DeviceAverageMeter(names, dev)
    per_step = []
    for i in range(3):
        load(i)
        per_step.append(step(eager)["batch"].clone())
    captured, warm = metrics.DeviceAverageMeter(names, dev), metrics.DeviceAverageMeter(names, dev)
    load(0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(warm)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(captured)
    assert captured.count.item() == 0                         # capturing runs nothing
    for i in range(3):
        load(i)
        graph.replay()
        assert torch.equal(out["batch"].view(torch.int32), per_step[i].view(torch.int32))
    torch.cuda.synchronize()
    assert torch.equal(captured.sums, eager.sums) and torch.equal(captured.count, eager.count) and eager.count.item() == 3.0
    ref = du.MeterRef()
    for b in per_step:
        ref.update({k: float(v) for k, v in zip(names, b.cpu().tolist())})
    assert captured.mean() == ref.mean()


# ------------------------------------------------------------------------------------------------------- model-level
def _mvsformer_p_args():
    return dict(fix=True, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
                depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
                vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                              att_fusion=True, nhead=6))


@pytest.fixture(scope="module")
def net(dev):
    import mvsformer_amd as m
    torch.manual_seed(1)
    model = m.DINOMVSNet(_mvsformer_p_args()).eval()
    m.cascade.randomize_bn_(model, seed=2)
    return model.to(dev)


class _Recorder(torch.nn.Module):
    """The model under ``valid_epoch`` with its ``refined_depth`` of every batch kept, so that the comparison loop sees the same maps."""

    def __init__(self, model):
        super().__init__()
        self.model, self.seen, self.modes = model, [], []

    def forward(self, imgs, proj, depth_values):
        self.modes.append(self.training)
        out = self.model(imgs, proj, depth_values)
        self.seen.append(out["refined_depth"].detach().clone())
        return out


@pytest.mark.parametrize("blended", [False, True], ids=["dtu", "blended"])
def test_valid_epoch(dev, net, blended):
    """Two synthetic batches (B = 2, 3 views, 64 x 64): ``valid_epoch`` equals the same loop written with per-batch calls, ``.item()`` and
    Python-float averaging (``mean_error`` included), returns 0-dim fp32 device tensors and leaves a training model in training mode."""
    from mvsformer_amd import metrics, synth
    B, V, H, W = 2, 3, 64, 64
    loader = []
    for s in range(2):
        sc = synth.make_scene(V, H, W, seed=5 + s)
        imgs = synth.render_features(sc, 1, 3, noise=0.02, batch=B, device=dev, dtype=torch.float32)
        imgs[1] = imgs[1].flip(-1) * 0.9                      # two different samples
        dv = synth.depth_range(B, device=dev)
        dv[1] = dv[1] * 1.03                                  # ... with different intervals
        g = torch.Generator().manual_seed(s)
        gt = (synth.plane_depth(sc, 1)[None].repeat(B, 1, 1) + 4.0 * torch.randn(B, H, W, generator=g)).to(dev)
        mask = (torch.rand(B, H, W, generator=g) < 0.6).to(torch.float32).to(dev)
        loader.append({"imgs": imgs, "proj_matrices": synth.proj_matrices(sc, batch=B, device=dev), "depth_values": dv,
                       "depth": {"stage4": gt}, "mask": {"stage4": mask}})
    rec = _Recorder(net).train()
    net.eval()
    got = metrics.valid_epoch(rec, loader, blended=blended)
    assert rec.training and rec.modes == [False, False] and len(rec.seen) == 2
    rec.eval()
    names = [du.ABS_KEY] + metrics.threshold_names(metrics.VALID_MULTIPLIERS)
    assert list(got) == names + ["mean_error"]
    ref = du.MeterRef()
    for sample, depth in zip(loader, rec.seen):
        dv = sample["depth_values"]
        o = metrics.depth_metrics(depth, sample["depth"]["stage4"], sample["mask"]["stage4"], depth_interval=dv[:, 1] - dv[:, 0],
                                  multipliers=metrics.VALID_MULTIPLIERS, per_sample_interval=blended)
        ref.update({k: o[k].item() for k in names})
        want_thr = du.thresholds_host((dv[:, 1] - dv[:, 0]).cpu().numpy(), metrics.VALID_MULTIPLIERS, blended)
        assert np.array_equal(o["thresholds"].cpu().numpy(), want_thr if blended else want_thr[:1].repeat(B, 0))
        assert (o["valid_count"] > 1000).all()
    mean = ref.mean()
    mean["mean_error"] = (mean["thres2mm_error"] + mean["thres4mm_error"] + mean["thres8mm_error"] + mean["thres14mm_error"]) / 4.0
    for k, v in got.items():
        assert v.dim() == 0 and v.dtype == torch.float32 and v.device.type == "cuda"
        assert v.item() == float(np.float32(mean[k])), (k, v.item(), mean[k])
    assert 0.0 < got["thres2mm_error"].item() <= 1.0


NV, SH, SW, NUM_VIEWS = 6, 256, 320, 3
PAIRS = [(i, [(i + 1) % NV, (i + 2) % NV, (i + 4) % NV]) for i in range(NV)]
TMP = [5.0, 5.0, 5.0, 1.0]


def test_scene_route_writes_depth_metric_txt(dev, net, tmp_path):
    """A scan of tests/test_hip_scene_inference.py's kind with synthetic ground truth: ``SceneInference.run(gt=...)`` fills a meter with
    test.py's seven entries; written as ``depth_metric.txt`` it equals per-view ``depth_metrics`` on ``DINOMVSNet.forward``'s
    ``refined_depth`` averaged by a host ``DictAverageMeter`` restatement (the two routes' depth maps are bitwise equal)."""
    import mvsformer_amd as m
    from mvsformer_amd import metrics, synth
    sc = synth.make_scene(NV, SH, SW, seed=4)
    imgs = synth.render_features(sc, 1, 3, noise=0.02, device=dev, dtype=torch.float32)[0]
    cams = torch.zeros(NV, 2, 4, 4, dtype=torch.float64)
    cams[:, 0] = sc.E
    cams[:, 1, :3, :3] = sc.K
    cams[:, 1, 3, 3] = 1.0
    dr = synth.depth_range(1, device=dev)
    names = [du.ABS_KEY] + metrics.threshold_names(metrics.TEST_MULTIPLIERS)
    ref, gts = du.MeterRef(), {}
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for r, srcs in PAIRS:
            views = [r] + srcs[:NUM_VIEWS - 1]
            proj = {}
            for k, s in enumerate(synth.STAGE_SCALES):
                pm = cams[views].clone()
                pm[:, 1, :3, :3] = torch.stack([synth.stage_intrinsics(sc.K, s)] * len(views))
                proj["stage%d" % (k + 1)] = pm[None].to(device=dev, dtype=torch.float32)
            depth = net(imgs[views][None], proj, dr, tmp=TMP)["refined_depth"]
            gt = depth[0] + (6.0 * torch.randn(SH, SW, generator=g) * torch.rand(SH, SW, generator=g)).to(dev)
            gts[r] = (gt, (torch.rand(SH, SW, generator=g) < 0.7).to(dev))
            o = metrics.depth_metrics(depth, gt[None], gts[r][1][None], depth_interval=dr[:, 1] - dr[:, 0], multipliers=metrics.TEST_MULTIPLIERS)
            ref.update({k: o[k].item() for k in names})
    si = m.SceneInference(net)
    cams32 = cams.to(device=dev, dtype=torch.float32)
    for v in range(NV):
        si.add_image(v, imgs[v], cams32[v], dr[0].contiguous())
    si.set_pairs(PAIRS, num_views=NUM_VIEWS)
    si.run(tmp=TMP, gt=gts)
    assert si.depth_meter.keys == names and si.depth_meter.count.item() == NV
    path = str(tmp_path / "depth_metric.txt")
    metrics.write_depth_metric_txt(path, si.depth_meter.mean())
    want = "".join(k + " " + str(v) + "\n" for k, v in ref.mean().items())
    assert open(path).read() == want
    assert len(want.splitlines()) == 7 and 0.0 < ref.mean()["thres1mm_error"] < 1.0
    from mvsformer_amd._lib import MvsHipError
    with pytest.raises(MvsHipError, match="ground truth"):
        si.run(tmp=TMP, gt={r: (d[:-1], k[:-1]) for r, (d, k) in gts.items()})
