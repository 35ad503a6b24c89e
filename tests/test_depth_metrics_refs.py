"""CPU checks of the depth metrics: the numpy restatement of tests/depth_metrics_util.py against the fixture recorded from the real
``utils.py`` (tests/golden/depth_metrics.npz), ``DeviceAverageMeter`` on CPU tensors against the recorded ``DictAverageMeter`` trace, the
device-built thresholds against the host's double arithmetic, and the C ABI of the new entries."""
import os
import re

import numpy as np
import pytest
import torch

import depth_metrics_util as du
from conftest import REPO, load_golden

HEADER = os.path.join(REPO, "include", "mvs_hip.h")


@pytest.fixture(scope="module")
def golden():
    return load_golden("depth_metrics.npz")


@pytest.mark.parametrize("name", list(du.FIXTURE_CASES))
def test_restatement_reproduces_the_reference(golden, name):
    """Ratios to 1 fp32 ulp; abs error to n * 2^-24 relative (the worst case of ANY fp32 summation order over n non-negative terms - the
    reference's order is torch's own); NaN exactly where the reference has NaN.  The inputs the builder makes are the recorded ones."""
    est, gt, mask = du.make_case(**du.FIXTURE_CASES[name])
    assert np.array_equal(est, golden[name + ".est"], equal_nan=True) and np.array_equal(gt, golden[name + ".gt"], equal_nan=True)
    assert np.array_equal(mask, golden[name + ".mask"].astype(bool))
    B = est.shape[0]
    thr = np.array(du.FIXTURE_THRES, dtype=np.float32)            # the Python scalar rounded to fp32, as `errors > thres` rounds it
    for i, band in enumerate(du.FIXTURE_BANDS):
        r = du.np_metrics(est, gt, mask, thr, band)
        # per image n roundings (n - 1 additions and the division); the batch value adds torch's fp32 mean of B values: B + 2 more
        for got, want, n in [(r["batch"][0], golden[name + ".abs"][i], r["n_band"].max() + B + 2)] + \
                            [(r["per_image"][b, 0], golden[name + ".abs_img"][b, i], r["n_band"][b]) for b in range(B)]:
            assert np.isnan(got) == np.isnan(want), (name, band)
            if not np.isnan(want):
                assert abs(got - float(want)) <= n * 2.0 ** -24 * abs(float(want)), (name, band, got, want)
    r = du.np_metrics(est, gt, mask, thr)
    assert np.array_equal(np.isnan(r["batch"][1:]), np.isnan(golden[name + ".thres"]))
    assert np.array_equal(np.isnan(r["per_image"][:, 1:]), np.isnan(golden[name + ".thres_img"]))
    assert du.ulps32(golden[name + ".thres_img"], r["per_image"][:, 1:]).max() <= 1.0
    # the batch value is torch's fp32 mean of B fp32 values: B + 2 roundings at most
    ok = ~np.isnan(golden[name + ".thres"])
    assert (np.abs(golden[name + ".thres"][ok] - r["batch"][1:][ok]) <= (B + 2) * 2.0 ** -24 * np.abs(r["batch"][1:][ok])).all()


def test_strict_comparison_is_in_fp32():
    """``float32(0.1) > 0.1`` is False in the reference (the scalar is rounded to fp32): an error of exactly float32(0.1) is not counted."""
    gt = np.zeros((1, 1, 4), np.float32)
    est = np.array([[[0.1, 0.1, 0.2, 0.0]]], dtype=np.float32)
    r = du.np_metrics(est, gt, np.ones((1, 1, 4), bool), np.array([0.1], np.float32))
    assert r["above"][0, 0] == 1


def test_device_meter_equals_the_recorded_trace(golden):
    """The same fp32 values added in double in the same order: sums, count and means equal the reference's exactly."""
    from mvsformer_amd.metrics import DeviceAverageMeter
    keys = [str(k) for k in golden["meter_keys"]]
    meter = DeviceAverageMeter(keys, "cpu")
    lazy = DeviceAverageMeter()                                     # the reference's constructor: keys and device from the first update
    ref = du.MeterRef()
    for t, row in enumerate(golden["meter_in"]):
        vals = {k: torch.tensor(v, dtype=torch.float32) for k, v in zip(keys, row)}
        assert all(float(vals[k]) == v for k, v in zip(keys, row))  # the recorded values ARE fp32 values
        meter.update(vals)
        lazy.update({k: float(v) for k, v in vals.items()})
        ref.update({k: float(v) for k, v in zip(keys, row)})
        assert np.array_equal(meter.sums.numpy(), golden["meter_data"][t]) and meter.count.item() == golden["meter_count"][t]
        assert [ref.data[k] for k in keys] == list(golden["meter_data"][t])
    mean = meter.mean()
    assert list(mean) == keys and [mean[k] for k in keys] == list(golden["meter_mean"])
    assert lazy.mean() == mean and lazy.keys == keys
    mt = meter.mean_tensors()
    assert all(v.dim() == 0 and v.dtype == torch.float32 for v in mt.values())
    assert [mt[k].item() for k in keys] == [float(np.float32(v)) for v in golden["meter_mean"]]
    meter.reset()
    assert meter.sums.abs().sum().item() == 0 and meter.count.item() == 0
    meter.update({k: torch.tensor(1.5) for k in keys}, n=2.0)
    assert meter.mean() == {k: 0.75 for k in keys}
    with pytest.raises(NotImplementedError):
        meter.update({k: "x" for k in keys})


@pytest.mark.parametrize("per_sample", [False, True])
def test_device_built_thresholds_equal_the_host_arithmetic(per_sample):
    """``build_thresholds`` (fp64 torch ops on the fp32 interval, here on CPU tensors) against ``float32(mult * (float(itv) / 2.65))`` /
    ``float32(mult * float(itv))`` bit for bit, with intervals that are not exact in fp32 (2.5 x 1.06 among them)."""
    from mvsformer_amd.metrics import build_thresholds, threshold_names
    rng = np.random.RandomState(0)
    itvs = np.concatenate([[np.float32(2.5) * np.float32(1.06), np.float32(2.65), np.float32(0.1), np.float32(1.0 / 3.0)],
                           (0.01 + 10.0 * rng.rand(60)).astype(np.float32)]).astype(np.float32)
    for mults in (du.VALID_MULT, du.TEST_MULT):
        if per_sample:
            got = build_thresholds(torch.from_numpy(itvs), mults, True)
            assert np.array_equal(got.numpy().view(np.uint32), du.thresholds_host(itvs, mults, True).view(np.uint32))
        else:
            for itv in itvs:
                batch = np.array([itv, 7.0, 9.0], np.float32)         # only interval[0] counts in the DTU form
                got = build_thresholds(torch.from_numpy(batch), mults, False)
                assert got.shape == (3, len(mults)) and got.dtype == torch.float32 and got.is_contiguous()
                assert np.array_equal(got.numpy().view(np.uint32), du.thresholds_host(batch, mults, False)[:1].repeat(3, 0).view(np.uint32))
    assert threshold_names((1, 2, 4, 8, 14, 20))[:2] == ["thres1mm_error", "thres2mm_error"]


def test_metrics_have_no_cpu_path():
    import mvsformer_amd as m
    from mvsformer_amd._lib import MvsHipError
    x = torch.zeros(1, 4, 4)
    for call in (lambda: m.Thres_metrics(x, x, x > 0, 1.0), lambda: m.AbsDepthError_metrics(x, x, x > 0),
                 lambda: m.depth_metrics(x, x, x > 0, torch.ones(1, 1))):
        with pytest.raises(MvsHipError):
            call()
    with pytest.raises(AssertionError):                             # utils.py:165, kept
        m.Thres_metrics(x, x, x > 0, torch.tensor(1.0))


def test_abi_of_the_new_entries():
    """The header, the ctypes table and the built library agree on the three entries; the sizing function counts one 48-byte row per block
    of MVS_DEPTH_METRICS_BLOCK_PIXELS pixels at the worst alignment; bad arguments are refused with MVS_EINVAL before any launch."""
    from mvsformer_amd import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    protos = {m.group(1): len(m.group(2).split(",")) if m.group(2).strip() not in ("", "void") else 0
              for m in re.finditer(r"(mvs_depth_metrics\w*)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}
    assert set(protos) == {"mvs_depth_metrics", "mvs_depth_metrics_acc_floats", "mvs_depth_metrics_block_pixels"}
    for n, nargs in protos.items():
        assert len(_lib.SIGNATURES[n][1]) == nargs, n
    P = int(re.search(r"#define\s+MVS_DEPTH_METRICS_BLOCK_PIXELS\s+(\d+)", src).group(1))
    assert int(re.search(r"#define\s+MVS_DEPTH_METRICS_MAX_K\s+(\d+)", src).group(1)) == ops.DEPTH_METRICS_MAX_K == 8
    lib = _lib.load()
    assert lib.mvs_depth_metrics_block_pixels() == P == ops.DEPTH_METRICS_BLOCK_PIXELS
    for B, HW in ((1, 1), (3, P - 3), (3, P - 2), (2, 2 * P + 3), (4, 1536 * 1152)):
        assert lib.mvs_depth_metrics_acc_floats(B, HW) == 12 * B * ((HW + 3 + P - 1) // P)
    assert lib.mvs_depth_metrics_acc_floats(0, 5) < 0 and lib.mvs_depth_metrics_acc_floats(1, 0) < 0 and lib.mvs_depth_metrics_acc_floats(1, 2 ** 31) < 0
    assert lib.mvs_depth_metrics_acc_floats(1, 2 ** 31 - 1) > 0
    fake = 0x1000                                                   # never dereferenced: every call below is refused on the host
    EINVAL = -22

    def call(B=1, K=1, HW=16, est=fake, acc=fake, thr=fake):
        return lib.mvs_depth_metrics(est, fake, fake, 0, thr, B, K, HW, 0, 0.0, 0.0, acc, fake, fake, fake, None, None, 1.0, None)
    assert call(K=9) == EINVAL and b"mvs_depth_metrics" in lib.mvs_last_error()
    assert call(K=-1) == EINVAL and call(B=0) == EINVAL and call(HW=0) == EINVAL and call(HW=2 ** 31) == EINVAL
    assert call(est=None) == EINVAL and call(thr=None) == EINVAL and call(est=fake + 2) == EINVAL and call(acc=fake + 4) == EINVAL


def test_install_rebinds_the_metrics_only_on_request(monkeypatch):
    import sys
    import types
    from mvsformer_amd import metrics
    from mvsformer_amd.install import install
    utils = types.ModuleType("utils")
    names = ("Thres_metrics", "AbsDepthError_metrics", "DictAverageMeter", "tensor2float")
    before = {n: object() for n in names}
    for n, o in before.items():
        setattr(utils, n, o)
    monkeypatch.setitem(sys.modules, "utils", utils)
    done = install()
    assert "utils" not in done and all(getattr(utils, n) is before[n] for n in names)
    done = install(metrics=True)
    assert sorted(done["utils"]) == sorted(names[:3])
    assert utils.Thres_metrics is metrics.Thres_metrics and utils.AbsDepthError_metrics is metrics.AbsDepthError_metrics
    assert utils.DictAverageMeter is metrics.DeviceAverageMeter and utils.tensor2float is before["tensor2float"]
    utils.DictAverageMeter().reset()                               # the reference's constructor call and its reset() before the first update


def test_infer_scan_ground_truth_files_and_metric_txt(tmp_path):
    """``tools/infer_scan.py``'s ground-truth reader (PFM depth, PNG mask valid above 10; ``%08d`` names or DTU's) and the line format of
    ``depth_metric.txt`` (test.py:325-327: ``key + ' ' + str(value)``)."""
    import importlib.util
    from PIL import Image
    from mvsformer_amd import data_io, metrics
    spec = importlib.util.spec_from_file_location("infer_scan_tool", os.path.join(REPO, "tools", "infer_scan.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.RandomState(0)
    depth = (500.0 + rng.rand(6, 8)).astype(np.float32)
    mask = (rng.rand(6, 8) * 255).astype(np.uint8)
    d, k = tmp_path / "d", tmp_path / "m"
    d.mkdir(), k.mkdir()
    data_io.save_pfm(str(d / "00000003.pfm"), depth)
    Image.fromarray(mask).save(str(k / "00000003.png"))
    data_io.save_pfm(str(d / "depth_map_0004.pfm"), depth + 1)
    Image.fromarray(mask).save(str(k / "depth_visual_0004.png"))
    for vid, want in ((3, depth), (4, depth + 1)):
        gd, gm = tool.load_gt(str(d), str(k), vid, "cpu")
        assert gd.dtype == torch.float32 and gm.dtype == torch.bool
        assert np.array_equal(gd.numpy(), want) and np.array_equal(gm.numpy(), mask > 10)
    with pytest.raises(SystemExit):
        tool.load_gt(str(d), str(k), 5, "cpu")
    means = {"abs_depth_error": 1.25, "thres1mm_error": 1.0 / 3.0}
    metrics.write_depth_metric_txt(str(tmp_path / "depth_metric.txt"), means)
    assert open(tmp_path / "depth_metric.txt").read() == "abs_depth_error 1.25\nthres1mm_error 0.3333333333333333\n"
