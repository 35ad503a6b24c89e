"""CPU tests of tests/fusion_filter_util.py, the float64 rule that tests/test_hip_fusion_edges.py holds the consistency-filter kernels to.

1. The util restates the reference: in float32 it reproduces the vectors of the real misc/fusion.py (tests/golden/fusion.npz) and
   oracle.ref_fusion on fresh inputs within the bounds tests/test_hip_fusion.py uses for them; in float64 it equals oracle.ref_fusion
   evaluated in float64 (pixel grid cast, nothing else touched) to 1e-9 relative, decisions exactly wherever their margin exceeds 1e-6.
2. Every case of the GPU test contains what it is there for and stays within the caps on undecided pixels (``static_exercise`` /
   ``dynamic_exercise``); both are computed from the float64 rule alone, so the GPU comparison cannot pass for want of pixels.
"""
import numpy as np
import pytest
import torch

import fusion_filter_util as fu
from conftest import load_golden

KEYS = ("ref_depth", "src_depths", "ref_cam", "src_cams")


def _golden_case(g, tag):
    return {k: g["%s_%s" % (tag, k)] for k in KEYS}


def _check_static(got, want):
    """the bounds of tests/test_hip_fusion.py::_check"""
    rep, wrep = got["reproj_xyd"].astype(np.float64), np.asarray(want["reproj_xyd"], np.float64)
    xy_err = np.abs(rep[:, :, :2] - wrep[:, :, :2])
    d_err = np.abs(rep[:, :, 2] - wrep[:, :, 2]) / np.maximum(np.abs(wrep[:, :, 2]), 1.0)
    assert (xy_err > 2e-3 + 4e-6 * np.abs(wrep[:, :, :2])).mean() < 1e-3, xy_err.max()
    assert (d_err > 1e-5).mean() < 1e-3, d_err.max()
    assert np.array_equal(got["in_range"], np.asarray(want["in_range"])[:, :, 0])
    mm = got["masks"] != np.asarray(want["masks"])[:, :, 0]
    assert mm.mean() < 2e-3, mm.mean()
    assert (got["mask"] != np.asarray(want["mask"])[:, 0]).mean() < 2e-3
    agree = ~mm.any(1)
    wave = np.asarray(want["ref_depth_ave"])[:, 0]
    assert (np.abs(got["ref_depth_ave"] - wave) / np.abs(wave))[agree].max() < 1e-5
    wpts = np.asarray(want["points"])
    assert np.abs(got["points"] - wpts)[np.broadcast_to(agree[:, None], wpts.shape)].max() < 1e-5 * np.abs(wpts).max()


def _check_dynamic(got, want):
    """the bounds of tests/test_hip_fusion.py::_check_dynamic"""
    rep, wrep = got["reproj_xyd"].astype(np.float64), np.asarray(want["reproj_xyd"], np.float64)
    err = np.abs(rep - wrep)
    assert (err > 2e-3 + 4e-6 * np.abs(wrep)).mean() < 1e-3, err.max()
    mm = got["masks"] != np.asarray(want["masks"])
    assert mm.mean() < 2e-3, mm.mean()
    assert (got["vis_mask"] != np.asarray(want["vis_mask"])[:, :, 0]).mean() < 2e-3
    assert (got["geo_mask"] != np.asarray(want["geo_mask"])[:, 0]).mean() < 2e-3
    agree = ~mm.any((1, 2))
    wave = np.asarray(want["ref_depth_ave"])[:, 0]
    assert (np.abs(got["ref_depth_ave"] - wave) / np.abs(wave))[agree].max() < 1e-5
    wpts = np.asarray(want["points"])
    assert np.abs(got["points"] - wpts)[np.broadcast_to(agree[:, None], wpts.shape)].max() < 1e-5 * np.abs(wpts).max()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float32_rule_reproduces_the_reference_vectors(tag):
    g = load_golden("fusion.npz")
    case = _golden_case(g, tag)
    thr = [float(x) for x in g[tag + "_thresholds"]]
    got = fu.static_rule(case, *thr, dtype=np.float32)
    _check_static(got, {k: g["%s_%s" % (tag, k)] for k in ("reproj_xyd", "in_range", "masks", "mask", "ref_depth_ave", "points")})
    bases = [float(x) for x in g[tag + "_dyn_bases"]]
    want = {k: g["%s_dyn_%s" % (tag, k)] for k in ("reproj_xyd", "masks", "vis_mask", "geo_mask", "ref_depth_ave", "points")}
    want["geo_mask"] = want["geo_mask"][0][:, None]          # the reference's broadcast for n > 1, see mvsformer_amd/fusion.py
    _check_dynamic(fu.dynamic_rule(case, *bases, dtype=np.float32), want)


def test_float32_rule_reproduces_the_oracle_on_fresh_inputs():
    from oracle import ref_fusion
    case = ref_fusion.make_fusion_case(n=2, v=5, h=36, w=52, seed=7, noise=0.006)
    want = ref_fusion.filter_depth_maps(*[case[k] for k in KEYS], 0.8, 0.015, 3)
    _check_static(fu.static_rule({k: case[k].numpy() for k in KEYS}, 0.8, 0.015, 3, np.float32), {k: v.numpy() for k, v in want.items()})
    case = ref_fusion.make_fusion_case(n=1, v=10, h=36, w=52, seed=11, noise=0.002)
    want = ref_fusion.dynamic_filter_depth_maps(*[case[k] for k in KEYS], 4, 1300)
    _check_dynamic(fu.dynamic_rule({k: case[k].numpy() for k in KEYS}, 4, 1300, np.float32), {k: v.numpy() for k, v in want.items()})


def _close(got, want, what):
    want = np.asarray(want, np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= 1e-9, (what, err.max())


def test_float64_rule_equals_the_oracle_in_float64(monkeypatch):
    from oracle import ref_fusion
    centres = ref_fusion.pixel_centres
    static = {name: fu.static_case(name)["case"] for name in ("5x65", "17x20")}
    dynamic = {name: fu.dynamic_case(name)["case"] for name in ("5x65", "4x64")}
    monkeypatch.setattr(ref_fusion, "pixel_centres", lambda h, w: centres(h, w).double())       # the scenes above are built: float32 grid
    for name, case in static.items():
        h, w, n, v, th, seed = fu.STATIC_CASES[name]
        args = [torch.from_numpy(case[k]).double() for k in KEYS]
        dist, dep = fu.THRESHOLDS[th]
        want = ref_fusion.filter_depth_maps(*args, dist, dep, 3)
        got = fu.static_rule(case, dist, dep, 3, np.float64)
        _close(got["reproj_xyd"], want["reproj_xyd"], "reproj_xyd")
        sure = (got["m_clamp"] > 1e-6) & (got["m_range"] > 1e-6)
        assert np.array_equal(got["in_range"][sure], want["in_range"].numpy()[:, :, 0][sure])
        sure &= (got["m_dist"] > 1e-6) & (got["m_dep"] > 1e-6)
        assert sure.mean() > 0.98
        assert np.array_equal(got["masks"][sure], want["masks"].numpy()[:, :, 0][sure])
        allsure = sure.all(1)
        assert np.array_equal(got["mask"][allsure], want["mask"].numpy()[:, 0][allsure])
        _close(got["ref_depth_ave"][allsure], want["ref_depth_ave"].numpy()[:, 0][allsure], "ref_depth_ave")
        sel = np.broadcast_to(allsure[:, None], got["points"].shape)
        _close(got["points"][sel], want["points"].numpy()[sel], "points")
    for name, case in dynamic.items():
        h, w, n, v, th, seed = fu.DYNAMIC_CASES[name]
        db, rb = fu.BASES[th]
        args = [torch.from_numpy(case[k]).double() for k in KEYS]
        want = ref_fusion.dynamic_filter_depth_maps(*args, db, rb)
        got = fu.dynamic_rule(case, db, rb, np.float64)
        _close(got["reproj_xyd"], want["reproj_xyd"], "dynamic reproj_xyd")
        sure = (got["m_cd"] > 1e-6) & (got["m_dd"] > 1e-6)                            # [n,v,v-1,h,w]
        assert sure.mean() > 0.98
        assert np.array_equal(got["masks"][sure], want["masks"].numpy()[sure])
        allsure = sure.all((1, 2))
        assert np.array_equal(got["vis_mask"][sure[:, :, -1]], want["vis_mask"].numpy()[:, :, 0][sure[:, :, -1]])
        geo = want["geo_mask"].numpy()
        geo = np.stack([geo[b, b] for b in range(n)]) if geo.shape[1] == n and n > 1 else geo[:, 0]     # [n,n,h,w] broadcast of the reference
        assert np.array_equal(got["geo_mask"][allsure], geo[allsure])
        _close(got["ref_depth_ave"][allsure], want["ref_depth_ave"].numpy()[:, 0][allsure], "dynamic ref_depth_ave")


def test_prob_filter_rule_is_the_oracle():
    from oracle import ref_fusion
    conf = torch.rand(3, 4, 5, 65, generator=torch.Generator().manual_seed(0))
    conf[0, 1, 0, :8] = 0.5                                                           # ties: the test is strict
    for C in range(1, 5):
        th = [0.3, 0.5, 0.2, 0.4][:C]
        assert np.array_equal(fu.prob_filter_rule(conf.numpy()[:, :C], th), ref_fusion.prob_filter(conf, th).numpy())
    assert not fu.prob_filter_rule(conf.numpy()[:, :2], [0.3, 0.5])[0, 0, 0, :8].any()


@pytest.mark.parametrize("name", list(fu.STATIC_CASES))
def test_static_case_is_exercised_and_within_caps(name):
    c = fu.static_case(name)
    v = fu.STATIC_CASES[name][3]
    figures, missed = fu.static_exercise(c["r64"], c["tol"], fu.thres_view_mask(c["r64"], 2), fu.thres_view_mask(c["r64"], 1 if v == 1 else v))
    print(name, figures)
    assert not missed, (missed, figures)
    assert fu.thres_view_mask(c["r64"], 1).all() and not fu.thres_view_mask(c["r64"], v + 2).any()


@pytest.mark.parametrize("name", list(fu.DYNAMIC_CASES))
def test_dynamic_case_is_exercised_and_within_caps(name):
    c = fu.dynamic_case(name)
    figures, missed = fu.dynamic_exercise(c["r64"], c["tol"])
    print(name, figures)
    assert not missed, (missed, figures)


def test_static_and_dynamic_sampling_differ():
    """the static filter blends back-projected taps, the dynamic one back-projects a blended depth: on the 5x65 scene some decided pixel's
    reprojected depths are further apart than 100 times the bar of either"""
    c = fu.dynamic_case("5x65")
    db, rb = c["bases"]
    s64 = fu.static_rule(c["case"], dtype=np.float64)
    s32 = fu.static_rule(c["case"], dtype=np.float32)
    stol = fu.static_tolerances(s64, fu.static_bars(s64, s32), 1.0, 0.01)
    diff = np.abs(s64["reproj_xyd"][:, :, 2] - c["r64"]["reproj_xyd"][:, :, 2])
    both = stol["blend_decided"] & c["tol"]["blend_decided"] & np.isfinite(diff)
    assert (diff > 100 * np.maximum(stol["reproj_xyd"][:, :, 2], c["tol"]["reproj_xyd"][:, :, 2]))[both].any()
