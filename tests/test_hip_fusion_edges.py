"""GPU tests of the depth-map consistency filters (csrc/fusion_core.h, fusion.hip, the job-table twins of pointcloud.hip) against the
float64 rule of tests/fusion_filter_util.py, at launch-tile edges, batch and view offsets, image borders and thresholds.

Decisions (``in_range``, per-view ``masks``, level masks, ``vis_mask``, ``mask``, ``geo_mask``) must equal the rule exactly wherever the
rule's margin exceeds the bar of the deciding quantity - no fraction, no flipped pixel; continuous outputs must lie within the per-pixel
tolerance.  Bars and tolerances are 4x the float32 rule's own error against the float64 rule plus the rule's sensitivity to the sample
index (fusion_filter_util.py); they never see a kernel's output.  tests/test_fusion_filter_refs.py checks on the CPU that every case
contains its edges and that at most 2 % of any compared tensor is undecided.  Every entry point runs twice and must repeat its bits.

Non-finite depths (the contract next to ``geo_view``): ``in_range`` and the view's mask are 0, the reprojected triple is unspecified,
pixels that do not touch the planted value keep their bits.
"""
import numpy as np
import pytest
import torch

import fusion_filter_util as fu

pytestmark = pytest.mark.gpu

KEYS = ("ref_depth", "src_depths", "ref_cam", "src_cams")
STATIC_ALL = ("mask", "ref_depth_ave", "points", "reproj_xyd", "in_range", "masks")
DYNAMIC_ALL = ("geo_mask", "ref_depth_ave", "points", "reproj_xyd", "masks", "vis_mask")


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _args(case, dev):
    return [torch.from_numpy(case[k]).to(dev) for k in KEYS]


def _np(out):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _twice(fn):
    a, b = _np(fn()), _np(fn())
    _same(a, b, "second run")
    return a


def _exact(got, want, decided, what):
    bad = (got.astype(bool) != want.astype(bool)) & decided
    assert not bad.any(), (what, "differs on %d decided entries, first at %s" % (bad.sum(), np.argwhere(bad)[0]))


def _within(got, want, tol, decided, what):
    """-> (largest error, largest error / tolerance) over the decided entries"""
    err = np.abs(got.astype(np.float64) - want)
    sel = decided & np.isfinite(want) & np.isfinite(tol)
    ratio = np.where(sel, err / np.maximum(tol, 1e-300), 0.0)
    assert not (np.where(sel, err, 0.0) > np.where(sel, tol, 0.0)).any(), (what, "error / tolerance", ratio.max(), "at", np.unravel_index(ratio.argmax(), ratio.shape))
    return float(np.where(sel, err, 0.0).max()), float(ratio.max())


def _b3(m):
    return np.broadcast_to(m[:, :, None], m.shape[:2] + (3,) + m.shape[2:])


def _report(kind, name, bars, seen, tol):
    print("EDGE %s %-6s bars(4x fp32 rule): %s" % (kind, name, " ".join("%s=%.2e" % (k, fu.MULT * v) for k, v in bars.items())))
    print("EDGE %s %-6s kernel max err (err/tol): %s | undecided: view %.4f pixel %.4f" % (
        kind, name, " ".join("%s=%.2e(%.2f)" % (k, e, r) for k, (e, r) in seen.items()), 1 - tol["view_decided"].mean(), 1 - tol["pixel_decided"].mean()))


# ---------------------------------------------------------------------------------------------------------------- static filter
def _compare_static(got, c, what):
    r, tol = c["r64"], c["tol"]
    seen = {}
    _exact(got["in_range"][:, :, 0], r["in_range"], tol["range_decided"], (what, "in_range"))
    _exact(got["masks"][:, :, 0], r["masks"], tol["view_decided"], (what, "masks"))
    _exact(got["mask"][:, 0], fu.thres_view_mask(r, 2), tol["pixel_decided"], (what, "mask"))
    seen["reproj_xyd"] = _within(got["reproj_xyd"], r["reproj_xyd"], tol["reproj_xyd"], _b3(tol["blend_decided"]), (what, "reproj_xyd"))
    seen["ref_depth_ave"] = _within(got["ref_depth_ave"][:, 0], r["ref_depth_ave"], tol["ref_depth_ave"], tol["pixel_decided"], (what, "ref_depth_ave"))
    seen["points"] = _within(got["points"], r["points"], tol["points"], np.broadcast_to(tol["pixel_decided"][:, None], r["points"].shape), (what, "points"))
    return seen


@pytest.mark.parametrize("name", list(fu.STATIC_CASES))
def test_geo_filter_against_the_rule(dev, name):
    from mvsformer_amd import fusion, ops
    c = fu.static_case(name)
    rd, sd, rc, sc = _args(c["case"], dev)
    dist, dep = c["thresholds"]
    v = sd.shape[1]
    full = _twice(lambda: ops.geo_filter(rd, sd, rc, sc, dist, dep, 2, want=STATIC_ALL))
    seen = _compare_static(full, c, name)
    _report("static", name, c["bars"], seen, c["tol"])
    # thres_view: msum >= thres_view - 1.1 makes 1 "always" and V + 2 "never"
    decided = c["tol"]["pixel_decided"]
    for tv in (1, 2, v, v + 2):
        lean = _twice(lambda: ops.geo_filter(rd, sd, rc, sc, dist, dep, tv, want=("mask",)))
        assert set(lean) == {"mask"}
        _exact(lean["mask"][:, 0], fu.thres_view_mask(c["r64"], tv), decided, (name, "mask at thres_view", tv))
        if tv == 1:
            assert lean["mask"].all()
        if tv == v + 2:
            assert not lean["mask"].any()
        if tv == 2:
            assert np.array_equal(lean["mask"], full["mask"])
    # the reference's three calls == the fused pass, bit for bit
    reproj, in_range = fusion.get_reproj(rd, sd, rc, sc)
    masks, mask = fusion.vis_filter(rd, reproj, in_range, dist, dep, 2)
    ave = fusion.ave_fusion(rd, reproj, masks)
    _same(_np(dict(reproj_xyd=reproj, in_range=in_range, masks=masks, mask=mask, ref_depth_ave=ave)),
          {k: full[k] for k in ("reproj_xyd", "in_range", "masks", "mask", "ref_depth_ave")}, (name, "op-level chain"))


@pytest.mark.parametrize("name", list(fu.STATIC_CASES))
def test_vis_filter_against_the_rule(dev, name):
    """vis_filter / ave_fusion alone, on the float64 rule's reprojection rounded to float32: the rule is evaluated on those very numbers, so
    the bars are the arithmetic ones without the sensitivity term"""
    from mvsformer_amd import ops
    c = fu.static_case(name)
    r, e = c["r64"], c["bars"]
    dist, dep = c["thresholds"]
    rep32, inr32, rd32 = r["reproj_xyd"].astype(np.float32), r["in_range"].astype(np.float32), c["case"]["ref_depth"]
    want = fu.static_vis(rd32[:, 0], rep32, inr32, dist, dep, 2, np.float64)
    dscale = np.maximum(1.0, np.maximum(np.abs(rd32[:, 0].astype(np.float64))[:, None], np.abs(rep32[:, :, 2].astype(np.float64))))
    d_dist = want["m_dist"] > fu.MULT * e["dist"] * np.maximum(1.0, want["dist"])
    d_dep = want["m_dep"] > fu.MULT * e["dep"] * dscale
    fails = (d_dist & ~(want["dist"] < dist)) | (d_dep & ~(want["dep_lhs"] < want["dep_rhs"]))
    view = (inr32 == 0) | fails | (d_dist & d_dep)
    assert view.mean() > 1 - fu.UNDECIDED_CAP
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rd32, rep32, inr32[:, :, None])]
    for tv in (1, 2, rep32.shape[1], rep32.shape[1] + 2):
        got = _twice(lambda: dict(zip(("masks", "mask", "ref_depth_ave"), ops.vis_filter(t[0], t[1], t[2], None, dist, dep, tv))))
        _exact(got["masks"][:, :, 0], want["masks"], view, (name, "masks"))
        _exact(got["mask"][:, 0], want["masks"].sum(1) >= tv - 1.1, view.all(1), (name, "mask", tv))
        tol_ave = fu.MULT * e["ave"] * np.maximum(1.0, np.abs(want["ref_depth_ave"]))
        _within(got["ref_depth_ave"][:, 0], want["ref_depth_ave"], tol_ave, view.all(1), (name, "ref_depth_ave"))
    # masks given: ave_fusion alone
    masks_in = torch.from_numpy(np.ascontiguousarray(want["masks"][:, :, None].astype(np.float32))).to(dev)
    got = _twice(lambda: dict(ref_depth_ave=ops.vis_filter(t[0], t[1], None, masks_in, 0.0, 0.0, 0.0, want_masks=False)[2]))
    _within(got["ref_depth_ave"][:, 0], want["ref_depth_ave"], tol_ave, np.ones(tol_ave.shape, bool), (name, "ave_fusion"))


# --------------------------------------------------------------------------------------------------------------- dynamic filter
def _compare_dynamic(got, c, what):
    r, tol = c["r64"], c["tol"]
    seen = {}
    if "masks" in got:
        _exact(got["masks"], r["masks"], tol["level_decided"], (what, "level masks"))
        _exact(got["vis_mask"][:, :, 0], r["vis_mask"], tol["level_decided"][:, :, -1], (what, "vis_mask"))
        seen["reproj_xyd"] = _within(got["reproj_xyd"], r["reproj_xyd"], tol["reproj_xyd"], _b3(tol["blend_decided"]), (what, "reproj_xyd"))
    _exact(got["geo_mask"][:, 0], r["geo_mask"], tol["geo_decided"], (what, "geo_mask"))
    seen["ref_depth_ave"] = _within(got["ref_depth_ave"][:, 0], r["ref_depth_ave"], tol["ref_depth_ave"], tol["pixel_decided"], (what, "ref_depth_ave"))
    seen["points"] = _within(got["points"], r["points"], tol["points"], np.broadcast_to(tol["pixel_decided"][:, None], r["points"].shape), (what, "points"))
    return seen


@pytest.mark.parametrize("name", list(fu.DYNAMIC_CASES))
def test_geo_filter_dynamic_against_the_rule(dev, name):
    from mvsformer_amd import ops
    c = fu.dynamic_case(name)
    rd, sd, rc, sc = _args(c["case"], dev)
    db, rb = c["bases"]
    full = _twice(lambda: ops.geo_filter_dynamic(rd, sd, rc, sc, db, rb, want=DYNAMIC_ALL))
    seen = _compare_dynamic(full, c, name)
    _report("dynamic", name, c["bars"], seen, c["tol"])
    lean = _twice(lambda: ops.geo_filter_dynamic(rd, sd, rc, sc, db, rb))
    assert set(lean) == {"geo_mask", "ref_depth_ave", "points"}
    _same(lean, {k: full[k] for k in lean}, (name, "without per-view outputs"))
    # vis_filter_dynamic on the fused pass's own reprojection == the fused pass
    op = _twice(lambda: ops.vis_filter_dynamic(rd, torch.from_numpy(full["reproj_xyd"]).to(dev), db, rb, want=("masks", "vis_mask", "geo_mask", "ref_depth_ave")))
    _same(op, {k: full[k] for k in op}, (name, "vis_filter_dynamic"))


@pytest.mark.parametrize("name", list(fu.DYNAMIC_CASES))
def test_vis_filter_dynamic_against_the_rule(dev, name):
    """on the float64 rule's reprojection rounded to float32; arithmetic bars only, as in test_vis_filter_against_the_rule"""
    from mvsformer_amd import ops
    c = fu.dynamic_case(name)
    e = c["bars"]
    db, rb = c["bases"]
    rd32 = c["case"]["ref_depth"]
    rep32 = np.where(np.isfinite(c["r64"]["reproj_xyd"]), c["r64"]["reproj_xyd"], 0.0).astype(np.float32)
    want = fu.dynamic_vis(rd32[:, 0], rep32, db, rb, np.float64)
    bar_cd = fu.MULT * e["cd"] * np.maximum(1.0, want["cd"])
    bar_dd = np.where(rd32[:, 0][:, None] == 0, 0.0, fu.MULT * e["dd"] * np.maximum(1.0, np.where(np.isfinite(want["dd"]), np.abs(want["dd"]), 1.0)))
    cd_k, dd_k = want["m_cd"] > bar_cd[:, :, None], want["m_dd"] > bar_dd[:, :, None]
    level = (cd_k & ~(want["cd"][:, :, None] < want["t_cd"])) | (dd_k & ~(want["dd"][:, :, None] < want["t_dd"])) | (cd_k & dd_k)
    assert level.mean() > 1 - fu.UNDECIDED_CAP
    ks = np.arange(2, level.shape[2] + 2).reshape(1, -1, 1, 1)
    geo_decided = ((want["masks"] & level).sum(1) >= ks).any(1) | ((want["masks"] | ~level).sum(1) < ks).all(1)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (rd32, rep32)]
    got = _twice(lambda: ops.vis_filter_dynamic(t[0], t[1], db, rb, want=("masks", "vis_mask", "geo_mask", "ref_depth_ave")))
    _exact(got["masks"], want["masks"], level, (name, "level masks"))
    _exact(got["vis_mask"][:, :, 0], want["vis_mask"], level[:, :, -1], (name, "vis_mask"))
    _exact(got["geo_mask"][:, 0], want["geo_mask"], geo_decided, (name, "geo_mask"))
    tol_ave = fu.MULT * e["ave"] * np.maximum(1.0, np.abs(want["ref_depth_ave"]))
    _within(got["ref_depth_ave"][:, 0], want["ref_depth_ave"], tol_ave, level[:, :, -1].all(1), (name, "ref_depth_ave"))


def test_dynamic_filter_refuses_a_single_source_view(dev):
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    case = fu.make_edge_case(1, 1, 5, 65, 2)
    rd, sd, rc, sc = _args(case, dev)
    with pytest.raises(MvsHipError):
        ops.geo_filter_dynamic(rd, sd, rc, sc)
    with pytest.raises(MvsHipError):
        ops.vis_filter_dynamic(rd, torch.zeros(1, 1, 3, 5, 65, device=dev), 4, 1300)


# ------------------------------------------------------------------------------------------------------------------ prob_filter
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_prob_filter_against_the_rule(dev, C):
    from mvsformer_amd import ops
    th = [0.3, 0.5, 0.2, 0.4][:C]
    for i, (h, w, *_) in enumerate(fu.STATIC_CASES.values()):
        rng = np.random.default_rng(10 * C + i)
        conf = rng.uniform(size=(3, C, h, w)).astype(np.float32)
        conf[1, C - 1, h - 1, w - 1] = np.float32(th[C - 1])                      # a tie at the last pixel of the last channel: strict >
        conf[2, 0, 0, 0] = np.nextafter(np.float32(th[0]), np.float32(1))
        want = fu.prob_filter_rule(conf, th)
        assert not want[1, 0, h - 1, w - 1] and 0 < want.mean() < 1
        tconf = torch.from_numpy(conf).to(dev)
        got = _twice(lambda: dict(mask=ops.prob_filter(tconf, th)))
        assert got["mask"].dtype == np.bool_ and np.array_equal(got["mask"], want)
        depth = rng.uniform(1, 2, size=(3, 1, h, w)).astype(np.float32)
        tdepth = torch.from_numpy(depth).to(dev)
        ops.prob_filter(tconf, th, depth_inplace=tdepth)
        assert np.array_equal(_bits(tdepth.cpu().numpy()), _bits(np.where(want, depth, np.float32(0))))


# -------------------------------------------------------------------------------------------------------------------- job table
JOBS = [(0, [3, 1]), (2, [5]), (1, [5, 3, 4, 0, 2]), (3, [2, 0])]                 # ragged, non-ascending; views 4 and 5 are never a reference


def _scene(h, w, dev):
    case = fu.make_edge_case(1, 5, h, w, 2)
    depth = np.concatenate([case["ref_depth"][0], case["src_depths"][0, :, 0]])                # [6,h,w]
    cams = np.concatenate([case["ref_cam"], case["src_cams"][0]])                             # [6,2,4,4]
    src = depth.copy()
    src[:, ::3, 1::4] = 0.0                                                                    # the prob-filtered copy a view contributes as a source
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (depth, src, cams)]


def _gather(depth, src, cams, r, srcs):
    s = torch.tensor(srcs, device=depth.device)
    return depth[r][None, None].contiguous(), src[s][None, :, None].contiguous(), cams[r][None].contiguous(), cams[s][None].contiguous()


@pytest.mark.parametrize("shape", [(5, 65), (9, 130)])
def test_scene_entry_points_repeat_the_per_sample_bits(dev, shape):
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    depth, src, cams = _scene(*shape, dev)
    table = ops.JobTable(JOBS, 6, dev)
    for dist, dep in fu.THRESHOLDS.values():
        got = _twice(lambda: ops.geo_filter_scene(table, depth, src, cams, dist, dep, 2, want=("mask", "ref_depth_ave", "points")))
        assert got["mask"].any() and not got["mask"].all()
        for i, (r, srcs) in enumerate(JOBS):
            one = _np(ops.geo_filter(*_gather(depth, src, cams, r, srcs), dist, dep, 2))
            _same({k: v[i] for k, v in got.items()}, {"mask": one["mask"][0, 0], "ref_depth_ave": one["ref_depth_ave"][0, 0], "points": one["points"][0]},
                  ("geo_filter_scene", shape, i))
    dyn_jobs = [j for j in JOBS if len(j[1]) >= 2] + [(2, [5, 4])]
    table = ops.JobTable(dyn_jobs, 6, dev)
    table.n_src[3] = 1                                       # the device table says: one source.  The host list still says two, so the call goes through
    for db, rb in fu.BASES.values():
        got = _twice(lambda: ops.geo_filter_dynamic_scene(table, depth, src, cams, db, rb, want=("geo_mask", "ref_depth_ave", "points")))
        assert got["geo_mask"][:3].any()
        for i, (r, srcs) in enumerate(dyn_jobs[:3]):
            one = _np(ops.geo_filter_dynamic(*_gather(depth, src, cams, r, srcs), db, rb))
            _same({k: v[i] for k, v in got.items()}, {"geo_mask": one["geo_mask"][0, 0], "ref_depth_ave": one["ref_depth_ave"][0, 0], "points": one["points"][0]},
                  ("geo_filter_dynamic_scene", shape, i))
        assert not got["geo_mask"][3].any() and not got["ref_depth_ave"][3].any() and not got["points"][3].any()       # nothing kept
    with pytest.raises(MvsHipError):
        ops.geo_filter_dynamic_scene(ops.JobTable([(0, [1])], 6, dev), depth, src, cams)


# ----------------------------------------------------------------------------------------------------------- non-finite depths
def test_non_finite_depths(dev):
    from mvsformer_amd import ops
    c = fu.static_case("5x65")
    r, tol = c["r64"], c["tol"]
    dist, dep = c["thresholds"]
    n, v, h, w = r["ix"].shape
    clean = _np(ops.geo_filter(*_args(c["case"], dev), dist, dep, 2, want=STATIC_ALL))
    case = {k: a.copy() for k, a in c["case"].items()}
    ref_plants = {(0, 2, 10): np.nan, (0, 2, 30): np.inf, (0, 3, 50): -np.inf}
    src_plants = {(1, 2, 1, 12): np.nan, (1, 2, 3, 33): np.inf, (2, 0, 2, 55): -np.inf}
    touched = np.zeros((n, v, h, w), bool)                    # (view, pixel) pairs whose blend reads a planted value, weight 0 included
    for (b, y, x), val in ref_plants.items():
        case["ref_depth"][b, 0, y, x] = val
        touched[b, :, y, x] = True
    src_touched = np.zeros_like(touched)
    for (b, s, y, x), val in src_plants.items():
        case["src_depths"][b, s, 0, y, x] = val
        src_touched[b, s] |= (r["tap_valid"][b, s] & (r["tap_x"][b, s] == x) & (r["tap_y"][b, s] == y)).any(0)
    assert src_touched.sum() >= 3
    sure = tol["blend_decided"]                               # the rule and the kernel read the same four taps
    got = _np(ops.geo_filter(*_args(case, dev), dist, dep, 2, want=STATIC_ALL))
    for (b, y, x) in ref_plants:
        assert not got["in_range"][b, :, 0, y, x].any() and not got["masks"][b, :, 0, y, x].any()
    hit = src_touched & sure & ~touched
    assert not got["masks"][:, :, 0][hit].any()
    assert np.array_equal(got["in_range"][:, :, 0][hit], clean["in_range"][:, :, 0][hit])
    free = ~touched & ~src_touched & sure
    assert free.mean() > 0.9
    for k in ("in_range", "masks"):
        assert np.array_equal(_bits(got[k])[:, :, 0][free], _bits(clean[k])[:, :, 0][free]), k
    assert np.array_equal(_bits(got["reproj_xyd"])[_b3(free)], _bits(clean["reproj_xyd"])[_b3(free)])
    free_px = (~touched & ~src_touched).all(1) & sure.all(1)
    for k in ("mask", "ref_depth_ave"):
        assert np.array_equal(_bits(got[k])[:, 0][free_px], _bits(clean[k])[:, 0][free_px]), k
    sel = np.broadcast_to(free_px[:, None], got["points"].shape)
    assert np.array_equal(_bits(got["points"])[sel], _bits(clean["points"])[sel])
