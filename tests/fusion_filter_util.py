"""TEST INFRASTRUCTURE - the depth-map consistency filters of misc/fusion.py as a per-pixel rule in numpy, written once over a dtype.

``static_rule`` is get_reproj -> vis_filter -> ave_fusion -> points (fusion.py:80-114, test.py:425-434), ``dynamic_rule`` is
get_reproj_dynamic -> vis_filter_dynamic -> the reduction of test.py:494-514, as oracle/ref_fusion.py restates them.  Pixels are
vectorised, samples and views are Python loops.  ``dtype`` (np.float64 or np.float32) is the type of EVERY operation, camera inverses
included; every product-sum is written in the order a matrix product takes it.  Next to the values the rule returns, for every decision
it takes, the distance of the deciding quantity from its switch point ("margin"), in that quantity's own unit.

Bars.  ``static_bars`` / ``dynamic_bars`` measure the reference's own arithmetic: the rule in float32 against the rule in float64 on the
same case, per quantity, as a scalar relative to a per-pixel scale (1 for quantities of order one, the magnitude for the rest, so a
prob-filtered tap that back-projects hundreds of pixels away counts by its ulp and not by its size).  ``static_tolerances`` /
``dynamic_tolerances`` turn them into what a float32 implementation with another operation order gets: ``MULT`` = 4 times the figure,
plus the rule's own sensitivity at the pixel - the bilinear gradient of the blend (taps outside the image count as 0, which is what
makes the zero-padding ring and a zero-depth tap steep) times the 4x error of the sample index.  A decision is DECIDED where its margin
exceeds its bar; a mask entry is decided when the decisions feeding it are, or when one of its tests decidedly fails (the entry is then 0
whatever the others say); a pixel when all its views are; the dynamic keep flag when the undecided level entries cannot change it in
either direction.  Nothing here ever sees a kernel's output.

``make_edge_case`` builds scenes on the cameras of ``oracle.ref_fusion.make_fusion_case``; ``static_exercise`` / ``dynamic_exercise``
count, on the float64 rule alone, what a case must contain for a comparison on it to mean something.
"""
import numpy as np

MULT = 4.0                       # a kernel gets 4x the float32 rule's own error
UNDECIDED_CAP, RING_CAP = 0.02, 0.05
ULP = 2.0 ** -23                 # floor of every measured figure: at 2x2 the sample a figure is the maximum over can be a few pixels, or empty,
                                 # and no float32 result of two and more rounded operations is known better than an ulp of its scale
_PLANE_N = np.array([0.15, -0.1, 1.0]) / np.linalg.norm([0.15, -0.1, 1.0])
_PLANE_D = 600.0
_TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))          # (dx, dy): nw, ne, sw, se - ATen's order


# ------------------------------------------------------------------------------------------------------------ camera algebra
def _grid(h, w, T):
    ys, xs = np.meshgrid(np.arange(h, dtype=T) + T(0.5), np.arange(w, dtype=T) + T(0.5), indexing="ij")
    return xs, ys


def _mat(M, p):
    """rows of M times the column p (a list of arrays), summed left to right"""
    out = []
    for i in range(M.shape[0]):
        acc = M[i, 0] * p[0]
        for j in range(1, len(p)):
            acc = acc + M[i, j] * p[j]
        out.append(acc)
    return out


def _img2cam(Kinv, x, y, d, T):
    """fusion.py:23-28"""
    c = _mat(Kinv, [x, y, np.ones_like(x)])
    den = c[2] + T(1e-9)
    return [ci / den * d for ci in c] + [np.ones_like(x)]


def _hom(M, p, T):
    """fusion.py:31-40 - a 4x4 times a homogeneous point, divided by (w + 1e-9)"""
    q = _mat(M, p)
    den = q[3] + T(1e-9)
    return [qi / den for qi in q]


def _cam2img(K, c, T):
    """fusion.py:43-47"""
    den = c[3] + T(1e-9)
    p = _mat(K, [c[0] / den, c[1] / den, c[2] / den])
    den = p[2] + T(1e-9)
    return p[0] / den, p[1] / den


class _Cams:
    def __init__(self, cam, T):
        cam = np.asarray(cam).astype(T)
        self.E, self.K = cam[0], cam[1, :3, :3]
        self.Ei, self.Ki = np.linalg.inv(self.E).astype(T), np.linalg.inv(self.K).astype(T)


def _a_to_b(a, b, x, y, d, T):
    """pixel (x, y) at depth d of camera a -> homogeneous point in camera b's frame"""
    return _hom(b.E, _hom(a.Ei, _img2cam(a.Ki, x, y, d, T), T), T)


def _cell(ix, iy, h, w, T):
    """ATen's bilinear cell: corner indices, tap weights (nw, ne, sw, se) and tap validities under zeros padding"""
    with np.errstate(invalid="ignore"):
        x0, y0 = np.floor(ix), np.floor(iy)
    fx1, fx0, fy1, fy0 = ix - x0, (x0 + T(1)) - ix, iy - y0, (y0 + T(1)) - iy
    wts = [fx0 * fy0, fx1 * fy0, fx0 * fy1, fx1 * fy1]
    xs = [x0 + T(dx) for dx, _ in _TAPS]
    ys = [y0 + T(dy) for _, dy in _TAPS]
    valid = [(a >= 0) & (a <= w - 1) & (b >= 0) & (b <= h - 1) for a, b in zip(xs, ys)]
    xi = [np.where(v, a, 0).astype(np.int64) for a, v in zip(xs, valid)]
    yi = [np.where(v, b, 0).astype(np.int64) for b, v in zip(ys, valid)]
    return wts, valid, xi, yi


def _int_margin(ix, iy, h, w):
    """distance of the sample index from the next integer (cell choice, tap validity); two pixels and more outside the image every tap of
    either cell is outside, whichever it is"""
    with np.errstate(invalid="ignore"):
        m = np.minimum(np.abs(ix - np.round(ix)), np.abs(iy - np.round(iy)))
        far = (ix < -2) | (ix > w + 1) | (iy < -2) | (iy > h + 1)
    return np.where(np.isfinite(m) & ~far, m, np.inf)


def _points(ref, xs, ys, ave, T):
    """test.py:432-434 -> [3,h,w], and d(point)/d(ave) for the tolerance"""
    c = _img2cam(ref.Ki, xs, ys, ave, T)
    p = _hom(ref.Ei, c, T)
    ray = _mat(ref.Ki, [xs, ys, np.ones_like(xs)])
    ray = [r / (ray[2] + T(1e-9)) for r in ray]
    slope = np.stack([np.abs(g) for g in _mat(ref.Ei[:3, :3], ray)])
    return np.stack(p[:3]), slope


def _unpack(case, T):
    rd, sd = np.asarray(case["ref_depth"]).astype(T)[:, 0], np.asarray(case["src_depths"]).astype(T)[:, :, 0]
    return rd, sd, np.asarray(case["ref_cam"]), np.asarray(case["src_cams"])


# ------------------------------------------------------------------------------------------------------------ static filter
def static_vis(ref_depth, reproj_xyd, in_range, dist_thresh, depth_thresh, thres_view, dtype=np.float64):
    """vis_filter + ave_fusion (fusion.py:101-114) on a materialised reproj_xyd [n,v,3,h,w] / in_range [n,v,h,w]; ref_depth [n,h,w]"""
    T = dtype
    rd, rep, inr = np.asarray(ref_depth).astype(T), np.asarray(reproj_xyd).astype(T), np.asarray(in_range).astype(T)
    h, w = rd.shape[-2:]
    xs, ys = _grid(h, w, T)
    with np.errstate(all="ignore"):
        dx, dy = rep[:, :, 0] - xs, rep[:, :, 1] - ys
        dist = np.sqrt(dx * dx + dy * dy)
        d = rep[:, :, 2]
        lhs, rhs = np.abs(rd[:, None] - d), np.maximum(rd[:, None], d) * T(depth_thresh)
        masks = np.minimum(np.minimum(inr, (dist < T(dist_thresh)).astype(T)), (lhs < rhs).astype(T))
        msum = masks.sum(1)
        ave = ((d * masks).sum(1) + rd) / (msum + T(1))
        m_dist, m_dep = np.abs(dist - T(dist_thresh)), np.abs(rhs - lhs)
    inf = T(np.inf)
    return dict(dist=dist, dep_lhs=lhs, dep_rhs=rhs, masks=masks, mask=msum >= T(thres_view) - T(1.1), ref_depth_ave=ave,
                m_dist=np.where(np.isfinite(m_dist), m_dist, inf), m_dep=np.where(np.isfinite(m_dep), m_dep, inf))


def static_rule(case, dist_thresh=1.0, depth_thresh=0.01, thres_view=2, dtype=np.float64):
    """-> dict of [n,v,h,w] per-view arrays (``reproj_xyd [n,v,3,h,w]``, ``tap_valid [n,v,4,h,w]``, ``tap_xyd [n,v,4,3,h,w]``,
    ``tap_x`` / ``tap_y`` / ``tap_depth`` [n,v,4,h,w]) and [n,h,w] per-pixel ones (``points [n,3,h,w]``)."""
    T = dtype
    rd, sd, rcam, scam = _unpack(case, T)
    n, v, h, w = sd.shape
    xs, ys = _grid(h, w, T)
    names = ("warp_x", "warp_y", "warp_cx", "warp_cy", "in_range", "ix", "iy", "m_clamp", "m_range", "m_cell")
    o = {k: np.zeros((n, v, h, w), T) for k in names}
    o.update(reproj_xyd=np.zeros((n, v, 3, h, w), T), tap_valid=np.zeros((n, v, 4, h, w), bool), tap_xyd=np.zeros((n, v, 4, 3, h, w), T),
             tap_x=np.zeros((n, v, 4, h, w), np.int64), tap_y=np.zeros((n, v, 4, h, w), np.int64), tap_depth=np.zeros((n, v, 4, h, w), T),
             tap_w=np.zeros((n, v, 4, h, w), T))
    pts, slope = np.zeros((n, 3, h, w), T), np.zeros((n, 3, h, w), T)
    with np.errstate(all="ignore"):
        for b in range(n):
            ref = _Cams(rcam[b], T)
            for s in range(v):
                src = _Cams(scam[b, s], T)
                # the source-grid image srcs2ref_xyd of get_reproj
                c = _a_to_b(src, ref, xs, ys, sd[b, s], T)
                sx, sy = _cam2img(ref.K, c, T)
                simg = (sx, sy, c[2])
                # project_img(dst = reference)
                qx, qy = _cam2img(src.K, _a_to_b(ref, src, xs, ys, rd[b], T), T)
                wx, wy = qx / T(w) * T(2) - T(1), qy / T(h) * T(2) - T(1)
                cx, cy = np.clip(wx, T(-1.1), T(1.1)), np.clip(wy, T(-1.1), T(1.1))
                inr = (T(-1) <= cx) & (cx <= T(1)) & (T(-1) <= cy) & (cy <= T(1))
                ix, iy = ((cx + T(1)) / T(2)) * T(w - 1), ((cy + T(1)) / T(2)) * T(h - 1)
                wts, valid, xi, yi = _cell(ix, iy, h, w, T)
                for k in range(4):
                    for q in range(3):
                        o["tap_xyd"][b, s, k, q] = np.where(valid[k], simg[q][yi[k], xi[k]], T(0))
                    o["tap_depth"][b, s, k] = np.where(valid[k], sd[b, s][yi[k], xi[k]], T(0))
                    o["tap_valid"][b, s, k], o["tap_x"][b, s, k], o["tap_y"][b, s, k], o["tap_w"][b, s, k] = valid[k], xi[k], yi[k], wts[k]
                for q in range(3):
                    acc = np.zeros((h, w), T)
                    for k in range(4):
                        acc = acc + np.where(valid[k], simg[q][yi[k], xi[k]] * wts[k], T(0))
                    o["reproj_xyd"][b, s, q] = acc
                o["warp_x"][b, s], o["warp_y"][b, s], o["warp_cx"][b, s], o["warp_cy"][b, s] = wx, wy, cx, cy
                o["in_range"][b, s], o["ix"][b, s], o["iy"][b, s] = inr, ix, iy
                m = np.minimum(np.abs(np.abs(wx) - T(1.1)) / np.maximum(T(1), np.abs(wx)), np.abs(np.abs(wy) - T(1.1)) / np.maximum(T(1), np.abs(wy)))
                o["m_clamp"][b, s] = np.where(np.isfinite(m), m, T(np.inf))
                o["m_range"][b, s] = np.minimum(np.abs(np.abs(cx) - T(1)), np.abs(np.abs(cy) - T(1)))
                o["m_cell"][b, s] = _int_margin(ix, iy, h, w)
        o.update(static_vis(rd, o["reproj_xyd"], o["in_range"], dist_thresh, depth_thresh, thres_view, T))
        for b in range(n):
            pts[b], slope[b] = _points(_Cams(rcam[b], T), xs, ys, o["ref_depth_ave"][b], T)
    o.update(points=pts, point_slope=slope, ref_depth=rd)
    return o


def _blend_slope(taps, valid):
    """upper bound of |d blend / d ix| + |d blend / d iy| inside the cell; taps [..,4,h,w] with invalid taps as 0"""
    t = [np.where(valid[..., k, :, :], taps[..., k, :, :], 0.0) for k in range(4)]
    return np.maximum(np.abs(t[1] - t[0]), np.abs(t[3] - t[2])) + np.maximum(np.abs(t[2] - t[0]), np.abs(t[3] - t[1]))


def _tap_scale(taps, valid):
    return np.maximum(1.0, np.where(valid, np.abs(taps), 0.0).max(-3))


def _finite_max(x, sel):
    x = np.asarray(x, np.float64)[sel]
    x = x[np.isfinite(x)]
    return float(x.max()) if x.size else 0.0


def _static_smooth(r):
    return r["tap_valid"].all(2) & (r["tap_depth"] > 0).all(2) & (r["ref_depth"][:, None] > 0) & (r["in_range"] > 0)


def static_bars(r64, r32):
    """the float32 rule's largest error against the float64 rule, per quantity (see the module docstring for the scales)"""
    allp = np.ones(r64["ix"].shape, bool)
    smooth = _static_smooth(r64)
    e = {}
    e["warp"] = max(_finite_max(np.abs(r32["warp_" + a].astype(np.float64) - r64["warp_" + a]) / np.maximum(1.0, np.abs(r64["warp_" + a])), allp)
                    for a in "xy")
    e["index"] = max(_finite_max(np.abs(r32[a].astype(np.float64) - r64[a]), allp) for a in ("ix", "iy"))
    err = np.abs(r32["reproj_xyd"].astype(np.float64) - r64["reproj_xyd"])
    for q, name in enumerate(("x", "y", "d")):
        e[name] = _finite_max(err[:, :, q] / _tap_scale(r64["tap_xyd"][:, :, :, q], r64["tap_valid"]), smooth)
    e["dist"] = _finite_max(np.abs(r32["dist"].astype(np.float64) - r64["dist"]) / np.maximum(1.0, r64["dist"]), smooth)
    dscale = np.maximum(1.0, np.maximum(np.abs(r64["ref_depth"][:, None]), np.abs(r64["reproj_xyd"][:, :, 2])))
    e["dep"] = _finite_max((np.abs(r32["dep_lhs"].astype(np.float64) - r64["dep_lhs"]) + np.abs(r32["dep_rhs"].astype(np.float64) - r64["dep_rhs"])) / dscale,
                           smooth)
    same = (r32["masks"] == r64["masks"]).all(1) & (smooth | (r64["masks"] == 0)).all(1)
    e["ave"] = _finite_max(np.abs(r32["ref_depth_ave"].astype(np.float64) - r64["ref_depth_ave"]) / np.maximum(1.0, np.abs(r64["ref_depth_ave"])), same)
    e["points"] = _finite_max(np.abs(r32["points"].astype(np.float64) - r64["points"]) / np.maximum(1.0, np.abs(r64["points"])),
                              np.broadcast_to(same[:, None], r64["points"].shape))
    return {k: max(x, ULP) for k, x in e.items()}


def static_tolerances(r64, e, dist_thresh, depth_thresh, mult=MULT):
    """-> per-pixel tolerances (``reproj_xyd``, ``ref_depth_ave``, ``points``), the decision bars and the decided sets"""
    delta = mult * e["index"]
    tol = np.zeros_like(r64["reproj_xyd"])
    sens = np.zeros_like(tol)
    for q, name in enumerate(("x", "y", "d")):
        taps = r64["tap_xyd"][:, :, :, q]
        sens[:, :, q] = delta * _blend_slope(taps, r64["tap_valid"])
        tol[:, :, q] = mult * e[name] * _tap_scale(taps, r64["tap_valid"]) + sens[:, :, q]
    bar_dist = mult * e["dist"] * np.maximum(1.0, np.where(np.isfinite(r64["dist"]), r64["dist"], 1.0)) + sens[:, :, 0] + sens[:, :, 1]
    dscale = np.maximum(1.0, np.maximum(np.abs(r64["ref_depth"][:, None]), np.abs(r64["reproj_xyd"][:, :, 2])))
    bar_dep = mult * e["dep"] * dscale + (1.0 + depth_thresh) * sens[:, :, 2]
    dec = dict(clamp=r64["m_clamp"] > mult * e["warp"], range=r64["m_range"] > mult * e["warp"], cell=r64["m_cell"] > delta,
               dist=r64["m_dist"] > bar_dist, dep=r64["m_dep"] > bar_dep)
    # masks = min(in_range, dist test, depth test): a test that decidedly fails settles the mask whatever the others say (a reference
    # depth of 0 whose taps all fall outside compares 0 < 0 in the depth test, margin 0, and is out of range all the same)
    fails = (dec["dist"] & ~(r64["dist"] < dist_thresh)) | (dec["dep"] & ~(r64["dep_lhs"] < r64["dep_rhs"]))
    view = dec["clamp"] & dec["range"] & ((r64["in_range"] == 0) | (dec["cell"] & (fails | (dec["dist"] & dec["dep"]))))
    pixel = (view & dec["cell"]).all(1)
    msum = r64["masks"].sum(1)
    tol_ave = (r64["masks"] * tol[:, :, 2]).sum(1) / (msum + 1.0) + mult * e["ave"] * np.maximum(1.0, np.abs(r64["ref_depth_ave"]))
    tol_pts = r64["point_slope"] * tol_ave[:, None] + mult * e["points"] * np.maximum(1.0, np.abs(r64["points"]))
    return dict(reproj_xyd=tol, ref_depth_ave=tol_ave, points=tol_pts, delta=delta, decisions=dec, range_decided=dec["clamp"] & dec["range"],
                blend_decided=dec["clamp"] & dec["cell"], view_decided=view, pixel_decided=pixel)


def static_ring(r64):
    """(view, pixel) pairs whose blend has one to three taps outside the source image"""
    nv = r64["tap_valid"].sum(2)
    return (nv >= 1) & (nv <= 3)


def static_exercise(r64, tol, mask_tv2, mask_tvV):
    """the exercise conditions of a static case on the float64 rule -> (dict of figures, list of the conditions missed).  A "view" is a
    source slot v over the whole batch: at 2x2 a single map has four pixels that share all four taps, so a planted zero empties it."""
    dv, dp = tol["view_decided"], tol["pixel_decided"]
    n, v, h, w = dv.shape
    ring, oor = static_ring(r64) & dv, (r64["in_range"] == 0) & dv
    clamped = ((np.abs(r64["warp_x"]) > 1.1) | (np.abs(r64["warp_y"]) > 1.1)) & dv
    zero_tap = ((r64["tap_depth"] == 0) & r64["tap_valid"]).any(2) & dv
    share = [(r64["masks"][:, s][dv[:, s]] > 0).mean() if dv[:, s].any() else 0.0 for s in range(v)]
    ring_all = static_ring(r64)
    f = dict(out_of_range=float(max(oor[b, s].mean() for b in range(n) for s in range(v))),
             ring=float(max(ring[b, s].mean() for b in range(n) for s in range(v))), clamped=int(clamped.sum()),
             zero_tap=float(zero_tap.mean()), ref_zero=int(((r64["ref_depth"] == 0) & dp).sum()), ref_negative=int(((r64["ref_depth"] < 0) & dp).sum()),
             mask_share=[float(x) for x in share], mask_tv_differs=int(((mask_tv2 != mask_tvV) & dp).sum()),
             undecided_view=float(1 - dv.mean()), undecided_pixel=float(1 - dp.mean()),
             undecided_range=float(1 - tol["range_decided"].mean()),
             undecided_ring=float(max(((ring_all[b, s] & ~dv[b, s]).sum() / max(ring_all[b, s].sum(), 1)) for b in range(n) for s in range(v))))
    miss = []
    if f["out_of_range"] < 0.05: miss.append("out_of_range")
    if f["ring"] < 0.01: miss.append("ring")
    if f["clamped"] < 1: miss.append("clamped")
    if f["zero_tap"] < 0.01: miss.append("zero_tap")
    if f["ref_zero"] < 1: miss.append("ref_zero")
    if f["ref_negative"] < 1: miss.append("ref_negative")
    if not all(0.02 <= x <= 0.98 for x in share): miss.append("mask_share")
    if v != 2 and f["mask_tv_differs"] < 1: miss.append("mask_tv_differs")      # at V = 2 the two settings are one
    if max(f["undecided_view"], f["undecided_pixel"], f["undecided_range"]) > UNDECIDED_CAP: miss.append("undecided_cap")
    if f["undecided_ring"] > RING_CAP: miss.append("ring_cap")
    return f, miss


# ------------------------------------------------------------------------------------------------------------ dynamic filter
def dynamic_vis(ref_depth, reproj_xyd, dist_base=4, rel_diff_base=1300, dtype=np.float64):
    """vis_filter_dynamic (fusion.py:153-165) + the reduction of test.py:494-514 on a materialised reproj_xyd [n,v,3,h,w]"""
    T = dtype
    rd, rep = np.asarray(ref_depth).astype(T), np.asarray(reproj_xyd).astype(T)
    n, v, _, h, w = rep.shape
    xs, ys = _grid(h, w, T)
    levels = np.arange(2, v + 1)
    with np.errstate(all="ignore"):
        dx, dy = rep[:, :, 0] - xs, rep[:, :, 1] - ys
        cd = np.sqrt(dx * dx + dy * dy)
        d = rep[:, :, 2]
        dd = np.abs(rd[:, None] - d) / rd[:, None]
        t_cd = (levels.astype(T) / T(dist_base)).reshape(1, 1, -1, 1, 1)
        t_dd = (levels.astype(T) / T(rel_diff_base)).reshape(1, 1, -1, 1, 1)
        masks = (cd[:, :, None] < t_cd) & (dd[:, :, None] < t_dd)                       # [n,v,v-1,h,w]
        m_cd, m_dd = np.abs(cd[:, :, None] - t_cd), np.abs(dd[:, :, None] - t_dd)
        vis = masks[:, :, -1]
        kmin = np.where(masks.any(2), 2 + np.argmax(masks, 2), v + 1)
        sums, vsum = masks.sum(1), vis.sum(1)
        ave = (np.where(vis, d, T(0)).sum(1) + rd) / (vsum.astype(T) + T(1))
        geo = np.zeros((n, h, w), bool)
        for k in range(2, v + 1):
            geo |= sums[:, k - 2] >= k
    inf = T(np.inf)
    return dict(cd=cd, dd=dd, t_cd=t_cd, t_dd=t_dd, masks=masks, vis_mask=vis, kmin=kmin, level_count=sums, geo_mask=geo, ref_depth_ave=ave,
                m_cd=np.where(np.isfinite(m_cd), m_cd, inf), m_dd=np.where(np.isfinite(m_dd), m_dd, inf))


def _dyn_back(src, ref, qx, qy, ds, T):
    c = _a_to_b(src, ref, qx, qy, ds, T)
    x, y = _cam2img(ref.K, c, T)
    return np.stack([x, y, c[2]])


def dynamic_rule(case, dist_base=4, rel_diff_base=1300, dtype=np.float64, index_step=0.0):
    """``index_step`` > 0 also returns ``reproj_sens``: the change of reproj_xyd when the sample index moves by that much in x and y"""
    T = dtype
    rd, sd, rcam, scam = _unpack(case, T)
    n, v, h, w = sd.shape
    xs, ys = _grid(h, w, T)
    o = {k: np.zeros((n, v, h, w), T) for k in ("qx", "qy", "ix", "iy", "src_depth", "m_cell", "depth_slope")}
    o.update(reproj_xyd=np.zeros((n, v, 3, h, w), T), reproj_sens=np.zeros((n, v, 3, h, w), T), tap_valid=np.zeros((n, v, 4, h, w), bool),
             tap_depth=np.zeros((n, v, 4, h, w), T), tap_x=np.zeros((n, v, 4, h, w), np.int64), tap_y=np.zeros((n, v, 4, h, w), np.int64))
    pts, slope = np.zeros((n, 3, h, w), T), np.zeros((n, 3, h, w), T)
    with np.errstate(all="ignore"):
        for b in range(n):
            ref = _Cams(rcam[b], T)
            for s in range(v):
                src = _Cams(scam[b, s], T)
                qx, qy = _cam2img(src.K, _a_to_b(ref, src, xs, ys, rd[b], T), T)
                gx, gy = qx / (T(w - 1) / T(2)) - T(1), qy / (T(h - 1) / T(2)) - T(1)
                ix, iy = ((gx + T(1)) / T(2)) * T(w - 1), ((gy + T(1)) / T(2)) * T(h - 1)
                wts, valid, xi, yi = _cell(ix, iy, h, w, T)
                ds = np.zeros((h, w), T)
                for k in range(4):
                    tap = np.where(valid[k], sd[b, s][yi[k], xi[k]], T(0))
                    ds = ds + tap * np.where(valid[k], wts[k], T(0))
                    o["tap_depth"][b, s, k], o["tap_valid"][b, s, k], o["tap_x"][b, s, k], o["tap_y"][b, s, k] = tap, valid[k], xi[k], yi[k]
                ds = np.where(np.isfinite(ix) & np.isfinite(iy), ds, T(np.nan))
                rep = _dyn_back(src, ref, qx, qy, ds, T)
                o["depth_slope"][b, s] = _blend_slope(o["tap_depth"][b, s], o["tap_valid"][b, s])
                if index_step:
                    step = T(index_step) * np.maximum(T(1), np.maximum(np.abs(ix) / T(w), np.abs(iy) / T(h))) * o["depth_slope"][b, s]
                    o["reproj_sens"][b, s] = np.maximum(np.abs(_dyn_back(src, ref, qx, qy, ds + step, T) - rep),
                                                        np.abs(_dyn_back(src, ref, qx, qy, ds - step, T) - rep))
                o["qx"][b, s], o["qy"][b, s], o["ix"][b, s], o["iy"][b, s], o["src_depth"][b, s], o["reproj_xyd"][b, s] = qx, qy, ix, iy, ds, rep
                o["m_cell"][b, s] = _int_margin(ix, iy, h, w)
        o.update(dynamic_vis(rd, o["reproj_xyd"], dist_base, rel_diff_base, T))
        for b in range(n):
            pts[b], slope[b] = _points(_Cams(rcam[b], T), xs, ys, o["ref_depth_ave"][b], T)
    o.update(points=pts, point_slope=slope, ref_depth=rd)
    return o


def _index_scale(r):
    h, w = r["ix"].shape[-2:]
    with np.errstate(invalid="ignore"):
        s = np.maximum(1.0, np.maximum(np.abs(r["ix"]) / w, np.abs(r["iy"]) / h))
    return np.where(np.isfinite(s), s, 1.0)


def _dynamic_smooth(r):
    return r["tap_valid"].all(2) & (r["tap_depth"] > 0).all(2) & (r["ref_depth"][:, None] > 0)


def dynamic_bars(r64, r32):
    with np.errstate(all="ignore"):                 # dd is inf - inf at a reference depth of 0
        return _dynamic_bars(r64, r32)


def _dynamic_bars(r64, r32):
    allp = np.ones(r64["ix"].shape, bool)
    smooth = _dynamic_smooth(r64)
    e = {}
    e["index"] = max(_finite_max(np.abs(r32[a].astype(np.float64) - r64[a]) / _index_scale(r64), allp) for a in ("ix", "iy"))
    err = np.abs(r32["reproj_xyd"].astype(np.float64) - r64["reproj_xyd"])
    for q, name in enumerate(("x", "y", "d")):
        e[name] = _finite_max(err[:, :, q] / np.maximum(1.0, np.abs(r64["reproj_xyd"][:, :, q])), smooth)
    e["src_depth"] = _finite_max(np.abs(r32["src_depth"].astype(np.float64) - r64["src_depth"]) / np.maximum(1.0, np.abs(r64["src_depth"])), smooth)
    e["cd"] = _finite_max(np.abs(r32["cd"].astype(np.float64) - r64["cd"]) / np.maximum(1.0, r64["cd"]), smooth)
    e["dd"] = _finite_max(np.abs(r32["dd"].astype(np.float64) - r64["dd"]) / np.maximum(1.0, np.abs(r64["dd"])), smooth)
    same = (r32["masks"] == r64["masks"]).all((1, 2)) & (smooth | ~r64["vis_mask"]).all(1)
    e["ave"] = _finite_max(np.abs(r32["ref_depth_ave"].astype(np.float64) - r64["ref_depth_ave"]) / np.maximum(1.0, np.abs(r64["ref_depth_ave"])), same)
    e["points"] = _finite_max(np.abs(r32["points"].astype(np.float64) - r64["points"]) / np.maximum(1.0, np.abs(r64["points"])),
                              np.broadcast_to(same[:, None], r64["points"].shape))
    return {k: max(x, ULP) for k, x in e.items()}


def dynamic_tolerances(r64, e, mult=MULT):
    """``r64`` must come from ``dynamic_rule(..., index_step=mult * e["index"])``"""
    sens = np.where(np.isfinite(r64["reproj_sens"]), r64["reproj_sens"], np.inf)
    mag = np.where(np.isfinite(r64["reproj_xyd"]), np.abs(r64["reproj_xyd"]), 1.0)
    tol = np.stack([mult * e[name] * np.maximum(1.0, mag[:, :, q]) for q, name in enumerate(("x", "y", "d"))], 2) + sens
    bar_cd = mult * e["cd"] * np.maximum(1.0, np.where(np.isfinite(r64["cd"]), r64["cd"], 1.0)) + sens[:, :, 0] + sens[:, :, 1]
    with np.errstate(all="ignore"):
        bar_dd = mult * e["dd"] * np.maximum(1.0, np.where(np.isfinite(r64["dd"]), np.abs(r64["dd"]), 1.0)) + sens[:, :, 2] / np.abs(r64["ref_depth"][:, None])
    bar_dd = np.where(r64["ref_depth"][:, None] == 0, 0.0, np.where(np.isnan(bar_dd), np.inf, bar_dd))     # x / 0 is no number below any level
    cell = r64["m_cell"] > mult * e["index"] * _index_scale(r64)
    cd_k, dd_k = r64["m_cd"] > bar_cd[:, :, None], r64["m_dd"] > bar_dd[:, :, None]
    cd_fail, dd_fail = cd_k & ~(r64["cd"][:, :, None] < r64["t_cd"]), dd_k & ~(r64["dd"][:, :, None] < r64["t_dd"])
    level = cell[:, :, None] & (cd_fail | dd_fail | (cd_k & dd_k))                     # [n,v,v-1,h,w]: this level's mask entry is decided
    dec = dict(cell=cell, cd=cd_k.all(2), dd=dd_k.all(2), level=level)
    view = level.all(2)
    # the keep rule over intervals: with the undecided entries at 0 some level already has its k views, or with them at 1 none has
    ks = np.arange(2, level.shape[2] + 2).reshape(1, -1, 1, 1)
    lo, hi = (r64["masks"] & level).sum(1), (r64["masks"] | ~level).sum(1)
    geo = (lo >= ks).any(1) | (hi < ks).all(1)
    pixel = (level[:, :, -1] & cell).all(1)                                              # ref_depth_ave and points: every view's last level
    vsum = r64["vis_mask"].sum(1)
    tol_ave = np.where(r64["vis_mask"], tol[:, :, 2], 0.0).sum(1) / (vsum + 1.0) + mult * e["ave"] * np.maximum(1.0, np.abs(r64["ref_depth_ave"]))
    tol_pts = r64["point_slope"] * tol_ave[:, None] + mult * e["points"] * np.maximum(1.0, np.abs(r64["points"]))
    return dict(reproj_xyd=tol, ref_depth_ave=tol_ave, points=tol_pts, decisions=dec, blend_decided=cell, level_decided=level, view_decided=view,
                geo_decided=geo, pixel_decided=pixel)


def dynamic_exercise(r64, tol):
    dv, dp = tol["view_decided"], tol["pixel_decided"]
    n, v, h, w = dv.shape
    first = [float(((r64["kmin"] == k) & dv).mean()) for k in range(2, v + 1)]
    cnt = r64["level_count"]                                                          # [n,v-1,h,w]: views passing level k
    passes = np.stack([cnt[:, k - 2] >= k for k in range(2, v + 1)], 1)
    early_only = passes[:, :-1].any(1) & ~passes[:, -1] & tol["geo_decided"] & dv.all(1)
    rejected = ~r64["geo_mask"] & (cnt[:, -1] >= 2) & tol["geo_decided"] & dv.all(1)
    ring = r64["tap_valid"].any(2) & ~r64["tap_valid"].all(2)
    zero_tap = ((r64["tap_depth"] == 0) & r64["tap_valid"]).any(2) & dv
    f = dict(first_level=first, kept_early_only=int(early_only.sum()), rejected_with_two=int(rejected.sum()), kept=float((r64["geo_mask"] & tol["geo_decided"]).mean()),
             ring=float(max((ring & dv)[b, s].mean() for b in range(n) for s in range(v))), zero_tap=float(zero_tap.mean()),
             ref_zero=int(((r64["ref_depth"] == 0) & dp).sum()), ref_negative=int(((r64["ref_depth"] < 0) & dp).sum()),
             undecided_level=float(1 - tol["level_decided"].mean()), undecided_view=float(1 - tol["level_decided"][:, :, -1].mean()),
             undecided_geo=float(1 - tol["geo_decided"].mean()), undecided_pixel=float(1 - dp.mean()),
             undecided_ring=float(max(((ring[b, s] & ~dv[b, s]).sum() / max(ring[b, s].sum(), 1)) for b in range(n) for s in range(v))))
    miss = []
    if min(first) < 0.005: miss.append("first_level")
    if v > 2 and f["kept_early_only"] < 1: miss.append("kept_early_only")          # V = 2 has no level below the last
    if v > 2 and f["rejected_with_two"] < 1: miss.append("rejected_with_two")      # at V = 2 a count of 2 keeps the pixel
    if f["ring"] < 0.01: miss.append("ring")
    if f["zero_tap"] < 0.01: miss.append("zero_tap")
    if f["ref_zero"] < 1: miss.append("ref_zero")
    if f["ref_negative"] < 1: miss.append("ref_negative")
    if max(f["undecided_level"], f["undecided_view"], f["undecided_geo"], f["undecided_pixel"]) > UNDECIDED_CAP: miss.append("undecided_cap")
    if f["undecided_ring"] > RING_CAP: miss.append("ring_cap")
    return f, miss


# ------------------------------------------------------------------------------------------------------------ prob_filter
def prob_filter_rule(conf, thresh):
    """fusion.py:69-77: AND over the channels of conf[:, i] > thresh[i], float32 against float32 -> bool [n,1,...]"""
    conf = np.asarray(conf, np.float32)
    keep = np.ones((conf.shape[0], 1) + conf.shape[2:], bool)
    for i, t in enumerate(thresh):
        keep &= conf[:, i:i + 1] > np.float32(t)
    return keep


# ------------------------------------------------------------------------------------------------------------ scenes
def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def render_plane(E, K, h, w):
    """depth map of the scene plane (make_fusion_case's: n . X = 600 in the world frame) seen by the camera (E, K), float64"""
    xs, ys = _grid(h, w, np.float64)
    rays = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(K[:3, :3]).T
    R, t = E[:3, :3], E[:3, 3]
    nr = R @ _PLANE_N
    return (_PLANE_D + nr @ t) / (rays @ nr)


def make_edge_case(n, v, h, w, seed, noise=0.0004, ramp=None, shift=(0.37, 0.41), roll=0.15, behind=True, zero_frac=0.03, outlier_frac=0.05,
                   focal=1.0):
    """Cameras of ``make_fusion_case(n, v, h, w, seed)``, then:
      * sample 0, source 0 is rolled by ``roll`` rad and translated so its image moves by ``shift`` (fractions of w, h): reference
        pixels land outside it, on its outer half-pixel ring and beyond the +-1.1 clamp;
      * with ``behind`` (and n, v >= 2) sample 1's last source is turned by pi about its y axis: every reference point has z < 0 there;
      * depth maps are rendered from the plane in float64; source s gets relative noise ``noise * (1 + s)`` (Gaussian) or, with
        ``ramp`` = the dynamic filter's rel_diff_base, uniform noise of +-2 (s + 2.5) / ramp (the blend of four
        taps narrows it again): the first level a view passes rises with s;
      * ``focal`` multiplies every focal length and divides every translation: at 2x2 make_fusion_case's f = 1.1 w makes a pixel 45 % of
        the depth wide, where the sampling offset of project_img alone (0.25 px there) fails the depth test everywhere;
      * make_fusion_case sizes its vertical baselines for 3:4 images (a disparity of up to 0.07 w pixels); they are scaled by min(1, 2h/w), or
        at h = 3..9 next to w = 63..130 hardly any source view would overlap the reference;
      * ``outlier_frac`` gross outliers everywhere, ``zero_frac`` zeroed source depths (plus one planted in sample 0, source 0), a zero
        and a negative reference depth in every sample.
    -> float32 arrays ``ref_depth [n,1,h,w]``, ``src_depths [n,v,1,h,w]``, ``ref_cam [n,2,4,4]``, ``src_cams [n,v,2,4,4]``."""
    from oracle import ref_fusion
    base = ref_fusion.make_fusion_case(n=n, v=v, h=h, w=w, seed=seed, noise=0.0, outlier_frac=0.0)
    rcam, scam = base["ref_cam"].numpy().astype(np.float64), base["src_cams"].numpy().astype(np.float64)
    rng = np.random.default_rng(seed)
    for cam in (rcam, scam):                       # a longer lens on the same pixel disparities (see STATIC_CASES, 2x2)
        cam[..., 1, 0, 0] *= focal
        cam[..., 1, 1, 1] *= focal
        cam[..., 0, :3, 3] /= focal
        cam[..., 0, 1, 3] *= min(1.0, 2.0 * h / w)
    f = scam[0, 0, 1, 0, 0]
    E = scam[0, 0, 0]
    E[:3, :3] = _rot("z", roll) @ E[:3, :3]
    E[:3, 3] = _rot("z", roll) @ E[:3, 3] + np.array([shift[0] * w, shift[1] * h, 0.0]) * _PLANE_D / f
    if behind and n >= 2 and v >= 2:
        E = scam[1, v - 1, 0]
        E[:3] = _rot("y", np.pi) @ E[:3]
    rcam, scam = rcam.astype(np.float32), scam.astype(np.float32)          # the cameras every rule and kernel reads
    rd = np.stack([render_plane(rcam[b, 0].astype(np.float64), rcam[b, 1].astype(np.float64), h, w) for b in range(n)])
    sd = np.stack([np.stack([render_plane(scam[b, s, 0].astype(np.float64), scam[b, s, 1].astype(np.float64), h, w) for s in range(v)]) for b in range(n)])
    rd = rd * (1 + noise * rng.standard_normal(rd.shape))
    for s in range(v):
        if ramp:
            sd[:, s] *= 1 + 2.0 * (s + 2.5) / ramp * rng.uniform(-1, 1, sd[:, s].shape)
        else:
            sd[:, s] *= 1 + noise * (1 + s) * rng.standard_normal(sd[:, s].shape)
    u = rng.uniform(size=sd.shape)
    sd = np.where(u < outlier_frac, sd * (1 + 0.2 * rng.standard_normal(sd.shape)), sd)
    sd = np.where(u > 1 - zero_frac, 0.0, sd)
    ur = rng.uniform(size=rd.shape)
    rd = np.where(ur < outlier_frac, rd * (1 + 0.2 * rng.standard_normal(rd.shape)), rd)
    sd[0, 0, h // 2, w // 2] = 0.0
    for b in range(n):
        rd[b, h - 1, (b * 7) % w] = 0.0
        rd[b, 0, (w - 1 - b * 5) % w] = -rd[b, 0, (w - 1 - b * 5) % w]
    return dict(ref_depth=np.ascontiguousarray(rd[:, None], np.float32), src_depths=np.ascontiguousarray(sd[:, :, None], np.float32),
                ref_cam=np.ascontiguousarray(rcam), src_cams=np.ascontiguousarray(scam))


THRESHOLDS = {"A": (1.0, 0.01), "B": (0.25, 0.002)}
BASES = {"A": (4.0, 1300.0), "B": (1.0, 400.0)}
# name -> (h, w, n, v, thresholds / bases key, seed): every launch-tile shape, n in {1, 3}, V in {1, 2, 5} / {2, 5, 16}, both settings
STATIC_CASES = {"2x2": (2, 2, 3, 2, "A", 1), "3x63": (3, 63, 3, 2, "B", 2), "4x64": (4, 64, 1, 1, "A", 1), "5x65": (5, 65, 3, 5, "B", 2),
                "9x130": (9, 130, 1, 5, "A", 2), "17x20": (17, 20, 3, 5, "A", 1)}
DYNAMIC_CASES = {"2x2": (2, 2, 3, 2, "A", 2), "3x63": (3, 63, 1, 5, "B", 2), "4x64": (4, 64, 3, 16, "A", 2), "5x65": (5, 65, 3, 5, "B", 2),
                 "9x130": (9, 130, 1, 16, "B", 2), "17x20": (17, 20, 3, 2, "A", 2)}
_cache = {}


def static_case(name):
    """scene, float64 rule, bars and tolerances of a static case; built once and shared (read-only) by every test"""
    key = ("static", name)
    if key not in _cache:
        h, w, n, v, th, seed = STATIC_CASES[name]
        case = make_edge_case(n, v, h, w, seed, focal=8.0 if w == 2 else 1.0)
        dist, dep = THRESHOLDS[th]
        r64 = static_rule(case, dist, dep, 2, np.float64)
        r32 = static_rule(case, dist, dep, 2, np.float32)
        bars = static_bars(r64, r32)
        _cache[key] = dict(case=case, thresholds=(dist, dep), r64=r64, r32=r32, bars=bars, tol=static_tolerances(r64, bars, dist, dep))
    return _cache[key]


def dynamic_case(name):
    key = ("dynamic", name)
    if key not in _cache:
        h, w, n, v, th, seed = DYNAMIC_CASES[name]
        db, rb = BASES[th]
        case = make_edge_case(n, v, h, w, seed, ramp=rb, focal=8.0 if w == 2 else 1.0)
        r32 = dynamic_rule(case, db, rb, np.float32)
        bars = dynamic_bars(dynamic_rule(case, db, rb, np.float64), r32)
        r64 = dynamic_rule(case, db, rb, np.float64, index_step=MULT * bars["index"])
        _cache[key] = dict(case=case, bases=(db, rb), r64=r64, r32=r32, bars=bars, tol=dynamic_tolerances(r64, bars))
    return _cache[key]


def thres_view_mask(r64, thres_view):
    return r64["masks"].sum(1) >= thres_view - 1.1
