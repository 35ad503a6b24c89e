"""Depth-map geometric consistency filtering on the HIP path — the reference's ``misc/fusion.py`` interface.

Same function names and argument meaning as reference misc/fusion.py:69-114 (``prob_filter``, ``get_reproj``,
``vis_filter``, ``ave_fusion``) plus ``filter_depth_maps``: the whole block of test.py:425-434 (reprojection, masks,
averaged depth, fused world points) in ONE pass over the reference pixels with nothing materialized in between.

    ref_depth [n,1,h,w]   srcs_depth [n,v,1,h,w]   ref_cam [n,2,4,4]   srcs_cam [n,v,2,4,4]   (cam[:,0]=E, cam[:,1,:3,:3]=K)

``SceneFusion`` / ``fuse_scan`` are the whole of test.py:404-560 (``filter_depth`` / ``dynamic_filter_depth`` /
``pcd_filter_worker``): every view of a scan on the device once, all reference views filtered in one launch through a job
table, the surviving points and colours compacted on the device into the PLY vertex records.

``GipumaFusion`` / ``gipuma_fuse_scan`` stand where the reference's default ``--filter_method gipuma`` (misc/gipuma.py ``gipuma_filter``) shells
out to the external ``fusibile`` binary: sequential over the reference views, a disparity test against every other view, the consistent
views' 3-D points averaged (``mvs_gipuma_fuse_scene``; the rule is restated in include/mvs_hip.h, parity with the binary is unverified).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops


def prob_filter(ref_prob: torch.Tensor, prob_thresh: Sequence[float], greater: bool = True) -> torch.Tensor:
    """fusion.py:69-77 — ``ref_prob [n,C,...]`` -> bool ``[n,1,...]``."""
    return ops.prob_filter(ref_prob, prob_thresh)


def get_reproj(ref_depth, srcs_depth, ref_cam, srcs_cam):
    """fusion.py:80-98 -> ``(reproj_xyd [n,v,3,h,w], in_range [n,v,1,h,w])``."""
    out = ops.geo_filter(ref_depth, srcs_depth, ref_cam, srcs_cam, want=("reproj_xyd", "in_range"))
    return out["reproj_xyd"], out["in_range"]


def vis_filter(ref_depth, reproj_xyd, in_range, img_dist_thresh, depth_thresh, vthresh):
    """fusion.py:101-109 -> ``(masks [n,v,1,h,w] float, mask [n,1,h,w] bool)``."""
    masks, mask, _ = ops.vis_filter(ref_depth, reproj_xyd, in_range, None, img_dist_thresh, depth_thresh, vthresh, want_ave=False)
    return masks, mask


def ave_fusion(ref_depth, reproj_xyd, masks):
    """fusion.py:112-114 -> ``[n,1,h,w]``."""
    return ops.vis_filter(ref_depth, reproj_xyd, None, masks, 0.0, 0.0, 0.0, want_masks=False)[2]


def filter_depth_maps(ref_depth, srcs_depth, ref_cam, srcs_cam, thres_disp: float, depth_thresh: float = 0.01,
                      thres_view: float = 2, with_intermediates: bool = False) -> Dict[str, torch.Tensor]:
    """test.py:425-434 fused: ``mask`` (bool), ``ref_depth_ave``, ``points`` [n,3,h,w]; with ``with_intermediates`` also
    ``reproj_xyd``, ``in_range``, ``masks``."""
    want = ("mask", "ref_depth_ave", "points") + (("reproj_xyd", "in_range", "masks") if with_intermediates else ())
    return ops.geo_filter(ref_depth, srcs_depth, ref_cam, srcs_cam, thres_disp, depth_thresh, thres_view, want=want)


def get_reproj_dynamic(ref_depth, srcs_depth, ref_cam, srcs_cam):
    """fusion.py:116-150 -> ``reproj_xyd [n,v,3,h,w]``."""
    return ops.geo_filter_dynamic(ref_depth, srcs_depth, ref_cam, srcs_cam, want=("reproj_xyd",))["reproj_xyd"]


def vis_filter_dynamic(ref_depth, reproj_xyd, dist_base=4, rel_diff_base=1300):
    """fusion.py:153-165 -> ``(masks [n,v,v-1,h,w] bool, mask [n,v,1,h,w] bool)``."""
    out = ops.vis_filter_dynamic(ref_depth, reproj_xyd, dist_base, rel_diff_base)
    return out["masks"], out["vis_mask"]


def dynamic_filter_depth_maps(ref_depth, srcs_depth, ref_cam, srcs_cam, dist_base=4, rel_diff_base=1300,
                              with_intermediates: bool = False) -> Dict[str, torch.Tensor]:
    """test.py:494-514 fused: ``geo_mask`` (bool ``[n,1,h,w]``: some level k in 2..v is passed by at least k source views),
    ``ref_depth_ave`` (mean of the reference depth and the level-v consistent reprojections), ``points``; with
    ``with_intermediates`` also ``reproj_xyd``, ``masks``, ``vis_mask``.  (For n > 1 the reference's ``geo_mask`` broadcasts
    ``[n,1,h,w] | [n,h,w]`` to ``[n,n,h,w]``; this returns its per-sample diagonal meaning.)"""
    want = ("geo_mask", "ref_depth_ave", "points") + (("reproj_xyd", "masks", "vis_mask") if with_intermediates else ())
    return ops.geo_filter_dynamic(ref_depth, srcs_depth, ref_cam, srcs_cam, dist_base, rel_diff_base, want=want)


def filter_scan(pair_folder: str, scan_folder: str, prob_threshold: Sequence[float], method: str = "pcd", thres_disp: float = 1.0,
                thres_view: float = 2, dist_base: float = 4, rel_diff_base: float = 1300, n_src_views: int = 10,
                device: str = "cuda:0"):
    """The per-scan loop of test.py:404-438 (``method='pcd'``, ``filter_depth``) / test.py:475-514 (``'dypcd'``,
    ``dynamic_filter_depth``) over the folder layout ``data_io.save_depth_outputs`` writes: for every reference view of
    ``pair.txt`` load the depth/confidence/camera files, zero the prob-filtered source depths (pcd only, as in the
    reference), run the fused consistency pass, AND with the reference view's own prob mask, and gather the surviving world
    points.  Returns ``{ref_id: (points [M,3] float32 numpy, stats dict)}``; colours and the PLY are the caller's business.
    """
    import torch
    from . import data_io
    if method not in ("pcd", "dypcd"):
        raise ValueError("method must be 'pcd' or 'dypcd'")
    views = {}
    for id_ref, id_srcs in data_io.read_pair_file(pair_folder + "/pair.txt"):
        s = {k: (torch.from_numpy(v).unsqueeze(0).to(device) if hasattr(v, "shape") else v)
             for k, v in data_io.load_filter_sample(scan_folder, id_ref, id_srcs, n_src_views).items()}
        src_depths = s["src_depths"].contiguous()
        if method == "pcd":
            for i in range(src_depths.shape[1]):
                ops.prob_filter(s["src_confs"][:, i].contiguous(), prob_threshold, depth_inplace=src_depths[:, i])
            out = filter_depth_maps(s["ref_depth"], src_depths, s["ref_cam"], s["src_cams"], thres_disp, 0.01, thres_view)
            geo = out["mask"]
        else:
            out = dynamic_filter_depth_maps(s["ref_depth"], src_depths, s["ref_cam"], s["src_cams"], dist_base, rel_diff_base)
            geo = out["geo_mask"]
        prob = prob_filter(s["ref_conf"].contiguous(), prob_threshold)
        keep = prob & geo
        pts = out["points"][0].permute(1, 2, 0)[keep[0, 0]]
        views[id_ref] = (pts.cpu().numpy(), dict(photo=prob.float().mean().item(), geo=geo.float().mean().item(),
                                                 final=keep.float().mean().item()))
    return views


class SceneFusion:
    """A scan held on the device: ``add_view`` once per view (tensors straight from ``DINOMVSNet``'s outputs, or numpy), ``set_pairs``
    with the view graph, ``fuse()`` -> the coloured point cloud of test.py:404-472 (``method='pcd'``) / :475-549 (``'dypcd'``).

    ``depth [H,W]`` (leading singleton dims allowed), ``conf [C,H,W]`` (``[H,W]`` = one channel), ``cam [2,4,4]``, ``img [3,H,W]`` uint8 or
    float32 in [0,1] (all views or none; without images the colours are 0).  ``prob_threshold``: one threshold per confidence channel;
    with ``combine_conf`` only ``prob_threshold[0]`` on channel 0 (test.py:415-422).  All views share H x W.
    """

    def __init__(self, method: str = "pcd", prob_threshold: Sequence[float] = (0.5,), thres_disp: float = 1.0, thres_view: float = 2,
                 dist_base: float = 4, rel_diff_base: float = 1300, combine_conf: bool = False, device: Optional[str] = None):
        if method not in ("pcd", "dypcd"):
            raise ValueError("method must be 'pcd' or 'dypcd'")
        self.method, self.combine_conf = method, bool(combine_conf)
        self.prob_threshold = [float(p) for p in prob_threshold]
        if not 1 <= len(self.prob_threshold) <= 4:
            raise ValueError("prob_threshold: 1..4 values, one per confidence channel")
        self.thres_disp, self.thres_view, self.dist_base, self.rel_diff_base = thres_disp, thres_view, dist_base, rel_diff_base
        self.device = torch.device(device) if device is not None else None
        if self.device is not None and self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.views: Dict[int, Tuple[torch.Tensor, torch.Tensor, torch.Tensor, Optional[torch.Tensor]]] = {}
        self.pairs: List[Tuple[int, List[int]]] = []
        self.hw: Optional[Tuple[int, int]] = None

    def _dev(self, a, name: str, dtypes) -> torch.Tensor:
        from ._lib import MvsHipError
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise MvsHipError("%s must be a GPU tensor or a numpy array: the MI355X HIP path is the only implementation (no CPU "
                                  "fallback)" % name)
            if self.device is None:
                self.device = a.device
        else:
            if self.device is None:
                self.device = torch.device("cuda:0")
            a = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        if a.device != self.device:
            raise MvsHipError("%s lives on %s, the scene on %s" % (name, a.device, self.device))
        if a.dtype not in dtypes:
            raise MvsHipError("%s must be %s, got %s" % (name, " or ".join(str(d) for d in dtypes), a.dtype))
        return a

    def add_view(self, view_id: int, depth, conf, cam, img=None) -> None:
        from ._lib import MvsHipError
        depth = self._dev(depth, "depth", (torch.float32,))
        conf = self._dev(conf, "conf", (torch.float32,))
        cam = self._dev(cam, "cam", (torch.float32,))
        if depth.dim() < 2 or depth.numel() != depth.shape[-1] * depth.shape[-2]:
            raise MvsHipError("depth must be [H,W] (leading singleton dimensions allowed), got %s" % (tuple(depth.shape),))
        h, w = depth.shape[-2:]
        depth = depth.reshape(h, w)
        if conf.dim() == 4 and conf.shape[0] == 1:
            conf = conf[0]
        if conf.dim() == 2:
            conf = conf[None]
        cam = cam.reshape(2, 4, 4) if cam.numel() == 32 else cam
        if conf.dim() != 3 or tuple(conf.shape[1:]) != (h, w) or tuple(cam.shape) != (2, 4, 4):
            raise MvsHipError("view %d: depth %s, conf %s, cam %s do not fit together" % (view_id, (h, w), tuple(conf.shape), tuple(cam.shape)))
        if img is not None:
            img = self._dev(img, "img", (torch.uint8, torch.float32))
            if img.dim() == 4 and img.shape[0] == 1:
                img = img[0]
            if tuple(img.shape) != (3, h, w):
                raise MvsHipError("view %d: img must be [3,%d,%d], got %s" % (view_id, h, w, tuple(img.shape)))
        if self.hw is None:
            self.hw = (h, w)
        if (h, w) != self.hw:
            raise MvsHipError("view %d is %dx%d, the scene %dx%d: all views of a scene share H x W" % (view_id, h, w, *self.hw))
        self.views[int(view_id)] = (depth, conf, cam, img)

    def set_pairs(self, pairs) -> None:
        """``[(ref_id, [src_id, ...])]`` in output order (``data_io.read_pair_file`` / ``load_scene()['pairs']``)."""
        self.pairs = [(int(r), [int(v) for v in srcs]) for r, srcs in pairs]

    @classmethod
    def from_folder(cls, pair_folder: str, scan_folder: str, n_src_views: int = 10, **kwargs) -> "SceneFusion":
        from . import data_io
        scene = data_io.load_scene(pair_folder, scan_folder, n_src_views)
        self = cls(**kwargs)
        for i, vid in enumerate(scene["view_ids"]):
            self.add_view(vid, scene["depths"][i], scene["confs"][i], scene["cams"][i], None if scene["imgs"] is None else scene["imgs"][i])
        self.set_pairs(scene["pairs"])
        return self

    def fuse(self, want: Sequence[str] = ("records", "xyz", "rgb"), with_intermediates: bool = False,
             on_device: bool = False) -> Dict[str, object]:
        """-> ``xyz [M,3]`` float32, ``rgb [M,3]`` uint8, ``records`` uint8 ``[M*15]`` (the PLY vertex body) as numpy arrays (those named
        in ``want``), ``counts_per_view {ref_id: points}``, ``stats {ref_id: {photo, geo, final}}`` (fractions of the view's pixels), and
        ``n_points``.  Points come in ``pairs`` order, row-major inside a view, as the reference concatenates them.  With
        ``with_intermediates`` also the device tensors the compaction read: ``photo_mask [Nv,H,W]`` (views in ``view_ids`` order),
        ``geo_mask [R,H,W]`` and ``points_dense [R,3,H,W]`` (one per pair).  ``on_device``: the arrays named in ``want`` stay device
        tensors (no copy to the host) - ``xyz`` is then what ``cloud_eval.evaluate`` takes as ``pred_xyz``."""
        from ._lib import MvsHipError
        if not self.pairs or not self.views:
            raise ValueError("SceneFusion.fuse: add_view() and set_pairs() first")
        ids = list(self.views)
        index = {v: i for i, v in enumerate(ids)}
        for r, srcs in self.pairs:
            for v in [r] + srcs:
                if v not in index:
                    raise ValueError("view %d is named in the pairs but was never added" % v)
            if not srcs:
                raise ValueError("reference view %d has no source views" % r)
            if self.method == "dypcd" and not 2 <= len(srcs) <= 16:
                raise MvsHipError("reference view %d has %d source views: the dynamic check takes 2..16" % (r, len(srcs)))
        imgs = [v[3] for v in self.views.values()]
        if any(i is None for i in imgs) and not all(i is None for i in imgs):
            raise ValueError("either every view has an image or none")
        if imgs[0] is not None and len({i.dtype for i in imgs}) != 1:
            raise ValueError("images must be all uint8 or all float32")
        nch = 1 if self.combine_conf else len(self.prob_threshold)
        if any(v[1].shape[0] < nch for v in self.views.values()):
            raise MvsHipError("%d thresholds but a view has fewer confidence channels" % nch)
        with torch.cuda.device(self.device):
            depths = torch.stack([v[0] for v in self.views.values()]).contiguous()
            confs = torch.stack([v[1][:nch] for v in self.views.values()]).contiguous()
            cams = torch.stack([v[2] for v in self.views.values()]).contiguous()
            images = None if imgs[0] is None else torch.stack(imgs).contiguous()
            table = ops.JobTable([(index[r], [index[v] for v in srcs]) for r, srcs in self.pairs], len(ids), self.device)
            # ONE prob-filter launch for the scene: every view's photometric mask, and (pcd) the zeroed copy it contributes as a source
            depth_src = depths.clone() if self.method == "pcd" else depths
            photo = ops.prob_filter(confs, self.prob_threshold[:nch], depth_inplace=depth_src if self.method == "pcd" else None)
            if self.method == "pcd":
                out = ops.geo_filter_scene(table, depths, depth_src, cams, self.thres_disp, 0.01, self.thres_view, want=("mask", "points"))
                geo = out["mask"]
            else:
                out = ops.geo_filter_dynamic_scene(table, depths, depth_src, cams, self.dist_base, self.rel_diff_base,
                                                   want=("geo_mask", "points"))
                geo = out["geo_mask"]
            comp = ops.pointcloud_compact(table, photo.view(len(ids), *self.hw), geo, out["points"], images, want=tuple(want))
            res: Dict[str, object] = {k: comp[k] if on_device else comp[k].cpu().numpy() for k in want}
        if with_intermediates:
            res.update(photo_mask=photo.view(len(ids), *self.hw), geo_mask=geo, points_dense=out["points"], view_ids=ids)
        hw = float(self.hw[0] * self.hw[1])
        st = comp["stats"]
        res["n_points"] = comp["total"]
        res["counts_per_view"] = {r: int(st[i, 2]) for i, (r, _) in enumerate(self.pairs)}
        res["stats"] = {r: dict(photo=st[i, 0] / hw, geo=st[i, 1] / hw, final=st[i, 2] / hw) for i, (r, _) in enumerate(self.pairs)}
        return res


def fuse_scan(pair_folder: str, scan_folder: str, plyfilename: str, prob_threshold: Sequence[float], method: str = "pcd",
              thres_disp: float = 1.0, thres_view: float = 2, dist_base: float = 4, rel_diff_base: float = 1300,
              combine_conf: bool = False, n_src_views: int = 10, device: str = "cuda:0") -> Dict[str, object]:
    """``pcd_filter_worker`` (test.py:552-560): the scan folder ``save_depth_outputs`` (+ ``images/``) left -> ``plyfilename``.
    Returns ``n_points``, ``stats``, ``counts_per_view`` and ``seconds`` = {load, device, write}."""
    import time
    from . import data_io
    t0 = time.perf_counter()
    scene = SceneFusion.from_folder(pair_folder, scan_folder, n_src_views, method=method, prob_threshold=prob_threshold,
                                    thres_disp=thres_disp, thres_view=thres_view, dist_base=dist_base, rel_diff_base=rel_diff_base,
                                    combine_conf=combine_conf, device=device)
    torch.cuda.synchronize(scene.device)
    t1 = time.perf_counter()
    out = scene.fuse(want=("records",))
    t2 = time.perf_counter()
    data_io.write_ply_records(plyfilename, out["records"], out["n_points"])
    t3 = time.perf_counter()
    return dict(n_points=out["n_points"], stats=out["stats"], counts_per_view=out["counts_per_view"],
                seconds=dict(load=t1 - t0, device=t2 - t1, write=t3 - t2))


def gipuma_tables(cams) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The per-view and per-pair tables of ``mvs_gipuma_fuse_scene`` from ``cams [Nv,2,4,4]`` (numpy or tensor), computed in float64 on the
    host and rounded once to float32: ``B [Nv,3,3] = R^T K^-1``, ``c [Nv,3] = -R^T t``, ``A [Nv,Nv,3,3]`` with ``A[r,s] = P_s[:, :3] B_r``,
    ``b [Nv,Nv,3]`` with ``b[r,s] = P_s[:, :3] c_r + P_s[:, 3]`` (``P_s = K_s [R_s | t_s]``) and ``fb [Nv,Nv] = K_r[0,0] |c_r - c_s|``."""
    cams = np.asarray(cams.detach().cpu() if isinstance(cams, torch.Tensor) else cams, dtype=np.float64)
    if cams.ndim != 4 or cams.shape[1:] != (2, 4, 4):
        raise ValueError("gipuma_tables: cams must be [Nv,2,4,4], got %s" % (cams.shape,))
    R, t, K = cams[:, 0, :3, :3], cams[:, 0, :3, 3], cams[:, 1, :3, :3]
    Rt = R.transpose(0, 2, 1)
    B = Rt @ np.linalg.inv(K)
    c = -(Rt @ t[:, :, None])[:, :, 0]
    M = K @ R                                                           # P_s[:, :3]
    p3 = (K @ t[:, :, None])[:, :, 0]                                   # P_s[:, 3]
    A = np.einsum("sij,rjk->rsik", M, B)
    b = np.einsum("sij,rj->rsi", M, c) + p3[None]
    fb = K[:, 0, 0][:, None] * np.linalg.norm(c[:, None] - c[None], axis=-1)
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in (B, c, A, b, fb))


class GipumaFusion(SceneFusion):
    """The scan-resident form of the reference's default filter (``gipuma_filter`` -> ``fusibile``): the surface of ``SceneFusion``
    (``add_view`` / ``set_pairs`` / ``from_folder`` / ``fuse``, the same return dictionary), the rule of ``mvs_gipuma_fuse_scene``.

    Views are processed in ``pairs`` order, each against its listed sources; ``pairs=None`` (``set_pairs`` never called): ascending view
    id, each against every other view, as ``gipuma_filter`` walks its sorted file names.  ``prob_threshold`` / ``combine_conf`` zero the
    depth of the pixels that fail (``probability_filter``, misc/gipuma.py:160-189) before any view is fused.  A point takes the colour
    of its reference pixel; there are no normals."""

    def __init__(self, prob_threshold: Sequence[float] = (0.5,), disp_threshold: float = 0.2, num_consistent: float = 3,
                 depth_min: float = 0.001, depth_max: float = 100000.0, combine_conf: bool = False, device: Optional[str] = None):
        super().__init__("pcd", prob_threshold, combine_conf=combine_conf, device=device)
        if not depth_min >= 0.0:
            raise ValueError("depth_min must be >= 0: a pixel zeroed by the probability filter has to stay ineligible")
        self.method = "gipuma"
        self.disp_threshold, self.num_consistent, self.depth_min, self.depth_max = disp_threshold, num_consistent, depth_min, depth_max

    def set_pairs(self, pairs) -> None:
        """``[(ref_id, [src_id, ...])]`` in processing order; ``None``: every view against all others, ascending id."""
        self.pairs = [] if pairs is None else [(int(r), [int(v) for v in srcs]) for r, srcs in pairs]

    @classmethod
    def from_folder(cls, pair_folder: str, scan_folder: str, n_src_views: int = 10, **kwargs) -> "GipumaFusion":
        """Every view of the scan folder that ``pair.txt`` names, in ascending id, each against all others (``n_src_views`` only bounds
        which views the loader reads; the pair lists themselves are not used)."""
        from . import data_io
        scene = data_io.load_scene(pair_folder, scan_folder, n_src_views)
        self = cls(**kwargs)
        for i in sorted(range(len(scene["view_ids"])), key=lambda i: scene["view_ids"][i]):
            self.add_view(scene["view_ids"][i], scene["depths"][i], scene["confs"][i], scene["cams"][i],
                          None if scene["imgs"] is None else scene["imgs"][i])
        return self

    def fuse(self, want: Sequence[str] = ("records", "xyz", "rgb"), with_intermediates: bool = False,
             on_device: bool = False) -> Dict[str, object]:
        """As ``SceneFusion.fuse``.  ``stats``: ``photo`` = pixels passing the probability filter, ``geo`` = pixels kept by the rule,
        ``final`` = both (= ``geo``: a filtered pixel has depth 0 and is never eligible).  ``with_intermediates`` adds ``photo_mask
        [Nv,H,W]``, ``geo_mask [R,H,W]``, ``points_dense [R,3,H,W]``, ``used [Nv,H,W]``, ``count [R,H,W]`` and ``view_ids``."""
        from ._lib import MvsHipError
        if len(self.views) < 2:
            raise ValueError("GipumaFusion.fuse: add_view() at least two views first")
        ids = list(self.views)
        index = {v: i for i, v in enumerate(ids)}
        pairs = self.pairs or [(r, [v for v in sorted(ids) if v != r]) for r in sorted(ids)]
        for r, srcs in pairs:
            for v in [r] + srcs:
                if v not in index:
                    raise ValueError("view %d is named in the pairs but was never added" % v)
            if not srcs:
                raise ValueError("reference view %d has no source views" % r)
        imgs = [v[3] for v in self.views.values()]
        if any(i is None for i in imgs) and not all(i is None for i in imgs):
            raise ValueError("either every view has an image or none")
        if imgs[0] is not None and len({i.dtype for i in imgs}) != 1:
            raise ValueError("images must be all uint8 or all float32")
        nch = 1 if self.combine_conf else len(self.prob_threshold)
        if any(v[1].shape[0] < nch for v in self.views.values()):
            raise MvsHipError("%d thresholds but a view has fewer confidence channels" % nch)
        with torch.cuda.device(self.device):
            depths = torch.stack([v[0] for v in self.views.values()]).contiguous()             # a copy: zeroed in place below
            confs = torch.stack([v[1][:nch] for v in self.views.values()]).contiguous()
            cams = torch.stack([v[2] for v in self.views.values()])
            images = None if imgs[0] is None else torch.stack(imgs).contiguous()
            tables = tuple(torch.from_numpy(t).to(self.device) for t in gipuma_tables(cams))
            table = ops.JobTable([(index[r], [index[v] for v in srcs]) for r, srcs in pairs], len(ids), self.device)
            photo = ops.prob_filter(confs, self.prob_threshold[:nch], depth_inplace=depths).view(len(ids), *self.hw)
            out = ops.gipuma_fuse_scene(depths, tables, table, self.disp_threshold, self.num_consistent, self.depth_min, self.depth_max,
                                        want_count=with_intermediates)
            comp = ops.pointcloud_compact(table, photo, out["keep"], out["points"], images, want=tuple(want))
            res: Dict[str, object] = {k: comp[k] if on_device else comp[k].cpu().numpy() for k in want}
        if with_intermediates:
            res.update(photo_mask=photo, geo_mask=out["keep"], points_dense=out["points"], used=out["used"], count=out["count"], view_ids=ids)
        hw = float(self.hw[0] * self.hw[1])
        st = comp["stats"]
        res["n_points"] = comp["total"]
        res["counts_per_view"] = {r: int(st[i, 2]) for i, (r, _) in enumerate(pairs)}
        res["stats"] = {r: dict(photo=st[i, 0] / hw, geo=st[i, 1] / hw, final=st[i, 2] / hw) for i, (r, _) in enumerate(pairs)}
        return res


def gipuma_fuse_scan(pair_folder: str, scan_folder: str, plyfilename: str, prob_threshold: Sequence[float], disp_threshold: float = 0.2,
                     num_consistent: float = 3, depth_min: float = 0.001, depth_max: float = 100000.0, combine_conf: bool = False,
                     n_src_views: int = 10, device: str = "cuda:0") -> Dict[str, object]:
    """``gipuma_filter`` (misc/gipuma.py:192-228) without the .dmb round trip and the external binary: the scan folder
    ``save_depth_outputs`` (+ ``images/``) left -> ``plyfilename``.  Returns what ``fuse_scan`` returns."""
    import time
    from . import data_io
    t0 = time.perf_counter()
    scene = GipumaFusion.from_folder(pair_folder, scan_folder, n_src_views, prob_threshold=prob_threshold, disp_threshold=disp_threshold,
                                     num_consistent=num_consistent, depth_min=depth_min, depth_max=depth_max, combine_conf=combine_conf,
                                     device=device)
    torch.cuda.synchronize(scene.device)
    t1 = time.perf_counter()
    out = scene.fuse(want=("records",))
    t2 = time.perf_counter()
    data_io.write_ply_records(plyfilename, out["records"], out["n_points"])
    t3 = time.perf_counter()
    return dict(n_points=out["n_points"], stats=out["stats"], counts_per_view=out["counts_per_view"],
                seconds=dict(load=t1 - t0, device=t2 - t1, write=t3 - t2))
