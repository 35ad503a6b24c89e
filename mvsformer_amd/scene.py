"""Scene-resident depth inference: every image of a scan goes through the FPN and the ViT ONCE.

``test.py`` evaluates a scan of N images as N samples of V views, so the 2-D networks run N*V times on N distinct images.  In eval mode a
view's feature maps do not depend on the sample it appears in (BatchNorm uses running statistics, ``general_eval.py`` prepares an image
the same way in every group), so :class:`SceneInference` keeps them in a feature BANK - four tensors ``[cap,H/s,W/s,C_s]`` channel-last,
written by ``DINOMVSNet.extract_features`` - and runs the cascade over the bank through a view table (``CascadeMVS.forward_bank``,
``ops.cv_*_views``).  :func:`plan` decides, on the host, which image is extracted into which slot before which sample.

images -> feature bank -> depth and confidence maps -> (``fusion.SceneFusion``) point cloud, all on the device; the reference's round trip
through ``.pfm`` / ``.npy`` files is optional (``save_to``).
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from . import ops, synth
from ._lib import MvsHipError

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # general_eval.py:31, the normalisation DINOMVSNet's inputs carry
IMAGENET_STD = (0.229, 0.224, 0.225)


def plan(pairs, num_views: int, capacity: Optional[int] = None, view_ids: Optional[Iterable[int]] = None, extract_batch: int = 1) -> List[dict]:
    """Host-side schedule of a scan.  ``pairs``: ``[(ref_id, [src_id, ...])]`` in ``pair.txt`` order; a sample is the reference view and its
    first ``num_views - 1`` sources.  ``capacity``: slots of the bank (``None``: one per distinct view).  ``view_ids``: the images that
    exist (``None``: not checked).  -> one step per reference view, in order::

        {"ref": ref_id, "views": [ref_id, src_id, ...], "extract": [(view_id, slot), ...], "table": [slot of each view]}

    ``extract`` is what has to be written into the bank BEFORE the step's sample runs; afterwards ``table`` names slots that hold exactly
    the sample's views.  A view is extracted when first needed and stays until its slot is taken: eviction is least-recently-used over
    the pair order and never touches a view of the current sample, so an evicted view is extracted again when next needed and no view is
    extracted twice for one sample.  With ``extract_batch > 1`` a step that has to extract anyway also extracts the views the FOLLOWING
    samples will need, into slots that are still free (never by evicting), until its batch is full: the 2-D networks then run on
    ``extract_batch`` images at a time."""
    if num_views < 2:
        raise ValueError("num_views must be at least 2 (a reference view and one source)")
    if extract_batch < 1:
        raise ValueError("extract_batch must be at least 1")
    known = None if view_ids is None else {int(v) for v in view_ids}
    samples: List[Tuple[int, List[int]]] = []
    for ref, srcs in pairs:
        views = [int(ref)] + [int(v) for v in list(srcs)[:num_views - 1]]
        if len(views) < 2:
            raise ValueError("reference view %d has no source views" % ref)
        if known is not None:
            for v in views:
                if v not in known:
                    raise ValueError("view %d is named by the pairs of reference view %d but is not among the images" % (v, int(ref)))
        samples.append((int(ref), views))
    distinct = {v for _, views in samples for v in views}
    if capacity is None:
        capacity = len(distinct)
    need = max((len(set(views)) for _, views in samples), default=1)
    if capacity < need:
        raise ValueError("capacity %d is smaller than the %d views of one sample" % (capacity, need))
    slot_of: Dict[int, int] = {}                            # resident view -> slot
    last_use: Dict[int, int] = {}                           # resident view -> step that last used (or prefetched) it
    free = list(range(capacity))
    steps: List[dict] = []
    for t, (ref, views) in enumerate(samples):
        extract: List[Tuple[int, int]] = []
        current = set(views)
        for v in views:
            if v in slot_of:
                continue
            if free:
                slot = free.pop(0)
            else:
                victim = min((u for u in slot_of if u not in current), key=lambda u: (last_use[u], slot_of[u]))
                slot = slot_of.pop(victim)
                del last_use[victim]
            slot_of[v] = slot
            extract.append((v, slot))
        for v in views:
            last_use[v] = t
        if extract and extract_batch > 1:                   # fill the batch with what the following samples need, free slots only
            for _, later in samples[t + 1:]:
                if not free or len(extract) >= extract_batch:
                    break
                for v in later:
                    if v not in slot_of and free and len(extract) < extract_batch:
                        slot_of[v] = free.pop(0)
                        last_use[v] = t
                        extract.append((v, slot_of[v]))
        steps.append({"ref": ref, "views": list(views), "extract": extract, "table": [slot_of[v] for v in views]})
    return steps


def stage_cams(cam: torch.Tensor, scales: Sequence[int] = synth.STAGE_SCALES) -> List[torch.Tensor]:
    """``cam [2,4,4]`` (extrinsic, full-resolution intrinsic) -> the per-stage ``[2,4,4]`` blocks of ``proj_matrices['stageK']``: the same
    extrinsic, the intrinsic's first two rows divided by the stage's scale (``synth.stage_intrinsics``, as ``general_eval.py`` does)."""
    out = []
    for s in scales:
        c = cam.clone()
        c[1, :3, :3] = synth.stage_intrinsics(cam[1, :3, :3], s)
        out.append(c)
    return out


class SceneInference:
    """A scan held on the device, images -> depth and confidence maps with every image through the 2-D networks once::

        si = SceneInference(model)                          # DINOMVSNet in eval() on the GPU
        si.add_image(view_id, img, cam, depth_range)        # img [3,H,W] float32, normalised as the model expects; cam [2,4,4]
        si.set_pairs(pairs, num_views=5)                    # data_io.read_pair_file order; first num_views - 1 sources
        out = si.run(tmp=[5., 5., 5., 1.], fusion=None)     # {ref_id: {"depth", "confidence", "cam"}} as device tensors

    ``capacity_views``: slots of the feature bank; the default is the whole scan when its bank fits ``max_bank_mb``, else as many views as
    fit (at least the views of one sample; :func:`plan` evicts least-recently-used).  ``extract_batch``: images per pass of the 2-D
    networks.  ``combine_conf``: keep only the stage-averaged confidence ``[H,W]`` the cascade produces instead of the four stage
    confidences ``[4,H,W]`` (test.py:289-292)."""

    def __init__(self, model, capacity_views: Optional[int] = None, max_bank_mb: float = 16384.0, extract_batch: int = 4,
                 combine_conf: bool = False):
        if model.training:
            raise MvsHipError("SceneInference is an inference path: put the model in eval() first")
        if not hasattr(model, "extract_features") or not hasattr(model, "forward_bank"):
            raise MvsHipError("SceneInference needs a DINOMVSNet (extract_features + forward_bank)")
        if extract_batch < 1:
            raise ValueError("extract_batch must be at least 1")
        self.model = model
        self.capacity_views = capacity_views
        self.max_bank_mb = float(max_bank_mb)
        self.extract_batch = int(extract_batch)
        self.combine_conf = bool(combine_conf)
        self.images: Dict[int, torch.Tensor] = {}
        self.cams: Dict[int, torch.Tensor] = {}
        self.depth_ranges: Dict[int, torch.Tensor] = {}
        self.pairs: List[Tuple[int, List[int]]] = []
        self.num_views = 0
        self.hw: Optional[Tuple[int, int]] = None
        self.device: Optional[torch.device] = None
        self.banks: Optional[Dict[str, torch.Tensor]] = None
        self.stats: Dict[str, object] = {}
        self.timing = False                                  # True: run() brackets extraction and cascade with HIP events (timings())
        self._events: Dict[str, list] = {"extract": [], "cascade": []}
        self.depth_meter = None                              # run(gt=...): the metrics.DeviceAverageMeter of the last run

    # ------------------------------------------------------------------------------------------------ inputs
    def _gpu(self, t, name: str) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise MvsHipError("%s must be a GPU tensor: the MI355X HIP path is the only implementation (no CPU fallback)" % name)
        if t.dtype != torch.float32:
            raise MvsHipError("%s must be float32, got %s" % (name, t.dtype))
        if self.device is None:
            self.device = t.device
        if t.device != self.device:
            raise MvsHipError("%s lives on %s, the scene on %s" % (name, t.device, self.device))
        return t.detach()

    def add_image(self, view_id: int, img, cam, depth_range) -> None:
        img, cam, depth_range = self._gpu(img, "img"), self._gpu(cam, "cam"), self._gpu(depth_range, "depth_range")
        if img.dim() != 3 or img.shape[0] != 3:
            raise MvsHipError("view %d: img must be [3,H,W], got %s" % (view_id, tuple(img.shape)))
        h, w = img.shape[1:]
        if h % 64 or w % 64:
            raise MvsHipError("view %d: the image is %dx%d; H and W must be multiples of 64 (resize / crop before add_image)" % (view_id, h, w))
        if self.hw is None:
            self.hw = (h, w)
        if (h, w) != self.hw:
            raise MvsHipError("view %d is %dx%d, the scene %dx%d: all views of a scene share H x W" % (view_id, h, w, *self.hw))
        if cam.numel() != 32:
            raise MvsHipError("view %d: cam must be [2,4,4], got %s" % (view_id, tuple(cam.shape)))
        if depth_range.dim() != 1 or depth_range.numel() < 2:
            raise MvsHipError("view %d: depth_range must be the 1-D hypothesis range [N >= 2], got %s" % (view_id, tuple(depth_range.shape)))
        self.images[int(view_id)] = img.contiguous()
        self.cams[int(view_id)] = cam.reshape(2, 4, 4).contiguous()
        self.depth_ranges[int(view_id)] = depth_range.contiguous()
        self.banks = None

    def set_pairs(self, pairs, num_views: int = 5) -> None:
        """``[(ref_id, [src_id, ...])]`` in output order (``data_io.read_pair_file``); a sample uses the first ``num_views - 1`` sources."""
        self.pairs = [(int(r), [int(v) for v in srcs]) for r, srcs in pairs]
        self.num_views = int(num_views)

    # ------------------------------------------------------------------------------------------------ the bank
    def view_bytes(self) -> int:
        """Bytes of one view's four feature maps in the bank (fp32)."""
        h, w = self.hw
        chans = list(self.model.args["feat_chs"])[::-1]     # stage 1 (1/8 resolution) is the widest
        return sum(4 * (h // s) * (w // s) * c for s, c in zip(synth.STAGE_SCALES, chans))

    def _capacity(self, n_distinct: int, per_sample: int) -> int:
        if self.capacity_views is not None:
            cap = int(self.capacity_views)
            if cap < per_sample:
                raise ValueError("capacity_views = %d is smaller than the %d views of one sample" % (cap, per_sample))
            return min(cap, n_distinct)
        fit = int(self.max_bank_mb * 2 ** 20 // self.view_bytes())
        if fit >= n_distinct:
            return n_distinct
        if fit < per_sample:
            raise ValueError("max_bank_mb = %.0f holds %d views of %d bytes, one sample needs %d" % (self.max_bank_mb, fit, self.view_bytes(), per_sample))
        return fit

    def _mark(self, what: str):
        """With ``timing``: an event pair on the current stream around a piece of run(); returns the closing call."""
        if not self.timing:
            return lambda: None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        self._events[what].append((a, b))
        return b.record

    def timings(self) -> Dict[str, float]:
        """Device milliseconds of the last ``run()`` with ``timing = True``: ``extract`` (2-D networks + the copy into the bank) and
        ``cascade`` (four stages + the confidence record), summed over the scan."""
        torch.cuda.synchronize(self.device)
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self._events.items()}

    def _extract(self, jobs: List[Tuple[int, int]]) -> None:
        """The 2-D networks on the named images, ``extract_batch`` at a time, into their bank slots."""
        for i in range(0, len(jobs), self.extract_batch):
            chunk = jobs[i:i + self.extract_batch]
            imgs = torch.stack([self.images[v] for v, _ in chunk]).unsqueeze(0)            # [1,n,3,H,W]
            feats = self.model.extract_features(imgs)
            slots = torch.tensor([s for _, s in chunk], device=self.device, dtype=torch.long)
            for k, bank in self.banks.items():
                f = ops.to_channels_last(feats[k].detach().to(torch.float32))[0]          # [n,h,w,C]; zero-copy from the eval decoder
                if tuple(f.shape[1:]) != tuple(bank.shape[1:]):
                    raise MvsHipError("extract_features gave %s %s, the bank holds %s" % (k, tuple(f.shape[1:]), tuple(bank.shape[1:])))
                bank.index_copy_(0, slots, f)
            self.stats["extracted"] += len(chunk)
            self.stats["extract_passes"] += 1

    # ------------------------------------------------------------------------------------------------ run
    def run(self, tmp=2.0, fusion=None, save_to: Optional[str] = None, gt=None, meter=None) -> Dict[int, Dict[str, torch.Tensor]]:
        """Depth and confidence of every reference view of the pairs, in their order.  -> ``{ref_id: {"depth": [H,W], "confidence":
        [4,H,W] (or [H,W] with combine_conf), "cam": [2,4,4]}}`` as device tensors.  ``fusion``: a ``fusion.SceneFusion`` that gets every
        finished view (with its de-normalised uint8 image) and the pairs - ``fusion.fuse()`` is then images -> point cloud with no file in
        between.  ``save_to``: a scan folder that gets the files the reference writes (``data_io.save_depth_outputs``, ``save_image``).
        ``gt``: ground truth per reference view, ``{ref_id: (depth [H,W], mask [H,W])}`` device tensors at output resolution (a mapping or a
        callable ``ref_id -> (depth, mask)``; mask fp32 valid where > 0.5, or bool).  Every view's depth map then goes into a
        ``metrics.DeviceAverageMeter`` (``meter``, or a fresh one) with test.py:310-320's seven entries - ``abs_depth_error`` and
        ``thres{1,2,4,8,14,20}mm_error`` at multiples of ``depth_interval / 2.65`` - by one launch sequence per view and no host
        synchronisation; the meter is ``self.depth_meter`` afterwards (``.mean()`` -> ``metrics.write_depth_metric_txt``)."""
        if not self.pairs or not self.images:
            raise ValueError("SceneInference.run: add_image() and set_pairs() first")
        if self.model.training:
            raise MvsHipError("SceneInference is an inference path: put the model in eval() first")
        distinct = []
        for r, srcs in self.pairs:
            for v in [r] + srcs[:self.num_views - 1]:
                if v not in distinct:
                    distinct.append(v)
        per_sample = max(len({r, *srcs[:self.num_views - 1]}) for r, srcs in self.pairs)
        for v in distinct:
            if v not in self.images:
                raise ValueError("view %d is named in the pairs but was never added" % v)
        cap = self._capacity(len(distinct), per_sample)
        steps = plan(self.pairs, self.num_views, cap, view_ids=self.images.keys(), extract_batch=self.extract_batch)
        h, w = self.hw
        nstage = len(self.model.ndepths)
        if nstage != 4:
            raise MvsHipError("SceneInference is built for the four-stage cascade (got %d stages)" % nstage)
        with torch.cuda.device(self.device), torch.no_grad():
            chans = list(self.model.args["feat_chs"])[::-1]
            self.banks = {"stage%d" % (i + 1): torch.empty(cap, h // s, w // s, c, device=self.device, dtype=torch.float32)
                          for i, (s, c) in enumerate(zip(synth.STAGE_SCALES, chans))}
            self.stats = {"capacity_views": cap, "views": len(distinct), "samples": len(steps), "extracted": 0, "extract_passes": 0,
                          "bank_bytes": sum(b.numel() * 4 for b in self.banks.values()), "view_bytes": self.view_bytes()}
            # proj_matrices of every sample up front: per stage the scan's cameras [Nd,2,4,4], gathered by each sample's views
            pos = {v: j for j, v in enumerate(distinct)}
            per_view = [stage_cams(self.cams[v]) for v in distinct]
            cams_k = [torch.stack([c[k] for c in per_view]) for k in range(nstage)]
            vidx = [torch.tensor([pos[v] for v in st["views"]], device=self.device, dtype=torch.long) for st in steps]
            nrefs = len(steps)
            depths = torch.empty(nrefs, h, w, device=self.device, dtype=torch.float32)
            confs = torch.empty((nrefs, h, w) if self.combine_conf else (nrefs, 4, h, w), device=self.device, dtype=torch.float32)
            out: Dict[int, Dict[str, torch.Tensor]] = {}
            self._events = {"extract": [], "cascade": []}
            self.depth_meter = None
            if gt is not None:
                from . import metrics as _metrics
                names = [_metrics.ABS_KEY] + _metrics.threshold_names(_metrics.TEST_MULTIPLIERS)
                self.depth_meter = meter if meter is not None else _metrics.DeviceAverageMeter(names, self.device)
            for i, st in enumerate(steps):
                if st["extract"]:
                    done = self._mark("extract")
                    self._extract(st["extract"])
                    done()
                done = self._mark("cascade")
                proj = {"stage%d" % (k + 1): cams_k[k].index_select(0, vidx[i]).unsqueeze(0) for k in range(nstage)}
                dv = self.depth_ranges[st["ref"]].unsqueeze(0)
                o = self.model.forward_bank(self.banks, [st["table"]], proj, dv, tmp=tmp)
                depths[i].copy_(o["refined_depth"][0])
                if self.combine_conf:
                    confs[i].copy_(o["photometric_confidence"][0])
                else:
                    ops.conf_stack([o["stage%d" % (k + 1)]["photometric_confidence"] for k in range(nstage)], confs[i])
                done()
                if gt is not None:
                    gt_depth, gt_mask = gt(st["ref"]) if callable(gt) else gt[st["ref"]]
                    if tuple(gt_depth.shape) != (h, w) or tuple(gt_mask.shape) != (h, w):
                        raise MvsHipError("view %d: ground truth is %s / %s, the depth map %dx%d (resize it beforehand)"
                                          % (st["ref"], tuple(gt_depth.shape), tuple(gt_mask.shape), h, w))
                    _metrics.depth_metrics(depths[i:i + 1], gt_depth.unsqueeze(0), gt_mask.unsqueeze(0), depth_interval=dv[:, 1] - dv[:, 0],
                                           multipliers=_metrics.TEST_MULTIPLIERS, meter=self.depth_meter)
                out[st["ref"]] = {"depth": depths[i], "confidence": confs[i], "cam": self.cams[st["ref"]]}
            if fusion is not None or save_to is not None:
                imgs8 = {v: self.image_uint8(v) for v in distinct}
            if fusion is not None:
                for r, o in out.items():
                    fusion.add_view(r, o["depth"], o["confidence"], o["cam"], imgs8[r])
                fusion.set_pairs(self.pairs)
            if save_to is not None:
                from . import data_io
                for r, o in out.items():
                    c = o["confidence"]
                    c = c[..., None] if c.dim() == 2 else c.permute(1, 2, 0)               # [H,W,C] on disk (test.py:292)
                    data_io.save_depth_outputs(save_to, r, o["depth"].cpu().numpy(), c.contiguous().cpu().numpy(), o["cam"].cpu().numpy())
                for v in distinct:
                    data_io.save_image(save_to, v, imgs8[v].permute(1, 2, 0).contiguous().cpu().numpy())
        return out

    def image_uint8(self, view_id: int) -> torch.Tensor:
        """``add_image``'s input de-normalised to the uint8 ``[3,H,W]`` the point cloud takes its colours from."""
        img = self.images[view_id]
        mean = torch.tensor(IMAGENET_MEAN, device=img.device, dtype=torch.float32).view(3, 1, 1)
        std = torch.tensor(IMAGENET_STD, device=img.device, dtype=torch.float32).view(3, 1, 1)
        return (img * std + mean).mul(255.0).round().clamp(0, 255).to(torch.uint8)
