"""``StageNet`` — one cascade stage of the plane-sweep path, drop-in for the reference class of the same name
(models/mvsformer_model.py:26-160): same constructor ``StageNet(args, ndepth, stage_idx)``, same
``forward(features, proj_matrices, depth_values, tmp=2.0)``, same output dict keys, same ``state_dict`` keys
(``vis.{0,1,2}.{conv,bn}.*``, ``vis.3.*``, ``cost_reg.*``).

Where the reference runs ~40 ATen launches per source view over materialized [B,C,D,H,W] temporaries, this
forward is 5 + 10 hand-written HIP launches per stage:

    mvs_proj_prepare -> mvs_nchw_to_nhwc (skipped for channel-last inputs) -> sweep A -> mvs_vis_wino_fwd -> sweep B
    -> 9 fused conv/deconv MFMA layers -> (mvs_prob3_fwd) -> mvs_head_fwd

The sweeps are chosen per stage (``sweep_plan``): coarse stages keep the per-view correlation volumes sweep A computes
(``mvs_cv_corr_fwd``), so that sweep B is a pure stream over them (``mvs_cv_merge_fwd``); fine stages recompute the
correlation in sweep B (``mvs_cv_entropy_fwd`` / ``mvs_cv_aggregate_fwd``) because their per-view volumes no longer fit the
Infinity Cache.  ``MVS_CV_TILED=1`` opts into the LDS-tiled sweeps of cost_volume_tiled.hip (they lose on the noisy
hypotheses a random-weight cascade predicts).

Training mode runs the same steps under :mod:`mvsformer_amd.autograd`; every ``depth_type``'s head is a HIP kernel there too (``HeadFn``
for 'ce' / 'was', ``MixupHeadFn`` for 'mixup_ce', ``RegHeadFn`` for the regression head - csrc/head_train.hip).  The hypotheses a stage is
given may ascend (linear depth) or descend (inverse depth) with d: nothing here depends on their order.

``DepthNet`` is the name BASELINE.json uses for the same thing.
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache, partial
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import ops, switches as sw
from ._lib import MvsHipError
from .module import ConvBnReLU, CostRegNet, CostRegNet3D, _publish_cache, _versions, pack_vis_params


VIS_HALO = 3          # receptive-field radius of the visibility CNN (three 3x3 layers): rows a band needs beyond its own
TILED = -1            # :func:`sweep_plan`: the LDS-tiled sweeps


class StageSwitches(NamedTuple):
    """The environment switches of a stage's eval sweeps, read once per forward (:func:`stage_switches`)."""
    tiled: bool = False           # MVS_CV_TILED
    store_max_mb: float = 160.0   # MVS_CV_STORE_MAX_MB
    store_bands: int = 1          # MVS_CV_STORE_BANDS
    vis: str = "x3"               # MVS_VIS (unset: MVS_VIS_WINO decides): x3 = split-form bf16 MFMA | wino = Winograd fp32 MFMA | valu = all-VALU


def stage_switches() -> StageSwitches:
    return StageSwitches(sw.flag("MVS_CV_TILED"), sw.number("MVS_CV_STORE_MAX_MB"), sw.integer("MVS_CV_STORE_BANDS"),
                         sw.text("MVS_VIS") or ("x3" if sw.flag("MVS_VIS_WINO") else "valu"))


def sweep_plan(store_bytes: int, H: int, tiled_ok: bool, ss: StageSwitches) -> int:
    """How the stage builds its cost volume: ``TILED`` = the LDS-tiled sweeps (MVS_CV_TILED=1, where the features allow them); 0 = recompute
    the correlation in sweep B; 1 = keep the per-view correlation volumes of the whole image (stored-correlation sweeps, built for C = 32 | 64: ``store_bytes``
    <= 0 otherwise); k > 1 = the same in k bands of reference rows, each band's store small enough to stay inside the 256 MB Infinity Cache next to the feature
    maps (MVS_CV_STORE_MAX_MB, default 160; 0 disables the path; MVS_CV_STORE_BANDS caps k, default 1 - banding is opt-in until it is measured faster at
    config-2 stage 2).  Measured at config 2 (profiles/r03_bench_sweeps.txt): stage 1 (127 MB) 0.30 -> 0.20 ms for the pair; stage 2 in one piece (254 MB:
    the round trip goes to HBM) 0.29 -> 0.32 ms."""
    if ss.tiled and tiled_ok:
        return TILED
    limit = ss.store_max_mb * 2 ** 20
    if store_bytes <= 0 or limit <= 0:
        return 0
    if store_bytes <= limit:
        return 1
    for k in range(2, ss.store_bands + 1):
        rows = -(-H // k) + 2 * VIS_HALO + 1                  # (+1: a band's first row is rounded down to even)
        if rows < H and store_bytes * rows / H <= limit:
            return k
    return 0


def _store_plan(feat_cl, D, G) -> int:
    """:func:`sweep_plan` of channel-last ``feat_cl [B,V,H,W,C]`` without the tiled sweeps."""
    return _store_plan_bytes(ops.cv_store_bytes(feat_cl, D, G), feat_cl.shape[2])


def _store_plan_bytes(nbytes: int, H: int) -> int:
    """:func:`sweep_plan` from the store's size (``ops.cv_store_bytes``; <= 0: not built for the shape) and the image height."""
    return sweep_plan(nbytes, H, False, stage_switches())


# Feature source of the sweeps: sizes, the maps for the LDS-tiled sweeps (None: not built for them), ``store_bytes(D, G)`` and the sweeps that
# read features (``ops.cv_*`` without their first arguments; ``corr`` = sweep A' on the whole image, ``corr_rows`` = on a band)
_Views = namedtuple("_Views", "B V C tiled store_bytes entropy aggregate corr corr_rows")


def _dense_views(feat) -> _Views:
    """Dense ``[B,V,C,H,W]`` maps; the direct sweeps read them channel-last, made on first use (zero-copy if they are already)."""
    B, V, C, H, W = feat.shape
    cl = lru_cache(None)(lambda: ops.to_channels_last(feat))
    on = lambda op: lambda *args, **kw: op(cl(), *args, **kw)
    return _Views(B, V, C, feat if ops.cv_tiled_supported(feat) else None, lambda D, G: ops.cv_store_bytes_of(B, V, C, G, D, H, W),
                  on(ops.cv_entropy), on(ops.cv_aggregate), on(ops.cv_corr), on(ops.cv_corr_rows))


def _bank_views(bank, rows) -> _Views:
    """A bank ``[N,H,W,C]`` channel-last + the host table ``rows [B][V]`` of the views each sample is made of (no LDS-tiled form)."""
    B, V = len(rows), len(rows[0])
    corr_rows = partial(ops.cv_corr_rows_views, bank, rows)
    return _Views(B, V, bank.shape[3], None, partial(ops.cv_bank_store_bytes, bank, B, V), partial(ops.cv_entropy_views, bank, rows),
                  partial(ops.cv_aggregate_views, bank, rows), lambda rt, hyp, G: corr_rows(rt, hyp, G, 0, bank.shape[1]), corr_rows)


_VIS_KERNELS = {"valu": lambda entropy, params, prepared: ops.vis(entropy, params), "x3": ops.vis_x3, "wino": ops.vis_wino}


class StageNet(nn.Module):
    def __init__(self, args, ndepth, stage_idx):
        super().__init__()
        self.args = args
        self.fusion_type = args.get("fusion_type", "cnn")
        self.ndepth = ndepth
        self.stage_idx = stage_idx
        in_channels = args["base_ch"]
        if self.fusion_type != "cnn":
            raise NotImplementedError(
                "fusion_type=%r: only 'cnn' (every shipped reference config) is built for MI355X" % self.fusion_type)
        model_th = args.get("model_th", 8)
        self.vis = nn.Sequential(ConvBnReLU(1, 16), ConvBnReLU(16, 16), ConvBnReLU(16, 8), nn.Conv2d(8, 1, 1), nn.Sigmoid())
        if ndepth <= model_th:
            self.cost_reg = CostRegNet3D(in_channels, args["base_ch"])
        else:
            self.cost_reg = CostRegNet(in_channels, args["base_ch"])
        self._vis_cache = None
        self._train_pack = None
        self._routed_by_cascade = False

    def _vis_params(self, ss: Optional[StageSwitches] = None):
        """-> (parameter block, the 3x3 layers' weights prepared for the selected kernel or None for the all-VALU form)."""
        mode = (ss or stage_switches()).vis
        key = (_versions(self.vis), mode)
        if self._vis_cache is None or self._vis_cache[0] != key:
            params = pack_vis_params(self.vis)
            prepared = ops.vis_x3_prepare(params) if mode == "x3" else ops.vis_wino_prepare(params) if mode == "wino" else None
            _publish_cache()                                    # cached tensors are read from any stream afterwards
            self._vis_cache = (key, params, prepared)
        return self._vis_cache[1:]

    def _vis_weight(self, entropy, vis_params, vis_prepared, mode: Optional[str] = None):
        """The visibility CNN on what :meth:`_vis_params` returned; ``mode``: what they were prepared for (default: the cached mode)."""
        mode = mode or (self._vis_cache[0][1] if self._vis_cache is not None else stage_switches().vis)
        return _VIS_KERNELS[mode](entropy, vis_params, vis_prepared)

    def _eval(self, src: _Views, proj_matrices, depth_values, tmp):
        """The eval forward over the feature source ``src``: step 2 of the reference forward (fused warp + group correlation + visibility-weighted
        aggregation) by :func:`sweep_plan`, then regularization + head."""
        ss, G = stage_switches(), self.args["base_ch"]
        proj = proj_matrices.detach().to(torch.float32).contiguous()
        hyp = depth_values.detach().to(torch.float32).contiguous()
        if hyp.dim() != 4:
            raise MvsHipError("depth_values must be [B,D,H,W]")
        rt, (vis_params, vis_prepared) = ops.proj_prepare(proj), self._vis_params(ss)
        vis = lambda entropy: self._vis_weight(entropy, vis_params, vis_prepared, ss.vis)
        D, H, W = hyp.shape[1:]
        plan = sweep_plan(src.store_bytes(D, G), H, src.tiled is not None, ss)
        if plan == TILED:                                       # LDS-tiled sweeps straight from the decoder's NCHW maps
            weight = vis(ops.cv_tiled_entropy(src.tiled, rt, hyp, G))
            volume, sim_depth = ops.cv_tiled_aggregate(src.tiled, rt, hyp, weight, G, want_sim_depth=True)
        elif plan == 0:
            volume, sim_depth = src.aggregate(rt, hyp, vis(src.entropy(rt, hyp, G)), G, want_sim_depth=True)
        elif plan == 1:
            entropy, store = src.corr(rt, hyp, G)
            volume, sim_depth = ops.cv_merge(store, hyp, vis(entropy), src.V, src.C, G, want_sim_depth=True)
        else:
            # row bands: sweep A' on the band + VIS_HALO rows either side (the rows the visibility CNN's 7 x 7 receptive field reaches),
            # the CNN on the band as an image of its own (exact inside the band: its zero padding only touches the halo rows or the true
            # image border), sweep B' on the band without the halo - the band's store is read back while it is still in the cache
            volume = torch.empty(src.B, G, D, H, W, device=hyp.device, dtype=torch.float32)
            sim_depth = torch.empty(src.B, H, W, device=hyp.device, dtype=torch.float32)
            hb, store = -(-H // plan), None
            for r0 in range(0, H, hb):
                r1 = min(H, r0 + hb)
                # an EVEN first row: the MFMA visibility kernels compute output rows in pairs (x3: one tile holds rows 2p and 2p + 1 with the
                # taps at different K positions; wino: F(2x2,3x3)), so a row's rounding depends on its parity in the image the CNN is given
                y0, y1 = max(0, (r0 - VIS_HALO) & ~1), min(H, r1 + VIS_HALO)
                entropy, store = src.corr_rows(rt, hyp, G, y0, y1 - y0, store)
                ops.cv_merge_rows(store, hyp, vis(entropy), src.V, src.C, G, y0, r0 - y0, r1 - r0, volume, sim_depth)
        return self._regularize_head(volume, sim_depth, hyp, depth_values, tmp)

    def forward(self, features, proj_matrices, depth_values, tmp=2.0):
        """``features [B,V,C,H,W]`` (view 0 = reference), ``proj_matrices [B,V,2,4,4]``, ``depth_values [B,D,H,W]``."""
        if features.shape[1] != proj_matrices.shape[1]:
            raise AssertionError("Different number of images and projection matrices")
        if self.training:
            return self._forward_train(features, proj_matrices, depth_values, tmp, self.args["base_ch"])
        return self._eval(_dense_views(features.detach().to(torch.float32)), proj_matrices, depth_values, tmp)

    def forward_bank(self, bank, view_idx, proj_matrices, depth_values, tmp=2.0):
        """Eval forward over a feature BANK: ``bank [N,H,W,C]`` channel-last holds a scene's views once each, ``view_idx [B,V]`` (host
        integers, column 0 = the reference view) says which of them sample ``b`` is made of; ``proj_matrices [B,V,2,4,4]`` and
        ``depth_values [B,D,H,W]`` as for :meth:`forward`.  Same plan, same kernels' arithmetic and same output dict as ``forward`` on
        ``bank[view_idx]`` - the sweeps read the views in place (``ops.cv_*_views``).  ``MVS_CV_TILED`` is ignored: the LDS-tiled sweeps
        have no indexed form."""
        if self.training:
            raise MvsHipError("StageNet.forward_bank is an inference path: call .eval() first (training reads [B,V,C,H,W] through forward)")
        if not isinstance(bank, torch.Tensor) or not bank.is_cuda or bank.dim() != 4:
            raise MvsHipError("bank must be a channel-last GPU tensor [N,H,W,C]: the MI355X HIP path is the only implementation (no CPU fallback)")
        rows = view_idx.tolist() if hasattr(view_idx, "tolist") else [list(r) for r in view_idx]
        if proj_matrices.shape[:2] != (len(rows), len(rows[0])):
            raise AssertionError("Different number of images and projection matrices")
        return self._eval(_bank_views(bank.detach(), rows), proj_matrices, depth_values, tmp)

    def _regularize_head(self, volume, sim_depth, hyp, depth_values, tmp):
        """Step 3 of the eval forward: regularization + head."""
        depth_type = self.args["depth_type"]
        if type(tmp) == list:
            tmp = tmp[self.stage_idx]
        if isinstance(self.cost_reg, CostRegNet3D):
            logits = self.cost_reg.logits(volume)               # conv11 + 1x1x1 prob fused: the 8-channel volume is never written
        else:
            x = self.cost_reg.features(volume)
            logits = ops.prob3(x, self.cost_reg.prob.weight.detach().to(torch.float32).contiguous())
        if depth_type in ("ce", "was"):
            pre, prob, depth, conf = ops.head(hyp, float(tmp), False, logits=logits)
        elif depth_type == "mixup_ce":                          # mvsformer_model.py:126-136
            pre, prob, _, _ = ops.head(hyp, 1.0, False, logits=logits)
            depth, conf = ops.mixup_head(prob, hyp)
        else:                                                   # regression head, mvsformer_model.py:137-146 (tmp unused)
            pre, prob, depth, conf = ops.head(hyp, 1.0, False, logits=logits)
            n = self._conf_window()
            if n:
                conf = ops.conf_regression(prob, n)
        return {"depth": depth, "prob_volume": prob, "photometric_confidence": conf, "depth_values": depth_values,
                "prob_volume_pre": pre, "sim_depth": sim_depth}

    def _conf_window(self):
        """Window of conf_regression for the regression head (mvsformer_model.py:139-146); 0 = plain max probability."""
        return 4 if self.ndepth >= 32 else 3 if self.ndepth == 16 else 2 if self.ndepth == 8 else 0

    def train_pack(self):
        """This stage's :class:`autograd.StagePack` (bf16 weight layouts of a training step in one launch + weight-gradient routing)."""
        from . import autograd as ag
        if self._train_pack is None or not self._train_pack.valid():
            self._train_pack = ag.StagePack(self)
        return self._train_pack

    def _forward_train(self, features, proj_matrices, depth_values, tmp, G):
        """Training branch (reference mvsformer_model.py:62-125 with ``self.training``): no similarity branch, batch-statistics
        BatchNorm everywhere, depth = hypothesis at the arg-max probability; gradients via :mod:`mvsformer_amd.autograd`."""
        from . import autograd as ag
        from .module import autocast_bf16
        if autocast_bf16() and ag._fused_layers():              # every bf16 weight layout of this stage's step in one launch
            pack = self.train_pack()
            pack.run(route=not self._routed_by_cascade)
            try:
                return self._forward_train_body(features, proj_matrices, depth_values, tmp, G)
            finally:
                if not self._routed_by_cascade:
                    pack.unroute()                              # the routed weights belong to this forward's graph only
        return self._forward_train_body(features, proj_matrices, depth_values, tmp, G)

    def _forward_train_body(self, features, proj_matrices, depth_values, tmp, G):
        from . import autograd as ag
        from .module import autocast_bf16
        proj = proj_matrices.detach().to(torch.float32).contiguous()
        hyp = depth_values.detach().to(torch.float32).contiguous()
        rt = ops.proj_prepare(proj)
        feat_cl = ops.to_channels_last(features.detach().to(torch.float32))
        entropy = ops.cv_entropy(feat_cl, rt, hyp, G, exact=True)           # sim_vol.detach() in the reference
        V = features.shape[1]
        weight = ag.vis_train_views(entropy, self.vis)                     # per-view statistics, one batched pass
        # under autocast the volume leaves the aggregation as bf16 channel-last too (the layout the bf16 regularizer reads) in the same launch
        volume = ag.AggregateFn.apply(features, weight, rt, hyp, G, feat_cl, autocast_bf16() and ag._fused_layers())
        if type(tmp) == list:
            tmp = tmp[self.stage_idx]
        pre = self.cost_reg(volume).squeeze(1)
        depth_type = self.args["depth_type"]
        if depth_type in ("ce", "was"):
            prob, depth, conf = ag.HeadFn.apply(pre, hyp, float(tmp))
        elif depth_type == "mixup_ce":                          # mvsformer_model.py:126-136, differentiable in prob_volume and depth
            prob, depth, conf = ag.MixupHeadFn.apply(pre, hyp)
        else:                                                   # regression head, mvsformer_model.py:137-146 (tmp unused)
            prob, depth, conf = ag.RegHeadFn.apply(pre, hyp, self._conf_window())
        return {"depth": depth, "prob_volume": prob, "photometric_confidence": conf.detach(), "depth_values": depth_values,
                "prob_volume_pre": pre}


DepthNet = StageNet
