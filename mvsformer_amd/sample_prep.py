"""Training and inference sample preparation on the device (csrc/sample_prep.hip).

``prepare_train_batch`` restates ``datasets/dtu_dataset_ms.py::__getitem__`` between the decoded bytes and the batch dict: the
``INTER_AREA`` pre-resize fused with the crop, the crop retry loop as a first-accepted search over ``K`` candidates, the ground-truth
pyramid, the four projection-matrix sets, ``depth_values``, PIL's colour jitter on uint8 and ``ToTensor`` / ``RandomGamma`` /
``Normalize``.  ``prepare_eval_views`` restates ``datasets/general_eval.py::scale_mvs_input`` (and ``read_img``'s edge padding).

The host only draws the random numbers (``draw_train_params``, in the reference's order from ``random``, ``numpy.random`` and ``torch``)
and writes them into small device tables (``TrainTables.write``, plain ``copy_``); every launch goes to the current stream, nothing
synchronises or reads back, and no launch geometry depends on the tables, so a batch can be prepared inside a ``CapturedStep``.
File discovery, PNG / JPEG decoding and the ``DataLoader`` are not here.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

OPS = ("brightness", "contrast", "saturation", "hue")


def jitter_range(value, name: str):
    """``ColorJitter._check_input`` (datasets/color_jittor.py:34-51): ``[lo, hi]`` or None when the operation does nothing."""
    center, bound, clip = (0.0, (-0.5, 0.5), False) if name == "hue" else (1.0, (0.0, float("inf")), True)
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError("If {} is a single number, it must be non negative.".format(name))
        value = [center - float(value), center + float(value)]
        if clip:
            value[0] = max(value[0], 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        if not bound[0] <= value[0] <= value[1] <= bound[1]:
            raise ValueError("{} values should be between {}".format(name, bound))
        value = list(value)
    else:
        raise TypeError("{} should be a single number or a list/tuple with lenght 2.".format(name))
    return None if value[0] == value[1] == center else value


@dataclass
class TrainParams:
    """What ``__getitem__`` draws for one sample."""
    view_ids: List[int]
    resize_scales: List[float]                                   # per view (the reference draws enlarge_scale inside the view loop)
    candidates: List[Tuple[int, int]]                            # (offset_y, offset_x) of the reference view, K of them
    src_offsets: List[Optional[Tuple[int, int]]]                 # per source view; None = the reference view's chosen offset (consist_crop)
    fn_idx: Optional[List[int]] = None
    factors: Optional[Tuple[float, float, float, float]] = None  # brightness, contrast, saturation, hue
    gamma: Optional[float] = None
    enabled: Tuple[bool, bool, bool, bool] = field(default=(True, True, True, True))


def draw_train_params(ref_view: int, src_views: List[int], nviews: int, crop_hw, src_hw=(1200, 1600), mode: str = "train", crop: bool = True,
                      augment: bool = True, aug_args: Optional[dict] = None, resize_range=(1.0, 1.2), resize_scale: float = 0.5,
                      consist_crop: bool = False, K: int = 4) -> TrainParams:
    """The random draws of ``dtu_dataset_ms.py::__getitem__`` (:255-333) in its order, from the global ``random``, ``numpy.random`` and
    ``torch`` generators: ``np.random.shuffle(src_views)`` (in place, as the reference), ``torch.randperm(4)``, four ``uniform_`` and
    ``np.random.uniform`` for gamma, then per view ``random.random()`` for ``enlarge_scale`` and ``random.randint`` twice per offset.
    The retry loop becomes ``K`` candidate offsets drawn back to back (the reference draws only as many as it rejects, so the streams
    agree with it up to the first accepted candidate).  ``src_hw`` stands where the reference has DTU's 1200 x 1600."""
    crop_h, crop_w = crop_hw
    H0, W0 = src_hw
    train = mode == "train"
    if not train:
        crop, augment = False, False
    if train:
        np.random.shuffle(src_views)
    view_ids = [ref_view] + list(src_views[:nviews - 1])
    p = TrainParams(view_ids=view_ids, resize_scales=[], candidates=[], src_offsets=[])
    if augment:
        rng = [jitter_range(aug_args[n], n) for n in OPS]
        p.enabled = tuple(r is not None for r in rng)
        p.fn_idx = [int(i) for i in torch.randperm(4)]
        # the reference indexes the range unconditionally (an operation whose range is None cannot be drawn there); drawn only where enabled
        p.factors = tuple(torch.tensor(1.0).uniform_(r[0], r[1]).item() if r is not None else (0.0 if n == "hue" else 1.0)
                          for r, n in zip(rng, OPS))
        p.gamma = float(np.random.uniform(aug_args["min_gamma"], aug_args["max_gamma"]))
    for i in range(len(view_ids)):
        if train:
            enlarge = resize_range[0] + random.random() * (resize_range[1] - resize_range[0])
            rs = float(max(np.clip((crop_h * enlarge) / H0, 0.45, 1.0), np.clip((crop_w * enlarge) / W0, 0.45, 1.0)))
        else:
            rs = resize_scale
        p.resize_scales.append(rs)
        rh, rw = (int(H0 * rs), int(W0 * rs)) if rs != 1.0 else (H0, W0)
        if rh < crop_h or rw < crop_w:
            raise ValueError("view %d: resized image %dx%d is smaller than the crop %dx%d" % (i, rh, rw, crop_h, crop_w))

        def offset():
            if crop:
                oy = random.randint(0, rh - crop_h)
                return oy, random.randint(0, rw - crop_w)
            return (rh - crop_h) // 2, (rw - crop_w) // 2
        if i == 0:
            p.candidates = [offset() for _ in range(K if (train and crop) else 1)]
        else:
            p.src_offsets.append(None if consist_crop else offset())
    return p


def hue_shift(hue_factor: float) -> int:
    """``np.uint8(hue_factor * 255)`` of torchvision's ``adjust_hue``: truncated toward zero, modulo 256."""
    return int(hue_factor * 255) & 0xFF


def arange_length(depth_min: float, depth_interval: float, ndepths: int) -> int:
    """Length of ``np.arange(depth_min, depth_interval * ndepths + depth_min, depth_interval)``."""
    return int(math.ceil((depth_interval * ndepths + depth_min - depth_min) / depth_interval))


def _f32_bits(x: float) -> int:
    return int(np.float32(x).view(np.int32))


class TrainTables:
    """The device tables of ``B`` samples and their pinned host twins; ``write`` is the only host -> device traffic of a batch.

    ``write`` copies asynchronously and records an event behind the copies; ``fill_host`` waits for that event before it touches the
    pinned memory again, so a pipelined caller (write, replay, write the next batch) cannot tear a table the copy engine is still
    reading.  The event completes when the copies have run, which is after whatever preceded them on that stream; the launches that
    follow ``write`` are never waited for."""

    def __init__(self, B: int, V: int, K: int, device="cuda"):
        self.B, self.V, self.K = B, V, K
        pin = torch.cuda.is_available()
        self.host = dict(ptab=torch.zeros(B, V, ops.PREP_VIEW_INTS, dtype=torch.int32, pin_memory=pin),
                         cand=torch.zeros(B, K, 2, dtype=torch.int32, pin_memory=pin),
                         jtab=torch.zeros(B, ops.PREP_JITTER_INTS, dtype=torch.int32, pin_memory=pin),
                         drange=torch.zeros(B, 2, dtype=torch.float64, pin_memory=pin))
        self.ptab, self.cand, self.jtab, self.drange = (self.host[k].to(device) for k in ("ptab", "cand", "jtab", "drange"))
        self.chosen = torch.zeros(B, 4, dtype=torch.int32, device=device)
        self.enabled = (True, True, True, True)
        self._copied = None                                       # event behind the last write's copies

    def fill_host(self, params: Sequence[TrainParams], src_hw, depth_min: Sequence[float], depth_interval: Sequence[float]) -> None:
        assert len(params) == self.B
        if self._copied is not None:
            self._copied.synchronize()
            self._copied = None
        H0, W0 = src_hw
        pt, cd, jt, dr = (self.host[k] for k in ("ptab", "cand", "jtab", "drange"))
        pt.zero_(), cd.zero_(), jt.zero_()
        for b, p in enumerate(params):
            assert len(p.resize_scales) == self.V and 1 <= len(p.candidates) <= self.K
            for v, rs in enumerate(p.resize_scales):
                rh, rw = (int(H0 * rs), int(W0 * rs)) if rs != 1.0 else (H0, W0)
                if W0 >= 3 * rw or H0 >= 3 * rh:
                    # the reference's range is 0.45 .. 1; from 3:1 on OpenCV's integer reductions take another path (resizeAreaFast)
                    raise _lib.MvsHipError("sample_prep: a reduction by 3 or more is not built (resize_scale %g)" % rs)
                off = None if v == 0 else p.src_offsets[v - 1]
                row = [rw, rh, 0 if off is None else off[1], 0 if off is None else off[0], int(off is None), _f32_bits(rs), int(rs != 1.0), 0]
                pt[b, v] = torch.tensor(row, dtype=torch.int32)
            cands = list(p.candidates) + [p.candidates[-1]] * (self.K - len(p.candidates))      # padding repeats the last: same outcome
            cd[b] = torch.tensor(cands, dtype=torch.int32)
            if p.fn_idx is not None:
                f = p.factors
                jt[b] = torch.tensor(list(p.fn_idx) + [sum(1 << k for k in range(4) if p.enabled[k]), int(p.gamma is not None), hue_shift(f[3]), 0,
                                                       _f32_bits(f[0]), _f32_bits(f[1]), _f32_bits(f[2]), _f32_bits(p.gamma or 1.0), 0, 0, 0, 0],
                                     dtype=torch.int32)
                self.enabled = tuple(p.enabled)
            dr[b, 0], dr[b, 1] = float(depth_min[b]), float(depth_interval[b])

    def write(self, params=None, src_hw=None, depth_min=None, depth_interval=None) -> None:
        """Fill the host twins (when ``params`` is given) and copy them to the device tables on the current stream."""
        if params is not None:
            self.fill_host(params, src_hw, depth_min, depth_interval)
        for k in ("ptab", "cand", "jtab", "drange"):
            getattr(self, k).copy_(self.host[k], non_blocking=True)
        if self.ptab.is_cuda:
            self._copied = torch.cuda.Event()
            self._copied.record()


def prepare_train_batch(imgs, depth_hr, mask_raw, intrinsics, extrinsics, tables: TrainTables, crop_hw, length: int, augment: bool = True,
                        require_positive: bool = True) -> dict:
    """``imgs`` uint8 ``[B,V,H0,W0,3]``, ``depth_hr`` fp32 and ``mask_raw`` uint8 ``[B,H0,W0]`` (reference view), ``intrinsics``
    ``[B,V,3,3]``, ``extrinsics`` ``[B,V,4,4]``, ``tables`` already written -> the reference's batch dict: ``imgs [B,V,3,h,w]``,
    ``proj_matrices`` / ``depth`` / ``mask`` ``{stage1..4}``, ``depth_values [B,length]`` (``length`` = :func:`arange_length`), plus
    ``offset`` int32 ``[B,4]`` (offset_y, offset_x, accepted, candidate index).  Six launches on the current stream, no synchronisation."""
    chosen = ops.prep_accept(mask_raw, tables.ptab, tables.cand, crop_hw, require_positive=require_positive, chosen=tables.chosen)
    depth, mask, proj, dv = ops.prep_geometry(depth_hr, mask_raw, tables.ptab, chosen, intrinsics, extrinsics, tables.drange, crop_hw, length)
    u8 = ops.prep_area_crop(imgs, tables.ptab, chosen, crop_hw)
    out, _, _ = ops.prep_jitter_tail(u8, tables.jtab if augment else None, has_contrast=tables.enabled[1])
    return {"imgs": out, "proj_matrices": proj, "depth": depth, "mask": mask, "depth_values": dv, "offset": chosen}


def scale_intrinsics(intrinsics: np.ndarray, src_hw, out_hw) -> np.ndarray:
    """``scale_mvs_input``'s camera half (general_eval.py:117-124): rows 0 and 1 of an fp32 3x3 times ``max_w / w`` and ``max_h / h``."""
    k = np.array(intrinsics, dtype=np.float32, copy=True)
    k[0, :] *= np.float32(1.0 * out_hw[1] / src_hw[1])
    k[1, :] *= np.float32(1.0 * out_hw[0] / src_hw[0])
    return k


def prepare_eval_views(images, intrinsics: Optional[np.ndarray], max_h: int, max_w: int, tt_pad: bool = False, standard_hw=None):
    """``images`` uint8 ``[V,H0,W0,3]`` on the device -> ``(imgs fp32 [V,3,H,W], intrinsics [V,3,3] numpy or None)``: ``read_img``'s 4-row
    edge padding (``tt_pad``), ``scale_mvs_input`` to ``max_w x max_h`` and, when ``standard_hw`` differs from that, the second resize
    to the scene's standard size (``fix_res``, general_eval.py:187-205).  The intrinsics are those of the UNPADDED camera file, as the
    reference reads them (its ``tt`` branch shifts the principal point itself)."""
    V, H0, W0, _ = images.shape
    pad = 4 if tt_pad else 0
    hw = (H0 + 2 * pad, W0)
    k = None if intrinsics is None else np.stack([scale_intrinsics(intrinsics[v], hw, (max_h, max_w)) for v in range(V)])
    if standard_hw is not None and tuple(standard_hw) != (max_h, max_w):
        u8 = ops.prep_eval_resize(images, (max_h, max_w), pad_rows=pad, want="u8")
        out = ops.prep_eval_resize(u8, standard_hw)
        if k is not None:
            k = np.stack([scale_intrinsics(k[v], (max_h, max_w), standard_hw) for v in range(V)])
        return out, k
    return ops.prep_eval_resize(images, (max_h, max_w), pad_rows=pad), k
