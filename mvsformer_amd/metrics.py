"""Depth metrics and the validation epoch on the device - the reference's ``utils.py:119-182`` (``Thres_metrics``, ``AbsDepthError_metrics``,
``DictAverageMeter``), ``trainer/mvsformer_trainer.py:216-283`` (``_valid_epoch``) and ``test.py:310-327`` (``depth_metric.txt``).

The reference gathers the valid pixels twice per metric and ends every metric in an ``.item()``: five host synchronisations per validation
batch, seven per view in ``test.py``, one more per sample for BlendedMVS' ``depth_interval[j]``.  :func:`depth_metrics` is one call of
``mvs_depth_metrics`` (csrc/metrics.hip: exact integer counts, errors added in double, fixed order, no atomics) for all images, all
thresholds and the batch means, and it can advance a :class:`DeviceAverageMeter` at the end of the same stream-ordered work; the thresholds
are built on the device from the depth interval in fp64 - the host's double arithmetic on the same fp32 interval, so they are the
reference's bit for bit without its ``.item()``.  Nothing here waits for the device until ``DeviceAverageMeter.mean()`` is asked for
Python floats.

``DeviceAverageMeter`` and :func:`build_thresholds` are plain torch and also work on CPU tensors; the metrics themselves are the HIP path
only (a CPU tensor is refused, there is no fallback).
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence

import torch

from . import ops
from ._lib import MvsHipError

ABS_KEY = "abs_depth_error"
VALID_MULTIPLIERS = (2, 4, 8, 14)               # trainer/mvsformer_trainer.py:249-264
TEST_MULTIPLIERS = (1, 2, 4, 8, 14, 20)         # test.py:312-318


def threshold_names(multipliers: Sequence[float]) -> list:
    """``(2, 4, 8, 14)`` -> ``['thres2mm_error', ...]``, the reference's keys."""
    return ["thres%gmm_error" % m for m in multipliers]


def build_thresholds(depth_interval: torch.Tensor, multipliers: Sequence[float], per_sample_interval: bool = False,
                     batch: Optional[int] = None) -> torch.Tensor:
    """``[B,K]`` fp32 thresholds from ``depth_interval [B]`` (``depth_values[:,1] - depth_values[:,0]``) on its own device, no host read.
    DTU form (``test.py:311``, trainer ``:259``): ``multiplier * (depth_interval[0] / 2.65)`` for every image; Blended form
    (``per_sample_interval``, trainer ``:247-257``): ``multiplier * depth_interval[j]``.  The arithmetic is fp64 on the fp32 interval - what
    Python does with ``depth_interval[0].item()`` - and the result is rounded to fp32 once, as ``errors > thres`` rounds its scalar."""
    itv = depth_interval.detach().reshape(-1).to(torch.float32).to(torch.float64)
    B = itv.numel() if batch is None else int(batch)
    if per_sample_interval:
        if itv.numel() != B:
            raise ValueError("per_sample_interval needs one interval per image: %d for a batch of %d" % (itv.numel(), B))
        thr = torch.stack([itv * float(m) for m in multipliers], dim=1)                    # [B,K]
    else:
        di = itv[0] / 2.65
        thr = torch.stack([di * float(m) for m in multipliers]).unsqueeze(0).expand(B, -1)
    return thr.to(torch.float32).contiguous()


class DeviceAverageMeter:
    """``DictAverageMeter`` (utils.py:119-145) with its sums on the device: ``update`` adds 0-dim tensors (or the dict :func:`depth_metrics`
    returns) into fp64 accumulators and a count, with no copy to the host; ``mean()`` is one device-to-host copy; ``mean_tensors()`` is none.
    The same fp32 values added in double in the same order as the reference's Python floats.  ``keys`` / ``device`` may be left to the first
    ``update`` (the reference's constructor takes no argument); Python floats are accepted as the reference's meter accepts them."""

    def __init__(self, keys: Optional[Iterable[str]] = None, device=None):
        self.keys = None if keys is None else list(keys)
        self.device = None if device is None else torch.device(device)
        self.sums: Optional[torch.Tensor] = None
        self.count: Optional[torch.Tensor] = None
        if self.keys is not None and self.device is not None:
            self._allocate()

    def _allocate(self) -> None:
        self.sums = torch.zeros(len(self.keys), dtype=torch.float64, device=self.device)
        self.count = torch.zeros(1, dtype=torch.float64, device=self.device)

    def _prepare(self, values) -> None:
        if self.sums is not None:
            return
        if self.keys is None:
            self.keys = [k for k, v in values.items() if isinstance(v, (float, int)) or (isinstance(v, torch.Tensor) and v.dim() == 0)]
        if self.device is None:
            tens = [v for v in values.values() if isinstance(v, torch.Tensor)]
            self.device = tens[0].device if tens else torch.device("cpu")
        self._allocate()

    def reset(self) -> None:
        if self.sums is not None:
            self.sums.zero_()
            self.count.zero_()

    def update(self, values: Dict[str, object], n: float = 1.0) -> None:
        self._prepare(values)
        vals = []
        for k in self.keys:
            v = values[k]
            if isinstance(v, torch.Tensor):
                if v.numel() != 1:
                    raise NotImplementedError("invalid data {}: shape {}".format(k, tuple(v.shape)))
                vals.append(v.detach().reshape(()).to(device=self.device, dtype=torch.float64))
            elif isinstance(v, (float, int)):
                vals.append(torch.full((), float(v), dtype=torch.float64, device=self.device))
            else:
                raise NotImplementedError("invalid data {}: {}".format(k, type(v)))
        self.sums += torch.stack(vals)
        self.count += float(n)

    def slot(self, names: Sequence[str]):
        """The contiguous slice of the sums that holds ``names`` in this order (for the fused update), or an error."""
        names = list(names)
        if self.sums is None:
            if self.keys is None:
                self.keys = names
            if self.device is None:
                raise ValueError("DeviceAverageMeter: give a device before the first fused update")
            self._allocate()
        try:
            i = self.keys.index(names[0])
        except ValueError:
            i = -1
        if i < 0 or self.keys[i:i + len(names)] != names:
            raise ValueError("DeviceAverageMeter: keys %s do not hold %s in this order" % (self.keys, names))
        return self.sums[i:i + len(names)]

    def mean(self) -> Dict[str, float]:
        if self.sums is None:
            return {}
        host = torch.cat([self.sums, self.count]).cpu().tolist()                          # the one copy
        return {k: v / host[-1] for k, v in zip(self.keys, host[:-1])}

    def mean_tensors(self) -> Dict[str, torch.Tensor]:
        """The means as 0-dim fp32 tensors on the meter's device (what ``_valid_epoch`` returns, trainer ``:279-280``)."""
        if self.sums is None:
            return {}
        m = (self.sums / self.count).to(torch.float32)
        return {k: m[i] for i, k in enumerate(self.keys)}


def _as_maps(depth_est, depth_gt, mask):
    """The reference's arguments -> ``[B,1,N]`` fp32 est / gt and an fp32 or byte mask, contiguous (``compute_metrics_for_each_image`` walks
    dimension 0)."""
    for name, t in (("depth_est", depth_est), ("depth_gt", depth_gt), ("mask", mask)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise MvsHipError("%s must be a GPU tensor: the MI355X HIP path is the only implementation (no CPU fallback)" % name)
    if depth_est.shape != depth_gt.shape or mask.shape != depth_gt.shape or depth_gt.dim() < 2:
        raise MvsHipError("depth metrics: shapes %s %s %s" % (tuple(depth_est.shape), tuple(depth_gt.shape), tuple(mask.shape)))
    B = depth_gt.shape[0]
    est = depth_est.detach().to(torch.float32).contiguous().view(B, 1, -1)
    gt = depth_gt.detach().to(torch.float32).contiguous().view(B, 1, -1)
    if mask.dtype not in (torch.bool, torch.uint8):
        mask = mask.detach().to(torch.float32)
    return est, gt, mask.detach().contiguous().view(B, 1, -1)


@torch.no_grad()
def depth_metrics(depth_est, depth_gt, mask, thresholds=None, *, depth_interval=None, multipliers=(), per_sample_interval=False, band=None,
                  names=None, meter: Optional[DeviceAverageMeter] = None, n: float = 1.0) -> Dict[str, torch.Tensor]:
    """All metrics of a batch in one call.  ``thresholds``: a device tensor ``[B,K]`` or ``[K]``, or None with ``depth_interval [B]`` and
    ``multipliers`` (:func:`build_thresholds`); ``band``: ``AbsDepthError_metrics``' ``thres=(lo, hi)``.  -> ``abs_depth_error`` and one
    entry per threshold (``names``; ``thres<m>mm_error`` for multipliers, ``thres_<k>`` otherwise) as 0-dim fp32 batch means, and
    ``valid_count [B]``, ``band_count [B]``, ``exceed_count [B,K]`` (int32, exact), ``per_image [B,1+K]``, ``batch [1+K]``, ``thresholds``.
    ``meter``: advanced by these batch means (and ``n``) by the same call's last launch."""
    est, gt, msk = _as_maps(depth_est, depth_gt, mask)
    B = est.shape[0]
    if thresholds is not None:
        thr = thresholds.detach().to(device=est.device, dtype=torch.float32)
        thr = (thr.unsqueeze(0).expand(B, -1) if thr.dim() == 1 else thr).contiguous()
        default = ["thres_%d" % k for k in range(thr.shape[1])]
    elif len(multipliers):
        if depth_interval is None:
            raise ValueError("depth_metrics: multipliers need depth_interval")
        thr = build_thresholds(depth_interval.to(est.device), multipliers, per_sample_interval, B)
        default = threshold_names(multipliers)
    else:
        thr, default = None, []
    names = default if names is None else list(names)
    K = 0 if thr is None else thr.shape[1]
    if len(names) != K:
        raise ValueError("depth_metrics: %d names for %d thresholds" % (len(names), K))
    sums = count = None
    if meter is not None:
        if meter.device is None:
            meter.device = est.device
        sums, count = meter.slot([ABS_KEY] + names), None
        count = meter.count
    counts, per_image, batch = ops.depth_metrics(est, gt, msk, thr, band=band, meter_sums=sums, meter_count=count, meter_n=float(n))
    out = {ABS_KEY: batch[0]}
    for k, name in enumerate(names):
        out[name] = batch[1 + k]
    out.update(valid_count=counts[:, 0], band_count=counts[:, 1], exceed_count=counts[:, 2:], per_image=per_image, batch=batch, thresholds=thr)
    return out


@torch.no_grad()
def Thres_metrics(depth_est, depth_gt, mask, thres):
    """utils.py:162-169: the batch mean of the per-image share of valid pixels with ``|est - gt| > thres`` (fp32, strict)."""
    assert isinstance(thres, (int, float))
    est, gt, msk = _as_maps(depth_est, depth_gt, mask)
    thr = torch.full((est.shape[0], 1), float(thres), dtype=torch.float32, device=est.device)
    return ops.depth_metrics(est, gt, msk, thr)[2][1]


@torch.no_grad()
def AbsDepthError_metrics(depth_est, depth_gt, mask, thres=None):
    """utils.py:173-182: the batch mean of the per-image mean abs error over the valid pixels (inside ``thres = (lo, hi)`` if given)."""
    est, gt, msk = _as_maps(depth_est, depth_gt, mask)
    band = None if thres is None else (float(thres[0]), float(thres[1]))
    return ops.depth_metrics(est, gt, msk, None, band=band)[2][0]


def _to_device(x, device):
    if isinstance(x, torch.Tensor):
        return x if x.device == device else x.to(device, non_blocking=True)
    if isinstance(x, dict):
        return {k: _to_device(v, device) for k, v in x.items()}
    return x


@torch.no_grad()
def valid_epoch(model, data_loader, *, blended: bool = False, multipliers: Sequence[float] = VALID_MULTIPLIERS) -> Dict[str, torch.Tensor]:
    """The body of ``_valid_epoch`` (trainer ``:216-283``) for one loader: ``model.eval()``, the fp32 eval forward, ``refined_depth`` against
    ``depth['stage4']`` / ``mask['stage4']`` with the DTU thresholds (or, ``blended``, each sample's own interval) into a meter, and
    ``mean_error`` = the mean of the threshold entries.  -> 0-dim fp32 device tensors (the trainer's ``all_reduce`` loop takes them as they
    are); no host synchronisation per batch; a model that was training is training again afterwards."""
    was_training = model.training
    model.eval()
    try:
        device = next(model.parameters()).device
        names = threshold_names(multipliers)
        meter = DeviceAverageMeter([ABS_KEY] + names, device)
        for sample in data_loader:
            sample = _to_device(sample, device)
            depth_gt, mask = sample["depth"]["stage4"], sample["mask"]["stage4"]
            depth_values = sample["depth_values"]
            depth_interval = depth_values[:, 1] - depth_values[:, 0]
            outputs = model.forward(sample["imgs"], sample["proj_matrices"], depth_values)
            depth_metrics(outputs["refined_depth"].detach(), depth_gt, mask, depth_interval=depth_interval, multipliers=multipliers,
                          per_sample_interval=blended, meter=meter)
        m64 = meter.sums / meter.count
        out = {k: m64[i].to(torch.float32) for i, k in enumerate(meter.keys)}
        err = m64[1]
        for i in range(2, len(meter.keys)):                  # trainer :274-275: left to right in double, then / 4.0
            err = err + m64[i]
        out["mean_error"] = (err / float(len(names))).to(torch.float32)
        return out
    finally:
        if was_training:
            model.train()


def write_depth_metric_txt(path, means: Dict[str, float]) -> None:
    """``depth_metric.txt`` in the line format of test.py:325-327."""
    with open(path, "w") as w:
        for k in means:
            w.write(k + " " + str(means[k]) + "\n")
