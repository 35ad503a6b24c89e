"""AdamW on the HIP path: ``torch.optim.AdamW``'s update (the reference's optimizer, train.py:98) for all parameter tensors of a group in
a few launches of ``mvs_adamw_step`` (csrc/optim.hip) instead of ATen's multi-tensor kernel.

Same constructor arguments as ``torch.optim.AdamW`` where they apply.  State: ``exp_avg``, ``exp_avg_sq`` per parameter; the step count is
ONE device scalar per group (``param_groups[i]['step']``, fp32), advanced by the kernel, so ``step()`` is capturable in a hipGraph as it is.
``state_dict()`` ALSO carries torch's per-parameter ``'step'`` (a copy of the group's count), so the checkpoint loads into
``torch.optim.AdamW`` and back; ``load_state_dict()`` accepts both layouts (the reference resumes with ``torch.load(map_location='cpu')`` +
``optimizer.load_state_dict``, train.py:110-117): the group's count is moved to the parameters' device, or seeded from the per-parameter
counts of a ``torch.optim.AdamW`` / reference checkpoint (which must agree within a group).
fp32 contiguous GPU parameters only; ``amsgrad`` and sparse gradients are not built; there is no CPU path.

Two forms of ``step()``:

* ``device_hyper=False`` (default): one launch set of ``mvs_adamw_step`` per parameter group; the scalar hyper-parameters (``lr``, betas,
  ``eps``, ``weight_decay``) travel as kernel arguments, so a hipGraph captures them BY VALUE: a learning-rate schedule needs a re-capture
  when the rate changes (or the eager ``step()``).  The step count is read from the device and does advance in a replay.
* ``device_hyper=True``: the reference's training recipe (train.py:78-100, trainer/mvsformer_trainer.py:39-45, 157-167: layer-wise groups, a
  ``LambdaLR`` stepped after every step, a ``GradScaler``, global-norm clipping) inside ONE capture.  The groups' hyper-parameters live in a
  device table that ``sync_hyper()`` refreshes with one small host-to-device copy when a scheduler has written ``group['lr']`` (an eager
  ``step()`` calls it; a captured step gets it through ``CapturedStep(before_replay=[opt.sync_hyper])``); the tensors of all groups share
  the launches of ``mvs_adamw_multi`` (their number does not depend on the number of groups); ``max_grad_norm`` and a ``GradScaler``'s
  ``grad_scale`` / ``found_inf`` are folded into one multiplier and one skip flag on the device by ``mvs_grad_norm`` - no ``.item()``, no
  host branch.  Extra keys of a group (``lr_scale``, ``vit_param``, ``initial_lr``) are carried and ignored as ``torch.optim.AdamW``
  ignores them: the reference hands its ``lr_scale`` groups to plain AdamW + ``LambdaLR`` and never applies the scale.

  Deliberate difference to torch: a non-finite gradient norm WITHOUT a ``GradScaler`` makes ``clip_grad_norm_`` + ``AdamW.step`` write NaN
  into every parameter; here the step is skipped (parameters, moments and counts keep their bits) and the device counter
  ``skipped_steps`` is incremented.

``clip_grad_norm_`` is the stand-alone form of the norm (torch's semantics, gradients scaled in place) for a trainer that keeps its
``torch.nn.utils.clip_grad_norm_`` line; ``vit_param_groups`` builds the layer-wise groups of the reference's ``models/lr_decay.py``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ops


HYPER_KEYS = ("lr", "weight_decay", "betas", "eps", "maximize")


def _fill_entries(items, need_state):
    """``items``: (parameter or None, gradient, exp_avg, exp_avg_sq, group index) -> the host table of ``MvsAdamEntry``."""
    arr = (_lib.AdamEntry * len(items))()
    for k, (p, g, m, v, gi) in enumerate(items):
        t = arr[k]
        t.g, t.n, t.group, t.reserved = g.data_ptr(), g.numel(), gi, 0
        if need_state:
            t.p, t.m, t.v = p.data_ptr(), m.data_ptr(), v.data_ptr()
    return arr


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False,
                 device_hyper=False, max_grad_norm=None):
        if amsgrad:
            raise _lib.MvsHipError("FusedAdamW: amsgrad is not built")
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdamW: lr %r, betas %r, eps %r, weight_decay %r" % (lr, betas, eps, weight_decay))
        if max_grad_norm is not None and not device_hyper:
            raise _lib.MvsHipError("FusedAdamW: max_grad_norm needs device_hyper=True (the clip coefficient is a device scalar of that path)")
        if max_grad_norm is not None and not float(max_grad_norm) == float(max_grad_norm):
            raise ValueError("FusedAdamW: max_grad_norm is NaN")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize))
        self.device_hyper = bool(device_hyper)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._dev = None                                     # device arrays of the device_hyper path, made at first use
        self._host_rows = None                               # what the device table holds
        if self.device_hyper:
            self._step_supports_amp_scaling = True           # torch.amp.GradScaler.step: grad_scale / found_inf are consumed on the device

    def state_dict(self):
        sd = super().state_dict()
        packed = {id(p): i for i, p in enumerate(q for g in self.param_groups for q in g["params"])}
        for g_live, g_out in zip(self.param_groups, sd["param_groups"]):
            if "step" not in g_live:
                continue
            count = g_live["step"].detach().to("cpu", torch.float32).clone()
            g_out["step"] = count
            for p in g_live["params"]:
                idx = packed[id(p)]
                st = sd["state"].get(idx)
                if st is not None:
                    st = sd["state"][idx] = dict(st)         # torch hands out the LIVE per-parameter dict: the count goes into a copy
                    st["step"] = count.clone()               # torch.optim.AdamW's layout: one count per parameter
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            params = [p for p in group["params"]]
            if not params:
                continue
            dev = params[0].device
            counts = {float(self.state[p]["step"]) for p in params if p in self.state and "step" in self.state[p]}
            if "step" in group and group["step"] is not None:
                group["step"] = torch.as_tensor(group["step"], dtype=torch.float32).detach().to(dev).reshape(())
            elif counts:
                if len(counts) != 1:
                    raise _lib.MvsHipError("FusedAdamW.load_state_dict: the parameters of one group carry different step counts %s (one count per group here)"
                                           % sorted(counts))
                group["step"] = torch.tensor(counts.pop(), device=dev, dtype=torch.float32)
            elif any(p in self.state and self.state[p] for p in params):
                raise _lib.MvsHipError("FusedAdamW.load_state_dict: moments without a step count: the bias corrections would restart at 1")
            for p in params:                                 # the per-parameter copies are not state here
                if p in self.state:
                    self.state[p].pop("step", None)
        if self.device_hyper and all(p.is_cuda for g in self.param_groups for p in g["params"]):
            self._device_state()                             # the loaded counts move into the device array now, not inside a later capture

    # ------------------------------------------------------------------------------------------- device_hyper=True
    def _device_state(self):
        """The device arrays of the ``device_hyper`` path: ``hyper`` [groups][8], ``steps`` [groups] (``param_groups[i]['step']`` is the view
        ``steps[i]``), ``ctl_f`` = (gradient norm, gradient multiplier), ``ctl_i`` = (skip flag, skipped steps)."""
        if not self.device_hyper:
            raise _lib.MvsHipError("FusedAdamW: built with device_hyper=False: there is no device table")
        n = len(self.param_groups)
        d = self._dev
        if d is None or d["steps"].numel() != n:
            params = [p for g in self.param_groups for p in g["params"]]
            if not params or not all(p.is_cuda and p.device == params[0].device for p in params):
                raise _lib.MvsHipError("FusedAdamW: fp32 dense GPU parameters of one device: the MI355X HIP path is the only implementation")
            dev = params[0].device
            skipped = d["ctl_i"] if d is not None else torch.zeros(2, device=dev, dtype=torch.int32)
            d = self._dev = dict(device=dev, steps=torch.zeros(n, device=dev, dtype=torch.float32),
                                 hyper=torch.zeros(n, _lib.ADAM_HYPER_STRIDE, device=dev, dtype=torch.float32),
                                 ctl_f=torch.zeros(2, device=dev, dtype=torch.float32), ctl_i=skipped, workspace=None)
            self._host_rows = None
        steps = d["steps"]
        for i, group in enumerate(self.param_groups):
            cur = group.get("step")
            if isinstance(cur, torch.Tensor) and cur.is_cuda and cur.dtype == torch.float32 and cur.dim() == 0 \
                    and cur.data_ptr() == steps.data_ptr() + 4 * i:
                continue
            if torch.cuda.is_current_stream_capturing():
                raise _lib.MvsHipError("FusedAdamW: param_groups[%d]['step'] is not in the device array yet: run one eager step() (or load_state_dict) before the capture" % i)
            if cur is not None:
                if not (isinstance(cur, torch.Tensor) and cur.is_cuda and cur.device == d["device"] and cur.dtype == torch.float32 and cur.numel() == 1):
                    raise _lib.MvsHipError("FusedAdamW: param_groups[..]['step'] must be one fp32 scalar on %s (got %r): load checkpoints through load_state_dict"
                                           % (d["device"], cur))
                steps[i].copy_(cur.detach().reshape(()))
            group["step"] = steps[i]
        return d

    def sync_hyper(self):
        """Brings the device table up to ``param_groups[i]['lr' | 'weight_decay' | 'betas' | 'eps' | 'maximize']``: if anything changed since
        the last call, ONE host-to-device copy from a pinned staging tensor on the current stream (no synchronisation).  Returns whether a
        copy was enqueued.  Call it after a scheduler's ``step()`` and before the replay of a captured step (``CapturedStep(before_replay=
        [opt.sync_hyper])``); an eager ``step()`` calls it itself."""
        d = self._device_state()
        rows = []
        for g in self.param_groups:
            lr, wd, (b1, b2), eps = float(g["lr"]), float(g["weight_decay"]), g["betas"], float(g["eps"])
            b1, b2 = float(b1), float(b2)
            if not (lr >= 0.0 and eps >= 0.0 and wd >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
                raise ValueError("FusedAdamW: lr %r, betas %r, eps %r, weight_decay %r" % (lr, (b1, b2), eps, wd))
            rows.append((lr, wd, b1, b2, eps, 1.0 if g["maximize"] else 0.0, 0.0, 0.0))
        if rows == self._host_rows:
            return False
        # a fresh pinned tensor per refresh: torch's host allocator hands its block out again only after this copy has run, so a host
        # that is several replays ahead of the GPU never overwrites a row that is still to be read
        staging = torch.tensor(rows, dtype=torch.float32).pin_memory()
        d["hyper"].copy_(staging, non_blocking=True)
        self._host_rows = rows
        return True

    @property
    def hyper_table(self):
        """The device table [groups][8]: lr, weight_decay, beta1, beta2, eps, maximize, 0, 0."""
        return self._device_state()["hyper"]

    @property
    def grad_norm(self):
        """0-dim fp32 device tensor: the norm of the (unscaled) gradients of the last step that computed one."""
        return self._device_state()["ctl_f"][0]

    @property
    def skipped_steps(self):
        """0-dim int32 device tensor: steps skipped because of an overflow flag or a non-finite gradient norm."""
        return self._device_state()["ctl_i"][1]

    def _step_device_hyper(self):
        d = self._device_state()
        if not torch.cuda.is_current_stream_capturing():
            self.sync_hyper()
        elif self._host_rows is None:
            raise _lib.MvsHipError("FusedAdamW: the device table is empty: run one eager step() or sync_hyper() before the capture")
        dev = d["device"]
        items = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_cuda or p.device != dev or g.is_sparse:
                    raise _lib.MvsHipError("FusedAdamW: fp32 dense GPU parameters of one device (got %s / %s on %s)" % (p.dtype, g.dtype, p.device))
                if not p.is_contiguous():
                    raise _lib.MvsHipError("FusedAdamW: a parameter is not contiguous")
                if not g.is_contiguous():
                    g = p.grad = g.contiguous()
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                items.append((p, g, st["exp_avg"], st["exp_avg_sq"], gi))
        if not items:
            return
        arr = _fill_entries(items, True)
        tab = ctypes.cast(arr, ctypes.c_void_p)
        scale, found = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        for name, t in (("grad_scale", scale), ("found_inf", found)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.numel() == 1):
                raise _lib.MvsHipError("FusedAdamW: %s must be one fp32 scalar on %s (got %r)" % (name, dev, t))
        gmul = skip = None
        if self.max_grad_norm is not None or scale is not None or found is not None:
            need = _lib.load().mvs_grad_norm_workspace_bytes(tab, len(items))
            if need < 0:
                raise _lib.MvsHipError("mvs_grad_norm_workspace_bytes refused the tensor table")
            if d["workspace"] is None or d["workspace"].numel() * 8 < need:
                d["workspace"] = torch.empty(need // 8, device=dev, dtype=torch.float64)
            gmul, skip = d["ctl_f"][1:].data_ptr(), d["ctl_i"].data_ptr()
            ops._call("mvs_grad_norm", "grad_norm", tab, len(items), float(self.max_grad_norm or 0.0), ops._ptr(scale), ops._ptr(found),
                      d["workspace"].data_ptr(), d["ctl_f"].data_ptr(), gmul, skip, ops._stream())
        ops._call("mvs_adamw_multi", "adamw_multi", tab, len(items), d["hyper"].data_ptr(), len(self.param_groups), d["steps"].data_ptr(),
                  gmul, skip, d["ctl_i"][1:].data_ptr(), ops._stream())
        ops.bump_weights_epoch()                             # parameters written through raw pointers: torch's _version does not move

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.device_hyper:
            self._step_device_hyper()
            return loss
        if getattr(self, "grad_scale", None) is not None or getattr(self, "found_inf", None) is not None:
            raise _lib.MvsHipError("FusedAdamW: AMP scaling (grad_scale / found_inf) needs device_hyper=True")
        for group in self.param_groups:
            todo = [p for p in group["params"] if p.grad is not None]
            if not todo:
                continue
            dev = todo[0].device
            if "step" not in group:
                group["step"] = torch.zeros((), device=dev, dtype=torch.float32)
            cnt = group["step"]
            if not (isinstance(cnt, torch.Tensor) and cnt.is_cuda and cnt.device == dev and cnt.dtype == torch.float32 and cnt.numel() == 1):
                raise _lib.MvsHipError("FusedAdamW: param_groups[..]['step'] must be one fp32 scalar on %s (got %r): load checkpoints through load_state_dict" % (dev, cnt))
            arr = (_lib.AdamTensor * len(todo))()
            for k, p in enumerate(todo):
                g = p.grad
                if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_cuda or p.device != dev or g.is_sparse:
                    raise _lib.MvsHipError("FusedAdamW: fp32 dense GPU parameters of one device (got %s / %s on %s)" % (p.dtype, g.dtype, p.device))
                if not p.is_contiguous():
                    raise _lib.MvsHipError("FusedAdamW: a parameter is not contiguous")
                if not g.is_contiguous():
                    g = p.grad = g.contiguous()
                st = self.state[p]
                if not st:
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                t = arr[k]
                t.p, t.g, t.m, t.v, t.n = p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
            b1, b2 = group["betas"]
            ops._call("mvs_adamw_step", "adamw", ctypes.cast(arr, ctypes.c_void_p), len(todo), float(group["lr"]), float(b1), float(b2),
                      float(group["eps"]), float(group["weight_decay"]), int(bool(group["maximize"])), group["step"].data_ptr(), ops._stream())
            ops.bump_weights_epoch()                         # parameters written through raw pointers: torch's _version does not move
        return loss


def clip_grad_norm_(parameters, max_norm):
    """``torch.nn.utils.clip_grad_norm_(parameters, max_norm)`` for ``norm_type=2``, ``error_if_nonfinite=False`` (the reference's
    ``trainer.grad_norm``, trainer/mvsformer_trainer.py:157-160) in three launch sets: ``mvs_grad_norm`` (blocks of 2048 values summed in
    double, then one block over the partials: no atomics, the same bits every run) and ``mvs_grad_scale_``.  Returns the total norm as a 0-dim
    device tensor; the gradients are multiplied by ``min(1, max_norm / (norm + 1e-6))`` in place.  fp32 dense GPU gradients of one device."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.tensor(0.0)
    dev = params[0].grad.device
    items = []
    for p in params:
        g = p.grad
        if not g.is_cuda or g.device != dev or g.dtype != torch.float32 or g.is_sparse:
            raise _lib.MvsHipError("clip_grad_norm_: fp32 dense GPU gradients of one device (got %s on %s): there is no CPU path" % (g.dtype, g.device))
        if not g.is_contiguous():
            g = p.grad = g.contiguous()
        items.append((None, g, None, None, 0))
    arr = _fill_entries(items, False)
    tab = ctypes.cast(arr, ctypes.c_void_p)
    need = _lib.load().mvs_grad_norm_workspace_bytes(tab, len(items))
    if need < 0:
        raise _lib.MvsHipError("mvs_grad_norm_workspace_bytes refused the tensor table")
    with torch.cuda.device(dev):
        work = torch.empty(need // 8, device=dev, dtype=torch.float64)
        out = torch.empty(2, device=dev, dtype=torch.float32)    # norm, multiplier
        ops._call("mvs_grad_norm", "grad_norm", tab, len(items), float(max_norm), None, None, work.data_ptr(), out.data_ptr(), out[1:].data_ptr(),
                  None, ops._stream())
        ops._call("mvs_grad_scale_", "grad_scale", tab, len(items), out[1:].data_ptr(), ops._stream())
    return out[0]


def _vit_layer_id(name, depth):
    """Layer of a ViT parameter for the layer-wise decay: the embeddings are layer 0, ``blocks.i`` is layer i + 1, ``cross_blocks`` get
    -1 (their own fixed scale), everything else (the final norm) the last layer ``depth``."""
    if name in ("cls_token", "pos_embed") or name.startswith("patch_embed"):
        return 0
    if name.startswith("cross_blocks"):
        return -1
    if name.startswith("blocks"):
        return int(name.split(".")[1]) + 1
    return depth


def vit_param_groups(vit, vit_lr, weight_decay=0.05, no_weight_decay_list=(), layer_decay=0.75):
    """The layer-wise parameter groups the reference builds for a fine-tuned ViT (``param_groups_lrd``, models/lr_decay.py:13-83; train.py:
    86-90): one group per (layer, decayed or not) in order of first appearance; 1-D parameters and the names of ``no_weight_decay_list`` get
    ``weight_decay`` 0; ``lr_scale`` = ``layer_decay ** (depth - layer)`` with depth = blocks + 1 (10 for ``cross_blocks``).  Keys as the
    reference's: ``lr``, ``lr_scale``, ``weight_decay``, ``params``, ``vit_param``.  ``lr_scale`` is information only: neither the reference's
    ``torch.optim.AdamW`` + ``LambdaLR`` nor ``FusedAdamW`` applies it."""
    depth = len(vit.blocks) + 1
    groups = {}
    for name, p in vit.named_parameters():
        if not p.requires_grad:
            continue
        decayed = not (p.ndim == 1 or name in no_weight_decay_list)
        layer = _vit_layer_id(name, depth)
        key = (layer, decayed)
        if key not in groups:
            groups[key] = dict(lr=vit_lr, lr_scale=10.0 if layer == -1 else layer_decay ** (depth - layer),
                               weight_decay=weight_decay if decayed else 0.0, params=[], vit_param=True)
        groups[key]["params"].append(p)
    return list(groups.values())
