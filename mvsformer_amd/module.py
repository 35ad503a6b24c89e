"""Host-side mirror of the hot-path symbols of the reference's ``models/module.py``.

Same class names, constructor signatures, forward signatures and ``state_dict`` keys as the reference
(models/module.py:83-165 ``Conv3d``/``Deconv3d``, :168-197 ``ConvBnReLU``, :469-505 ``CostRegNet``, :550-594
``CostRegNet3D``, :597-619 ``depth_regression``/``conf_regression``, :633-653 the inverse-depth schedulers), so a
reference checkpoint loads with ``strict=True`` and ``models/mvsformer_model.py`` can use them unchanged.  The
``nn.Conv3d`` / ``nn.BatchNorm3d`` children are parameter holders only (they keep ``.to()``, ``state_dict()``,
DDP and SyncBatchNorm conversion working); every forward runs the hand-written HIP kernels of
``libmvs_hip.so`` through :mod:`mvsformer_amd.ops`.  There is no PyTorch/CPU fallback.

Eval-mode BatchNorm is folded into a per-channel ``scale``/``shift`` pair applied in the conv epilogue;
folded parameters and the MFMA-friendly weight packing are cached and rebuilt when a parameter or a pack-time switch changes.
Training mode (``module.train()``) runs raw conv -> batch-statistics BatchNorm -> ReLU (+ skip) through the autograd
functions of :mod:`mvsformer_amd.autograd`, whose forward and backward are HIP kernels as well.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import ops, switches as sw
from ._lib import MvsHipError
from .switches import SMALL_MAX_WORK, _parse_small_limit


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _bn_fold(bn: nn.modules.batchnorm._BatchNorm) -> Tuple[torch.Tensor, torch.Tensor]:
    """Eval BatchNorm as y = x*scale + shift (fp32, on the module's device)."""
    var = bn.running_var.detach().to(torch.float32)
    mean = bn.running_mean.detach().to(torch.float32)
    g = bn.weight.detach().to(torch.float32) if bn.weight is not None else torch.ones_like(var)
    b = bn.bias.detach().to(torch.float32) if bn.bias is not None else torch.zeros_like(var)
    scale = g / torch.sqrt(var + bn.eps)
    return scale.contiguous(), (b - mean * scale).contiguous()


def _versions(*mods: Optional[nn.Module]) -> tuple:
    """Cache key of everything derived from the modules' parameters / buffers: torch's (data_ptr, _version) per tensor + the epoch of
    raw-pointer writes (``ops.bump_weights_epoch``: FusedAdamW, training-mode BatchNorm kernels, replayed hipGraphs)."""
    return (ops.weights_epoch(),) + tuple((t.data_ptr(), t._version) for m in mods if m is not None for t in list(m.parameters()) + list(m.buffers()))


def _publish_cache() -> None:
    """Packed weights / folded BatchNorm are produced by kernels on the CURRENT stream and then reused by every later
    forward, possibly on other streams (bench.py walks reference views over several).  The cache is rebuilt only when a
    parameter changes, so one stream synchronization per rebuild makes the cached tensors safe to read from any stream."""
    if torch.cuda.is_available():
        torch.cuda.current_stream().synchronize()


def autocast_bf16() -> bool:
    """True inside ``torch.autocast('cuda', dtype=torch.bfloat16)`` (how BASELINE configs[2] trains; the reference trainer wraps
    the model in ``torch.cuda.amp.autocast``, trainer/mvsformer_trainer.py:104-106) or with MVS_TRAIN_BF16=1: the regularizer
    then runs on bf16 channel-last activations and the bf16 matrix cores."""
    if sw.flag("MVS_TRAIN_BF16"):
        return True
    try:
        if hasattr(torch, "get_autocast_dtype"):
            return torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
        return torch.is_autocast_enabled() and torch.get_autocast_gpu_dtype() == torch.bfloat16
    except Exception:                                                    # noqa: BLE001 - torch builds without these queries
        return False


def _multi_use(t, link=None):
    """A training-layer output that feeds more than one consumer (a skip connection) or a consumer of another kind (the head): its
    BatchNorm's backward sums cannot be taken by ONE consumer's data gradient (autograd.LayerBf16Fn) - drop the tag that offers it.
    With a ``link`` (autograd.SkipLink) the strided consumer's data gradient WILL be the tensor's total gradient: the tag stays."""
    if link is None and hasattr(t, "_mvs_bn"):
        del t._mvs_bn
    return t


def _skip_links(x, n=3):
    """``n`` SkipLinks for one forward of a U-Net on the fused bf16 training layers, else Nones (MVS_TRAIN_SKIPLINK=0: autograd adds)."""
    from . import autograd as ag
    if x.dtype == torch.bfloat16 and ag._fused_layers() and sw.flag("MVS_TRAIN_SKIPLINK"):
        return tuple(ag.SkipLink() for _ in range(n))
    return (None,) * n


def _train_conv_bn_act(x, conv, bn, relu, residual, transposed_sd=None, take=None, give=None):
    """Training-mode layer: raw (transposed) conv -> batch-stat BN -> ReLU (+ residual), all autograd-tracked HIP ops.
    bf16 channel-last input (``[B,D,H,W,C]``) selects the bf16 kernels, fp32 ``[B,C,D,H,W]`` the fp32 ones."""
    from . import autograd as ag
    if x.dtype == torch.bfloat16:
        if conv.bias is not None or bn is None:
            raise MvsHipError("bf16 training layer without BatchNorm / with bias is not built")
        # MVS_BN_FUSED_STATS=1: the convolution's epilogue takes the batch statistics of its output instead of a separate pass over y.
        # Measured 13.5 vs 13.3 ms per step (one partial row per wavefront makes the fixed-order reduce long): off by default.
        fused = 1 if sw.flag("MVS_BN_FUSED_STATS") else 0
        pk = ag.packed_of(conv)                              # this step's layouts if the stage's StagePack made them (one launch per stage)
        if ag._fused_layers() and not ag._bn_synced(bn):
            # statistics stay on this rank: the whole layer is one autograd node (conv with the statistics in its epilogue -> finalize ->
            # normalize): 8 graph nodes per layer and step instead of 11
            if transposed_sd is None:
                s = tuple(conv.stride)
                return ag.LayerBf16Fn.apply(x, ag.route_of(conv), bn.weight, bn.bias, residual, bn, bool(relu), 0, (s[0], s[1]), 1, pk, take, give)
            return ag.LayerBf16Fn.apply(x, ag.route_of(conv), bn.weight, bn.bias, residual, bn, bool(relu), 1, (transposed_sd, 2), 1, pk, take, give)
        if take is not None:
            _multi_use(x)                                    # no hand-over on the unfused chain: the tag (if any) must not promise one
        if transposed_sd is None:
            s = tuple(conv.stride)
            out = ag.ConvBf16Fn.apply(x, ag.route_of(conv), (s[0], s[1]), fused, pk)
        else:
            out = ag.DeconvBf16Fn.apply(x, ag.route_of(conv), transposed_sd, fused, pk)
        y, sums = out if fused else (out, None)
        return ag.BnActBf16Fn.apply(y, bn.weight, bn.bias, residual, bn, bool(relu), 1, sums)
    if transposed_sd is None:
        s = tuple(conv.stride)
        y = ag.ConvFn.apply(x, conv.weight, (s[0], s[1]))
    else:
        y = ag.DeconvFn.apply(x, conv.weight, transposed_sd)
    if conv.bias is not None:
        raise MvsHipError("training-mode conv with bias (bn=False) is not built")
    if bn is None:
        raise MvsHipError("training-mode layer without BatchNorm is not built")
    return ag.BnActFn.apply(y, bn.weight, bn.bias, residual, bn, bool(relu))


# ---------------------------------------------------------------------------------------------------------
# layer holders (reference models/module.py:83-165, 168-197); first, which kernel serves one in eval mode: pure functions of plain values
# ---------------------------------------------------------------------------------------------------------
_SMALL_LIMITS = _parse_small_limit(sw.text("MVS_CONV_SMALL_MAX_WORK"))      # (Conv3d, Deconv3d); read once: not on every forward of every layer
_WINDOW = 1 << 31        # bytes a buffer descriptor of the split-form kernels addresses


class RouteSwitches(NamedTuple):
    """The switch values one eval forward of a regularizer routes by (read once per forward, :func:`route_switches`)."""
    min_voxels: int = sw.TABLE["MVS_CONV_X3_MIN_VOXELS"].default      # output voxels from which a layer takes the split form
    small_limit: Tuple[int, int] = SMALL_MAX_WORK      # (Conv3d, Deconv3d)
    conv_x3: str = "1"                                 # MVS_CONV_X3: "0" off, "strided" / "s1" one kind of convolution only (diagnostics)
    conv_wino: Optional[str] = None                    # MVS_CONV_WINO: "1" packs the Winograd form of the stride-1 convolutions
    tail: str = "x3"                                   # MVS_TAIL
    fuse_prob: bool = True                             # MVS_FUSE_PROB


def route_switches() -> RouteSwitches:
    return RouteSwitches(sw.integer("MVS_CONV_X3_MIN_VOXELS"), _SMALL_LIMITS, sw.text("MVS_CONV_X3"), sw.text("MVS_CONV_WINO"),
                         sw.text("MVS_TAIL"), sw.flag("MVS_FUSE_PROB"))


def _small_limit(rs: RouteSwitches, transposed: bool) -> int:
    return 0 if rs.conv_x3 == "0" else rs.small_limit[1 if transposed else 0]      # MVS_CONV_X3=0 turns every split form off


def conv_route(cin, cout, stride, in_shape, forms, rs: RouteSwitches, wino_ok: bool = False) -> str:
    """Kernel of a 3x3x3 convolution with ``stride = (depth, height/width)`` on an input of ``in_shape = (D, H, W)`` voxels per channel.
    ``forms``: the packed forms the layer has; ``wino_ok``: ``ops.conv3d_wino_supported`` of the shape."""
    D, H, W = in_shape
    # 3-term bf16 split form (csrc/conv3d_x3.hip: fp32-equivalent, bf16 matrix cores) from min_voxels output voxels up - below that the launch
    # is too small to fill the chip with its 16 x 16 x D tiles and the fp32-MFMA kernel wins.  (The count floors H and W by the stride.)
    # A sample beyond the kernel's 2 GiB buffer window falls through to the 64-bit-addressed fp32-MFMA kernel.
    if "x3" in forms and rs.conv_x3 != "0" and D * (H // stride[1]) * (W // stride[1]) >= rs.min_voxels and cin * D * H * W * 4 < _WINDOW:
        return "x3"
    # small-volume split form (csrc/conv3d_x3_small.hip): CostRegNet's inner layers at the coarse stages, by output voxels x Cin x Cout
    if "small" in forms and ((D - 1) // stride[0] + 1) * ((H - 1) // stride[1] + 1) * ((W - 1) // stride[1] + 1) * cin * cout <= _small_limit(rs, False):
        return "small"
    if "wino" in forms and wino_ok:                      # Winograd F(2x2,3x3) fp32 MFMA, where MVS_CONV_WINO=1 packed it
        return "wino"
    return "fp32"


def deconv_route(cin, cout, sd, in_shape, forms, rs: RouteSwitches, x3_ok: bool = False, residual_bytes: int = 0) -> str:
    """Kernel of a 3x3x3 transposed convolution of stride ``(sd, 2, 2)``.  ``x3_ok``: ``ops.deconv3d_x3_supported`` of the layer;
    ``residual_bytes``: one sample of the skip tensor added in the epilogue (0 without one)."""
    D, H, W = in_shape
    if sd == 1:
        # split-form transposed conv (csrc/conv3d_x3.hip) where it beats the fp32-MFMA kernel: conv7 / conv9 at real sizes; 8 output channels
        # (conv11) fill half a matrix tile.  It handles column pairs, and its window is 2 GiB per input sample, 4 GiB per residual sample.
        if cout >= 16 and rs.conv_x3 != "0" and x3_ok and W % 2 == 0 and 4 * D * H * W >= rs.min_voxels \
                and cin * D * H * W * 4 < _WINDOW and residual_bytes < 2 * _WINDOW:
            return "x3"
        return "fp32"
    if "small" in forms and D * H * W * cin * cout <= _small_limit(rs, True):      # small-volume split form, by INPUT voxels x Cin x Cout
        return "small"
    return "fp32"


def tail_route(cin, cout, sd, in_shape, rs: RouteSwitches, skip_bytes: int = 0) -> str:
    """conv11 (transposed, stride ``(sd, 2, 2)``) + the 1x1x1 ``prob``: one launch or two.  ``skip_bytes``: the WHOLE batch of the skip
    volume - unlike the layers' per-sample windows, the tail kernel's descriptor covers the call."""
    D, H, W = in_shape
    if not (cout == 8 and sd == 1 and W % 4 == 0 and rs.fuse_prob):      # the fused kernels are built for 8 channels, four columns per lane
        return "unfused"
    # split form (csrc/tail_x3.hip) for the shape it is built for (16 -> 8) from min_voxels up; MVS_TAIL=fp32 keeps the fp32-MFMA tail
    if cin == 16 and rs.conv_x3 != "0" and rs.tail == "x3" and 4 * D * H * W >= rs.min_voxels and skip_bytes < _WINDOW:
        return "tail_x3"
    return "tail_fp32"


class _EvalLayer:
    """Eval-mode state of ONE 3x3x3 (transposed) convolution with its BatchNorm or bias: the check of what is built, the folded
    ``scale`` / ``shift``, the packed weight forms and the key they were made under (the tensors' versions + the pack-time switches, so a
    parameter update or an environment change rebuilds on the next forward).  Not an ``nn.Module`` - no ``state_dict`` key - and it holds no
    module either: the owner passes ``conv`` / ``bn`` in, so SyncBatchNorm conversion or a replaced child cannot leave it behind."""

    _key = None

    @staticmethod
    def check(conv) -> Tuple[int, int]:
        """-> ``(depth stride, height/width stride)`` of a layer the kernels are built for, else MvsHipError."""
        s = tuple(conv.stride)
        if isinstance(conv, nn.ConvTranspose3d):
            if tuple(conv.kernel_size) != (3, 3, 3) or tuple(conv.padding) != (1, 1, 1) or conv.groups != 1:
                raise MvsHipError("Deconv3d: only kernel 3, padding 1, groups 1 is built (got %s)" % conv)
            if (s, tuple(conv.output_padding)) not in (((2, 2, 2), (1, 1, 1)), ((1, 2, 2), (0, 1, 1))):
                raise MvsHipError("Deconv3d: stride %s / output_padding %s is not built" % (s, tuple(conv.output_padding)))
        elif tuple(conv.kernel_size) != (3, 3, 3) or tuple(conv.padding) != (1, 1, 1) or tuple(conv.dilation) != (1, 1, 1) or conv.groups != 1:
            raise MvsHipError("Conv3d: only kernel 3, padding 1, dilation 1, groups 1 is built (got %s)" % conv)
        elif s not in ((1, 1, 1), (2, 2, 2), (1, 2, 2)):
            raise MvsHipError("Conv3d: stride %s is not built" % (s,))
        return s[0], s[1]

    def _sync(self, conv, bn, rs: RouteSwitches) -> None:
        key = (_versions(conv, bn), rs.conv_x3, rs.conv_wino, rs.small_limit)
        if key == self._key:
            return
        self.transposed = isinstance(conv, nn.ConvTranspose3d)
        self.cin, self.cout, self.stride = cin, cout, s = conv.in_channels, conv.out_channels, self.check(conv)
        w = _f32c(conv.weight)
        self.forms = forms = {"fp32": ops.conv3d_pack(w, self.transposed, s[0])}
        # the split forms of the stride-(1,2,2) transposed layers (deconv x3, the tail) are packed by the first forward that routes to them
        self.x3_ok = self.transposed and s[0] == 1 and ops.deconv3d_x3_supported(cin, cout, 1)
        if self.transposed:
            if s[0] == 2 and cout >= 16 and _small_limit(rs, True) > 0 and ops.conv3d_small_supported(cin, cout, 2, True):
                forms["small"] = ops.conv3d_small_pack(w, 2, True)
        else:
            # Winograd F(2x2,3x3) fp32-MFMA image of the stride-1 layers (conv2 / conv4 / conv6): opt-in for eval (MVS_CONV_WINO=1) because the
            # split form is as fast at the sizes that matter (reproducible under concurrent streams since DESIGN.md 4.7c: test_hip_multistream.py)
            if s == (1, 1) and cin % 4 == 0 and cout % 16 == 0 and cout <= 64 and rs.conv_wino == "1":
                forms["wino"] = ops.conv3d_wino_pack(w)
            # split form for every layer shape it is built for (stride (1,1,1) and (1,2,2)); MVS_CONV_X3 = "strided" / "s1": one kind only
            if rs.conv_x3 != "0" and ops.conv3d_x3_supported(cin, cout, s) \
                    and not (rs.conv_x3 == "strided" and s[1] == 1) and not (rs.conv_x3 == "s1" and s[1] == 2):
                forms["x3"] = ops.conv3d_x3_pack(w, s)
            if s[0] == s[1] and _small_limit(rs, False) > 0 and ops.conv3d_small_supported(cin, cout, s[0], False):
                forms["small"] = ops.conv3d_small_pack(w, s[0], False)
        self.scale, self.shift = _bn_fold(bn) if bn is not None else (None, _f32c(conv.bias) if conv.bias is not None else None)
        _publish_cache()
        self._key = key

    def _late_form(self, name: str, conv, pack):
        if name not in self.forms:
            self.forms[name] = pack(_f32c(conv.weight))
            _publish_cache()
        return self.forms[name]

    def run(self, conv, bn, relu: bool, x, residual, rs: RouteSwitches):
        """The layer on ``x [B,Cin,D,H,W]`` (+ ``residual`` before the ReLU) through the kernel its route names."""
        self._sync(conv, bn, rs)
        cin, cout, stride, f, scale, shift = self.cin, self.cout, self.stride, self.forms, self.scale, self.shift
        if not self.transposed:
            route = conv_route(cin, cout, stride, x.shape[2:], f, rs, "wino" in f and ops.conv3d_wino_supported(cin, cout, *x.shape[2:]))
            if route == "x3":
                return ops.conv3d_x3(x, f["x3"], cin, cout, stride, scale, shift, residual, relu=relu)
            if route == "small":
                return ops.conv3d_small(x, f["small"], cin, cout, stride[0], False, scale, shift, residual, relu=relu)
            if route == "wino":
                return ops.conv3d_wino(x, f["wino"], cin, cout, scale, shift, residual, relu=relu)
            return ops.conv3d(x, f["fp32"], cin, cout, stride, scale, shift, residual, relu=relu, tag="conv3d_%dto%d_s%d%d" % (cin, cout, *stride))
        sd = stride[0]
        route = deconv_route(cin, cout, sd, x.shape[2:], f, rs, self.x3_ok, 0 if residual is None else residual[0].numel() * 4)
        if route == "x3":
            return ops.deconv3d_x3(x, self._late_form("x3", conv, lambda w: ops.deconv3d_x3_pack(w, sd)), cin, cout, sd, scale, shift, residual, relu=relu)
        if route == "small":
            return ops.conv3d_small(x, f["small"], cin, cout, 2, True, scale, shift, residual, relu=relu)
        return ops.deconv3d(x, f["fp32"], cin, cout, sd, scale, shift, residual, relu=relu, tag="deconv3d_%dto%d_s%d" % (cin, cout, sd))

    def run_tail(self, conv, bn, x, skip, w1, b1, rs: RouteSwitches):
        """The layer (ReLU, ``skip`` added) followed by the 1x1x1 convolution ``(w1, b1)`` to one channel: ``[B,D,2H,2W]``, as ONE launch
        (the 8-channel volume between the two is never written) when the shape allows, else as two."""
        self._sync(conv, bn, rs)
        route = tail_route(self.cin, self.cout, self.stride[0], x.shape[2:], rs, skip.numel() * 4)
        if route == "tail_x3":
            return ops.tail_x3(x, self._late_form("tail_x3", conv, ops.tail_x3_pack), self.scale, self.shift, skip, w1, b1, relu=True)
        if route == "tail_fp32":
            return ops.deconv3d_prob1(x, self.forms["fp32"], self.cin, self.scale, self.shift, skip, w1, b1, relu=True)
        return ops.prob1(self.run(conv, bn, True, x, skip, rs), w1, b1).squeeze(1)


class Conv3d(nn.Module):
    """conv(bias = not bn) -> BatchNorm3d -> ReLU, as reference ``Conv3d`` (module.py:83-123)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, relu=True, bn=True, bn_momentum=0.1, init_method="xavier", **kwargs):
        super().__init__()
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.conv = nn.Conv3d(in_channels, out_channels, kernel_size, stride=stride, bias=(not bn), **kwargs)
        self.bn = nn.BatchNorm3d(out_channels, momentum=bn_momentum) if bn else None
        self.relu = relu
        self._layer = _EvalLayer()

    def forward(self, x, residual: Optional[torch.Tensor] = None, take=None, _rs: Optional[RouteSwitches] = None):
        if self.training:
            return _train_conv_bn_act(x, self.conv, self.bn, self.relu, residual, take=take)
        return self._layer.run(self.conv, self.bn, self.relu, x, residual, _rs or route_switches())


class Deconv3d(nn.Module):
    """conv_transpose(bias = not bn) -> BatchNorm3d -> ReLU, as reference ``Deconv3d`` (module.py:126-165)."""

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, relu=True, bn=True, bn_momentum=0.1, init_method="xavier", **kwargs):
        super().__init__()
        self.out_channels = out_channels
        self.conv = nn.ConvTranspose3d(in_channels, out_channels, kernel_size, stride=stride, bias=(not bn), **kwargs)
        self.bn = nn.BatchNorm3d(out_channels, momentum=bn_momentum) if bn else None
        self.relu = relu
        self._layer = _EvalLayer()

    def forward(self, x, residual: Optional[torch.Tensor] = None, give=None, _rs: Optional[RouteSwitches] = None):
        if self.training:
            _EvalLayer.check(self.conv)
            return _train_conv_bn_act(x, self.conv, self.bn, self.relu, residual, transposed_sd=self.conv.stride[0], give=give)
        return self._layer.run(self.conv, self.bn, self.relu, x, residual, _rs or route_switches())


class ConvBnReLU(nn.Module):
    """2-D conv(bias=False) -> BatchNorm2d -> ReLU holder (reference module.py:168-197).  Used only inside
    ``StageNet.vis``, whose four layers run as one fused HIP launch (:func:`pack_vis_params`)."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, stride: int = 1, pad: int = 1, dilation: int = 1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=pad, dilation=dilation, bias=False)
        self.bn = nn.BatchNorm2d(out_channels)

    def forward(self, x):
        raise MvsHipError("ConvBnReLU is a parameter holder; the fused visibility CNN runs through StageNet (mvs_vis_fwd)")


def pack_vis_params(vis: nn.Sequential) -> torch.Tensor:
    """Flatten ``StageNet.vis`` (ConvBnReLU(1,16), ConvBnReLU(16,16), ConvBnReLU(16,8), Conv2d(8,1,1), Sigmoid) into the
    3689-float parameter block of ``mvs_vis_fwd`` (layout documented in csrc/vis_net.hip)."""
    c0, c1, c2, c3 = vis[0], vis[1], vis[2], vis[3]
    shapes = [tuple(c.conv.weight.shape) for c in (c0, c1, c2)] + [tuple(c3.weight.shape)]
    if shapes != [(16, 1, 3, 3), (16, 16, 3, 3), (8, 16, 3, 3), (1, 8, 1, 1)]:
        raise MvsHipError("vis CNN has unexpected shapes %s" % (shapes,))
    parts = []
    for c in (c0, c1, c2):
        w = _f32c(c.conv.weight)                               # [cout, cin, 3, 3] -> [cin, tap, cout]
        parts.append(w.permute(1, 2, 3, 0).reshape(-1))
        s, b = _bn_fold(c.bn)
        parts += [s, b]
    parts += [_f32c(c3.weight).reshape(-1), _f32c(c3.bias).reshape(-1)]
    out = torch.cat(parts).contiguous()
    assert out.numel() == ops.VIS_PARAM_FLOATS
    return out


# ---------------------------------------------------------------------------------------------------------
# regularizers (reference models/module.py:469-505, 550-594)
# ---------------------------------------------------------------------------------------------------------
def _volume_input(net, x: torch.Tensor, strided: int, bf16_ok: bool):
    """The cost volume as the layers of ``net`` take it: fp32 ``[B,C,D,H,W]`` - or, if ``bf16_ok``, the bf16 channel-last ``[B,D,H,W,C]`` it already
    is (autograd.AggregateFn as_bf16).  -> (x, whether it is the latter).  ``strided``: how many of D, H, W (from the right) the U-Net halves."""
    if not isinstance(net.inner, nn.Identity):
        raise MvsHipError("%s: in_channels != base channels (1x1x1 'inner' conv) is not built" % type(net).__name__)
    pre16 = bf16_ok and x.dtype == torch.bfloat16
    if not pre16:
        x = x.to(torch.float32)
    x = x if x.is_contiguous() else x.contiguous()
    dhw = tuple(x.shape[1:4] if pre16 else x.shape[2:])[-strided:]
    if any(n % 8 for n in dhw):
        raise MvsHipError("%s needs %s divisible by 8 (three stride-2 levels), got %s" % (type(net).__name__, ("H, W", "D, H, W")[strided - 2], dhw))
    return x, pre16


class CostRegNet(nn.Module):
    """3-D U-Net with stride-2 down/up-sampling in D, H, W (reference ``CostRegNet``).  ``forward(x[B,Cin,D,H,W])``
    returns ``[B,1,D,H,W]`` logits (``[B,base,D,H,W]`` features if ``last_layer=False``)."""

    def __init__(self, in_channels, base_channels, last_layer=True):
        super().__init__()
        self.last_layer = last_layer
        b = base_channels
        self.conv1 = Conv3d(in_channels, b * 2, stride=2, padding=1)
        self.conv2 = Conv3d(b * 2, b * 2, padding=1)
        self.conv3 = Conv3d(b * 2, b * 4, stride=2, padding=1)
        self.conv4 = Conv3d(b * 4, b * 4, padding=1)
        self.conv5 = Conv3d(b * 4, b * 8, stride=2, padding=1)
        self.conv6 = Conv3d(b * 8, b * 8, padding=1)
        self.conv7 = Deconv3d(b * 8, b * 4, stride=2, padding=1, output_padding=1)
        self.conv9 = Deconv3d(b * 4, b * 2, stride=2, padding=1, output_padding=1)
        self.conv11 = Deconv3d(b * 2, b * 1, stride=2, padding=1, output_padding=1)
        if in_channels != base_channels:
            self.inner = nn.Conv3d(in_channels, base_channels, 1, 1)
        else:
            self.inner = nn.Identity()
        if self.last_layer:
            self.prob = nn.Conv3d(base_channels, 1, 3, stride=1, padding=1, bias=False)

    def features(self, x: torch.Tensor) -> torch.Tensor:
        """Everything up to (not including) ``prob``; residual adds are fused into the deconv epilogues."""
        x, pre16 = _volume_input(self, x, 3, self.training)
        if self.training and autocast_bf16() and not pre16:
            from . import autograd as ag
            x = ag.ToBf16Fn.apply(x)                     # fp32 cost volume -> bf16 channel-last; every layer below follows the dtype
        if not self.training:
            rs = route_switches()
            c2 = self.conv2(self.conv1(x, _rs=rs), _rs=rs)
            c4 = self.conv4(self.conv3(c2, _rs=rs), _rs=rs)
            y = self.conv7(self.conv6(self.conv5(c4, _rs=rs), _rs=rs), residual=c4, _rs=rs)
            return self.conv11(self.conv9(y, residual=c2, _rs=rs), residual=x, _rs=rs)
        # training: each skip tensor's two gradients meet in the strided convolution's data-gradient epilogue (autograd.SkipLink)
        l0, l2, l4 = _skip_links(x)
        c2 = _multi_use(self.conv2(self.conv1(x, take=l0)), l2)
        c4 = _multi_use(self.conv4(self.conv3(c2, take=l2)), l4)
        y = self.conv6(self.conv5(c4, take=l4))
        y = self.conv7(y, residual=c4, give=l4)
        y = self.conv9(y, residual=c2, give=l2)
        return _multi_use(self.conv11(y, residual=x, give=l0))

    def forward(self, x):
        y = self.features(x)
        if self.last_layer:
            if self.training:
                from . import autograd as ag
                # N = 1 conv embedded in an 8-channel MFMA conv (zero rows) so forward, dgrad and wgrad reuse the conv kernels
                pk = ag.packed_of(self.prob) if y.dtype == torch.bfloat16 else None
                if pk is not None and ag._fused_layers():
                    # the 8 -> 1 parameter packed as an 8 -> 8 map by the stage's StagePack (no padded copy of the weight), channel 0 of
                    # the result straight to fp32
                    y = ag.Select0Bf16Fn.apply(ag.ConvBf16Fn.apply(y, ag.route_of(self.prob), (1, 1), 0, pk, 8)).unsqueeze(1)
                else:
                    w8 = torch.nn.functional.pad(self.prob.weight, (0, 0, 0, 0, 0, 0, 0, 0, 0, 7))
                    if y.dtype == torch.bfloat16:        # autocast: the logits come out of a half-precision conv, then fp32
                        y = ag.FromBf16Fn.apply(ag.ConvBf16Fn.apply(y, w8, (1, 1)))[:, :1]
                    else:
                        y = ag.ConvFn.apply(y, w8, (1, 1))[:, :1]
            else:
                y = ops.prob3(y, _f32c(self.prob.weight)).unsqueeze(1)
        return y


def _deconv_seq(cin, cout):
    return nn.Sequential(
        nn.ConvTranspose3d(cin, cout, kernel_size=3, padding=1, output_padding=(0, 1, 1), stride=(1, 2, 2), bias=False),
        nn.BatchNorm3d(cout), nn.ReLU(inplace=True))


class CostRegNet3D(nn.Module):
    """3-D U-Net with stride (1,2,2): depth resolution kept (reference ``CostRegNet3D``).  The decoder layers are
    ``nn.Sequential(ConvTranspose3d, BatchNorm3d, ReLU)`` so the checkpoint keys are ``convN.0.weight`` / ``convN.1.*``."""

    def __init__(self, in_channels, base_channel=8):
        super().__init__()
        b = base_channel
        self.conv1 = Conv3d(in_channels, b * 2, kernel_size=3, stride=(1, 2, 2), padding=1)
        self.conv2 = Conv3d(b * 2, b * 2, padding=1)
        self.conv3 = Conv3d(b * 2, b * 4, kernel_size=3, stride=(1, 2, 2), padding=1)
        self.conv4 = Conv3d(b * 4, b * 4, padding=1)
        self.conv5 = Conv3d(b * 4, b * 8, kernel_size=3, stride=(1, 2, 2), padding=1)
        self.conv6 = Conv3d(b * 8, b * 8, padding=1)
        self.conv7 = _deconv_seq(b * 8, b * 4)
        self.conv9 = _deconv_seq(b * 4, b * 2)
        self.conv11 = _deconv_seq(b * 2, b)
        if in_channels != base_channel:
            self.inner = nn.Conv3d(in_channels, base_channel, 1, 1)
        else:
            self.inner = nn.Identity()
        self.prob = nn.Conv3d(base_channel, 1, 1, stride=1, padding=0)
        self._layers = {name: _EvalLayer() for name in ("conv7", "conv9", "conv11")}

    def _up(self, name: str, x, residual, give=None, _rs: Optional[RouteSwitches] = None):
        seq = getattr(self, name)
        if self.training:
            _EvalLayer.check(seq[0])
            return _train_conv_bn_act(x, seq[0], seq[1], True, residual, transposed_sd=seq[0].stride[0], give=give)
        return self._layers[name].run(seq[0], seq[1], True, x, residual, _rs or route_switches())

    def logits(self, x: torch.Tensor) -> torch.Tensor:
        """Eval-mode ``forward`` without the channel axis, ``[B,D,H,W]``: conv11 and the 1x1x1 ``prob`` as one launch where that is built."""
        rs = None if self.training else route_switches()
        y, skip = self._trunk(x, rs)
        if self.training:
            return ops.prob1(self._up("conv11", y, skip), *self.prob_params()).squeeze(1)
        return self._layers["conv11"].run_tail(self.conv11[0], self.conv11[1], y, skip, *self.prob_params(), rs)

    def _trunk(self, x: torch.Tensor, rs: Optional[RouteSwitches]):
        """Everything up to conv9, without SkipLinks: returns (conv9 output, skip tensor of conv11 = the input volume)."""
        x, _ = _volume_input(self, x, 2, False)
        c2 = self.conv2(self.conv1(x, _rs=rs), _rs=rs)
        c4 = self.conv4(self.conv3(c2, _rs=rs), _rs=rs)
        y = self.conv6(self.conv5(c4, _rs=rs), _rs=rs)
        y = self._up("conv7", y, c4, _rs=rs)
        return self._up("conv9", y, c2, _rs=rs), x

    def features(self, x: torch.Tensor) -> torch.Tensor:
        if not self.training:
            rs = route_switches()
            y, skip = self._trunk(x, rs)
            return self._up("conv11", y, skip, _rs=rs)
        x, pre16 = _volume_input(self, x, 2, True)
        if autocast_bf16() and not pre16:
            from . import autograd as ag
            x = ag.ToBf16Fn.apply(x)                     # fp32 cost volume -> bf16 channel-last; every layer below follows the dtype
        l0, l2, l4 = _skip_links(x)
        c2 = _multi_use(self.conv2(self.conv1(x, take=l0)), l2)
        c4 = _multi_use(self.conv4(self.conv3(c2, take=l2)), l4)
        y = self.conv6(self.conv5(c4, take=l4))
        y = self._up("conv7", y, c4, l4)
        y = self._up("conv9", y, c2, l2)
        return _multi_use(self._up("conv11", y, x, l0))

    def prob_params(self):
        return _f32c(self.prob.weight).reshape(-1), _f32c(self.prob.bias).reshape(-1)

    def forward(self, x):
        y = self.features(x)
        if self.training:
            from . import autograd as ag
            if y.dtype == torch.bfloat16:                # the 1x1x1 head and everything after it are fp32 again
                if ag._fused_layers():
                    return ag.HeadBf16Fn.apply(y, self.prob.weight, self.prob.bias, False).unsqueeze(1)
                y = ag.FromBf16Fn.apply(y)
            return ag.Prob1Fn.apply(y, self.prob.weight, self.prob.bias)
        w, b = self.prob_params()
        return ops.prob1(y, w, b)


# ---------------------------------------------------------------------------------------------------------
# heads and schedulers (reference models/module.py:597-619, 622-653, 687-699)
# ---------------------------------------------------------------------------------------------------------
def depth_regression(p, depth_values):
    """``sum_d p * depth_values``; ``depth_values`` is ``[B,D,H,W]`` or ``[B,D]`` (reference module.py:597-603)."""
    if depth_values.dim() > 2 and depth_values.shape != p.shape:
        depth_values = depth_values.expand_as(p)
    return ops.depth_regression(p.to(torch.float32).contiguous(), depth_values.to(torch.float32).contiguous())


def conf_regression(p, n=4):
    """Windowed probability mass around the expected index (reference module.py:606-619)."""
    return ops.conf_regression(p.detach().to(torch.float32).contiguous(), n)


def init_inverse_range(cur_depth, ndepths, device, dtype, H, W):
    """Reference signature (module.py:633); ``device``/``dtype`` are accepted for compatibility, output is fp32 on
    ``cur_depth``'s device."""
    return ops.init_inverse_range(cur_depth.to(torch.float32).contiguous(), ndepths, H, W)


def init_range(cur_depth, ndepths, device, dtype, H, W):
    """Reference signature (module.py:622); ``device``/``dtype`` are accepted for compatibility, output is fp32 on
    ``cur_depth``'s device."""
    return ops.init_range(cur_depth.to(torch.float32).contiguous(), ndepths, H, W)


def schedule_range(cur_depth, ndepth, depth_inteval_pixel, H, W):
    """Reference signature (module.py:687): ``depth_inteval_pixel [B]`` is the stage's ratio times the depth interval already."""
    return ops.schedule_range(cur_depth.to(torch.float32).contiguous(), depth_inteval_pixel.to(torch.float32).contiguous(), ndepth, 1.0, H, W)


def schedule_inverse_range(depth, depth_hypo, ndepths, split_itv, H, W):
    """Reference signature (module.py:642)."""
    return ops.schedule_inverse_range(depth.to(torch.float32).contiguous(), depth_hypo.to(torch.float32).contiguous(),
                                      ndepths, float(split_itv), H, W)
