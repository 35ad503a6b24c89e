"""The ``MVS_*`` environment switches of the Python package: one table, one reader.

Every switch the package reads has a row in :data:`TABLE` (the README's switch table is :func:`readme_table` of it) and is read through
:func:`flag`, :func:`integer`, :func:`number` or :func:`text`; a name without a row raises, so a typo cannot create a switch.  Kinds:

* ``on``:  on unless the value is ``"0"``         * ``off``: on only if the value is ``"1"``
* ``int`` / ``float``: ``int(value)`` / ``float(value)``        * ``str``: the text, one of ``values`` where those are given

``read`` says when the package looks: ``call`` (every call that reaches the site), ``pack`` (when a layer's cached weights are rebuilt; the
caches carry these values in their keys, so a change rebuilds on the next forward) or ``import``.  The variables that
``libmvs_hip.so`` reads itself (``mvs::env_int`` / ``mvs::env_str``) are not in this table.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple


class Switch(NamedTuple):
    name: str
    default: object                          # what an unset variable means (None: see ``meaning``)
    kind: str                                # "on" | "off" | "int" | "float" | "str"
    meaning: str
    read: str = "call"                       # "call" | "pack" | "import"
    values: Optional[Tuple[str, ...]] = None  # kind "str": the accepted values, where the package validates them


_ROWS = (
    # regularizer, eval
    Switch("MVS_CONV_X3", "1", "str", "`0` = regularizer layers on the fp32 instead of the bf16 matrix cores (3-term split form, DESIGN §4.7; also turns the "
           "small-volume split form off); `strided` / `s1` = split form for the stride-(1,2,2) / the stride-1 convolutions only (diagnostics)", "pack"),
    Switch("MVS_CONV_X3_MIN_VOXELS", 40 * 1024, "int", "output voxels from which a layer uses the split form; below, it keeps the fp32 kernel"),
    Switch("MVS_CONV_SMALL_MAX_WORK", None, "str", "`conv,deconv` or one value for both: voxels x Cin x Cout up to which the small-volume split form "
           "serves a layer (unset: 16777216,8388608; `0` = never)", "import"),
    Switch("MVS_CONV_WINO", None, "str", "`1` = Winograd fp32 convolution for the stride-1 layers in eval (opt-in: the split form is as fast); the training "
           "forward uses it unless `0`", "pack"),
    Switch("MVS_FUSE_PROB", True, "on", "`0` = conv11 and the 1x1x1 `prob` as two launches"),
    Switch("MVS_TAIL", "x3", "str", "anything but `x3` (say `fp32`) = the fused conv11 + `prob` tail on the fp32 instead of the bf16 matrix cores"),
    # cost volume and visibility CNN
    Switch("MVS_CV_FAST", False, "off", "`1` = sweeps with one reciprocal + hardware exp2/log2 instead of the reference's op order with IEEE divisions"),
    Switch("MVS_CV_STORE_MAX_MB", 160.0, "float", "size limit of a coarse stage's stored correlation; 0 = always recompute"),
    Switch("MVS_CV_STORE_BANDS", 1, "int", "row bands in which a stage whose store is larger may run the stored-correlation sweeps (bit-identical)"),
    Switch("MVS_CV_TILED", False, "off", "`1` = the LDS-tiled sweeps instead of the direct-gather sweeps (DESIGN §4.2c; ignored by `StageNet.forward_bank`)"),
    Switch("MVS_VIS", None, "str", "visibility CNN on the bf16 matrix cores in split form (`x3`) / Winograd fp32 MFMA (`wino`) / all-VALU (`valu`); "
           "unset: `x3`, or `valu` with `MVS_VIS_WINO=0`", "pack", ("x3", "wino", "valu")),
    Switch("MVS_VIS_WINO", True, "on", "`0` = `MVS_VIS=valu` where `MVS_VIS` is unset", "pack"),
    Switch("MVS_TRANSPOSE_MULTI", True, "on", "`0` = one NCHW -> NHWC transpose launch per stage instead of one for the cascade"),
    # feature extraction
    Switch("MVS_FPN_X3", "1", "str", "`0` = the FPN's full-resolution layers on the fp32 matrix cores; `strip` = the decoder's last level as the split-form "
           "strip kernel (`csrc/fpn_x3.hip`) instead of the contraction-first kernel (`csrc/fpn_cp.hip`)", "pack"),
    Switch("MVS_FPN_V2_TAIL", True, "on", "`0` = `FPNDecoderV2`'s full-resolution tail through the generic split-form GEMMs (up map written, added, read back) "
           "instead of the fused kernel (`csrc/fpn_v2_tail.hip`)", "pack"),
    Switch("MVS_VIT_PACKED", True, "on", "`0` = the ViT with operands split inside every GEMM block instead of pre-split"),
    Switch("MVS_VIT_FLASH", True, "on", "`0` = materialized attention in every block of the unpacked eval ViT (`MVS_VIT_PACKED=0`)"),
    Switch("MVS_VIT_TRAIN_FLASH", True, "on", "`0` = ViT training (`\"fix\": false`) with materialized attention instead of `csrc/vit_flash_train.hip`"),
    # training
    Switch("MVS_TRAIN_BF16", False, "off", "`1` = bf16 regularizer in training without an autocast context"),
    Switch("MVS_TRAIN_FUSED", True, "on", "`0` = separate conv / BatchNorm autograd nodes, per-layer weight packing and fp32 heads instead of the fused layer nodes"),
    Switch("MVS_TRAIN_SKIPLINK", True, "on", "`0` = autograd adds a skip tensor's two gradients (instead of the strided layer's data-gradient epilogue)"),
    Switch("MVS_TRAIN_WGRAD_GROUP", True, "on", "`0` = every layer runs its own weight gradient instead of one grouped launch per kernel instance"),
    Switch("MVS_TRAIN_WGRAD_SCOPE", "cascade", "str", "`stage` = one weight-gradient group per stage instead of one for the cascade"),
    Switch("MVS_BN_FUSED_STATS", False, "off", "`1` = the unfused bf16 training convolution takes the batch statistics in its epilogue (measured slower)"),
    Switch("MVS_VIS_BF16", True, "on", "`0` = the visibility CNN stays fp32 under autocast"),
    Switch("MVS_VIS_PER_VIEW", False, "off", "`1` = the training visibility CNN runs view by view instead of batched over the source views"),
    Switch("MVS_CV_BWD", "own", "str", "scatter of the cost-volume backward: per-wavefront LDS windows with owner election / block-shared window with "
           "LDS atomics / global atomics (DESIGN §4.5)", "call", ("own", "lds", "direct")),
    Switch("MVS_CV_BWD_WINDOW", None, "str", "`log2(WX),WY` texel window of the cost-volume backward (unset: `5,20` for `own`, `6,24` for `lds`)"),
    # diagnostics
    Switch("MVS_TAG_SHAPES", False, "off", "`1` = the grouped weight gradient's timer tag carries its shape"),
    Switch("MVS_HIP_LIB", None, "str", "path of another build of `libmvs_hip.so` (`make -C mvsformer_amd/csrc variants` or `exp`)", "import"),
)
TABLE = {s.name: s for s in _ROWS}


def _get(name: str, kinds) -> Tuple[Switch, Optional[str]]:
    row = TABLE.get(name)
    if row is None or row.kind not in kinds:
        raise KeyError("%s is not a%s switch of mvsformer_amd.switches.TABLE" % (name, "" if row is None else " " + "/".join(kinds)))
    return row, os.environ.get(name)


def flag(name: str) -> bool:
    row, v = _get(name, ("on", "off"))
    return v != "0" if row.kind == "on" else v == "1"


def integer(name: str) -> int:
    row, v = _get(name, ("int",))
    return int(row.default if v is None else v)


def number(name: str) -> float:
    row, v = _get(name, ("float",))
    return float(row.default if v is None else v)


def text(name: str, error=ValueError) -> Optional[str]:
    """The variable's text (the row's default if it is unset); a row with ``values`` accepts nothing else (``error`` is raised)."""
    row, v = _get(name, ("str",))
    if v is None:
        return row.default
    if row.values is not None and v not in row.values:
        raise error("%s must be one of %s, not %r" % (name, ", ".join(row.values), v))
    return v


# The small-volume split-form kernel (csrc/conv3d_x3_small.hip) serves a layer while voxels x Cin x Cout stays below these bounds (output voxels
# of a convolution, input voxels of a transposed convolution): measured per layer at the two coarse config-2 stages (profiles/r04_bench_small.txt),
# it wins 4-21 us per launch below them and loses above (its vector ALU bound grows with the volume, the tiled kernels' latency chains do not).
SMALL_MAX_WORK = (16 << 20, 8 << 20)      # (Conv3d, Deconv3d); MVS_CONV_SMALL_MAX_WORK="conv,deconv" overrides, "0,0" = never


def _parse_small_limit(text) -> Tuple[int, int]:
    """``"conv,deconv"`` or one value for both; anything else is a configuration error reported at import, not in the middle of a forward."""
    if not text:
        return SMALL_MAX_WORK
    try:
        v = [int(t) for t in text.split(",")]
    except ValueError:
        v = []
    if len(v) == 1:
        v = v * 2
    if len(v) != 2 or min(v) < 0:
        raise ValueError("MVS_CONV_SMALL_MAX_WORK must be 'conv,deconv' or one non-negative integer, got %r" % (text,))
    return v[0], v[1]


def readme_table() -> str:
    """The switch table as the README shows it (tests/test_routes.py holds the two together)."""
    def shown(s):
        if s.default is None:
            return "unset"
        if s.kind in ("on", "off"):
            return "1" if s.default else "0"
        return "%g" % s.default if s.kind == "float" else str(s.default)
    head = "| name | default | meaning | read |\n|---|---|---|---|\n"
    return head + "".join("| `%s` | %s | %s | %s |\n" % (s.name, shown(s), s.meaning, s.read) for s in _ROWS)
