"""Which kernel an eval-mode layer takes - the regularizer's (mvsformer_amd.module.conv_route / deconv_route / tail_route), the FPN's
(mvsformer_amd.fpn.encoder_route / decoder_route / v2_tail_route) and a stage's sweeps (mvsformer_amd.stagenet.sweep_plan, the visibility mode):
pure functions, no GPU, no library - and the MVS_* switch table (mvsformer_amd.switches) with its README rendering."""
import ast
import itertools
import os
import re

import pytest

from mvsformer_amd import switches
from mvsformer_amd.module import RouteSwitches, conv_route, deconv_route, tail_route

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEF = RouteSwitches()                       # the defaults: 40960 voxels, small limits 16 << 20 / 8 << 20
GIB = 1 << 30


def test_route_defaults_are_the_documented_ones():
    assert DEF.min_voxels == 40960 and DEF.small_limit == (16 << 20, 8 << 20)
    assert (DEF.conv_x3, DEF.tail, DEF.fuse_prob) == ("1", "x3", True)


@pytest.mark.parametrize("cin,cout,stride,shape,forms,wino_ok,want", [
    (16, 16, (1, 1), (4, 80, 128), {"x3", "small"}, False, "x3"),           # 40960 voxels: exactly the threshold
    (16, 16, (1, 1), (4, 80, 127), {"x3", "small"}, False, "small"),        # 40640 voxels
    (16, 16, (1, 1), (4, 80, 127), {"x3"}, False, "fp32"),
    (8, 16, (1, 2), (5, 129, 254), {"x3"}, False, "fp32"),                  # floor count 5*64*127 = 40640 (the true output is 41275 voxels)
    (8, 16, (1, 2), (5, 130, 254), {"x3"}, False, "x3"),                    # 5*65*127 = 41275
    (64, 64, (1, 1), (4, 32, 32), {"small", "wino"}, True, "small"),        # work exactly 16 << 20
    (64, 64, (1, 1), (4, 32, 33), {"small", "wino"}, True, "wino"),
    (64, 64, (1, 1), (4, 32, 33), {"small", "wino"}, False, "fp32"),
    (8, 8, (1, 1), (64, 1024, 1024), {"x3"}, False, "fp32"),                # one sample is exactly 2 GiB
    (8, 8, (1, 1), (63, 1024, 1024), {"x3"}, False, "x3"),
    (16, 32, (2, 2), (8, 16, 24), {"small"}, False, "small"),               # stride 2: the TRUE output size (4*8*12 voxels) counts
    (16, 32, (2, 2), (8, 16, 24), set(), False, "fp32"),
])
def test_conv_route(cin, cout, stride, shape, forms, wino_ok, want):
    assert conv_route(cin, cout, stride, shape, forms | {"fp32"}, DEF, wino_ok) == want


@pytest.mark.parametrize("cin,cout,shape,x3_ok,res_bytes,want", [
    (32, 16, (4, 32, 80), True, 0, "x3"),                                   # 4*D*H*W = 40960: exactly the threshold
    (32, 16, (4, 32, 79), True, 0, "fp32"),                                 # odd W (and 40448 voxels)
    (32, 16, (4, 31, 80), True, 0, "fp32"),                                 # 39680 voxels
    (32, 16, (5, 41, 50), True, 0, "x3"),                                   # 41000 voxels, W even
    (32, 16, (5, 50, 41), True, 0, "fp32"),                                 # the same volume with W odd
    (16, 8, (4, 32, 80), True, 0, "fp32"),                                  # cout 8 against 16
    (32, 16, (4, 32, 80), False, 0, "fp32"),                                # not built for the shape
    (32, 16, (4, 32, 80), True, 4 * GIB - 4, "x3"),                         # the residual's window: 4 GiB per sample
    (32, 16, (4, 32, 80), True, 4 * GIB, "fp32"),
    (8, 16, (63, 1024, 1024), True, 0, "x3"),                               # the input's window: 2 GiB per sample
    (8, 16, (64, 1024, 1024), True, 0, "fp32"),
])
def test_deconv_route_stride_122(cin, cout, shape, x3_ok, res_bytes, want):
    assert deconv_route(cin, cout, 1, shape, {"fp32"}, DEF, x3_ok, res_bytes) == want


@pytest.mark.parametrize("cin,cout,shape,forms,want", [
    (64, 32, (4, 32, 32), {"small"}, "small"),                              # D*H*W*cin*cout = 8 << 20 exactly (INPUT voxels)
    (64, 32, (4, 32, 33), {"small"}, "fp32"),
    (64, 32, (4, 32, 32), set(), "fp32"),                                   # the form was not packed (cout < 16, or not built)
])
def test_deconv_route_stride_222(cin, cout, shape, forms, want):
    assert deconv_route(cin, cout, 2, shape, forms | {"fp32"}, DEF) == want


@pytest.mark.parametrize("cin,cout,sd,shape,rs,skip_bytes,want", [
    (16, 8, 1, (4, 32, 80), DEF, 0, "tail_x3"),                             # 4*D*H*W = 40960
    (16, 8, 1, (4, 31, 80), DEF, 0, "tail_fp32"),                           # below the threshold: fused, fp32 matrix cores
    (16, 8, 1, (4, 80, 30), DEF, 0, "unfused"),                             # W % 4
    (16, 8, 1, (4, 80, 32), DEF, 0, "tail_x3"),
    (32, 8, 1, (4, 32, 80), DEF, 0, "tail_fp32"),                           # cin not 16
    (16, 16, 1, (4, 32, 80), DEF, 0, "unfused"),                            # cout not 8
    (16, 8, 2, (4, 32, 80), DEF, 0, "unfused"),                             # stride (2,2,2)
    (16, 8, 1, (4, 32, 80), DEF._replace(tail="fp32"), 0, "tail_fp32"),     # MVS_TAIL=fp32
    (16, 8, 1, (4, 32, 80), DEF._replace(fuse_prob=False), 0, "unfused"),   # MVS_FUSE_PROB=0
    (16, 8, 1, (4, 32, 80), DEF, 2 * GIB - 4, "tail_x3"),                   # the skip volume against the window, whole batch:
    (16, 8, 1, (4, 32, 80), DEF, 2 * GIB, "tail_fp32"),                     # two samples of 1 GiB are over, though each one is under
])
def test_tail_route(cin, cout, sd, shape, rs, skip_bytes, want):
    assert tail_route(cin, cout, sd, shape, rs, skip_bytes) == want


def test_conv_x3_off_leaves_no_split_form():
    """MVS_CONV_X3=0: nothing routes to x3, small or tail_x3, whatever forms a layer (still) has and however large it is."""
    off = DEF._replace(conv_x3="0", min_voxels=0)
    shapes = [(4, 8, 8), (4, 80, 128), (8, 64, 96)]
    forms = {"fp32", "x3", "small", "wino"}
    for (cin, cout), stride, shape in itertools.product([(8, 16), (16, 16), (64, 64)], [(1, 1), (1, 2), (2, 2)], shapes):
        assert conv_route(cin, cout, stride, shape, forms, off, True) in ("wino", "fp32")
        assert conv_route(cin, cout, stride, shape, forms, off, False) == "fp32"
    for (cin, cout), sd, shape in itertools.product([(32, 16), (16, 8), (64, 32)], [1, 2], shapes):
        assert deconv_route(cin, cout, sd, shape, forms, off, True) == "fp32"
        assert tail_route(cin, cout, sd, shape, off) in ("tail_fp32", "unfused")
    assert tail_route(16, 8, 1, (4, 32, 80), off) == "tail_fp32"


# ------------------------------------------------------------------------------------------------------------------------------ FPN
FPN_CH = {"conv00": (3, 8), "conv01": (8, 8), "downsample1": (8, 16), "conv10": (16, 16), "conv11": (16, 16), "downsample2": (16, 32),
          "conv20": (32, 32), "conv21": (32, 32), "downsample3": (32, 64), "conv30": (64, 64), "conv31": (64, 64)}


def _fpn_switches(monkeypatch, x3):
    from mvsformer_amd.fpn import fpn_switches
    monkeypatch.delenv("MVS_FPN_X3", raising=False) if x3 is None else monkeypatch.setenv("MVS_FPN_X3", x3)
    return fpn_switches()


@pytest.mark.parametrize("x3,x3_ok,x3s_ok,want", [
    (None, True, False, "x3"), (None, True, True, "x3"), (None, False, True, "x3s"), (None, False, False, "fp32"),
    ("strip", True, False, "x3"), ("strip", True, True, "x3"), ("strip", False, True, "x3s"), ("strip", False, False, "fp32"),
    ("0", True, False, "fp32"), ("0", True, True, "fp32"), ("0", False, True, "fp32"), ("0", False, False, "fp32"),
])
def test_encoder_route(monkeypatch, x3, x3_ok, x3s_ok, want):
    from mvsformer_amd.fpn import FPNEncoder, encoder_route
    fs = _fpn_switches(monkeypatch, x3)
    assert [name for name, _, _ in FPNEncoder.LAYERS] == list(FPN_CH)
    for name, k, stride in FPNEncoder.LAYERS:
        assert encoder_route(*FPN_CH[name], k, stride, x3_ok, x3s_ok, fs) == want, name


@pytest.mark.parametrize("x3,want", [
    (None, [("fpn_lvl_x3", False), ("fpn_lvl_x3", True), ("fpn_cp", False)]),      # level 2 hands over channel-last: fpn_cp reads it
    ("strip", [("fpn_lvl_x3", False), ("fpn_lvl_x3", False), ("fpn_x3", False)]),
    ("0", [("fpn", False), ("fpn", False), ("fpn", False)]),
])
def test_decoder_route(monkeypatch, x3, want):
    from mvsformer_amd.fpn import decoder_route
    fs = _fpn_switches(monkeypatch, x3)
    assert [decoder_route(level, fs) for level in (1, 2, 3)] == want


@pytest.mark.parametrize("tail_chs,switch,want", [(True, None, "fused"), (True, "1", "fused"), (True, "0", "gemm"), (False, None, "gemm"),
                                                  (False, "0", "gemm")])
def test_v2_tail_route(monkeypatch, tail_chs, switch, want):
    from mvsformer_amd.fpn import fpn_switches, v2_tail_route
    monkeypatch.delenv("MVS_FPN_V2_TAIL", raising=False) if switch is None else monkeypatch.setenv("MVS_FPN_V2_TAIL", switch)
    assert fpn_switches().v2_tail is (switch != "0")
    assert v2_tail_route(tail_chs, fpn_switches()) == want


# --------------------------------------------------------------------------------------------------------------------------- sweeps
MB = 2 ** 20
# the store sizes ``ops.cv_store_bytes`` gives at config 2 (pinned with the library in test_abi.py): stage 1 = 5 views of 144x192, C 64, D 32: 121.5 MiB
# (the "127 MB"); stage 2 = 288x384, C 32, D 16: 243 MiB (the "254 MB")
S1, S2 = 127401984, 254803968


@pytest.mark.parametrize("nbytes,H,limit_mb,bands,want", [
    (S1, 144, 160.0, 1, 1),                                                 # 127 MB: one store for the whole image
    (S2, 288, 160.0, 1, 0),                                                 # 254 MB: recompute (banding is opt-in)
    (-1, 576, 160.0, 1, 0),                                                 # C = 16: not built for the shape
    (S2, 288, 160.0, 4, 2),                                                 # two bands of 144 + 7 rows: 133 MB each
    (S1, 144, 160.0, 4, 1),
    (S2, 288, 70.0, 4, 4),                                                  # 72 + 7 rows: 69.7 MB
    (S1, 144, 70.0, 4, 2),
    (S2, 288, 400.0, 4, 1),
    (S1, 144, 0.0, 4, 0),                                                   # limit 0: the stored-correlation sweeps are off
    (160 * MB, 144, 160.0, 1, 1),                                           # exactly the limit
    (160 * MB + 1, 144, 160.0, 1, 0),
])
def test_sweep_plan(nbytes, H, limit_mb, bands, want):
    from mvsformer_amd.stagenet import TILED, StageSwitches, sweep_plan
    ss = StageSwitches(store_max_mb=limit_mb, store_bands=bands)
    assert (S1 / MB, S2 / MB) == (121.5, 243.0)
    for tiled_ok in (False, True):
        assert sweep_plan(nbytes, H, tiled_ok, ss) == want                  # MVS_CV_TILED unset: what the features allow does not matter
        assert sweep_plan(nbytes, H, tiled_ok, ss._replace(tiled=True)) == (TILED if tiled_ok else want)
    assert TILED not in (0, 1, 2, 3, 4)


def test_stage_switches_defaults_are_the_documented_ones(monkeypatch):
    from mvsformer_amd.stagenet import StageSwitches, stage_switches
    for name in ("MVS_CV_TILED", "MVS_CV_STORE_MAX_MB", "MVS_CV_STORE_BANDS", "MVS_VIS", "MVS_VIS_WINO"):
        monkeypatch.delenv(name, raising=False)
    assert stage_switches() == StageSwitches() == (False, 160.0, 1, "x3")
    monkeypatch.setenv("MVS_CV_TILED", "1"), monkeypatch.setenv("MVS_CV_STORE_MAX_MB", "70"), monkeypatch.setenv("MVS_CV_STORE_BANDS", "4")
    assert stage_switches() == (True, 70.0, 4, "x3")


@pytest.mark.parametrize("vis,wino,want", [(None, None, "x3"), (None, "0", "valu"), ("x3", None, "x3"), ("x3", "0", "x3"), ("wino", None, "wino"),
                                           ("wino", "0", "wino"), ("valu", None, "valu"), ("valu", "0", "valu")])
def test_visibility_mode(monkeypatch, vis, wino, want):
    from mvsformer_amd.stagenet import stage_switches
    for name, value in (("MVS_VIS", vis), ("MVS_VIS_WINO", wino)):
        monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)
    assert stage_switches().vis == want


def test_eval_forwards_read_no_switch_themselves():
    """In fpn.py and stagenet.py the switch-tuple readers are the only functions that call the switch reader: no ``forward`` / ``forward_bank`` (or
    anything else, the eval body ``StageNet._eval`` included) holds a ``sw.`` call."""
    for name, readers in (("fpn.py", {"fpn_switches"}), ("stagenet.py", {"stage_switches"})):
        src = open(os.path.join(REPO, "mvsformer_amd", name), encoding="utf-8").read()
        assert re.search(r"^from \. import .*\bswitches as sw\b", src, re.M), name
        seen, forwards = set(), 0
        for fn in ast.walk(ast.parse(src)):
            if isinstance(fn, ast.FunctionDef):
                forwards += fn.name in ("forward", "forward_bank")
                if any(isinstance(n, ast.Name) and n.id == "sw" for n in ast.walk(fn)):
                    seen.add(fn.name)
        assert seen == readers and forwards >= 2, (name, seen)


# --------------------------------------------------------------------------------------------------------------------------- switch table
def _readme_rows():
    text = open(os.path.join(REPO, "README.md"), encoding="utf-8").read()
    block = text[text.index("### Environment switches of the Python package"):text.index("### Environment knobs of libmvs_hip.so")]
    return [line for line in block.splitlines() if line.startswith("| `MVS_")]


def test_readme_table_is_the_switch_table():
    rows = _readme_rows()
    assert [re.match(r"\| `(MVS_\w+)`", r).group(1) for r in rows] == list(switches.TABLE)           # every name, both ways, same order
    assert rows == [r for r in switches.readme_table().splitlines() if r.startswith("| `MVS_")]     # and nothing the table does not say


def test_only_switches_py_reads_the_environment_for_mvs_names():
    pkg = os.path.join(REPO, "mvsformer_amd")
    read = re.compile(r"os\.(environ|getenv)\b[^\n]*MVS_|MVS_[^\n]*os\.(environ|getenv)\b")
    for name in sorted(os.listdir(pkg)):
        if name.endswith(".py") and name != "switches.py":
            src = open(os.path.join(pkg, name), encoding="utf-8").read()
            assert not read.search(src), name
            if name != "sharding.py":                        # (the torch.distributed variables there are no switches)
                assert "os.environ" not in src and "os.getenv" not in src, name


def test_unknown_switch_raises(monkeypatch):
    monkeypatch.setenv("MVS_CONV_X4", "1")
    for reader in (switches.flag, switches.integer, switches.number, switches.text):
        with pytest.raises(KeyError):
            reader("MVS_CONV_X4")
    with pytest.raises(KeyError):
        switches.flag("MVS_CONV_X3")                         # a switch of another kind is a mistake too, not a truthiness guess


@pytest.mark.parametrize("name", [s.name for s in switches.TABLE.values() if s.kind in ("on", "off")])
def test_on_off_idioms(monkeypatch, name):
    """``on``: what ``os.environ.get(name, "1") != "0"`` gave; ``off``: what ``os.environ.get(name, "0") == "1"`` gave."""
    on = switches.TABLE[name].kind == "on"
    assert switches.TABLE[name].default is on
    monkeypatch.delenv(name, raising=False)
    assert switches.flag(name) is on
    for value, want in (("0", False), ("1", True), ("2", on)):
        monkeypatch.setenv(name, value)
        assert switches.flag(name) is want


def test_typed_and_validated_switches(monkeypatch):
    for name in ("MVS_CONV_X3_MIN_VOXELS", "MVS_CV_STORE_MAX_MB", "MVS_VIS", "MVS_CV_BWD", "MVS_FPN_X3", "MVS_CONV_X3", "MVS_CONV_WINO"):
        monkeypatch.delenv(name, raising=False)
    assert switches.integer("MVS_CONV_X3_MIN_VOXELS") == 40960 and switches.number("MVS_CV_STORE_MAX_MB") == 160.0
    assert (switches.text("MVS_VIS"), switches.text("MVS_CV_BWD"), switches.text("MVS_FPN_X3")) == (None, "own", "1")
    assert (switches.text("MVS_CONV_X3"), switches.text("MVS_CONV_WINO")) == ("1", None)
    monkeypatch.setenv("MVS_CONV_X3_MIN_VOXELS", "0")
    monkeypatch.setenv("MVS_CV_STORE_MAX_MB", "0.5")
    assert switches.integer("MVS_CONV_X3_MIN_VOXELS") == 0 and switches.number("MVS_CV_STORE_MAX_MB") == 0.5
    for name, ok, bad in (("MVS_VIS", "wino", "winograd"), ("MVS_CV_BWD", "direct", "")):
        monkeypatch.setenv(name, ok)
        assert switches.text(name) == ok
        monkeypatch.setenv(name, bad)
        with pytest.raises(ValueError):
            switches.text(name)
    with pytest.raises(RuntimeError):                        # the site's own error type (ops.cv_aggregate_bwd raises MvsHipError)
        switches.text("MVS_CV_BWD", error=RuntimeError)
    for value in ("0", "strip", "anything"):                 # three-valued, not validated: 0 | strip | anything else
        monkeypatch.setenv("MVS_FPN_X3", value)
        assert switches.text("MVS_FPN_X3") == value
