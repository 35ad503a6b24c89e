"""Which kernel an eval-mode regularizer layer takes (mvsformer_amd.module.conv_route / deconv_route / tail_route: pure functions, no GPU, no
library) and the MVS_* switch table (mvsformer_amd.switches) with its README rendering."""
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
