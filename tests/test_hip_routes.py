"""Which kernels the regularizers launch under each switch set, on ONE live network with no cache reset between the sets, against the launch
orders recorded before the routing was gathered into module.conv_route / deconv_route / tail_route (test_hip_routes.json: launch tags only,
from a fresh network per switch set).  The "paths agree" tests elsewhere would pass if every switch set took the same route; this one would not."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SETS = [{}, {"MVS_CONV_X3_MIN_VOXELS": "0"}, {"MVS_CONV_X3": "0"}, {"MVS_CONV_X3": "0", "MVS_CONV_WINO": "1"},
        {"MVS_CONV_X3_MIN_VOXELS": "0", "MVS_TAIL": "fp32"}, {"MVS_FUSE_PROB": "0"}]
SWITCHES = sorted({k for env in SETS for k in env})
CASES = {"costregnet": ("CostRegNet", lambda n, x: n(x), (1, 8, 8, 16, 24)),
         "costregnet3d_logits": ("CostRegNet3D", lambda n, x: n.logits(x), (1, 8, 4, 64, 96)),
         "costregnet3d_forward": ("CostRegNet3D", lambda n, x: n(x), (1, 8, 4, 64, 96))}


def _name(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_hip_routes.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", sorted(CASES))
def test_switch_sets_take_the_recorded_routes(dev, monkeypatch, recorded, case):
    import mvsformer_amd as m
    from mvsformer_amd import ops
    cls, run, shape = CASES[case]
    torch.manual_seed(3)
    net = getattr(m, cls)(8, 8).eval()
    m.randomize_bn_(net, 5)
    net = net.to(dev)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(11)).to(dev)
    orders, outs = {}, {}
    for env in SETS:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with torch.no_grad(), ops.kernel_timer() as kt:
            outs[_name(env)] = run(net, x)
        # on a live network the pack launches of a rebuild come before the layer launches: compared without them (as recorded)
        orders[_name(env)] = [t for t in kt.order if "pack" not in t and "prepare" not in t]
    for name, order in orders.items():
        print(case, name, order)
        assert order == recorded[case][name], (case, name)
    assert len({tuple(o) for o in orders.values()}) > 1, "every switch set took the same route"
    ref = outs["MVS_CONV_X3=0"]
    s = ref.abs().max().item()
    for name, y in outs.items():
        assert y.shape == ref.shape and (y - ref).abs().max().item() < 5e-6 * s, (case, name)
