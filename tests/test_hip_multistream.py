"""Run-to-run reproducibility under concurrent HIP streams: 30 full-size config-2 cascades spread over
three streams must be BIT-equal to the single-stream result, on the default kernel path and on the two opt-in Winograd paths that were
the victims of the round-3 finding (with packed fp32 instructions in the build, the Winograd convolution, the Winograd visibility CNN and
the fused conv11+prob tail returned results that differed from run to run when split-form bf16-MFMA kernels shared their CUs).

This file is also the reproducer: ``python tests/test_hip_multistream.py [N]`` prints, per variant, how many of N cascades differ and in
which stage outputs (``MVS_HIP_LIB=<path>`` points the package at an alternative build of the library, e.g. ``make -C mvsformer_amd/csrc
variants`` builds the library with packed fp32 allowed everywhere / only in the victims / only in the split-form kernels)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

VARIANTS = {"default": {}, "conv_wino": {"MVS_CONV_WINO": "1", "MVS_CONV_X3": "strided"}, "vis_wino": {"MVS_VIS": "wino"}}
KEYS = ("refined_depth", "photometric_confidence")


def _stage_outputs(o):
    out = {k: o[k] for k in KEYS}
    for i in range(1, 5):
        out["stage%d.prob_volume_pre" % i] = o["stage%d" % i]["prob_volume_pre"]
        out["stage%d.sim_depth" % i] = o["stage%d" % i]["sim_depth"]
    return out


def run_variant(env, n_runs, dev, H=1152, W=1536):
    """-> list of (run index, [names of differing outputs]) for the runs that are not bit-equal to the single-stream reference."""
    import mvsformer_amd as m
    from mvsformer_amd import synth
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        torch.manual_seed(0)
        net = m.CascadeMVS().eval()
        m.randomize_bn_(net, seed=1)
        net = net.to(dev)
        feats, proj, dv, _ = synth.make_inputs(5, H, W, seed=0, device=dev)
        tmp = [5.0, 5.0, 5.0, 1.0]
        ref = _stage_outputs(net(feats, proj, dv, tmp=tmp))
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream(device=dev) for _ in range(3)]
        bad = []
        for base in range(0, n_runs, 6):                     # six cascades in flight at a time (memory: ~1.3 GB of outputs each)
            outs = []
            for i in range(base, min(base + 6, n_runs)):
                with torch.cuda.stream(streams[i % 3]):
                    outs.append((i, _stage_outputs(net(feats, proj, dv, tmp=tmp))))
            torch.cuda.synchronize()
            for i, o in outs:
                diff = [k for k, v in o.items() if not torch.equal(v, ref[k])]
                if diff:
                    bad.append((i, diff))
            del outs
        return bad
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_three_stream_cascades_bit_equal_to_single_stream(dev, variant):
    bad = run_variant(VARIANTS[variant], 30, dev)
    assert not bad, "%d of 30 three-stream cascades differ from the single-stream result: %s" % (len(bad), bad[:4])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    d = torch.device("cuda:0")
    for name in sorted(VARIANTS):
        bad = run_variant(VARIANTS[name], n, d)
        print("lib=%s variant=%s: %d of %d three-stream cascades differ from the single-stream result%s" % (
            os.environ.get("MVS_HIP_LIB", "libmvs_hip.so"), name, len(bad), n, (": " + str(bad[:3])) if bad else ""), flush=True)
