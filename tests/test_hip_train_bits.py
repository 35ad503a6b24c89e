"""Bit pin of the training BatchNorm / bf16 convolution entry points against the commit BEFORE the BatchNorm finalize and the convolution
work plan were gathered into csrc/bn_core.h and csrc/bf16_conv_plan.h.  test_hip_train_bits.json holds the sha256 of the raw bytes of every
output; it was recorded by running this module as a script (``python tests/test_hip_train_bits.py OUT.json``) in a checkout of that parent
commit, and is NEVER regenerated from the code under test: a digest that moves is a change of arithmetic (an expression reordered, a
float/double step moved, a reduction walked in another order), which is what that refactor - and the next one - must not do.  Every input
comes from a seeded CPU generator; only ``ops`` functions that existed in the parent are used."""
import hashlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
# (name, cin, cout, gather, stride, input [B,D,H,W], taps, groups)
CONVS = [("c8_16_four_per_block", 8, 16, 0, (1, 1), (4, 4, 12, 40), 27, (1, 2)),
         ("c32_32_ksplit", 32, 32, 0, (1, 1), (2, 2, 4, 20), 27, (1, 2)),
         ("t16_8_two_parity", 16, 8, 1, (2, 2), (2, 2, 4, 10), 27, (1,)),
         ("c8_8_taps9_ragged", 8, 8, 0, (1, 1), (2, 1, 6, 70), 9, (1,))]


def _rand(seed, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale + shift


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _put(out, prefix, names, tensors):
    assert len(names) == len(tensors), prefix
    for n, t in zip(names, tensors):
        out["%s/%s" % (prefix, n)] = _digest(t)


def _bn_params(C, seed, dev):
    return [(_rand(seed, C, scale=0.3, shift=1.0)).to(dev), _rand(seed + 1, C, scale=0.2).to(dev), _rand(seed + 2, C, scale=0.1).to(dev),
            (_rand(seed + 3, C).abs() + 0.5).to(dev)]


def fp32_cases(dev):
    from mvsformer_amd import ops
    out = {}
    x = _rand(1, 2, 8, 3, 5, 7, scale=1.5, shift=0.7).to(dev)
    sums = ops.bn_stats(x)
    _put(out, "bn_stats", ["sums"], [sums])
    n = 2 * 3 * 5 * 7
    g, b, rm, rv = _bn_params(8, 10, dev)
    _put(out, "bn_finalize", ["scale", "shift", "mean", "invstd", "rm", "rv"], list(ops.bn_finalize(sums, g, b, rm, rv, 0.1, 1e-5, n)) + [rm, rv])
    g, b, rm, rv = _bn_params(4, 20, dev)
    _put(out, "bn_finalize_grouped", ["scale", "shift", "mean", "invstd", "rm", "rv"],
         list(ops.bn_finalize_grouped(sums, g, b, rm, rv, 0.1, 1e-5, n, 2)) + [rm, rv])
    g, b, rm, rv = _bn_params(8, 30, dev)
    cd = torch.tensor([float(n // 4096), float(n % 4096)], device=dev)
    _put(out, "bn_finalize_count_dev", ["scale", "shift", "mean", "invstd", "rm", "rv"],
         list(ops.bn_finalize(sums, g, b, rm, rv, 0.1, 1e-5, 1.0, cd)) + [rm, rv])
    return out


def bf16_bn_cases(dev):
    from mvsformer_amd import ops
    out = {}
    for name, shape, groups, with_res in (("g1", (2, 3, 5, 7, 8), 1, False), ("g2_res_relu", (4, 3, 5, 7, 16), 2, True)):
        C = shape[-1]
        x = _rand(40 + C, *shape, scale=1.3, shift=0.4).to(torch.bfloat16).to(dev)
        res = _rand(41 + C, *shape).to(torch.bfloat16).to(dev) if with_res else None
        g, b, rm, rv = _bn_params(C, 50 + C, dev)
        nbt = torch.zeros(1, dtype=torch.int64, device=dev)
        y, sc, sh, mu, istd = ops.bf16_bn_train_fwd(x, res, with_res, g, b, rm, rv, 0.1, 1e-5, groups, nbt)
        _put(out, "bf16_bn_train_fwd/" + name, ["y", "scale", "shift", "mean", "invstd", "rm", "rv", "nbt"], [y, sc, sh, mu, istd, rm, rv, nbt])
        dy = _rand(42 + C, *shape).to(torch.bfloat16).to(dev)
        sums = ops.bf16_bn_bwd_reduce(dy, x, sc, sh, mu, istd, with_res, groups)
        _put(out, "bf16_bn_bwd_reduce/" + name, ["sums"], [sums])
        count = x.numel() // C // groups
        gg = g.repeat(groups)
        dx = ops.bf16_bn_bwd_apply(dy, x, sc, sh, mu, istd, gg, sums, count, with_res, None, groups)
        dx2, dgb = ops.bf16_bn_bwd_apply(dy, x, sc, sh, mu, istd, gg, sums, count, with_res, None, groups, True)
        _put(out, "bf16_bn_bwd_apply/" + name, ["dx", "dx_with_dgb", "dgb"], [dx, dx2, dgb])
    return out


def conv_cases(dev):
    from mvsformer_amd import ops
    out = {}
    for name, cin, cout, gather, stride, shape, taps, groups_set in CONVS:
        seed = 100 + cin + 2 * cout + taps
        x = _rand(seed, *shape, cin).to(torch.bfloat16).to(dev)
        wshape = ((cout, cin) if gather == 0 else (cin, cout)) + ((3, 3, 3) if taps == 27 else (3, 3))
        w = _rand(seed + 1, *wshape, scale=0.1).to(dev)
        wp = ops.bf16_pack(w, gather, cin, cout) if taps == 27 else ops.PackTable([(w, 0, cin, cout)]).run()[0]
        for groups in groups_set:
            key = "%s/g%d" % (name, groups)
            if taps == 27:
                _put(out, "bf16_conv3d_stats/" + key, ["y", "sums"], ops.bf16_conv3d_stats(x, wp, cin, cout, gather, stride, groups))
            g, b, rm, rv = _bn_params(cout, seed + 2, dev)
            nbt = torch.zeros(1, dtype=torch.int64, device=dev)
            y, z, st = ops.bf16_conv3d_bn_fwd(x, wp, cin, cout, gather, stride, None, True, g, b, rm, rv, 0.1, 1e-5, groups, nbt, taps)
            _put(out, "bf16_conv3d_bn_fwd/" + key, ["y", "z", "stats", "rm", "rv", "nbt"], [y, z, st, rm, rv, nbt])
            # the backward form: this convolution's output is the gradient arriving at a BatchNorm(+ReLU) whose input was bn_y
            bn_y = _rand(seed + 6, *y.shape, scale=1.2, shift=0.3).to(torch.bfloat16).to(dev)
            bn4 = torch.stack([_rand(seed + 7, groups * cout, scale=0.2, shift=1.0), _rand(seed + 8, groups * cout, scale=0.5),
                               _rand(seed + 9, groups * cout, scale=0.3, shift=0.3), _rand(seed + 10, groups * cout).abs() + 0.5]).to(dev)
            addend = _rand(seed + 11, *y.shape).to(torch.bfloat16).to(dev)
            _put(out, "bf16_conv3d_bnbwd/" + key, ["dz", "sums"], ops.bf16_conv3d_bnbwd(x, wp, cin, cout, gather, stride, bn_y, bn4, True, groups, taps))
            _put(out, "bf16_conv3d_bnbwd/" + key + "/addend", ["dz", "sums"],
                 ops.bf16_conv3d_bnbwd(x, wp, cin, cout, gather, stride, bn_y, bn4, True, groups, taps, addend))
    return out


FAMILIES = {"fp32_bn": fp32_cases, "bf16_bn": bf16_bn_cases, "bf16_conv": conv_cases}


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(HERE, "test_hip_train_bits.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_training_outputs_keep_the_parents_bits(recorded, family):
    got = FAMILIES[family](torch.device("cuda:0"))
    torch.cuda.synchronize()
    assert sorted(got) == sorted(recorded[family]), "the set of pinned outputs changed"
    moved = [k for k in sorted(got) if got[k] != recorded[family][k]]
    assert not moved, "outputs whose bytes differ from the parent commit's: %s" % moved


if __name__ == "__main__":          # recording: run in a checkout of the parent commit only (see the docstring)
    sys.path.insert(0, os.path.dirname(HERE))
    digests = {k: f(torch.device("cuda:0")) for k, f in sorted(FAMILIES.items())}
    torch.cuda.synchronize()
    with open(sys.argv[1], "w") as fh:
        json.dump(digests, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded %d digests" % sum(len(v) for v in digests.values()))
