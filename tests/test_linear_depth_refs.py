"""Pins the references of tests/test_hip_linear_depth.py without a GPU: the plain-torch restatement of the two linear schedulers
(tests/linear_depth_util.py) reproduces the REAL reference's outputs (tests/golden/linear_depth_sched.npz) bit for bit in fp32, the restated
regression / mixup heads' float64 autograd gradients are self-consistent, and the seeded head inputs keep the mixup head's undecided pixels
under the cap the GPU test allows."""
import numpy as np
import pytest
import torch

from conftest import load_golden

import linear_depth_util as lu


def test_schedulers_restatement_equals_the_reference_bitwise():
    g = load_golden("linear_depth_sched.npz")
    rng = lu.init_range_inputs()
    for D, H, W in lu.INIT_CASES:
        got = lu.init_range(rng, D, H, W)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy(), g["init_D%d" % D]), D
        assert (got[:, 1:] > got[:, :-1]).all()             # linear hypotheses ascend with d
    prev, step = lu.schedule_range_inputs()
    for D, H, W in lu.SCHED_CASES:
        c = lu.clamped(prev, step, D)
        assert not c[0].any() and 0 < int(c[1].sum()) < c[1].numel()     # the clamp sits next to unclamped neighbours
        got = lu.schedule_range(prev, D, step, H, W)
        assert np.array_equal(got.numpy(), g["sched_D%d_%dx%d" % (D, H, W)]), (D, H, W)
        assert got.min() >= 0.01


@pytest.mark.parametrize("head", ["reg", "mixup"])
def test_head_restatement_gradcheck(head):
    pre, hyp, _, _ = lu.head_inputs(4, 2, 3, seed=5)
    pre, hyp = pre.double().requires_grad_(True), hyp.double()
    assert lu.mixup_decided(pre.detach()).all()
    fn = (lambda p: lu.reg_head(p, hyp)[:2]) if head == "reg" else (lambda p: lu.mixup_head(p, hyp)[:2])
    assert torch.autograd.gradcheck(fn, (pre,), eps=1e-6, atol=1e-7, rtol=1e-5)


def test_mixup_head_formula_of_the_backward():
    """d(depth)/d(p_l) = (h_l - depth)/s with s = p_l + p_r + 1e-7: the closed form the kernel uses against autograd in float64."""
    pre, hyp, r_depth, _ = lu.head_inputs(5, 5, 7, seed=6)
    pre, hyp = pre.double().requires_grad_(True), hyp.double()
    prob, depth, _, idx = lu.mixup_head(pre, hyp)
    (dprob,) = torch.autograd.grad((depth * r_depth.double()).sum(), prob, retain_graph=True)
    i = idx.unsqueeze(1)
    pl, pr = prob.gather(1, i), prob.gather(1, i + 1)
    hl, hr = hyp.gather(1, i), hyp.gather(1, i + 1)
    s = pl + pr + 1e-7
    want = torch.zeros_like(prob).scatter(1, i, r_depth.double().unsqueeze(1) * (hl - depth.unsqueeze(1)) / s)
    want = want.scatter(1, i + 1, r_depth.double().unsqueeze(1) * (hr - depth.unsqueeze(1)) / s)
    assert (dprob - want).abs().max() <= 1e-9 * want.abs().max()


def test_mixup_inputs_keep_undecided_pixels_under_the_cap():
    """At most 1 % of the pixels of the GPU test's seeded inputs may be left out of its depth / dpre comparison."""
    for D in (2, 4, 5, 8, 32):
        for H, W in ((5, 7), (3, 90)):
            pre = lu.head_inputs(D, H, W, seed=lu.HEAD_SEED + D)[0]
            assert (~lu.mixup_decided(pre)).double().mean().item() <= 0.01, (D, H, W)
