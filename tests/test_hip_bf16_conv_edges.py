"""The bf16 training convolutions (``bf16_conv_kernel`` with its epilogue and fused-statistics forms, ``bf16_wgrad_kernel`` +
``bf16_wgrad_reduce_kernel`` of csrc/bf16_train.hip) through ``mvsformer_amd.ops`` against float64 on each side of every branch of their
work plans (``mvsplan::conv_plan``, ``wgrad_plan``).  Cases, references and the derivation of the per-element bounds:
``tests/bf16_conv_edge_util.py``; that the cases reach what they claim, and that the bounds reject eight subtly wrong kernels:
``tests/test_bf16_conv_edge_refs.py`` (CPU).  The two forms of the K loop are selected by shape, never by MVS_BF16_KSPLIT_ITEMS (read once
per process).  Every test prints ``BF16EDGE <case> <output> max|err| share-of-bound``; the comparison is over ALL elements."""
import pytest
import torch

import bf16_conv_edge_util as U

pytestmark = pytest.mark.gpu

# Largest share of the bound per family when recorded on an MI355X: bf16 outputs 0.995 (the 2^-8 rounding term dominates: the correctly
# rounded reference reaches 0.995 too), the two K-loop forms against each other 0.46, forward sums / stats4 / running statistics 0.044,
# bnbwd sums 0.006, dW 0.010 (0.23 on the two-voxel probes), the integer-operand dW exact.


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _check(case, what, got, ref, bound):
    got = torch.as_tensor(got).detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (case, what, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), (case, what)
    err, sh = U.share(got, ref, bound)
    print("BF16EDGE %-34s %-14s err %.3e  share %.3f" % (case, what, err, sh))
    assert sh <= 1.0, "%s %s: |got - float64| reaches %.3f of its bound (max err %.3e)" % (case, what, sh, err)
    return sh


def _pack(ops, w, c, dev):
    """Forward layout of the module's weight: Conv3d ``[cout,cin,...]`` src 0, ConvTranspose3d ``[cin,cout,...]`` src 1; 2-D through a PackTable."""
    w = w.to(dev).contiguous()
    if c.taps == 9:
        return ops.PackTable([(w, 0, c.cin, c.cout)]).run()[0]
    return ops.bf16_pack(w, c.gather, c.cin, c.cout)


def _run_conv(ops, c, t, dev, x=None):
    x = U.to_cl(t["x"] if x is None else x).to(dev)
    wp = _pack(ops, t["w"], c, dev)
    if c.taps == 9:
        return ops.bf16_conv3d(x, wp, c.cin, c.cout, c.gather, c.stride, taps=9)
    return ops.bf16_conv3d(x, wp, c.cin, c.cout, c.gather, c.stride,
                           scale=t["scale"].to(dev) if c.scale else None, shift=t["shift"].to(dev) if c.scale else None,
                           residual=U.to_cl(t["residual"]).to(dev) if c.residual else None, relu=c.relu)


# ------------------------------------------------------------------------------------------------------------------- bf16_conv_kernel
@pytest.mark.parametrize("name", [c.name for c in U.CONV_CASES])
def test_conv_vs_fp64(dev, name):
    """Row chunks, column parities, every dispatched instance (K split below 768 items, four items per block above), the epilogue."""
    from mvsformer_amd import ops
    c = U.CONV_CASE[name]
    y = _run_conv(ops, c, U.conv_inputs(c), dev)
    assert y.dtype == torch.bfloat16
    _check(name, "y", U.from_cl(y), *U.conv_expect(c))


@pytest.mark.parametrize("c", U.KSPLIT_CASES, ids=[c.name for c in U.KSPLIT_CASES])
def test_ksplit_both_sides_of_the_threshold(dev, c):
    """The batch of two (774 items: four per block, two idle wavefronts at the end) and each sample alone (387 items: K split) on the same
    data: both against float64, and against each other within twice the accumulation term - two correct fp32 sums in different orders, K u32 S
    each.  That holds for the fp32 values BEFORE the rounding; an output lies within half a bf16 spacing of its own, so the outputs may differ
    by 2 K u32 S + the two half spacings (taken exactly, at the device's values).  No bit equality: the order differs by design."""
    from mvsformer_amd import ops
    t = U.conv_inputs(c)
    ref, bound = U.conv_expect(c)
    both = U.from_cl(_run_conv(ops, c, t, dev))
    _check(c.name, "four-per-block", both, ref, bound)
    acc = U.accumulation_term(c)
    for b in range(c.B):
        one = U.from_cl(_run_conv(ops, c._replace(B=1), t, dev, x=t["x"][b:b + 1]))
        _check(c.name, "ksplit[%d]" % b, one, ref[b:b + 1], bound[b:b + 1])
        _check(c.name, "forms[%d]" % b, one, both[b:b + 1], 2.0 * acc[b:b + 1] + U.bf16_half_ulp(one) + U.bf16_half_ulp(both[b:b + 1]))


# ------------------------------------------------------------------------------------------------------------------- fused statistics forms
def _stat_args(ops, name, dev):
    t = U.stat_inputs(name)
    c = U.REFUSED_CASE if name == U.REFUSED_CASE.name else U.STAT_CASE[name]
    return c, t, U.to_cl(t["x"]).to(dev), _pack(ops, t["w"], t["case"], dev)


@pytest.mark.parametrize("name", [c.name for c in U.STAT_CASES if c.taps == 27])
def test_conv_stats_vs_fp64(dev, name):
    """``bf16_conv3d_stats``: the output against float64, the sums against float64 sums of that output."""
    from mvsformer_amd import ops
    c, t, x, wp = _stat_args(ops, name, dev)
    y, sums = ops.bf16_conv3d_stats(x, wp, c.cin, c.cout, c.gather, c.stride, c.groups)
    yd = U.from_cl(y)
    _check(name, "stats y", yd, *U.stat_conv_expect(name))
    s1, s2, b1, b2 = U.fwd_sums_expect(yd, c.groups)
    n = c.groups * c.cout
    assert sums.dtype == torch.float64 and sums.numel() == 2 * n
    _check(name, "stats sum", sums[:n], s1, b1)
    _check(name, "stats sumsq", sums[n:], s2, b2)


@pytest.mark.parametrize("relu,with_res", [(True, True), (False, False)], ids=["relu+res", "plain"])
@pytest.mark.parametrize("name", [c.name for c in U.STAT_CASES])
def test_conv_bn_fwd_vs_fp64(dev, name, relu, with_res):
    """``bf16_conv3d_bn_fwd``: y against float64; ``stats4``, the running statistics and ``num_batches_tracked`` against ``mvsbn::finalize`` /
    ``running_update`` in double on float64 sums of the device's y; z against the affine form of the device's y and ``stats4``."""
    from mvsformer_amd import ops
    c, t, x, wp = _stat_args(ops, name, dev)
    res = U.to_cl(t["residual"]).to(dev) if with_res else None
    rm, rv = t["running_mean"].clone().to(dev), t["running_var"].clone().to(dev)
    nbt = torch.tensor(3, dtype=torch.int64, device=dev)
    y, z, st = ops.bf16_conv3d_bn_fwd(x, wp, c.cin, c.cout, c.gather, c.stride, res, relu, t["gamma"].to(dev), t["beta"].to(dev), rm, rv,
                                      t["momentum"], t["eps"], c.groups, nbt, c.taps)
    yd = U.from_cl(y)
    _check(name, "bn_fwd y", yd, *U.stat_conv_expect(name))
    s1, s2, b1, b2 = U.fwd_sums_expect(yd, c.groups)
    count = float(yd.numel() // (c.groups * c.cout))
    e = U.finalize_expect(s1, s2, b1, b2, count, t["gamma"], t["beta"], t["eps"], t["momentum"], t["running_mean"], t["running_var"], c.groups)
    st = st.cpu()
    for i, k in enumerate(("scale", "shift", "mean", "invstd")):
        _check(name, "bn_fwd " + k, st[i], *e[k])
    assert torch.equal(st[4], t["gamma"].repeat(c.groups))
    _check(name, "bn_fwd run_mean", rm, *e["running_mean"])
    _check(name, "bn_fwd run_var", rv, *e["running_var"])
    assert int(nbt) == 3 + c.groups
    _check(name, "bn_fwd z", U.from_cl(z), *U.affine_expect(yd, st[0], st[1], relu, t["residual"] if with_res else None, c.groups))


@pytest.mark.parametrize("with_addend", [False, True], ids=["alone", "addend"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("name", [c.name for c in U.STAT_CASES])
def test_conv_bnbwd_vs_fp64(dev, name, relu, with_addend):
    """``bf16_conv3d_bnbwd``: dz against the float64 convolution + ``addend``; the two BatchNorm backward sums against float64 sums over the
    device's dz with the mask decided exactly (5 % of the pre-activations are exactly 0 and must mask to 0); no element excluded."""
    from mvsformer_amd import ops
    c, t, x, wp = _stat_args(ops, name, dev)
    addend = U.to_cl(t["addend"]).to(dev) if with_addend else None
    dz, sums = ops.bf16_conv3d_bnbwd(x, wp, c.cin, c.cout, c.gather, c.stride, U.to_cl(t["bn_y"]).to(dev), t["bn4"].to(dev), relu, c.groups,
                                     c.taps, addend)
    dzd = U.from_cl(dz)
    _check(name, "bnbwd dz", dzd, *U.stat_conv_expect(name, with_addend))
    s1, s2, b1, b2 = U.bwd_sums_expect(dzd, t["bn_y"], t["bn4"], relu, c.groups)
    n = c.groups * c.cout
    assert sums.dtype == torch.float32 and sums.numel() == 2 * n
    _check(name, "bnbwd sum g", sums[:n], s1, b1)
    _check(name, "bnbwd sum g*xhat", sums[n:], s2, b2)


def test_grouped_rows_that_straddle_groups_are_refused(dev):
    """groups = 2, four items per block, 3 items per sample: both fused forms raise."""
    from mvsformer_amd import ops
    c, t, x, wp = _stat_args(ops, U.REFUSED_CASE.name, dev)
    with pytest.raises(ops._lib.MvsHipError):
        ops.bf16_conv3d_bn_fwd(x, wp, c.cin, c.cout, c.gather, c.stride, None, True, t["gamma"].to(dev), t["beta"].to(dev), None, None, 0.1, 1e-5,
                               c.groups, None, c.taps)
    with pytest.raises(ops._lib.MvsHipError):
        ops.bf16_conv3d_bnbwd(x, wp, c.cin, c.cout, c.gather, c.stride, U.to_cl(t["bn_y"]).to(dev), t["bn4"].to(dev), True, c.groups, c.taps)


# ------------------------------------------------------------------------------------------------------------------- bf16_wgrad_kernel
@pytest.mark.parametrize("name", [c.name for c in U.WGRAD_CASES])
def test_wgrad_vs_fp64(dev, name):
    """``ops.bf16_conv3d_wgrad`` elementwise against the float64 sum: patch edges in all three axes, PH = 8 / 4 / 2, ragged depth segments,
    ``Bt`` of 2 p and 2 p - 1, every instance, two channel groups, more work items than blocks; entries whose window lies outside ``Bt``
    (bound 0) exactly 0."""
    from mvsformer_amd import ops
    c = U.WGRAD_CASE[name]
    A, Bt = U.wgrad_inputs(name)
    dW = ops.bf16_conv3d_wgrad(A.to(torch.bfloat16).to(dev), Bt.to(torch.bfloat16).to(dev), c.stride, c.taps, c.cb_out)
    ref, bound = U.wgrad_expect(name)
    assert dW.dtype == torch.float32
    _check(name, "dW", dW, ref, bound)
    if c.probe:
        outside = bound == 0
        assert int(outside.sum()) > 0 and bool((dW.cpu()[outside] == 0).all())
