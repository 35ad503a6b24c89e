"""CPU-side checks of tests/test_hip_bf16_conv_edges.py (no GPU): the float64 references of ``bf16_conv_edge_util`` agree with torch
autograd through ``conv3d`` / ``conv_transpose3d``, the case tables reach the branches of ``mvsplan::conv_plan`` and ``wgrad_plan`` they claim
(read from the launchers' own planner), correct outputs in other precisions stay inside every bound, and eight subtly wrong kernels - built
by perturbing the reference's own result, never a kernel - land outside them (the seventh and eighth: a dropped voxel, and a block that
skips its second work item, on the case with more work items than blocks)."""
import pytest
import torch
import torch.nn.functional as F

import bf16_conv_edge_util as U


def _plan(c):
    return U.plan_conv(c.B, c.cin, c.D, c.H, c.W, c.gather, c.stride[0], c.stride[1], c.taps)


def _wplan(c):
    return U.plan_wgrad(c.nb, c.CA, c.CB, c.Dp, c.Hp, c.Wp, c.stride[1])


# ------------------------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("stride", U.STRIDES)
def test_references_in_float32_are_torch_autograd(stride):
    """The data-gradient forms and the weight-gradient sums are the gradients of ``conv3d`` / ``conv_transpose3d`` (what the existing bf16
    layer tests compare with): a strided Conv3d's data gradient is the transposed form of the same weight read as ``[cin, cout]``, a
    stride-1 one the convolution with channels swapped and taps mirrored, a ConvTranspose3d's the strided convolution; ``dW`` of a Conv3d is
    ``wgrad_sum(dy, x)``, of a ConvTranspose3d ``wgrad_sum(x, dy)``."""
    g = torch.Generator().manual_seed(5)
    s3 = (stride[0], stride[1], stride[1])
    cin, cout = 8, 16
    D, H, W = (3, 4, 6) if stride == (1, 1) else (4, 6, 10)             # even where strided: the transposed form returns 2x the grid
    x = U.bf(torch.randn(2, cin, D, H, W, generator=g)).requires_grad_(True)
    w = U.bf(torch.randn(cout, cin, 3, 3, 3, generator=g) / 15).requires_grad_(True)
    y = F.conv3d(x, w, None, stride=s3, padding=1)
    R = U.bf(torch.randn(y.shape, generator=g))
    (y * R).sum().backward()
    if stride == (1, 1):
        dx = U.conv_raw(R, w.detach().transpose(0, 1).flip(2, 3, 4), 0, stride, 27, torch.float32)
    else:
        dx = U.conv_raw(R, w.detach(), 1, stride, 27, torch.float32)
    dw = U.wgrad_sum(R.permute(0, 2, 3, 4, 1), x.detach().permute(0, 2, 3, 4, 1), stride, 27, None, torch.float32)
    for what, got, want in (("dx", dx, x.grad), ("dw", dw, w.grad)):
        err = (got - want).abs().max().item() / want.abs().max().item()
        print("autograd agreement conv s%d%d %s %.2e" % (stride + (what, err)))
        assert got.shape == want.shape and err < 2e-6, (what, err)
    if stride == (1, 1):
        return
    xt = U.bf(torch.randn(2, cout, 2, 3, 5, generator=g)).requires_grad_(True)
    wt = U.bf(torch.randn(cout, cin, 3, 3, 3, generator=g) / 15).requires_grad_(True)
    yt = F.conv_transpose3d(xt, wt, None, stride=s3, padding=1, output_padding=(s3[0] - 1, 1, 1))
    assert torch.equal(yt.detach(), U.conv_raw(xt.detach(), wt.detach(), 1, stride, 27, torch.float32))
    Rt = U.bf(torch.randn(yt.shape, generator=g))
    (yt * Rt).sum().backward()
    dxt = U.conv_raw(Rt, wt.detach(), 0, stride, 27, torch.float32)
    dwt = U.wgrad_sum(xt.detach().permute(0, 2, 3, 4, 1), Rt.permute(0, 2, 3, 4, 1), stride, 27, None, torch.float32)
    for what, got, want in (("dx", dxt, xt.grad), ("dw", dwt, wt.grad)):
        err = (got - want).abs().max().item() / want.abs().max().item()
        print("autograd agreement deconv s%d%d %s %.2e" % (stride + (what, err)))
        assert got.shape == want.shape and err < 2e-6, (what, err)


def test_wgrad_sum_2d_and_short_operand():
    """``taps`` = 9 is the centre depth plane of the 27; a ``Bt`` of 2 p - 1 is the 2 p one whose last plane / row / column is zero."""
    c = U.WGRAD_CASE["wg-2d-c16_8-cbout1"]
    A, Bt = U.wgrad_inputs(c.name)
    full = U.wgrad_sum(A, Bt, c.stride, 27, None, torch.float64)
    assert torch.equal(U.wgrad_expect(c.name)[0], full[:, :c.cb_out, 1])
    g = torch.Generator().manual_seed(1)
    A = torch.randn(1, 2, 3, 4, 8, generator=g).double()
    Bs = torch.randn(1, 3, 5, 7, 8, generator=g).double()
    Bl = F.pad(Bs, (0, 0, 0, 1, 0, 1, 0, 1))
    assert torch.equal(U.wgrad_sum(A, Bs, (2, 2), 27, None, torch.float64), U.wgrad_sum(A, Bl, (2, 2), 27, None, torch.float64))


# ------------------------------------------------------------------------------------------------------------------- what the tables reach
def test_conv_plan_formulas_on_known_shapes():
    p = U.plan_conv(2, 64, 3, 129, 5, 0, 1, 1)
    assert (p.Do, p.Ho, p.Wo, p.nwchunks, p.items_per_sample, p.items, p.ksplit, p.block_rows) == (3, 129, 5, 1, 387, 774, False, 194)
    p = U.plan_conv(2, 16, 2, 3, 65, 1, 2, 2, 27, 2)
    assert (p.Do, p.Ho, p.Wo, p.wpar, p.nwchunks, p.items_per_sample, p.rows_per_sample, p.samples) == (4, 6, 130, True, 2, 96, 24, 2)
    assert U.plan_conv(2, 8, 1, 3, 20, 0, 1, 1, 27, 2).rows_per_sample == -1 and U.plan_conv(2, 8, 1, 3, 20, 0, 1, 1, 27, 1).rows_per_sample == 2
    assert U.plan_conv(1, 32, 4, 4, 64, 0, 1, 1, 9).ksplit is False


def test_row_chunk_cases_reach_their_edges():
    rows = [c for c in U.CONV_CASES if c.name.startswith("row-")]
    for stride in U.STRIDES:
        cs = [c for c in rows if c.stride == stride]
        assert {_plan(c).Wo for c in cs} == {1, 15, 16, 17, 63, 64, 65, 129}
        assert {1, 2, 3} == {c.D for c in cs} == {c.H for c in cs}
        assert {_plan(c).nwchunks for c in cs} == {1, 2, 3}
        b1 = [_plan(c).items % 4 for c in cs if c.B == 1]
        assert 0 in b1 and set(b1) - {0}, "B = 1 with and without idle wavefronts in the last block"
        if stride[1] == 2:
            for Wo in (1, 15, 16, 17, 63, 64, 65, 129):
                assert {c.W for c in cs if _plan(c).Wo == Wo} == {2 * Wo - 1, 2 * Wo}
            assert any(c.H % 2 for c in cs) and any(c.H % 2 == 0 for c in cs)
        if stride[0] == 2:
            assert any(c.D % 2 for c in cs) and any(c.D % 2 == 0 for c in cs)
    assert all(c.gather == 0 and not _plan(c).ksplit for c in rows)


def test_parity_cases_reach_their_edges():
    par = [c for c in U.CONV_CASES if c.name.startswith("par-")]
    for stride in U.STRIDES[1:]:
        cs = [c for c in par if c.stride == stride]
        assert {c.W for c in cs} == {1, 31, 32, 33, 63, 64, 65}
        assert all(_plan(c).wpar for c in cs) and {_plan(c).nwchunks for c in cs} == {1, 2}
        assert min(_plan(c).Wo for c in cs) == 2 and max(_plan(c).Wo for c in cs) == 130
        assert {1, 2, 3} == {c.D for c in cs} == {c.H for c in cs}


def test_every_dispatched_instance_has_a_case():
    """<CIN, NT, GATHER, SD, SHW, KSPLIT> of ``launch_conv`` + the two 2-D ones; Cout = 8 (the ``co0 >= Cout`` skip) with every Cin."""
    nt = {8: 1, 16: 1, 32: 2, 64: 4}
    reached = {(c.cin, nt[c.cout], c.gather, c.stride, c.taps, _plan(c).ksplit) for c in U.CONV_CASES}
    for gather in (0, 1):
        for stride in U.STRIDES:
            for cin in (8, 16, 32, 64):
                for n in (1, 2, 4):
                    for ks in ((False, True) if cin >= 32 else (False,)):
                        assert (cin, n, gather, stride, 27, ks) in reached, (cin, n, gather, stride, ks)
            inst = [c for c in U.CONV_CASES if c.name.startswith("inst-g%d-s%d%d" % ((gather,) + stride))]
            assert {(c.cin, c.cout) for c in inst} == {(a, b) for a in (8, 16, 32, 64) for b in (8, 16, 32, 64)}
            assert all(_plan(c).nwchunks == 2 for c in inst), "chunk-crossing"
            big = [c for c in U.CONV_CASES if c.name.startswith("inst4-g%d-s%d%d" % ((gather,) + stride))]
            assert all(U.KSPLIT_ITEMS < _plan(c).items <= 800 and not _plan(c).ksplit for c in big) and len(big) == 6
    assert {(c.cin, c.cout) for c in U.CONV_CASES if c.taps == 9} == {(8, 8), (8, 16), (16, 8), (16, 16)}


def test_ksplit_cases_sit_on_both_sides_of_the_threshold():
    """Fails loudly if the default of MVS_BF16_KSPLIT_ITEMS moves: the case would otherwise go vacuous."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "mvsformer_amd", "csrc", "bf16_conv_plan.h")).read()
    m = re.search(r'env_int\("MVS_BF16_KSPLIT_ITEMS",\s*(\d+)\)', src)
    assert m and int(m.group(1)) == U.KSPLIT_ITEMS
    assert {c.cin for c in U.KSPLIT_CASES} == {32, 64}
    for c in U.KSPLIT_CASES:
        both, one = _plan(c), _plan(c._replace(B=1))
        assert (both.items, both.ksplit, both.items % 4) == (774, False, 2)
        assert (one.items, one.ksplit) == (387, True)


def test_epilogue_cases_cover_every_combination():
    for gather in (0, 1):
        got = {(c.scale, c.relu, c.residual) for c in U.CONV_CASES if c.name.startswith("epi-g%d" % gather)}
        assert len(got) == 7 and (False, False, False) not in got


def test_statistics_cases_reach_their_rows():
    P = {c.name: U.stat_plan(c) for c in U.STAT_CASES}
    p = P["st-b1-items6"]
    assert p.items % 4 == 2 and not p.ksplit and p.samples == 1
    p = P["st-b2-g1-ips3"]
    assert (p.items_per_sample, p.ksplit, p.samples, p.rows_per_sample, p.block_rows) == (3, False, 1, 2, 2)
    p = P["st-b2-g2-ips4"]
    assert (p.items_per_sample % 4, p.ksplit, p.samples, p.rows_per_sample) == (0, False, 2, 1)
    p = P["st-b4-g2-ksplit-ips3"]
    assert (p.items_per_sample, p.ksplit, p.samples, p.rows_per_sample, p.block_rows) == (3, True, 4, 3, 12)
    p = P["st-transposed-wo130"]
    assert p.wpar and p.Wo == 130 and p.nwchunks == 2 and p.rows_per_sample == 2
    assert U.STAT_CASE["st-2d"].taps == 9 and P["st-2d"].items == 6
    r = U.stat_plan(U.REFUSED_CASE)
    assert r.rows_per_sample == -1 and not r.ksplit and U.REFUSED_CASE.groups == 2
    for c in U.STAT_CASES:                                    # zero pre-activations are there, and exactly zero
        t = U.stat_inputs(c.name)
        sc, sh = U.per_sample(t["bn4"][0], c.B, c.groups, c.cout), U.per_sample(t["bn4"][1], c.B, c.groups, c.cout)
        pre32 = torch.addcmul(sh.expand_as(t["bn_y"]), t["bn_y"], sc.expand_as(t["bn_y"]))
        assert torch.equal(pre32.double(), t["bn_y"].double() * sc.double() + sh.double()), "the mask's fmaf is exact in fp32"
        assert bool((pre32[t["zero_at"]] == 0).all()) and int(t["zero_at"].sum()) >= 20


def test_wgrad_cases_reach_their_edges():
    P = {c.name: _wplan(c) for c in U.WGRAD_CASES}
    for c in U.WGRAD_CASES:
        p = P[c.name]
        assert p.PH == c.PH and (p.TA, p.TB) == c.inst, (c.name, p)
        assert c.nb * c.Dp * c.Hp * c.Wp <= 100000
        itemsB = (p.PH * c.stride[1] + 2) * (U.WG_PW * c.stride[1] + 2) * (c.CB // 8)
        assert itemsB <= 1024, "a shape the library refuses"
    grid = [c for c in U.WGRAD_CASES if c.name.startswith("wg-c")]
    assert {c.Wp for c in grid} == {15, 16, 17, 33} and {c.Dp for c in grid} == {1, 2, 3, 5}
    for PH in (8, 4, 2):
        assert {c.Hp - PH for c in grid if c.PH == PH} == {-1, 0, 1}
    assert {c.stride for c in grid} == set(U.STRIDES)
    for stride in U.STRIDES[1:]:
        assert {c.short for c in grid if c.stride == stride} == {False, True}
    assert {c.inst for c in U.WGRAD_CASES} >= {(1, 1), (2, 1), (2, 2), (1, 4)}
    assert any(P[c.name].nseg == 2 and P[c.name].dseg == 3 and c.Dp == 5 for c in grid), "ragged depth segments 3 + 2"
    assert any(c.taps == 9 and c.cb_out < c.CB for c in U.WGRAD_CASES)
    assert any(P[c.name].gy > 1 and c.CA == 64 and c.CB <= 16 for c in U.WGRAD_CASES)
    # (the block count is the one at PH = 8, so the PH = 4 / 2 cases with two patch rows also give a block a second work item)
    assert any(P[c.name].npatch > P[c.name].blocks for c in grid if c.PH < 8) and any(P[c.name].npatch <= P[c.name].blocks for c in grid)
    for name in U.MANY_ITEMS_CASES:
        p = P[name]
        assert (p.gy, p.npr, p.npc, p.nseg, p.dseg, p.npatch, p.blocks) == (2, 5, 13, 2, 2, 260, 256)
    A = U.wgrad_inputs("wg-items260-blocks256-tail")[0]
    assert int((A != 0).any(-1).sum()) == 4 * 2 * 8 * 16 and bool((A[0] == 0).all()) and bool((A[1, :, :32] == 0).all()) and bool((A[1, :, :, :176] == 0).all())
    assert bool((U.wgrad_expect("wg-items260-blocks256-int")[1] == 0).all())
    assert P[U.SEGMENT_CASE].nseg == 2
    for c in U.WGRAD_CASES:
        if c.probe:
            ref, bound = U.wgrad_expect(c.name)
            assert bool((bound[:, :, 2] == 0).all()) and bool((bound[:, :, :, 2] == 0).all()) and bool((bound[..., 2] == 0).all())
            assert bool((bound[:, :, :2, :2, :2] > 0).all()) and bool((ref[bound == 0] == 0).all())


# ------------------------------------------------------------------------------------------------------------------- the bounds hold ...
@pytest.mark.parametrize("group", ["row", "par", "inst-", "inst4", "epi"])
def test_correct_outputs_stay_inside_the_conv_bounds(group):
    """The reference rounded to bf16, and the fp32 evaluation of the layer rounded to bf16, inside every bound."""
    worst = 0.0
    for c in [c for c in U.CONV_CASES if c.name.startswith(group)]:
        ref, bound = U.conv_expect(c)
        for got in (U.bf(ref.float()), U.bf(U.conv_eval(c, torch.float32))):
            s = U.share(got, ref, bound)[1]
            worst = max(worst, s)
            assert s <= 1.0, (c.name, s)
    print("correct outputs, %s: worst share of the bound %.3f" % (group, worst))


def test_correct_outputs_stay_inside_the_wgrad_and_sum_bounds():
    for c in U.WGRAD_CASES:
        A, Bt = U.wgrad_inputs(c.name)
        ref, bound = U.wgrad_expect(c.name)
        assert U.inside(U.wgrad_sum(A, Bt, c.stride, c.taps, c.cb_out, torch.float32), ref, bound), c.name
    for c in U.STAT_CASES:
        t = U.stat_inputs(c.name)
        for addend in (False, True):
            ref, bound = U.stat_conv_expect(c.name, addend)
            dz = U.bf(ref.float())
            assert U.inside(dz, ref, bound)
            for relu in (False, True):
                s1, s2, b1, b2 = U.bwd_sums_expect(dz, t["bn_y"], t["bn4"], relu, c.groups)
                f = dz * ((t["bn_y"] * U.per_sample(t["bn4"][0], c.B, c.groups, c.cout) + U.per_sample(t["bn4"][1], c.B, c.groups, c.cout)) > 0).float() \
                    if relu else dz
                s1f = f.reshape(c.B // c.groups, c.groups, c.cout, -1).sum(dim=(0, 3)).reshape(-1)       # an fp32 sum in another order
                assert U.inside(s1f, s1, b1), c.name
        y = U.bf(U.stat_conv_expect(c.name)[0].float())
        s1, s2, b1, b2 = U.fwd_sums_expect(y, c.groups)
        assert U.inside((y * y).reshape(c.B // c.groups, c.groups, c.cout, -1).sum(dim=(0, 3)).reshape(-1), s2, (c.B * 4 + 1) * b2)


def test_finalize_expect_is_batchnorm():
    """``finalize_expect`` against ``torch.nn.functional.batch_norm`` in float64 (training mode, running statistics updated)."""
    g = torch.Generator().manual_seed(2)
    y = torch.randn(3, 8, 2, 3, 5, generator=g).double() * 2 + 1
    gamma, beta = torch.rand(8, generator=g).double() + 0.5, torch.randn(8, generator=g).double()
    rm, rv = torch.randn(8, generator=g).double(), torch.rand(8, generator=g).double() + 0.5
    s1, s2, b1, b2 = U.fwd_sums_expect(y, 1)
    mom, eps = 0.125, 2.0 ** -16                                # fp32-representable: finalize_expect holds them as the kernel does
    e = U.finalize_expect(s1, s2, b1, b2, 90.0, gamma, beta, eps, mom, rm, rv, 1)
    rm2, rv2 = rm.clone(), rv.clone()
    z = F.batch_norm(y, rm2, rv2, gamma, beta, True, mom, eps)
    mine = y * e["scale"][0].view(1, -1, 1, 1, 1) + e["shift"][0].view(1, -1, 1, 1, 1)
    assert (mine - z).abs().max().item() < 1e-12
    assert (e["running_mean"][0] - rm2).abs().max().item() < 1e-12 and (e["running_var"][0] - rv2).abs().max().item() < 1e-12
    assert all(bool((b > 0).all()) and bool((b < 1e-3 * (v.abs() + 1)).all()) for v, b in e.values())


# ------------------------------------------------------------------------------------------------------------------- ... and reject mutations
def _kernel_like(ref):
    return U.bf(ref.float())


def _first(prefix):
    return next(c for c in U.CONV_CASES if c.name.startswith(prefix))


def test_mutation_dropped_tap_at_a_border_voxel():
    for name, vox, tap in (("inst-g0-s11-c8_16", (0, 0, 0, 64), (1, 1, 0)), ("inst-g0-s22-c64_64", (0, 0, 0, 64), (2, 2, 0)),
                           (_first("row-s12-w257-").name, (0, 0, 0, 128), (1, 1, 1))):
        c = U.CONV_CASE[name]
        ref, bound = U.conv_expect(c)
        assert not U.inside(_kernel_like(U.mutate_drop_tap(c, *vox, tap)), ref, bound), name


def test_mutation_last_column_of_a_chunk_zeroed():
    for name, col in (("inst-g0-s11-c16_16", 63), (_first("row-s22-w257-").name, 127), ("inst-g1-s12-c16_8", 127), ("inst-g1-s22-c32_32", 126)):
        c = U.CONV_CASE[name]
        ref, bound = U.conv_expect(c)
        assert ref.shape[-1] > col
        assert not U.inside(_kernel_like(U.mutate_zero_column(c, col)), ref, bound), name


def test_mutation_parity_taps_swapped():
    for name in (_first("par-s12-w33-").name, "inst-g1-s22-c16_16", "epi-g1-affine+relu+res"):
        c = U.CONV_CASE[name]
        ref, bound = U.conv_expect(c)
        bad = U.mutate_swap_parity_taps(c)
        assert torch.equal(bad[..., 0::2], ref[..., 0::2]), "the even parity has one tap per axis: unchanged"
        assert not U.inside(_kernel_like(bad), ref, bound), name


@pytest.mark.parametrize("name", [c.name for c in U.STAT_CASES])
def test_mutation_relu_mask_and_addend_order(name):
    c, t = U.STAT_CASE[name], U.stat_inputs(name)
    dz = _kernel_like(U.stat_conv_expect(name, True)[0])
    s1, s2, b1, b2 = U.bwd_sums_expect(dz, t["bn_y"], t["bn4"], True, c.groups)
    m1, m2, _, _ = U.bwd_sums_expect(dz, t["bn_y"], t["bn4"], True, c.groups, ge=True)            # mask taken as >= 0
    assert not U.inside(m1, s1, b1), "sum g"
    # the second sum of a zero pre-activation is g (y - mean) invstd: rejected in every (group, channel) that has one with g != 0, y != mean
    mu = U.per_sample(t["bn4"][2], c.B, c.groups, c.cout)
    seen = U.group_sum((t["zero_at"] & (dz != 0) & (t["bn_y"] != mu)).double(), c.groups) > 0
    assert int(seen.sum()) >= c.groups * c.cout // 2, "most channels have such a voxel"
    assert bool(((m2 - s2).abs() > b2)[seen].all()), "sum g*xhat"
    assert bool((m2 == s2)[~seen].all())
    late = _kernel_like(U.stat_conv_expect(name, False)[0])                                         # addend added after the sums
    for relu in (False, True):
        s1, s2, b1, b2 = U.bwd_sums_expect(dz, t["bn_y"], t["bn4"], relu, c.groups)
        l1, l2, _, _ = U.bwd_sums_expect(late, t["bn_y"], t["bn4"], relu, c.groups)
        assert not U.inside(l1, s1, b1) and not U.inside(l2, s2, b2)


def _largest_term_voxel(name):
    """The voxel of ``A`` whose removal changes ``dW`` most (centre tap): where a dropped voxel is easiest to see - and the old criterion
    still does not."""
    A, Bt = U.wgrad_inputs(name)
    c = U.WGRAD_CASE[name]
    assert c.stride == (1, 1)
    score = A.abs().amax(-1) * Bt.abs().amax(-1)
    n, d, h, w = (int(v) for v in torch.unravel_index(score.argmax(), score.shape))
    return n, d, h, w


def test_mutation_dropped_voxel_and_what_the_old_criterion_saw():
    """One voxel missing from a ``dW`` sum of 1445: outside the elementwise bound, yet ``max|err| / max|dW| < 1e-2`` accepts it - the gap
    this suite closes.  Every other voxel of the case is tried at a stride of 97 as well."""
    name = U.OFFSET_CASE
    ref, bound = U.wgrad_expect(name)
    bad = U.mutate_drop_voxel(name, *_largest_term_voxel(name))
    err = (bad - ref).abs().max().item()
    print("dropped voxel: max|err| %.3f = %.2e of max|dW| %.1f; share of the bound %.1f" % (err, err / ref.abs().max().item(), ref.abs().max().item(),
                                                                                           U.share(bad.float(), ref, bound)[1]))
    assert not U.inside(bad.float(), ref, bound)
    assert U.old_criterion(bad.float(), ref), "the old criterion accepts a dropped voxel"
    c = U.WGRAD_CASE[name]
    for flat in range(0, c.Dp * c.Hp * c.Wp, 97):
        d, h, w = flat // (c.Hp * c.Wp), (flat // c.Wp) % c.Hp, flat % c.Wp
        bad = U.mutate_drop_voxel(name, 0, d, h, w).float()
        assert not U.inside(bad, ref, bound) and U.old_criterion(bad, ref), (d, h, w)
    # zero-mean operands: every small case of the table rejects it too
    for small in ("wg-c16_16-s11-d1h7w15-n1", "wg-c32_32-s22-d3h2w17-n1"):
        if small in U.WGRAD_CASE:
            r, b = U.wgrad_expect(small)
            assert not U.inside(U.mutate_drop_voxel(small, 0, 0, 0, 0).float(), r, b), small


@pytest.mark.parametrize("name", U.MANY_ITEMS_CASES)
def test_mutation_second_work_item_of_a_block_dropped(name):
    """The case with more work items than blocks (260 on 256): a block that returned after its first item - each of items 256 .. 259 in
    turn, and all four - lands outside the bound; so does one dropped voxel of such an item, and (integer operands) of any item."""
    c = U.WGRAD_CASE[name]
    p = _wplan(c)
    ref, bound = U.wgrad_expect(name)
    A, Bt = U.wgrad_inputs(name)
    assert U.inside(U.wgrad_sum(A, Bt, c.stride, c.taps, c.cb_out, torch.float32), ref, bound)
    for item in range(p.blocks, p.npatch):
        s = U.share(U.mutate_drop_item(name, item).float(), ref, bound)[1]
        print("%s without work item %d: share of the bound %.3g" % (name, item, s))
        assert s > 1.0, (name, item)
    n, d, h, w = U.wgrad_item_region(c, p.blocks)
    assert not U.inside(U.mutate_drop_voxel(name, n, d.start, h.start + 3, w.start + 5).float(), ref, bound)
    if c.data == "int":
        assert not U.inside(U.mutate_drop_voxel(name, 0, 1, 17, 100).float(), ref, bound)


def test_mutation_last_depth_segment_dropped():
    ref, bound = U.wgrad_expect(U.SEGMENT_CASE)
    assert not U.inside(U.mutate_drop_last_segment(U.SEGMENT_CASE).float(), ref, bound)
    ragged = [c.name for c in U.WGRAD_CASES if c.Dp == 5 and _wplan(c).nseg == 2 and not c.probe]
    assert len(ragged) >= 2
    for name in ragged:
        ref, bound = U.wgrad_expect(name)
        assert not U.inside(U.mutate_drop_last_segment(name).float(), ref, bound), name
