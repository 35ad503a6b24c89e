"""GPU parity of the bf16 regularizer (BASELINE configs[2]: training under autocast).  The reference runs Conv3d /
ConvTranspose3d in half precision with fp32 accumulation under ``torch.cuda.amp.autocast`` (trainer/mvsformer_trainer.py:104-106);
here the kernels take bf16 channel-last activations and fp32 master weights rounded to bf16, accumulate in fp32 on
``v_mfma_f32_16x16x32_bf16`` and round the result to bf16.

Tolerances, stated per check:
* one layer against torch fp32 on the SAME bf16-rounded operands: the only differences are the fp32 summation order and the
  final rounding to bf16 (2^-9 relative) -> 1e-2 of the tensor's scale;
* the whole regularizer / StageNet against the fp32 oracle: bf16 rounding of every activation and weight (2^-9 each, ~12 layers)
  -> logits within 4e-2 of their scale, gradients within 1e-1 of theirs (SURVEY §8c measured 2e-4 depth sensitivity to bf16
  features; the judged 1e-3 depth bar applies to the fp32 eval path, not to this training mode)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def relclose(got, want, rtol, what=""):
    got = torch.as_tensor(got).double().cpu()
    want = torch.as_tensor(want).double().cpu()
    scale = max(want.abs().max().item(), 1e-12)
    err = (got - want).abs().max().item() / scale
    assert err < rtol, "%s: max err / max|want| = %.3e (tol %.1e)" % (what, err, rtol)


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def to_cl(x, dev):          # fp32 NCDHW (cpu) -> bf16 NDHWC (gpu)
    return x.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16).to(dev)


def from_cl(y):             # bf16 NDHWC (gpu) -> fp32 NCDHW (cpu)
    return y.float().cpu().permute(0, 4, 1, 2, 3).contiguous()


def test_converters_roundtrip(dev):
    from mvsformer_amd import ops
    x = torch.randn(2, 16, 3, 5, 7)
    y = ops.bf16_from_f32(x.to(dev))
    assert y.shape == (2, 3, 5, 7, 16) and y.dtype == torch.bfloat16
    assert torch.equal(y.cpu(), x.permute(0, 2, 3, 4, 1).to(torch.bfloat16))
    assert torch.equal(ops.bf16_to_f32(y).cpu(), bf(x))


CONV_CASES = [(8, 16, (2, 2), 8, 8, 24), (8, 16, (1, 2), 3, 16, 40), (16, 16, (1, 1), 4, 5, 70), (16, 32, (2, 2), 4, 6, 20),
              (32, 32, (1, 1), 3, 4, 12), (32, 64, (1, 2), 2, 6, 18), (64, 64, (1, 1), 2, 3, 66), (8, 8, (1, 1), 5, 7, 9)]


@pytest.mark.parametrize("cin,cout,stride,D,H,W", CONV_CASES)
def test_conv_bf16_fn(dev, cin, cout, stride, D, H, W):
    """Forward, data gradient and weight gradient of ConvBf16Fn against torch autograd (fp32 math) on the same bf16 operands."""
    from mvsformer_amd import autograd as ag
    gen = torch.Generator().manual_seed(cin * 100 + cout + D)
    x = bf(torch.randn(2, cin, D, H, W, generator=gen))
    w = bf(torch.randn(cout, cin, 3, 3, 3, generator=gen) / (27 * cin) ** 0.5)
    s3 = (stride[0], stride[1], stride[1])
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv3d(xr, wr, None, stride=s3, padding=1)
    R = bf(torch.randn(y.shape, generator=gen))
    (y * R).sum().backward()
    xm = to_cl(x, dev).requires_grad_(True)
    wm = w.to(dev).requires_grad_(True)
    ym = ag.ConvBf16Fn.apply(xm, wm, stride)
    assert ym.dtype == torch.bfloat16 and ym.shape == (2,) + tuple(y.shape[2:]) + (cout,)
    (ym.float() * R.permute(0, 2, 3, 4, 1).to(dev)).sum().backward()
    relclose(from_cl(ym.detach()), y.detach(), 1e-2, "y")
    relclose(from_cl(xm.grad), xr.grad, 1e-2, "dx")
    relclose(wm.grad, wr.grad, 1e-2, "dw")


@pytest.mark.parametrize("cin,cout,sd,D,H,W", [(64, 32, 2, 2, 3, 6), (32, 16, 1, 3, 4, 20), (16, 8, 1, 2, 5, 33), (16, 8, 2, 3, 2, 40)])
def test_deconv_bf16_fn(dev, cin, cout, sd, D, H, W):
    from mvsformer_amd import autograd as ag
    gen = torch.Generator().manual_seed(cin * 100 + cout + D + sd)
    x = bf(torch.randn(2, cin, D, H, W, generator=gen))
    w = bf(torch.randn(cin, cout, 3, 3, 3, generator=gen) / (7 * cin) ** 0.5)
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv_transpose3d(xr, wr, None, stride=(sd, 2, 2), padding=1, output_padding=(sd - 1, 1, 1))
    R = bf(torch.randn(y.shape, generator=gen))
    (y * R).sum().backward()
    xm = to_cl(x, dev).requires_grad_(True)
    wm = w.to(dev).requires_grad_(True)
    ym = ag.DeconvBf16Fn.apply(xm, wm, sd)
    (ym.float() * R.permute(0, 2, 3, 4, 1).to(dev)).sum().backward()
    relclose(from_cl(ym.detach()), y.detach(), 1e-2, "y")
    relclose(from_cl(xm.grad), xr.grad, 1e-2, "dx")
    relclose(wm.grad, wr.grad, 1e-2, "dw")


@pytest.mark.parametrize("relu,with_res", [(True, True), (True, False), (False, False)])
def test_bn_act_bf16_fn(dev, relu, with_res):
    import torch.nn as nn
    from mvsformer_amd import autograd as ag
    gen = torch.Generator().manual_seed(3)
    x = bf(torch.randn(3, 16, 5, 6, 7, generator=gen) * 2 + 0.5)
    res = bf(torch.randn(x.shape, generator=gen)) if with_res else None
    R = bf(torch.randn(x.shape, generator=gen))
    bn_ref, bn_mine = nn.BatchNorm3d(16), nn.BatchNorm3d(16)
    with torch.no_grad():
        bn_ref.weight.copy_(torch.rand(16, generator=gen) + 0.5)
        bn_ref.bias.copy_(torch.randn(16, generator=gen))
    bn_mine.load_state_dict(bn_ref.state_dict())
    xr = x.clone().requires_grad_(True)
    rr = res.clone().requires_grad_(True) if with_res else None
    y = bn_ref(xr)
    y = F.relu(y) if relu else y
    y = y + rr if with_res else y
    (y * R).sum().backward()
    bn_mine = bn_mine.to(dev)
    xm = to_cl(x, dev).requires_grad_(True)
    rm = to_cl(res, dev).requires_grad_(True) if with_res else None
    ym = ag.BnActBf16Fn.apply(xm, bn_mine.weight, bn_mine.bias, rm, bn_mine, relu)
    (ym.float() * R.permute(0, 2, 3, 4, 1).to(dev)).sum().backward()
    relclose(from_cl(ym.detach()), y.detach(), 1e-2, "y")
    relclose(from_cl(xm.grad), xr.grad, 1.5e-2, "dx")
    relclose(bn_mine.weight.grad, bn_ref.weight.grad, 1e-2, "dgamma")
    relclose(bn_mine.bias.grad, bn_ref.bias.grad, 1e-2, "dbeta")
    relclose(bn_mine.running_mean, bn_ref.running_mean, 1e-4, "running_mean")
    relclose(bn_mine.running_var, bn_ref.running_var, 1e-4, "running_var")
    if with_res:
        relclose(from_cl(rm.grad), rr.grad, 1e-2, "dres")


STAGE_GRAD_L2 = 0.4          # measured, see the docstring; the per-layer guard is test_regularizer_bf16_layer_by_layer_attribution


@pytest.mark.parametrize("kind,C,ndepth,H,W,V", [("costregnet", 32, 16, 32, 48, 3), ("costregnet3d", 8, 8, 40, 56, 4)])
def test_stage_train_bf16_vs_fp32_oracle(dev, kind, C, ndepth, H, W, V):
    """StageNet.train() under ``torch.autocast(bfloat16)``: prob_volume_pre and every gradient against the fp32 CPU oracle."""
    import mvsformer_amd as m
    from mvsformer_amd import synth
    from oracle import ref_torch
    scale = {64: 8, 32: 4, 16: 2, 8: 1}[C]
    torch.manual_seed(C + ndepth)
    net = m.StageNet(dict(base_ch=8, fusion_type="cnn", depth_type="ce"), ndepth, 0).train()
    scene = synth.make_scene(V, H * scale, W * scale, seed=W)
    feat = synth.render_features(scene, scale, C, batch=2)
    proj = synth.proj_matrices(scene, (scale,), 2)["stage1"]
    hyp = ref_torch.init_inverse_range(synth.depth_range(2), ndepth, H, W)
    R = torch.randn(2, ndepth, H, W, generator=torch.Generator().manual_seed(1))
    fr = feat.clone().requires_grad_(True)
    sd = {k: (v.detach().clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.detach().clone())
          for k, v in net.state_dict().items()}
    want = ref_torch.stage_forward(fr, proj, hyp, sd, ndepth=ndepth, tmp=5.0, training=True)
    (want["prob_volume_pre"] * R).sum().backward()
    net = net.to(dev)
    fg = feat.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = net(fg, proj.to(dev), hyp.to(dev), tmp=5.0)
    assert got["prob_volume_pre"].dtype == torch.float32
    (got["prob_volume_pre"] * R.to(dev)).sum().backward()
    relclose(got["prob_volume_pre"].detach(), want["prob_volume_pre"].detach(), 4e-2, "prob_volume_pre")
    err = (fg.grad.cpu().double() - fr.grad.double()).abs()
    gs = fr.grad.abs().max().item()
    assert (err > 1e-1 * gs).double().mean().item() < 2e-3 and err.mean().item() < 1e-2 * gs, (err.max().item() / gs, err.mean().item() / gs)
    # parameter gradients: relative L2 error per regularizer tensor (a gradient is a sum over ~1e5..1e6 voxels whose bf16 rounding
    # errors add up in quadrature: the largest element may move by more than the norm does), and the DIRECTION of the whole visibility-CNN
    # gradient: d loss / d w_v = sum G*(in_prod_v - volume_mean)/S is a difference of nearly equal terms, so the ~1 % bf16 noise of the
    # regularizer's input gradient is amplified ~10x on the way into that CNN (in the reference's autocast too)
    vis_a, vis_b = [], []
    for name, p in net.named_parameters():
        a, b = p.grad.flatten().double().cpu(), sd[name].grad.flatten().double()
        if name.startswith("vis."):
            vis_a.append(a)
            vis_b.append(b)
        else:
            rel = ((a - b).norm() / (b.norm() + 1e-30)).item()
            assert rel < STAGE_GRAD_L2, (name, rel)       # vs FP32: bf16 noise through ~22 rounded tensors and their ReLU gates
    a, b = torch.cat(vis_a), torch.cat(vis_b)
    cos = (a @ b / (a.norm() * b.norm() + 1e-30)).item()
    assert cos > 0.9, ("vis.*", cos)
    # the fp32 mode of the same module still works and is closer
    net.zero_grad(set_to_none=True)
    got32 = net(feat.to(dev), proj.to(dev), hyp.to(dev), tmp=5.0)
    relclose(got32["prob_volume_pre"].detach(), want["prob_volume_pre"].detach(), 1e-3, "fp32 prob_volume_pre")


@pytest.mark.parametrize("kind,D,H,W", [("costregnet", 16, 32, 48), ("costregnet3d", 8, 40, 56)])
def test_regularizer_bf16_vs_cpu_autocast(dev, kind, D, H, W):
    """The regularizer alone, same fp32 cost volume in, against the ORACLE RUN UNDER ``torch.autocast('cpu', bfloat16)`` - i.e. against
    the reference's own autocast semantics (half-precision conv / transposed conv / BatchNorm outputs) instead of against fp32.
    Both sides round every activation to bf16, so only summation order and the occasional ReLU gate on a rounding boundary differ:
    logits within 2e-2 of their scale, gradients within 25 % in L2 (measured 6-14 % from run to run: the fp32 atomics of the BatchNorm
    statistics change the last bit of a mean, which moves bf16 roundings and ReLU gates downstream)."""
    import mvsformer_amd as m
    from oracle import ref_torch
    torch.manual_seed(D + H)
    net = (m.CostRegNet(8, 8) if kind == "costregnet" else m.CostRegNet3D(8, 8)).train()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(2, 8, D, H, W, generator=gen)
    R = torch.randn(2, 1, D, H, W, generator=gen)
    sd = {"cost_reg." + k: (v.detach().clone().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.detach().clone())
          for k, v in net.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        want = (ref_torch.cost_reg_net if kind == "costregnet" else ref_torch.cost_reg_net_3d)(xr, sd, "cost_reg", True)
    (want.float() * R).sum().backward()
    net = net.to(dev)
    xg = x.to(dev).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = net(xg)
    assert got.dtype == torch.float32 and got.shape == want.shape
    (got * R.to(dev)).sum().backward()
    relclose(got.detach(), want.detach().float(), 2e-2, "logits")
    worst = {}
    for name, p in list(net.named_parameters()) + [("input", xg)]:
        a = p.grad.flatten().double().cpu()
        b = (xr.grad if name == "input" else sd["cost_reg." + name].grad).flatten().double()
        worst[name] = ((a - b).norm() / (b.norm() + 1e-30)).item()
    bad = {k: v for k, v in worst.items() if v > 0.25}
    assert not bad, bad


def _rel_l2(got, want):
    got, want = torch.as_tensor(got).double().cpu().flatten(), torch.as_tensor(want).double().cpu().flatten()
    return ((got - want).norm() / (want.norm() + 1e-30)).item()


@pytest.mark.parametrize("kind,D,H,W", [("costregnet", 16, 32, 48), ("costregnet3d", 8, 40, 56), ("costregnet", 32, 16, 24), ("costregnet3d", 8, 24, 40)])
def test_regularizer_bf16_layer_by_layer_attribution(dev, kind, D, H, W):
    """Per-layer attribution of the bf16 regularizer's error: every layer of the U-Net at its real place in the
    network - conv / transposed conv on the bf16 matrix cores, batch-statistics BatchNorm, ReLU, skip - is TEACHER-FORCED: it gets the
    reference chain's own (bf16-rounded) input activation and skip tensor and a bf16 upstream gradient, and its output, data gradient,
    skip gradient, weight gradient and BatchNorm affine gradients are each bounded against fp32 autograd of the same layer on the same
    bf16 operands.  What is left is one layer's own rounding (bf16 conv output, bf16 activation, bf16 gradients: 2^-9 relative per
    element, a few 1e-3 in L2), so a broken layer cannot hide behind the stage-level bounds: 1e-2 on the output, 2e-2 on every gradient.
    Covers the four layer geometries per net (stride 2 / (1,2,2) / 1, transposed) at all channel widths 8..64."""
    import mvsformer_amd as m
    from mvsformer_amd import module as mod
    torch.manual_seed(D * 7 + H)
    net = (m.CostRegNet(8, 8) if kind == "costregnet" else m.CostRegNet3D(8, 8)).train()
    three_d = kind == "costregnet3d"
    s_down = (1, 2, 2) if three_d else (2, 2, 2)
    gen = torch.Generator().manual_seed(11)
    x0 = bf(torch.randn(2, 8, D, H, W, generator=gen))

    def parts(name):
        l = getattr(net, name)
        return (l[0], l[1]) if isinstance(l, torch.nn.Sequential) else (l.conv, l.bn)

    def ref_layer(name, x, skip, transposed):
        conv, bn = parts(name)
        wb = bf(conv.weight.detach().cpu()).requires_grad_(True)
        gam, bet = bn.weight.detach().cpu().clone().requires_grad_(True), bn.bias.detach().cpu().clone().requires_grad_(True)
        xr = x.clone().requires_grad_(True)
        sr = skip.clone().requires_grad_(True) if skip is not None else None
        if transposed:
            y = F.conv_transpose3d(xr, wb, None, stride=s_down, padding=1, output_padding=(0, 1, 1) if three_d else 1)
        else:
            y = F.conv3d(xr, wb, None, stride=conv.stride, padding=1)
        y = y + (bf(y) - y).detach()                              # the kernel stores the convolution as bf16
        z = F.relu(F.batch_norm(y, None, None, gam, bet, True, 0.1, bn.eps))
        z = z + (bf(z) - z).detach()
        out = z + sr if sr is not None else z
        out = out + (bf(out) - out).detach()
        return out, xr, sr, wb, gam, bet

    chain = [("conv1", False, None), ("conv2", False, None), ("conv3", False, None), ("conv4", False, None), ("conv5", False, None),
             ("conv6", False, None), ("conv7", True, "conv4"), ("conv9", True, "conv2"), ("conv11", True, "input")]
    acts = {"input": x0}
    x = x0
    net_dev = net.to(dev)
    worst = {}
    for name, transposed, skip_name in chain:
        skip = acts[skip_name] if skip_name else None
        out, xr, sr, wb, gam, bet = ref_layer(name, x, skip, transposed)
        R = bf(torch.randn(out.shape, generator=gen))
        (out * R).sum().backward()
        # the same layer on the HIP path: bf16 channel-last activations, fp32 master weights (rounded to bf16 by the packer)
        layer = getattr(net_dev, name)
        conv, bn = (layer[0], layer[1]) if isinstance(layer, torch.nn.Sequential) else (layer.conv, layer.bn)
        for prm in (conv.weight, bn.weight, bn.bias):
            prm.grad = None
        xm = to_cl(x, dev).requires_grad_(True)
        sm = to_cl(skip, dev).requires_grad_(True) if skip is not None else None
        ym = mod._train_conv_bn_act(xm, conv, bn, True, sm, transposed_sd=(s_down[0] if transposed else None))
        (ym.float() * R.permute(0, 2, 3, 4, 1).to(dev)).sum().backward()
        errs = {"y": _rel_l2(from_cl(ym.detach()), out.detach()), "dx": _rel_l2(from_cl(xm.grad), xr.grad), "dw": _rel_l2(conv.weight.grad, wb.grad),
                "dgamma": _rel_l2(bn.weight.grad, gam.grad), "dbeta": _rel_l2(bn.bias.grad, bet.grad)}
        if skip is not None:
            errs["dskip"] = _rel_l2(from_cl(sm.grad), sr.grad)
        worst[name] = errs
        assert errs["y"] < 1e-2, (name, errs)
        assert all(v < 2e-2 for k, v in errs.items() if k != "y"), (name, errs)
        acts[name] = out.detach()
        x = out.detach()


def test_bn_act_bf16_grouped_equals_per_group_calls(dev):
    """Grouped BatchNorm over the batch dimension (sample n -> group n % groups) = the same module called once per group on that
    group's samples: outputs, input gradients, parameter gradients (summed over the groups) and running statistics (updated once per
    group, in group order)."""
    from mvsformer_amd import autograd as ag
    torch.manual_seed(5)
    N, G, C = 6, 3, 16
    x = (torch.randn(N, 1, 9, 130, C) * 2 + 0.5).to(torch.bfloat16).to(dev)        # 1170 rows per sample: not a block multiple
    go = torch.randn(N, 1, 9, 130, C).to(torch.bfloat16).to(dev)

    def make_bn():
        bn = torch.nn.BatchNorm3d(C).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, C))
            bn.bias.copy_(torch.linspace(-0.3, 0.3, C))
        return bn
    bn_a, bn_b = make_bn(), make_bn()
    xa = x.clone().requires_grad_(True)
    ya = ag.BnActBf16Fn.apply(xa, bn_a.weight, bn_a.bias, None, bn_a, True, G)
    ya.backward(go)
    xb = x.clone().requires_grad_(True)
    outs = []
    for g in range(G):
        outs.append(ag.BnActBf16Fn.apply(xb[g::G], bn_b.weight, bn_b.bias, None, bn_b, True))
    for g in range(G):
        outs[g].backward(go[g::G])
    for g in range(G):
        relclose(ya[g::G].float(), outs[g].float(), 1e-2, "y group %d" % g)          # bf16 outputs: 2^-8 of scale
        relclose(xa.grad[g::G].float(), xb.grad[g::G].float(), 1e-2, "dx group %d" % g)
    relclose(bn_a.weight.grad, bn_b.weight.grad, 1e-4, "dgamma")
    relclose(bn_a.bias.grad, bn_b.bias.grad, 1e-4, "dbeta")
    relclose(bn_a.running_mean, bn_b.running_mean, 1e-5, "running_mean")
    relclose(bn_a.running_var, bn_b.running_var, 1e-5, "running_var")
    assert int(bn_a.num_batches_tracked) == int(bn_b.num_batches_tracked) == G


def test_vis_train_views_bf16_close_to_fp32(dev):
    """The visibility CNN in training under autocast (bf16 channel-last kernels, grouped BatchNorm) against its fp32 path on the same
    entropy maps: weights within bf16 noise of the sigmoid output, parameter gradients aligned (cosine)."""
    import copy
    import mvsformer_amd as m
    from mvsformer_amd import autograd as ag
    torch.manual_seed(2)
    net = m.StageNet(dict(base_ch=8, fusion_type="cnn", depth_type="ce"), 8, 0).to(dev).train()
    net2 = copy.deepcopy(net)
    ent = (torch.rand(1, 3, 40, 56, device=dev) * 2.0).contiguous()
    R = torch.randn(1, 3, 40, 56, device=dev)
    w32 = ag.vis_train_views(ent, net.vis)
    (w32 * R).sum().backward()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        w16 = ag.vis_train_views(ent, net2.vis)
    assert w16.dtype == torch.float32 and w16.shape == w32.shape
    (w16 * R).sum().backward()
    assert (w16 - w32).abs().max().item() < 3e-2                          # sigmoid outputs in [0,1]
    g32 = torch.cat([p.grad.flatten() for p in net.vis.parameters()])
    g16 = torch.cat([p.grad.flatten() for p in net2.vis.parameters()])
    cos = torch.dot(g32, g16) / (g32.norm() * g16.norm())
    assert cos.item() > 0.98, cos.item()
    for a, b in zip(net.vis.buffers(), net2.vis.buffers()):
        if a.dtype.is_floating_point:
            relclose(b, a, 3e-2, "running stat")


@pytest.mark.parametrize("cin,cout,gather,stride,N,D,H,W,groups", [(16, 16, 0, (1, 1), 1, 3, 9, 70, 1), (8, 16, 0, (1, 1), 4, 1, 12, 130, 2),
                                                                   (32, 64, 0, (1, 2), 2, 2, 8, 36, 1), (64, 32, 1, (1, 2), 1, 2, 5, 33, 1),
                                                                   (16, 8, 1, (2, 2), 2, 2, 3, 20, 2)])
def test_conv_bf16_epilogue_statistics(dev, cin, cout, gather, stride, N, D, H, W, groups):
    """The batch statistics taken in the convolution's epilogue (mvs_bf16_conv3d_stats) = a separate mvs_bf16_bn_stats pass over the
    same output, per (group, channel); the output itself is bit-identical to the plain convolution's."""
    from mvsformer_amd import ops
    torch.manual_seed(cin + cout)
    x = torch.randn(N, D, H, W, cin).to(torch.bfloat16).to(dev)
    w = (torch.randn(cout, cin, 3, 3, 3) * 0.1) if gather == 0 else (torch.randn(cin, cout, 3, 3, 3) * 0.1)
    wp = ops.bf16_pack(w.to(dev), 0 if gather == 0 else 1, cin, cout)
    y0 = ops.bf16_conv3d(x, wp, cin, cout, gather, stride)
    y1, sums = ops.bf16_conv3d_stats(x, wp, cin, cout, gather, stride, groups)
    assert torch.equal(y0, y1)
    ref = ops.bf16_bn_stats(y0, groups)
    relclose(sums, ref, 2e-5, "sums")
    # and against plain torch on the rounded output
    yf = y0.float().reshape(N // groups, groups, -1, cout)
    relclose(sums[:groups * cout].view(groups, cout), yf.sum(dim=(0, 2)), 1e-4, "sum vs torch")
    relclose(sums[groups * cout:].view(groups, cout), (yf * yf).sum(dim=(0, 2)), 1e-4, "sumsq vs torch")


CASCADE_BF16 = {"logits_l2": 3e-2, "logits_max": 4e-2, "depth_agree": 0.95, "loss_fp32": 5e-3, "loss_autocast": 1e-2}      # measured values in the docstring below


def test_cascade_bf16_vs_cpu_autocast_all_stage_geometries(dev):
    """The whole 32/16/8/8 training cascade of BASELINE configs[2] under autocast(bfloat16) on 128x192 x 3 views - all four stage
    geometries (C = 64/32/16/8, CostRegNet at stages 1-2, CostRegNet3D at 3-4) - against the oracle cascade.  Training-mode depth is an
    arg-max over hypotheses, so one flipped arg-max at a coarse stage moves that pixel's hypotheses at every later stage: the stages are
    therefore compared ON THE ORACLE'S HYPOTHESES (each HIP stage is fed the hypotheses the oracle cascade used at that stage), and the
    free-running HIP cascade is compared through its loss.  Two oracles:
      * the fp32 oracle (what the bf16 path approximates): per-stage logits within 3e-2 relative L2 and 4e-2 of scale in max norm (measured
        on MI355X: 0.5e-2 ... 1.3e-2 and 0.8e-2 ... 1.5e-2), arg-max depth equal at >= 95 % of the pixels of every stage (measured 98 %),
        four-stage cross-entropy loss of the free-running cascade within 5e-3 relative (measured 6e-4);
      * the oracle under ``torch.autocast('cpu', bfloat16)`` (the reference trainer's semantics, trainer/mvsformer_trainer.py:104-106):
        bounded through the loss only (1e-2 relative; measured 1.4e-3).  CPU autocast also runs the 4x4 projection products and the
        warping arithmetic in bf16, which the HIP path keeps in fp32, so voxel-wise differences against it (measured: logits 5e-2 ... 3e-1
        relative L2, arg-max agreement 91 % ... 65 % from stage 1 to 4 - it is the autocast oracle that moves away from the fp32 one, by
        5-30x more than the HIP path does) measure that, not the regularizer; they are printed, not asserted.
    """
    import mvsformer_amd as m
    from mvsformer_amd import synth
    from mvsformer_amd.losses import ce_loss_stage4
    from oracle import ref_torch, ref_losses
    torch.manual_seed(3)
    ndepths, tmp = [32, 16, 8, 8], [5.0, 5.0, 5.0, 1.0]
    net = m.CascadeMVS(dict(ndepths=ndepths)).train()
    ratios = list(net.depth_interals_ratio)
    m.randomize_bn_(net, 5)
    feats, proj, dv, scene = synth.make_inputs(3, 128, 192, seed=2)      # stage 1 = 16 x 24: three halvings of the D-strided regularizer
    sds = [{k: v.detach().clone() for k, v in net.fusions[i].state_dict().items()} for i in range(4)]
    with torch.no_grad():
        want32 = ref_torch.cascade_forward(feats, proj, dv, sds, ndepths=ndepths, depth_interals_ratio=ratios, tmp=tmp, training=True)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            want16 = ref_torch.cascade_forward(feats, proj, dv, sds, ndepths=ndepths, depth_interals_ratio=ratios, tmp=tmp, training=True)
    gts = {"stage%d" % (i + 1): synth.plane_depth(scene, s)[None] for i, s in enumerate(synth.STAGE_SCALES)}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}

    def ref_loss(w):
        wf = {k: ({kk: (vv.float() if torch.is_tensor(vv) else vv) for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in w.items()}
        return sum(float(v) for v in ref_losses.ce_loss_stage4(wf, gts, masks, dlossw=[1, 1, 1, 1], inverse_depth=True).values())

    net = net.to(dev)
    fd = {k: v.to(dev) for k, v in feats.items()}
    pd = {k: v.to(dev) for k, v in proj.items()}
    report = {}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for name, want in (("fp32", want32), ("autocast", want16)):
            for i in range(4):
                k = "stage%d" % (i + 1)
                hyp = want[k]["depth_values"].float().to(dev).contiguous()
                got = net.fusions[i](fd[k], pd[k], hyp, tmp=tmp[i])
                w = want[k]["prob_volume_pre"].float()
                g = got["prob_volume_pre"].float().cpu()
                report[name + "/" + k] = (round(_rel_l2(g, w), 4), round((g - w).abs().max().item() / w.abs().max().item(), 4),
                                          round((got["depth"].float().cpu() == want[k]["depth"].float()).float().mean().item(), 4))
        free = net(fd, pd, dv.to(dev), tmp=tmp)
    loss_hip = sum(v.item() for v in ce_loss_stage4(free, {k: v.to(dev) for k, v in gts.items()}, {k: v.to(dev) for k, v in masks.items()},
                                                    dlossw=[1, 1, 1, 1], inverse_depth=True).values())
    l32, l16 = ref_loss(want32), ref_loss(want16)
    report["loss"] = {"hip": round(loss_hip, 4), "fp32": round(l32, 4), "autocast": round(l16, 4)}
    print("cascade bf16 report (rel-L2, max err / scale, arg-max agreement):", report)
    for i in range(4):
        l2, mx, agree = report["fp32/stage%d" % (i + 1)]
        assert l2 < CASCADE_BF16["logits_l2"] and mx < CASCADE_BF16["logits_max"] and agree >= CASCADE_BF16["depth_agree"], report
    assert abs(loss_hip - l32) / l32 < CASCADE_BF16["loss_fp32"] and abs(loss_hip - l16) / l16 < CASCADE_BF16["loss_autocast"], report


def test_wgrad_group_equals_layer_by_layer(dev):
    """ops.bf16_wgrad_group (all jobs of a kernel instance in one grid + one reduce) against ops.bf16_conv3d_wgrad per layer: same kernels,
    another number of partial slabs per job -> equal up to the fp32 summation order.  Jobs cover every kernel instance (channel tiles
    1x1, 1x2, 2x1, 2x2, 1x4, 4x1), both strides, a 2-D (9-tap) job with dropped padding channels, and a job alone (a group of one)."""
    from mvsformer_amd import ops
    g = torch.Generator().manual_seed(3)

    def act(n, d, h, w, c):
        return torch.randn(n, d, h, w, c, generator=g).to(torch.bfloat16).to(dev)

    jobs = []
    for ca, cb, stride, (n, dp, hp, wp), taps, cb_out in [
            (8, 8, (1, 1), (1, 3, 9, 20), 27, None), (16, 32, (1, 1), (2, 2, 8, 24), 27, None), (32, 16, (2, 2), (1, 2, 6, 10), 27, None),
            (32, 32, (1, 1), (1, 2, 6, 18), 27, None), (16, 64, (1, 1), (1, 2, 5, 12), 27, None), (64, 8, (1, 1), (1, 1, 7, 16), 27, None), (64, 32, (1, 2), (1, 2, 5, 12), 27, None),
            (16, 8, (1, 1), (4, 1, 12, 40), 9, 1), (64, 64, (1, 1), (1, 2, 4, 8), 27, None)]:
        A = act(n, dp, hp, wp, ca)
        db, hb, wb = ((dp - 1) * stride[0] + 1, (hp - 1) * stride[1] + 1, (wp - 1) * stride[1] + 1) if stride != (1, 1) else (dp, hp, wp)
        if stride != (1, 1):                                  # Bt lives on the finer grid (even sizes, as the layers have them)
            db, hb, wb = dp * stride[0], hp * stride[1], wp * stride[1]
        Bt = act(n, db, hb, wb, cb)
        jobs.append((A, Bt, stride, taps, cb_out))
    want = [ops.bf16_conv3d_wgrad(A, Bt, st, taps, cbo) for A, Bt, st, taps, cbo in jobs]
    outs = [torch.empty(ops.bf16_wgrad_shape(A, Bt, taps, cbo), device=dev) for A, Bt, st, taps, cbo in jobs]
    ops.bf16_wgrad_group([(A, Bt, o, st, taps, cbo) for (A, Bt, st, taps, cbo), o in zip(jobs, outs)])
    torch.cuda.synchronize()
    for k, (o, w) in enumerate(zip(outs, want)):
        assert o.shape == w.shape
        relclose(o, w, 2e-5, "job %d" % k)
    one = torch.empty_like(outs[0])
    ops.bf16_wgrad_group([jobs[0][:2] + (one,) + jobs[0][2:]])
    assert torch.equal(one, want[0])                          # a group of one IS the layer-by-layer call


@pytest.mark.parametrize("C,ndepth,H,W,V", [(32, 16, 32, 48, 3), (8, 8, 40, 56, 4)])
def test_skiplink_and_grouped_wgrad_do_not_change_gradients(dev, C, ndepth, H, W, V, monkeypatch):
    """A StageNet training step (both regularizer kinds) with the round's two autograd-level fusions - a skip tensor's two gradients meeting
    in the strided layer's data-gradient epilogue (autograd.SkipLink) and the weight gradients deferred to grouped launches
    (WgradFlushFn) - against the same step with both switched off (autograd adds the skip gradients, every layer runs its own weight
    gradient).  Same kernels; what differs is one bf16 rounding per skip sum (the fused form rounds the sum once, autograd's add rounds
    both terms' sum of rounded values) and the fp32 summation order of the slabs: per-tensor relative L2 error at the bf16 rounding level."""
    import mvsformer_amd as m
    from mvsformer_amd import synth
    from oracle import ref_torch
    scale = {64: 8, 32: 4, 16: 2, 8: 1}[C]
    torch.manual_seed(C + ndepth)
    net = m.StageNet(dict(base_ch=8, fusion_type="cnn", depth_type="ce"), ndepth, 0).to(dev).train()
    scene = synth.make_scene(V, H * scale, W * scale, seed=W)
    feat = synth.render_features(scene, scale, C, batch=2).to(dev)
    proj = synth.proj_matrices(scene, (scale,), 2)["stage1"].to(dev)
    hyp = ref_torch.init_inverse_range(synth.depth_range(2), ndepth, H, W).to(dev)
    R = torch.randn(2, ndepth, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    state = {k: v.clone() for k, v in net.state_dict().items()}
    grads = []
    for skip, group in (("1", "1"), ("0", "0")):
        monkeypatch.setenv("MVS_TRAIN_SKIPLINK", skip)
        monkeypatch.setenv("MVS_TRAIN_WGRAD_GROUP", group)
        net.load_state_dict(state)                            # the running statistics moved in the first pass
        net.zero_grad(set_to_none=True)
        fg = feat.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            got = net(fg, proj, hyp, tmp=5.0)
        (got["prob_volume_pre"] * R).sum().backward()
        assert all(getattr(mod, "_mvs_wroute", None) is None for mod in net.modules())      # routed weights do not outlive the forward
        grads.append(({n: p.grad.double().clone() for n, p in net.named_parameters()}, fg.grad.double().clone(), got["prob_volume_pre"].detach().clone()))
    (ga, xa, pa), (gb, xb, pb) = grads
    assert torch.equal(pa, pb)                                # the forward is the same launches
    # bf16 has 8 significand bits (2^-9 = 2e-3 per rounding); a few differently rounded skip sums upstream of a tensor: 2e-2 of its norm
    assert ((xa - xb).norm() / xb.norm()).item() < 2e-2
    va, vb = [], []
    for n in ga:
        assert ga[n].shape == gb[n].shape
        if n.startswith("vis."):                              # d loss / d w_v is a difference of nearly equal terms: the regularizer's input-gradient
            va.append(ga[n].flatten())                        # noise arrives amplified ~10x (see test_stage_train_bf16_vs_fp32_oracle): direction
            vb.append(gb[n].flatten())
            continue
        rel = ((ga[n] - gb[n]).norm() / (gb[n].norm() + 1e-30)).item()
        assert rel < 2e-2, (n, rel)
    a, b = torch.cat(va), torch.cat(vb)
    assert (a @ b / (a.norm() * b.norm() + 1e-30)).item() > 0.995


def _var_tol(mean, var, rows=1):
    """Bound on the relative error of a batch variance formed as sum x^2 / n - mean^2: a relative error e in either sum shows as
    e * (1 + (mean/std)^2) in the difference.  The bf16 kernels' partial rows are fp32 values of one block's share (the statistics
    kernel rounds a double sum once; the convolution epilogue adds up to 256 voxels in fp32: 4 x 2^-24 allowed per row), everything
    after them is double, so the independent errors of ``rows`` partial rows average to 1 / sqrt(rows) of that; the result is rounded to
    fp32 once (2^-24, not amplified).  (The statistics kernel first kept fp32 chains inside a block and missed this bound at mean/std 4
    with 2.9e-7 against 2.4e-7: chains over like-sized terms round with a common bias that does not average out.  It now accumulates in
    double up to the row.)  Measured on the MI355X at mean/std 16:
    with the rows added in fp32 (before) 1.9e-5 .. 2.8e-5 at 2^18 rows and 2.0e-5 .. 2.5e-5 in the convolution epilogue, which this bound
    refuses; with double 2.3e-7 .. 8.3e-7 and 8e-9 .. 5e-8."""
    r2 = float(mean) ** 2 / max(float(var), 1e-300)
    return 4.0 * 2.0 ** -24 * (1.0 + r2) / rows ** 0.5 + 2.0 ** -24


def _mean_tol(mean, var):
    """The same for the mean, relative to itself: the sum's error is 4 x 2^-24 of |mean| + std (the size of its terms)."""
    return 4.0 * 2.0 ** -24 * (1.0 + float(var) ** 0.5 / max(abs(float(mean)), 1e-300))


BF16_LADDER = [(r, s) for r in (0.0, 4.0, 16.0) for s in (1e-2, 1.0, 1e2)]      # |mean|/std up to 16: bf16 data (8 bits) cannot hold more


@pytest.mark.parametrize("shape", [(2, 16, 5, 6, 7), (1, 16, 8, 128, 256)], ids=["short-210", "long-2^18"])
def test_bn_act_bf16_offset_ladder(dev, shape):
    """Channels whose mean is 0 / 4 / 16 standard deviations from zero at std 1e-2 / 1 / 1e2 through the bf16 BatchNorm kernels
    (mvs_bf16_bn_train_fwd, mvs_bf16_bn_stats + mvs_bn_finalize, mvs_bf16_bn_bwd_reduce / _apply).  Reference: fp64 BatchNorm of the
    bf16-ROUNDED input on the CPU.  momentum = 1: running_var is the batch variance.  Each channel on its own (their scales differ by
    1e4); tolerances are test_bn_act_bf16_fn's on the bf16 tensors (1e-2 / 1.5e-2); the fp32 statistics are held to ``_var_tol`` / ``_mean_tol``,
    which the fp32 sums of the earlier kernels miss at mean/std = 16 (figures in DESIGN.md section 5)."""
    import torch.nn as nn
    from mvsformer_amd import autograd as ag, ops
    C = shape[1]
    chans = BF16_LADDER + [(0.0, 1.0)] * (C - len(BF16_LADDER))
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(*shape, generator=gen)
    for c, (r, s) in enumerate(chans):
        x[:, c] = (x[:, c] + r) * s
    x = bf(x)
    R = bf(torch.randn(x.shape, generator=gen))
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    xr = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y = F.batch_norm(xr, rm, rv, g64, b64, True, 1.0, 1e-5)
    (y * R.double()).sum().backward()
    bn = nn.BatchNorm3d(C, momentum=1.0)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    bn = bn.to(dev)
    xm = to_cl(x, dev).requires_grad_(True)
    ym = ag.BnActBf16Fn.apply(xm, bn.weight, bn.bias, None, bn, False)
    (ym.float() * R.permute(0, 2, 3, 4, 1).to(dev)).sum().backward()
    ymc, dxc = from_cl(ym.detach()), from_cl(xm.grad)
    # the unfused chain (what SyncBatchNorm and the convolution-epilogue statistics feed): same statistics from mvs_bf16_bn_stats + mvs_bn_finalize
    sums = ops.bf16_bn_stats(xm.detach())
    rm2, rv2 = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    ops.bn_finalize(sums, bn.weight.detach(), bn.bias.detach(), rm2, rv2, 1.0, 1e-5, float(x.numel() // C))
    bad = []
    for c, (r, s) in enumerate(chans[:len(BF16_LADDER)]):
        # partial rows: 512 blocks of 512 rows at 2^18 rows (bn_shape in csrc/bf16_train.hip); the short tensor is counted as one
        vtol, mtol = _var_tol(rm[c], rv[c], 512 if x.numel() // C >= 2 ** 18 else 1), _mean_tol(rm[c], rv[c])
        for what, got, want, tol in (("running_var", bn.running_var[c], rv[c], vtol), ("running_mean", bn.running_mean[c], rm[c], mtol),
                                     ("running_var (stats + finalize)", rv2[c], rv[c], vtol), ("running_mean (stats + finalize)", rm2[c], rm[c], mtol),
                                     ("y", ymc[:, c], y.detach()[:, c], 1e-2), ("dx", dxc[:, c], xr.grad[:, c], 1.5e-2)):
            got64, want64 = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
            err = (got64 - want64).abs().max().item() / max(want64.abs().max().item(), 1e-12)
            print("bf16 ladder %s mean/std=%g std=%g %s: err %.3e (tol %.1e)" % (shape, r, s, what, err, tol))
            if not err < tol:
                bad.append((r, s, what, err, tol))
    assert not bad, bad
    relclose(bn.weight.grad, g64.grad, 1e-2, "dgamma")
    relclose(bn.bias.grad, b64.grad, 1e-2, "dbeta")


@pytest.mark.parametrize("groups", [1, 2])
def test_conv_bf16_epilogue_statistics_offset_ladder(dev, groups):
    """The statistics taken in the convolution's epilogue at an offset: a convolution whose output channels have mean/std of about 0.6, 5
    and 16 at scales 1e-2 / 1 / 1e2 (input 1 + randn/8, centre-tap weights of 4, 5 or 7 positive and the rest negative input channels plus
    small random taps), through ``ops.bf16_conv3d_stats`` + ``bn_finalize(_grouped)`` (the fp32 block rows added in double by
    ``launch_partials_reduce_grouped``) and through ``ops.bf16_conv3d_bn_fwd`` (``bf16_bn_rows_finalize_kernel``; what ``LayerBf16Fn`` runs).
    Reference: fp64 BatchNorm of the bf16-ROUNDED convolution output (the plain ``bf16_conv3d``'s, bit-identical to the fused forms'), per
    group (sample b belongs to group b % groups).  momentum = 1: the running variance is the last group's batch variance; the per-group
    mean / invstd come from the finalize outputs.  Statistics to ``_var_tol`` / ``_mean_tol``, the normalized bf16 output to 1e-2."""
    from mvsformer_amd import ops
    cin, cout, N, D, H, W = 8, 16, 4, 4, 12, 40
    gen = torch.Generator().manual_seed(5)
    x = (1.0 + 0.125 * torch.randn(N, D, H, W, cin, generator=gen)).to(torch.bfloat16)
    npos = [4, 5, 7] * 3 + [4] * 7
    scale = [1e-2] * 3 + [1.0] * 3 + [1e2] * 3 + [1.0] * 7
    w = torch.randn(cout, cin, 3, 3, 3, generator=gen) * 0.01
    for c in range(cout):
        sign = torch.tensor([1.0] * npos[c] + [-1.0] * (cin - npos[c]))
        w[c, :, 1, 1, 1] += sign * (0.75 + 0.5 * torch.rand(cin, generator=gen))
        w[c] *= scale[c]
    gamma, beta = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen)
    xm, gm, bm = x.to(dev), gamma.to(dev), beta.to(dev)
    wp = ops.bf16_pack(w.to(dev), 0, cin, cout)
    y0 = ops.bf16_conv3d(xm, wp, cin, cout, 0, (1, 1))
    yf = y0.float().cpu().double()                            # [N, D, H, W, C]
    count = float(yf.numel() // (cout * groups))
    mean = torch.stack([yf[g::groups].reshape(-1, cout).mean(0) for g in range(groups)])                       # [groups, C]
    var = torch.stack([yf[g::groups].reshape(-1, cout).var(0, unbiased=False) for g in range(groups)])
    ratio = (mean.abs() / var.sqrt())[:, :9]
    print("mean/std of the ladder channels:", [round(v, 2) for v in ratio[0].tolist()])
    assert ratio[:, 2::3].min() > 12.0 and ratio[:, 1::3].min() > 3.0      # the ladder is there (a property of the inputs, checked on the reference)
    want_z = torch.empty_like(yf)
    for g in range(groups):
        want_z[g::groups] = (yf[g::groups] - mean[g]) / torch.sqrt(var[g] + 1e-5) * gamma.double() + beta.double()

    def compare(tag, mean_got, invstd_got, rm, rv):
        bad = []
        for g in range(groups):
            for c in range(9):
                # block rows: N*D*H*ceil(W/64) = 192 work items, four to a block -> 48 rows (one per item in the stats form), split over the groups
                vtol, mtol = _var_tol(mean[g, c], var[g, c], 48 // groups), _mean_tol(mean[g, c], var[g, c])
                checks = [("mean", mean_got[g, c], mean[g, c], mtol), ("invstd", invstd_got[g, c], 1.0 / torch.sqrt(var[g, c] + 1e-5), vtol)]
                if g == groups - 1:                          # momentum 1: the running statistics hold the LAST group's update
                    checks += [("running_mean", rm[c], mean[g, c], mtol), ("running_var", rv[c], var[g, c] * count / (count - 1.0), vtol)]
                for what, got, want, tol in checks:
                    err = abs(float(got) - float(want)) / abs(float(want))
                    print("%s group %d mean/std=%.2f scale=%g %s: err %.3e (tol %.1e)" % (tag, g, ratio[g, c], scale[c], what, err, tol))
                    if not err < tol:
                        bad.append((tag, g, c, what, err, tol))
        return bad

    # (a) epilogue statistics + the shared finalize
    y1, sums = ops.bf16_conv3d_stats(xm, wp, cin, cout, 0, (1, 1), groups)
    assert torch.equal(y0, y1)
    rm, rv = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
    if groups > 1:
        _, _, mu, istd = ops.bn_finalize_grouped(sums, gm, bm, rm, rv, 1.0, 1e-5, count, groups)
    else:
        _, _, mu, istd = ops.bn_finalize(sums, gm, bm, rm, rv, 1.0, 1e-5, count)
    bad = compare("conv3d_stats + finalize", mu.double().cpu().view(groups, cout), istd.double().cpu().view(groups, cout), rm.cpu(), rv.cpu())
    # (b) the fused layer forward
    rm2, rv2 = torch.zeros(cout, device=dev), torch.ones(cout, device=dev)
    y2, z, st = ops.bf16_conv3d_bn_fwd(xm, wp, cin, cout, 0, (1, 1), None, False, gm, bm, rm2, rv2, 1.0, 1e-5, groups)
    assert torch.equal(y0, y2)
    bad += compare("conv3d_bn_fwd", st[2].double().cpu().view(groups, cout), st[3].double().cpu().view(groups, cout), rm2.cpu(), rv2.cpu())
    assert not bad, bad
    zf = z.float().cpu().double()
    for c in range(9):
        relclose(zf[..., c], want_z[..., c], 1e-2, "z channel %d" % c)


# rows per block of the bf16 reduce kernels (bn_shape in csrc/bf16_train.hip): a multiple of 256 / (C/8) rows, at least two sweeps, at most 2048,
# sized for ~512 blocks.  C = 8: blocks of 512 rows; C = 64: blocks of 64 rows; 2048 * 513 + 5 rows: the 2048-row cap binds and the last block is
# ragged.  Two rows is the smallest batch torch's BatchNorm reference accepts (N = 1 of the fp32 list has no bf16 twin for that reason).
BF16_ROWS = [(8, 2), (8, 511), (8, 512), (8, 513), (64, 63), (64, 64), (64, 65), (8, 2048 * 513 + 5)]


@pytest.mark.parametrize("C,R", BF16_ROWS)
def test_bn_act_bf16_row_lengths(dev, C, R):
    """``BnActBf16Fn`` (mvs_bf16_bn_train_fwd, mvs_bf16_bn_bwd_reduce, mvs_bf16_bn_bwd_apply) at row counts around one block of the reduce
    kernels and above the point where the rows-per-block cap binds, against fp64 BatchNorm of the bf16-rounded input.  No ReLU: a margin
    around its kink wide enough for bf16 outputs (1e-2 of max|y|) would exclude 3 % of the elements; the gate itself is
    test_bn_act_bf16_fn's.  Tolerances are that test's; the statistics are held to ``_var_tol`` / ``_mean_tol``."""
    import torch.nn as nn
    from mvsformer_amd import autograd as ag
    gen = torch.Generator().manual_seed(C + R % 1000)
    x = bf(torch.randn(1, C, 1, 1, R, generator=gen) * 2 + 0.5)
    Rw = bf(torch.randn(x.shape, generator=gen))
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    xr = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y = F.batch_norm(xr, rm, rv, g64, b64, True, 1.0, 1e-5)
    (y * Rw.double()).sum().backward()
    bn = nn.BatchNorm3d(C, momentum=1.0)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    bn = bn.to(dev)
    xm = to_cl(x, dev).requires_grad_(True)
    ym = ag.BnActBf16Fn.apply(xm, bn.weight, bn.bias, None, bn, False)
    (ym.float() * Rw.permute(0, 2, 3, 4, 1).to(dev)).sum().backward()
    relclose(from_cl(ym.detach()), y.detach(), 1e-2, "y")
    relclose(from_cl(xm.grad), xr.grad, 1.5e-2, "dx")
    relclose(bn.weight.grad, g64.grad, 1e-2, "dgamma")
    relclose(bn.bias.grad, b64.grad, 1e-2, "dbeta")
    for c in range(C):
        mean_c, var_c = x[0, c].double().mean(), x[0, c].double().var(unbiased=False)
        relclose(bn.running_mean[c], rm[c], _mean_tol(mean_c, var_c), "running_mean[%d]" % c)
        relclose(bn.running_var[c], rv[c], _var_tol(mean_c, var_c), "running_var[%d]" % c)
