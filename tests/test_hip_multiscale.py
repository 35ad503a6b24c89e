"""GPU tests of the ``multi_scale`` variant: the fused full-resolution tail of ``FPNDecoderV2`` (csrc/fpn_v2_tail.hip) against fp64 torch,
``VITDecoderStage4`` (both forms) and ``VITDecoderStage4NoAtt`` in eval against an fp64 restatement (tests/multiscale_util.py) and in
train() against the real reference modules (tests/golden/vit_decoder_ms_train.npz), the composed ``DINOMVSNet(multi_scale=True)`` against the
real reference model (dinomvsnet_ms_e2e.npz), one training forward + backward of it, and ``SceneInference`` over it."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden

import multiscale_util as mu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(got, want):
    return (got.double().cpu() - want.double().cpu()).abs().max().item() / max(1e-12, want.double().abs().max().item())


# ----------------------------------------------------------------------------------------------------------------- the fused tail
# fine tile of csrc/fpn_v2_tail.hip: 30 x 14 -> coarse (7, 15) is exactly one tile, (6, 14) / (8, 16) sit one fine pixel pair either side
TAIL_SHAPES = [(1, 1, 1), (1, 8, 8), (2, 9, 13), (3, 2, 17), (1, 17, 8), (1, 7, 15), (1, 6, 14), (1, 8, 16)]
TAIL_TOL = 2e-5                                              # two split-form layers deep: the project's bar for such a pair (test_hip_fpn.py)


def _tail_decoder(seed):
    """An FPNDecoderV2 whose BatchNorm shifts are LARGE (|beta| ~ 3): a halo position written as ReLU(shift) + skip instead of 0 moves the
    border pixels by O(1) of the map's scale."""
    import mvsformer_amd as m
    g = torch.Generator().manual_seed(seed)
    dec = m.FPNDecoderV2([8, 16, 32, 64]).eval()
    with torch.no_grad():
        for mod in dec.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.copy_(0.5 + torch.rand(mod.weight.shape, generator=g))
                mod.bias.copy_(3.0 + torch.randn(mod.bias.shape, generator=g))
                mod.running_mean.copy_(0.3 * torch.randn(mod.bias.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.bias.shape, generator=g))
            elif isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * 0.15)
                mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
    return dec


def _bn64(x, bn):
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return x * s[None, :, None, None] + (bn.bias.double() - bn.running_mean.double() * s)[None, :, None, None]


def _tail_fp64(dec, out3, conv01):
    up = F.conv_transpose2d(out3.double(), dec.upsample3[0].weight.double(), dec.upsample3[0].bias.double(), stride=2, padding=1)
    x = torch.relu(_bn64(up, dec.upsample3[1])) + conv01.double()
    y = _bn64(F.conv2d(x, dec.out4[0].weight.double(), dec.out4[0].bias.double(), padding=1), dec.out4[1])
    return y * torch.sigmoid(y)


def _ring(t):
    m = torch.zeros(t.shape[-2:], dtype=torch.bool)
    m[0], m[-1], m[:, 0], m[:, -1] = True, True, True, True
    return t[..., m]


@pytest.mark.parametrize("N,h,w", TAIL_SHAPES)
def test_fused_tail_vs_fp64(dev, N, h, w):
    """``ops.fpn_v2_tail`` against the fp64 computation on the whole map and on the border ring; the GEMM route of the parent commit on the
    same inputs gives the error the fused kernel may at most double (a rounding-order change, not another algorithm)."""
    from mvsformer_amd import fpn, ops, vit
    dec = _tail_decoder(7)
    g = torch.Generator().manual_seed(100 * N + 10 * h + w)
    out3, conv01 = torch.randn(N, 16, h, w, generator=g), torch.randn(N, 8, 2 * h, 2 * w, generator=g)
    want = _tail_fp64(dec, out3, conv01)                      # [N,8,2h,2w]
    dec = dec.to(dev)
    o3, c01 = out3.to(dev).permute(0, 2, 3, 1).contiguous(), conv01.to(dev).permute(0, 2, 3, 1).contiguous()
    fold_up, fold_out = vit._fold(dec.upsample3[0], dec.upsample3[1]), vit._fold(dec.out4[0], dec.out4[1])
    prep = ops.fpn_v2_tail_prepare(vit._f(dec.upsample3[0].weight), fold_up, vit._f(dec.out4[0].weight), fold_out)
    got = ops.fpn_v2_tail(o3, c01, *prep).permute(0, 3, 1, 2)
    up = vit.VITDecoderStage4Single._up(o3, vit._convT_matrices(dec.upsample3[0].weight), fold_up, fpn.ACT_RELU_GEMM)
    gemm = fpn.FPNDecoderV2._conv3(up.add_(c01), vit._conv3_matrix(dec.out4[0].weight, 8), fold_out).permute(0, 3, 1, 2)
    torch.cuda.synchronize()
    scale = want.abs().max().item()
    e_tail, e_gemm = (got.double().cpu() - want).abs().max().item() / scale, (gemm.double().cpu() - want).abs().max().item() / scale
    e_ring = (_ring(got.double().cpu()) - _ring(want)).abs().max().item() / scale
    print("tail (%d,%d,%d): fused %.3e (border ring %.3e), GEMM route %.3e of the map's scale %.3g" % (N, h, w, e_tail, e_ring, e_gemm, scale))
    assert got.shape == want.shape
    assert e_ring < TAIL_TOL, e_ring
    assert e_tail < TAIL_TOL, e_tail
    assert e_tail <= 2.0 * e_gemm, (e_tail, e_gemm)


@pytest.mark.parametrize("N,h,w", [(2, 9, 13), (1, 1, 1)])
def test_decoder_v2_switch_routes_agree(dev, monkeypatch, N, h, w):
    """``FPNDecoderV2.forward`` under MVS_FPN_V2_TAIL=1 (the fused kernel, default) and =0 (the GEMM route): the same first three maps bit for
    bit, the full-resolution map within the tail's bound - and the default really launches the new kernel."""
    dec = _tail_decoder(9).to(dev)
    g = torch.Generator().manual_seed(5)
    c = [8, 16, 32, 64]
    convs = [torch.randn(N, c[i], h << (3 - i), w << (3 - i), generator=g).to(dev) for i in range(4)]
    vits = [torch.randn(N, c[3 - i], h << i, w << i, generator=g).to(dev) for i in range(3)]
    outs = {}
    for v in ("1", "0"):
        monkeypatch.setenv("MVS_FPN_V2_TAIL", v)             # (part of the cache key: the next forward packs again)
        outs[v] = [o.clone() for o in dec(*convs, *vits)]
        assert ("tail" in dec._cache[1]) == (v == "1")
    torch.cuda.synchronize()
    for a, b in zip(outs["1"][:3], outs["0"][:3]):
        assert torch.equal(a, b)
    assert outs["1"][3].shape == (N, 8, 8 * h, 8 * w) and outs["1"][3].permute(0, 2, 3, 1).is_contiguous()
    assert _rel(outs["1"][3], outs["0"][3]) < TAIL_TOL


def test_tail_refuses_other_channel_counts(dev):
    from mvsformer_amd import _lib
    lib = _lib.load()
    assert lib.mvs_fpn_v2_tail_prepared_bytes(16, 8, 8) == (4 * 4 * 16 * 8 + 9 * 8 * 8) * 4
    assert lib.mvs_fpn_v2_tail_prepared_bytes(32, 16, 16) == -1 and lib.mvs_fpn_v2_tail_prepared_bytes(16, 8, 16) == -1
    x = torch.zeros(64, device=dev)
    p = x.data_ptr()
    assert lib.mvs_fpn_v2_tail(p, p, p, p, p, 1, 32, 16, 16, 1, 1, p, None) < 0 and b"mvs_fpn_v2_tail" in lib.mvs_last_error()


# ------------------------------------------------------------------------------------------------------------ the ViT decoders, eval
def _decoder(kind, seed):
    import mvsformer_amd as m
    from oracle.weights import make_vit_state_dict
    _, cls, args = next(d for d in mu.DECODERS if d[0] == kind)
    dec = getattr(m, cls)(args)
    sd = make_vit_state_dict({k: list(v.shape) for k, v in dec.state_dict().items()}, seed)
    dec.load_state_dict(sd, strict=True)
    return dec, sd


_EVAL_REF = {}


def _eval_case(kind, shape):
    """The fp64 reference of one (module, shape), computed once and shared by the two routes."""
    key = (kind, shape)
    if key not in _EVAL_REF:
        B, C, h, w = shape
        g = torch.Generator().manual_seed(sum(shape))
        x, att = torch.randn(B, C, h, w, generator=g), torch.rand(B, 6, h, w, generator=g) * 0.05
        _, sd = _decoder(kind, 71)
        with torch.no_grad():
            _EVAL_REF[key] = (x, att, mu.decoder_fp64(kind, sd, x, att))
    return _EVAL_REF[key]


@pytest.mark.parametrize("packed", ["1", "0"])
@pytest.mark.parametrize("shape", [(1, 384, 1, 1), (2, 384, 3, 5), (1, 384, 8, 10)])
@pytest.mark.parametrize("kind", [d[0] for d in mu.DECODERS])
def test_vit_decoders_eval_vs_fp64(dev, monkeypatch, kind, shape, packed):
    monkeypatch.setenv("MVS_VIT_PACKED", packed)
    x, att, want = _eval_case(kind, shape)
    dec, _ = _decoder(kind, 71)
    dec = dec.to(dev).eval()
    got = dec(x.to(dev), att.to(dev))
    got = got if isinstance(got, tuple) else (got,)
    torch.cuda.synchronize()
    assert dec._cache[1]["packed"] == (packed == "1")
    assert len(got) == len(want)
    B, _, h, w = shape
    for i, (o, ww) in enumerate(zip(got, want)):
        assert o.shape == ww.shape and o.shape[2:] == (h << (2 + i), w << (2 + i))
        assert o.permute(0, 2, 3, 1).is_contiguous()         # logical NCHW over channel-last memory
        e = _rel(o, ww)
        print("%s %s packed=%s out%d: %.3e" % (kind, shape, packed, i + 1, e))
        assert e < 2e-5, (i, e)


# --------------------------------------------------------------------------------------------------------- the ViT decoders, training
@pytest.mark.parametrize("kind", [d[0] for d in mu.DECODERS])
def test_vit_decoders_training_vs_reference(dev, kind):
    """train() against the REAL reference modules (tools/gen_multiscale_golden.py): outputs 2e-5, loss 1e-4, input and parameter gradients 2e-4,
    running statistics 1e-5 - the bars of test_vit_decoder_training_mode_vs_reference_gradients."""
    g = load_golden("vit_decoder_ms_train.npz")
    wseed, iseed = mu.TRAIN_SEEDS[kind]
    dec, _ = _decoder(kind, wseed)
    assert list(dec.state_dict()) == list(json.loads(str(g[kind + ".keys"])))
    dec = dec.to(dev).train()
    feat, att, gen = mu.train_inputs(iseed)
    feat, att = feat.to(dev).requires_grad_(True), att.to(dev).requires_grad_(True)
    outs = dec(feat, att)
    outs = outs if isinstance(outs, tuple) else (outs,)
    loss = sum((o * torch.randn(o.shape, generator=gen).to(dev)).sum() for o in outs)
    loss.backward()
    torch.cuda.synchronize()
    p = kind + "."
    for i, o in enumerate(outs, start=1):
        assert _rel(mu.sample(o), torch.from_numpy(g[p + "out%d" % i])) < 2e-5, i
        assert abs(float(o.double().norm()) - float(g[p + "out%d.norm" % i])) < 2e-5 * float(g[p + "out%d.norm" % i])
    assert abs(float(loss) - float(g[p + "loss"])) < 1e-4 * abs(float(g[p + "loss"]))
    assert _rel(mu.sample(feat.grad), torch.from_numpy(g[p + "dfeat"])) < 2e-4
    assert abs(float(feat.grad.double().norm()) - float(g[p + "dfeat.norm"])) < 2e-4 * float(g[p + "dfeat.norm"])
    if p + "datt" in g:
        assert _rel(att.grad, torch.from_numpy(g[p + "datt"])) < 2e-4
    worst = 0.0
    for k, prm in dec.named_parameters():
        want = torch.from_numpy(g[p + "grad." + k])
        got = mu.sample(prm.grad).cpu()
        if want.abs().max() < 1e-2:                          # a conv bias in front of a batch-statistics BatchNorm: zero in exact arithmetic
            assert got.abs().max().item() < 1e-2, k
            continue
        e = (got - want).abs().max().item() / max(1e-12, want.abs().max().item())
        worst = max(worst, e)
        assert e < 2e-4, (k, e)
        assert abs(float(prm.grad.double().norm()) - float(g[p + "norm." + k])) < 2e-4 * float(g[p + "norm." + k]) + 1e-7, k
    for k, b in dec.named_buffers():
        if b.dtype.is_floating_point:
            assert (b.cpu() - torch.from_numpy(g[p + "buf." + k])).abs().max() < 1e-5, k
    print("%s: worst parameter-gradient error %.2e" % (kind, worst))


# ------------------------------------------------------------------------------------------------------------------ the composed model
def _e2e_inputs(dev):
    z = load_golden("dinomvsnet_e2e.npz")                    # the multi-scale golden was recorded on the same images and cameras
    raw = np.load(os.path.join(GOLDEN, "dinomvsnet_e2e.npz"))
    digest = hashlib.sha256(raw["imgs"].tobytes() + raw["depth_range"].tobytes()).hexdigest()
    imgs = torch.from_numpy(z["imgs"].astype(np.float32)).to(dev)
    proj = {"stage%d" % i: torch.from_numpy(z["proj_stage%d" % i]).to(dev) for i in range(1, 5)}
    return imgs, proj, torch.from_numpy(z["depth_range"]).to(dev), digest


def test_multi_scale_model_images_to_depth_vs_reference_golden(dev):
    """``DINOMVSNet(multi_scale=True)`` in eval against the REAL reference model: ``features_stage1..4`` 1e-4 (stage 1 whole: the real check;
    the generator picks weights at which the reference's stage depths vary over the image and its own confidence is well conditioned), every stage's depth and
    ``refined_depth`` 1e-3 relative, confidence 2e-3."""
    import mvsformer_amd as m
    from oracle.weights import make_model_state_dict
    g = load_golden("dinomvsnet_ms_e2e.npz")
    shapes = json.load(open(os.path.join(GOLDEN, "dinomvsnet_ms_shapes.json")))
    net = m.DINOMVSNet(mu.model_args(multi_scale=True))
    sd = make_model_state_dict(shapes, int(g["seed"]))
    net.load_state_dict(sd, strict=True)
    assert list(net.state_dict().keys()) == list(sd.keys())
    net = net.to(dev).eval()
    imgs, proj, dv, digest = _e2e_inputs(dev)
    assert digest == str(g["inputs_sha256"])
    feats = net.extract_features(imgs)
    for s in range(1, 5):
        f = feats["stage%d" % s]
        want = torch.from_numpy(g["features_stage%d" % s])
        e = _rel(f if s == 1 else mu.sample(f, 8192), want)
        print("features_stage%d: %.3e" % (s, e))
        assert e < 1e-4, (s, e)
        assert abs(float(f.double().norm()) - float(g["norm_stage%d" % s])) < 1e-4 * float(g["norm_stage%d" % s]), s
    out = net(imgs, proj, dv, tmp=[float(t) for t in g["tmps"]])
    torch.cuda.synchronize()
    for i in range(1, 5):
        want = torch.from_numpy(g["s%d_depth" % i])
        rel = ((out["stage%d" % i]["depth"].cpu() - want).abs() / want.abs()).max().item()
        assert rel < 1e-3, (i, rel)
    want = torch.from_numpy(g["refined_depth"])
    assert ((out["refined_depth"].cpu() - want).abs() / want.abs()).max().item() < 1e-3
    assert (out["photometric_confidence"].cpu() - torch.from_numpy(g["photometric_confidence"])).abs().max() < 2e-3


def test_multi_scale_model_training_forward_backward(dev):
    """One training forward + backward (fix=True, 64 x 64, 3 views, fp32): a finite loss, a finite non-zero gradient for every parameter of the
    decoder, decoder_vit, encoder and fusions (but the convolution biases in front of a batch-statistics BatchNorm: zero up to rounding), and
    decoder_vit's input gradients against the fp64 restatement of the same module fed the gradients its three outputs received."""
    import mvsformer_amd as m
    from mvsformer_amd import losses, synth
    torch.manual_seed(3)
    net = m.DINOMVSNet(mu.model_args(multi_scale=True))
    m.cascade.randomize_bn_(net, seed=4)
    net = net.to(dev).train()
    _, proj, dv, scene = synth.make_inputs(3, 64, 64, seed=5)
    imgs = synth.render_features(scene, 1, 3, noise=0.02).to(dev)
    proj = {k: v.to(dev) for k, v in proj.items()}
    gts = {"stage%d" % (i + 1): synth.plane_depth(scene, s).to(torch.float32).unsqueeze(0).to(dev) for i, s in enumerate((8, 4, 2, 1))}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}
    seen = {}
    real = net.decoder_vit.forward

    def recording(x, att):
        x, att = x.detach().requires_grad_(True), att.detach().requires_grad_(True)
        outs = tuple(o.view_as(o) for o in real(x, att))     # views: their .grad is what the REST of the model sends back, without the part
        for o in outs:                                       # that out1 / out2 also receive from the next decoder of the chain
            o.retain_grad()
        seen.update(x=x, att=att, outs=outs)
        return outs
    net.decoder_vit.forward = recording
    out = net(imgs, proj, dv.to(dev), tmp=[5.0, 5.0, 5.0, 1.0])
    loss = sum(losses.ce_loss_stage4(out, gts, masks, [1.0, 1.0, 1.0, 1.0], inverse_depth=True).values())
    assert torch.isfinite(loss.detach()).all()
    loss.backward()
    torch.cuda.synchronize()
    bn_fed = set()                                           # conv biases whose output goes straight into a batch-statistics BatchNorm
    for pre, mod in net.named_modules():
        if isinstance(mod, torch.nn.Sequential):
            kids = list(mod.named_children())
            for (n0, a), (_, b) in zip(kids, kids[1:]):
                if isinstance(a, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Conv3d, torch.nn.ConvTranspose3d)) and "BatchNorm" in type(b).__name__:
                    bn_fed.add("%s.%s.bias" % (pre, n0))
    checked = 0
    for k, p in net.named_parameters():
        if k.split(".")[0] not in ("decoder", "decoder_vit", "encoder", "fusions"):
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        if k not in bn_fed:
            assert p.grad.abs().max().item() > 0, k
            checked += 1
    assert checked > 150
    sd = {k: v.detach().cpu() for k, v in net.decoder_vit.state_dict().items()}
    x64, a64 = seen["x"].detach().cpu().double().requires_grad_(True), seen["att"].detach().cpu().double().requires_grad_(True)
    ref = mu.decoder_fp64("chain", sd, x64, a64, training=True)
    for o, r in zip(seen["outs"], ref):
        assert _rel(o, r.detach()) < 2e-5
    torch.autograd.backward(ref, [o.grad.detach().cpu().double() for o in seen["outs"]])
    assert _rel(seen["x"].grad, x64.grad) < 2e-4 and _rel(seen["att"].grad, a64.grad) < 2e-4


def test_scene_inference_over_a_multi_scale_model(dev):
    """``SceneInference`` over three views gives the depth of the per-sample ``forward`` within tests/test_hip_scene_inference.py's bar (1e-3)."""
    import mvsformer_amd as m
    from mvsformer_amd import synth
    NV, H, W, TMP = 3, 128, 192, [5.0, 5.0, 5.0, 1.0]
    torch.manual_seed(1)
    net = m.DINOMVSNet(mu.model_args(multi_scale=True)).eval()
    m.cascade.randomize_bn_(net, seed=2)
    net = net.to(dev)
    sc = synth.make_scene(NV, H, W, seed=4)
    imgs = synth.render_features(sc, 1, 3, noise=0.02, device=dev, dtype=torch.float32)[0]
    cams = torch.zeros(NV, 2, 4, 4, dtype=torch.float64)
    cams[:, 0] = sc.E
    cams[:, 1, :3, :3] = sc.K
    cams[:, 1, 3, 3] = 1.0
    dr = synth.depth_range(1, device=dev)
    pairs = [(i, [(i + 1) % NV, (i + 2) % NV]) for i in range(NV)]
    si = m.SceneInference(net)
    for v in range(NV):
        si.add_image(v, imgs[v], cams[v].to(device=dev, dtype=torch.float32), dr[0].contiguous())
    si.set_pairs(pairs, num_views=3)
    got = si.run(tmp=TMP)
    for r, srcs in pairs:
        views = [r] + srcs
        proj = {}
        for k, s in enumerate(synth.STAGE_SCALES):
            pm = cams[views].clone()
            pm[:, 1, :3, :3] = torch.stack([synth.stage_intrinsics(sc.K, s)] * len(views))
            proj["stage%d" % (k + 1)] = pm[None].to(device=dev, dtype=torch.float32)
        want = net(imgs[views][None], proj, dr, tmp=TMP)["refined_depth"][0]
        assert ((got[r]["depth"] - want).abs() / want.abs()).max().item() <= 1e-3, r
