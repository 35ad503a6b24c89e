"""Training mode of the DINO ViT-small branch ("fix": false; mvsformer_amd/vit.py ``_ViTTrainFn``, csrc/vit_train.hip, the A-transposed mode of
``mvs_gemm_x3``) on the GPU: each backward piece against fp64 torch autograd on the CPU and run twice for bitwise equality, the whole ViT's
forward and parameter gradients against ``oracle/ref_vit.py`` in fp64, and ``DINOMVSNet`` with ``fix=False`` against the same model with
``fix=True``.  The backward pieces at row, chunk and tile edges, per slice: tests/test_hip_vit_edges.py."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / max(1e-30, want.norm().item())).item()


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


@pytest.mark.parametrize("N", [17, 321, 1729])
@pytest.mark.parametrize("with_da", [False, True])
def test_attention_backward_vs_fp64(dev, N, with_da):
    from mvsformer_amd import vit as V
    B, NH, hd = 2, 6, 64
    C = NH * hd
    g = torch.Generator().manual_seed(N * 2 + int(with_da))
    qkv = _rand(g, B, N, 3 * C)
    qkv[..., :2 * C] *= 0.35                                    # peaked, not saturated, attention
    dout = _rand(g, B, N, C)
    da = _rand(g, B, NH, N, scale=float(N) ** 0.5) if with_da else None
    qkv_d = qkv.to(dev, torch.float32)
    p, out = V.attention_train_fwd(qkv_d, NH)
    dqkv = V.attention_train_bwd(qkv_d, p, dout.to(dev, torch.float32), NH, None if da is None else da.to(dev, torch.float32))
    dqkv2 = V.attention_train_bwd(qkv_d, p, dout.to(dev, torch.float32), NH, None if da is None else da.to(dev, torch.float32))
    torch.cuda.synchronize()
    assert torch.equal(dqkv, dqkv2)
    x = qkv.clone().requires_grad_(True)
    q, k, v = x.reshape(B, N, 3, NH, hd).permute(2, 0, 3, 1, 4)
    att = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1)
    o = (att @ v).transpose(1, 2).reshape(B, N, C)
    loss = (o * dout).sum()
    if da is not None:
        loss = loss + (att[:, :, 0] * da).sum()                # the CLS row's gradient (mvsformer_model.py:223,253)
    loss.backward()
    assert _l2(p, att) < 1e-5 and _l2(out, o) < 1e-5
    for j, name in enumerate("qkv"):
        r = _l2(dqkv[..., j * C:(j + 1) * C], x.grad[..., j * C:(j + 1) * C])
        assert r < 1e-5, (name, r)


def test_attention_backward_full_matrix_gradient(dev):
    """The whole attention matrix's gradient (``forward_with_last_att``'s output) folds into dS row by row."""
    from mvsformer_amd import vit as V
    B, NH, hd, N = 1, 6, 64, 50
    C = NH * hd
    g = torch.Generator().manual_seed(3)
    qkv, dout, da = _rand(g, B, N, 3 * C) * 0.35, _rand(g, B, N, C), _rand(g, B, NH, N, N, scale=5.0)
    qkv_d = qkv.to(dev, torch.float32)
    p, _ = V.attention_train_fwd(qkv_d, NH)
    dqkv = V.attention_train_bwd(qkv_d, p, dout.to(dev, torch.float32), NH, da.to(dev, torch.float32))
    x = qkv.clone().requires_grad_(True)
    q, k, v = x.reshape(B, N, 3, NH, hd).permute(2, 0, 3, 1, 4)
    att = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1)
    ((att @ v).transpose(1, 2).reshape(B, N, C) * dout).sum().add((att * da).sum()).backward()
    assert _l2(dqkv, x.grad) < 1e-5


def test_layernorm_backward_and_colsum(dev):
    from mvsformer_amd import ops
    g = torch.Generator().manual_seed(5)
    R, C = 777, 384
    x, dy, res = _rand(g, R, C) * 2 + 0.3, _rand(g, R, C), _rand(g, R, C)
    gamma, beta = 0.5 + torch.rand(C, generator=g, dtype=torch.float64), _rand(g, C, scale=0.1)
    f = lambda t: t.to(dev, torch.float32).contiguous()
    y, mean, rstd = ops.layernorm_stats(f(x), f(gamma), f(beta), 1e-6)
    assert torch.equal(y, ops.layernorm(f(x), f(gamma), f(beta), 1e-6))
    dx = ops.layernorm_bwd(f(dy), f(x), mean, rstd, f(gamma), res=f(res))
    dgb = ops.colsum(f(dy), f(x), mean, rstd)
    db = ops.colsum(f(dy))
    dx2, dgb2, db2 = ops.layernorm_bwd(f(dy), f(x), mean, rstd, f(gamma), res=f(res)), ops.colsum(f(dy), f(x), mean, rstd), ops.colsum(f(dy))
    assert torch.equal(dx, dx2) and torch.equal(dgb, dgb2) and torch.equal(db, db2)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    (F.layer_norm(xr, (C,), gr, br, 1e-6) * dy).sum().backward()
    assert _l2(dx, xr.grad + res) < 1e-5
    assert _l2(dgb[:C], gr.grad) < 1e-5 and _l2(dgb[C:], br.grad) < 1e-5 and _l2(db, dy.sum(0)) < 1e-6
    # column sums over a long row (the position table's gradient summed over images)
    big = _rand(g, 3, 321 * 384)
    assert _l2(ops.colsum(f(big), cols=321 * 384), big.sum(0)) < 1e-6


def test_gelu_backward(dev):
    from mvsformer_amd import ops
    g = torch.Generator().manual_seed(6)
    x, dy = _rand(g, 100003) * 3, _rand(g, 100003)
    xd, dyd = x.to(dev, torch.float32), dy.to(dev, torch.float32)
    y, dx = ops.gelu(xd), ops.gelu_bwd(dyd, xd)
    assert torch.equal(dx, ops.gelu_bwd(dyd, xd))
    xr = x.clone().requires_grad_(True)
    yr = F.gelu(xr)
    (yr * dy).sum().backward()
    assert _l2(y, yr) < 1e-6 and _l2(dx, xr.grad) < 1e-6
    # the same GELU as the GEMM epilogue's act 1
    A = xd[:64 * 32].reshape(64, 32).contiguous()
    eye = torch.eye(32, device=dev)
    c = torch.empty(64, 32, device=dev)
    ops.gemm_x3(A, eye, c, 64, 32, 32, 32, 32, 32, act=1)
    assert _l2(c, ops.gelu(A)) < 1e-6


@pytest.mark.parametrize("shape", [(1605, 384, 1536), (70, 33, 129), (2 * 321, 1152, 384)])
def test_gemm_x3_a_transposed(dev, shape):
    """``a_mode = 3``: dW = dY^T X with dY ``[K][M]`` read as stored."""
    from mvsformer_amd import ops
    K, M, N = shape
    g = torch.Generator().manual_seed(K)
    dy, x = _rand(g, K, M), _rand(g, K, N)
    out = torch.empty(M, N, device=dev)
    args = (M, N, K, M, N, N)
    ops.gemm_x3(dy.to(dev, torch.float32), x.to(dev, torch.float32), out, *args, b_kn=True, a_mode=3)
    out2 = torch.empty_like(out)
    ops.gemm_x3(dy.to(dev, torch.float32), x.to(dev, torch.float32), out2, *args, b_kn=True, a_mode=3)
    assert torch.equal(out, out2)
    assert _l2(out, dy.t() @ x) < 1e-5


@pytest.mark.parametrize("case", [(14, 14, 16, 20), (14, 14, 8, 10), (14, 14, 40, 40), (256, 320, 128, 160), (7, 9, 23, 5)])
def test_bicubic_adjoint(dev, case):
    from mvsformer_amd import ops
    H, W, Ho, Wo = case
    g = torch.Generator().manual_seed(H * Wo)
    planes = 5
    x, dy = _rand(g, planes, H, W), _rand(g, planes, Ho, Wo)
    if (H, W) == (14, 14) and (Ho, Wo) != (40, 40):
        sf = ((Ho + 0.1) / 14, (Wo + 0.1) / 14)                 # the position table: by scale factor (vision_transformer.py:407-411)
        rh, rw = 1.0 / sf[0], 1.0 / sf[1]
        ref = lambda t: F.interpolate(t[None], scale_factor=sf, mode="bicubic", align_corners=False)[0]
    else:
        rh, rw = H / Ho, W / Wo
        ref = lambda t: F.interpolate(t[None], size=(Ho, Wo), mode="bicubic", align_corners=False)[0]
    xd, dyd = x.to(dev, torch.float32), dy.to(dev, torch.float32)
    dx = ops.bicubic_resize_bwd(dyd, H, W, rh, rw)
    assert torch.equal(dx, ops.bicubic_resize_bwd(dyd, H, W, rh, rw))
    xr = x.clone().requires_grad_(True)
    (ref(xr) * dy).sum().backward()
    assert _l2(dx, xr.grad) < 1e-5
    lhs = (ops.bicubic_resize(xd, Ho, Wo, rh, rw).double().cpu() * dy).sum().item()
    rhs = (x * dx.double().cpu()).sum().item()
    assert abs(lhs - rhs) < 1e-5 * (x.norm() * dy.norm()).item()


def test_vit_training_mode_matches_eval_on_golden(dev):
    """On the golden ViT input (tests/golden/vit_small.npz) the training-mode ``forward_with_cls_att`` gives the eval path's tokens and CLS
    attention row; the plain ``forward`` stays eval-only (the model never calls it: mvsformer_model.py:216-220)."""
    import mvsformer_amd as m
    from mvsformer_amd._lib import MvsHipError
    from oracle.weights import load_vit_shapes, make_vit_state_dict
    g = load_golden("vit_small.npz")
    net = m.vit_small(patch_size=16, qk_scale="default")
    net.load_state_dict(make_vit_state_dict(load_vit_shapes("vit_small"), int(g["seeds"][0])), strict=True)
    net = net.to(dev).eval()
    x = torch.from_numpy(g["vit_imgs"].astype(np.float32)).to(dev)
    with torch.no_grad():
        tok_eval, att_eval = net.forward_with_cls_att(x)
    tok_train, att_train = net.train().forward_with_cls_att(x)
    # two fp32-equivalent paths (eval: pre-split operands, flash attention; training: materialized): 6.5e-6 / 2.3e-5 measured
    assert _l2(tok_train, tok_eval) < 1e-5 and _l2(att_train, att_eval) < 1e-4
    assert _l2(tok_train, torch.from_numpy(g["vit_feat"])) < 1e-4 and _l2(att_train[:, :, 1:], torch.from_numpy(g["att_cls"])) < 1e-4
    with pytest.raises(MvsHipError, match="forward_with_last_att"):
        net(x)


def _vit_pair(dev, seed=11):
    import mvsformer_amd as m
    from oracle.weights import load_vit_shapes, make_vit_state_dict
    sd = make_vit_state_dict(load_vit_shapes("vit_small"), seed)
    net = m.vit_small(patch_size=16, qk_scale="default")
    net.load_state_dict(sd, strict=True)
    return net.to(dev), sd


@pytest.mark.parametrize("shape", [(2, 128, 160), (1, 256, 320)])
def test_vit_training_forward_backward_vs_oracle(dev, shape):
    """The whole ViT in training mode against oracle/ref_vit.py under fp64 autograd: tokens and the CLS attention row, then the gradient of
    every parameter for a fixed random projection of both outputs."""
    from oracle import ref_vit
    B, H, W = shape
    net, sd = _vit_pair(dev)
    net.train()
    g = torch.Generator().manual_seed(H)
    img = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64)
    tok, att = net.forward_with_cls_att(img.to(dev, torch.float32))
    wt, wa = _rand(g, *tok.shape), _rand(g, *att.shape, scale=30.0)
    ((tok * wt.to(dev, torch.float32)).sum() + (att * wa.to(dev, torch.float32)).sum()).backward()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    sdd = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    rt, ra = ref_vit.vit_forward_with_last_att(sdd, img)
    ra = ra[:, :, 0]
    ((rt * wt).sum() + (ra * wa).sum()).backward()
    assert _l2(tok, rt) < 1e-5 and _l2(att, ra) < 1e-5, (_l2(tok, rt), _l2(att, ra))
    worst = max((_l2(grads[k], sdd[k].grad), k) for k in grads)
    assert worst[0] < 1e-4, worst
    assert set(grads) == set(sd)
    # run to run: bitwise equal
    net.zero_grad()
    tok2, att2 = net.forward_with_cls_att(img.to(dev, torch.float32))
    ((tok2 * wt.to(dev, torch.float32)).sum() + (att2 * wa.to(dev, torch.float32)).sum()).backward()
    assert torch.equal(tok, tok2) and torch.equal(att, att2)
    assert all(torch.equal(grads[k], p.grad) for k, p in net.named_parameters())


def test_vit_training_last_att(dev):
    """``forward_with_last_att`` returns the tokens and the whole last-block matrix (its gradient on any row flows back)."""
    from oracle import ref_vit
    net, sd = _vit_pair(dev, seed=12)
    net.train()
    g = torch.Generator().manual_seed(1)
    img = torch.rand(1, 3, 64, 80, generator=g, dtype=torch.float64)
    tok, att = net.forward_with_last_att(img.to(dev, torch.float32))
    wa = _rand(g, *att.shape, scale=10.0)
    (att * wa.to(dev, torch.float32)).sum().backward()
    sdd = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    rt, ra = ref_vit.vit_forward_with_last_att(sdd, img)
    (ra * wa).sum().backward()
    assert _l2(att, ra) < 1e-5
    for k, p in net.named_parameters():
        if sdd[k].grad is None:                                # the last MLP and the final norm do not reach the attention
            assert not p.grad.any(), k
        else:
            assert _l2(p.grad, sdd[k].grad) < 1e-4, k
    assert _l2(tok, rt) < 1e-5


def _dino_args(fix):
    return dict(fix=fix, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
                depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
                vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                              att_fusion=True, nhead=6, vit_path=""))


def _cancelled(grads, k):
    w = k[:-len("bias")] + "weight"
    return k.endswith(".bias") and grads.get(w) is not None and grads[k].norm() < 1e-4 * grads[w].norm()


def test_dinomvsnet_fix_false_extract_features(dev):
    """``fix=False``: the features equal ``fix=True``'s, every ViT parameter gets a finite non-zero gradient and every other gradient matches
    ``fix=True``'s (the free-running cascade is chaotic in the last ulp, so the comparison is on ``extract_features`` under a fixed random
    projection of its four outputs)."""
    import mvsformer_amd as m
    from oracle.weights import load_model_shapes, make_model_state_dict
    sd = make_model_state_dict(load_model_shapes(), 7)
    nets = {}
    for fix in (True, False):
        net = m.DINOMVSNet(_dino_args(fix))
        net.load_state_dict(sd, strict=True)
        nets[fix] = net.to(dev).train()
    g = torch.Generator().manual_seed(2)
    imgs = torch.rand(1, 3, 3, 256, 320, generator=g).to(dev)
    feats, grads = {}, {}
    for fix, net in nets.items():
        f = net.extract_features(imgs)
        gg = torch.Generator().manual_seed(9)
        loss = sum((v * torch.randn(v.shape, generator=gg).to(dev)).sum() for _, v in sorted(f.items()))
        loss.backward()
        feats[fix] = {k: v.detach() for k, v in f.items()}
        grads[fix] = {k: p.grad for k, p in net.named_parameters()}
    for k in feats[True]:                                      # two fp32-equivalent ViT paths (eval pre-split / training): 1.7e-5 measured
        assert _l2(feats[False][k], feats[True][k]) < 5e-5, k
    worst = (0.0, None)
    for k, gr in grads[False].items():
        if k.startswith("vit."):
            assert gr is not None and torch.isfinite(gr).all() and gr.abs().max() > 0, k
            assert grads[True][k] is None
        elif _cancelled(grads[True], k):                       # a bias that a batch-statistics BatchNorm cancels: its gradient is round-off
            assert (gr - grads[True][k]).norm() < 1e-4 * grads[True][k[:-len("bias")] + "weight"].norm(), k
        elif grads[True][k] is not None:
            worst = max(worst, (_l2(gr, grads[True][k]), k))
    print("fix=False vs fix=True: worst non-ViT gradient rel L2 %.3e (%s)" % worst)
    assert worst[0] < 1e-4, worst


def test_dinomvsnet_fix_false_training_step_and_cache(dev):
    """One full ``ce_loss_stage4`` step with ``fix=False`` is finite; after a ``FusedAdamW`` step an eval forward equals that of a fresh model
    that loaded the updated ``state_dict`` (the ViT's packed weight caches were rebuilt)."""
    import mvsformer_amd as m
    from mvsformer_amd import losses, synth
    from mvsformer_amd.optim import FusedAdamW
    from oracle.weights import load_model_shapes, make_model_state_dict
    V, H, W = 3, 256, 320
    net = m.DINOMVSNet(_dino_args(False))
    net.load_state_dict(make_model_state_dict(load_model_shapes(), 7), strict=True)
    net = net.to(dev)
    feats, proj, dv, _ = synth.make_inputs(V, H, W, seed=4)
    g = torch.Generator().manual_seed(3)
    imgs = torch.rand(1, V, 3, H, W, generator=g).to(dev)
    proj = {k: v.to(dev) for k, v in proj.items()}
    dv = dv.to(dev)
    net.eval()
    with torch.no_grad():
        before = net(imgs, proj, dv)["stage4"]["depth"].clone()       # fills the eval caches
    net.train()
    out = net(imgs, proj, dv, tmp=[5.0, 5.0, 5.0, 1.0])
    scene = synth.make_scene(V, H, W, 4)
    gts = {"stage%d" % (i + 1): synth.plane_depth(scene, s).to(torch.float32).unsqueeze(0).to(dev) for i, s in enumerate((8, 4, 2, 1))}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}
    ls = losses.ce_loss_stage4(out, gts, masks, [1.0, 1.0, 1.0, 1.0], inverse_depth=True)
    opt = FusedAdamW(list(net.parameters()), lr=1e-3)
    opt.zero_grad()
    sum(ls.values()).backward()
    assert all(torch.isfinite(v.detach()).all() for v in ls.values())
    for k, p in net.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), k
    assert all(p.grad is not None for k, p in net.named_parameters() if k.startswith("vit."))
    opt.step()
    net.eval()
    with torch.no_grad():
        after = net(imgs, proj, dv)["stage4"]["depth"]
    fresh = m.DINOMVSNet(_dino_args(False))
    fresh.load_state_dict(copy.deepcopy(net.state_dict()), strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        want = fresh(imgs, proj, dv)["stage4"]["depth"]
    assert torch.equal(after, want)
    assert not torch.equal(after, before)


def test_vit_training_step_graph_capture(dev):
    """A ``fix=False`` ViT training step (forward + backward) captured with ``torch.cuda.graph`` and replayed equals the eager step."""
    net, _ = _vit_pair(dev, seed=13)
    net.train()
    g = torch.Generator().manual_seed(4)
    img = torch.rand(2, 3, 128, 160, generator=g).to(dev)
    wt = torch.randn(2, 81, 384, generator=g).to(dev)
    wa = torch.randn(2, 6, 81, generator=g).to(dev)
    params = list(net.parameters())

    def step():
        tok, att = net.forward_with_cls_att(img)
        return torch.autograd.grad((tok * wt).sum() + (att * wa).sum(), params)

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager))
