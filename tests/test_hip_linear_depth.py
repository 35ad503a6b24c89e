"""GPU tests of the linear-depth cascade (``inverse_depth=False``) and of the HIP training heads of the regression / ``mixup_ce`` depth types:
the two schedulers against the REAL reference's outputs (tests/golden/linear_depth_sched.npz), ``autograd.RegHeadFn`` / ``MixupHeadFn`` against
the float64 restatement of tests/linear_depth_util.py (pinned on the CPU by tests/test_linear_depth_refs.py), the composed
``DINOMVSNet(inverse_depth=False, depth_type='re')`` against the real model (linear_depth_e2e.npz) directly and through ``SceneInference``, and
one training step of the four-stage cascade against the real ``StageNet``s (linear_depth_train_*.npz), eager and captured."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_err

import linear_depth_util as lu
import multiscale_util as mu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------------------------------- schedulers
def test_init_range_equals_the_reference_bitwise(dev):
    import mvsformer_amd as m
    g = load_golden("linear_depth_sched.npz")
    rng = lu.init_range_inputs().to(dev)
    for D, H, W in lu.INIT_CASES:
        got = m.init_range(rng, D, dev, torch.float32, H, W)
        assert np.array_equal(got.cpu().numpy(), g["init_D%d" % D]), D


@pytest.mark.parametrize("D,H,W", lu.SCHED_CASES)
def test_schedule_range_vs_reference(dev, D, H, W):
    """Same interpolation as ``schedule_inverse_range``: the bound of its golden test (tests/test_hip_parity.py, 2e-6 relative).  Both the
    device-resident ratio form of ``ops.schedule_range`` and the reference-signature wrapper (already multiplied interval)."""
    import mvsformer_amd as m
    from mvsformer_amd import ops
    g = load_golden("linear_depth_sched.npz")
    prev, step = lu.schedule_range_inputs()
    want = g["sched_D%d_%dx%d" % (D, H, W)]
    got = m.schedule_range(prev.to(dev), D, step.to(dev), H, W).cpu()
    e = rel_err(got, want)
    print("schedule_range D=%d %dx%d: %.3e" % (D, H, W, e))
    assert e < 2e-6
    c = lu.clamped(prev, step, D)[1]
    assert 0 < int(c.sum()) < c.numel() and bool(got.min() >= 0.01)          # (fp32 0.01, as the clamp rounds it)
    ratio = 2.0                                              # an exact factor: ratio * (step / ratio) is step bit for bit
    assert torch.equal(ops.schedule_range(prev.to(dev), (step / ratio).to(dev), D, ratio, H, W).cpu(), got)


def test_schedule_range_refusals(dev):
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    prev, step = lu.schedule_range_inputs()
    with pytest.raises(MvsHipError):
        ops.schedule_range(prev.to(dev), step.to(dev), 4, 1.0, 8, 10)       # 3 x 5 is not half of 8 x 10
    with pytest.raises(MvsHipError):
        ops.schedule_range(prev, step, 4, 1.0, 6, 10)                       # CPU tensors
    with pytest.raises(MvsHipError):
        ops.schedule_range(prev.to(dev), step.to(dev), 1, 1.0, 6, 10)       # D = 1
    with pytest.raises(MvsHipError):
        ops.init_range(lu.init_range_inputs(), 4, 5, 7)                     # CPU tensor


# ------------------------------------------------------------------------------------------------------------------------- training heads
HEAD_TOL = 1e-6           # tests/test_hip_head_edges.py, the ce head against float64: probabilities / confidence absolute, depth relative
UPSTREAM = ["depth", "prob", "both"]


def _head_case(D, H, W, dev):
    pre, hyp, r_depth, r_prob = lu.head_inputs(D, H, W, seed=lu.HEAD_SEED + D)
    return pre, hyp, r_depth, r_prob


def _want(head, pre, hyp, r_depth, r_prob, upstream):
    p64 = pre.double().requires_grad_(True)
    out = (lu.reg_head if head == "reg" else lu.mixup_head)(p64, hyp.double())
    loss = (out[1] * r_depth.double()).sum() * (upstream != "prob") + (out[0] * r_prob.double()).sum() * (upstream != "depth")
    (dpre,) = torch.autograd.grad(loss, p64)
    return [o.detach() for o in out], dpre


@pytest.mark.parametrize("upstream", UPSTREAM)
@pytest.mark.parametrize("H,W", lu.HEAD_SHAPES)
@pytest.mark.parametrize("D", lu.HEAD_DEPTHS)
@pytest.mark.parametrize("head", ["reg", "mixup"])
def test_training_heads_vs_float64(dev, head, D, H, W, upstream):
    """Forward (prob, depth, conf) and ``dpre`` against float64 autograd of the restatement.  ``dpre`` is held to HEAD_TOL of the gradient's
    own scale (max |dpre| of the case), the form the absolute 1e-6 on probabilities of scale 1 takes for a quantity of another scale.  Mixup:
    depth / dpre only where float64 decides the winning pair (linear_depth_util.mixup_decided; at most 1 % left out, checked on the CPU)."""
    from mvsformer_amd import autograd as ag
    pre, hyp, r_depth, r_prob = _head_case(D, H, W, dev)
    (wprob, wdepth, wconf, *_), wdpre = _want(head, pre, hyp, r_depth, r_prob, upstream)
    x = pre.to(dev).requires_grad_(True)
    prob, depth, conf = ag.RegHeadFn.apply(x, hyp.to(dev), 0) if head == "reg" else ag.MixupHeadFn.apply(x, hyp.to(dev))
    assert not conf.requires_grad and prob.requires_grad and depth.requires_grad
    loss = 0.0
    if upstream != "prob":
        loss = loss + (depth * r_depth.to(dev)).sum()
    if upstream != "depth":
        loss = loss + (prob * r_prob.to(dev)).sum()
    (dpre,) = torch.autograd.grad(loss, x)
    ok = lu.mixup_decided(pre) if head == "mixup" else torch.ones(pre.shape[0], H, W, dtype=torch.bool)
    assert (~ok).double().mean().item() <= 0.01
    e_prob = (prob.detach().cpu().double() - wprob).abs().max().item()
    e_conf = (conf.cpu().double() - wconf).abs()[ok].max().item()
    e_depth = ((depth.detach().cpu().double() - wdepth).abs() / wdepth.abs())[ok].max().item()
    okd = ok.unsqueeze(1).expand_as(wdpre)
    e_dpre = (dpre.cpu().double() - wdpre).abs()[okd].max().item() / wdpre.abs()[okd].max().item()
    print("%s D=%d %dx%d %s: prob %.2e conf %.2e depth %.2e dpre %.2e" % (head, D, H, W, upstream, e_prob, e_conf, e_depth, e_dpre))
    assert e_prob < HEAD_TOL and e_conf < HEAD_TOL and e_depth < HEAD_TOL and e_dpre < HEAD_TOL


def test_reg_head_windowed_confidence_and_refusals(dev):
    """The windowed confidence is ``conf_regression`` on the head's own probabilities (a value, not part of the gradient checks); D = 1 and CPU
    tensors are refused."""
    from mvsformer_amd import autograd as ag, ops
    from mvsformer_amd._lib import MvsHipError
    pre, hyp, _, _ = _head_case(8, 5, 7, dev)
    prob, depth, conf = ag.RegHeadFn.apply(pre.to(dev), hyp.to(dev), 2)
    assert torch.equal(conf, ops.conf_regression(prob, 2))
    prob0, depth0, conf0 = ag.RegHeadFn.apply(pre.to(dev), hyp.to(dev), 0)
    assert torch.equal(prob0, prob) and torch.equal(depth0, depth) and torch.equal(conf0, prob.max(1)[0])
    one = torch.zeros(1, 1, 4, 4)
    for fn in (lambda a, b: ag.RegHeadFn.apply(a, b, 0), ag.MixupHeadFn.apply):
        with pytest.raises(MvsHipError):
            fn(one.to(dev), one.to(dev))                    # D = 1
        with pytest.raises(MvsHipError):
            fn(pre, hyp)                                    # CPU tensors
    with pytest.raises(MvsHipError):
        ops.reg_head_bwd(one.to(dev), one.to(dev), None, None)
    with pytest.raises(MvsHipError):
        ops.mixup_train_bwd(one.to(dev), one.to(dev), torch.zeros(1, 4, 4, dtype=torch.int32, device=dev), None, None)


# ------------------------------------------------------------------------------------------------------------------------- composition, eval
def _e2e(dev):
    import mvsformer_amd as m
    from oracle.weights import load_model_shapes, make_model_state_dict
    g = load_golden("linear_depth_e2e.npz")
    raw = np.load(os.path.join(GOLDEN, "dinomvsnet_e2e.npz"))
    assert hashlib.sha256(raw["imgs"].tobytes() + raw["depth_range"].tobytes()).hexdigest() == str(g["inputs_sha256"])
    net = m.DINOMVSNet(dict(mu.model_args(multi_scale=False), inverse_depth=False, depth_type="re"))
    net.load_state_dict(make_model_state_dict(load_model_shapes(), int(g["seed"])), strict=True)
    net = net.to(dev).eval()
    imgs = torch.from_numpy(raw["imgs"].astype(np.float32)).to(dev)
    proj = {"stage%d" % i: torch.from_numpy(raw["proj_stage%d" % i]).to(dev) for i in range(1, 5)}
    return g, net, imgs, proj, torch.from_numpy(raw["depth_range"]).to(dev), [float(t) for t in g["tmps"]]


def test_linear_depth_model_images_to_depth_vs_reference_golden(dev):
    """``DINOMVSNet(inverse_depth=False, depth_type='re')`` in eval against the REAL reference model: every stage's depth and ``refined_depth``
    1e-3 relative, confidence 2e-3 (the bounds of tests/test_hip_multiscale.py's e2e test); then the same through ``SceneInference``
    (``CascadeMVS.forward_bank``)."""
    import mvsformer_amd as m
    g, net, imgs, proj, dv, tmp = _e2e(dev)
    out = net(imgs, proj, dv, tmp=tmp)
    torch.cuda.synchronize()
    for i in range(1, 5):
        want = torch.from_numpy(g["s%d_depth" % i])
        hyp = out["stage%d" % i]["depth_values"]
        assert (hyp[:, 1:] >= hyp[:, :-1]).all()            # linear hypotheses ascend
        rel = ((out["stage%d" % i]["depth"].cpu() - want).abs() / want.abs()).max().item()
        print("stage %d depth: %.3e" % (i, rel))
        assert rel < 1e-3, (i, rel)
    want = torch.from_numpy(g["refined_depth"])
    assert ((out["refined_depth"].cpu() - want).abs() / want.abs()).max().item() < 1e-3
    e = (out["photometric_confidence"].cpu() - torch.from_numpy(g["photometric_confidence"])).abs().max().item()
    print("confidence: %.3e" % e)
    assert e < 2e-3
    si = m.SceneInference(net)
    for v in range(imgs.shape[1]):
        si.add_image(v, imgs[0, v], proj["stage4"][0, v], dv[0].contiguous())
    si.set_pairs([(0, [1, 2])], num_views=3)
    got = si.run(tmp=tmp)[0]["depth"].cpu()
    rel = ((got - want[0]).abs() / want[0].abs()).max().item()
    print("SceneInference depth: %.3e" % rel)
    assert rel < 1e-3


# ------------------------------------------------------------------------------------------------------------------------- composition, training
def _train_net(dev, depth_type):
    import mvsformer_amd as m
    net = m.CascadeMVS(dict(lu.TRAIN_ARGS, depth_type=depth_type))
    net.load_state_dict(lu.train_state_dict(), strict=True)
    return net.to(dev).train()


def _losses(depth_type, out, gts, masks, dv):
    from mvsformer_amd import losses
    if depth_type == "mixup_ce":
        return losses.mixup_ce_loss_stage4(out, gts, masks, lu.TRAIN_DLOSSW, inverse_depth=False)
    return losses.reg_loss_stage4(out, gts, masks, lu.TRAIN_DLOSSW, dv[:, 1] - dv[:, 0], inverse_depth=False)


@pytest.mark.parametrize("depth_type,golden", [("re", "linear_depth_train_re.npz"), ("mixup_ce", "linear_depth_train_mixup.npz")])
def test_linear_depth_training_step_vs_reference(dev, depth_type, golden):
    """One fp32 training step of the four-stage cascade against the REAL ``StageNet``s in the reference's loop (mvsformer_model.py:273-306,
    ``inverse_depth=False``) with the bounds of ``test_mvsformer_p_training_step_vs_reference``: (1) the free-running ``forward`` - which picks
    ``init_range`` / ``schedule_range`` itself - at stage 1 (loss 1e-3) and for finite losses; (2) the step TEACHER-FORCED (every stage scheduled
    from the reference's own previous depth, which is the reference's graph exactly: the hypotheses are detached): losses 1e-5, sampled
    parameter gradients 3e-2 (median per stage) / 0.25 (any tensor) relative L2."""
    import mvsformer_amd as m
    g = load_golden(golden)
    net = _train_net(dev, depth_type)
    feats, proj, dv, gts, masks = lu.train_inputs(dev)
    state0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out = net(feats, proj, dv, tmp=2.0)
    ls = _losses(depth_type, out, gts, masks, dv)
    assert abs(float(ls["stage1"].detach()) - float(g["losses"][0])) < 1e-3 * float(g["losses"][0])
    assert all(torch.isfinite(v.detach()).all() for v in ls.values())
    for i in range(1, 5):
        hyp = out["stage%d" % i]["depth_values"]
        assert (hyp[:, 1:] >= hyp[:, :-1]).all()
    del out, ls
    net.load_state_dict(state0, strict=True)
    outs, prev = {}, None
    itv = (dv[:, 1] - dv[:, 0]).contiguous()
    for i in range(4):
        f = feats["stage%d" % (i + 1)]
        H, W = f.shape[-2:]
        if i == 0:
            hyp = m.init_range(dv, net.ndepths[0], dev, torch.float32, H, W)
        else:
            hyp = m.schedule_range(prev, net.ndepths[i], net.depth_interals_ratio[i] * itv, H, W)
        outs["stage%d" % (i + 1)] = o = net.fusions[i](f, proj["stage%d" % (i + 1)], hyp, tmp=2.0)
        prev = torch.from_numpy(g["s%d_depth" % (i + 1)]).to(dev)
        got = o["depth"].detach().cpu()
        bad = ((got - prev.cpu()).abs() > 1e-3 * prev.cpu().abs()).float().mean().item()
        e_pre = (mu.sample(o["prob_volume_pre"]).cpu() - torch.from_numpy(g["s%d_pre" % (i + 1)])).abs().max().item()
        print("stage %d: depth off by > 1e-3 on %.4f of the pixels, prob_volume_pre samples %.2e" % (i + 1, bad, e_pre))
        assert bad < 3e-3, i
    ls = _losses(depth_type, outs, gts, masks, dv)
    sum(ls.values()).backward()
    torch.cuda.synchronize()
    print("stage losses: " + ", ".join("%.6f (reference %.6f)" % (float(ls["stage%d" % i].detach()), float(g["losses"][i - 1])) for i in range(1, 5)))
    for i in range(1, 5):
        assert abs(float(ls["stage%d" % i].detach()) - float(g["losses"][i - 1])) < 1e-5 * float(g["losses"][i - 1]), i
    errs = []
    for k, p in net.named_parameters():
        want = torch.from_numpy(g["grad." + k])
        got = mu.sample(p.grad, lu.GRAD_SAMPLE).cpu()
        if want.abs().max() < 1e-3 * max(1.0, float(g["norm." + k])) and float(g["norm." + k]) < 1e-2:
            assert got.abs().max().item() < 1e-2, k        # conv biases in front of batch-statistics BatchNorm: zero up to rounding noise
            continue
        errs.append((float((got - want).double().norm()) / max(1e-12, float(want.double().norm())), k))
    errs.sort(reverse=True)
    print("relative L2 gradient errors over the samples, five worst: " + ", ".join("%s %.1e" % (k, e) for e, k in errs[:5]))
    assert errs[0][0] < 0.25, errs[0]
    for pre in ("fusions.0", "fusions.1", "fusions.2", "fusions.3"):
        sub = sorted(e for e, k in errs if k.startswith(pre))
        assert sub[len(sub) // 2] < 3e-2, (pre, sub[len(sub) // 2])


def test_captured_linear_regression_step_matches_eager(dev):
    """The 're' step of the golden's cascade captured with ``graphs.CapturedStep`` and replayed against the eager step from the same state, with
    the criterion of tests/test_hip_graph.py (loss 1e-6 relative, state 1e-6 + 1e-4 of each tensor's scale).  No host read enters the
    step: ``schedule_range`` takes the depth interval from the device."""
    from mvsformer_amd.graphs import CapturedStep
    net = _train_net(dev, "re")
    feats, proj, dv, gts, masks = lu.train_inputs(dev)
    opt = torch.optim.SGD(net.parameters(), lr=1e-4)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = sum(_losses("re", net(feats, proj, dv, tmp=2.0), gts, masks, dv).values())
        loss.backward()
        opt.step()
        return loss

    graphed = CapturedStep(step, warmup=3, keep_graph=True)
    print("captured 're' step nodes:", graphed.node_counts())
    state = {k: v.clone() for k, v in net.state_dict().items()}
    loss_g = graphed().clone()
    after_g = {k: v.clone() for k, v in net.state_dict().items()}
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(state[k])
    loss_e = step().clone()
    assert abs(loss_e.item() - loss_g.item()) <= 1e-6 * abs(loss_e.item()), (loss_e.item(), loss_g.item())
    for k, v in net.state_dict().items():
        if v.dtype.is_floating_point:
            assert (v - after_g[k]).abs().max().item() <= 1e-6 + 1e-4 * v.abs().max().item(), k
        else:
            assert torch.equal(v, after_g[k]), k
