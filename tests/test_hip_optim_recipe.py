"""The reference's training recipe on the HIP optimizer path (mvsformer_amd/optim.py, ``FusedAdamW(device_hyper=True)``): parameter groups,
a learning-rate schedule, global-norm clipping and a GradScaler with every changing input on the device, eager and inside ONE captured
hipGraph.  Tensors of the odd shapes of tests/test_hip_training.py::test_fused_adamw_vs_torch (one value, ragged tails of the 2048-value
blocks, more tensors than one launch holds) spread over six groups, one parameter without a gradient."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1,), (7, 3), (2049,), (64, 64, 27), (5000,)] + [(3 + i, 5) for i in range(90)]
NVALUES = sum(math.prod(s) for s in SHAPES)
GROUPS = [dict(lr=3e-3, weight_decay=0.0), dict(lr=1e-3, weight_decay=0.02), dict(lr=5e-4, weight_decay=0.05), dict(lr=2e-3, weight_decay=0.01),
          dict(lr=1e-3, weight_decay=0.0), dict(lr=7e-4, weight_decay=0.1)]
COMMON = dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.02)
DEV = torch.device("cuda:0")


def warmup_cosine(it, warm=4, total=12):
    """Linear warm-up over ``warm`` steps, then half a cosine down to ``total`` (the shape of the reference's schedule, utils.py:441)."""
    if it < warm:
        return (it + 1) / warm
    return 0.5 * (1.0 + math.cos(math.pi * (it - warm) / max(1, total - warm)))


def make_params(seed=0, dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV, dtype)) for s in SHAPES]
    frozen = torch.nn.Parameter(torch.ones(4, device=DEV, dtype=dtype))          # never gets a gradient
    return ps, frozen


def grouped(ps, frozen, ngroups=len(GROUPS)):
    """Parameter k goes to group k % ngroups (so a launch holds tensors of every group); the frozen one to group 0."""
    out = []
    for gi in range(ngroups):
        spec = dict(GROUPS[gi % len(GROUPS)])
        spec["lr"] *= 1.0 + 0.01 * (gi // len(GROUPS))
        spec["params"] = [p for k, p in enumerate(ps) if k % ngroups == gi] + ([frozen] if gi == 0 else [])
        out.append(spec)
    return out


def make_grads(steps, seed=1, norms=None):
    """``steps`` lists of gradients (CPU, fp32); with ``norms`` the global norm of step i is about norms[i]."""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for it in range(steps):
        mul = 1.0 if norms is None else norms[it] / math.sqrt(NVALUES)
        out.append([torch.randn(s, generator=gen) * mul for s in SHAPES])
    return out


def set_grads(ps, grads, mul=1.0):
    for p, g in zip(ps, grads):
        p.grad = (g.to(p.device, p.dtype) * mul)


def rel_err(x, ref):
    return (x.detach().double() - ref.detach().double()).abs().max().item() / max(1e-12, ref.detach().abs().max().item())


def test_one_group_is_bit_identical_to_the_by_value_kernel():
    """One group, no clipping: ``mvs_adamw_multi`` reads from the device table what ``mvs_adamw_step`` gets as arguments and does the same
    arithmetic in the same order: parameters and both moments are equal bit for bit after four steps (16-byte and 4-byte accesses alike:
    the update is elementwise)."""
    from mvsformer_amd.optim import FusedAdamW
    pa, fa = make_params()
    pb, fb = make_params()
    oa = FusedAdamW(pa + [fa], device_hyper=True, **COMMON)
    ob = FusedAdamW(pb + [fb], **COMMON)
    for grads in make_grads(4):
        set_grads(pa, grads)
        set_grads(pb, grads)
        oa.step()
        ob.step()
    torch.cuda.synchronize()
    for k, (x, y) in enumerate(zip(pa, pb)):
        assert torch.equal(x, y), (k, SHAPES[k])
        assert torch.equal(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"]) and torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"]), k
    assert torch.equal(fa, fb) and fa not in oa.state
    assert float(oa.param_groups[0]["step"]) == 4.0 == float(ob.param_groups[0]["step"])
    assert oa.param_groups[0]["step"].dim() == 0 and oa.param_groups[0]["step"].is_cuda
    # an unaligned view (a gradient bucket, a flat buffer): the 4-byte path gives the same bits
    flat_p, flat_g = torch.zeros(2049 + 1, device=DEV), torch.zeros(2049 + 1, device=DEV)
    q = torch.nn.Parameter(flat_p[1:])
    q.data.fill_(0.5)
    r = torch.nn.Parameter(torch.full((2049,), 0.5, device=DEV))
    oq, orr = FusedAdamW([q], device_hyper=True, **COMMON), FusedAdamW([r], **COMMON)
    g = make_grads(1, seed=5)[0][2].to(DEV)
    flat_g[1:].copy_(g)
    q.grad, r.grad = flat_g[1:], g.clone()
    assert q.data_ptr() % 16 != 0
    oq.step()
    orr.step()
    assert torch.equal(q.detach(), r.detach())


def test_schedule_and_groups_vs_torch():
    """Six groups under a warm-up-cosine ``LambdaLR`` (12 steps, the warm-up ends after 4) against ``torch.optim.AdamW`` under the same
    scheduler on the same data: the project's figure for this comparison, 2e-6 of each tensor's scale (same arithmetic in another order).
    The scheduler writes ``group['lr']``; the eager ``step()`` carries it to the device table."""
    from mvsformer_amd.optim import FusedAdamW
    pa, fa = make_params()
    pb, fb = make_params()
    oa = FusedAdamW(grouped(pa, fa), device_hyper=True, **COMMON)
    ob = torch.optim.AdamW(grouped(pb, fb), **COMMON)
    sa, sb = torch.optim.lr_scheduler.LambdaLR(oa, warmup_cosine), torch.optim.lr_scheduler.LambdaLR(ob, warmup_cosine)
    seen = []
    for grads in make_grads(12):
        set_grads(pa, grads)
        set_grads(pb, grads)
        oa.step()
        ob.step()
        seen.append(oa.hyper_table[:, 0].clone())
        sa.step()
        sb.step()
    torch.cuda.synchronize()
    worst = max(rel_err(x, y) for x, y in zip(pa, pb))
    print("schedule + groups vs torch.optim.AdamW: worst error / scale = %.3e" % worst)
    for k, (x, y) in enumerate(zip(pa, pb)):
        assert rel_err(x, y) < 2e-6, (k, SHAPES[k], rel_err(x, y))
    assert torch.equal(fa, fb)
    for gi, g in enumerate(oa.param_groups):
        assert float(g["step"]) == 12.0, gi
    lr0 = torch.stack(seen)[:, 0].cpu()                       # group 0's rate as the kernel read it, step by step
    want = torch.tensor([GROUPS[0]["lr"] * warmup_cosine(i) for i in range(12)], dtype=torch.float32)
    assert torch.equal(lr0, want), (lr0, want)
    assert lr0[0] < lr0[3] and lr0[11] < lr0[4]
    sd = oa.state_dict()                                      # the interchange with torch.optim.AdamW checkpoints survives the device arrays
    ot = torch.optim.AdamW(grouped(*make_params()), **COMMON)
    ot.load_state_dict(sd)
    assert float(ot.state[ot.param_groups[1]["params"][0]]["step"]) == 12.0
    oc = FusedAdamW(grouped(*make_params()), device_hyper=True, **COMMON)
    oc.load_state_dict(ob.state_dict())
    assert float(oc.param_groups[3]["step"]) == 12.0 and oc.param_groups[3]["step"].data_ptr() == oc._device_state()["steps"].data_ptr() + 12


CLIP_MAX = 1.0
CLIP_NORMS = [10.0, 0.5, 10.0, 0.3, 8.0, 0.9]                 # about 10 x max_grad_norm on some steps, below it on others


def run_clip_ours():
    from mvsformer_amd.optim import FusedAdamW
    ps, fz = make_params()
    opt = FusedAdamW(grouped(ps, fz), device_hyper=True, max_grad_norm=CLIP_MAX, **COMMON)
    norms = []
    for grads in make_grads(len(CLIP_NORMS), norms=CLIP_NORMS):
        set_grads(ps, grads)
        opt.step()
        norms.append(opt.grad_norm.clone())
    torch.cuda.synchronize()
    return ps, opt, torch.stack(norms).cpu()


def run_clip_torch(dtype):
    ps, fz = make_params(dtype=dtype)
    opt = torch.optim.AdamW(grouped(ps, fz), **COMMON)
    norms = []
    for grads in make_grads(len(CLIP_NORMS), norms=CLIP_NORMS):
        set_grads(ps, grads)
        norms.append(torch.nn.utils.clip_grad_norm_(ps, CLIP_MAX).clone())
        opt.step()
    torch.cuda.synchronize()
    return ps, torch.stack(norms).cpu()


def test_clipping_vs_float64():
    """Global-norm clipping folded into the update (``max_grad_norm``) against the same recipe in float64 (``torch.optim.AdamW`` +
    ``torch.nn.utils.clip_grad_norm_`` on double copies).  With e_torch the error of torch's fp32 recipe against that and e_hip ours, both
    as max |diff| / max |p| per tensor: e_hip <= 2 * e_torch + 2.4e-7 (two fp32 ulps of scale as the floor; the factor 2 is the margin for
    another summation order of the norm).  The stored norm: 1e-6 relative of the fp64 norm.  The stand-alone ``clip_grad_norm_`` leaves
    torch's clipped gradients in ``p.grad`` within 2 ulps of scale."""
    from mvsformer_amd.optim import clip_grad_norm_
    p64, n64 = run_clip_torch(torch.float64)
    p32, _ = run_clip_torch(torch.float32)
    ours, opt, norms = run_clip_ours()
    e_torch = [rel_err(a, r) for a, r in zip(p32, p64)]
    e_hip = [rel_err(a, r) for a, r in zip(ours, p64)]
    print("clipping vs float64: max e_torch = %.3e, max e_hip = %.3e" % (max(e_torch), max(e_hip)))
    print("norms fp64 %s ours %s" % (n64.tolist(), norms.tolist()))
    assert n64[0] > 5 * CLIP_MAX and n64[1] < CLIP_MAX
    for k, (eh, et) in enumerate(zip(e_hip, e_torch)):
        assert eh <= 2 * et + 2.4e-7, (k, SHAPES[k], eh, et)
    assert ((norms.double() - n64).abs() / n64).max().item() <= 1e-6, (norms, n64)
    assert int(opt.skipped_steps) == 0 and all(float(g["step"]) == len(CLIP_NORMS) for g in opt.param_groups)
    # stand-alone: a norm 10 x max_norm (scaled in place) and one below it (the coefficient clamps to 1: the bits stay)
    for target in (10.0, 0.5):
        pa, _ = make_params()
        pb, _ = make_params()
        grads = make_grads(1, seed=7, norms=[target])[0]
        set_grads(pa, grads)
        set_grads(pb, grads)
        n_ref = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
        na = clip_grad_norm_(pa, CLIP_MAX)
        nb = torch.nn.utils.clip_grad_norm_(pb, CLIP_MAX)
        assert na.is_cuda and na.dim() == 0
        assert abs(float(na) - n_ref) <= 1e-6 * n_ref, (float(na), float(nb), n_ref)
        for k, (x, y) in enumerate(zip(pa, pb)):
            assert (x.grad - y.grad).abs().max().item() <= 2 * 1.2e-7 * y.grad.abs().max().item(), (target, k)
            if target < CLIP_MAX:
                assert torch.equal(x.grad, grads[k].to(DEV))


def test_clipping_is_deterministic():
    """No atomics, fixed summation order: two runs of the clipped recipe from the same state give the same bits."""
    a, _, na = run_clip_ours()
    b, _, nb = run_clip_ours()
    assert torch.equal(na, nb)
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), k


def test_grad_scaler_protocol_without_host_reads(monkeypatch):
    """``torch.amp.GradScaler.step`` on an optimizer that declares ``_step_supports_amp_scaling``: the scaler sets ``grad_scale`` /
    ``found_inf`` and both are consumed on the device.  Step A has one inf in one gradient: parameters, moments and every step count keep
    their bits and ``update()`` halves the scale.  Step B is clean: equal to ``torch.optim.AdamW(fused=True)`` under a scaler of its own
    (2e-6 of scale).  With and without a preceding ``unscale_``.  Around ``scaler.step(opt)`` ``Tensor.item`` / ``.cpu`` raise on GPU
    tensors: none is called."""
    from mvsformer_amd.optim import FusedAdamW
    orig_item, orig_cpu = torch.Tensor.item, torch.Tensor.cpu

    def guard(orig, what):
        def f(self, *a, **k):
            if self.is_cuda:
                raise AssertionError("Tensor.%s() on a GPU tensor inside scaler.step(optimizer)" % what)
            return orig(self, *a, **k)
        return f

    for unscale_first in (False, True):
        pa, fa = make_params()
        pb, fb = make_params()
        oa = FusedAdamW(grouped(pa, fa), device_hyper=True, **COMMON)
        ob = torch.optim.AdamW(grouped(pb, fb), fused=True, **COMMON)
        sca, scb = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10), torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
        for sc in (sca, scb):
            sc.scale(torch.ones((), device=DEV))              # the scale tensor is made at the first scale(): the gradients here are scaled by hand
        grads = make_grads(3, seed=3)
        kept = None
        for it, tag in enumerate(("first", "A", "B")):
            scale = 1024.0 if it < 2 else 512.0
            set_grads(pa, grads[it], scale)
            set_grads(pb, grads[it], scale)
            if tag == "A":
                pa[3].grad[5, 7, 11] = float("inf")           # data, as an fp16 overflow would leave it
                pb[3].grad[5, 7, 11] = float("inf")
                kept = ([p.detach().clone() for p in pa], [oa.state[p]["exp_avg"].clone() for p in pa], [oa.state[p]["exp_avg_sq"].clone() for p in pa],
                        oa._device_state()["steps"].clone())
            if unscale_first:
                sca.unscale_(oa)
                scb.unscale_(ob)
            with monkeypatch.context() as mp:
                mp.setattr(torch.Tensor, "item", guard(orig_item, "item"))
                mp.setattr(torch.Tensor, "cpu", guard(orig_cpu, "cpu"))
                sca.step(oa)
            assert not hasattr(oa, "grad_scale") and not hasattr(oa, "found_inf")
            scb.step(ob)
            sca.update()
            scb.update()
            torch.cuda.synchronize()
            if tag == "A":
                for k, p in enumerate(pa):
                    assert torch.equal(p.detach(), kept[0][k]) and torch.equal(oa.state[p]["exp_avg"], kept[1][k]) and torch.equal(oa.state[p]["exp_avg_sq"], kept[2][k]), k
                assert torch.equal(oa._device_state()["steps"], kept[3]) and all(float(g["step"]) == 1.0 for g in oa.param_groups)
                assert sca.get_scale() == 512.0 and scb.get_scale() == 512.0
                assert int(oa.skipped_steps) == 1
            else:
                assert sca.get_scale() == scale
        worst = max(rel_err(x, y) for x, y in zip(pa, pb))
        print("GradScaler (unscale_ first: %s): worst error / scale vs torch fused AdamW = %.3e" % (unscale_first, worst))
        for k, (x, y) in enumerate(zip(pa, pb)):
            assert rel_err(x, y) < 2e-6, (unscale_first, k, SHAPES[k], rel_err(x, y))
        assert all(float(g["step"]) == 2.0 for g in oa.param_groups) and int(oa.skipped_steps) == 1
        assert torch.equal(fa, fb)


def optimizer_only_step(ngroups, max_grad_norm=CLIP_MAX):
    """An optimizer whose gradients are static tensors (refilled with ``copy_`` between replays) and the step function to capture."""
    from mvsformer_amd.optim import FusedAdamW
    ps, fz = make_params()
    opt = FusedAdamW(grouped(ps, fz, ngroups), device_hyper=True, max_grad_norm=max_grad_norm, **COMMON)
    for p in ps:
        p.grad = torch.zeros_like(p)

    def fill(grads):
        with torch.no_grad():
            for p, g in zip(ps, grads):
                p.grad.copy_(g.to(DEV))

    def step():
        opt.step()
        return opt.grad_norm

    return ps, opt, fill, step


def test_captured_step_follows_the_schedule():
    """An optimizer-only step captured ONCE; ``before_replay=[opt.sync_hyper]`` carries the scheduler's rate into the device table before
    every replay: 8 replays with ``sched.step()`` between them equal 8 eager steps from the same start bit for bit (same kernels, same
    inputs, no atomics) - and differ from the same 8 replays without the hook (the rate really moved)."""
    from mvsformer_amd.graphs import CapturedStep
    ps, opt, fill, step = optimizer_only_step(len(GROUPS))
    grads = make_grads(8, seed=11, norms=[10.0, 0.5, 10.0, 0.3, 8.0, 0.9, 3.0, 0.7])
    fill(grads[0])
    graphed = CapturedStep(step, warmup=3, before_replay=[opt.sync_hyper])
    torch.cuda.synchronize()
    start = ([p.detach().clone() for p in ps], [opt.state[p]["exp_avg"].clone() for p in ps], [opt.state[p]["exp_avg_sq"].clone() for p in ps],
             opt._device_state()["steps"].clone())
    assert float(start[3][0]) == 3.0                          # the warm-up runs

    def restore():
        with torch.no_grad():
            for k, p in enumerate(ps):
                p.copy_(start[0][k])
                opt.state[p]["exp_avg"].copy_(start[1][k])
                opt.state[p]["exp_avg_sq"].copy_(start[2][k])
            opt._device_state()["steps"].copy_(start[3])

    def run(fn, hook):
        restore()
        sched = torch.optim.lr_scheduler.LambdaLR(opt, warmup_cosine)          # a fresh scheduler: the rate starts at warmup_cosine(0) again
        opt.sync_hyper()
        graphed.before_replay = [opt.sync_hyper] if hook else []
        rates = []
        for g in grads:
            fill(g)
            fn()
            rates.append(opt.hyper_table[0, 0].clone())
            sched.step()
        torch.cuda.synchronize()
        return [p.detach().clone() for p in ps], torch.stack(rates).cpu()

    replayed, r_rates = run(graphed, True)
    eager, e_rates = run(step, True)
    stale, s_rates = run(graphed, False)
    assert torch.equal(r_rates, e_rates) and len(set(r_rates.tolist())) > 4, r_rates
    assert len(set(s_rates.tolist())) == 1, s_rates
    for k, (x, y) in enumerate(zip(replayed, eager)):
        assert torch.equal(x, y), (k, SHAPES[k], rel_err(x, y))
    assert any(not torch.equal(x, y) for x, y in zip(replayed, stale))
    assert float(opt.param_groups[0]["step"]) == 11.0


def test_launches_do_not_scale_with_groups():
    """The kernel nodes of the captured optimizer-only step over the same tensors as ONE group and as 28 groups (the reference's layer-wise
    ViT groups + the rest): equal."""
    from mvsformer_amd.graphs import CapturedStep
    counts = {}
    for ngroups in (1, 28):
        ps, opt, fill, step = optimizer_only_step(ngroups)
        fill(make_grads(1, seed=13)[0])
        assert len(opt.param_groups) == ngroups
        nc = CapturedStep(step, warmup=2, keep_graph=True).node_counts()
        if nc is None:
            pytest.skip("the runtime does not hand the captured graph out: node_counts() is None")
        counts[ngroups] = nc
    print("kernel nodes of the optimizer-only step: %s" % counts)
    assert counts[1]["kernel"] == counts[28]["kernel"], counts
    assert 0 < counts[28]["kernel"] <= 8, counts             # 95 tensors: 2 + 1 launches of the norm, 2 + 1 of the update


def test_whole_recipe_captured_matches_eager():
    """The small cascade step of tests/test_hip_graph.py with the reference recipe's ingredients - two parameter groups, ``LambdaLR``,
    ``max_grad_norm``, ``GradScaler``, bf16 autocast - captured once: one replay against one eager step from the same state with that file's
    bounds (loss 1e-6 relative, state 1e-6 + 1e-4 * max); three more replays with the scheduler stepping keep the loss finite and skip
    nothing."""
    import mvsformer_amd as m
    from mvsformer_amd import synth
    from mvsformer_amd.graphs import CapturedStep
    from mvsformer_amd.losses import ce_loss_stage4
    from mvsformer_amd.optim import FusedAdamW
    dev = DEV
    feats, proj, dv, scene = synth.make_inputs(3, 128, 192, seed=4, device=dev)
    gts = {"stage%d" % (i + 1): synth.plane_depth(scene, s, device=dev)[None] for i, s in enumerate(synth.STAGE_SCALES)}
    masks = {k: torch.ones_like(v) for k, v in gts.items()}
    torch.manual_seed(0)
    net = m.CascadeMVS(dict(ndepths=[8, 8, 4, 4])).to(dev).train()
    vectors = [p for p in net.parameters() if p.ndim == 1]
    others = [p for p in net.parameters() if p.ndim != 1]
    opt = FusedAdamW([dict(params=vectors, weight_decay=0.0, lr=2e-4), dict(params=others)], lr=1e-4, weight_decay=0.01, device_hyper=True, max_grad_norm=5.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: warmup_cosine(it, warm=4, total=12))
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(feats, proj, dv, tmp=[5.0, 5.0, 5.0, 1.0])
        loss = sum(ce_loss_stage4(out, gts, masks, dlossw=[1, 1, 1, 1]).values())
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return loss

    graphed = CapturedStep(step, warmup=3, before_replay=[opt.sync_hyper])
    torch.cuda.synchronize()
    params = list(net.parameters())
    state = {k: v.clone() for k, v in net.state_dict().items()}
    ostate = ([opt.state[p]["exp_avg"].clone() for p in params], [opt.state[p]["exp_avg_sq"].clone() for p in params], opt._device_state()["steps"].clone(),
              scaler._scale.clone(), scaler._growth_tracker.clone())

    def restore():
        with torch.no_grad():
            for k, v in net.state_dict().items():
                v.copy_(state[k])
            for k, p in enumerate(params):
                opt.state[p]["exp_avg"].copy_(ostate[0][k])
                opt.state[p]["exp_avg_sq"].copy_(ostate[1][k])
            opt._device_state()["steps"].copy_(ostate[2])
            scaler._scale.copy_(ostate[3])
            scaler._growth_tracker.copy_(ostate[4])

    loss_g = graphed().clone()
    after_g = {k: v.clone() for k, v in net.state_dict().items()}
    steps_g = opt._device_state()["steps"].clone()
    restore()
    loss_e = step().clone()
    torch.cuda.synchronize()
    print("whole recipe: loss replay %.6f eager %.6f, grad norm %.4f, skipped %d" % (loss_g.item(), loss_e.item(), float(opt.grad_norm), int(opt.skipped_steps)))
    assert abs(loss_e.item() - loss_g.item()) <= 1e-6 * abs(loss_e.item()), (loss_e.item(), loss_g.item())
    moved = 0
    for k, v in net.state_dict().items():
        if v.dtype.is_floating_point:
            assert (v - after_g[k]).abs().max().item() <= 1e-6 + 1e-4 * v.abs().max().item(), k
            moved += int(not torch.equal(v, state[k]))
        else:
            assert torch.equal(v, after_g[k]), k
    assert moved > 100 and torch.equal(steps_g, opt._device_state()["steps"]) and float(steps_g[0]) == 4.0
    rates = [float(opt.hyper_table[1, 0])]
    for _ in range(3):
        sched.step()
        loss = graphed()
        assert math.isfinite(loss.item()), loss
        rates.append(float(opt.hyper_table[1, 0]))
    assert int(opt.skipped_steps) == 0 and float(opt.param_groups[1]["step"]) == 7.0
    assert rates[0] < rates[1] < rates[2] < rates[3], rates    # the warm-up reached the captured step
