"""TEST INFRASTRUCTURE — CPU oracle for the training losses: restates reference
models/losses.py:304-350 (ce_loss_stage4, focal=False), :353-408 (mixup_ce_loss_stage4) and :51-85 (reg_loss_stage4) for one stage,
in the order of operations the reference uses.  Pinned by tests/golden/ce_loss.npz and other_losses.npz (values and gradients produced
by the real functions).  Never imported by the product path.

Precision: every loss takes its DISCRETE decisions (the CE bin index and validity, the reg-loss range mask, the Wasserstein nearest-hypothesis
index, the mixup interval index and range mask) from float32 comparisons of the float32 values of ``depth_values`` / ``depth_gt`` / ``mask``,
whatever dtype the arguments have: those comparisons define the reference (ground truths that sit exactly on a float32 bin edge move to the
neighbouring bin when the edges are re-evaluated in float64).  The CONTINUOUS part (log-sum-exp, mix weights, smooth-L1, the Sinkhorn
iterations) runs in the dtype of the differentiable argument, so passing float64 tensors gives a float64 value and, through autograd, a
float64 gradient for exactly the pixels and bins the float32 reference selects.  With float32 arguments nothing changes."""
import torch
import torch.nn.functional as F


def _f32(x):
    """The float32 value the discrete decisions are taken on (exact for inputs that were float32 before a ``.double()``)."""
    return x.detach().to(torch.float32)


def gt_bins(depth_values, depth_gt, mask, inverse_depth=True):
    """losses.py:309-335 -> (gt_index [B,H,W] long, final_mask [B,H,W] bool), index in flipped order when inverse."""
    depth_values, depth_gt, mask = _f32(depth_values), _f32(depth_gt), _f32(mask)
    gt = depth_gt.unsqueeze(1)
    dv = torch.flip(depth_values, dims=[1]) if inverse_depth else depth_values
    half = (dv[:, 1:] - dv[:, :-1]).abs() / 2
    half = torch.cat([half, half[:, -1:]], dim=1)
    lo, hi = dv[:, 0:1] - half[:, 0:1], dv[:, -1:] + half[:, -1:]
    outside = torch.clamp((gt < lo).float() + (gt > hi).float(), 0, 1)
    final = ((1 - outside).squeeze(1) * (mask > 0.5).float()).bool()
    index = ((dv + half) <= gt.expand_as(dv)).float().sum(dim=1, keepdim=True).long()
    return torch.clamp_max(index, dv.shape[1] - 1).squeeze(1), final


def ce_loss_stage(prob_volume_pre, depth_values, depth_gt, mask, inverse_depth=True, weight=1.0):
    index, final = gt_bins(depth_values, depth_gt, mask, inverse_depth)
    logits = torch.flip(prob_volume_pre, dims=[1]) if inverse_depth else prob_volume_pre
    return weight * F.cross_entropy(logits.permute(0, 2, 3, 1)[final, :], index[final], reduction="mean")


def ce_loss_stage4(inputs, depth_gt_ms, mask_ms, dlossw, inverse_depth=True):
    return {k: ce_loss_stage(inputs[k]["prob_volume_pre"].float(), inputs[k]["depth_values"], depth_gt_ms[k], mask_ms[k], inverse_depth,
                             1.0 if dlossw is None else dlossw[int(k[-1]) - 1]) for k in ("stage1", "stage2", "stage3", "stage4")}


def mixup_bins(depth_values, depth_gt, mask, inverse_depth=True):
    """losses.py:358-376 -> (index of the interval's left hypothesis [B,H,W] long in flipped order, float mask [B,H,W]: in range and mask > 0.5)."""
    gt32 = _f32(depth_gt).unsqueeze(1)
    dv32 = torch.flip(_f32(depth_values), dims=[1]) if inverse_depth else _f32(depth_values)
    outside = torch.clamp((gt32 < dv32[:, 0:1]).float() + (gt32 > dv32[:, -1:]).float(), 0, 1)
    final = (1 - outside).squeeze(1) * (_f32(mask) > 0.5).float()
    index = (dv32[:, 1:] <= gt32.expand_as(dv32[:, :-1])).float().sum(dim=1, keepdim=True).long()
    return torch.clamp_max(index, dv32.shape[1] - 2).squeeze(1), final


def mixup_ce_loss_stage(prob_volume_pre, depth_values, depth_gt, mask, inverse_depth=True, weight=1.0):
    """losses.py:358-399 for one stage."""
    dt = prob_volume_pre.dtype
    index, final = mixup_bins(depth_values, depth_gt, mask, inverse_depth)
    final = final.to(dt)
    gt = depth_gt.to(dt).unsqueeze(1)
    dv = torch.flip(depth_values.to(dt), dims=[1]) if inverse_depth else depth_values.to(dt)
    logits = torch.flip(prob_volume_pre, dims=[1]) if inverse_depth else prob_volume_pre
    left = torch.gather(dv[:, :-1], 1, index.unsqueeze(1))
    itv = torch.gather((dv[:, 1:] - dv[:, :-1]).abs(), 1, index.unsqueeze(1))
    wl = torch.clamp((gt - left).abs() / itv, 0, 1).squeeze(1)
    wr = 1 - wl
    ll = F.cross_entropy(logits[:, :-1], index, reduction="none")
    lr = F.cross_entropy(logits[:, 1:], index, reduction="none")
    den = final.sum() + 1e-6
    return weight * ((ll * wl * final).sum() / den + (lr * wr * final).sum() / den)


def mixup_ce_loss_stage4(inputs, depth_gt_ms, mask_ms, dlossw, inverse_depth=True):
    return {k: mixup_ce_loss_stage(inputs[k]["prob_volume_pre"].float(), inputs[k]["depth_values"], depth_gt_ms[k], mask_ms[k], inverse_depth,
                                   1.0 if dlossw is None else dlossw[int(k[-1]) - 1]) for k in ("stage1", "stage2", "stage3", "stage4")}


def reg_select(depth_values, depth_gt, mask, mask_out_range=False, inverse_depth=True):
    """losses.py:58-74 -> the pixels the mean runs over [B,H,W] bool."""
    sel = _f32(mask) > 0.5
    if mask_out_range:
        dv = torch.flip(_f32(depth_values), dims=[1]) if inverse_depth else _f32(depth_values)
        half = (dv[:, 1:] - dv[:, :-1]).abs() / 2
        half = torch.cat([half, half[:, -1:]], dim=1)
        lo, hi = dv[:, 0] - half[:, 0], dv[:, -1] + half[:, -1]
        outside = torch.clamp((_f32(depth_gt) < lo).float() + (_f32(depth_gt) > hi).float(), 0, 1)
        sel = sel & (1 - outside).bool()
    return sel


def reg_loss_stage(depth, depth_values, depth_gt, mask, interval, mask_out_range=False, inverse_depth=True, weight=1.0):
    """losses.py:56-84 for one stage; ``interval [B]``."""
    itv = interval.to(depth.dtype).reshape(-1, 1, 1)
    sel = reg_select(depth_values, depth_gt, mask, mask_out_range, inverse_depth)
    return weight * F.smooth_l1_loss((depth / itv)[sel], (depth_gt.to(depth.dtype) / itv)[sel], reduction="mean")


def reg_loss_stage4(inputs, depth_gt_ms, mask_ms, dlossw, depth_interval, mask_out_range=False, inverse_depth=True):
    return {k: reg_loss_stage(inputs[k]["depth"], inputs[k]["depth_values"], depth_gt_ms[k], mask_ms[k], depth_interval, mask_out_range,
                              inverse_depth, 1.0 if dlossw is None else dlossw[int(k[-1]) - 1]) for k in ("stage1", "stage2", "stage3", "stage4")}


def make_loss_case(seed=0, B=2, sizes=((32, 8, 12), (16, 16, 24), (8, 24, 32), (4, 40, 56)), inverse_depth=True):
    """Four stages of (D,H,W): inverse-depth hypothesis columns around a smooth surface, logits peaked near the truth plus
    noise, ground truth partly outside the hypothesis range, partly masked out, some landing exactly on a bin edge."""
    g = torch.Generator().manual_seed(seed)
    inputs, gts, masks = {}, {}, {}
    for s, (D, H, W) in enumerate(sizes):
        ys, xs = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
        surf = (600 + 120 * xs - 80 * ys + 25 * torch.sin(6 * xs)).expand(B, H, W).clone()
        width = 0.25 / (s + 1)
        inv_c = 1.0 / surf * (1 + 0.02 * torch.randn(B, H, W, generator=g))
        steps = torch.linspace(-1, 1, D).view(1, D, 1, 1)
        inv = inv_c.unsqueeze(1) * (1 + width * steps)                     # ascending inverse depth = descending depth
        dv = 1.0 / inv if inverse_depth else torch.flip(1.0 / inv, dims=[1])
        gt = surf * (1 + 0.5 * width * torch.randn(B, H, W, generator=g))
        gt[:, : H // 8] *= 1.5                                             # far out of range
        sel = torch.rand(B, H, W, generator=g) < 0.02                      # exactly on a right edge: the <= comparison
        dvf = torch.flip(dv, dims=[1]) if inverse_depth else dv
        edge = dvf[:, D // 2] + (dvf[:, D // 2 + 1] - dvf[:, D // 2]).abs() / 2 if D > 2 else dvf[:, 0]
        gt = torch.where(sel, edge, gt)
        mask = (torch.rand(B, H, W, generator=g) > 0.2).float() * torch.rand(B, H, W, generator=g).clamp_min(0.51)
        mask[:, :, : W // 10] = 0.3                                        # below the 0.5 threshold
        logits = -((dv - gt.unsqueeze(1)).abs() / (surf.unsqueeze(1) * width / D * 2)) + 0.7 * torch.randn(B, D, H, W, generator=g)
        key = "stage%d" % (s + 1)
        inputs[key] = dict(depth_values=dv.contiguous(), prob_volume_pre=logits.contiguous())
        gts[key], masks[key] = gt.contiguous(), mask.contiguous()
    return inputs, gts, masks


def nearest_hypothesis(depth_values, depth_gt):
    """losses.py:136-138: index of the hypothesis nearest to the ground truth [B,H,W] long, the first one on a tie (torch.min)."""
    return (_f32(depth_values) - _f32(depth_gt)[:, None]).abs().min(1)[1]


def sinkhorn_stage(prob, depth_values, depth_gt, mask, iters=10, eps=1.0, weight=1.0):
    """models/losses.py:88-128 with ``continuous=False``: the log-domain Sinkhorn plan between each pixel's probability column and the one-hot of
    the hypothesis nearest to the ground truth, cost |i - j| / eps (the reference's signs: + cost in the exponent), loss = mean over
    ``mask > 0.5`` of sum_ij T_ij |i - j|.  Plain torch (autograd gives the gradient through all iterations)."""
    B, D, H, W = prob.shape
    ar = torch.arange(D, dtype=prob.dtype)
    Dm = (ar[:, None] - ar[None, :]).abs()                                   # [D (i: prediction), D (j: ground truth)]
    gi = nearest_hypothesis(depth_values, depth_gt).reshape(B * H * W)
    mu = torch.zeros(B * H * W, D, dtype=prob.dtype)
    mu[torch.arange(B * H * W), gi] = 1.0
    nu = prob.permute(0, 2, 3, 1).reshape(B * H * W, D)
    log_mu, log_nu = (mu + 1e-12).log(), (nu + 1e-12).log()
    u, v = torch.zeros_like(log_nu), torch.zeros_like(log_mu)
    for _ in range(iters):
        v = log_mu - torch.logsumexp(Dm[None] / eps + u[:, :, None], dim=1)
        u = log_nu - torch.logsumexp(Dm[None] / eps + v[:, None, :], dim=2)
    T = (Dm[None] / eps + u[:, :, None] + v[:, None, :]).exp()
    sel = (_f32(mask) > 0.5).reshape(-1)
    return weight * (T * Dm[None]).reshape(B * H * W, -1)[sel].sum(-1).mean()


def wasserstein_loss(inputs, depth_gt_ms, mask_ms, dlossw, ot_iter=10, ot_eps=1.0):
    return {k: sinkhorn_stage(inputs[k]["prob_volume"], inputs[k]["depth_values"], depth_gt_ms[k], mask_ms[k], ot_iter, ot_eps, dlossw[i])
            for i, k in enumerate(k for k in inputs if "stage" in k)}
