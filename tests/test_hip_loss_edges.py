"""The four training losses of ``csrc/loss.hip`` (``mvs_ce_loss_fwd``, ``mvs_mixup_ce_loss_fwd``, ``mvs_reg_loss_fwd``, ``mvs_was_loss_fwd`` and
``mvs_ce_loss_bwd_scale``) against ``oracle/ref_losses.py`` evaluated in float64 - the discrete decisions (bin, validity, range mask, nearest
hypothesis, mixup interval) taken from the reference's float32 comparisons - at the shapes the goldens never reach: B = 1 / 3, depth counts
that are no power of two, pixel counts that are no multiple of the 256-pixel block (of the 4-pixel block of the Wasserstein kernel), blocks
and batch entries without a single valid pixel, every ``ot_iter`` / ``ot_eps`` pair, peaked inputs and the refusals.

A case is a tuple ``(kind, D, H, W, B, inverse, variant, extra)``; ``build_case`` makes its float32 inputs on the CPU (seeded), ``ref_eval`` the
float64 (or float32) reference value and gradient of ``gout * loss``, ``hip_eval`` the same through ``ops.*`` + ``ops.ce_loss_bwd_scale``.

Tolerances: what the golden tests hold these kernels to - CE 2e-6 max(1, |loss|) and 2e-6 max|grad|; mixup and reg 3e-6 (of max(1, |loss|), of
max|grad|); Wasserstein 1e-5 and 1e-4 max|grad| - or, where the float32 arithmetic itself cannot keep that, 4 x the deviation of the float32
CPU oracle from the float64 oracle ON THAT CASE (same arithmetic, another summation order; the device's association order can plausibly add
up to a few times as much).  ``DEV32`` records that deviation for every case, measured on the CPU with ``measure_dev32()``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WEIGHT, GOUT = 0.6, 1.7                   # stage weight and upstream gradient: both != 1

BASE_TOL = {"ce": (2e-6, 2e-6), "mixup": (3e-6, 3e-6), "reg": (3e-6, 3e-6), "was": (1e-5, 1e-4)}      # (loss / max(1,|loss|), grad / max|grad|)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def case_id(c):
    kind, D, H, W, B, inverse, variant, extra = c
    s = "%s-D%d-%dx%d-B%d-%s-%s" % (kind, D, H, W, B, "inv" if inverse else "fwd", variant)
    return s + ("-" + "-".join(str(e) for e in extra) if extra else "")


# ------------------------------------------------------------------------------------------------------------------ the cases
SHAPES = [(2, 1, 1),        # one pixel, one row of the partial-sum grid per batch entry, the smallest D
          (3, 3, 85),       # 255 pixels: one block, its last lane idle
          (5, 16, 16),      # 256 pixels: exactly one full block
          (33, 1, 257),     # two blocks, the second with ONE pixel
          (48, 7, 37),      # 259 pixels, D = 48
          (64, 2, 300)]     # three blocks, tail of 88


def _plain(kind, extras=((),)):
    out = []
    for i, (D, H, W) in enumerate(SHAPES):
        for B, inverse in ((1, i % 2 == 0), (3, i % 2 == 1)):      # B = 1 and 3, both depth orders over the list
            for e in extras:
                out.append((kind, D, H, W, B, inverse, "plain", e))
    return out


# masks that empty whole blocks (5 x 1 x 300: blocks of 256 + 44 pixels; 64 + 11 blocks of the 4-pixel Wasserstein kernel)
def _blocks(kind, extra=()):
    return [(kind, 5, 1, 300, 1, True, "tail_only", extra),        # all-masked block: the first 256 pixels masked, only the tail block valid
            (kind, 5, 1, 300, 1, False, "head_only", extra),       # all-masked block: the ragged tail block is the empty one
            (kind, 5, 1, 300, 3, True, "batch_masked", extra)]     # batch entry 1 fully masked (its partial rows are all zero), 0 and 2 are not


# peaked: logits spread +-80.  ce-D48-7x37-B3-inv-peaked is the regression case of the softmax in the CE / mixup gradient: exp(l - (max + log s))
# rounded at the size of the logits and missed the gradient by 3.9e-6 max|grad|; exp((l - max) - log s) keeps it at the float32 oracle's 2e-7
CE_CASES = _plain("ce") + _blocks("ce") + [("ce", 48, 7, 37, 3, True, "peaked", ()), ("ce", 5, 16, 16, 1, False, "peaked", ())]
MIXUP_CASES = _plain("mixup") + _blocks("mixup") + [("mixup", 48, 7, 37, 3, True, "peaked", ()), ("mixup", 3, 3, 85, 1, False, "peaked", ())]
REG_CASES = _plain("reg", ((0,), (1,))) + _blocks("reg", (1,))     # extra = (mask_out_range,)

# Wasserstein: extra = (ot_iter, ot_eps); H*W in {1, 2, 3, 5, 259}, D in {1, 2, 3, 5, 15, 16, 17, 24, 31, 32}, B in {1, 3}
WAS_CASES = [
    ("was", 1, 1, 1, 1, True, "plain", (1, 1.0)),         # D = 1: one lane holds the whole plan, cost 0
    ("was", 2, 1, 2, 3, True, "plain", (3, 0.5)),         # H*W % 4 = 2: two waves of the only block have pix >= HW
    ("was", 3, 3, 1, 1, True, "plain", (10, 1.0)),        # H*W % 4 = 3, D no power of two
    ("was", 5, 1, 5, 3, True, "plain", (16, 2.0)),        # H*W % 4 = 1, the deepest iteration count (all LDS rows of a_k / b_k)
    ("was", 15, 7, 37, 1, True, "plain", (10, 1.0)),      # D < 16: the upper half of every row is empty (max -inf); 259 pixels, H*W % 4 = 3
    ("was", 16, 1, 3, 1, True, "plain", (3, 0.5)),        # D = 16: the upper half is exactly empty
    ("was", 17, 1, 5, 3, True, "plain", (10, 1.0)),       # 16 < D < 32: ONE entry in the upper half
    ("was", 24, 7, 37, 1, True, "plain", (3, 0.5)),       # 16 < D < 32, upper half partly filled, 65 blocks
    ("was", 31, 1, 2, 1, True, "plain", (16, 2.0)),       # 16 < D < 32: one lane short of a full row
    ("was", 32, 1, 5, 3, True, "plain", (1, 1.0)),        # full rows, a single iteration (a_0 = 0 feeds the reverse sweep directly)
    ("was", 24, 1, 1, 1, True, "plain", (16, 2.0)),       # one pixel: a grid of exactly one row
    ("was", 5, 7, 37, 3, True, "plain", (10, 1.0)),       # D < 16, multi-block, B = 3
    ("was", 31, 3, 1, 1, True, "plain", (10, 1.0)),
] + _blocks("was", (10, 1.0)) + [
    ("was", 17, 1, 5, 1, True, "onehot", (10, 1.0)),      # every probability column exactly one-hot: the others sit on the +1e-12 floor
    ("was", 8, 1, 7, 1, True, "midway", (10, 1.0)),       # ground truth exactly midway between two hypotheses: the tie goes to the first
]

ALL_CASES = CE_CASES + MIXUP_CASES + REG_CASES + WAS_CASES

# Deviation of the float32 CPU oracle from the float64 oracle per case: (|loss32 - loss64|, max|grad32 - grad64| / max|grad64|), from
# measure_dev32().  The bound of a case is max(base tolerance, 4 x this).
DEV32 = {
    "ce-D2-1x1-B1-inv-plain": (3.7e-08, 1.6e-07),
    "ce-D2-1x1-B3-fwd-plain": (5.0e-08, 1.2e-07),
    "ce-D3-3x85-B1-fwd-plain": (5.0e-08, 1.3e-07),
    "ce-D3-3x85-B3-inv-plain": (3.3e-09, 1.4e-07),
    "ce-D5-16x16-B1-inv-plain": (7.7e-08, 1.8e-07),
    "ce-D5-16x16-B3-fwd-plain": (3.5e-08, 1.4e-07),
    "ce-D33-1x257-B1-fwd-plain": (7.9e-08, 1.1e-07),
    "ce-D33-1x257-B3-inv-plain": (3.1e-08, 1.6e-07),
    "ce-D48-7x37-B1-inv-plain": (7.1e-08, 1.6e-07),
    "ce-D48-7x37-B3-fwd-plain": (1.7e-08, 1.5e-07),
    "ce-D64-2x300-B1-fwd-plain": (2.5e-08, 1.3e-07),
    "ce-D64-2x300-B3-inv-plain": (5.8e-08, 2.0e-07),
    "ce-D5-1x300-B1-inv-tail_only": (6.6e-08, 1.8e-07),
    "ce-D5-1x300-B1-fwd-head_only": (5.1e-08, 1.8e-07),
    "ce-D5-1x300-B3-inv-batch_masked": (2.0e-08, 1.4e-07),
    "ce-D48-7x37-B3-inv-peaked": (1.9e-06, 2.7e-07),
    "ce-D5-16x16-B1-fwd-peaked": (1.2e-06, 1.3e-07),
    "mixup-D2-1x1-B1-inv-plain": (0.0e+00, 0.0e+00),
    "mixup-D2-1x1-B3-fwd-plain": (0.0e+00, 0.0e+00),
    "mixup-D3-3x85-B1-fwd-plain": (7.8e-08, 2.0e-07),
    "mixup-D3-3x85-B3-inv-plain": (1.9e-08, 2.2e-07),
    "mixup-D5-16x16-B1-inv-plain": (8.0e-08, 2.3e-07),
    "mixup-D5-16x16-B3-fwd-plain": (1.0e-07, 2.6e-07),
    "mixup-D33-1x257-B1-fwd-plain": (2.6e-08, 1.8e-07),
    "mixup-D33-1x257-B3-inv-plain": (2.1e-08, 1.7e-07),
    "mixup-D48-7x37-B1-inv-plain": (2.6e-09, 2.2e-07),
    "mixup-D48-7x37-B3-fwd-plain": (7.5e-09, 2.8e-07),
    "mixup-D64-2x300-B1-fwd-plain": (4.6e-08, 2.3e-07),
    "mixup-D64-2x300-B3-inv-plain": (4.1e-08, 2.3e-07),
    "mixup-D5-1x300-B1-inv-tail_only": (1.1e-08, 1.8e-07),
    "mixup-D5-1x300-B1-fwd-head_only": (2.4e-09, 1.8e-07),
    "mixup-D5-1x300-B3-inv-batch_masked": (5.6e-08, 2.8e-07),
    "mixup-D48-7x37-B3-inv-peaked": (4.7e-06, 3.8e-07),
    "mixup-D3-3x85-B1-fwd-peaked": (7.2e-07, 2.0e-07),
    "reg-D2-1x1-B1-inv-plain-0": (1.8e-07, 1.3e-07),
    "reg-D2-1x1-B1-inv-plain-1": (1.8e-07, 1.3e-07),
    "reg-D2-1x1-B3-fwd-plain-0": (1.8e-07, 1.2e-06),
    "reg-D2-1x1-B3-fwd-plain-1": (1.8e-07, 1.2e-06),
    "reg-D3-3x85-B1-fwd-plain-0": (3.7e-08, 1.8e-06),
    "reg-D3-3x85-B1-fwd-plain-1": (5.3e-08, 1.8e-06),
    "reg-D3-3x85-B3-inv-plain-0": (2.6e-08, 1.5e-06),
    "reg-D3-3x85-B3-inv-plain-1": (3.1e-08, 1.4e-06),
    "reg-D5-16x16-B1-inv-plain-0": (6.4e-08, 1.7e-06),
    "reg-D5-16x16-B1-inv-plain-1": (9.3e-08, 1.7e-06),
    "reg-D5-16x16-B3-fwd-plain-0": (2.1e-08, 1.8e-06),
    "reg-D5-16x16-B3-fwd-plain-1": (1.0e-08, 1.7e-06),
    "reg-D33-1x257-B1-fwd-plain-0": (1.1e-08, 1.7e-06),
    "reg-D33-1x257-B1-fwd-plain-1": (2.7e-08, 1.7e-06),
    "reg-D33-1x257-B3-inv-plain-0": (4.1e-08, 1.8e-06),
    "reg-D33-1x257-B3-inv-plain-1": (5.7e-08, 1.8e-06),
    "reg-D48-7x37-B1-inv-plain-0": (3.8e-08, 1.6e-06),
    "reg-D48-7x37-B1-inv-plain-1": (8.8e-09, 1.6e-06),
    "reg-D48-7x37-B3-fwd-plain-0": (1.8e-08, 1.9e-06),
    "reg-D48-7x37-B3-fwd-plain-1": (3.2e-08, 2.0e-06),
    "reg-D64-2x300-B1-fwd-plain-0": (2.5e-08, 1.6e-06),
    "reg-D64-2x300-B1-fwd-plain-1": (2.7e-08, 1.6e-06),
    "reg-D64-2x300-B3-inv-plain-0": (3.0e-09, 1.8e-06),
    "reg-D64-2x300-B3-inv-plain-1": (5.5e-09, 1.8e-06),
    "reg-D5-1x300-B1-inv-tail_only-1": (1.7e-07, 1.4e-06),
    "reg-D5-1x300-B1-fwd-head_only-1": (1.8e-08, 1.8e-06),
    "reg-D5-1x300-B3-inv-batch_masked-1": (3.2e-08, 1.9e-06),
    "was-D1-1x1-B1-inv-plain-1-1.0": (0.0e+00, 0.0e+00),
    "was-D2-1x2-B3-inv-plain-3-0.5": (3.3e-08, 1.9e-07),
    "was-D3-3x1-B1-inv-plain-10-1.0": (1.9e-08, 9.8e-08),
    "was-D5-1x5-B3-inv-plain-16-2.0": (1.1e-08, 2.9e-07),
    "was-D15-7x37-B1-inv-plain-10-1.0": (8.1e-09, 2.2e-06),
    "was-D16-1x3-B1-inv-plain-3-0.5": (2.2e-07, 3.5e-07),
    "was-D17-1x5-B3-inv-plain-10-1.0": (7.3e-08, 9.7e-07),
    "was-D24-7x37-B1-inv-plain-3-0.5": (5.5e-09, 1.1e-06),
    "was-D31-1x2-B1-inv-plain-16-2.0": (1.7e-07, 1.6e-06),
    "was-D32-1x5-B3-inv-plain-1-1.0": (7.0e-07, 1.3e-06),
    "was-D24-1x1-B1-inv-plain-16-2.0": (6.2e-08, 1.3e-06),
    "was-D5-7x37-B3-inv-plain-10-1.0": (9.9e-09, 3.8e-07),
    "was-D31-3x1-B1-inv-plain-10-1.0": (4.0e-08, 7.6e-07),
    "was-D5-1x300-B1-inv-tail_only-10-1.0": (2.7e-08, 3.3e-07),
    "was-D5-1x300-B1-fwd-head_only-10-1.0": (3.6e-08, 3.8e-07),
    "was-D5-1x300-B3-inv-batch_masked-10-1.0": (2.6e-09, 6.1e-07),
    "was-D17-1x5-B1-inv-onehot-10-1.0": (2.9e-07, 1.7e-06),
    "was-D8-1x7-B1-inv-midway-10-1.0": (1.1e-07, 2.2e-07),
}


# ------------------------------------------------------------------------------------------------------------------ inputs
def build_case(c):
    """-> dict of float32 CPU tensors: x (logits | prob | depth), dv, gt, mask (+ interval for reg)."""
    from oracle import ref_losses
    kind, D, H, W, B, inverse, variant, extra = c
    seed = 1000 + 7 * D + 3 * H * W + B + (50 if inverse else 0)
    gen = torch.Generator().manual_seed(seed)
    inputs, gts, masks = ref_losses.make_loss_case(seed=seed, B=B, sizes=((D, H, W),), inverse_depth=inverse)
    dv, logits = inputs["stage1"]["depth_values"], inputs["stage1"]["prob_volume_pre"]
    gt, mask = gts["stage1"].clone(), masks["stage1"].clone()
    # one pixel per batch entry valid for every loss: the ground truth on a hypothesis, mask 1
    gt[:, -1, -1] = dv[:, D // 2, -1, -1]
    mask[:, -1, -1] = 1.0
    flat = mask.reshape(B, -1)                              # a view: the edits below land in mask
    if variant == "tail_only":
        flat[:, :256] = 0.2
        flat[:, 256:] = 0.9
        gt.reshape(B, -1)[:, 256:] = dv.reshape(B, D, -1)[:, D // 2, 256:] * 1.0001
    elif variant == "head_only":
        flat[:, 256:] = 0.0
        flat[:, :256:3] = 0.9
        gt.reshape(B, -1)[:, :256:3] = dv.reshape(B, D, -1)[:, D // 2, :256:3] * 0.9999
    elif variant == "batch_masked":
        flat[1] = 0.5                                       # not > 0.5
    out = dict(dv=dv, gt=gt, mask=mask)
    if kind in ("ce", "mixup"):
        if variant == "peaked":
            logits = (torch.rand(B, D, H, W, generator=gen) * 2 - 1) * 80.0
        out["x"] = logits.contiguous()
    elif kind == "reg":
        # depth around the truth by ~ +-1.5 intervals: both zones of the smooth L1; intervals of ~ 40 keep depth / itv ~ 15, so that the float32
        # cancellation in depth / itv - gt / itv (2^-23 of that) stays near the base tolerance
        out["interval"] = torch.tensor([37.0, 52.5, 41.25][:B])
        out["x"] = (gt + out["interval"].reshape(B, 1, 1) * 1.5 * torch.randn(B, H, W, generator=gen)).contiguous()
    else:
        prob = torch.softmax(logits, 1)
        if variant == "onehot":
            hot = torch.randint(0, D, (B, 1, H, W), generator=gen)
            prob = torch.zeros(B, D, H, W).scatter_(1, hot, 1.0)
        elif variant == "midway":
            # hypotheses 1000 - 8 d (exact), ground truth 4 below hypothesis k: |dv[k] - gt| == |dv[k+1] - gt| == 4 exactly
            dv = (1000.0 - 8.0 * torch.arange(D, dtype=torch.float32)).reshape(1, D, 1, 1).expand(B, D, H, W).contiguous()
            k = torch.randint(0, D - 1, (B, H, W), generator=gen)
            gt = torch.gather(dv, 1, k.unsqueeze(1)).squeeze(1) - 4.0
            mask = torch.ones(B, H, W)
            assert torch.equal(ref_losses.nearest_hypothesis(dv, gt), k)      # the reference takes the first of the two
            prob = torch.softmax(torch.randn(B, D, H, W, generator=gen), 1)
            out.update(dv=dv, gt=gt, mask=mask)
        out["x"] = prob.contiguous()
    return out


def valid_pixels(c, t):
    """The float32 decisions: bool [B,H,W] of the pixels that enter the loss (+ the CE bin index)."""
    from oracle import ref_losses
    kind, inverse, extra = c[0], c[5], c[7]
    if kind == "ce":
        index, final = ref_losses.gt_bins(t["dv"], t["gt"], t["mask"], inverse)
        return final, index
    if kind == "mixup":
        return ref_losses.mixup_bins(t["dv"], t["gt"], t["mask"], inverse)[1] > 0, None
    if kind == "reg":
        return ref_losses.reg_select(t["dv"], t["gt"], t["mask"], bool(extra[0]), inverse), None
    return t["mask"] > 0.5, None


def ref_eval(c, t, dtype):
    """-> (loss as a Python float, d (GOUT * loss) / d x) of the CPU oracle in ``dtype``."""
    from oracle import ref_losses
    kind, inverse, extra = c[0], c[5], c[7]
    x = t["x"].to(dtype).requires_grad_(True)
    dv, gt, mask = t["dv"].to(dtype), t["gt"].to(dtype), t["mask"].to(dtype)
    if kind == "ce":
        loss = ref_losses.ce_loss_stage(x, dv, gt, mask, inverse, WEIGHT)
    elif kind == "mixup":
        loss = ref_losses.mixup_ce_loss_stage(x, dv, gt, mask, inverse, WEIGHT)
    elif kind == "reg":
        loss = ref_losses.reg_loss_stage(x, dv, gt, mask, t["interval"].to(dtype), bool(extra[0]), inverse, WEIGHT)
    else:
        loss = ref_losses.sinkhorn_stage(x, dv, gt, mask, extra[0], extra[1], WEIGHT)
    assert loss.dtype == dtype
    (GOUT * loss).backward()
    return loss.item(), x.grad


def measure_dev32(cases=None):
    """CPU only: the DEV32 table (float32 oracle against float64 oracle) for ``cases``."""
    out = {}
    for c in cases or ALL_CASES:
        t = build_case(c)
        l64, g64 = ref_eval(c, t, torch.float64)
        l32, g32 = ref_eval(c, t, torch.float32)
        out[case_id(c)] = (abs(l32 - l64), ((g32.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-300)).item())
    return out


def hip_eval(c, t, dev, want_grad=True, want_index=False):
    from mvsformer_amd import ops
    kind, inverse, extra = c[0], c[5], c[7]
    x, dv, gt, mask = (t[k].to(dev) for k in ("x", "dv", "gt", "mask"))
    if kind == "ce":
        return ops.ce_loss(x, dv, gt, mask, inverse, WEIGHT, want_grad=want_grad, want_index=want_index)
    if kind == "mixup":
        return ops.mixup_ce_loss(x, dv, gt, mask, inverse, WEIGHT, want_grad=want_grad)
    if kind == "reg":
        return ops.reg_loss(x, gt, mask, t["interval"].to(dev), dv if extra[0] else None, inverse, WEIGHT, want_grad=want_grad)
    return ops.was_loss(x, dv, gt, mask, extra[0], extra[1], WEIGHT, want_grad=want_grad)


def check_case(c, dev):
    from mvsformer_amd import ops
    kind = c[0]
    t = build_case(c)
    valid, index = valid_pixels(c, t)
    nvalid = int(valid.sum())
    assert all(int(v.sum()) >= 1 for i, v in enumerate(valid) if not (c[6] == "batch_masked" and i == 1)), "a batch entry without a valid pixel"
    want_loss, want_grad = ref_eval(c, t, torch.float64)

    res = hip_eval(c, t, dev, want_index=(kind == "ce"))
    loss, acc, grad_unscaled = res[:3]
    grad = ops.ce_loss_bwd_scale(grad_unscaled, acc, torch.tensor([GOUT], device=dev), WEIGHT).cpu().double()
    loss_nograd = hip_eval(c, t, dev, want_grad=False)[0]

    dev32 = DEV32[case_id(c)]
    tol_loss = max(BASE_TOL[kind][0] * max(1.0, abs(want_loss)), 4.0 * dev32[0])
    tol_grad = max(BASE_TOL[kind][1], 4.0 * dev32[1]) * want_grad.abs().max().item()
    err_loss = abs(loss.item() - want_loss)
    err_grad = (grad - want_grad).abs().max().item()
    print("%s: loss %.9g want %.9g err %.3e (tol %.3e)  grad err %.3e of max %.3e = %.3e (tol %.3e)  valid %d" % (
        case_id(c), loss.item(), want_loss, err_loss, tol_loss, err_grad, want_grad.abs().max().item(),
        err_grad / max(want_grad.abs().max().item(), 1e-300), tol_grad / max(want_grad.abs().max().item(), 1e-300), nvalid))
    assert err_loss <= tol_loss
    assert grad.shape == want_grad.shape and err_grad <= tol_grad
    if kind == "ce":
        assert torch.equal(res[3].cpu(), valid) and torch.equal(res[4].cpu().long(), index)
    if kind == "mixup":                   # the float sum of the mask + 1e-6, added in float32 as the reference does
        assert acc[1].item() == (torch.tensor(float(nvalid), dtype=torch.float32) + torch.tensor(1e-6, dtype=torch.float32)).item()
    else:
        assert acc[1].item() == nvalid
    inval = ~valid
    g = grad if kind == "reg" else grad.permute(0, 2, 3, 1)
    assert (g[inval] == 0).all(), "gradient on an invalid pixel"
    assert torch.equal(loss_nograd.cpu().view(torch.int32), loss.cpu().view(torch.int32)), "want_grad=False changes the loss"


@pytest.mark.parametrize("c", CE_CASES, ids=case_id)
def test_ce_loss_vs_fp64(dev, c):
    check_case(c, dev)


@pytest.mark.parametrize("c", MIXUP_CASES, ids=case_id)
def test_mixup_ce_loss_vs_fp64(dev, c):
    check_case(c, dev)


@pytest.mark.parametrize("c", REG_CASES, ids=case_id)
def test_reg_loss_vs_fp64(dev, c):
    check_case(c, dev)


@pytest.mark.parametrize("c", WAS_CASES, ids=case_id)
def test_was_loss_vs_fp64(dev, c):
    check_case(c, dev)


@pytest.mark.parametrize("kind,extra", [("ce", ()), ("mixup", ()), ("reg", (0,)), ("reg", (1,)), ("was", (10, 1.0))])
def test_nothing_valid(dev, kind, extra):
    """No pixel with mask > 0.5 (two blocks of all-zero partial rows): the means over an empty selection are NaN as in the reference, the
    mixup loss, whose denominator is sum(mask) + 1e-6, is exactly 0 with an all-zero gradient."""
    from mvsformer_amd import ops
    c = (kind, 5, 1, 300, 3, True, "plain", extra)
    t = build_case(c)
    t["mask"] = torch.full_like(t["mask"], 0.5)
    want, _ = ref_eval(c, t, torch.float64)
    loss, acc, grad_unscaled = hip_eval(c, t, dev)[:3]
    assert (grad_unscaled == 0).all()
    if kind == "mixup":
        assert want == 0.0 and loss.item() == 0.0
        assert acc[1].item() == torch.tensor(1e-6, dtype=torch.float32).item()
        grad = ops.ce_loss_bwd_scale(grad_unscaled, acc, torch.tensor([GOUT], device=dev), WEIGHT)
        assert (grad == 0).all()
    else:
        assert want != want and torch.isnan(loss).item()
        assert acc[1].item() == 0.0


def test_refusals(dev):
    """Shapes and settings that are not built are refused before anything is launched."""
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError

    def args(D):
        return (torch.full((1, D, 2, 3), 1.0 / D, device=dev), torch.arange(1, D + 1, device=dev, dtype=torch.float32).reshape(1, D, 1, 1).expand(1, D, 2, 3).contiguous(),
                torch.ones(1, 2, 3, device=dev), torch.ones(1, 2, 3, device=dev))
    with pytest.raises(MvsHipError):
        ops.was_loss(*args(33))                                    # a row of the plan is one wavefront half: D <= 32
    for it in (0, 17):
        with pytest.raises(MvsHipError):
            ops.was_loss(*args(8), ot_iter=it)                     # LDS holds the iterates of 1 .. 16 iterations
    with pytest.raises(MvsHipError):
        ops.was_loss(*args(8), ot_eps=0.0)
    with pytest.raises(MvsHipError):
        ops.ce_loss(*args(1), True)                                # D = 1: no interval
    with pytest.raises(MvsHipError):
        ops.mixup_ce_loss(*args(1), True)
    loss, _, _ = ops.was_loss(*args(8))                            # the same arguments within the limits run
    assert torch.isfinite(loss).item()
