"""``csrc/head.hip`` against float64 at the edges of its launches: ``mvs_head_fwd`` (generic kernel, register-resident kernel in its small and
large launch, fused 1x1x1 conv), ``mvs_depth_regression``, ``mvs_conf_regression``, ``mvs_init_inverse_range``, ``mvs_schedule_inverse_range`` and
``mvs_conf_accumulate``.  Every kernel maps one lane to one pixel in blocks of 64 x 4 (64 x 1 in the small register launch), so the maps here
are 1 x 1, W = 63 / 64 / 65 / 130 (one lane short of a block, exactly one, one lane and two lanes into the next ones) with H % 4 != 0.

The reference is ``oracle/ref_torch.py`` plus plain softmax / gather on float64 copies of the same float32 inputs.  Inputs are seeded and built
on the CPU; where a result depends on a discrete choice (argmax, a floor) the inputs keep every pixel away from the decision boundary - or put
it exactly on it where the tie rule is what is tested - so every pixel is compared."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

HW_LIST = [(1, 1), (3, 63), (5, 64), (2, 65), (7, 130)]      # W crosses the 64-lane block at 65 and 130; H % 4 = 1, 3, 1, 2, 3
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def hypotheses(B, D, H, W, gen):
    """Inverse-depth columns (descending depth) around a per-pixel centre, as the cascade's schedulers produce them."""
    centre = 1.0 / (500.0 + 300.0 * torch.rand(B, 1, H, W, generator=gen))
    steps = torch.linspace(-1, 1, D).view(1, D, 1, 1) if D > 1 else torch.zeros(1, 1, 1, 1)
    return (1.0 / (centre * (1 + 0.25 * steps))).contiguous()


def first_argmax(l):
    """Index of the FIRST maximum along dim 1 (exact comparisons on the given values)."""
    eq = l == l.max(1, keepdim=True)[0]
    first = eq & (eq.long().cumsum(1) == 1)
    assert (first.sum(1) == 1).all()
    return first.long().argmax(1)


def gapped_logits(B, D, H, W, gen, ties=True):
    """Logits whose maximum leads the runner-up by >= 0.75 (a factor 2 in probability: no rounding can swap them), except on every 5th pixel,
    where two - every 10th: three, if D allows - logits are EXACTLY the same maximum."""
    l = torch.randn(B, D, H, W, generator=gen) * 2.0
    l.scatter_add_(1, l.argmax(1, keepdim=True), torch.full((B, 1, H, W), 0.75))
    if ties and D >= 2:
        flat = l.reshape(B, D, H * W)                        # a view
        top = flat.max(1)[0]
        for p in range(0, H * W, 5):
            where = torch.randperm(D, generator=gen)[:(3 if (p % 10 == 0 and D >= 3) else 2)]
            flat[:, where, p] = top[:, p].unsqueeze(1)
    return l.contiguous()


def head_reference(l, dv, tmp):
    l64, dv64 = l.double(), dv.double()
    prob = torch.softmax(l64, 1)
    arg = first_argmax(l)
    return dict(prob=prob, conf=prob.max(1)[0], arg=arg, depth_train=torch.gather(dv, 1, arg.unsqueeze(1)).squeeze(1),
                depth_eval=(torch.softmax(l64 * tmp, 1) * dv64).sum(1))


def check_head(out, want, training):
    pre, prob, depth, conf = (o.cpu() for o in out)
    assert (prob.double() - want["prob"]).abs().max().item() < 1e-6
    assert (conf.double() - want["conf"]).abs().max().item() < 1e-6
    if training:
        assert torch.equal(depth, want["depth_train"]), "training depth is not the hypothesis at the first argmax on %d pixels" % (
            depth != want["depth_train"]).sum().item()
    else:
        assert rel_err(depth, want["depth_eval"]) < 1e-6
    # equal logits give equal probabilities bit for bit, so the confidence is the probability AT the first argmax
    assert torch.equal(conf, torch.gather(prob, 1, want["arg"].unsqueeze(1)).squeeze(1))


def _head_cases():
    out, i = [], 0
    for D in (1, 2, 3, 5, 33, 48, 4, 8, 16, 32):             # the first six: generic kernel; the last four: register-resident kernel (small launch)
        for H, W in HW_LIST:
            out.append((D, H, W, (1, 3)[i % 2], (1.0, 5.0)[(i // 2) % 2], bool((i // 4) % 2)))
            i += 1
    return out


@pytest.mark.parametrize("D,H,W,B,tmp,training", _head_cases())
def test_head_logits_in_memory(dev, D, H, W, B, tmp, training):
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(100 * D + H * W + B)
    dv, l = hypotheses(B, D, H, W, gen), gapped_logits(B, D, H, W, gen)
    out = ops.head(dv.to(dev), tmp, training, logits=l.to(dev))
    check_head(out, head_reference(l, dv, tmp), training)


@pytest.mark.parametrize("H,W,training", [
    (514, 510, True),     # 262 140 pixels: the LAST size of the one-wavefront-per-block launch (grid.y = H = 514)
    (514, 511, True),     # large-launch register head: 262 654 >= 256 * 1024 pixels, 4 rows per block, H % 4 = 2, W % 64 = 63
    (514, 511, False),
])
def test_head_register_kernel_large_launch(dev, H, W, training):
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(H + W)
    dv, l = hypotheses(1, 4, H, W, gen), gapped_logits(1, 4, H, W, gen)
    out = ops.head(dv.to(dev), 5.0, training, logits=l.to(dev))
    check_head(out, head_reference(l, dv, 5.0), training)


@pytest.mark.parametrize("C,D,H,W,B,training", [(8, 5, 1, 1, 1, True), (16, 8, 1, 1, 3, False), (8, 8, 3, 65, 3, False), (16, 5, 3, 65, 1, True),
                                                (8, 3, 6, 130, 1, False), (16, 4, 6, 130, 3, True)])
def test_head_fused_conv(dev, C, D, H, W, B, training):
    """The fused 1x1x1 conv: ``prob_volume_pre`` against a float64 conv (the bound of a chain of C fused multiply-adds and the bias add:
    (C + 1) 2^-24 (sum |w x| + |b|)), everything else against the float64 head of that float64 conv.  The inputs are re-seeded until the
    float64 logits' top two are >= 1e-3 apart on every pixel - 100 x the conv's rounding - so the exact argmax check exempts no pixel."""
    from mvsformer_amd import ops
    for seed in range(50):
        gen = torch.Generator().manual_seed(1000 * C + 10 * D + H * W + seed * 7919)
        x8 = torch.randn(B, C, D, H, W, generator=gen)
        w1, b1 = torch.randn(C, generator=gen) * 0.4, torch.randn(1, generator=gen)
        pre64 = (x8.double() * w1.double().view(1, C, 1, 1, 1)).sum(1) + b1.double()
        top2 = pre64.topk(2, dim=1)[0]
        if (top2[:, 0] - top2[:, 1]).min().item() >= 1e-3:
            break
    else:
        raise AssertionError("no seed with a clear argmax on every pixel")
    mag = (x8.double() * w1.double().view(1, C, 1, 1, 1)).abs().sum(1) + b1.double().abs()
    assert (mag * (C + 1) * EPS).max().item() < 1e-5
    dv = hypotheses(B, D, H, W, gen)
    out = ops.head(dv.to(dev), 5.0, training, x8=x8.to(dev), w1=w1.to(dev), b1=b1.to(dev))
    assert ((out[0].cpu().double() - pre64).abs() <= (C + 1) * EPS * mag).all()
    check_head(out, head_reference(pre64, dv, 5.0), training)


@pytest.mark.parametrize("D", [5, 8])                         # generic and register-resident kernel
@pytest.mark.parametrize("training", [True, False])
def test_head_extreme_logits(dev, D, training):
    """Logits spread over +-80 and tmp * logit up to +-400, far beyond the float32 range of exp: no NaN or infinity anywhere, probabilities still
    sum to 1, the argmax rule still holds."""
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(D)
    B, H, W = 3, 3, 65
    dv = hypotheses(B, D, H, W, gen)
    l = (torch.rand(B, D, H, W, generator=gen) * 2 - 1) * 80.0
    l.scatter_add_(1, l.argmax(1, keepdim=True), torch.full((B, 1, H, W), 0.75))
    l[:, 0, 0, 0], l[:, D - 1, 0, 0] = -80.0, 80.0          # the full spread inside one column
    out = ops.head(dv.to(dev), 5.0, training, logits=l.to(dev))
    for o in out[1:]:
        assert torch.isfinite(o).all()
    assert (out[1].cpu().double().sum(1) - 1.0).abs().max().item() < 1e-6
    check_head(out, head_reference(l, dv, 5.0), training)


@pytest.mark.parametrize("per_pixel", [True, False])
@pytest.mark.parametrize("D", [1, 5, 48])
@pytest.mark.parametrize("H,W", HW_LIST)
def test_depth_regression(dev, H, W, D, per_pixel):
    """sum_d p dv for both hypothesis layouts.  A chain of D multiply-adds on positive terms: |error| <= (D + 1) 2^-24 sum |p dv|."""
    from mvsformer_amd import ops
    from oracle import ref_torch
    B = 3
    gen = torch.Generator().manual_seed(D * 1000 + H * W)
    p = torch.softmax(torch.randn(B, D, H, W, generator=gen) * 2, 1)
    dv = hypotheses(B, D, H, W, gen) if per_pixel else hypotheses(B, D, 1, 1, gen).reshape(B, D).contiguous()
    got = ops.depth_regression(p.to(dev), dv.to(dev)).cpu().double()
    want = ref_torch.depth_regression(p.double(), dv.double())
    assert got.shape == want.shape
    assert ((got - want).abs() <= (D + 1) * EPS * want).all()


def conf_columns(B, D, H, W, gen):
    """Probability columns for conf_regression: even pixels random, every expectation sum_d p d at least 1e-3 away from an integer (columns
    that are not get redrawn) - 30 x the worst float32 rounding of that sum at D = 33 - odd pixels exactly one-hot (the expectation is an
    exact integer in float32 and in float64)."""
    p = torch.softmax(torch.randn(B, D, H, W, generator=gen) * 1.5, 1)
    ar = torch.arange(D, dtype=torch.float64).view(1, D, 1, 1)
    if D > 1:
        for _ in range(100):
            e = (p.double() * ar).sum(1, keepdim=True)
            bad = ((e - e.round()).abs() < 1e-3).expand_as(p)
            if not bad.any():
                break
            p = torch.where(bad, torch.softmax(torch.randn(B, D, H, W, generator=gen) * 1.5, 1), p)
        else:
            raise AssertionError("could not keep the expectations away from the integers")
    hot = torch.zeros(B, D, H, W).scatter_(1, torch.randint(0, D, (B, 1, H, W), generator=gen), 1.0)
    odd = (torch.arange(H * W).reshape(1, 1, H, W) % 2 == 1).expand_as(p)
    return torch.where(odd, hot, p).contiguous()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("D,H,W", [(1, 1, 1), (2, 3, 63), (8, 2, 65), (33, 7, 130), (8, 5, 64), (2, 7, 130)])
def test_conf_regression(dev, D, H, W, n):
    """The window of n probabilities around floor(sum_d p d): clipped at both ends of the column (D = 2 and 8), wider than the column
    (n > D).  Up to n additions, a division and a product: |error| <= (n + 2) 2^-24 of the window's sum."""
    from mvsformer_amd import ops
    from oracle import ref_torch
    B = 3
    gen = torch.Generator().manual_seed(D * 100 + H * W)
    p = conf_columns(B, D, H, W, gen)
    ar = torch.arange(D, dtype=torch.float32).reshape(1, D)
    assert torch.equal(ref_torch.depth_regression(p, ar).long(), ref_torch.depth_regression(p.double(), ar.double()).long())     # same floor in both
    got = ops.conf_regression(p.to(dev), n).cpu().double()
    want = ref_torch.conf_regression(p.double(), n)
    assert got.shape == want.shape
    assert ((got - want).abs() <= (n + 2) * EPS * want + 1e-12).all(), (got - want).abs().max().item()


@pytest.mark.parametrize("N", [1, 2, 192])
@pytest.mark.parametrize("D", [2, 3, 48])
def test_init_inverse_range(dev, D, N):
    """Uniform inverse-depth planes between range[:, 0] and range[:, -1] on a 5 x 70 map (W > 64, H % 4 = 1), B = 3.  Two reciprocals, a
    quotient, a multiply-add on positive terms and a reciprocal: < 1e-6 relative, the bound of the golden test."""
    from mvsformer_amd import ops
    from oracle import ref_torch
    B, H, W = 3, 5, 70
    gen = torch.Generator().manual_seed(D * 7 + N)
    near = 400.0 + 100.0 * torch.rand(B, 1, generator=gen)
    rng = (near + torch.linspace(0, 1, N).view(1, N) * 500.0).contiguous() if N > 1 else near.contiguous()
    got = ops.init_inverse_range(rng.to(dev), D, H, W).cpu()
    want = ref_torch.init_inverse_range(rng.double(), D, H, W)
    assert got.shape == want.shape and rel_err(got, want) < 1e-6
    assert (got == got[:, :, :1, :1]).all()                   # a plane is one value per batch entry
    if N == 1:                                                # near == far: every plane is the same depth
        assert (got == got[:, :1]).all()


@pytest.mark.parametrize("H,W", [(2, 2),       # Hl = Wl = 1: the align_corners scale of a one-pixel axis is 0
                                 (2, 130),     # Hl = 1 only; W crosses two 64-lane blocks
                                 (6, 4),       # H % 4 = 2
                                 (10, 66)])    # W crosses 64, H % 4 = 2
@pytest.mark.parametrize("D,Dp,B", [(2, 3, 1), (16, 3, 3), (2, 8, 3), (16, 8, 1)])
def test_schedule_inverse_range(dev, H, W, D, Dp, B):
    from mvsformer_amd import ops
    from oracle import ref_torch
    gen = torch.Generator().manual_seed(H * W + D + Dp)
    prev_hyp = hypotheses(B, Dp, H // 2, W // 2, gen)
    prev_depth = (prev_hyp[:, Dp // 2] * (1 + 0.02 * torch.randn(B, H // 2, W // 2, generator=gen))).contiguous()
    got = ops.schedule_inverse_range(prev_depth.to(dev), prev_hyp.to(dev), D, 0.8, H, W).cpu()
    want = ref_torch.schedule_inverse_range(prev_depth.double(), prev_hyp.double(), D, 0.8, H, W)
    assert got.shape == want.shape and (want > 0).all()
    assert rel_err(got, want) < 2e-6


def test_schedule_inverse_range_refusals(dev):
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    gen = torch.Generator().manual_seed(0)
    hyp = hypotheses(1, 3, 1, 2, gen).to(dev)
    with pytest.raises(MvsHipError):
        ops.schedule_inverse_range(hyp[:, 1].contiguous(), hyp, 4, 0.8, 3, 4)      # odd H (3 // 2 == 1 passes the half-size check)
    with pytest.raises(MvsHipError):
        ops.schedule_inverse_range(hyp[:, 1].contiguous(), hyp, 4, 0.8, 2, 5)      # odd W
    with pytest.raises(MvsHipError):
        ops.schedule_inverse_range(hyp[:, 1].contiguous(), hyp[:, :2].contiguous(), 4, 0.8, 2, 4)      # Dp = 2: no hypotheses 1 and 2
    assert torch.isfinite(ops.schedule_inverse_range(hyp[:, 1].contiguous(), hyp, 4, 0.8, 2, 4)).all()


@pytest.mark.parametrize("H,W,Hf,Wf", [(3, 9, 24, 72),      # x8, Wf crosses 64
                                       (3, 17, 12, 68),     # x4
                                       (5, 33, 10, 66),     # x2, Hf % 4 = 2
                                       (5, 70, 5, 70),      # x1, Hf % 4 = 1
                                       (5, 7, 13, 18)])     # non-integer scales 5/13 and 7/18
def test_conf_accumulate(dev, H, W, Hf, Wf):
    """acc += weight * nearest-upsampled confidence, twice into the same acc with different maps and weights (a read-modify-write, not a
    store).  Each term passes through at most three float32 roundings: |error| <= 3 * 2^-24 (|acc0| + |w1 c1| + |w2 c2|)."""
    import numpy as np
    from mvsformer_amd import ops
    B = 3
    # the kernel's source pixel floor(dst * (float)in / (float)out) is the exact rational floor(dst * in / out) at these sizes
    for n_in, n_out in ((H, Hf), (W, Wf)):
        dst = np.arange(n_out)
        kernel_src = np.minimum(np.floor(dst.astype(np.float32) * (np.float32(n_in) / np.float32(n_out))).astype(np.int64), n_in - 1)
        assert (kernel_src == (dst * n_in) // n_out).all()
    gen = torch.Generator().manual_seed(H * W + Hf)
    c1, c2 = torch.rand(B, H, W, generator=gen), torch.rand(B, H, W, generator=gen)
    acc0 = torch.rand(B, Hf, Wf, generator=gen)
    w1, w2 = 0.75, 1.3
    up = lambda c: F.interpolate(c.double().unsqueeze(1), [Hf, Wf], mode="nearest").squeeze(1)
    iy, ix = (torch.arange(Hf) * H) // Hf, (torch.arange(Wf) * W) // Wf
    assert torch.equal(up(c1), c1.double()[:, iy][:, :, ix])                    # F.interpolate picks that pixel too
    want = acc0.double() + w1 * up(c1) + w2 * up(c2)
    acc = acc0.to(dev)
    ops.conf_accumulate(c1.to(dev), acc, w1)
    ops.conf_accumulate(c2.to(dev), acc, w2)
    bound = 3 * EPS * (acc0.double().abs() + w1 * up(c1).abs() + w2 * up(c2).abs())
    assert ((acc.cpu().double() - want).abs() <= bound).all()
