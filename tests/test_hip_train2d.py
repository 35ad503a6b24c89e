"""GPU parity of the 2-D training pieces, each against the same operation in fp64 on the CPU: the three modes of
``mvs_conv2d_gemm_x3`` (``ops.conv2d_fwd_x3`` / ``conv2d_dgrad_x3`` / ``conv2d_wgrad_x3``) called directly and through
``fpn.Conv2dFn`` / ``vit.ConvT2dFn``, the decoder's bilinear x2 upsampling + lateral add and its adjoint
(``csrc/fpn_train.hip``), ``fpn.BiasFn``, ``ops.ewise_mul`` / ``vit.MulFn``.

Inputs come from a seeded CPU generator and are fp32 values, so both sides see the same numbers; the metric is
``test_hip_training.relclose``'s (max |err| / max |want|).  Tolerances are the project's: 2e-5 on convolution outputs and 5e-5 on
their gradients (``test_conv_fn_grads``), 1e-6 on elementwise and upsampling results (``test_small_fns``).  Where a case is marked
``wide`` the bound is instead 4 x the error of torch's OWN fp32 implementation of the op against the same fp64 reference on the same
inputs (computed on the CPU inside the test, never through this project's kernels), if that is larger: the factor covers a different
but equally valid summation order."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def relerr(got, want):
    got = torch.as_tensor(got).detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-12)


def check(got, want, tol, what, torch32=None):
    """``torch32``: the same quantity from torch's fp32 CPU implementation - widens ``tol`` to 4 x its error (module docstring)."""
    err = relerr(got, want)
    if torch32 is not None:
        e32 = relerr(torch32, want)
        print("%s: torch fp32 err %.3e" % (what, e32))
        tol = max(tol, 4.0 * e32)
    print("%s: err %.3e (tol %.1e)" % (what, err, tol))
    assert err < tol, "%s: max err / max|want| = %.3e (tol %.1e)" % (what, err, tol)


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


# (why, N, Cin, Cout, H, W, KS, S, P)
CONV2D_CASES = [
    ("FPNEncoder conv0: 7x7/s1/p3 on the 3-channel image", 2, 3, 8, 12, 20, 7, 1, 3),
    ("FPNEncoder 5x5/s1/p2", 1, 8, 8, 9, 13, 5, 1, 2),
    ("FPNEncoder 5x5/s2/p2, even H and W", 2, 8, 24, 12, 16, 5, 2, 2),
    ("5x5/s2/p2, odd H and W", 1, 3, 8, 11, 15, 5, 2, 2),
    ("5x5/s2/p2, odd H, even W", 1, 8, 1, 7, 10, 5, 2, 2),
    ("FPNEncoder 3x3/s1/p1", 2, 24, 24, 7, 9, 3, 1, 1),
    ("FPNEncoder 3x3/s2/p1, even H and W", 1, 24, 64, 10, 14, 3, 2, 1),
    ("3x3/s2/p1, odd H and W", 2, 64, 24, 9, 13, 3, 2, 1),
    ("3x3/s2/p1, even H, odd W", 1, 1, 3, 6, 9, 3, 2, 1),
    ("decoder 1x1/s1/p0", 2, 64, 8, 6, 10, 1, 1, 0),
    ("decoder 3x3/s1/p1, 64 -> 3 (Cout not a multiple of 8)", 1, 64, 3, 5, 12, 3, 1, 1),
    ("Ho*Wo = 1 (a 1x1 map under 3x3/p1)", 2, 8, 8, 1, 1, 3, 1, 1),
    ("Ho*Wo = 1 under 5x5/s2/p2 (a 1x2 map)", 1, 3, 24, 1, 2, 5, 2, 2),
    ("Ho*Wo = 31: one short K step", 1, 1, 1, 1, 31, 1, 1, 0),
    ("Ho*Wo = 32: exactly one K step", 2, 8, 3, 4, 8, 3, 1, 1),
    ("Ho*Wo = 33: nsplit = 2, the last split holds ONE pixel", 1, 3, 8, 3, 11, 3, 1, 1),
    ("Ho*Wo = 33 with batch 2", 2, 24, 1, 3, 11, 3, 1, 1),
    ("Ho*Wo = 70: nsplit = 3, ragged last split of 6 pixels", 2, 8, 8, 7, 10, 3, 1, 1),
    ("4x4/s2/p1 as a plain convolution (the transposed convolutions' data gradient)", 2, 8, 24, 6, 10, 4, 2, 1),
]


def _conv2d_ref(x, w, dy, S, P, dtype):
    xr, wr = x.to(dtype).requires_grad_(True), w.to(dtype).requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride=S, padding=P)
    dx, dw = torch.autograd.grad(y, (xr, wr), dy.to(dtype))
    return y.detach(), dx, dw


def _conv2d_inputs(seed, N, Cin, Cout, H, W, KS, S, P):
    gen = torch.Generator().manual_seed(seed)
    x = randn(gen, N, Cin, H, W)
    w = randn(gen, Cout, Cin, KS, KS) / (KS * KS * Cin) ** 0.5
    Ho, Wo = (H + 2 * P - KS) // S + 1, (W + 2 * P - KS) // S + 1
    dy = randn(gen, N, Cout, Ho, Wo)
    return x, w, dy


@pytest.mark.parametrize("why,N,Cin,Cout,H,W,KS,S,P", CONV2D_CASES, ids=[c[0] for c in CONV2D_CASES])
def test_conv2d_x3_modes_direct(dev, why, N, Cin, Cout, H, W, KS, S, P):
    from mvsformer_amd import ops
    x, w, dy = _conv2d_inputs(N + Cin + Cout + H + W + KS, N, Cin, Cout, H, W, KS, S, P)
    y, dx, dw = _conv2d_ref(x, w, dy, S, P, torch.float64)
    xm, wm, dym = x.to(dev), w.to(dev), dy.to(dev)
    ym = ops.conv2d_fwd_x3(xm, wm, S, P)
    assert ym.shape == y.shape
    check(ym, y, 2e-5, "y")
    check(ops.conv2d_dgrad_x3(dym, wm, S, P, H, W), dx, 5e-5, "dX")
    check(ops.conv2d_wgrad_x3(dym, xm, KS, S, P), dw, 5e-5, "dW")


def test_conv2d_wgrad_large_reduction(dev):
    """A 256x320 map, 8 -> 8 channels: K = 81 920 pixels in 1280 splits of 64, added by mvs_partials_reduce.  ``wide``: torch's fp32
    CPU weight gradient measured 8.3e-6 against fp64 on these inputs, so the project's 5e-5 is the bound in force (4 x 8.3e-6 is smaller)."""
    from mvsformer_amd import ops
    N, Cin, Cout, H, W, KS, S, P = 1, 8, 8, 256, 320, 3, 1, 1
    x, w, dy = _conv2d_inputs(11, N, Cin, Cout, H, W, KS, S, P)
    _, _, dw = _conv2d_ref(x, w, dy, S, P, torch.float64)
    _, _, dw32 = _conv2d_ref(x, w, dy, S, P, torch.float32)
    check(ops.conv2d_wgrad_x3(dy.to(dev), x.to(dev), KS, S, P), dw, 5e-5, "dW", torch32=dw32)


@pytest.mark.parametrize("idx", [0, 3, 7, 15, 17])
def test_conv2d_fn_autograd(dev, idx):
    from mvsformer_amd.fpn import Conv2dFn
    why, N, Cin, Cout, H, W, KS, S, P = CONV2D_CASES[idx]
    x, w, dy = _conv2d_inputs(100 + idx, N, Cin, Cout, H, W, KS, S, P)
    y, dx, dw = _conv2d_ref(x, w, dy, S, P, torch.float64)
    xm, wm = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    ym = Conv2dFn.apply(xm, wm, S, P)
    (ym * dy.to(dev)).sum().backward()
    check(ym, y, 2e-5, "y")
    check(xm.grad, dx, 5e-5, "dX")
    check(wm.grad, dw, 5e-5, "dW")


# (N, Cin, Cout, h, w): ConvTranspose2d 4x4/s2/p1 - the ViT decoder's and FPNDecoderV2's upsamplings
CONVT_CASES = [(1, 8, 3, 1, 1), (2, 24, 8, 1, 5), (1, 64, 24, 3, 1), (2, 8, 8, 5, 7), (1, 3, 1, 9, 3), (2, 64, 64, 4, 6)]


@pytest.mark.parametrize("N,Cin,Cout,h,w", CONVT_CASES)
def test_convt2d_fn_autograd(dev, N, Cin, Cout, h, w):
    from mvsformer_amd.vit import ConvT2dFn
    gen = torch.Generator().manual_seed(N + Cin + Cout + h + w)
    x = randn(gen, N, Cin, h, w)
    wt = randn(gen, Cin, Cout, 4, 4) / (4 * Cin) ** 0.5
    dy = randn(gen, N, Cout, 2 * h, 2 * w)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    y = F.conv_transpose2d(xr, wr, None, stride=2, padding=1)
    assert y.shape == dy.shape
    dx, dw = torch.autograd.grad(y, (xr, wr), dy.double())
    xm, wm = x.to(dev).requires_grad_(True), wt.to(dev).requires_grad_(True)
    ym = ConvT2dFn.apply(xm, wm, 2, 1)
    (ym * dy.to(dev)).sum().backward()
    check(ym, y, 2e-5, "y")
    check(xm.grad, dx, 5e-5, "dX")
    check(wm.grad, dw, 5e-5, "dW")


# h, w from 1, 2, 3, 17, 129 (2w = 258 > 256: a second block in x of the forward kernel), square and not; w = 257: the BACKWARD kernel has
# one thread per input column, so only there does it take a second block in x
UPSAMPLE_HW = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (3, 17), (17, 3), (17, 17), (1, 129), (129, 1), (2, 129), (129, 3), (17, 129), (129, 129),
               (1, 257), (3, 257)]


def _up64(x, dtype=torch.float64):
    return F.interpolate(x.to(dtype), scale_factor=2, mode="bilinear", align_corners=True)


@pytest.mark.parametrize("with_lateral", [True, False])
@pytest.mark.parametrize("h,w", UPSAMPLE_HW)
def test_upsample2x_add_and_bwd_direct(dev, h, w, with_lateral):
    """``wide``: the kernel (like ATen) forms the source coordinate ``dst * (in-1)/(out-1)`` in fp32, so at 129 source pixels the
    interpolation weight carries up to 128 * 2^-24 = 7.6e-6 of rounding, and already 1e-6 at 17 pixels.  torch's fp32 CPU interpolate
    measured against fp64 on these inputs: 6.1e-6 forward / 6.5e-6 backward at 129x129, 1.3e-6 / 9.1e-7 at 3x17 - so the bound is
    4 x torch's error at every size above a handful of pixels, 1e-6 below."""
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(1000 * h + w)
    x = randn(gen, 2, 3, h, w)
    lat = randn(gen, 2, 3, 2 * h, 2 * w) if with_lateral else None
    g = randn(gen, 2, 3, 2 * h, 2 * w)
    want = _up64(x) + (lat.double() if with_lateral else 0.0)
    w32 = _up64(x, torch.float32) + (lat if with_lateral else 0.0)
    xm, gm = x.to(dev), g.to(dev)
    ym = ops.upsample2x_add(xm, lat.to(dev) if with_lateral else None)
    check(ym, want, 1e-6, "y", torch32=w32)
    # backward against fp64 autograd
    xr = x.double().requires_grad_(True)
    (dx,) = torch.autograd.grad(_up64(xr), xr, g.double())
    x32 = x.clone().requires_grad_(True)
    (dx32,) = torch.autograd.grad(_up64(x32, torch.float32), x32, g)
    dxm = ops.upsample2x_bwd(gm)
    check(dxm, dx, 1e-6, "dx", torch32=dx32)
    # adjoint identity <U x, g> == <x, U^T g>, in fp64 on the kernel's outputs.  Bound: every output element is ~6 fp32 operations
    # (2^-24 each, < 4e-7 if all errors lined up) of its terms' magnitude -> 1e-6 of sum |U x| |g|.
    ux = ops.upsample2x_add(xm, None).double().cpu()
    lhs = (ux * g.double()).sum().item()
    rhs = (x.double() * dxm.double().cpu()).sum().item()
    bound = 1e-6 * (ux.abs() * g.double().abs()).sum().item()
    print("adjoint: |lhs - rhs| = %.3e (bound %.3e)" % (abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


@pytest.mark.parametrize("h,w", [(1, 1), (3, 17), (17, 129), (129, 2)])
def test_upsample_add_fn_autograd(dev, h, w):
    from mvsformer_amd.fpn import UpsampleAddFn
    gen = torch.Generator().manual_seed(7 * h + w)
    x, lat, g = randn(gen, 1, 5, h, w), randn(gen, 1, 5, 2 * h, 2 * w), randn(gen, 1, 5, 2 * h, 2 * w)
    xr, lr = x.double().requires_grad_(True), lat.double().requires_grad_(True)
    y = _up64(xr) + lr
    dx, dl = torch.autograd.grad(y, (xr, lr), g.double())
    x32, l32 = x.clone().requires_grad_(True), lat.clone().requires_grad_(True)
    y32 = _up64(x32, torch.float32) + l32
    (dx32,) = torch.autograd.grad(y32, x32, g)
    xm, lm = x.to(dev).requires_grad_(True), lat.to(dev).requires_grad_(True)
    ym = UpsampleAddFn.apply(xm, lm)
    (ym * g.to(dev)).sum().backward()
    check(ym, y, 1e-6, "y", torch32=y32)
    check(xm.grad, dx, 1e-6, "dx", torch32=dx32)
    assert torch.equal(lm.grad.cpu(), g)                      # the lateral branch's gradient is dy itself


ELEMS = [1, 3, 4, 5, 1023, 1024, 1025]                        # the 4-wide vector body and the scalar tail of the elementwise kernels


@pytest.mark.parametrize("n", ELEMS)
def test_ewise_mul_and_mul_fn(dev, n):
    from mvsformer_amd import ops
    from mvsformer_amd.vit import MulFn
    gen = torch.Generator().manual_seed(n)
    a, b, g = randn(gen, n), randn(gen, n), randn(gen, n)
    out = ops.ewise_mul(a.to(dev), b.to(dev))
    check(out, a.double() * b.double(), 1e-6, "a*b")
    assert torch.equal(out.cpu(), (a.double() * b.double()).float())      # an fp32 product is correctly rounded: every element, tail included
    am, bm = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    ym = MulFn.apply(am, bm)
    (ym * g.to(dev)).sum().backward()
    check(ym, a.double() * b.double(), 1e-6, "y")
    check(am.grad, g.double() * b.double(), 1e-6, "da")
    check(bm.grad, g.double() * a.double(), 1e-6, "db")


@pytest.mark.parametrize("n", ELEMS)
def test_bias_fn(dev, n):
    from mvsformer_amd.fpn import BiasFn
    gen = torch.Generator().manual_seed(50 + n)
    x, bias, g = randn(gen, 2, 3, 1, n), randn(gen, 3), randn(gen, 2, 3, 1, n)
    xm, bm = x.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    ym = BiasFn.apply(xm, bm)
    (ym * g.to(dev)).sum().backward()
    check(ym, x.double() + bias.double().view(1, 3, 1, 1), 1e-6, "y")
    assert torch.equal(xm.grad.cpu(), g)
    check(bm.grad, g.double().sum(dim=(0, 2, 3)), 1e-6, "dbias")


def test_bad_arguments_are_refused_before_any_launch(dev):
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    x = torch.zeros(1, 3, 4, 4, device=dev)
    with pytest.raises(MvsHipError):
        ops.conv2d_fwd_x3(x, torch.zeros(8, 3, 3, 3, device=dev), 3, 1)          # stride 3 is not built
    with pytest.raises(MvsHipError):
        ops.ewise_mul(torch.zeros(4, device=dev), torch.zeros(5, device=dev))
    with pytest.raises(MvsHipError):
        ops.upsample2x_add(x.cpu(), None)
