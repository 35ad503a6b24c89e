"""The small training kernels of ``csrc/train.hip`` and ``csrc/bf16_head.hip`` on their own, against float64 on fresh seeded inputs, at the
sizes where their launches change: one element, one short of / exactly / one past a 256-thread block (a 1024-voxel block of the bf16 head
backward, a 4-wide vector of ``ewise_mul``, a 64-pixel tile of the layout transpose) and, for ``mvs_prob1_bwd``, more voxels than its capped
grid covers in one trip.  Bounds are the float32 (bfloat16) rounding of the operations each kernel performs, written next to each test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24                          # half an ulp of 1 in float32: the relative error of one rounded operation


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("HW", [1, 255, 257])
@pytest.mark.parametrize("D", [1, 3, 48])
def test_softmax_bwd(dev, D, HW, B):
    """dpre = p (dp - sum_d dp p).  The dot product is a chain of D fused multiply-adds (<= D eps sum|dp p|), then one subtraction and one
    product: |error| <= (D + 4) eps p (sum|dp p| + |dp|)."""
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(D * 1000 + HW + B)
    p = torch.softmax(torch.randn(B, D, 1, HW, generator=gen) * 2, 1)
    dp = torch.randn(B, D, 1, HW, generator=gen)
    got = ops.softmax_bwd(p.to(dev), dp.to(dev)).cpu().double()
    p64, dp64 = p.double(), dp.double()
    want = p64 * (dp64 - (dp64 * p64).sum(1, keepdim=True))
    bound = (D + 4) * EPS * p64 * ((dp64 * p64).abs().sum(1, keepdim=True) + dp64.abs())
    assert got.shape == want.shape and ((got - want).abs() <= bound).all(), ((got - want).abs() / bound.clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("B,N", [(2, 135),                  # below the cap of 512 / B blocks: one trip of the grid-stride loop
                                 (1, 512 * 256 + 77),       # prob1_bwd grid-stride loop: 513 chunks on 512 blocks, block 0 alone makes a second, ragged trip
                                 (3, 171 * 256 + 5)])       # prob1_bwd grid-stride loop: the cap is ceil(512 / 3) = 171 blocks per batch entry, 5 voxels left over
@pytest.mark.parametrize("C", [1, 8, 16])
def test_prob1_bwd(dev, C, B, N):
    """dx = w[c] dl: one product, |error| <= 2 eps |dx|.  dw[c] = sum dl x[c] and dbias = sum dl: 1e-5 of sum |terms|.  The block sums reach
    dw | dbias through float atomics, whose order is not fixed, so two runs agree within that bound but need not be bitwise equal."""
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(C * 31 + B)
    x = torch.randn(B, C, 1, 1, N, generator=gen)
    w = torch.randn(C, generator=gen)
    dl = torch.randn(B, 1, 1, 1, N, generator=gen)
    xd, wd, dld = x.to(dev), w.to(dev), dl.to(dev)
    dx, dwb = ops.prob1_bwd(xd, wd, dld)
    dx2, dwb2 = ops.prob1_bwd(xd, wd, dld)
    want_dx = w.double().view(1, C, 1, 1, 1) * dl.double()
    assert dx.shape == x.shape and ((dx.cpu().double() - want_dx).abs() <= 2 * EPS * want_dx.abs()).all()
    assert torch.equal(dx, dx2)
    terms = torch.cat([(dl.double() * x.double()).permute(1, 0, 2, 3, 4).reshape(C, -1), dl.double().reshape(1, -1)], 0)      # [C + 1, B N]
    want, scale = terms.sum(1), terms.abs().sum(1)
    assert dwb.shape == (C + 1,)
    assert ((dwb.cpu().double() - want).abs() <= 1e-5 * scale).all(), ((dwb.cpu().double() - want).abs() / scale).max().item()
    assert ((dwb2.cpu().double() - want).abs() <= 1e-5 * scale).all()
    assert ((dwb.cpu().double() - dwb2.cpu().double()).abs() <= 1e-5 * scale).all()


def test_prob1_bwd_refuses_17_channels(dev):
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    with pytest.raises(MvsHipError):
        ops.prob1_bwd(torch.zeros(1, 17, 1, 1, 8, device=dev), torch.zeros(17, device=dev), torch.zeros(1, 1, 1, 1, 8, device=dev))


NS = [1, 3, 4, 5, 1023, 1024, 1025]      # below / at / past a 4-wide vector and a 1024-element block of ewise_mul, a 256-thread block of the others


@pytest.mark.parametrize("n", NS)
def test_sigmoid_fwd_bwd(dev, n):
    """y = 1 / (1 + exp(-x)): exp within 2 ulps, one addition, one division, each half an ulp -> 4 ulps = 8 eps relative.
    dx = dy y (1 - y): three rounded operations, 4 eps relative."""
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=gen) * 4.0
    y = ops.sigmoid(x.to(dev))
    want = torch.sigmoid(x.double())
    assert y.shape == x.shape and ((y.cpu().double() - want).abs() <= 8 * EPS * want).all()
    dy = torch.randn(n, generator=gen)
    dx = ops.sigmoid_bwd(y, dy.to(dev)).cpu().double()
    y64 = y.cpu().double()                                   # the backward's input is the float32 y it is given
    want = dy.double() * y64 * (1 - y64)
    assert ((dx - want).abs() <= 4 * EPS * want.abs()).all()


@pytest.mark.parametrize("n", NS)
def test_ewise_mul(dev, n):
    """One rounded product per element: half an ulp from the float64 product, and bit for bit the IEEE float32 product."""
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(n)
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    got = ops.ewise_mul(a.to(dev), b.to(dev)).cpu()
    want = a.double() * b.double()
    assert got.shape == a.shape and ((got.double() - want).abs() <= EPS * want.abs()).all()
    assert torch.equal(got, a * b)


@pytest.mark.parametrize("HW", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("C", [8, 16, 32, 64])             # every instantiation of nhwc_to_nchw_kernel
def test_nhwc_to_nchw(dev, C, HW):
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(C + HW)
    x = torch.randn(1, 3, 1, HW, C, generator=gen)
    got = ops.to_channels_first(x.to(dev)).cpu()
    assert torch.equal(got, x.permute(0, 1, 4, 2, 3).contiguous())


@pytest.mark.parametrize("N", [1, 255, 257])
def test_bf16_embed_ch0(dev, N):
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(N)
    x = torch.randn(N, generator=gen) * 3.0
    got = ops.bf16_embed_ch0(x.to(dev)).cpu()
    assert got.shape == (N, 8) and got.dtype == torch.bfloat16
    assert torch.equal(got[:, 0], x.to(torch.bfloat16))
    assert (got[:, 1:] == 0).all()


@pytest.mark.parametrize("sigmoid", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("N", [1, 255, 256, 257,            # around a 256-voxel block of the forward
                               1023, 1024,
                               1025,                        # bf16_head_bwd ragged last block: 1 voxel in the second 1024-voxel block
                               4099])                       # bf16_head_bwd ragged last block: 5 blocks, 3 voxels in the last one
def test_bf16_head_fwd_bwd(dev, N, with_w, with_bias, sigmoid):
    """out = act(sum_c w[c] x[c] + bias) on bf16 channel-last voxels and its backward.  bf16 values are exact in float64, so the reference is
    the float64 dot product of the very same values.

    Forward without sigmoid: 1e-6 of the sum of the absolute terms, sum_c |w x| + |bias| (the bias is one of the added terms: with the
    channel-0 select and |x0| << |bias| the rounding of the one addition is relative to the bias).
    Forward with sigmoid (the kernel uses the fast exponential): 4 x the deviation of a float32 torch.sigmoid of the float64 pre-activation
    from the float64 sigmoid, with a floor of 4 float32 ulps of 1 (4.8e-7).  Measured over these cases: float32 torch.sigmoid deviates by
    up to 8.8e-8 (4 x = 3.5e-7, so the floor is the bound); the HIP forward's deviation has not been measured on a device yet - the test
    prints both per case (run with -s) before it asserts.
    dx: one bf16 rounding of the float64 value, |error| <= 2^-8 |want|.  dwb = [dw | dbias]: 1e-5 of sum |terms|, and bitwise equal
    between two runs - the per-block partial rows are added in a fixed order."""
    from mvsformer_amd import ops
    gen = torch.Generator().manual_seed(N * 8 + 4 * with_w + 2 * with_bias + sigmoid)
    x = torch.randn(N, 8, generator=gen).to(torch.bfloat16)
    w = torch.randn(8, generator=gen) if with_w else None
    bias = torch.randn(1, generator=gen) if with_bias else None
    xd = x.to(dev)
    wd, bd = (None if v is None else v.to(dev) for v in (w, bias))
    w64 = w.double() if with_w else torch.tensor([1.0] + [0.0] * 7, dtype=torch.float64)
    b64 = bias.double() if with_bias else torch.zeros(1, dtype=torch.float64)
    terms = x.double() * w64
    pre, scale = terms.sum(1) + b64, terms.abs().sum(1) + b64.abs()

    out = ops.bf16_head_fwd(xd, wd, bd, sigmoid)
    assert out.shape == (N,) and out.dtype == torch.float32
    got = out.cpu().double()
    if sigmoid:
        want = torch.sigmoid(pre)
        dev32 = (torch.sigmoid(pre.float()).double() - want).abs().max().item()
        tol = max(4 * dev32, 4 * 2.0 ** -23)
        print("bf16 head sigmoid N=%d: HIP deviation %.3e, float32 torch.sigmoid deviation %.3e, bound %.3e" % (N, (got - want).abs().max().item(), dev32, tol))
        assert (got - want).abs().max().item() <= tol
    else:
        assert ((got - pre).abs() <= 1e-6 * scale).all(), ((got - pre).abs() / scale.clamp_min(1e-300)).max().item()

    dout = torch.randn(N, generator=gen)
    dd = dout.to(dev)
    dx, dwb = ops.bf16_head_bwd(xd, wd, out if sigmoid else None, dd)
    dx2, dwb2 = ops.bf16_head_bwd(xd, wd, out if sigmoid else None, dd)
    dl = dout.double() * (got * (1 - got) if sigmoid else 1.0)                # from the float32 y the backward is given
    want_dx = dl.unsqueeze(1) * w64
    assert dx.shape == (N, 8) and dx.dtype == torch.bfloat16
    assert ((dx.cpu().double() - want_dx).abs() <= 2.0 ** -8 * want_dx.abs()).all()
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16))
    if not with_w:
        assert dwb is None and dwb2 is None                                  # the channel-0 select has no parameters
        return
    t = torch.cat([dl.unsqueeze(1) * x.double(), dl.unsqueeze(1)], 1)         # [N, 9]
    want, tscale = t.sum(0), t.abs().sum(0)
    assert dwb.shape == (9,)
    assert ((dwb.cpu().double() - want).abs() <= 1e-5 * tscale).all(), ((dwb.cpu().double() - want).abs() / tscale).max().item()
    assert torch.equal(dwb.view(torch.int32), dwb2.view(torch.int32))
