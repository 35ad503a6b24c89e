"""Case tables, float64 references, error bounds and mutation helpers for the bf16 training convolutions of ``csrc/bf16_train.hip``
(``bf16_conv_kernel`` with its fused statistics forms, ``bf16_wgrad_kernel`` + ``bf16_wgrad_reduce_kernel``).  No GPU code: used by
``tests/test_hip_bf16_conv_edges.py`` (MI355X) and checked by ``tests/test_bf16_conv_edge_refs.py`` (CPU).

Operands.  Every input is drawn in fp32 and rounded to bf16 first, so the device and the reference see identical operands; the reference
is ``torch.nn.functional.conv3d`` / ``conv_transpose3d`` in float64 (plain float64 sums for the weight gradient).

Bounds, per element (u32 = 2^-24, ubf = 2^-8 the unit roundoffs of fp32 / bf16, C_ACC = 2):

* fp32 accumulation.  The kernel forms acc = sum of K products of bf16 numbers (each exact in fp32) in some order, in fp32.  Any summation
  order of K terms t_i commits at most K - 1 roundings, each at most u32 times a partial sum, which is at most S = sum |t_i|:
  |acc - ref| <= gamma_{K-1} S <= K u32 S =: E0 (Higham, Accuracy and Stability of Numerical Algorithms, 4.2).  S is the float64 convolution
  of |x| with |w|; K = 27 Cin, 9 Cin for the 2-D kernel, Cin times the taps that exist for the voxel's parities in the transposed form
  (1 per even, 2 per odd coordinate of a strided axis, 3 per unstrided axis - the taps the kernel walks).
* bf16 output.  got = rn_bf16(v) with |v - ref| <= E: |got - ref| <= ubf |v| + E <= ubf |ref| + (1 + ubf) E.  The bound used is
  ubf |ref| + C_ACC E: C_ACC = 2 covers the (1 + ubf) and leaves a factor of ~2 for a matrix core that adds the products of one
  instruction with another internal rounding than a chain of IEEE additions.
* epilogue, in the order of ``bf16_conv_kernel``: v1 = fmaf(acc, scale, shift) - one rounding of a value of size at most |ref_acc scale| +
  |shift| (+ the propagated error): E1 = |scale| E0 + u32 (|ref_acc scale| + |shift|); the ReLU is 1-Lipschitz: E2 = E1; v3 = v2 + residual
  is one more fp32 addition: E3 = E2 + u32 (|ref_v2| + |residual|); then the bf16 rounding as above.  (Second-order terms u32 E are inside C_ACC.)
* fp32 ``dW``: only the accumulation term, C_ACC K u32 S with K = the voxels summed (batch x Dp x Hp x Wp) and S = sum |A| |Bt|.  Where S is 0 -
  the tap's window lies outside ``Bt`` for every voxel that has a non-zero ``A`` - the bound is 0: the entry must be exactly 0.  K counts
  the voxels whose ``A`` is non-zero (a zero term adds an exact zero).  Integer operands whose sum of |products| stays below 2^24 make
  every fp32 operation exact: bound 0 everywhere (the one case of 66 560 voxels, where K u32 S of random data would exceed |dW|).
* sums (``bf16_conv3d_stats``, ``stats4`` of ``bf16_conv3d_bn_fwd``, ``sums`` of ``bf16_conv3d_bnbwd``) are compared with float64 sums over the
  DEVICE'S OWN bf16 output (the kernel sums what it rounded): C_ACC K u32 sum|terms|.  The forward statistics are fp32 only up to a row of at
  most 256 voxels (one work item of 64, or one block of four) and added in double from there: K = SUM_CHAIN = 256.  The backward sums
  stay fp32 to the end: K = the voxels of one (group, channel), + 3 for the roundings inside a term g (y - mean) invstd.
  ``stats4`` and the running statistics follow from the sums by ``mvsbn::finalize`` / ``running_update`` in double; their bounds
  propagate the sums' bounds through those formulas (exact interval ends for 1/sqrt) plus u32 per fp32 rounding (``finalize_expect``); a
  running-statistics update (1 - m) r + m v in fp32 rounds 1 - m, both products and the sum, v itself was rounded to fp32: 6 u32 of the
  two products' sizes covers those 4.5.
* ReLU mask of ``bnbwd``: ``fmaf(bn_y, scale, shift) > 0`` in fp32.  ``nice_bn4`` draws scale from {+-0.5, +-1, +-2}, shift, mean in multiples
  of 1/8 and invstd from {0.5, 1, 2}; with bn_y in bf16 that fmaf is exact, so the reference decides every mask bit identically - no element
  is excluded - and ~5 % of the pre-activations are planted at exactly 0 (they must mask to 0)."""
import collections
import functools
import itertools

import torch
import torch.nn.functional as F

import conv_plan_reader

U32 = 2.0 ** -24
UBF = 2.0 ** -8
C_ACC = 2.0
SUM_CHAIN = 256
OLD_RTOL = 1e-2                 # the criterion of test_conv_bf16_fn / test_deconv_bf16_fn: max|err| / max|want| < 1e-2
_CONSTS = conv_plan_reader.fields("bf16_consts")
KSPLIT_ITEMS, WG_PW = _CONSTS["KSPLIT_ITEMS"], _CONSTS["WG_PW"]      # the largest launch that splits K; patch columns of the weight gradient


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def to_cl(x):
    """fp32 ``[B,C,D,H,W]`` (bf16-representable) -> bf16 channel-last ``[B,D,H,W,C]``."""
    return x.permute(0, 2, 3, 4, 1).contiguous().to(torch.bfloat16)


def from_cl(y):
    """channel-last ``[B,D,H,W,C]`` (any dtype, any device) -> float64 ``[B,C,D,H,W]`` on the CPU."""
    return y.detach().cpu().double().permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------------------------------------------------------- the plans
ConvPlan = collections.namedtuple("ConvPlan", "Do Ho Wo wpar nwchunks items_per_sample items ksplit block_rows samples rows_per_sample")


def plan_conv(B, Cin, Di, Hi, Wi, gather, sd, shw, taps=27, groups=1):
    """``mvsplan::conv_plan`` of csrc/bf16_conv_plan.h, asked of the header itself (tests/conv_plan_tool.cpp)."""
    return conv_plan_reader.plan(ConvPlan, "bf16_conv", B, Cin, Di, Hi, Wi, gather, sd, shw, taps, groups)


WgradPlan = collections.namedtuple("WgradPlan", "PH npr npc npatch dseg nseg TA TB gy blocks")


def plan_wgrad(nbatch, CA, CB, Dp, Hp, Wp, shw):
    """``mvsplan::wgrad_plan`` for a layer of its own (not grouped)."""
    return conv_plan_reader.plan(WgradPlan, "bf16_wgrad", nbatch, CA, CB, Dp, Hp, Wp, shw, 0)


# ------------------------------------------------------------------------------------------------------------------- convolution cases
ConvCase = collections.namedtuple("ConvCase", "name B cin cout gather stride D H W taps scale relu residual")


def _cc(name, B, cin, cout, gather, stride, D, H, W, taps=27, scale=False, relu=False, residual=False):
    return ConvCase(name, B, cin, cout, gather, stride, D, H, W, taps, scale, relu, residual)


_DH = [(1, 1), (2, 3), (3, 2), (1, 3), (3, 1), (2, 2), (3, 3), (1, 2), (2, 1)]
STRIDES = [(1, 1), (1, 2), (2, 2)]


def _row_chunk_cases():
    """1. Conv3d, Wo in {1, 15, 16, 17, 63, 64, 65, 129}; stride 2: the odd and the even Wi of the same Wo; D, H cycle through {1, 2, 3}^2."""
    out, k = [], 0
    for stride in STRIDES:
        for Wo in (1, 15, 16, 17, 63, 64, 65, 129):
            for Wi in ([Wo] if stride[1] == 1 else [2 * Wo - 1, 2 * Wo]):
                D, H = _DH[k % len(_DH)]
                B = 1 if k % 3 else 2
                cin, cout = ((8, 8), (8, 16), (16, 8))[k % 3]
                out.append(_cc("row-s%d%d-w%d-d%dh%d-b%d-c%d_%d" % (stride + (Wi, D, H, B, cin, cout)), B, cin, cout, 0, stride, D, H, Wi))
                k += 1
    return out


def _parity_cases():
    """2. ConvTranspose3d, Wi in {1, 31, 32, 33, 63, 64, 65}: Wo = 2 .. 130 crosses the 128-column chunk."""
    out, k = [], 0
    for stride in STRIDES[1:]:
        for Wi in (1, 31, 32, 33, 63, 64, 65):
            D, H = _DH[(k + 1) % len(_DH)]
            B = 2 if k % 3 else 1
            cin, cout = ((16, 8), (8, 8), (8, 16))[k % 3]
            out.append(_cc("par-s%d%d-w%d-d%dh%d-b%d-c%d_%d" % (stride + (Wi, D, H, B, cin, cout)), B, cin, cout, 1, stride, D, H, Wi))
            k += 1
    return out


def _instance_cases():
    """3. every <CIN, NT, GATHER, SD, SHW, KSPLIT> instance ``launch_conv`` dispatches, and the two ``taps = 9`` ones.  ``inst-``: one
    chunk-crossing row shape per gather and stride, B = 1 (Cin >= 32 runs K-split there: at most 16 items).  ``inst4-``: Cin >= 32 with more
    than 768 items, the four-items-per-block instances - narrow rows (Wo <= 6), so that 780 .. 800 items stay a few thousand voxels:
        gather 0 (1,1): [2, 3, 130, 5]          Do Ho nwchunks B = 3 * 130 * 1 * 2 = 780
        gather 0 (1,2): [2, 3, 259, 5]          3 * 130 * 1 * 2 = 780          gather 0 (2,2): [2, 5, 259, 5]     3 * 130 * 1 * 2 = 780
        gather 1 (1,2): [2, 4, 25, 3]           4 * 50 * 1 * 2 parities * 2 = 800      gather 1 (2,2): [2, 2, 25, 3]      4 * 50 * 2 * 2 = 800
        gather 1 (1,1): [2, 3, 130, 5]          780"""
    out = []
    big = {(0, (1, 1)): (3, 130, 5), (0, (1, 2)): (3, 259, 5), (0, (2, 2)): (5, 259, 5),
           (1, (1, 1)): (3, 130, 5), (1, (1, 2)): (4, 25, 3), (1, (2, 2)): (2, 25, 3)}
    for gather, stride in itertools.product((0, 1), STRIDES):
        W = 65 if (gather == 1 and stride[1] == 2) else 65 * stride[1]
        for cin, cout in itertools.product((8, 16, 32, 64), repeat=2):
            out.append(_cc("inst-g%d-s%d%d-c%d_%d" % ((gather,) + stride + (cin, cout)), 1, cin, cout, gather, stride, 2, 2, W))
        for cin, cout in itertools.product((32, 64), (16, 32, 64)):
            D, H, Wn = big[(gather, stride)]
            out.append(_cc("inst4-g%d-s%d%d-c%d_%d" % ((gather,) + stride + (cin, cout)), 2, cin, cout, gather, stride, D, H, Wn))
    for cin, cout in itertools.product((8, 16), repeat=2):
        out.append(_cc("inst-2d-c%d_%d" % (cin, cout), 2, cin, cout, 0, (1, 1), 3, 3, 65, taps=9))
    return out


def _epilogue_cases():
    """5. scale/shift, relu, residual alone and together, one shape of each gather."""
    out = []
    for gather, stride, W in ((0, (1, 1), 65), (1, (2, 2), 33)):
        for scale, relu, residual in itertools.product((False, True), repeat=3):
            if scale or relu or residual:
                name = "epi-g%d-%s" % (gather, "+".join(n for n, f in (("affine", scale), ("relu", relu), ("res", residual)) if f))
                out.append(_cc(name, 2, 16, 16, gather, stride, 2, 3, W, 27, scale, relu, residual))
    return out


CONV_CASES = _row_chunk_cases() + _parity_cases() + _instance_cases() + _epilogue_cases()
CONV_CASE = {c.name: c for c in CONV_CASES}
assert len(CONV_CASE) == len(CONV_CASES)

# 4. K split on both sides of its threshold, same data.  conv_plan of [2, 3, 129, 5, Cin] at stride 1: Do Ho Wo = 3, 129, 5; nwchunks =
# (5 + 63) / 64 = 1; items_per_sample = 3 * 129 * 1 = 387; items = 774 > 768 -> four items per block, 774 % 4 = 2 (two idle wavefronts in
# the last block); each sample alone: 387 <= 768 -> K split.
KSPLIT_CASES = [_cc("ksplit-c%d" % cin, 2, cin, 16, 0, (1, 1), 3, 129, 5) for cin in (32, 64)]


def out_dims(c):
    p = plan_conv(c.B, c.cin, c.D, c.H, c.W, c.gather, c.stride[0], c.stride[1], c.taps)
    return p.Do, p.Ho, p.Wo


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


def _wshape(c):
    k = (3, 3, 3) if c.taps == 27 else (3, 3)
    return ((c.cout, c.cin) if c.gather == 0 else (c.cin, c.cout)) + k


@functools.lru_cache(maxsize=None)
def conv_inputs(name_or_case):
    """CPU fp32 inputs of a case, all bf16-representable where the kernel takes bf16 (shared, never modified): ``x [B,cin,D,H,W]``, ``w`` as
    the module holds it (``[cout,cin,3,3,3]``, 2-D ``[cout,cin,3,3]``, transposed ``[cin,cout,3,3,3]``), ``scale, shift [cout]`` fp32,
    ``residual [B,cout,Do,Ho,Wo]``."""
    c = CONV_CASE[name_or_case] if isinstance(name_or_case, str) else name_or_case
    g = _gen(c.name)
    x = bf(torch.randn(c.B, c.cin, c.D, c.H, c.W, generator=g))
    w = bf(torch.randn(_wshape(c), generator=g) / (c.taps * c.cin) ** 0.5)
    Do, Ho, Wo = out_dims(c)
    scale = (torch.rand(c.cout, generator=g) + 0.5) * torch.where(torch.rand(c.cout, generator=g) < 0.3, -1.0, 1.0)
    shift = torch.randn(c.cout, generator=g) * 0.5
    residual = bf(torch.randn(c.B, c.cout, Do, Ho, Wo, generator=g))
    return dict(x=x, w=w, scale=scale, shift=shift, residual=residual)


# ------------------------------------------------------------------------------------------------------------------- convolution reference
def conv_raw(x, w, gather, stride, taps, dtype):
    """The raw convolution in ``dtype``: Conv3d k3 p1 (``taps`` = 9: the 2-D kernel on every depth plane) or ConvTranspose3d k3 p1
    output_padding stride - 1."""
    x, w = x.to(dtype), w.to(dtype)
    s3 = (stride[0], stride[1], stride[1])
    if taps == 9:
        return F.conv3d(x, w.unsqueeze(2), None, stride=1, padding=(0, 1, 1))
    if gather == 0:
        return F.conv3d(x, w, None, stride=s3, padding=1)
    return F.conv_transpose3d(x, w, None, stride=s3, padding=1, output_padding=(s3[0] - 1, s3[1] - 1, s3[2] - 1))


def conv_terms(c):
    """K per output voxel ``[1,1,Do,Ho,Wo]`` float64: the products one output sums (module docstring)."""
    Do, Ho, Wo = out_dims(c)
    if c.gather == 0:
        return torch.full((1, 1, Do, Ho, Wo), float(c.taps * c.cin), dtype=torch.float64)

    def axis(n, s):
        return torch.full((n,), 3.0, dtype=torch.float64) if s == 1 else 1.0 + (torch.arange(n) % 2).double()
    kd, kh, kw = axis(Do, c.stride[0]), axis(Ho, c.stride[1]), axis(Wo, c.stride[1])
    return (c.cin * kd.view(-1, 1, 1) * kh.view(1, -1, 1) * kw.view(1, 1, -1)).view(1, 1, Do, Ho, Wo)


def epilogue(acc, e0, scale=None, shift=None, relu=False, residual=None):
    """The epilogue of ``bf16_conv_kernel`` on the reference ``acc`` with accumulation bound ``e0`` (both ``[B,C,...]``, one dtype) ->
    ``(value before the bf16 rounding, its error bound before C_ACC)``; per-channel ``scale, shift [C]``."""
    v, e = acc, e0
    if scale is not None:
        sc, sh = scale.to(acc.dtype).view(1, -1, 1, 1, 1), shift.to(acc.dtype).view(1, -1, 1, 1, 1)
        e = sc.abs() * e + U32 * ((acc * sc).abs() + sh.abs())
        v = acc * sc + sh
    if relu:
        v = v.clamp_min(0)
    if residual is not None:
        r = residual.to(acc.dtype)
        e = e + U32 * (v.abs() + r.abs())
        v = v + r
    return v, e


def bf16_bound(ref, e):
    return UBF * ref.abs() + C_ACC * e


def conv_eval(c, dtype=torch.float64, w=None):
    """The whole layer of case ``c`` (raw convolution + its epilogue) in ``dtype``, before the bf16 rounding; ``w`` replaces the weight."""
    t = conv_inputs(c)
    acc = conv_raw(t["x"], t["w"] if w is None else w, c.gather, c.stride, c.taps, dtype)
    return epilogue(acc, torch.zeros_like(acc), t["scale"] if c.scale else None, t["shift"] if c.scale else None, c.relu,
                    t["residual"] if c.residual else None)[0]


@functools.lru_cache(maxsize=None)
def conv_expect(name_or_case):
    """-> ``(ref, bound)`` float64 ``[B,cout,Do,Ho,Wo]`` of a case's bf16 output."""
    c = CONV_CASE[name_or_case] if isinstance(name_or_case, str) else name_or_case
    t = conv_inputs(c)
    acc = conv_raw(t["x"], t["w"], c.gather, c.stride, c.taps, torch.float64)
    S = conv_raw(t["x"].abs(), t["w"].abs(), c.gather, c.stride, c.taps, torch.float64)
    ref, e = epilogue(acc, conv_terms(c) * U32 * S, t["scale"] if c.scale else None, t["shift"] if c.scale else None, c.relu,
                      t["residual"] if c.residual else None)
    return ref, bf16_bound(ref, e)


def accumulation_term(name_or_case):
    """K u32 S of the raw convolution, ``[B,cout,Do,Ho,Wo]``: what two correct evaluations in different orders may differ by, twice."""
    c = CONV_CASE[name_or_case] if isinstance(name_or_case, str) else name_or_case
    t = conv_inputs(c)
    return conv_terms(c) * U32 * conv_raw(t["x"].abs(), t["w"].abs(), c.gather, c.stride, c.taps, torch.float64)


def bf16_half_ulp(v):
    """Half the spacing of bf16 at ``v`` (float64, 0 at 0): how far the fp32 value that rounded to ``v`` may have been from it."""
    e = torch.frexp(v.double())[1]                             # |v| in [2^(e-1), 2^e): ulp 2^(e-8)
    return torch.where(v == 0, torch.zeros_like(v, dtype=torch.float64), torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 9))


def share(got, ref, bound):
    """-> ``(max|got - ref|, max over ALL elements of |got - ref| / bound)``; an element whose bound is 0 must be exact."""
    err = (torch.as_tensor(got).detach().cpu().double() - ref).abs()
    bound = bound.expand_as(err)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return err.max().item(), ratio.max().item()


def inside(got, ref, bound):
    return share(got, ref, bound)[1] <= 1.0


def old_criterion(got, want):
    """The criterion the existing bf16 layer tests hold ``dW`` to."""
    want = want.double()
    return (torch.as_tensor(got).double() - want).abs().max().item() / max(want.abs().max().item(), 1e-12) < OLD_RTOL


# ------------------------------------------------------------------------------------------------------------------- fused statistics forms
StatCase = collections.namedtuple("StatCase", "name B groups cin cout gather stride D H W taps claim")

STAT_CASES = [
    StatCase("st-b1-items6", 1, 1, 8, 16, 0, (1, 1), 1, 3, 65, 27, "B = 1, 6 items: the last block has two idle wavefronts"),
    StatCase("st-b2-g1-ips3", 2, 1, 16, 8, 0, (1, 1), 1, 3, 20, 27, "one group, 3 items per sample: block 0 straddles the samples"),
    StatCase("st-b2-g2-ips4", 2, 2, 8, 16, 0, (1, 2), 2, 3, 33, 27, "two groups, 4 items per sample: one block row per sample"),
    StatCase("st-b4-g2-ksplit-ips3", 4, 2, 32, 32, 0, (1, 1), 1, 3, 9, 27, "two groups, K split, 3 items (= rows) per sample"),
    StatCase("st-transposed-wo130", 2, 2, 16, 8, 1, (1, 2), 1, 1, 65, 27, "transposed stride 2, Wo = 130: two 128-chunks x two parities"),
    StatCase("st-2d", 1, 1, 8, 16, 0, (1, 1), 2, 3, 33, 9, "taps = 9, 6 items"),
]
STAT_CASE = {c.name: c for c in STAT_CASES}
# groups = 2, four items per block, 3 items per sample: a block row would hold samples of both groups
REFUSED_CASE = StatCase("st-refused", 2, 2, 8, 8, 0, (1, 1), 1, 3, 20, 27, "refused")


def stat_plan(c):
    return plan_conv(c.B, c.cin, c.D, c.H, c.W, c.gather, c.stride[0], c.stride[1], c.taps, c.groups)


def nice_bn4(groups, cout, g):
    """``bn4 [4, groups*cout]`` = scale | shift | mean | invstd with values for which the mask and the terms are exact in fp32."""
    n = groups * cout
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)] * torch.where(torch.rand(n, generator=g) < 0.4, -1.0, 1.0)
    shift = torch.randint(-8, 9, (n,), generator=g).float() / 8
    mean = torch.randint(-4, 5, (n,), generator=g).float() / 8
    invstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=g)]
    return torch.stack([scale, shift, mean, invstd]).contiguous()


def per_sample(v, B, groups, cout):
    """``v [groups*cout]`` -> ``[B, cout, 1, 1, 1]``: sample b reads group b % groups."""
    return v.view(groups, cout)[torch.arange(B) % groups].view(B, cout, 1, 1, 1)


@functools.lru_cache(maxsize=None)
def stat_inputs(name):
    """Inputs of a statistics case: the convolution's (``x, w``, as ``conv_inputs``), ``residual`` / ``addend`` (output shape), the
    BatchNorm parameters of ``bn_fwd`` and ``bn_y, bn4`` of ``bnbwd`` (channels-first fp32; ``bn_y`` has ~5 % of its pre-activations
    ``bn_y scale + shift`` at exactly 0)."""
    c = REFUSED_CASE if name == REFUSED_CASE.name else STAT_CASE[name]
    g = _gen(c.name)
    cc = _cc(c.name, c.B, c.cin, c.cout, c.gather, c.stride, c.D, c.H, c.W, c.taps)
    x = bf(torch.randn(c.B, c.cin, c.D, c.H, c.W, generator=g))
    w = bf(torch.randn(_wshape(cc), generator=g) / (c.taps * c.cin) ** 0.5 * 2.0)
    Do, Ho, Wo = out_dims(cc)
    oshape = (c.B, c.cout, Do, Ho, Wo)
    residual = bf(torch.randn(oshape, generator=g))
    gamma, beta = torch.rand(c.cout, generator=g) + 0.5, torch.randn(c.cout, generator=g)
    rm, rv = torch.randn(c.cout, generator=g), torch.rand(c.cout, generator=g) + 0.5
    bn4 = nice_bn4(c.groups, c.cout, g)
    bn_y = bf(torch.randn(oshape, generator=g))
    sc, sh = per_sample(bn4[0], c.B, c.groups, c.cout), per_sample(bn4[1], c.B, c.groups, c.cout)
    zero_at = torch.rand(oshape, generator=g) < 0.05
    bn_y = torch.where(zero_at, (-sh / sc).expand(oshape), bn_y)
    assert torch.equal(bf(bn_y), bn_y)
    return dict(case=cc, x=x, w=w, residual=residual, addend=residual, gamma=gamma, beta=beta, running_mean=rm, running_var=rv,
                momentum=0.1, eps=1e-5, bn4=bn4, bn_y=bn_y, zero_at=zero_at)


@functools.lru_cache(maxsize=None)
def stat_conv_expect(name, addend=False):
    """``(ref, bound)`` of the raw convolution of a statistics case [+ ``addend``, one fp32 addition before the rounding]."""
    t = stat_inputs(name)
    c = t["case"]
    acc = conv_raw(t["x"], t["w"], c.gather, c.stride, c.taps, torch.float64)
    S = conv_raw(t["x"].abs(), t["w"].abs(), c.gather, c.stride, c.taps, torch.float64)
    ref, e = epilogue(acc, conv_terms(c) * U32 * S, residual=t["addend"] if addend else None)
    return ref, bf16_bound(ref, e)


def group_sum(v, groups):
    """``v [B,C,D,H,W]`` -> ``[groups*C]`` float64: sums per (group, channel), sample b in group b % groups."""
    B, C = v.shape[0], v.shape[1]
    return v.double().reshape(B // groups, groups, C, -1).sum(dim=(0, 3)).reshape(-1)


def fwd_sums_expect(y_dev, groups):
    """float64 ``(s1, s2, b1, b2)`` per (group, channel) of the device's own output ``y_dev [B,C,D,H,W]``: sum, sum of squares, bounds."""
    y = y_dev.double()
    s1, s2 = group_sum(y, groups), group_sum(y * y, groups)
    k = C_ACC * SUM_CHAIN * U32
    return s1, s2, k * group_sum(y.abs(), groups), k * s2


def bwd_sums_expect(dz_dev, bn_y, bn4, relu, groups, ge=False):
    """float64 ``(s1, s2, b1, b2)`` of the BatchNorm backward sums over the device's own gradient ``dz_dev``: g = dz [bn_y scale + shift >
    0 or not relu], s1 = sum g, s2 = sum g (bn_y - mean) invstd.  ``ge``: the mutation ``>= 0``."""
    B, C = dz_dev.shape[0], dz_dev.shape[1]
    sc, sh, mu, inv = (per_sample(bn4[i].double(), B, groups, C) for i in range(4))
    pre = bn_y.double() * sc + sh
    g = dz_dev.double() * ((pre >= 0) if ge else (pre > 0)).double() if relu else dz_dev.double()
    t2 = g * (bn_y.double() - mu) * inv
    k = C_ACC * (dz_dev.numel() // (groups * C) + 3) * U32
    return group_sum(g, groups), group_sum(t2, groups), k * group_sum(g.abs(), groups), k * group_sum(t2.abs(), groups)


def finalize_expect(s1, s2, b1, b2, count, gamma, beta, eps, momentum, rm0, rv0, groups):
    """``mvsbn::finalize`` + ``running_update`` in float64 from sums ``[groups*C]`` with bounds ``b1, b2`` -> dict of ``(value, bound)``:
    scale, shift, mean, invstd ``[groups*C]``, running_mean, running_var ``[C]`` (the groups' updates in order)."""
    C = gamma.numel()
    eps, momentum = float(torch.tensor(eps, dtype=torch.float32)), float(torch.tensor(momentum, dtype=torch.float32))     # as the kernel holds them
    gam, bet = gamma.double().repeat(groups), beta.double().repeat(groups)
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    b_mean = b1 / count
    b_var = b2 / count + (2 * mean.abs() + b_mean) * b_mean

    def f(v):
        return 1.0 / torch.sqrt(v + eps)
    invstd = f(var)
    b_inv = torch.maximum((f(var + b_var) - invstd).abs(), (f((var - b_var).clamp_min(0)) - invstd).abs()) + U32 * invstd
    scale = gam * invstd
    b_scale = gam.abs() * b_inv + U32 * scale.abs()
    shift = bet - mean * scale
    b_shift = mean.abs() * b_scale + scale.abs() * b_mean + b_mean * b_scale + U32 * shift.abs()
    rm, rv = rm0.double().clone(), rv0.double().clone()
    b_rm, b_rv = torch.zeros_like(rm), torch.zeros_like(rv)
    n1 = count / (count - 1.0) if count > 1 else 1.0
    for q in range(groups):
        sl = slice(q * C, (q + 1) * C)
        b_rm = (1 - momentum) * b_rm + momentum * (b_mean[sl] + U32 * mean[sl].abs()) + 6 * U32 * ((1 - momentum) * rm.abs() + momentum * mean[sl].abs())
        rm = (1 - momentum) * rm + momentum * mean[sl]
        ub = var[sl] * n1
        b_rv = (1 - momentum) * b_rv + momentum * (b_var[sl] * n1 + U32 * ub) + 6 * U32 * ((1 - momentum) * rv.abs() + momentum * ub)
        rv = (1 - momentum) * rv + momentum * ub
    return dict(scale=(scale, b_scale), shift=(shift, b_shift), mean=(mean, b_mean + U32 * mean.abs()), invstd=(invstd, b_inv),
                running_mean=(rm, b_rm), running_var=(rv, b_rv))


def affine_expect(y_dev, scale, shift, relu, residual, groups):
    """z = [relu](y scale + shift) [+ residual] of ``bf16_affine_act_kernel`` in float64 on the device's own ``y`` and ``stats4`` rows ->
    ``(ref, bound)``: one fmaf, one addition, the bf16 rounding."""
    B, C = y_dev.shape[0], y_dev.shape[1]
    sc, sh = per_sample(scale.double(), B, groups, C), per_sample(shift.double(), B, groups, C)
    y = y_dev.double()
    v = y * sc + sh
    e = U32 * ((y * sc).abs() + sh.abs())
    if relu:
        v = v.clamp_min(0)
    if residual is not None:
        e = e + U32 * (v.abs() + residual.double().abs())
        v = v + residual.double()
    return v, bf16_bound(v, e)


# ------------------------------------------------------------------------------------------------------------------- weight gradient
WgCase = collections.namedtuple("WgCase", "name nb CA CB Dp Hp Wp stride short taps cb_out offset probe PH inst claim data")


def _wg(name, nb, CA, CB, Dp, Hp, Wp, stride, short, PH, inst, claim="", taps=27, cb_out=None, offset=0.0, probe=False, data="randn"):
    return WgCase(name, nb, CA, CB, Dp, Hp, Wp, stride, short, taps, cb_out, offset, probe, PH, inst, claim, data)


def _wgrad_cases():
    """PH from the 56 KB ring of four Bt planes, 4 (PH s + 2)(16 s + 2) CB 2 bytes <= 57344:
        s = 1: 1440 CB  -> CB <= 32: PH 8 (46080 at 32); CB = 64: 92160 > 57344, PH 4 (4 * 6 * 18 * 64 * 2 = 55296)
        s = 2: PH 8: 4896 CB -> CB = 8: 39168; CB = 16: 78336 >, PH 4: 2720 CB = 43520; CB = 32: 87040 >, PH 2: 1632 CB = 52224
    Each (CA, CB, stride) below runs Hp = PH - 1, PH, PH + 1 while Wp cycles {15, 16, 17, 33}, Dp cycles {1, 2, 3, 5} (5 = segments of 3 and 2
    depths) and the strided axes of Bt alternate between 2 p and 2 p - 1 (``short``)."""
    combos = [(16, 16, (1, 1), 8, (1, 1)), (16, 8, (1, 2), 8, (1, 1)), (16, 8, (2, 2), 8, (1, 1)),
              (8, 64, (1, 1), 4, (1, 4)), (32, 16, (2, 2), 4, (2, 1)), (16, 16, (1, 2), 4, (1, 1)),
              (32, 32, (1, 2), 2, (2, 2)), (32, 32, (2, 2), 2, (2, 2)), (16, 32, (1, 1), 8, (1, 2))]
    out, k = [], 0
    for CA, CB, stride, PH, inst in combos:
        for dh in (-1, 0, 1):
            Wp, Dp = (15, 16, 17, 33)[k % 4], (1, 2, 3, 5)[(k // 2 + k) % 4]
            nb, short = 1 + k % 2, bool((k // 3) % 2)
            out.append(_wg("wg-c%d_%d-s%d%d-d%dh%dw%d-n%d%s" % (CA, CB, stride[0], stride[1], Dp, PH + dh, Wp, nb, "-short" if short else ""),
                           nb, CA, CB, Dp, PH + dh, Wp, stride, short, PH, inst))
            k += 1
    out += [
        _wg("wg-2d-c16_8-cbout1", 2, 16, 8, 3, 9, 17, (1, 1), False, 8, (1, 1), "taps = 9, cb_out 1 < CB", taps=9, cb_out=1),
        _wg("wg-2d-c8_16-cbout5", 1, 8, 16, 2, 7, 33, (1, 1), False, 8, (1, 1), "taps = 9, cb_out 5 < CB", taps=9, cb_out=5),
        _wg("wg-gy2-c64_16-s11", 1, 64, 16, 3, 9, 17, (1, 1), False, 8, (2, 1), "CA 64 x CB 16: two channel groups"),
        _wg("wg-gy2-c64_8-s12", 2, 64, 8, 2, 8, 15, (1, 2), True, 8, (2, 1), "CA 64 x CB 8: two channel groups"),
        # the old criterion's blind spot: 1 x 5 x 17 x 17 = 1445 voxels of positive-mean operands (what a ReLU leaves), see the refs test
        _wg("wg-offset-1445", 1, 16, 16, 5, 17, 17, (1, 1), False, 8, (1, 1), "mean-1 operands, 1445 voxels", offset=1.0),
        # more work items than blocks.  CA 64 x CB 8: nA = 4, nB = 1 -> TB = 1, TA = min(4, 4, 2) = 2, gy = 2, target = 512 / 2 = 256.  PH = 8
        # (s = 1, CB = 8), npr = 40 / 8 = 5, npc = 208 / 16 = 13: 2 * 5 * 13 = 130 columns; nseg = ceil(256 / 130) = 2 <= Dp / 2 = 2, dseg = 2:
        # npatch = 260.  blocks = min(target 256, 130 * 2 = 260) = 256 < 260: blocks 0 .. 3 take a second work item.  66 560 voxels - with
        # random operands K u32 S of that many voxels exceeds |dW| itself, so the case runs on data for which the bound bites:
        #   -int   integer operands in [-3, 3]: every product and partial sum is an integer below 2^24 (S <= 9 * 66 560), so every fp32
        #          operation is exact in any order: the bound is 0, dW must equal the float64 sum bit for bit;
        #   -tail  random operands, A non-zero only inside work items 256 .. 259 (the second items of blocks 0 .. 3: sample 1, patch row 4,
        #          patch columns 11 and 12, both depth segments - 1024 voxels): K = the voxels that have a non-zero A (the others add exact zeros).
        _wg("wg-items260-blocks256-int", 2, 64, 8, 4, 40, 208, (1, 1), False, 8, (2, 1), "npatch 260 > blocks 256, exact", data="int"),
        _wg("wg-items260-blocks256-tail", 2, 64, 8, 4, 40, 208, (1, 1), False, 8, (2, 1), "npatch 260 > blocks 256, second items only", data="tail"),
    ]
    for stride in STRIDES:
        out.append(_wg("wg-probe-s%d%d" % stride, 2, 16, 16, 3, 9, 17, stride, True, 8 if stride[1] == 1 else 4, (1, 1),
                       "A non-zero only in the last depth, row and column", probe=True))
    return out


WGRAD_CASES = _wgrad_cases()
WGRAD_CASE = {c.name: c for c in WGRAD_CASES}
assert len(WGRAD_CASE) == len(WGRAD_CASES)
OFFSET_CASE, SEGMENT_CASE = "wg-offset-1445", "wg-offset-1445"       # Dp = 5: segments [0, 3) and [3, 5)
MANY_ITEMS_CASES = ["wg-items260-blocks256-int", "wg-items260-blocks256-tail"]


def wgrad_item_region(c, item):
    """Work item -> ``(n, depth slice, row slice, column slice)`` of ``A``, decoded as ``wgrad_body`` decodes ``col``."""
    p = plan_wgrad(c.nb, c.CA, c.CB, c.Dp, c.Hp, c.Wp, c.stride[1])
    seg, r = item % p.nseg, item // p.nseg
    pcx, r = r % p.npc, r // p.npc
    pry, n = r % p.npr, r // p.npr
    return n, slice(seg * p.dseg, min((seg + 1) * p.dseg, c.Dp)), slice(pry * p.PH, min((pry + 1) * p.PH, c.Hp)), \
        slice(pcx * WG_PW, min((pcx + 1) * WG_PW, c.Wp))


def bt_dims(c):
    def dim(p, s):
        return p if s == 1 else 2 * p - (1 if c.short else 0)
    return dim(c.Dp, c.stride[0]), dim(c.Hp, c.stride[1]), dim(c.Wp, c.stride[1])


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name):
    """``A [nb,Dp,Hp,Wp,CA]``, ``Bt [nb,Db,Hb,Wb,CB]`` fp32 channel-last, bf16-representable."""
    c = WGRAD_CASE[name]
    g = _gen(c.name)
    Db, Hb, Wb = bt_dims(c)
    sd = 0.5 if c.offset else 1.0
    if c.data == "int":
        A = torch.randint(-3, 4, (c.nb, c.Dp, c.Hp, c.Wp, c.CA), generator=g).float()
        Bt = torch.randint(-3, 4, (c.nb, Db, Hb, Wb, c.CB), generator=g).float()
        return A, Bt
    A = bf(torch.randn(c.nb, c.Dp, c.Hp, c.Wp, c.CA, generator=g) * sd + c.offset)
    Bt = bf(torch.randn(c.nb, Db, Hb, Wb, c.CB, generator=g) * sd + c.offset)
    if c.data == "tail":
        p = plan_wgrad(c.nb, c.CA, c.CB, c.Dp, c.Hp, c.Wp, c.stride[1])
        keep = torch.zeros(c.nb, c.Dp, c.Hp, c.Wp, 1)
        for item in range(p.blocks, p.npatch):
            n, d, h, w = wgrad_item_region(c, item)
            keep[n, d, h, w] = 1.0
        A = A * keep
    if c.probe:
        keep = torch.zeros(c.nb, c.Dp, c.Hp, c.Wp, 1)
        keep[:, -1, -1, -1] = 1.0
        A = A * keep
    return A, Bt


def wgrad_sum(A, Bt, stride, taps, cb_out, dtype):
    """``dW[a][b][kd][kh][kw] = sum_{n,p} A[n][p][a] Bt[n][p s - 1 + k][b]`` (zero outside ``Bt``) as plain sums in ``dtype``; ``taps`` = 9:
    kd = 1 only, ``[CA,cb_out,3,3]``."""
    A, Bt = A.to(dtype), Bt.to(dtype)
    N, Dp, Hp, Wp, CA = A.shape
    _, Db, Hb, Wb, CB = Bt.shape
    cb_out = CB if cb_out is None else cb_out
    s = (stride[0], stride[1], stride[1])
    need = [(p - 1) * st + 3 for p, st in zip((Dp, Hp, Wp), s)]               # padded extent: indices -1 .. (p - 1) s + 1
    hi = [max(0, n - 1 - d) for n, d in zip(need, (Db, Hb, Wb))]
    Bp = F.pad(Bt, (0, 0, 1, hi[2], 1, hi[1], 1, hi[0]))
    dW = torch.zeros(CA, cb_out, 3, 3, 3, dtype=dtype)
    for kd, kh, kw in itertools.product(range(3), repeat=3):
        if taps == 9 and kd != 1:
            continue
        Bs = Bp[:, kd:kd + (Dp - 1) * s[0] + 1:s[0], kh:kh + (Hp - 1) * s[1] + 1:s[1], kw:kw + (Wp - 1) * s[2] + 1:s[2], :cb_out]
        dW[:, :, kd, kh, kw] = torch.einsum("ndhwa,ndhwb->ab", A, Bs)
    return dW if taps == 27 else dW[:, :, 1].contiguous()


@functools.lru_cache(maxsize=None)
def wgrad_expect(name):
    """-> ``(ref, bound)`` float64 of a case's fp32 ``dW``."""
    c = WGRAD_CASE[name]
    A, Bt = wgrad_inputs(name)
    ref = wgrad_sum(A, Bt, c.stride, c.taps, c.cb_out, torch.float64)
    S = wgrad_sum(A.abs(), Bt.abs(), c.stride, c.taps, c.cb_out, torch.float64)
    if c.data == "int":
        assert S.max().item() < 2 ** 24
        return ref, torch.zeros_like(ref)
    K = int((A != 0).any(dim=-1).sum())                       # the voxels summed: one whose A is zero adds an exact zero in any order
    return ref, C_ACC * K * U32 * S


# ------------------------------------------------------------------------------------------------------------------- mutations
# Each returns what a subtly wrong kernel would have produced, built from the reference's own arithmetic (float64), never from a kernel.
def mutate_drop_tap(c, b, od, oh, ow, tap):
    """Conv3d case ``c``: the raw output without tap ``(kd, kh, kw)`` at output voxel ``(b, od, oh, ow)``."""
    assert c.gather == 0 and c.taps == 27 and not (c.scale or c.relu or c.residual)
    t = conv_inputs(c)
    ref = conv_expect(c)[0].clone()
    i = [o * s - 1 + k for o, s, k in zip((od, oh, ow), (c.stride[0], c.stride[1], c.stride[1]), tap)]
    assert all(0 <= v < n for v, n in zip(i, (c.D, c.H, c.W))), "the dropped tap must exist"
    ref[b, :, od, oh, ow] -= t["w"].double()[:, :, tap[0], tap[1], tap[2]] @ t["x"].double()[b, :, i[0], i[1], i[2]]
    return ref


def mutate_zero_column(c, col):
    ref = conv_expect(c)[0].clone()
    ref[..., col] = 0
    return ref


def mutate_swap_parity_taps(c):
    """ConvTranspose3d with column stride 2: the two taps of the odd column parity (kw = 0, 2) swapped; even columns (kw = 1) unchanged."""
    assert c.gather == 1 and c.stride[1] == 2
    w = conv_inputs(c)["w"].clone()
    w[..., [0, 2]] = w[..., [2, 0]]
    return conv_eval(c, torch.float64, w=w)


def mutate_drop_voxel(name, n, d, h, w):
    """``dW`` of a wgrad case without voxel ``(n, d, h, w)`` of ``A``."""
    c = WGRAD_CASE[name]
    A, Bt = wgrad_inputs(name)
    A = A.clone()
    A[n, d, h, w] = 0
    return wgrad_sum(A, Bt, c.stride, c.taps, c.cb_out, torch.float64)


def mutate_drop_item(name, item):
    """``dW`` of a wgrad case without one work item (a column of patches over a depth segment)."""
    c = WGRAD_CASE[name]
    A, Bt = wgrad_inputs(name)
    A = A.clone()
    n, d, h, w = wgrad_item_region(c, item)
    A[n, d, h, w] = 0
    return wgrad_sum(A, Bt, c.stride, c.taps, c.cb_out, torch.float64)


def mutate_drop_last_segment(name):
    c = WGRAD_CASE[name]
    p = plan_wgrad(c.nb, c.CA, c.CB, c.Dp, c.Hp, c.Wp, c.stride[1])
    assert p.nseg > 1
    A, Bt = wgrad_inputs(name)
    A = A.clone()
    A[:, (p.nseg - 1) * p.dseg:] = 0
    return wgrad_sum(A, Bt, c.stride, c.taps, c.cb_out, torch.float64)
