"""The non-fused ViT primitives (csrc/vit.hip, csrc/vit_train.hip: ``gemm_x3`` in all four kernel instances, LayerNorm forward / statistics /
backward, ``colsum``, the row softmax and its backward, GELU, flash ``attention_x3``, the bicubic resize and its adjoint) against fp64 at tile
and row edges, with a PER-SLICE metric.

Metric: ``max|got - want|`` over a slice divided by ``max|want|`` over that slice (floored at 1e-30); the worst slice counts.  A slice is a
row of a matrix, a 256-element block of an elementwise result, the whole vector for ``colsum`` and for LayerNorm's mean / rstd (vector
outputs, one value per row, like a column sum).  ``want`` is the operation in fp64 on the CPU from the same fp32 inputs, ``ref32`` the same
formula in plain fp32 torch, and the bound is the contract of ``test_gemm_x3_vs_fp64``: ``err(got) < 3 * err(ref32) + 2e-7`` (``+ 5e-7`` for
the flash attention, as in ``test_attention_x3_flash_vs_fp64``).

Every case is built on the CPU by a ``*_case`` function below (inputs, ``want``, ``ref32``); tests/test_vit_edge_refs.py runs all of them
without a GPU and checks that ``err(ref32)`` is finite, non-zero and below 1e-4 and that no slice of ``want`` is identically zero, so the
``3 * err(ref32)`` term is what bounds the kernels.  Two kinds of case are marked instead of being dropped:
  * ``exact``: the result is exactly representable by construction (LayerNorm over one feature gives beta, a softmax over one element gives 1,
    its backward 0, a one-row column sum is the row, a one-column sum of dyadic inputs has no rounding, a 1x1 -> 1x1 resize is the pixel, attention over one key - or with one key 50 above
    the rest - is that key's V).  There
    ``err(ref32)`` is zero (the CPU check asserts that instead) and the bound is its floor; LayerNorm's and the softmax's closed forms are
    asserted exactly as well.
  * ``zero_ok`` (bicubic adjoint when down-sampling by more than 2): input rows that no output reads have a gradient of exactly zero; the
    floor of the metric then demands an exact zero from the kernel.
"""
import functools
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FACTOR = 3.0                                                 # err(got) < FACTOR * err(ref32) + FLOOR
FLOOR = 2e-7
FLOOR_ATT = 5e-7


# ---------------------------------------------------------------------------------------------------------------- metric
def _slices(t, kind):
    t = t.detach().double().cpu()
    if kind == "row":
        return t.reshape(-1, t.shape[-1])
    if kind == "all":
        return t.reshape(1, -1)
    assert kind == "block"
    t = t.reshape(-1)
    pad = (-t.numel()) % 256
    return torch.cat([t, t.new_zeros(pad)]).reshape(-1, 256)


def slice_err(got, want, kind):
    """Worst slice of max|got - want| / max(max|want|, 1e-30).  NaN anywhere in ``got`` gives NaN (which fails every ``<``)."""
    g, w = _slices(got, kind), _slices(want, kind)
    assert g.shape == w.shape, (g.shape, w.shape)
    e = (g - w).abs().max(1).values / w.abs().max(1).values.clamp_min(1e-30)
    return float("nan") if torch.isnan(e).any() else e.max().item()


def zero_slices(want, kind):
    return int((_slices(want, kind).abs().max(1).values == 0).sum())


@dataclass
class Out:
    """One checked output of a case."""
    name: str
    want: torch.Tensor                                       # fp64
    ref32: torch.Tensor                                      # fp32 twin
    kind: str = "row"                                        # slice kind
    exact: bool = False                                      # want is exactly representable by construction (see the module docstring)
    zero_ok: bool = False                                    # structurally zero slices of want are allowed


def check(got, out: Out, factor=FACTOR, floor=FLOOR):
    err, err32 = slice_err(got, out.want, out.kind), slice_err(out.ref32, out.want, out.kind)
    print("%s: err %.3e, err32 %.3e, ratio %.2f" % (out.name, err, err32, err / max(err32, 1e-300)))
    assert err < factor * err32 + floor, (out.name, err, err32)
    return err, err32


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k * 1000) if isinstance(k, float) else int(k) for k in key))) % (2 ** 31))


def _f32(x):
    return float(np.float32(x))


# Row scales / means of the LayerNorm and column-sum inputs: s from {1e-3, 1, 30}, m from {0, 5, -200}, paired so that |m| / s <= 7.  The fp32
# mean of a row carries ONE final rounding of up to 2^-25 |m|, i.e. 3e-8 |m| / s of the row's scale in the normalized values.  At |m| / s <= 7
# that is one rounding among the many of the row; at (s, m) = (1, -200) it is 6e-6 and alone decides the row's error in the kernel and in ref32
# alike, so the ratio of the two errors says which way two single roundings fell, not how good the kernel is (an fp32 model of the kernel's own
# summation order lands 4 x above torch's there); s = 1e-3 with m = 5 or -200 puts ref32 itself at 3e-4 .. 1e-2.  (30, -200) is the two-pass
# variance against a large mean: a one-pass E[x^2] - mean^2 would lose 2^-24 * 200^2 / 900 = 2.7e-6 of the variance, 1.3e-6 of y.
ROW_STATS = [(1.0, 0.0), (1e-3, 0.0), (30.0, -200.0), (30.0, 5.0), (1.0, 5.0), (30.0, 0.0)]


def _row_stats(rows, first):
    st = [ROW_STATS[(first + r) % len(ROW_STATS)] for r in range(rows)]
    return torch.tensor([s for s, _ in st], dtype=torch.float64)[:, None], torch.tensor([m for _, m in st], dtype=torch.float64)[:, None]


# ---------------------------------------------------------------------------------------------------------------- 1. gemm_x3
@dataclass(frozen=True)
class G:
    """A ``gemm_x3`` call.  ``lda`` / ``ldb`` / ``ldc`` = 0: the tight stride.  ``inst``: the kernel instance ``launch_gemm`` picks (asserted
    against :func:`gemm_instance`, which restates its conditions)."""
    M: int
    N: int
    K: int
    inst: str = ""
    nb1: int = 1
    nb2: int = 1
    lda: int = 0
    ldb: int = 0
    ldc: int = 0
    a_off: int = 0
    b_off: int = 0
    c_off: int = 0
    b_kn: bool = False
    a_mode: int = 0
    sA: Tuple[int, int] = (0, 0)
    sB: Tuple[int, int] = (0, 0)
    sC: Tuple[int, int] = (0, 0)
    alpha: float = 1.0
    scale: bool = False
    shift: bool = False
    act: int = 0
    mul: bool = False
    res: bool = False
    amp: float = 1.0                                         # scale of A's entries (the epilogue cases: pre-activations out to +-12)

    def ld(self):
        lda = self.lda or (self.M if self.a_mode == 3 else self.K)
        ldb = self.ldb or (self.N if self.b_kn else self.K)
        return lda, ldb, self.ldc or self.N

    def id(self):
        d = G(self.M, self.N, self.K)
        extra = ["%s=%s" % (k, getattr(self, k)) for k in self.__dataclass_fields__ if k not in ("M", "N", "K", "inst", "amp") and
                 getattr(self, k) != getattr(d, k)]
        return "%s-%dx%dx%d%s" % (self.inst, self.M, self.N, self.K, ("-" + ",".join(extra)).replace(" ", "") if extra else "")


def gemm_instance(g: G) -> str:
    """``launch_gemm`` (csrc/vit.hip) restated: the pipelined ("fast") kernel needs a_mode == 0, b_kn == 0, K % 32 == 0, lda / ldb and the
    four A / B batch strides multiples of 4 floats, 16-byte aligned A and B pointers (a device allocation is aligned to at least 256 bytes, so
    this is a_off % 4 == 0 and b_off % 4 == 0; the GPU test asserts the allocation's alignment) and operands below 2 GiB; anything else goes
    to the general kernel.  Either kernel runs as its 128-row instance <2> when M >= 2048 (MVS_GEMM_BIG_M unset), else as <1>."""
    lda, ldb, _ = g.ld()
    aligned = g.K % 32 == 0 and lda % 4 == 0 and ldb % 4 == 0 and all(s % 4 == 0 for s in g.sA + g.sB) and g.a_off % 4 == 0 and g.b_off % 4 == 0 \
        and g.M * lda * 4 < 2 ** 31 and g.N * ldb * 4 < 2 ** 31
    fast = g.a_mode == 0 and not g.b_kn and aligned
    return ("fast" if fast else "general") + ("<2>" if g.M >= 2048 else "<1>")


def _gemm_cases():
    c = []
    # fast <1>: K = 32 (the second prefetch entirely out of range), odd tile counts (K = 32, 96, 160: the `if (k0 < a.K)` tail) and even
    # ones (64), rows beyond M / N served by the out-of-range buffer offset (every shape but 64 x 64)
    for M, N, K in ((1, 1, 32), (63, 65, 32), (64, 64, 64), (65, 63, 96), (129, 130, 160)):
        c.append(G(M, N, K, "fast<1>"))
    # batched, distinct strides per operand, A broadcast over the first batch axis (stride 0); all A / B strides multiples of 4
    c.append(G(65, 63, 96, "fast<1>", nb1=2, nb2=3, sA=(0, 65 * 96 + 8), sB=(3 * 63 * 96 + 12, 63 * 96 + 4), sC=(3 * 65 * 63 + 7, 65 * 63 + 1)))
    # fast <2>: the 128-row tile from M = 2048 on; M on both sides of the 128- and the 64-row boundaries, N = 64 / 65, one and three K tiles
    for M in (2048, 2049, 2048 + 127, 2048 + 129):
        for N in (64, 65):
            for K in (32, 96):
                c.append(G(M, N, K, "fast<2>"))
    c.append(G(2049, 65, 32, "fast<2>", nb2=2, sA=(0, 2049 * 32 + 4), sB=(0, 65 * 32 + 8), sC=(0, 2049 * 65 + 3)))
    # general <1>, one disqualifier of the fast kernel at a time
    for K in (1, 7, 8, 9, 31, 33, 100):                      # lda % 4 != 0: alternate rows 16-byte aligned -> vector and scalar loads mixed per thread
        c.append(G(70, 67, K, "general<1>", lda=K + 1, ldb=K + 3))
    c.append(G(70, 67, 64, "general<1>", lda=65))            # only lda
    c.append(G(70, 67, 64, "general<1>", ldb=67))            # only ldb
    c.append(G(70, 67, 40, "general<1>"))                    # only K % 32 (aligned rows: vector loads up to the K tail)
    for off in (1, 2, 3):                                    # a base pointer 4, 8, 12 bytes off with aligned strides: every load scalar
        c.append(G(70, 67, 64, "general<1>", lda=68, a_off=off))
        c.append(G(70, 67, 64, "general<1>", ldb=68, b_off=off))
    for N in (1, 7, 9, 63, 65, 130):                         # B stored [K][N]: the n + e < N tail
        c.append(G(33, N, 40, "general<1>", b_kn=True, ldb=N + 3))
    c.append(G(70, 67, 45, "general<1>", a_mode=3, lda=72, b_kn=True))      # A stored [K][M], lda > M (the weight gradient's form)
    c.append(G(70, 67, 45, "general<1>", a_mode=3, lda=73, b_kn=False, ldb=47))
    # general <2>
    c.append(G(2048 + 65, 67, 33, "general<2>"))
    c.append(G(2048 + 65, 67, 40, "general<2>", b_kn=True, ldb=70))
    return c


def _epilogue_cases():
    """One fast and one general shape, ldc = N + 5, c_off = 3 (which also offsets mul and res), alpha = -0.37; every act x {scale, shift};
    mul, res and both.  amp puts the pre-activations' standard deviation at about 4: both tails of GELU / Swish out to +-12."""
    c = []
    for inst, K, kw in (("fast<1>", 96, {}), ("general<1>", 100, dict(lda=101))):
        base = dict(ldc=67 + 5, c_off=3, alpha=-0.37, amp=1.1, **kw)
        for act in (0, 1, 2, 3):
            for scale, shift in ((True, False), (False, True), (True, True), (False, False)):
                c.append(G(70, 67, K, inst, act=act, scale=scale, shift=shift, **base))
        for mul, res in ((True, False), (False, True), (True, True)):
            c.append(G(70, 67, K, inst, act=1, scale=True, shift=True, mul=mul, res=res, **base))
    return c


GEMM_CASES = _gemm_cases()
EPILOGUE_CASES = _epilogue_cases()


@dataclass
class GemmData:
    g: G
    bufA: torch.Tensor
    bufB: torch.Tensor
    idxC: torch.Tensor                                       # [nb1][nb2][M][N] -> flat index into the C buffer (before c_off)
    lenC: int
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    bufmul: Optional[torch.Tensor]
    bufres: Optional[torch.Tensor]
    pre: torch.Tensor                                        # fp64 pre-activation
    out: Out


def _index(shape, strides, off):
    n = off + sum((s - 1) * st for s, st in zip(shape, strides)) + 1
    return torch.arange(n).as_strided(shape, strides, off), n


def _fill(idx, n, gen, amp=1.0):
    """A flat buffer of n floats, NaN except at the addressed elements (a read outside them poisons the result)."""
    buf = torch.full((n + 8,), float("nan"))
    u = idx.reshape(-1).unique()
    buf[u] = torch.randn(u.numel(), generator=gen) * amp
    return buf


def _act(v, act):
    return (v, F.gelu(v), v * torch.sigmoid(v), torch.relu(v))[act]


@functools.lru_cache(maxsize=None)
def gemm_case(g: G) -> GemmData:
    lda, ldb, ldc = g.ld()
    gen = _gen(g.M, g.N, g.K, lda, ldb, g.a_off, g.b_off, g.act, g.scale, g.shift, g.mul, g.res, g.nb1, g.nb2)
    sC = g.sC if g.nb1 * g.nb2 > 1 else (0, 0)
    idxA, nA = _index((g.nb1, g.nb2, g.M, g.K), g.sA + ((1, lda) if g.a_mode == 3 else (lda, 1)), g.a_off)
    idxB, nB = _index((g.nb1, g.nb2, g.N, g.K), g.sB + ((1, ldb) if g.b_kn else (ldb, 1)), g.b_off)
    idxC, nC = _index((g.nb1, g.nb2, g.M, g.N), sC + (ldc, 1), g.c_off)
    bufA, bufB = _fill(idxA, nA, gen, g.amp), _fill(idxB, nB, gen)
    A, B = bufA[idxA], bufB[idxB]
    scale = torch.rand(g.N, generator=gen) + 0.5 if g.scale else None
    shift = torch.randn(g.N, generator=gen) * 2 if g.shift else None
    bufmul = _fill(idxC, nC, gen) if g.mul else None
    bufres = _fill(idxC, nC, gen) if g.res else None

    def run(A, B, dt):                                       # the kernel's documented order: alpha, scale / shift, act, mul, res
        v = (A.to(dt) @ B.to(dt).transpose(-1, -2)) * torch.tensor(_f32(g.alpha), dtype=dt)
        if scale is not None:
            v = v * scale.to(dt)
        if shift is not None:
            v = v + shift.to(dt)
        pre = v
        v = _act(v, g.act)
        if bufmul is not None:
            v = v * bufmul[idxC].to(dt)
        if bufres is not None:
            v = v + bufres[idxC].to(dt)
        return pre, v

    pre, want = run(A, B, torch.float64)
    _, ref32 = run(A, B, torch.float32)
    return GemmData(g, bufA, bufB, idxC, nC + 8, scale, shift, bufmul, bufres, pre, Out("gemm " + g.id(), want, ref32, "row"))


SENTINEL = 777.25


def _run_gemm(dev, d: GemmData):
    from mvsformer_amd import ops
    g = d.g
    lda, ldb, ldc = g.ld()
    A, B = d.bufA.to(dev), d.bufB.to(dev)
    assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0           # what gemm_instance() assumes of a device allocation
    opt = lambda t: None if t is None else t.to(dev)
    outs = []
    for _ in range(2):
        C = torch.full((d.lenC,), SENTINEL, device=dev)
        ops.gemm_x3(A, B, C, g.M, g.N, g.K, lda, ldb, ldc, nb1=g.nb1, nb2=g.nb2, sA=g.sA, sB=g.sB, sC=g.sC if g.nb1 * g.nb2 > 1 else (0, 0), b_kn=g.b_kn,
                    a_mode=g.a_mode, alpha=g.alpha, scale=opt(d.scale), shift=opt(d.shift), act=g.act, mul=opt(d.bufmul), res=opt(d.bufres),
                    a_off=g.a_off, b_off=g.b_off, c_off=g.c_off)
        outs.append(C)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])                     # fixed order: bitwise reproducible
    C = outs[0].cpu()
    untouched = torch.ones(d.lenC, dtype=torch.bool)
    untouched[d.idxC.reshape(-1)] = False
    assert bool((C[untouched] == SENTINEL).all()), "wrote outside C (gap columns / before c_off / past the last row)"
    return C[d.idxC]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert os.environ.get("MVS_GEMM_BIG_M") is None and os.environ.get("MVS_GEMM_FAST") is None      # gemm_instance() describes the defaults
    return torch.device("cuda:0")


@pytest.mark.parametrize("g", GEMM_CASES, ids=G.id)
def test_gemm_x3_instances_vs_fp64(dev, g):
    """All four instances of ``launch_gemm`` (the id names the one each case reaches; see :func:`gemm_instance`)."""
    assert gemm_instance(g) == g.inst
    d = gemm_case(g)
    check(_run_gemm(dev, d), d.out)


@pytest.mark.parametrize("g", EPILOGUE_CASES, ids=G.id)
def test_gemm_x3_epilogue_vs_fp64(dev, g):
    assert gemm_instance(g) == g.inst
    d = gemm_case(g)
    check(_run_gemm(dev, d), d.out)


# ---------------------------------------------------------------------------------------------------------------- 2. LayerNorm
LN_C = (1, 2, 63, 64, 65, 384, 1023, 1024)
LN_ROWS = (1, 3, 4, 5, 9)
LN_EPS = 1e-6


@dataclass
class LnData:
    x: torch.Tensor
    gamma: torch.Tensor
    beta: torch.Tensor
    dy: torch.Tensor
    res: torch.Tensor
    y: Out
    mean: Out
    rstd: Out
    dx: Out
    dx_res: Out


@functools.lru_cache(maxsize=None)
def ln_case(C, rows) -> LnData:
    gen = _gen(C, rows, 2)
    s, m = _row_stats(rows, LN_C.index(C) if C in LN_C else C)
    if C == 2:
        # Two features normalize to +-1 whatever x is: dx is only what eps lets through, eps / (var + eps)^1.5 of dy.  With var >> eps it is
        # a cancellation residue at 1e-6 of its terms, and fp32 (kernel and ref32 alike) returns rounding noise.  Every row of this one
        # width is drawn as (s, m) = (1e-3, 0): var ~ eps = 1e-6, and the gradient is of the order of its terms.
        s, m = torch.full_like(s, 1e-3), torch.zeros_like(m)
    x = (torch.randn(rows, C, generator=gen, dtype=torch.float64) * s + m).float()
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    dy, res = torch.randn(rows, C, generator=gen), torch.randn(rows, C, generator=gen)
    if C == 2:
        # ... and with g = dy * gamma, dx = +-rstd * (1 - xhat^2) * (g0 - g1) / 2: a row whose g0 and g1 nearly agree is the rounding of
        # g - mean(g), |g0 + g1| / |g0 - g1| times 2^-24, in any fp32 formula.  Opposite signs (gamma > 0) keep that factor below 1.
        dy[:, 1] = -dy[:, 1].abs() * torch.sign(dy[:, 0])
    eps = _f32(LN_EPS)                                       # the kernels take eps as a float

    def run(dt):
        xr = x.to(dt).clone().requires_grad_(True)
        y = F.layer_norm(xr, (C,), gamma.to(dt), beta.to(dt), eps)
        dx, = torch.autograd.grad((y * dy.to(dt)).sum(), xr)
        mean = xr.detach().mean(1)
        rstd = (xr.detach().var(1, unbiased=False) + eps).rsqrt()
        return y.detach(), mean, rstd, dx, dx + res.to(dt)

    w, r = run(torch.float64), run(torch.float32)
    ex = C == 1                                              # one feature: y = beta, mean = x, dx = 0 (+ res), exactly
    if ex:                                                   # (autograd's own formula leaves a residue of 1e-13 of rstd * dy there: the closed form)
        w = w[:3] + (torch.zeros(rows, 1, dtype=torch.float64), res.double())
        r = r[:3] + (torch.zeros(rows, 1), res.clone())
    tag = "layernorm C=%d rows=%d " % (C, rows)
    mean_ex = C <= 2 and bool((w[1].float().double() == w[1]).all())    # (one feature, or two whose sum needs no rounding: the means are fp32 numbers)
    outs = [Out(tag + n, w[i], r[i], k, exact=e) for i, (n, k, e) in enumerate((("y", "row", ex), ("mean", "all", mean_ex), ("rstd", "all", False),
                                                                                ("dx", "row", ex), ("dx+res", "row", ex)))]
    return LnData(x, gamma, beta, dy, res, *outs)


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("C", LN_C)
def test_layernorm_fwd_stats_bwd_vs_fp64(dev, C, rows):
    from mvsformer_amd import ops
    d = ln_case(C, rows)
    f = lambda t: t.to(dev)
    x, gamma, beta, dy, res = f(d.x), f(d.gamma), f(d.beta), f(d.dy), f(d.res)
    y0 = ops.layernorm(x, gamma, beta, LN_EPS)
    y, mean, rstd = ops.layernorm_stats(x, gamma, beta, LN_EPS)
    y2, mean2, rstd2 = ops.layernorm_stats(x, gamma, beta, LN_EPS)
    assert torch.equal(y0, y) and torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    check(y, d.y), check(mean, d.mean), check(rstd, d.rstd)
    # the backward reads the GPU's own statistics, as the model does
    dx, dxr = ops.layernorm_bwd(dy, x, mean, rstd, gamma), ops.layernorm_bwd(dy, x, mean, rstd, gamma, res=res)
    assert torch.equal(dx, ops.layernorm_bwd(dy, x, mean, rstd, gamma)) and torch.equal(dxr, ops.layernorm_bwd(dy, x, mean, rstd, gamma, res=res))
    check(dx, d.dx), check(dxr, d.dx_res)
    if C == 1:
        assert torch.equal(y.cpu(), d.beta.expand(rows, 1)) and not dx.any() and torch.equal(dxr.cpu(), d.res)


# ---------------------------------------------------------------------------------------------------------------- 3. colsum
CS_ROWS = (1, 63, 64, 65, 128, 129)
CS_C = (1, 255, 256, 257, 384)


@dataclass
class CsData:
    dy: torch.Tensor
    x: torch.Tensor
    mean: torch.Tensor
    rstd: torch.Tensor
    plain: Out
    dgamma: Out
    dbeta: Out


@functools.lru_cache(maxsize=None)
def colsum_case(rows, C) -> CsData:
    """Column sums of dy, and LayerNorm's (dgamma | dbeta) = (sum dy * (x - mean) * rstd | sum dy).  mean / rstd are inputs of the kernel:
    per row near the row's m and 1 / s (not the row's exact statistics, so that C = 1 does not make dgamma identically zero)."""
    gen = _gen(rows, C, 3)
    s, m = _row_stats(rows, rows + C)
    if C == 1:
        # One column: each output is a single number, and the ratio of two single rounding errors (kernel / ref32) is a coin toss.  The inputs
        # are dyadic instead - dy and x - mean multiples of 1/8, rstd a power of two that follows 1 / s - so that every product and every partial sum
        # is exact in fp32: the kernel must return the exact sums (an ``exact`` case), whatever its order of summation.
        k8 = lambda: torch.round(torch.randn(rows, 1, generator=gen, dtype=torch.float64) * 8) / 8
        mean = m.float().reshape(rows)
        x = (m + k8()).float()
        dy = k8().float()
        rstd = torch.exp2((-torch.round(torch.log2(s))).clamp(-2, 2)).float().reshape(rows)      # 1/4 .. 4: sums of 129 terms stay below 24 bits
    else:
        x = (torch.randn(rows, C, generator=gen, dtype=torch.float64) * s + m).float()
        dy = torch.randn(rows, C, generator=gen)
        mean = (m + 0.1 * s * torch.randn(rows, 1, generator=gen, dtype=torch.float64)).float().reshape(rows)
        rstd = (1.0 / (s * (1.0 + 0.2 * torch.rand(rows, 1, generator=gen, dtype=torch.float64)))).float().reshape(rows)

    def run(dt):
        d = dy.to(dt)
        return (d * ((x.to(dt) - mean.to(dt)[:, None]) * rstd.to(dt)[:, None])).sum(0), d.sum(0)

    (g64, b64), (g32, b32) = run(torch.float64), run(torch.float32)
    tag = "colsum %dx%d " % (rows, C)
    ex = rows == 1 or C == 1                                 # one row: its column sum is the row itself; one column: exact sums (above)
    return CsData(dy, x, mean, rstd, Out(tag + "plain", b64, b32, "all", exact=ex), Out(tag + "dgamma", g64, g32, "all", exact=C == 1),
                  Out(tag + "dbeta", b64, b32, "all", exact=ex))


@functools.lru_cache(maxsize=None)
def colsum_long_case() -> Out:
    gen = _gen(257, 5)
    dy = torch.randn(2, 257, 5, generator=gen)
    out = Out("colsum 2x(257x5)", dy.double().sum(0).reshape(-1), dy.sum(0).reshape(-1), "all")
    out.dy = dy
    return out


@pytest.mark.parametrize("C", CS_C)
@pytest.mark.parametrize("rows", CS_ROWS)
def test_colsum_vs_fp64(dev, rows, C):
    from mvsformer_amd import ops
    d = colsum_case(rows, C)
    dy, x, mean, rstd = (t.to(dev) for t in (d.dy, d.x, d.mean, d.rstd))
    plain, both = ops.colsum(dy), ops.colsum(dy, x, mean, rstd)
    assert torch.equal(plain, ops.colsum(dy)) and torch.equal(both, ops.colsum(dy, x, mean, rstd))
    assert both.shape == (2 * C,)
    check(plain, d.plain), check(both[:C], d.dgamma), check(both[C:], d.dbeta)


def test_colsum_long_rows_vs_fp64(dev):
    from mvsformer_amd import ops
    d = colsum_long_case()
    dy = d.dy.to(dev)
    got = ops.colsum(dy, cols=257 * 5)
    assert torch.equal(got, ops.colsum(dy, cols=257 * 5)) and got.shape == (257 * 5,)
    check(got, d)


# ---------------------------------------------------------------------------------------------------------------- 4. softmax rows, forward and backward
SM_N = (1, 2, 255, 256, 257, 1729, 8191, 8192)
SM_ROWS = (1, 5)
SM_SCALES = (0.125, 1.0)
SM_KINDS = ("ordinary", "peaked", "shifted")


@functools.lru_cache(maxsize=None)
def softmax_case(N, rows, scale, kind) -> Out:
    """ordinary: randn * 4; peaked: one entry 60 (after scaling) above the rest; shifted: every scaled entry near +80, so only the max
    subtraction keeps exp finite.  Both scales are powers of two: scale * x is exact in every precision."""
    gen = _gen(N, rows, scale, SM_KINDS.index(kind))
    x = torch.randn(rows, N, generator=gen, dtype=torch.float64) * 4
    if kind == "peaked":
        j = torch.randint(0, N, (rows,), generator=gen)
        x[torch.arange(rows), j] = x.max(1).values + 60.0 / scale
    elif kind == "shifted":
        x = (80.0 + x / 4) / scale
    x = x.float()
    out = Out("softmax N=%d rows=%d scale=%g %s" % (N, rows, scale, kind), torch.softmax(x.double() * scale, -1), torch.softmax(x * scale, -1), "row",
              exact=N == 1)
    out.x = x
    return out


@pytest.mark.parametrize("scale", SM_SCALES)
@pytest.mark.parametrize("rows", SM_ROWS)
@pytest.mark.parametrize("N", SM_N)
def test_softmax_rows_vs_fp64(dev, N, rows, scale):
    from mvsformer_amd import ops
    for kind in SM_KINDS:
        d = softmax_case(N, rows, scale, kind)
        got = ops.softmax_rows_(d.x.clone().to(dev), scale)
        assert float((got.double().sum(-1) - 1).abs().max()) < 1e-6, kind
        check(got, d)
        if N == 1:
            assert bool((got == 1).all())


SB_N = (1, 2, 255, 256, 257, 1729)
SB_BH = (1, 3)
SB_DA = ("none", "cls", "all")
SB_BIG = (8192, 1, "cls")                                    # N = 8192 with a single head (256 MiB per matrix); not reduced to 4097
SB_SCALE = 0.125


@dataclass
class SbData:
    p: torch.Tensor
    dp: torch.Tensor
    da: Optional[torch.Tensor]
    out: Out


def softmax_bwd_case(N, BH, da_form) -> SbData:
    """p = the fp64 softmax of random logits rounded to fp32; want = scale * p * (g - rowsum(p * g)), g = dp + da."""
    gen = _gen(N, BH, SB_DA.index(da_form), 4)
    # (logits of unit variance: a row with one p near 1 has dS = p (g - delta) with delta ~ g there, a cancellation by 1 / (1 - p_max) that
    # belongs to the inputs, not to the kernel)
    p = torch.softmax(torch.randn(BH, N, N, generator=gen).double(), -1).float()
    dp = torch.randn(BH, N, N, generator=gen)
    da = None if da_form == "none" else torch.randn((BH, N) if da_form == "cls" else (BH, N, N), generator=gen)

    def run(dt):
        g = dp.to(dt)
        if da_form == "cls":
            g = g.clone()
            g[:, 0] += da.to(dt)
        elif da_form == "all":
            g = g + da.to(dt)
        pd = p.to(dt)
        return torch.tensor(SB_SCALE, dtype=dt) * pd * (g - (pd * g).sum(-1, keepdim=True))

    return SbData(p, dp, da, Out("softmax_bwd N=%d BH=%d da=%s" % (N, BH, da_form), run(torch.float64), run(torch.float32), "row", exact=N == 1))


def _run_softmax_bwd(dev, d: SbData, da_form):
    from mvsformer_amd import ops
    p, dp = d.p.to(dev), d.dp.to(dev)
    da = None if d.da is None else d.da.to(dev)
    ds = ops.attention_softmax_bwd(p, dp, SB_SCALE, da)
    assert torch.equal(ds, ops.attention_softmax_bwd(p, dp, SB_SCALE, da))
    check(ds, d.out)
    if da_form == "cls":                                     # only row 0 has a dA: the other rows are the no-dA result, bit for bit
        plain = ops.attention_softmax_bwd(p, dp, SB_SCALE)
        assert torch.equal(ds[:, 1:], plain[:, 1:])
        assert p.shape[-1] == 1 or not torch.equal(ds[:, 0], plain[:, 0])
    if p.shape[-1] == 1:
        assert not ds.any()                                  # p = 1: g - p * g = 0 exactly


@pytest.mark.parametrize("da_form", SB_DA)
@pytest.mark.parametrize("BH", SB_BH)
@pytest.mark.parametrize("N", SB_N)
def test_attention_softmax_bwd_vs_fp64(dev, N, BH, da_form):
    _run_softmax_bwd(dev, softmax_bwd_case(N, BH, da_form), da_form)


def test_attention_softmax_bwd_longest_row_vs_fp64(dev):
    """N = 8192, the longest row the kernel takes (all 32 register slots of every thread), one head."""
    _run_softmax_bwd(dev, softmax_bwd_case(*SB_BIG), SB_BIG[2])


# ---------------------------------------------------------------------------------------------------------------- 5. GELU
GELU_N = (1, 255, 256, 257, 100003)
GELU_POINTS = (0.0, 1e-30, -1e-30, 40.0, -40.0)             # at +-40 the derivative is 1 / 0 and exp(-800) underflows


@dataclass
class GeluData:
    x: torch.Tensor
    dy: torch.Tensor
    y: Out
    dx: Out


@functools.lru_cache(maxsize=None)
def gelu_case(n) -> GeluData:
    """x uniform over [-12, 12] in random order (every 256-block holds values of order 1..12: below about -5.5 an fp32 GELU is a rounded
    zero, so a block of only such values would measure 1 + erf's cancellation in ref32 as well), the special points at fixed places, and the
    last element - a block of its own when n % 256 == 1 - at 0.9."""
    gen = _gen(n, 5)
    x = (torch.rand(n, generator=gen, dtype=torch.float64) * 24 - 12).float()
    if n > len(GELU_POINTS) + 1:
        x[1:1 + len(GELU_POINTS)] = torch.tensor(GELU_POINTS)
    x[-1] = 0.9
    dy = torch.randn(n, generator=gen)

    def run(dt):
        xr = x.to(dt).clone().requires_grad_(True)
        y = F.gelu(xr)
        dx, = torch.autograd.grad((y * dy.to(dt)).sum(), xr)
        return y.detach(), dx

    (y64, d64), (y32, d32) = run(torch.float64), run(torch.float32)
    return GeluData(x, dy, Out("gelu n=%d y" % n, y64, y32, "block"), Out("gelu n=%d dx" % n, d64, d32, "block"))


@pytest.mark.parametrize("n", GELU_N)
def test_gelu_fwd_bwd_vs_fp64(dev, n):
    from mvsformer_amd import ops
    d = gelu_case(n)
    x, dy = d.x.to(dev), d.dy.to(dev)
    y, dx = ops.gelu(x), ops.gelu_bwd(dy, x)
    assert torch.equal(y, ops.gelu(x)) and torch.equal(dx, ops.gelu_bwd(dy, x))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    check(y, d.y), check(dx, d.dx)


# ---------------------------------------------------------------------------------------------------------------- 6. flash attention
AT_N = (1, 2, 31, 32, 33, 63, 65, 97)                        # 32-key tiles, 64-query blocks; N = 64 is test_hip_vit.py's
AT_BH = ((1, 1), (2, 3))
AT_PEAKED = (2, 3, 97, True)                                 # the peak in the last, partial key tile (key 96 of 97)


@functools.lru_cache(maxsize=None)
def attention_case(B, NH, N, peaked=False) -> Out:
    """softmax(Q K^T / 8) V per head; the slice is one token's 64 outputs of one head.  peaked: feature 0 of every query is 8 and of the last
    key 50 (0 for the other keys), the other features scaled down: that key's logit is 50 above logits of order 1, the other keys' weights
    are below 2^-53 and the result is that key's V, exactly, in fp64 as well."""
    hd, C = 64, NH * 64
    gen = _gen(B, NH, N, int(peaked), 6)
    qkv = torch.randn(B, N, 3 * C, generator=gen) * 1.7
    if peaked:
        qkv[..., :2 * C] *= 0.5
        for h in range(NH):
            qkv[:, :, h * hd] = 8.0
            qkv[:, :, C + h * hd] = 0.0
            qkv[:, N - 1, C + h * hd] = 50.0

    def run(dt):
        q, k, v = (qkv[:, :, i * C:(i + 1) * C].reshape(B, N, NH, hd).permute(0, 2, 1, 3).to(dt) for i in range(3))
        return torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, -1) @ v          # [B, NH, N, hd]

    out = Out("attention B=%d NH=%d N=%d%s" % (B, NH, N, " peaked" if peaked else ""), run(torch.float64), run(torch.float32), "row", exact=N == 1 or peaked)
    out.qkv = qkv
    return out


def _run_attention(dev, d: Out, B, NH, N):
    from mvsformer_amd import ops
    hd = 64
    qkv = d.qkv.to(dev)
    vt = ops.attention_vt(qkv, NH)
    ldv = (N + 3) // 4 * 4
    assert vt.shape == (B, NH, hd, ldv)
    got = ops.attention_x3(qkv, vt, NH, hd ** -0.5)
    check(got.reshape(B, N, NH, hd).permute(0, 2, 1, 3), d, floor=FLOOR_ATT)
    if N % 4:                                                # "the padding must be finite" (mvs_attention_x3): any finite padding, same bits
        vt[..., N:] = 1e3
        assert torch.equal(ops.attention_x3(qkv, vt, NH, hd ** -0.5), got)


@pytest.mark.parametrize("bh", AT_BH)
@pytest.mark.parametrize("N", AT_N)
def test_attention_x3_tile_edges_vs_fp64(dev, N, bh):
    _run_attention(dev, attention_case(bh[0], bh[1], N), bh[0], bh[1], N)


def test_attention_x3_peak_in_last_partial_tile_vs_fp64(dev):
    B, NH, N, _ = AT_PEAKED
    _run_attention(dev, attention_case(*AT_PEAKED), B, NH, N)


# ---------------------------------------------------------------------------------------------------------------- 7. bicubic resize and its adjoint
# (H, W, Ho, Wo, by scale factor): one-pixel axes, strong up-sampling (clamped edge taps carry most of the weight), strong down-sampling
# (r > 2: inputs that no output reads), a wide row (two blocks of 256), and the position table's form r = 1 / ((out + 0.1) / 14)
BC_CASES = ((1, 1, 1, 1, False), (1, 1, 5, 3, False), (1, 7, 4, 7, False), (2, 2, 9, 9, False), (5, 4, 1, 1, False), (16, 16, 3, 5, False),
            (3, 300, 7, 257, False), (14, 14, 1, 37, True))
BC_PLANES = (1, 3)


@dataclass
class BcData:
    x: torch.Tensor
    dy: torch.Tensor
    rh: float
    rw: float
    y: Out
    dx: Out


@functools.lru_cache(maxsize=None)
def bicubic_case(case, planes) -> BcData:
    H, W, Ho, Wo, by_factor = case
    gen = _gen(H, W, Ho, Wo, planes, 7)
    x, dy = torch.randn(planes, H, W, generator=gen), torch.randn(planes, Ho, Wo, generator=gen)
    if by_factor:
        sf = ((Ho + 0.1) / H, (Wo + 0.1) / W)
        rh, rw = 1.0 / sf[0], 1.0 / sf[1]
        ref = lambda t: F.interpolate(t[None], scale_factor=sf, mode="bicubic", align_corners=False)[0]
    else:
        rh, rw = H / Ho, W / Wo
        ref = lambda t: F.interpolate(t[None], size=(Ho, Wo), mode="bicubic", align_corners=False)[0]

    def run(dt):
        xr = x.to(dt).clone().requires_grad_(True)
        y = ref(xr)
        assert y.shape == (planes, Ho, Wo)
        dx, = torch.autograd.grad((y * dy.to(dt)).sum(), xr)
        return y.detach(), dx

    (y64, d64), (y32, d32) = run(torch.float64), run(torch.float32)
    tag = "bicubic %dx%d->%dx%d planes=%d " % (H, W, Ho, Wo, planes)
    ex = (H, W, Ho, Wo) == (1, 1, 1, 1)
    return BcData(x, dy, rh, rw, Out(tag + "y", y64, y32, "row", exact=ex), Out(tag + "dx", d64, d32, "row", exact=ex, zero_ok=max(rh, rw) > 2))


@pytest.mark.parametrize("planes", BC_PLANES)
@pytest.mark.parametrize("case", BC_CASES, ids=lambda c: "%dx%d-%dx%d" % c[:4])
def test_bicubic_fwd_adjoint_vs_fp64(dev, case, planes):
    from mvsformer_amd import ops
    H, W, Ho, Wo, _ = case
    d = bicubic_case(case, planes)
    x, dy = d.x.to(dev), d.dy.to(dev)
    y = ops.bicubic_resize(x, Ho, Wo, d.rh, d.rw)
    dx = ops.bicubic_resize_bwd(dy, H, W, d.rh, d.rw)
    assert torch.equal(dx, ops.bicubic_resize_bwd(dy, H, W, d.rh, d.rw))
    check(y, d.y), check(dx, d.dx)
    lhs = (y.double().cpu() * d.dy.double()).sum().item()    # <R x, dy> = <x, R^T dy>
    rhs = (d.x.double() * dx.double().cpu()).sum().item()
    assert abs(lhs - rhs) < 1e-5 * (d.x.double().norm() * d.dy.double().norm()).item()


# ---------------------------------------------------------------------------------------------------------------- every case, for tests/test_vit_edge_refs.py
def all_case_outputs():
    """Yields every ``Out`` of every parametrised case above (the CPU-side check of the references iterates this)."""
    for g in GEMM_CASES + EPILOGUE_CASES:
        yield gemm_case(g).out
    for C in LN_C:
        for rows in LN_ROWS:
            d = ln_case(C, rows)
            yield from (d.y, d.mean, d.rstd, d.dx, d.dx_res)
    for rows in CS_ROWS:
        for C in CS_C:
            d = colsum_case(rows, C)
            yield from (d.plain, d.dgamma, d.dbeta)
    yield colsum_long_case()
    for N in SM_N:
        for rows in SM_ROWS:
            for scale in SM_SCALES:
                for kind in SM_KINDS:
                    yield softmax_case(N, rows, scale, kind)
    for N in SB_N:
        for BH in SB_BH:
            for da in SB_DA:
                yield softmax_bwd_case(N, BH, da).out
    yield softmax_bwd_case(*SB_BIG).out
    for n in GELU_N:
        d = gelu_case(n)
        yield from (d.y, d.dx)
    for N in AT_N:
        for B, NH in AT_BH:
            yield attention_case(B, NH, N)
    yield attention_case(*AT_PEAKED)
    for case in BC_CASES:
        for planes in BC_PLANES:
            d = bicubic_case(case, planes)
            yield from (d.y, d.dx)
