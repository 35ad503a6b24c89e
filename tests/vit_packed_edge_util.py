"""Case lists and CPU-side builders of tests/test_hip_vit_packed_edges.py (the packed ViT inference kernels, csrc/vit_packed.hip) and of
tests/test_vit_packed_edge_refs.py.  Pure CPU: every ``*_case`` function returns the fp32 inputs, ``want`` (the operation in fp64 from the same
fp32 inputs) and ``ref32`` (the same formula in plain fp32 torch) as :class:`Out` objects of test_hip_vit_edges.py; the metric and the bound
are that module's (``err(got) < 3 * err(ref32) + floor`` per slice, a slice = one row of the result).

Layouts restated here from include/mvs_hip.h (not imported from the package, so that the host code that prepares the operands is checked too):
the packed piece order (:func:`packed_rows`), the key permutation of V^T (:data:`VT_PERM`), the implicit convolutions' weight matrices
(:func:`conv3_matrix`, :func:`convT_matrices`) and ``launch_pgemm``'s choice of kernel instance (:func:`x3p_instance`)."""
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from test_hip_vit_edges import Out, ROW_STATS, _act, _f32, _gen, _row_stats          # noqa: F401  (ROW_STATS: re-exported)

LOG2E = 1.4426950408889634
BF16_MAX = 3.3895313892515355e38


def up(n, m):
    return (n + m - 1) // m * m


# ---------------------------------------------------------------------------------------------------------------- layouts
def packed_rows(buf: torch.Tensor, rows_alloc: int, K: int) -> torch.Tensor:
    """The raw bytes of a packed ``[rows_alloc][K]`` buffer regrouped per ROW: ``[rows_alloc][K/32 * 3 terms * 4 chunks * 16 bytes]``.
    Piece (rt, ks, term) = 1 KiB at ((rt * K/32 + ks) * 3 + term) KiB, lane = chunk * 16 + r % 16, 16 bytes per lane."""
    RT, KS = rows_alloc // 16, K // 32
    b = buf.detach().cpu().reshape(-1)[:RT * KS * 3072].reshape(RT, KS, 3, 4, 16, 16)
    return b.permute(0, 4, 1, 2, 3, 5).reshape(rows_alloc, KS * 3 * 4 * 16)


# V^T: element e of chunk c of a 32-key step <-> key (e < 4 ? 4c + e : 16 + 4c + e - 4) of the step; VT_PERM[key] = its position c * 8 + e
VT_PERM = [0] * 32
for _c in range(4):
    for _e in range(8):
        VT_PERM[4 * _c + _e if _e < 4 else 16 + 4 * _c + _e - 4] = _c * 8 + _e


def vt_unpermute(vt: torch.Tensor) -> torch.Tensor:
    """``[..., Np]`` in stored order -> key order."""
    Np = vt.shape[-1]
    idx = torch.tensor([s * 32 + VT_PERM[k] for s in range(Np // 32) for k in range(32)])
    return vt[..., idx]


def conv3_matrix(w: torch.Tensor, cp: int) -> torch.Tensor:
    """``[N, cin, 3, 3]`` -> ``[N, 9 * cp]``, k = (ky * 3 + kx) * cp + c, channels zero-padded to cp."""
    n, cin = w.shape[:2]
    m = torch.zeros(n, 9, cp)
    m[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(n, 9, cin)
    return m.reshape(n, 9 * cp)


def convT_matrices(w: torch.Tensor, cp: int) -> torch.Tensor:
    """ConvTranspose2d(4, stride 2, padding 1) weight ``[cin, N, 4, 4]`` -> ``[4 classes, N, 4 * cp]``: class = ph * 2 + pw (output parity),
    k = (th * 2 + tw) * cp + c, taps ky = (1, 3) for ph = 0 and (0, 2) for ph = 1, kx likewise."""
    cin, n = w.shape[:2]
    ks = ((1, 3), (0, 2))
    out = torch.zeros(4, n, 4, cp)
    for ph in range(2):
        for pw in range(2):
            for th in range(2):
                for tw in range(2):
                    out[ph * 2 + pw, :, th * 2 + tw, :cin] = w[:, :, ks[ph][th], ks[pw][tw]].t()
    return out.reshape(4, n, 4 * cp)


# ---------------------------------------------------------------------------------------------------------------- kernel instances
# X3P_CASE of launch_pgemm: (mode, GTT, TI, NW, WJ)
X3P_INSTANCES = {(0, 8, 128, 8, 4), (0, 8, 128, 4, 2), (0, 8, 64, 4, 2), (0, 8, 128, 8, 1), (0, 8, 64, 4, 1), (0, 7, 128, 8, 1), (0, 7, 128, 4, 1),
                 (0, 7, 64, 4, 1), (1, 8, 128, 8, 4), (1, 8, 128, 4, 2), (1, 7, 128, 8, 1), (1, 7, 128, 4, 1), (1, 8, 128, 8, 1)}
# the children of family 6: (MVS_X3P_CFG, MVS_X3P_CFG_QKV); where mode 1 has no such instance the qkv form keeps its default
CHILD_CFGS = (("8,128,4,2", "8,128,4,2"), ("8,128,8,1", "8,128,8,1"), ("8,64,4,1", "8,128,8,4"), ("7,128,4,1", "7,128,4,1"), ("7,64,4,1", "8,128,8,4"))
NO_INSTANCE_CFG = "8,32,4,1"


def x3p_instance(mode: int, M: int, N: int, act: int = 0, packed_out: bool = False) -> Tuple[Tuple[int, int, int, int, int], str]:
    """``launch_pgemm``'s default choice restated (MVS_X3P_CFG / MVS_X3P_CFG_QKV unset): the instance and the branch that chose it."""
    if mode == 0 and act == 1 and packed_out:
        return (0, 8, 64, 4, 2), "gelu+packed"
    if mode == 0 and N <= 64:
        return (0, 8, 64, 4, 2), "N<=64"

    def fill(rows):
        t = ((M + rows - 1) // rows) * ((N + 127) // 128)
        return t / float((t + 255) // 256 * 256)

    if fill(112) > fill(128) + 0.05:
        return (mode, 7, 128, 8, 1), "fill"
    return (mode, 8, 128, 8, 4), "default"


def inst_name(inst):
    return "m%d:%d,%d,%d,%d" % inst


# ---------------------------------------------------------------------------------------------------------------- 1. pack / unpack
PACK_R = (1, 15, 16, 17, 37)
PACK_K = (32, 64, 96, 512)
PACK_SPECIALS = (3.4028234663852886e38, -3.4028234663852886e38, 3.39e38, -3.39e38, BF16_MAX, -BF16_MAX, 0.0, -0.0, 2.0 ** -126, -2.0 ** -126,
                 1.2345 * 2.0 ** -110, 2.0 ** -110, 1.2345 * 2.0 ** -111, 1.7 * 2.0 ** -120, 1.999 * 2.0 ** -126, 2.0 ** -127, 3 * 2.0 ** -149, -2.0 ** -149)
PACK_EXACT_FROM = 2.0 ** -110                                # the lsb of an fp32 with exponent e is 2^(e - 23); the smallest bf16 subnormal is 2^-133
PACK_ABS_BELOW = 2.0 ** -126


def _pack_cases():
    c = []
    for i, R in enumerate(PACK_R):
        for j, ra in enumerate((up(R, 16), up(R, 16) + 16, up(R + 1, 128))):
            c.append((R, PACK_K[(i + j) % 4], ra))
    return c


PACK_CASES = _pack_cases()


@functools.lru_cache(maxsize=None)
def pack_case(R, K) -> torch.Tensor:
    """fp32 [R][K]: exponents from 2^-125 to 2^+125, the special values first (every case has at least 32 elements)."""
    gen = _gen(R, K, 11)
    x = (torch.randn(R, K, generator=gen, dtype=torch.float64) * torch.exp2(torch.randint(-125, 126, (R, K), generator=gen).double())).float()
    x.reshape(-1)[:len(PACK_SPECIALS)] = torch.tensor(PACK_SPECIALS, dtype=torch.float64).float()
    assert bool(torch.isfinite(x).all())
    return x


def split3_model(x: torch.Tensor):
    """csrc/split3.h on the CPU: h = bf16(clamp(v)), m = bf16(v - h), l = bf16(v - h - m), round to nearest even, subnormals kept."""
    h = x.clamp(-BF16_MAX, BF16_MAX).bfloat16().float()
    r = x - h
    m = r.bfloat16().float()
    l = (r - m).bfloat16().float()
    return h, m, l


def check_roundtrip(got: torch.Tensor, x: torch.Tensor):
    """Bit-exact for |v| >= 2^-110, within 2^-126 below (zeros: equal as numbers; the split of -0 sums to +0)."""
    big = x.abs() >= PACK_EXACT_FROM
    assert torch.equal(got[big].view(torch.int32), x[big].view(torch.int32))
    assert bool(((got[~big].double() - x[~big].double()).abs() <= PACK_ABS_BELOW).all())
    assert bool((got[x == 0] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 2. LayerNorm -> packed
LNP_C = (32, 64, 96, 384, 480, 512)
LNP_NP_N = ((16, 1), (16, 16), (32, 17), (64, 37), (224, 197))
LNP_EPS = 1e-6
LNP_CASES = [(C, Np, N, 1 if (i + j) % 2 else 3) for i, C in enumerate(LNP_C) for j, (Np, N) in enumerate(LNP_NP_N)]


@dataclass
class LnpData:
    x: torch.Tensor                                          # [images * Np][C], padding rows NaN / 1e30
    gamma: torch.Tensor
    beta: torch.Tensor
    valid: torch.Tensor                                      # [images * Np] bool
    y: Out                                                   # the valid rows, [images * N][C]


@functools.lru_cache(maxsize=None)
def lnp_case(C, Np, N, images) -> LnpData:
    gen = _gen(C, Np, N, images, 12)
    rows = images * N
    s, m = _row_stats(rows, C + N)
    xv = (torch.randn(rows, C, generator=gen, dtype=torch.float64) * s + m).float()
    gamma, beta = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    x = torch.empty(images, Np, C)
    x[:, N:] = float("nan")
    x[:, N::2] = 1e30
    x[:, :N] = xv.reshape(images, N, C)
    valid = torch.zeros(images, Np, dtype=torch.bool)
    valid[:, :N] = True
    eps = _f32(LNP_EPS)
    run = lambda dt: F.layer_norm(xv.to(dt), (C,), gamma.to(dt), beta.to(dt), eps)
    return LnpData(x.reshape(images * Np, C), gamma, beta, valid.reshape(-1),
                   Out("layernorm_x3p C=%d Np=%d N=%d images=%d" % (C, Np, N, images), run(torch.float64), run(torch.float32), "row"))


# ---------------------------------------------------------------------------------------------------------------- 3. gemm_x3p
@dataclass(frozen=True)
class PG:
    """A ``gemm_x3p`` call.  ``outs``: "C" (fp32), "P" (packed) or "CP"; ``tight``: A and B allocated to the next multiple of 16 rows (the row
    tiles of a block beyond them exist only as the buffer range check's zeros), else to the next multiple of 128."""
    M: int
    N: int
    K: int
    ss: bool = False                                         # scale and shift
    act: int = 0
    res: bool = False
    outs: str = "C"
    tight: bool = True

    def inst(self):
        return x3p_instance(0, self.M, self.N, self.act, "P" in self.outs)

    def id(self):
        i, why = self.inst()
        return "%s(%s)-%dx%dx%d-%s%s%s%s-%s" % (inst_name(i), why, self.M, self.N, self.K, self.outs, "-ss" if self.ss else "", "-gelu" if self.act else "",
                                               "-res" if self.res else "", "tight" if self.tight else "128")


PG_M = (1, 15, 16, 17, 111, 112, 113, 127, 128, 129, 225, 257)
PG_N = (4, 60, 64, 68, 124, 128, 132, 192, 260)
PG_K = (32, 64, 96, 160, 384)
_PG_EPI = ((False, 0, False), (True, 0, False), (False, 1, False), (True, 1, True), (True, 0, True), (False, 1, True), (True, 1, False), (False, 0, True))


def _pg(M, N, K, v, tight=None):
    ss, act, res = _PG_EPI[v % 8]
    if M * N < 4096:                                         # too few values for both GELU tails (see test_vit_packed_edge_refs.py)
        act = 0
    outs = ("C", "P", "CP")[v % 3] if N % 32 == 0 else "C"
    return PG(M, N, K, ss, act, res and "C" in outs, outs, bool(v % 2) if tight is None else tight)


def _pg_cases():
    c = []
    for i, M in enumerate(PG_M):                             # every M with three N (36 (M, N) pairs cover every N four times), K cycling
        for d in (0, 4, 7):
            c.append(_pg(M, PG_N[(i + d) % 9], PG_K[(i + d) % 5], 3 * i + d))
    c.append(_pg(113, 132, 1536, 4))                         # 48 K steps
    # the GELU + packed epilogue with N > 64 (fc1's form): the 64-column instance by its second condition
    c.append(PG(129, 128, 96, True, 1, True, "CP", True))
    c.append(PG(257, 192, 160, False, 1, False, "P", False))
    # 112-row blocks: 10 x 12 = 120 blocks against 8 x 12 = 96 (fills 0.469 / 0.375), the last row block holds one row; and with 13
    # column blocks M = 113 (2 x 13 against 1 x 13) and M = 225 (3 x 13 against 2 x 13: 0.152 / 0.102)
    c.append(PG(1009, 1536, 32, True, 0, True, "CP", True))
    c.append(PG(113, 1664, 32, False, 0, False, "C", True))
    c.append(PG(225, 1664, 64, True, 1, False, "CP", False))
    return c


PG_CASES = _pg_cases()
# family 6: every case crosses the 112- and / or the 128-row seam
PG_SWEEP = [PG(113, 132, 96, True, 0, True, "C", True), PG(129, 64, 32, False, 0, False, "CP", True), PG(225, 128, 64, True, 1, True, "CP", False),
            PG(257, 192, 160, True, 1, False, "P", True), PG(127, 4, 32, False, 0, False, "C", True), PG(128, 260, 96, True, 0, False, "C", False),
            PG(112, 68, 64, False, 0, True, "C", True), PG(241, 128, 384, False, 0, False, "CP", True), PG(337, 60, 32, True, 0, False, "C", True),
            PG(1, 64, 64, True, 0, True, "CP", True)]
SENTINEL = 777.25
SENTINEL_BYTE = 0x5A


@dataclass
class PGData:
    g: PG
    A: torch.Tensor
    B: torch.Tensor
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    res: Optional[torch.Tensor]                              # [M][N + 4] (C's stride)
    pre: torch.Tensor
    out: Out


def _epi(v, scale, shift, act, dt):
    if scale is not None:
        v = v * scale.to(dt)
    if shift is not None:
        v = v + shift.to(dt)
    return v, _act(v, act)


@functools.lru_cache(maxsize=None)
def pg_case(g: PG) -> PGData:
    gen = _gen(g.M, g.N, g.K, g.act, int(g.ss), int(g.res), 13)
    amp = 4.5 / math.sqrt(g.K) if g.act else 1.0            # GELU: pre-activations of standard deviation >= 4.5, both tails beyond +-12
    A, B = torch.randn(g.M, g.K, generator=gen) * amp, torch.randn(g.N, g.K, generator=gen)
    scale = torch.rand(g.N, generator=gen) + 0.75 if g.ss else None
    shift = torch.randn(g.N, generator=gen) * 2 if g.ss else None
    res = torch.randn(g.M, g.N + 4, generator=gen) if g.res else None

    def run(dt):
        pre, v = _epi(A.to(dt) @ B.to(dt).t(), scale, shift, g.act, dt)
        return pre, v + res[:, :g.N].to(dt) if res is not None else v

    pre, want = run(torch.float64)
    return PGData(g, A, B, scale, shift, res, pre, Out("gemm_x3p " + g.id(), want, run(torch.float32)[1], "row"))


# ---------------------------------------------------------------------------------------------------------------- 4. qkv -> attention, CLS row
@dataclass(frozen=True)
class QA:
    images: int
    heads: int
    N: int
    Np: int
    pattern: str = ""                                        # "" = random weights; "a".."f": the designed score patterns

    def inst(self):
        return x3p_instance(1, self.images * self.Np, 3 * self.heads * 64)

    def id(self):
        return "%s-B%d-H%d-N%d-Np%d%s" % (inst_name(self.inst()[0]), self.images, self.heads, self.N, self.Np, "-" + self.pattern if self.pattern else "")


QA_N = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 197, 257)
QA_PATTERNS = "abcdef"
QA_PATTERN_N = 161                                           # six key steps, the last one holding a single key


def _qa_cases():
    c = [QA((1, 3)[i % 2], (2, 4, 6)[i % 3], N, up(N, 32)) for i, N in enumerate(QA_N)]
    c += [QA(3, 2, 5, 64), QA(1, 4, 33, 128)]                # Np beyond the rounded N
    c += [QA(5, 2, 17, 32), QA(7, 4, 32, 32), QA(7, 2, 9, 32), QA(5, 6, 1, 32)]       # Np = 32: one GEMM row block spans several images
    c += [QA(4, 6, 250, 256)]                                # 1024 rows x 9 column blocks: 90 blocks of 112 rows against 72 (0.352 / 0.281): the qkv form's 112-row default
    c += [QA(1 + (i % 2) * 2, 2, QA_PATTERN_N, up(QA_PATTERN_N, 32), p) for i, p in enumerate(QA_PATTERNS)]
    return c


QA_CASES = _qa_cases()
QA_BIG = QA(1, 2, 8192, 8192)
QA_SWEEP = [QA(1, 2, 97, 128), QA(3, 2, 33, 64), QA(7, 2, 17, 32), QA(5, 4, 32, 32), QA(1, 6, 113, 128), QA(2, 2, 129, 160), QA(1, 2, 225, 256),
            QA(3, 4, 5, 64), QA(1, 2, QA_PATTERN_N, 192, "b"), QA(3, 2, QA_PATTERN_N, 192, "c")]
HD = 64
SCALE = HD ** -0.5
QSCALE = _f32(SCALE * LOG2E)                                 # what gemm_x3p_qkv passes down as a float


@dataclass
class QAData:
    c: QA
    x: torch.Tensor                                          # [images][Np][C], rows >= N zero
    W: torch.Tensor                                          # [3C][C]
    bias: Optional[torch.Tensor]
    q: Out                                                   # [images][heads][N][64] (times QSCALE)
    k: Out
    v: Out
    att: Out                                                 # [images][heads][rows][64]
    cls: Out                                                 # [images][heads][N]
    logits: torch.Tensor                                     # fp64, natural base, [images][heads][rows][N]
    rows: Optional[torch.Tensor] = None                      # the checked query rows (None: all N)


def _pattern_x(c: QA, gen):
    """x = [qa (32) | ka (32) | v (64)] per token (C = 128), W a 0 / 1 selection: q_h = (qa, 0), k_h = (ka, 0), v_h = the v columns (head 1:
    reversed).  qa = (8, noise), ka = (b_key, noise): the logit of (query, key) is b_key + noise . noise / 8 in natural units."""
    N, L2 = c.N, math.log(2.0)
    step = torch.arange(N) // 32
    jit = torch.rand(N, generator=gen, dtype=torch.float64)
    if c.pattern == "a":
        b = torch.randn(N, generator=gen, dtype=torch.float64) * 2
    elif c.pattern == "b":                                   # one key 50 above the rest, in the last (partial) key tile
        b = torch.randn(N, generator=gen, dtype=torch.float64)
        b[N - 1] = b[:N - 1].max() + 52.0
    elif c.pattern == "c":                                   # + 7 base-2 units per key step: the reference is raised on alternate steps, P reaches 2^7
        b = (7.0 * step - 0.5 * jit) * L2
    elif c.pattern == "d":                                   # + 9.5 per step: raised at every step
        b = (9.5 * step - 0.5 * jit) * L2
    elif c.pattern == "e":                                   # descending from the first key: raised once
        b = -(0.1 * torch.arange(N, dtype=torch.float64) + 0.05 * jit) * L2
        b[1:] -= 1.0
    else:                                                    # "f": everything near + 80
        b = 80.0 + torch.randn(N, generator=gen, dtype=torch.float64)
    x = torch.zeros(c.images, c.Np, 128, dtype=torch.float64)
    x[:, :N, 0] = 8.0
    x[:, :N, 1:32] = torch.randn(c.images, N, 31, generator=gen, dtype=torch.float64) * 0.3
    x[:, :N, 32] = b
    x[:, :N, 33:64] = torch.randn(c.images, N, 31, generator=gen, dtype=torch.float64) * 0.3
    x[:, :N, 64:] = torch.randn(c.images, N, 64, generator=gen, dtype=torch.float64) * 1.7
    W = torch.zeros(3, 2, 64, 128)
    for h in range(2):
        for d in range(32):
            W[0, h, d, d] = 1.0
            W[1, h, d, 32 + d] = 1.0
        for d in range(64):
            W[2, h, d, 64 + d if h == 0 else 127 - d] = 1.0
    return x.float(), W.reshape(384, 128)


def qa_case(c: QA, rows: Optional[torch.Tensor] = None) -> QAData:
    """``rows``: restrict the attention reference to these query rows (the N = 8192 case); the CLS row is always query 0."""
    C = c.heads * HD
    gen = _gen(c.images, c.heads, c.N, c.Np, QA_PATTERNS.find(c.pattern), 14)
    if c.pattern:
        assert c.heads == 2
        x, W = _pattern_x(c, gen)
        bias = None
    else:
        x = torch.zeros(c.images, c.Np, C)
        x[:, :c.N] = torch.randn(c.images, c.N, C, generator=gen)
        W, bias = torch.randn(3 * C, C, generator=gen) * (1.7 / C ** 0.5), torch.randn(3 * C, generator=gen) * 0.3
    sel = slice(None) if rows is None else rows

    def run(dt):
        qkv = x[:, :c.N].to(dt) @ W.to(dt).t()
        if bias is not None:
            qkv = qkv + bias.to(dt)
        q, k, v = (qkv[..., i * C:(i + 1) * C].reshape(c.images, c.N, c.heads, HD).permute(0, 2, 1, 3) for i in range(3))
        logits = (q[:, :, sel] @ k.transpose(-1, -2)) * torch.tensor(SCALE, dtype=dt)
        p = torch.softmax(logits, -1)
        cls = torch.softmax((q[:, :, :1] @ k.transpose(-1, -2)) * torch.tensor(SCALE, dtype=dt), -1)[:, :, 0]
        return q * torch.tensor(QSCALE, dtype=dt), k, v, p @ v, cls, logits

    w, r = run(torch.float64), run(torch.float32)
    tag = "qkv/attention %s " % c.id()
    sel_exact = bool(c.pattern)                              # a 0 / 1 W: k and v are elements of x
    outs = [Out(tag + n, w[i], r[i], "row", exact=e) for i, (n, e) in enumerate((("q", False), ("k", sel_exact), ("v", sel_exact),
                                                                                ("att", c.pattern == "b"), ("cls", c.N == 1)))]
    return QAData(c, x, W, bias, *outs, logits=w[5], rows=rows)


qa_case_cached = functools.lru_cache(maxsize=None)(qa_case)


@functools.lru_cache(maxsize=None)
def qa_big_case() -> QAData:
    gen = _gen(8192, 15)
    rows = torch.cat([torch.tensor([0, 8191]), torch.randint(1, 8191, (30,), generator=gen)])
    return qa_case(QA_BIG, rows)


def step_maxima(logits: torch.Tensor) -> torch.Tensor:
    """Per query row the maximum logit of every 32-key step, in base-2 units: ``[..., steps]``."""
    N = logits.shape[-1]
    pad = F.pad(logits, (0, up(N, 32) - N), value=float("-inf"))
    return pad.reshape(logits.shape[:-1] + (-1, 32)).max(-1).values * LOG2E


# ---------------------------------------------------------------------------------------------------------------- 5. conv_x3p
@dataclass(frozen=True)
class CV:
    mode: int                                                # 1: 3x3 pad 1; 2: transposed 4x4 stride 2 pad 1
    images: int
    h: int
    w: int
    Cp: int
    cin: int
    N: int
    act: int = 0
    ss: bool = False
    mul: bool = False
    outs: str = "C"
    spare16: bool = True                                     # the map's allocation: pixels rounded up to 16 with at least one spare row, else to the next 128

    @property
    def M(self):
        return self.images * self.h * self.w

    def rows_out(self):
        return self.M * (4 if self.mode == 2 else 1)

    def rows_alloc(self):
        return up(self.M + 1, 16) if self.spare16 else up(self.M + 1, 128)

    def inst(self):
        return x3p_instance(0, self.M, self.N, self.act, "P" in self.outs)

    def id(self):
        i, why = self.inst()
        return "%s(%s)-mode%d-%dx%dx%d-Cp%d(%d)-N%d-act%d%s%s-%s" % (inst_name(i), why, self.mode, self.images, self.h, self.w, self.Cp, self.cin, self.N, self.act,
                                                                   "-ss" if self.ss else "", "-mul" if self.mul else "", self.outs)


CV_GEOM = ((1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 7, 9), (3, 4, 11), (1, 8, 16), (2, 12, 12))
CV_CP = ((32, 20), (64, 44), (128, 100))                     # (Cp, real channels)
CV_N = (4, 64, 72, 132)


def _cv(mode, geom, v):
    images, h, w = geom
    Cp, cin = CV_CP[v % 3]
    N = CV_N[v % 4]
    act = v % 4
    if act in (1, 2) and images * h * w * N < 4096:          # too few values for both tails (see test_vit_packed_edge_refs.py)
        act = 3 if act == 1 else 0
    outs = ("CP", "P", "C")[(v // 4) % 3] if N % 32 == 0 else "C"
    return CV(mode, images, h, w, Cp, cin, N, act, bool(v % 2), bool((v // 2) % 2), outs, bool((v // 3) % 2))


def _cv_cases():
    c = []
    for mode in (1, 2):
        for i, geom in enumerate(CV_GEOM):
            for d in (0, 5, 10):
                c.append(_cv(mode, geom, 3 * i + d + (7 if mode == 2 else 0)))
    return c


CV_CASES = _cv_cases()
CV_SWEEP = [CV(1, 2, 7, 9, 64, 44, 72, 2, True, True, "C"), CV(2, 2, 7, 9, 64, 44, 64, 3, False, False, "CP"), CV(1, 3, 4, 11, 32, 20, 132, 1, True, False, "C"),
            CV(2, 3, 4, 11, 128, 100, 4, 0, False, True, "C"), CV(1, 1, 8, 16, 32, 20, 64, 1, True, True, "CP", False), CV(2, 1, 8, 16, 64, 44, 72, 2, True, False, "C"),
            CV(1, 2, 12, 12, 128, 100, 64, 3, False, True, "P"), CV(2, 2, 12, 12, 32, 20, 132, 1, True, True, "C"), CV(1, 1, 9, 13, 64, 44, 4, 0, True, False, "C"),
            CV(2, 1, 1, 1, 32, 20, 64, 0, False, False, "CP")]


@dataclass
class CVData:
    c: CV
    xcl: torch.Tensor                                        # channel-last map [M][Cp], channels >= cin zero
    Wm: torch.Tensor                                         # mode 1: [N][9 Cp]; mode 2: [4][N][4 Cp]
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    mul: Optional[torch.Tensor]                              # [rows_out][N + 4]
    pre: torch.Tensor
    out: Out                                                 # [rows_out][N], mode 2 in the interleaved (image, 2y + ph, 2x + pw) order


@functools.lru_cache(maxsize=None)
def cv_case(c: CV) -> CVData:
    gen = _gen(c.mode, c.images, c.h, c.w, c.Cp, c.N, c.act, int(c.ss), int(c.mul), 16)
    taps = 9 if c.mode == 1 else 4
    amp = (5.5 if c.act in (1, 2) else 1.0) / math.sqrt(taps * c.cin)
    x = torch.randn(c.images, c.cin, c.h, c.w, generator=gen)
    xcl = torch.zeros(c.M, c.Cp)
    xcl[:, :c.cin] = x.permute(0, 2, 3, 1).reshape(c.M, c.cin)
    if c.mode == 1:
        w = torch.randn(c.N, c.cin, 3, 3, generator=gen) * amp
        Wm = conv3_matrix(w, c.Cp)
        conv = lambda dt: F.conv2d(x.to(dt), w.to(dt), padding=1)
    else:
        w = torch.randn(c.cin, c.N, 4, 4, generator=gen) * amp
        Wm = convT_matrices(w, c.Cp)
        conv = lambda dt: F.conv_transpose2d(x.to(dt), w.to(dt), stride=2, padding=1)
    scale = torch.rand(c.N, generator=gen) + 0.75 if c.ss else None
    shift = torch.randn(c.N, generator=gen) * 2 if c.ss else None
    mul = torch.randn(c.rows_out(), c.N + 4, generator=gen) if c.mul else None

    def run(dt):
        pre, v = _epi(conv(dt).permute(0, 2, 3, 1).reshape(c.rows_out(), c.N), scale, shift, c.act, dt)
        return pre, v * mul[:, :c.N].to(dt) if mul is not None else v

    pre, want = run(torch.float64)
    return CVData(c, xcl, Wm, scale, shift, mul, pre, Out("conv_x3p " + c.id(), want, run(torch.float32)[1], "row"))


# ---------------------------------------------------------------------------------------------------------------- every case, for tests/test_vit_packed_edge_refs.py
def all_case_outputs():
    for case in LNP_CASES:
        yield lnp_case(*case).y
    for g in PG_CASES + PG_SWEEP:
        yield pg_case(g).out
    for c in QA_CASES + QA_SWEEP:
        d = qa_case_cached(c)
        yield from (d.q, d.k, d.v, d.att, d.cls)
    d = qa_big_case()
    yield from (d.q, d.k, d.v, d.att, d.cls)
    for c in CV_CASES + CV_SWEEP:
        yield cv_case(c).out
