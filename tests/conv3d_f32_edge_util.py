"""Plans (read from the launchers' own planner), case tables, float64 references, per-element bounds and mutation helpers for the fp32 training convolutions:
``conv3d_kernel`` (csrc/conv3d_fwd.hip), ``deconv3d_kernel`` (csrc/conv3d.hip), ``wino_conv3d_kernel`` (csrc/conv3d_wino.hip) and
``wgrad_tiled_kernel`` / ``wgrad_kernel`` (csrc/wgrad.hip).  No GPU code: used by ``tests/test_hip_conv3d_f32_edges.py`` and
``tests/conv3d_f32_edge_child.py`` (MI355X) and checked by ``tests/test_conv3d_f32_edge_refs.py`` (CPU).

References: ``torch.nn.functional.conv3d`` / ``conv_transpose3d`` in float64, plain float64 sums for ``dW``.

Bounds, per element (``U32`` = 2^-24 and ``C_ACC`` = 2 are those of ``bf16_conv_edge_util``):

* direct kernels (conv, deconv).  acc = a sum of K products of fp32 numbers in fp32, in some order.  Each product is rounded once (or fused
  into the addition: fewer roundings) and each of the K - 1 additions once; every rounding is at most u32 times a quantity bounded by
  S = sum |x| |w|.  |acc - ref| <= C_ACC K u32 S: K for the additions, and C_ACC = 2 covers the products' roundings (another K) to first
  order.  S is the float64 convolution of |x| with |w|.  K = 27 Cin for the convolution (the kernel walks every tap; padding adds exact
  zeros); in the transposed form K = Cin times the taps the kernel walks for the voxel's parities: 3 per unstrided axis, 1 per even and 2
  per odd coordinate of a strided axis (``deconv3d_kernel``, ``ndtap`` / ``1 + hh`` / ``1 + pw``).
* epilogue ``bn_act`` (csrc/conv_common.h): v1 = fmaf(acc, scale, shift), one rounding of a value of size at most |acc scale| + |shift|:
  E1 = |scale| E0 + u32 (|ref scale| + |shift|); the ReLU is 1-Lipschitz; v3 = v2 + residual is one more addition:
  E3 = E2 + u32 (|v2| + |residual|) - ``bf16_conv_edge_util.epilogue``, which this module uses as it stands.  The output is fp32: no
  further rounding, bound = C_ACC E3.
* ``dW``: K = the voxels summed (batch x Dp x Hp x Wp), S = sum |A| |Bt|: C_ACC K u32 S.  Where S is 0 - the tap's window lies outside
  ``Bt`` for every voxel - the bound is 0 and the entry must be exactly 0 (the tiled kernel and the first kernel add an exact 0.0f by atomics).
* Winograd F(2x2, 3x3), as ``wino_conv3d_kernel`` / ``wino_pack_kernel`` compute it.  With d a 4 x 4 input patch, g a 3 x 3 filter:
      X = B^T d B         every entry a signed sum of 4 patch values, formed by two subtractions / additions in a row: 2 roundings
      U = G g G^T         entries of G in {0, +-1/2, 1}: the products G G g are exact, the sum of up to 9 of them commits <= 8 roundings
      Z_xi = sum over (kd, cin) of U_xi X_xi      K = (depth taps inside the volume) x Cin terms in fp32 on the matrix core
      o = A^T Z A         each output a signed sum of 9 Z: s = Z + Z + Z (2 roundings), o = s + s + s (2 roundings): 4 roundings
  Every rounding is at most u32 times a partial result, and every partial result is bounded in magnitude by the same pipeline run on
  absolute values: T = |A^T| ( sum (|G| |g| |G^T|) (.) (|B^T| |d| |B|) ) |A|, computed in float64 (``wino_pipeline(..., absolute=True)``).
  On any path from an operand to an output there are 2 + 8 + 4 = 14 roundings besides the K of the accumulation (products + additions,
  counted as C_ACC K above), so E0 = (K + 14) u32 T and the bound is C_ACC E0 (the 14 doubled too: simple, and second-order terms stay
  inside).  T >= S of the direct sum (|sum| <= sum | |); on random data T / S has a median of 7 .. 9 and reaches 17 at volume borders (printed by the
  refs test): that is the worst case of the transform's cancellations, the price of deriving the bound from the algorithm as written.  The same
  pipeline without absolute values equals the direct float64 convolution to 1e-13 (checked by the refs test): the mirror is the algorithm.
* integer cases: operands are small integers, sum of |products| < 2^24 (4 T < 2^24 for Winograd, whose U holds quarter integers: exact in
  fp32 without rescaling the weights, since every partial sum is a multiple of 1/4 below 2^22).  Every fp32 operation is exact in any
  order: bound 0, ``torch.equal``.

Weight-gradient blocks.  A block of ``wgrad_tiled_kernel`` owns tiles y, y + gy, y + 2 gy ..: the counts of two blocks of one launch differ
by at most one, so "one block with one tile and another with three" cannot occur in ONE launch.  The tables hold, per (MT, SHW), single-tile
cases (every block one tile: the loop leaves at ``if (!has_next) break``) and a multi-tile case in which some blocks own 3 tiles and the
others 2 (the prefetch loop iterates, and its last round differs between blocks)."""
import collections
import functools
import itertools

import torch
import torch.nn.functional as F

import conv_plan_reader
from bf16_conv_edge_util import C_ACC, U32, epilogue, inside, share          # noqa: F401  (re-exported for the tests)

GUARD = 777.25
STRIDES = [(1, 1), (1, 2), (2, 2)]


def ceil_div(a, b):
    return -(-a // b)


def _gen(name):
    return torch.Generator().manual_seed(sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31))


# ===================================================================================================================== plans
# What the launchers do, asked of csrc/conv3d_plan.h itself through tests/conv_plan_tool.cpp (conv_plan_reader).
ConvPlan = collections.namedtuple("ConvPlan", "form NT TD TH MT TW CC NP nsplit Do Ho Wo grid nblocks chunks")
FORMS = ("22", "42", "22s64", "22s")          # 2x2x64 all channels | 4x2x64 | 2x2x64 channels split | 2x2x32 channels split


def form_tw(form):
    """Output voxels along W of a block of ``form``."""
    return conv_plan_reader.fields("conv_tile", form)["TW"]


def plan_conv(B, Cin, Cout, Di, Hi, Wi, sd, shw, force=None):
    """``mvs_conv3d_fwd``: the form launched and its grid; ``force`` = MVS_CONV_TILE."""
    return conv_plan_reader.plan(ConvPlan, "conv", B, Cin, Cout, Di, Hi, Wi, sd, shw, force or "-")


DeconvPlan = collections.namedtuple("DeconvPlan", "route NT TWI THI TDI Do Ho Wo grid chunks")


def deconv_plan(B, Cin, Cout, Di, Hi, Wi, sd):
    """``mvs_deconv3d_fwd``: a block covers 32 input columns (+1 halo), 2 input rows and, SD == 1, 2 output depths (= input depths), SD == 2,
    1 input depth; 8 input channels per chunk.  ``route`` "s1": stride-1 depth with 8 / 16 output channels goes to the split-form kernel of
    csrc/deconv3d_s1.hip, which is not this module's subject."""
    return conv_plan_reader.plan(DeconvPlan, "deconv", B, Cin, Cout, Di, Hi, Wi, sd)


WinoPlan = collections.namedtuple("WinoPlan", "NT ngroups grid chunks prefetch")


def wino_supported(Cin, Cout, D, H, W):
    return conv_plan_reader.fields("wino", 1, Cin, Cout, D, H, W, 0)["supported"]


def wino_plan(B, Cin, Cout, D, H, W, env_nt=None):
    """A block = 4 tile rows (8 output rows) x 32 output columns of one depth plane x 16 NT channels; ``env_nt`` = MVS_WINO_NT.
    ``prefetch``: the kernel fetches the next chunk of 4 input channels under the current one's MFMAs when there is more than one."""
    got = conv_plan_reader.fields("wino", B, Cin, Cout, D, H, W, int(env_nt or 0))
    assert got["supported"]
    return conv_plan_reader.plan(WinoPlan, "wino", B, Cin, Cout, D, H, W, int(env_nt or 0), prefetch=got["chunks"] > 1)


WgPlan = collections.namedtuple("WgPlan", "MT SHW TH SEG nchunk hblocks wblocks ntiles gy tiles_min tiles_max vec_a")


def plan_wgrad(nbatch, CA, CB, Dp, Hp, Wp, shw):
    """``wgrad_tiled_kernel``.  Block y walks tiles y, y + gy, ..: ``tiles_min`` / ``tiles_max`` per block; ``vec_a``: the kernel loads A
    in 128-bit pieces when rows are 16-byte aligned."""
    got = conv_plan_reader.fields("wgrad", nbatch, CA, CB, Dp, Hp, Wp, shw)
    return conv_plan_reader.plan(WgPlan, "wgrad", nbatch, CA, CB, Dp, Hp, Wp, shw, tiles_min=got["ntiles"] // got["gy"],
                                 tiles_max=ceil_div(got["ntiles"], got["gy"]), vec_a=Wp % 4 == 0)


WgV1Plan = collections.namedtuple("WgV1Plan", "MT nchunk rows gy rows_per_wave")


def wgrad_v1_plan(nbatch, CA, CB, Dp, Hp):
    """``wgrad_kernel``: a block's four wavefronts walk rows 4 y + wave, + 4 gy, .."""
    got = conv_plan_reader.fields("wgrad_v1", nbatch, CA, CB, Dp, Hp)
    return conv_plan_reader.plan(WgV1Plan, "wgrad_v1", nbatch, CA, CB, Dp, Hp, rows_per_wave=ceil_div(got["rows"], 4 * got["gy"]))


# ===================================================================================================================== conv cases
# kind: conv | dgrad (ops.conv3d with the "dgrad" pack of a [cin, cout] layer weight) | deconv | wino | wino-dgrad
# force: MVS_CONV_TILE (conv, dgrad) or MVS_WINO_NT (wino); None = unset.  want: plan fields the planner must show for this case.
Case = collections.namedtuple("Case", "name kind force B cin cout stride D H W scale relu residual data want claim")


def _case(name, kind, force, B, cin, cout, stride, D, H, W, want, claim, epi=(False, False, False), data="randn"):
    return Case(name, kind, force, B, cin, cout, stride, D, H, W, epi[0], epi[1], epi[2], data, tuple(sorted(want.items())), claim)


_CINS, _COUTS = (4, 8, 12, 16), (8, 16, 24, 40, 48, 64)
_EPIS = [e for e in itertools.product((False, True), repeat=3) if any(e)]


def _epi_name(e):
    return "+".join(n for n, f in zip(("affine", "relu", "res"), e) if f) or "raw"


def _in_extent(o, s, odd):
    """Input extent whose stride-s output extent is ``o``: odd = 2 o - 1 (the last tap falls outside), even = 2 o."""
    return o if s == 1 else (2 * o - 1 if odd else 2 * o)


def _tile_edge_cases(form, force, tag, strides, dos):
    """``Wo`` in {TW - 1, TW, TW + 1} x the strides of one tile form, each twice.  Ho changes every third case ({1, 3}), Do every second
    (``dos``), Cin every case with period 4 ({4, 8, 12, 16}) and Cout with period 6 ({8, 16, 24, 40, 48, 64}), so that within one stride's
    six cases Ho = 1 meets Cin 4, 8, 12 and Ho = 3 meets Cin 16, 4, 8 (the next stride the other way round); stride-2 extents alternate
    odd / even per Wo.  EVERY stride-(1,1) case has a "dgrad" twin on the same shape with cin != cout: Ho in {1, 3}, Cin in {4, 8, 12, 16}."""
    out, k = [], 0
    TW = form_tw(form)
    for stride in strides:
        for Wo in (TW - 1, TW, TW + 1):
            for rep in range(2):
                Ho, Do = (1, 3)[(k // 3) % 2], dos[(k // 2) % len(dos)]
                cin, cout = _CINS[k % 4], _COUTS[(k + k // 6) % 6]
                odd = bool((k // 2 + k) % 2)                   # each Wo once with odd and once with even extents
                B = 1 + (k % 3 == 2)
                D, H, W = _in_extent(Do, stride[0], odd), _in_extent(Ho, stride[1], not odd), _in_extent(Wo, stride[1], odd)
                want = dict(form=form, Wo=Wo, Ho=Ho, Do=Do)
                if force is None and Wo > 32:                  # unforced and wider than 32: the model decides (Cin = 4 halves the 32-voxel
                    del want["form"]                           # form's useful work per chunk, so a 64-voxel form can win on few blocks)
                claim = "%s: Wo = TW%+d, Ho %d, Do %d, Cin %d, Cout %d" % (form, Wo - TW, Ho, Do, cin, cout)
                name = "%s-s%d%d-w%d-d%dh%d-b%d-c%d_%d" % (tag, stride[0], stride[1], W, D, H, B, cin, cout)
                out.append(_case(name, "conv", force, B, cin, cout, stride, D, H, W, want, claim))
                if stride == (1, 1):
                    cout2 = cout if cout != cin else 24
                    out.append(_case(name + "-dgrad", "dgrad", force, B, cin, cout2, stride, D, H, W, want, claim + " (dgrad pack)"))
                k += 1
    return out


def _forced_cases():
    out = _tile_edge_cases("22", "22", "f22", STRIDES, (1, 2, 3, 5))
    out += _tile_edge_cases("42", "42", "f42", STRIDES[:2], (3, 5))
    # MVS_CONV_TILE=42 with Do = 2: the 4-row form is refused (Do < 3) and the model decides - a small volume, so the 32-voxel form
    out.append(_case("f42-fallback-do2", "conv", "42", 1, 8, 16, (1, 1), 2, 3, 65, dict(form="22s", Do=2), "42 forced, Do = 2: falls back to the model"))
    # ... and under stride (2,2) the form is not built at all
    out.append(_case("f42-fallback-s22", "conv", "42", 1, 8, 16, (2, 2), 5, 5, 129, dict(form="22s"), "42 forced, SD = 2: falls back to the model"))
    out += _tile_edge_cases("22s", "22s", "f22s", STRIDES, (1, 2, 3, 5))
    for form in ("22", "42", "22s"):
        out.append(_case("f%s-int" % form, "conv", form, 2, 12, 24 if form != "42" else 16, (1, 1), 3, 3, 65, dict(form=form),
                         "%s: integer operands, exact" % form, data="int"))
    return out


def _default_cases():
    """In-process cases (MVS_CONV_TILE unset).  The edge table of the 32-voxel form once more, unforced (Wo <= 32 forces that form; at
    Wo = 33 the model decides and the planner says what ran).  Then the shapes on which the model picks a 64-voxel form by itself although the
    32-voxel form would need more than one round of 256 blocks (``BIG_DEFAULT``; the refs test asserts both through the planner), the
    epilogue in all eight combinations on three shapes, and the integer cases."""
    out = _tile_edge_cases("22s", None, "d22s", STRIDES, (1, 2, 3, 5))
    big = [
        # name                  B cin cout stride   D   H    W    form     CC
        ("d22-s11-c8",          1, 8, 8, (1, 1),    3, 85, 65, "22", 8),
        ("d22-s11-c24",         1, 8, 24, (1, 1),   3, 85, 65, "22", 8),
        ("d22-s11-c40",         1, 8, 40, (1, 1),   3, 65, 65, "22", 4),
        ("d42-s11",             1, 8, 8, (1, 1),    3, 57, 257, "42", 8),
        ("d22s64-s11-c24",      1, 8, 24, (1, 1),   3, 43, 65, "22s64", 8),
        ("d22s64-s11-c40",      1, 8, 40, (1, 1),   3, 21, 65, "22s64", 4),
        ("d22-s12-c8",          1, 8, 8, (1, 2),    2, 113, 513, "22", 8),
        ("d22-s12-c24",         1, 12, 24, (1, 2),  3, 129, 129, "22", 4),
        ("d42-s12",             1, 8, 8, (1, 2),    3, 169, 129, "42", 4),
        ("d22s64-s12-c24",      1, 8, 24, (1, 2),   3, 85, 129, "22s64", 4),
        ("d22s64-s12-c40",      1, 8, 40, (1, 2),   3, 41, 129, "22s64", 4),
        ("d22-s22-c8",          1, 8, 8, (2, 2),    5, 169, 129, "22", 4),
        ("d22-s22-c24",         1, 8, 24, (2, 2),   5, 169, 129, "22", 4),
        ("d22s64-s22-c24",      1, 8, 24, (2, 2),   5, 85, 129, "22s64", 4),
    ]
    for name, B, cin, cout, stride, D, H, W, form, cc in big:
        out.append(_case(name, "conv", None, B, cin, cout, stride, D, H, W, dict(form=form, CC=cc),
                         "the model picks %s by itself, CC %d" % (form, cc)))
    out.append(_case("d42-s11-dgrad", "dgrad", None, 1, 8, 16, (1, 1), 3, 57, 257, dict(form="42"), "the model picks 42, dgrad pack"))
    for e in _EPIS:                                               # the epilogue on three shapes: 4-byte stores (Wo = 33), 16-byte stores (two forms)
        out.append(_case("depi-22s-" + _epi_name(e), "conv", None, 2, 8, 24, (1, 1), 2, 3, 33, dict(form="22s"), "epilogue, Wo % 4 != 0", e))
        out.append(_case("depi-42-" + _epi_name(e), "conv", None, 1, 8, 8, (1, 2), 3, 169, 136, dict(form="42"), "epilogue, 16-byte stores (Wo 68)", e))
        out.append(_case("depi-22-" + _epi_name(e), "conv", None, 1, 8, 16, (1, 1), 2, 68, 260, dict(form="22"), "epilogue, 16-byte stores", e))
    out.append(_case("d22s-int", "conv", None, 2, 12, 24, (1, 1), 3, 3, 33, dict(form="22s"), "22s: integer operands, exact", data="int"))
    out.append(_case("d22s64-int", "conv", None, 1, 12, 24, (1, 1), 3, 43, 65, dict(form="22s64"), "22s64: integer operands, exact", data="int"))
    return out, [r[0] for r in big]


def _deconv_cases():
    """Wi in {1, 31, 32, 33} (the launcher's 32 input columns +- 1), Di, Hi cycle {1, 2, 3}, Cin cycles {8, 16, 24, 64}, Cout cycles
    {8, 16, 24, 48} under sd = 2 and {24, 48} under sd = 1 (8 / 16 there belong to deconv3d_s1.hip); each shape raw and with the whole
    epilogue."""
    out, k = [], 0
    for sd in (1, 2):
        for Wi in (1, 31, 32, 33):
            for rep in range(2):
                Di, Hi = (1, 2, 3)[k % 3], (1, 2, 3)[(k // 3 + rep) % 3]
                cin = (8, 16, 24, 64)[k % 4]
                cout = ((24, 48) if sd == 1 else (8, 16, 24, 48))[(k + k // 4) % (2 if sd == 1 else 4)]
                B = 1 + k % 2
                want = dict(route="deconv3d_kernel", Wo=2 * Wi)
                claim = "deconv sd %d: Wi = 32%+d, Di %d, Hi %d, Cin %d, Cout %d" % (sd, Wi - 32, Di, Hi, cin, cout)
                name = "dc-s%d-w%d-d%dh%d-b%d-c%d_%d" % (sd, Wi, Di, Hi, B, cin, cout)
                out.append(_case(name, "deconv", None, B, cin, cout, (sd, 2), Di, Hi, Wi, want, claim))
                out.append(_case(name + "-epi", "deconv", None, B, cin, cout, (sd, 2), Di, Hi, Wi, want, claim + ", epilogue", (True, True, True)))
                k += 1
        out.append(_case("dc-s%d-int" % sd, "deconv", None, 2, 16, 24, (sd, 2), 3, 3, 33, dict(route="deconv3d_kernel"), "integer operands, exact", data="int"))
    return out


def _wino_cases():
    """W in {4, 28, 32, 36, 68}, H in {1, 2, 7, 8, 9}, D in {1, 3}, B in {1, 3}, Cin in {4, 8, 12, 64}, Cout in {16, 32, 48, 64}; every shape
    with MVS_WINO_NT unset and = 2 (Cout 16 / 48 stay NT = 1 under it)."""
    out, k = [], 0
    for W in (4, 28, 32, 36, 68):
        for H in (1, 2, 7, 8, 9):
            cin, cout = (4, 8, 12, 64)[k % 4], (16, 32, 48, 64)[(k + k // 4) % 4]
            D, B = (1, 3)[k % 2], (1, 3)[(k // 2) % 2]
            dgrad = k % 5 == 3
            if dgrad and cin == cout:
                cout = 32
            for env in (None, "2"):
                nt = 2 if (env == "2" and cout % 32 == 0) else 1
                want = dict(NT=nt, chunks=cin // 4)
                claim = "wino NT %d: W %d, H %d, D %d, B %d, %d chunk(s)%s" % (nt, W, H, D, B, cin // 4, ", as data gradient" if dgrad else "")
                name = "wn%s-w%dh%dd%d-b%d-c%d_%d%s" % ("2" if env else "", W, H, D, B, cin, cout, "-dgrad" if dgrad else "")
                out.append(_case(name, "wino-dgrad" if dgrad else "wino", env, B, cin, cout, (1, 1), D, H, W, want, claim))
            k += 1
    for env in (None, "2"):
        for e in (_EPIS if env is None else _EPIS[-1:]):
            out.append(_case("wn%s-epi-%s" % ("2" if env else "", _epi_name(e)), "wino", env, 2, 8, 32, (1, 1), 2, 9, 36,
                             dict(NT=2 if env else 1), "wino epilogue", e))
        out.append(_case("wn%s-int" % ("2" if env else ""), "wino", env, 2, 12, 32, (1, 1), 3, 9, 36, dict(NT=2 if env else 1),
                         "integer operands, exact", data="int"))
    return out


# ``ConvFn`` / ``DeconvFn`` routing (extents the stride divides, as autograd needs them): name -> (forward wrapper, data-gradient wrapper)
ROUTE_CASES = [
    _case("rt-wino-wino", "conv", None, 2, 16, 32, (1, 1), 3, 9, 36, {}, "forward and data gradient both Winograd"),
    _case("rt-wino-dgrad", "conv", None, 1, 8, 48, (1, 1), 2, 7, 36, {}, "forward Winograd; 8 gradient channels: the direct kernel, dgrad pack"),
    _case("rt-direct-dgrad", "conv", None, 1, 8, 8, (1, 1), 2, 3, 33, {}, "W % 4 != 0: direct forward, direct dgrad"),
    _case("rt-s12-deconv", "conv", None, 1, 24, 16, (1, 2), 3, 6, 66, {}, "stride (1,2,2): deconv3d_kernel<sd 1> (24 channels) as data gradient"),
    _case("rt-s22-deconv", "conv", None, 1, 8, 24, (2, 2), 4, 6, 66, {}, "stride (2,2,2): deconv3d_kernel<sd 2> as data gradient"),
    _case("rt-dc-s2", "deconv", None, 1, 24, 24, (2, 2), 3, 2, 32, {}, "DeconvFn sd 2"),
    _case("rt-dc-s1", "deconv", None, 2, 16, 48, (1, 2), 2, 1, 33, {}, "DeconvFn sd 1"),
]
ROUTES = {"rt-wino-wino": ("conv3d_wino", "conv3d_wino"), "rt-wino-dgrad": ("conv3d_wino", "conv3d"), "rt-direct-dgrad": ("conv3d", "conv3d"),
          "rt-s12-deconv": ("conv3d", "deconv3d"), "rt-s22-deconv": ("conv3d", "deconv3d"), "rt-dc-s2": ("deconv3d", "conv3d"),
          "rt-dc-s1": ("deconv3d", "conv3d")}

FORCED_CASES = _forced_cases()
DEFAULT_CASES, BIG_DEFAULT = _default_cases()
DECONV_CASES = _deconv_cases()
WINO_CASES = _wino_cases()
ALL_CASES = FORCED_CASES + DEFAULT_CASES + DECONV_CASES + WINO_CASES
CASE = {c.name: c for c in ALL_CASES + ROUTE_CASES}
assert len(CASE) == len(ALL_CASES) + len(ROUTE_CASES)
CHILD_FORMS = ("22", "42", "22s")


def forced_cases(force):
    return [c for c in FORCED_CASES if c.force == force]


def case_plan(c):
    if c.kind in ("conv", "dgrad"):
        return plan_conv(c.B, c.cin, c.cout, c.D, c.H, c.W, c.stride[0], c.stride[1], c.force)
    if c.kind == "deconv":
        return deconv_plan(c.B, c.cin, c.cout, c.D, c.H, c.W, c.stride[0])
    return wino_plan(c.B, c.cin, c.cout, c.D, c.H, c.W, c.force)


def out_dims(c):
    if c.kind == "deconv":
        return c.D * c.stride[0], c.H * 2, c.W * 2
    return (c.D - 1) // c.stride[0] + 1, (c.H - 1) // c.stride[1] + 1, (c.W - 1) // c.stride[1] + 1


def _get(c):
    return CASE[c] if isinstance(c, str) else c


@functools.lru_cache(maxsize=None)
def case_inputs(name_or_case):
    """CPU fp32 inputs (shared, never modified): ``x [B,cin,D,H,W]``; ``w`` in the layout the wrapper's pack takes - conv / wino
    ``[cout,cin,3,3,3]``, deconv / dgrad ``[cin,cout,3,3,3]`` (dgrad: the weight of the LAYER whose data gradient is computed, layer
    Cout = this kernel's Cin), wino-dgrad: the layer's ``[cin,cout,3,3,3]`` which the caller flips and transposes as ``ConvFn.backward``
    does; ``scale, shift [cout]``; ``residual [B,cout,Do,Ho,Wo]``."""
    c = _get(name_or_case)
    g = _gen(c.name)
    wshape = ((c.cout, c.cin) if c.kind in ("conv", "wino") else (c.cin, c.cout)) + (3, 3, 3)
    Do, Ho, Wo = out_dims(c)
    if c.data == "int":
        x = torch.randint(-3, 4, (c.B, c.cin, c.D, c.H, c.W), generator=g).float()
        w = torch.randint(-3, 4, wshape, generator=g).float()
    else:
        x = torch.randn(c.B, c.cin, c.D, c.H, c.W, generator=g)
        w = torch.randn(wshape, generator=g) / (27 * c.cin) ** 0.5
    scale = (torch.rand(c.cout, generator=g) + 0.5) * torch.where(torch.rand(c.cout, generator=g) < 0.3, -1.0, 1.0)
    shift = torch.randn(c.cout, generator=g) * 0.5
    residual = torch.randn(c.B, c.cout, Do, Ho, Wo, generator=g)
    return dict(x=x, w=w, scale=scale, shift=shift, residual=residual)


# ===================================================================================================================== references
def conv_weight(c, w):
    """The ``[cout,cin,3,3,3]`` weight of the stride-(1,1) / strided convolution that a conv / dgrad / wino case computes."""
    return w if c.kind in ("conv", "wino") else w.flip(2, 3, 4).transpose(0, 1)


def raw_ref(c, x, w, dtype=torch.float64):
    """The raw layer in ``dtype``.  The data-gradient kinds are evaluated as what they are - the transposed convolution with the layer's
    weight - not as the flipped convolution the kernels run."""
    x, w = x.to(dtype), w.to(dtype)
    s3 = (c.stride[0], c.stride[1], c.stride[1])
    if c.kind in ("conv", "wino"):
        return F.conv3d(x, w, None, stride=s3, padding=1)
    if c.kind in ("dgrad", "wino-dgrad"):
        return F.conv_transpose3d(x, w, None, stride=1, padding=1)
    return F.conv_transpose3d(x, w, None, stride=s3, padding=1, output_padding=(s3[0] - 1, 1, 1))


def terms(c):
    """K per output voxel, ``[1,1,Do,Ho,Wo]`` float64 (module docstring)."""
    Do, Ho, Wo = out_dims(c)
    if c.kind == "deconv":
        def axis(n, s):
            return torch.full((n,), 3.0, dtype=torch.float64) if s == 1 else 1.0 + (torch.arange(n) % 2).double()
        kd, kh, kw = axis(Do, c.stride[0]), axis(Ho, 2), axis(Wo, 2)
        return (c.cin * kd.view(-1, 1, 1) * kh.view(1, -1, 1) * kw.view(1, 1, -1)).view(1, 1, Do, Ho, Wo)
    if c.kind in ("wino", "wino-dgrad"):                       # the depth taps inside the volume (the kernel skips the others) x Cin, + 14
        z = torch.arange(Do)
        nd = ((z - 1 >= 0).double() + 1.0 + (z + 1 < Do).double())
        return (c.cin * nd + 14.0).view(1, 1, Do, 1, 1).expand(1, 1, Do, Ho, Wo)
    return torch.full((1, 1, Do, Ho, Wo), 27.0 * c.cin, dtype=torch.float64)


_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
_G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def wino_pipeline(x, w, absolute=False):
    """F(2x2, 3x3) over (H, W), direct over D, in float64, step by step as csrc/conv3d_wino.hip: ``x [B,Cin,D,H,W]``, ``w [Cout,Cin,3,3,3]``
    -> ``[B,Cout,D,H,W]``.  ``absolute``: every operand and every coefficient by magnitude - the bound's T."""
    x, w = x.double(), w.double()
    BT, G, AT = (m.abs() if absolute else m for m in (_BT, _G, _AT))
    if absolute:
        x, w = x.abs(), w.abs()
    B, Cin, D, H, W = x.shape
    th, tw = ceil_div(H, 2), ceil_div(W, 2)
    xp = F.pad(x, (1, 2 * tw - W + 1, 1, 2 * th - H + 1, 1, 1))
    d = xp.unfold(3, 4, 2).unfold(4, 4, 2)                                     # [B,Cin,D+2,th,tw,4,4]
    X = torch.einsum("ai,bczhwij,ej->bczhwae", BT, d, BT)                      # B^T d B
    U = torch.einsum("ai,ockij,ej->ockae", G, w, G)                            # [Cout,Cin,kd,4,4]
    Z = sum(torch.einsum("ocae,bczhwae->bozhwae", U[:, :, kd], X[:, :, kd:kd + D]) for kd in range(3))
    o = torch.einsum("pa,bozhwae,qe->bozhpwq", AT, Z, AT)                      # [B,Cout,D,th,2,tw,2]
    return o.reshape(B, w.shape[0], D, 2 * th, 2 * tw)[..., :H, :W].contiguous()


def _epi_args(c, t):
    return (t["scale"] if c.scale else None, t["shift"] if c.scale else None, c.relu, t["residual"] if c.residual else None)


@functools.lru_cache(maxsize=None)
def expect(name_or_case):
    """-> ``(ref, bound)`` float64 ``[B,cout,Do,Ho,Wo]`` of a case's fp32 output."""
    c = _get(name_or_case)
    t = case_inputs(c)
    acc = raw_ref(c, t["x"], t["w"])
    if c.kind in ("wino", "wino-dgrad"):
        S = wino_pipeline(t["x"], conv_weight(c, t["w"]), absolute=True)
    else:
        S = raw_ref(c, t["x"].abs(), t["w"].abs())
    if c.data == "int":
        assert 4 * S.max().item() < 2 ** 24
        assert not (c.scale or c.relu or c.residual)
        return acc, torch.zeros_like(acc)
    ref, e = epilogue(acc, terms(c) * U32 * S, *_epi_args(c, t))
    return ref, C_ACC * e


def evaluate(c, x=None, w=None):
    """The whole layer of case ``c`` in float64 with ``x`` / ``w`` replaced (mutations)."""
    c = _get(c)
    t = case_inputs(c)
    acc = raw_ref(c, t["x"] if x is None else x, t["w"] if w is None else w)
    return epilogue(acc, torch.zeros_like(acc), *_epi_args(c, t))[0]


# ===================================================================================================================== weight gradient
# orient "conv": A = dY, Bt = X (Bt extents 2 p - 1 or 2 p under stride 2: ``short``); "deconv": A = X, Bt = dY (always 2 p).
WgCase = collections.namedtuple("WgCase", "name orient nb CA CB Dp Hp Wp stride short data want claim")


def _wg(name, orient, nb, CA, CB, Dp, Hp, Wp, stride, short, want, claim, data="randn"):
    assert orient == "conv" or not short
    return WgCase(name, orient, nb, CA, CB, Dp, Hp, Wp, stride, short, data, tuple(sorted(want.items())), claim)


def _wg_edge_cases():
    """CA in {8, 16, 24, 40, 48, 64} (MT 1, 1, 2, 3, 3, 4) x Wp in {SEG - 1, SEG, SEG + 1, SEG + 4} x shw in {1, 2}; Hp cycles {1, TH, TH + 1},
    CB cycles {1, 4, 5, 8, 64}, sd cycles {1, 2}, nbatch cycles {1, 3}, Dp = 1 every other case (else 2 or 3), the orientation and the short
    (odd) Bt extents alternate.  All of them single-tile blocks (gy == ntiles)."""
    out, k = [], 0
    for shw in (1, 2):
        for CA in (8, 16, 24, 40, 48, 64):
            tile = plan_wgrad(1, CA, 1, 1, 1, 1, shw)
            MT, TH, SEG = tile.MT, tile.TH, tile.SEG
            for dw in (-1, 0, 1, 4):
                Wp, Hp = SEG + dw, (1, TH, TH + 1)[k % 3]
                CB, sd, nb = (1, 4, 5, 8, 64)[k % 5], 1 + (k // 2) % 2, (1, 3)[(k // 3) % 2]
                Dp = 1 if k % 2 == 0 else 2 + (k // 4) % 2
                orient = "conv" if (k % 4 < 2 or (sd, shw) == (1, 1)) else "deconv"
                short = orient == "conv" and k % 2 == 1
                want = dict(MT=MT, SHW=shw, tiles_max=1, vec_a=Wp % 4 == 0, wblocks=ceil_div(Wp, SEG), hblocks=ceil_div(Hp, TH))
                claim = "MT %d SHW %d: Wp = SEG%+d (%s A loads), Hp %d of TH %d, CB %d" % (MT, shw, dw, "128-bit" if Wp % 4 == 0 else "32-bit", Hp, TH, CB)
                name = "wg-%s-a%d_b%d-s%d%d-d%dh%dw%d-n%d%s" % (orient[0], CA, CB, sd, shw, Dp, Hp, Wp, nb, "-short" if short else "")
                out.append(_wg(name, orient, nb, CA, CB, Dp, Hp, Wp, (sd, shw), short, want, claim))
                k += 1
    return out


def _wg_multi_cases():
    """Per (MT, SHW) one launch in which blocks own 3 and 2 tiles (CB = 64: 16 channel chunks, gy = 32), random and integer operands:
        MT 4, shw 1: CA 64, nb 2, Dp 6, Hp 13 (TH 2: 7), Wp 8        84 tiles = 2 * 32 + 20
        MT 3, shw 1: CA 40, nb 2, Dp 6, Hp 13, Wp 9                  84
        MT 2, shw 1: CA 24, nb 2, Dp 7, Hp 9 (TH 4: 3), Wp 65 (2)    84
        MT 1, shw 1: CA 16, nb 2, Dp 7, Hp 17 (TH 8: 3), Wp 65 (2)   84
        shw 2 (TH 4, SEG 32): nb 2, Dp 6, Hp 9 (3), Wp 33 (2)        72 = 2 * 32 + 8"""
    shapes = {(4, 1): (64, 2, 6, 13, 8), (3, 1): (40, 2, 6, 13, 9), (2, 1): (24, 2, 7, 9, 65), (1, 1): (16, 2, 7, 17, 65),
              (4, 2): (64, 2, 6, 9, 33), (3, 2): (48, 2, 6, 9, 33), (2, 2): (32, 2, 6, 9, 33), (1, 2): (8, 2, 6, 9, 33)}
    out = []
    for (MT, shw), (CA, nb, Dp, Hp, Wp) in sorted(shapes.items()):
        sd = 1 + (MT % 2)
        for data in ("randn", "int"):
            orient = "conv" if data == "randn" else "deconv"
            want = dict(MT=MT, SHW=shw, tiles_max=3, tiles_min=2, gy=32)
            out.append(_wg("wgm-mt%d-shw%d-%s" % (MT, shw, data), orient, nb, CA, 64, Dp, Hp, Wp, (sd, shw), orient == "conv", want,
                           "MT %d SHW %d: blocks own 3 and 2 tiles%s" % (MT, shw, ", exact" if data == "int" else ""), data))
    return out


WG_EDGE_CASES = _wg_edge_cases()
WG_MULTI_CASES = _wg_multi_cases()
# the first kernel's row loop: CB = 256 -> 64 channel chunks, gy = min(1024 / 64, ..) = 16; rows = 2 * 6 * 13 = 156 > 4 gy = 64: 3 rounds
WG_V1_ROWS_CASE = _wg("wgv1-rows156-gy16", "conv", 2, 16, 256, 6, 13, 8, (1, 1), False, dict(), "V1: rows 156 > 4 gy = 64")
WG_CASES = WG_EDGE_CASES + WG_MULTI_CASES + [WG_V1_ROWS_CASE]
WG_CASE = {c.name: c for c in WG_CASES}
assert len(WG_CASE) == len(WG_CASES)
WG_V1_CASES = WG_CASES                        # the first kernel runs every edge and multi-tile case of the tiled one, and its own row-loop case


def wg_plan(c):
    return plan_wgrad(c.nb, c.CA, c.CB, c.Dp, c.Hp, c.Wp, c.stride[1])


def bt_dims(c):
    def dim(p, s):
        return p if s == 1 else 2 * p - (1 if c.short else 0)
    return dim(c.Dp, c.stride[0]), dim(c.Hp, c.stride[1]), dim(c.Wp, c.stride[1])


@functools.lru_cache(maxsize=None)
def wg_inputs(name):
    """``A [nb,CA,Dp,Hp,Wp]``, ``Bt [nb,CB,Db,Hb,Wb]`` fp32, as ``ops.conv3d_wgrad`` takes them."""
    c = WG_CASE[name]
    g = _gen(c.name)
    Db, Hb, Wb = bt_dims(c)
    if c.data == "int":
        return (torch.randint(-3, 4, (c.nb, c.CA, c.Dp, c.Hp, c.Wp), generator=g).float(),
                torch.randint(-3, 4, (c.nb, c.CB, Db, Hb, Wb), generator=g).float())
    return torch.randn(c.nb, c.CA, c.Dp, c.Hp, c.Wp, generator=g), torch.randn(c.nb, c.CB, Db, Hb, Wb, generator=g)


def wgrad_sum(A, Bt, stride, dtype=torch.float64):
    """``dW[a][b][kd][kh][kw] = sum_{n,p} A[n][a][p] Bt[n][b][p s - 1 + k]`` (zero outside ``Bt``) as plain sums in ``dtype``.  With
    ``A = dY, Bt = X`` this is ``nn.Conv3d.weight.grad`` ``[Cout,Cin,3,3,3]``, with ``A = X, Bt = dY`` ``nn.ConvTranspose3d.weight.grad``
    ``[Cin,Cout,3,3,3]`` (the two orientations of csrc/wgrad.hip)."""
    A, Bt = A.to(dtype), Bt.to(dtype)
    N, CA, Dp, Hp, Wp = A.shape
    _, CB, Db, Hb, Wb = Bt.shape
    s = (stride[0], stride[1], stride[1])
    need = [(p - 1) * st + 3 for p, st in zip((Dp, Hp, Wp), s)]
    hi = [max(0, n - 1 - d) for n, d in zip(need, (Db, Hb, Wb))]
    Bp = F.pad(Bt, (1, hi[2], 1, hi[1], 1, hi[0]))
    dW = torch.zeros(CA, CB, 3, 3, 3, dtype=dtype)
    for kd, kh, kw in itertools.product(range(3), repeat=3):
        Bs = Bp[:, :, kd:kd + (Dp - 1) * s[0] + 1:s[0], kh:kh + (Hp - 1) * s[1] + 1:s[1], kw:kw + (Wp - 1) * s[2] + 1:s[2]]
        dW[:, :, kd, kh, kw] = torch.einsum("nadhw,nbdhw->ab", A, Bs)
    return dW


@functools.lru_cache(maxsize=None)
def wg_expect(name):
    c = WG_CASE[name]
    A, Bt = wg_inputs(name)
    ref = wgrad_sum(A, Bt, c.stride)
    S = wgrad_sum(A.abs(), Bt.abs(), c.stride)
    if c.data == "int":
        assert S.max().item() < 2 ** 24
        return ref, torch.zeros_like(ref)
    return ref, C_ACC * (c.nb * c.Dp * c.Hp * c.Wp) * U32 * S


def wg_tile_region(c, tile):
    """Tile index -> ``(n, d, row slice, column slice)`` of ``A``, decoded as ``fetch`` of ``wgrad_tiled_kernel`` decodes ``tl``."""
    p = wg_plan(c)
    w0 = (tile % p.wblocks) * p.SEG
    h0 = ((tile // p.wblocks) % p.hblocks) * p.TH
    d = (tile // (p.wblocks * p.hblocks)) % c.Dp
    n = tile // (p.wblocks * p.hblocks * c.Dp)
    return n, d, slice(h0, min(h0 + p.TH, c.Hp)), slice(w0, min(w0 + p.SEG, c.Wp))


# ===================================================================================================================== guards
def guarded(t, fill):
    """``t [B,C,D,H,W]`` -> ``(view, buffer)``: the same values in the middle of a flat buffer with one D plane (H W elements) of ``fill``
    before and behind it; the view is contiguous and keeps every alignment a row of W elements has."""
    plane = t.shape[-1] * t.shape[-2]
    buf = torch.full((t.numel() + 2 * plane,), fill, dtype=t.dtype, device=t.device)
    view = buf[plane:plane + t.numel()].view(t.shape)
    view.copy_(t)
    return view, buf


def guards_intact(buf, numel, plane, fill=GUARD):
    b = buf.detach().cpu()
    return bool((b[:plane] == fill).all()) and bool((b[plane + numel:] == fill).all()) and b.numel() == numel + 2 * plane


# ===================================================================================================================== mutations
# Each returns what a subtly wrong kernel would have produced, built from the reference's own arithmetic (float64), never from a kernel.
def mutate_drop_tap(c, b, o, tap):
    """conv / dgrad / wino kinds: the output without tap ``(kd, kh, kw)`` (of the convolution that is run) at output voxel ``o``."""
    c = _get(c)
    t = case_inputs(c)
    assert c.kind != "deconv" and not (c.scale or c.relu or c.residual)
    w = conv_weight(c, t["w"]).double()
    i = [ov * s - 1 + k for ov, s, k in zip(o, (c.stride[0], c.stride[1], c.stride[1]), tap)]
    assert all(0 <= v < n for v, n in zip(i, (c.D, c.H, c.W))), "the dropped tap must exist"
    ref = expect(c)[0].clone()
    ref[b, :, o[0], o[1], o[2]] -= w[:, :, tap[0], tap[1], tap[2]] @ t["x"].double()[b, :, i[0], i[1], i[2]]
    return ref


def mutate_drop_tap_deconv(c, b, i, tap):
    """deconv: the output without the contribution of input voxel ``i`` through tap ``(kd, kh, kw)``."""
    c = _get(c)
    t = case_inputs(c)
    assert c.kind == "deconv" and not (c.scale or c.relu or c.residual)
    o = [iv * s - 1 + k for iv, s, k in zip(i, (c.stride[0], 2, 2), tap)]
    assert all(0 <= v < n for v, n in zip(o, out_dims(c)))
    ref = expect(c)[0].clone()
    ref[b, :, o[0], o[1], o[2]] -= t["w"].double()[:, :, tap[0], tap[1], tap[2]].t() @ t["x"].double()[b, :, i[0], i[1], i[2]]
    return ref


def mutate_shift_halo_column(c, tile_w0, TW):
    """One tile's right halo column read one column too far left: output columns of the tile ``[tile_w0, tile_w0 + TW)`` are computed from
    an input whose first column behind the tile repeats the column before it; the other tiles are untouched."""
    c = _get(c)
    t = case_inputs(c)
    Wo = out_dims(c)[2]
    last = min(tile_w0 + TW, Wo) - 1
    if c.kind == "deconv":                                     # input coordinates: the +1 halo column of the 32-column tile
        halo, cols = min(tile_w0 + TW, c.W - 1), slice(2 * tile_w0, min(2 * (tile_w0 + TW), Wo))
    else:
        halo, cols = last * c.stride[1] + 1, slice(tile_w0, last + 1)
    assert 1 <= halo < c.W, "the halo column must exist"
    x = t["x"].clone()
    x[..., halo] = x[..., halo - 1]
    ref = expect(c)[0].clone()
    ref[..., cols] = evaluate(c, x=x)[..., cols]
    return ref


def mutate_drop_row_end(c, tile_w0, TW):
    """The last voxel of one tile row (first batch item, channel, depth and row) left at 0."""
    c = _get(c)
    ref = expect(c)[0].clone()
    ref[0, 0, 0, 0, min(tile_w0 + TW, ref.shape[-1]) - 1] = 0
    return ref


def mutate_swap_channels(ref):
    """Output channels (rows of ``dW``) 15 and 16 exchanged."""
    assert ref.shape[1 if ref.dim() == 5 and ref.shape[-1] != 3 else 0] > 16
    ref = ref.clone()
    if ref.shape[-3:] == (3, 3, 3):
        ref[[15, 16]] = ref[[16, 15]]
    else:
        ref[:, [15, 16]] = ref[:, [16, 15]]
    return ref


def mutate_wg_drop_voxels(name, regions):
    c = WG_CASE[name]
    A, Bt = wg_inputs(name)
    A = A.clone()
    for n, d, h, w in regions:
        A[n, :, d, h, w] = 0
    return wgrad_sum(A, Bt, c.stride)


def mutate_wg_drop_tap(name, tap):
    ref = wg_expect(name)[0].clone()
    ref[:, :, tap[0], tap[1], tap[2]] = 0
    return ref


def mutate_wg_drop_row_end(name, tile=0):
    """The last voxel of the first row of a tile missing from the sum."""
    n, d, h, w = wg_tile_region(WG_CASE[name], tile)
    return mutate_wg_drop_voxels(name, [(n, d, h.start, w.stop - 1)])


def mutate_wg_shift_halo_column(name, tile=0):
    """The Bt column just right of a tile's own columns (its kw = 2 halo) replaced by its left neighbour, for that tile's voxels only."""
    c = WG_CASE[name]
    A, Bt = wg_inputs(name)
    n, d, h, w = wg_tile_region(c, tile)
    halo = (w.stop - 1) * c.stride[1] + 1
    assert 1 <= halo < Bt.shape[-1]
    keep = torch.zeros_like(A)
    keep[n, :, d, h, w] = 1
    B2 = Bt.clone()
    B2[..., halo] = B2[..., halo - 1]
    return wgrad_sum(A * (1 - keep), Bt, c.stride) + wgrad_sum(A * keep, B2, c.stride)


def mutate_wg_skip_second_tile(name):
    """Block 0's second tile (tile index gy) skipped."""
    c = WG_CASE[name]
    p = wg_plan(c)
    assert p.tiles_max >= 2
    return mutate_wg_drop_voxels(name, [wg_tile_region(c, p.gy)])
