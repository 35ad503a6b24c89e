"""The cost-volume training op (``ops.cv_aggregate(exact=True)`` forward, ``ops.cv_aggregate_bwd`` in its three forms ``direct`` / ``lds`` /
``own``, ``autograd.AggregateFn``) against a float64 reference of the same op, at the edges of the kernels' tilings.

The reference (``cv_train_ref``) is a pure function of exactly what the kernels receive - channel-last features, the float32 ``rt`` rows,
hypotheses, visibility weights, the upstream gradient - written dtype-generically in torch: coordinates as ``oracle/ref_torch.py``'s
``sweep_coordinates`` (including the round trip through normalised coordinates), the bilinear / zeros / ``align_corners=True`` sample as four
explicit gathers, ``group_correlation``, the weighted mean with ``+1e-6``; no gradient through the grid or the hypotheses; gradients by autograd.
Evaluated in float64 it is the reference, in float32 the yardstick.  ``tests/test_cv_train_edge_refs.py`` (CPU) pins it to autograd through
``ref_torch.homo_warping_3D_with_mask`` + ``group_correlation``, checks the table below and what the cases claim to exercise, and shows that
four subtly wrong backwards would fail these bounds.

Tolerances.  ``DEV32[case] = (volume, dfeat, dweight)`` is the max-norm deviation of the float32 CPU evaluation of the reference from the
float64 one relative to max|reference|, from ``measure_dev32()``.  The kernel is the same arithmetic in another summation order (and atomics add
their own order), so it is held to ``4 x DEV32`` of its case - the margin of ``test_hip_loss_edges.py`` - with DEV32 floored where it came out
luckily small, and never looser than what ``test_aggregate_fn_grads`` holds (1e-4 volume, 2e-4 gradients):

    bound = min(CAP, 4 * max(DEV32, U32 * sqrt(n)))        U32 = 2^-24, float32 unit roundoff

The floor: a float32 sum of n terms commits n roundings, each at most U32 times the running partial sum; the partial sums are of the size of
the result (they are what the max-norm scale measures), and roundings of independent sign accumulate like a random walk, so the expected error
of such a sum is ~ U32 * sqrt(n) of the result (Higham, Accuracy and Stability of Numerical Algorithms, 2.8; the worst case U32 * n is never
seen with data of mixed sign).  n is the longest sum behind one element of the output, counted per case in ``longest_sums``:
    volume   4 taps * CPG channels * (V - 1) views
    dfeat    the larger of 4 taps * D planes * (V - 1) views (reference view) and the largest number of taps that land on one source texel
             (counted on the reference: H * W * D in the fully degenerate case)
    dweight  4 taps * C channels * D planes (sum_{g,d} G * ip_v)
The criterion is the max norm over ALL elements.

``dweight`` with one source view (V = 2): volume_mean = in_prod * w / (w + 1e-6), so d volume / d w = in_prod * 1e-6 / (w + 1e-6)^2 - the two
terms sum G*ip_v / S and T / S of the kernel (and of autograd) cancel to ~1e-6 of their size, and max|dweight| says nothing about the
arithmetic.  For V = 2, DEV32 and the kernel's deviation of ``dweight`` are therefore relative to max|sum_{g,d} G * ip_v| / S, the size of the
terms that cancel.

Degenerate geometry where z crosses zero stays out of this comparison (division by z + 1e-6 is discontinuous there):
``test_aggregate_bwd_own_near_singular_projection`` covers it kernel against kernel.  ``test_cases_avoid_z_near_zero`` keeps z > 0.25 here."""
import collections
import functools
import math

import pytest
import torch

G = 8
U32 = 2.0 ** -24
CAP = {"volume": 1e-4, "dfeat": 2e-4, "dweight": 2e-4}        # what test_aggregate_fn_grads holds; no case may need more
OUTPUTS = ("volume", "dfeat", "dweight")
QCAP = 128                                                    # OW_QCAP of cost_volume_bwd.hip

Case = collections.namedtuple("Case", "name geom B V C D H W bf16 guard")

# name                      geometry  B  V  C   D   H   W
#   synth       DTU-like rig (mvsformer_amd.synth), another scene and another hypothesis jitter (+-20 %) per batch entry
#   border      hand-written rt: the source shows the reference magnified 1.25x - 1.4x about its centre, sheared: 50.5 % of the samples have a
#               2 x 2 footprint that is not wholly inside the source image (taps with weight 0, half-valid footprints, clamped offsets),
#               36.0 % lie wholly outside, on all four sides (test_border_case_leaves_the_image_on_every_side)
#   minify      hand-written rt: ix = 0.25 x + c + t / d - an 8 x 4 tile's 32 pixels share ~3 x 2 footprint origins per plane
#   degenerate  hand-written rt with rotation columns 0 and 1 zero: every pixel of a plane maps to ONE sub-pixel position (views 1, 3: the same
#               for all planes; view 2: moving with the plane) - 32 lanes contend for one origin
#   wild        synth rig, hypotheses jittered by +-40 % per pixel: taps all over the source image, most of them outside a 8 x 4 window
CASES = [
    Case("v2-c8-d1-3x5-b2", "synth", 2, 2, 8, 1, 3, 5, False, False),
    Case("v3-c16-d7-4x8-b1", "synth", 1, 3, 16, 7, 4, 8, False, False),
    Case("v3-c16-d7-4x8-b1-bf16grad", "synth", 1, 3, 16, 7, 4, 8, True, False),
    Case("v5-c32-d8-5x9-b3", "synth", 3, 5, 32, 8, 5, 9, False, False),
    Case("v7-c8-d9-4x16-b1", "synth", 1, 7, 8, 9, 4, 16, False, False),
    Case("v7-c64-d17-5x17-b2", "synth", 2, 7, 64, 17, 5, 17, False, False),
    Case("border-v3-c16-d9-13x19-b2", "border", 2, 3, 16, 9, 13, 19, False, True),
    Case("minify-v3-c32-d8-8x17-b1", "minify", 1, 3, 32, 8, 8, 17, False, True),
    Case("degenerate-v4-c8-d9-6x10-b1", "degenerate", 1, 4, 8, 9, 6, 10, False, True),
    Case("wild-v3-c16-d17-8x16-b1", "wild", 1, 3, 16, 17, 8, 16, False, True),
]
CASE = {c.name: c for c in CASES}
AUTOGRAD_CASE = "v5-c32-d8-5x9-b3"                            # through autograd.AggregateFn, channels-first in and out
MISSQ_CASE = "wild-v3-c16-d17-8x16-b1"

# (volume, dfeat, dweight) from measure_dev32(); test_cv_train_edge_refs.py asserts that the table still is what the helper measures
DEV32 = {
    "v2-c8-d1-3x5-b2": (2.8e-07, 2.7e-07, 1.5e-07),
    "v3-c16-d7-4x8-b1": (9.0e-07, 7.5e-07, 9.6e-07),
    "v3-c16-d7-4x8-b1-bf16grad": (9.0e-07, 7.8e-07, 7.3e-07),
    "v5-c32-d8-5x9-b3": (1.5e-06, 7.5e-07, 1.1e-06),
    "v7-c8-d9-4x16-b1": (1.6e-06, 1.9e-06, 1.5e-06),
    "v7-c64-d17-5x17-b2": (2.1e-06, 1.7e-06, 2.4e-06),
    "border-v3-c16-d9-13x19-b2": (4.3e-06, 2.3e-06, 2.6e-06),
    "minify-v3-c32-d8-8x17-b1": (7.3e-07, 8.5e-07, 9.3e-07),
    "degenerate-v4-c8-d9-6x10-b1": (9.3e-07, 7.7e-07, 1.5e-06),
    "wild-v3-c16-d17-8x16-b1": (2.7e-06, 1.4e-06, 1.1e-06),
}

MODES = [("direct", None), ("lds", None), ("own", None), ("own", "3,4")]

# Recorded on an MI355X with the table above (deviation from float64 per case, output and backward form; the volume is the same launch in all):
#   v2-c8-d1-3x5-b2                volume   bound 1.1e-06   direct 2.84e-07  lds 2.84e-07  own 2.84e-07  own 3,4 2.84e-07
#   v2-c8-d1-3x5-b2                dfeat    bound 1.1e-06   direct 3.28e-07  lds 3.28e-07  own 3.28e-07  own 3,4 3.28e-07
#   v2-c8-d1-3x5-b2                dweight  bound 1.3e-06   direct 7.60e-08  lds 7.60e-08  own 7.60e-08  own 3,4 7.60e-08
#   v3-c16-d7-4x8-b1               volume   bound 3.6e-06   direct 8.99e-07  lds 8.99e-07  own 8.99e-07  own 3,4 8.99e-07
#   v3-c16-d7-4x8-b1               dfeat    bound 3.0e-06   direct 7.50e-07  lds 7.50e-07  own 7.50e-07  own 3,4 7.50e-07
#   v3-c16-d7-4x8-b1               dweight  bound 5.0e-06   direct 8.63e-07  lds 8.06e-07  own 8.06e-07  own 3,4 8.06e-07
#   v3-c16-d7-4x8-b1-bf16grad      volume   bound 3.6e-06   direct 8.99e-07  lds 8.99e-07  own 8.99e-07  own 3,4 8.99e-07
#   v3-c16-d7-4x8-b1-bf16grad      dfeat    bound 3.1e-06   direct 7.57e-07  lds 7.57e-07  own 7.57e-07  own 3,4 7.57e-07
#   v3-c16-d7-4x8-b1-bf16grad      dweight  bound 5.0e-06   direct 8.09e-07  lds 8.09e-07  own 8.09e-07  own 3,4 8.09e-07
#   v5-c32-d8-5x9-b3               volume   bound 6.0e-06   direct 1.49e-06  lds 1.49e-06  own 1.49e-06  own 3,4 1.49e-06  AggregateFn 1.49e-06
#   v5-c32-d8-5x9-b3               dfeat    bound 3.0e-06   direct 8.30e-07  lds 8.30e-07  own 8.30e-07  own 3,4 8.30e-07  AggregateFn 8.30e-07
#   v5-c32-d8-5x9-b3               dweight  bound 7.6e-06   direct 1.11e-06  lds 1.11e-06  own 1.11e-06  own 3,4 1.11e-06  AggregateFn 1.11e-06
#   v7-c8-d9-4x16-b1               volume   bound 6.4e-06   direct 1.62e-06  lds 1.62e-06  own 1.62e-06  own 3,4 1.62e-06
#   v7-c8-d9-4x16-b1               dfeat    bound 7.6e-06   direct 1.77e-06  lds 1.77e-06  own 1.77e-06  own 3,4 1.77e-06
#   v7-c8-d9-4x16-b1               dweight  bound 6.0e-06   direct 1.45e-06  lds 1.45e-06  own 1.45e-06  own 3,4 1.45e-06
#   v7-c64-d17-5x17-b2             volume   bound 8.4e-06   direct 2.12e-06  lds 2.12e-06  own 2.12e-06  own 3,4 2.12e-06
#   v7-c64-d17-5x17-b2             dfeat    bound 6.8e-06   direct 1.66e-06  lds 1.66e-06  own 1.66e-06  own 3,4 1.66e-06
#   v7-c64-d17-5x17-b2             dweight  bound 1.6e-05   direct 2.52e-06  lds 2.45e-06  own 2.45e-06  own 3,4 2.45e-06
#   border-v3-c16-d9-13x19-b2      volume   bound 1.7e-05   direct 4.35e-06  lds 4.35e-06  own 4.35e-06  own 3,4 4.35e-06
#   border-v3-c16-d9-13x19-b2      dfeat    bound 9.2e-06   direct 2.33e-06  lds 2.33e-06  own 2.33e-06  own 3,4 2.33e-06
#   border-v3-c16-d9-13x19-b2      dweight  bound 1.0e-05   direct 2.66e-06  lds 2.60e-06  own 2.60e-06  own 3,4 2.60e-06
#   minify-v3-c32-d8-8x17-b1       volume   bound 2.9e-06   direct 7.29e-07  lds 7.29e-07  own 7.29e-07  own 3,4 7.29e-07
#   minify-v3-c32-d8-8x17-b1       dfeat    bound 5.2e-06   direct 7.00e-07  lds 8.46e-07  own 8.06e-07  own 3,4 8.06e-07
#   minify-v3-c32-d8-8x17-b1       dweight  bound 7.6e-06   direct 8.93e-07  lds 8.93e-07  own 8.93e-07  own 3,4 8.93e-07
#   degenerate-v4-c8-d9-6x10-b1    volume   bound 3.7e-06   direct 9.25e-07  lds 9.25e-07  own 9.25e-07  own 3,4 9.25e-07
#   degenerate-v4-c8-d9-6x10-b1    dfeat    bound 5.5e-06   direct 3.41e-07  lds 5.10e-07  own 3.45e-07  own 3,4 3.45e-07
#   degenerate-v4-c8-d9-6x10-b1    dweight  bound 6.0e-06   direct 1.45e-06  lds 1.45e-06  own 1.45e-06  own 3,4 1.45e-06
#   wild-v3-c16-d17-8x16-b1        volume   bound 1.1e-05   direct 2.69e-06  lds 2.69e-06  own 2.69e-06  own 3,4 2.69e-06
#   wild-v3-c16-d17-8x16-b1        dfeat    bound 5.6e-06   direct 1.39e-06  lds 1.47e-06  own 1.43e-06  own 3,4 1.43e-06
#   wild-v3-c16-d17-8x16-b1        dweight  bound 7.9e-06   direct 1.00e-06  lds 1.03e-06  own 1.03e-06  own 3,4 1.03e-06
# stats of the wild case with the 8 x 4 window: 60204 taps = 15051 (reference) x 4 lanes, 19196 of them missed the window, over 16 queues.


# ------------------------------------------------------------------------------------------------------------------- the reference
def sweep_taps_ref(rt_v, hyp, H, W, dtype):
    """``rt_v [B,12]``, ``hyp [B,D,H,W]`` -> the four bilinear taps of every sample, in ``dtype``: ``idx`` 4 x ``[B,D,HW]`` (clamped in
    bounds), ``wgt`` 4 x ``[B,D,HW]`` (0 outside the image), the footprint origin ``x0, y0``, the source-camera ``z`` and the fractions ``wx, wy``.  Order of
    operations of ``ref_torch.sweep_coordinates`` and of ``grid_sample(align_corners=True)``; taps ordered 00, 01 (x+1), 10 (y+1), 11."""
    B, D = hyp.shape[0], hyp.shape[1]
    r = rt_v.to(dtype)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    x, y = xs.reshape(1, 1, -1), ys.reshape(1, 1, -1)

    def c(i):
        return r[:, i].reshape(B, 1, 1)

    dep = hyp.to(dtype).reshape(B, D, -1)
    X = [(c(3 * k) * x + c(3 * k + 1) * y + c(3 * k + 2)) * dep + c(9 + k) for k in range(3)]
    zz = X[2] + 1e-6
    un = (X[0] / zz) / ((W - 1) / 2) - 1
    vn = (X[1] / zz) / ((H - 1) / 2) - 1
    ix = ((un + 1) / 2) * (W - 1)
    iy = ((vn + 1) / 2) * (H - 1)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx, wy = ix - x0, iy - y0
    ex, ey = 1 - wx, 1 - wy
    idx, wgt = [], []
    for dy, dx, w in ((0, 0, ey * ex), (0, 1, ey * wx), (1, 0, wy * ex), (1, 1, wy * wx)):
        xx, yy = x0 + dx, y0 + dy
        valid = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
        idx.append(yy.clamp(0, H - 1).long() * W + xx.clamp(0, W - 1).long())
        wgt.append(torch.where(valid, w, torch.zeros_like(w)))
    return idx, wgt, x0.long(), y0.long(), X[2], wx, wy


Ref = collections.namedtuple("Ref", "volume dfeat dweight dw_scale ip")


def cv_train_ref(feat_cl, rt, hyp, weight, R, dtype, taps_fn=sweep_taps_ref):
    """``feat_cl [B,V,H,W,C]``, ``rt [B,V-1,12]``, ``hyp [B,D,H,W]``, ``weight [B,V-1,H,W]``, upstream gradient ``R [B,G,D,H,W]`` ->
    ``volume [B,G,D,H,W]``, ``dfeat [B,V,H,W,C]``, ``dweight [B,V-1,H,W]``, all in ``dtype``.  ``dw_scale``: max|sum_{g,d} R * ip_v| / S,
    the size of the two terms whose difference is ``dweight`` (module docstring, V = 2); ``ip``: the per-view correlations."""
    B, V, H, W, C = feat_cl.shape
    D, HW, CPG = hyp.shape[1], H * W, C // G
    f = feat_cl.detach().to(dtype).requires_grad_(True)
    w = weight.detach().to(dtype).requires_grad_(True)
    Rd = R.detach().to(dtype)
    ref = f[:, 0].reshape(B, 1, HW, G, CPG)
    vol_sum, w_sum, ips = 0.0, 0.0, []
    for v in range(V - 1):
        with torch.no_grad():
            idx, wgt = taps_fn(rt[:, v], hyp, H, W, dtype)[:2]
        src = f[:, v + 1].reshape(B, HW, C)
        warped = 0.0
        for k in range(4):
            tap = torch.gather(src, 1, idx[k].reshape(B, D * HW, 1).expand(-1, -1, C)).reshape(B, D, HW, C)
            warped = warped + tap * wgt[k].unsqueeze(-1)
        ip = (ref * warped.reshape(B, D, HW, G, CPG)).mean(dim=-1).permute(0, 3, 1, 2).reshape(B, G, D, H, W)
        ips.append(ip.detach())
        vol_sum = vol_sum + ip * w[:, v].reshape(B, 1, 1, H, W)
        w_sum = w_sum + w[:, v]
    vol = vol_sum / (w_sum.reshape(B, 1, 1, H, W) + 1e-6)
    (vol * Rd).sum().backward()
    S = w_sum.detach() + 1e-6
    dw_scale = max(((Rd * ip).sum(dim=(1, 2)) / S).abs().max().item() for ip in ips)
    return Ref(vol.detach(), f.grad, w.grad, dw_scale, ips)


# ----------------------------------------------------------------------------------------------------------------------- the cases
def rt_from_proj(proj):
    """``proj [B,V,2,4,4]`` -> ``rt [B,V-1,12]`` in float32, the way the oracle forms its matrices (``src_proj @ inverse(ref_proj)``)."""
    from oracle import ref_torch
    ref_P = ref_torch.compose_projection(proj[:, 0])
    rows = []
    for v in range(1, proj.shape[1]):
        M = torch.matmul(ref_torch.compose_projection(proj[:, v]), torch.inverse(ref_P))
        rows.append(torch.cat([M[:, :3, :3].reshape(-1, 9), M[:, :3, 3]], dim=1))
    return torch.stack(rows, dim=1).contiguous()


def _hand_rt(rows):
    return torch.tensor(rows, dtype=torch.float32).reshape(1, len(rows), 12)


def synth_geometry(c, gen, jitter):
    from mvsformer_amd import synth
    rts, hyps, projs = [], [], []
    for b in range(c.B):
        scene = synth.make_scene(c.V, c.H * 8, c.W * 8, seed=c.C + c.D + 17 * b)
        proj = synth.proj_matrices(scene, (8,))["stage1"]
        z = synth.plane_depth(scene, 8)
        hyp = 1.0 / (1.0 / z[None, None] + torch.linspace(-1, 1, c.D).view(1, c.D, 1, 1) * (4e-5 + 2e-5 * b))
        hyps.append(hyp * (1.0 - jitter + 2.0 * jitter * torch.rand(hyp.shape, generator=gen)))
        rts.append(rt_from_proj(proj))
        projs.append(proj)
    return torch.cat(rts), torch.cat(hyps).float().contiguous(), torch.cat(projs)


def hand_geometry(c, gen):
    """z = d for every hand-written ``rt`` (third rotation row 0 0 1, no translation along z), d in (1, 2)."""
    H, W, D = c.H, c.W, c.D
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    if c.geom == "border":
        def view(sx, sy, shx, shy, tx, ty):                  # ix = cx + sx (x - cx) + shx (y - cy) + tx / d
            return [sx, shx, cx - sx * cx - shx * cy, shy, sy, cy - sy * cy - shy * cx, 0, 0, 1, tx, ty, 0]
        rts = [_hand_rt([view(1.35, 1.3, 0.15, -0.1, 1.1, -0.7), view(1.25, 1.4, -0.2, 0.12, -0.9, 1.3)]),
               _hand_rt([view(1.4, 1.3, 0.1, 0.2, -1.4, 0.8), view(1.3, 1.35, -0.12, -0.18, 0.6, -1.2)])]
        rt = torch.cat(rts[:c.B])
    elif c.geom == "minify":
        rt = _hand_rt([[0.25, 0.0, 3.3, 0.0, 0.25, 2.2, 0, 0, 1, 0.8, 0.6, 0],
                       [0.25, 0.02, 5.15, -0.015, 0.25, 1.4, 0, 0, 1, -1.1, 0.9, 0]])
    else:                                                     # degenerate
        rt = _hand_rt([[0, 0, 4.37, 0, 0, 2.61, 0, 0, 1, 0, 0, 0],
                       [0, 0, 2.18, 0, 0, 1.77, 0, 0, 1, 3.1, 1.9, 0],
                       [0, 0, 6.83, 0, 0, 3.29, 0, 0, 1, 0, 0, 0]])
    assert rt.shape == (c.B, c.V - 1, 12)
    planes = torch.linspace(1.05, 1.9, D).view(1, D, 1, 1) if D > 1 else torch.full((1, 1, 1, 1), 1.5)
    hyp = planes * (0.97 + 0.06 * torch.rand(c.B, D, H, W, generator=gen))
    return rt.contiguous(), hyp.float().contiguous(), None


@functools.lru_cache(maxsize=None)
def build_case(name):
    """CPU float32 inputs of a case (shared, never modified): ``feat_cl, rt, hyp, weight, R`` and, for the synth rigs, ``proj``."""
    c = CASE[name]
    gen = torch.Generator().manual_seed(1000 * c.B + 100 * c.V + c.C + c.D + c.H * c.W)
    if c.geom in ("synth", "wild"):
        rt, hyp, proj = synth_geometry(c, gen, 0.4 if c.geom == "wild" else 0.2)
    else:
        rt, hyp, proj = hand_geometry(c, gen)
    feat_cl = torch.randn(c.B, c.V, c.H, c.W, c.C, generator=gen)
    weight = torch.rand(c.B, c.V - 1, c.H, c.W, generator=gen) * 0.8 + 0.1
    R = torch.randn(c.B, G, c.D, c.H, c.W, generator=gen)
    if c.bf16:
        R = R.bfloat16().float()                              # the gradient the bf16 regularizer hands back; the reference sees the same values
    return dict(feat_cl=feat_cl, rt=rt, hyp=hyp, weight=weight, R=R, proj=proj)


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    t = build_case(name)
    return cv_train_ref(t["feat_cl"], t["rt"], t["hyp"], t["weight"], t["R"], dtype)


@functools.lru_cache(maxsize=None)
def tap_census(name, dtype=torch.float64):
    """What the taps of a case do, counted on the reference: ``taps`` = non-zero-weight taps (what ``stats[0]`` counts per lane),
    ``fragile`` = samples within 1e-4 px of a texel row / column (a tap there may have weight exactly 0 in one precision and not in the
    other), ``partial`` / ``outside`` = share of samples whose 2 x 2 footprint is not wholly / not at all inside the source image,
    ``hits`` = most non-zero-weight taps on one source texel, ``zmin``, and ``sides`` = samples beyond each image side (l, r, t, b)."""
    c, t = CASE[name], build_case(name)
    taps = fragile = partial = outside = samples = hits = 0
    zmin, sides = math.inf, [0, 0, 0, 0]
    for v in range(c.V - 1):
        idx, wgt, x0, y0, z, wx, wy = sweep_taps_ref(t["rt"][:, v], t["hyp"], c.H, c.W, dtype)
        nz = torch.stack([w != 0 for w in wgt])
        taps += int(nz.sum())
        n_in = torch.stack([w > 0 for w in wgt]).sum(0)
        inb = (x0 >= 0) & (x0 + 1 <= c.W - 1) & (y0 >= 0) & (y0 + 1 <= c.H - 1)
        partial += int((~inb).sum())
        outside += int((n_in == 0).sum())
        samples += x0.numel()
        zmin = min(zmin, z.min().item())
        for frac in (wx, wy):
            fragile += int(((frac < 1e-4) | (frac > 1 - 1e-4)).sum())
        for i, m in enumerate((x0 + 1 < 0, x0 > c.W - 1, y0 + 1 < 0, y0 > c.H - 1)):
            sides[i] += int(m.sum())
        for b in range(c.B):
            cnt = torch.zeros(c.H * c.W, dtype=torch.long)
            for k in range(4):
                cnt.scatter_add_(0, idx[k][b].reshape(-1), nz[k][b].reshape(-1).long())
            hits = max(hits, int(cnt.max()))
    return dict(taps=taps, fragile=fragile, partial=partial / samples, outside=outside / samples, hits=hits, zmin=zmin, sides=sides)


def longest_sums(name):
    """n of the module docstring per output."""
    c = CASE[name]
    return dict(volume=4 * (c.C // G) * (c.V - 1), dfeat=max(4 * c.D * (c.V - 1), tap_census(name)["hits"]), dweight=4 * c.C * c.D)


def scales(name):
    """What a deviation of each output is relative to: max|reference|, except ``dweight`` with one source view (module docstring)."""
    r = reference(name)
    return dict(volume=r.volume.abs().max().item(), dfeat=r.dfeat.abs().max().item(),
                dweight=r.dw_scale if CASE[name].V == 2 else r.dweight.abs().max().item())


def deviation(name, volume, dfeat, dweight):
    """max|got - reference| / scale per output, over all elements."""
    r, s = reference(name), scales(name)
    return {k: (torch.as_tensor(g).detach().cpu().double() - getattr(r, k)).abs().max().item() / s[k]
            for k, g in (("volume", volume), ("dfeat", dfeat), ("dweight", dweight))}


def measure_dev32(names=None):
    """CPU only: the DEV32 table for ``names`` (all cases by default)."""
    out = {}
    for name in names or [c.name for c in CASES]:
        r32 = reference(name, torch.float32)
        d = deviation(name, r32.volume, r32.dfeat, r32.dweight)
        out[name] = tuple(d[k] for k in OUTPUTS)
    return out


def bounds(name):
    n = longest_sums(name)
    return {k: min(CAP[k], 4.0 * max(DEV32[name][i], U32 * math.sqrt(n[k]))) for i, k in enumerate(OUTPUTS)}


# ------------------------------------------------------------------------------------------------------------------- GPU tests
@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


SENTINEL = 12345.0


def _check(name, what, dev_by_output):
    b = bounds(name)
    for k in OUTPUTS:
        if k in dev_by_output:
            print("CVEDGE %-30s %-12s %-8s dev %.3e  dev32 %.3e  bound %.3e" % (name, what, k, dev_by_output[k], DEV32[name][OUTPUTS.index(k)], b[k]))
    for k, v in dev_by_output.items():
        assert v <= b[k], "%s %s %s: deviation %.3e from float64 exceeds %.3e" % (name, what, k, v, b[k])


@pytest.mark.gpu
@pytest.mark.parametrize("mode,window", MODES, ids=["direct", "lds", "own", "own-window-8x4"])
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_cv_train_vs_fp64(dev, monkeypatch, name, mode, window):
    """Training forward and one form of the backward against float64.  The tiny window (``own``, 8 x 4 texels) runs with a ``stats`` tensor:
    ``stats[0]`` counts the scattered taps per lane (C / 4 lanes per pixel) and must be the reference's count of non-zero-weight taps; on the
    wild case ``stats[1]``, the taps that missed the window, must fill every wavefront's 128-entry queue four times over on average."""
    from mvsformer_amd import ops
    c, t = CASE[name], build_case(name)
    feat, rt, hyp, w = (t[k].to(dev) for k in ("feat_cl", "rt", "hyp", "weight"))
    R = t["R"].to(dev)
    gvol = R.permute(0, 2, 3, 4, 1).contiguous().bfloat16() if c.bf16 else R       # bf16 channel-last [B,D,H,W,G]: exact, R is pre-rounded
    monkeypatch.setenv("MVS_CV_BWD", mode)
    if window is None:
        monkeypatch.delenv("MVS_CV_BWD_WINDOW", raising=False)
    else:
        monkeypatch.setenv("MVS_CV_BWD_WINDOW", window)
    stats = torch.zeros(2, dtype=torch.int32, device=dev) if window is not None else None
    vol, _ = ops.cv_aggregate(feat, rt, hyp, w, G, False, exact=True)
    if c.guard:
        # guards of dfeat's size around the hole that the backward's dfeat allocation will most likely reuse
        n = feat.numel()
        g0, hole, g1 = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
        g0.fill_(SENTINEL), g1.fill_(SENTINEL)
        del hole
    df, dw = ops.cv_aggregate_bwd(feat, rt, hyp, w, vol, gvol, G, stats=stats)
    torch.cuda.synchronize()
    if c.guard:
        assert torch.isfinite(vol).all() and torch.isfinite(df).all() and torch.isfinite(dw).all()
        assert bool((g0 == SENTINEL).all()) and bool((g1 == SENTINEL).all()), "guard tensor written"
    what = mode if window is None else "%s %s" % (mode, window)
    _check(name, what, deviation(name, vol, df, dw))
    if stats is not None:
        census, lanes = tap_census(name), c.C // 4
        s0, s1 = int(stats[0]), int(stats[1])
        queues = -(-c.W // 8) * -(-c.H // 4) * (c.C // 8) * c.B * (c.V - 1)
        print("CVEDGE %-30s stats taps %d (reference %d x %d lanes, fragile %d)  missed %d over %d queues" %
              (name, s0, census["taps"], lanes, census["fragile"], s1, queues))
        assert s0 % lanes == 0 and abs(s0 // lanes - census["taps"]) <= 2 * census["fragile"], (s0, lanes, census["taps"], census["fragile"])
        assert 0 <= s1 <= s0
        if name == MISSQ_CASE:
            assert s1 > 4 * QCAP * queues, (s1, queues)


@pytest.mark.gpu
def test_aggregate_fn_vs_fp64(dev, monkeypatch):
    """``autograd.AggregateFn`` end to end: channels-first features in, channels-first gradients out, default backward."""
    from mvsformer_amd import autograd as ag
    monkeypatch.delenv("MVS_CV_BWD", raising=False)
    monkeypatch.delenv("MVS_CV_BWD_WINDOW", raising=False)
    name = AUTOGRAD_CASE
    t = build_case(name)
    fm = t["feat_cl"].permute(0, 1, 4, 2, 3).contiguous().to(dev).requires_grad_(True)
    wm = t["weight"].to(dev).requires_grad_(True)
    vm = ag.AggregateFn.apply(fm, wm, t["rt"].to(dev), t["hyp"].to(dev), G)
    (vm * t["R"].to(dev)).sum().backward()
    assert fm.grad.shape == fm.shape and wm.grad.shape == wm.shape
    _check(name, "AggregateFn", deviation(name, vm, fm.grad.permute(0, 1, 3, 4, 2), wm.grad))
