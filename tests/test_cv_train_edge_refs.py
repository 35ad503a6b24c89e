"""CPU-side checks of tests/test_hip_cv_train_edges.py (no GPU): its float64 reference is pinned to the oracle the goldens pin, its DEV32 table
is what ``measure_dev32()`` measures, its cases exercise what their table claims, and four subtly wrong backwards - built by perturbing the
reference's own results, never a kernel - land outside the bounds the kernels are held to."""
import math

import pytest
import torch

import test_hip_cv_train_edges as E

NAMES = [c.name for c in E.CASES]


# Agreement of the reference, evaluated in float32, with float32 autograd through ref_torch.homo_warping_3D_with_mask + group_correlation on
# the same ``proj`` (max norm relative to max|oracle|; ``rt`` is ``src_proj @ inverse(ref_proj)`` as the oracle forms it).  Measured:
#   v3-c16-d7-4x8-b1   volume 1.2e-07  dfeat 1.6e-07  dweight 1.1e-07
#   v5-c32-d8-5x9-b3   volume 6.6e-07  dfeat 3.1e-07  dweight 2.9e-07
# The two differ in how the rays are formed (a matmul there, three multiply-adds here) and in ATen's own arithmetic inside grid_sample,
# i.e. in float32 rounding of the sample position (~1e-7 px times a feature difference of order 1); asserted with a margin of 3.
ORACLE_AGREEMENT = 2e-6


@pytest.mark.parametrize("name", ["v3-c16-d7-4x8-b1", "v5-c32-d8-5x9-b3"])
def test_reference_in_float32_is_the_oracle(name):
    from oracle import ref_torch
    t = E.build_case(name)
    proj, hyp, R = t["proj"], t["hyp"], t["R"]
    V = proj.shape[1]
    assert torch.equal(E.rt_from_proj(proj), t["rt"])
    fr = t["feat_cl"].permute(0, 1, 4, 2, 3).contiguous().requires_grad_(True)
    wr = t["weight"].clone().requires_grad_(True)
    ref_P = ref_torch.compose_projection(proj[:, 0])
    vol_sum = 0.0
    for v in range(1, V):
        warped, _ = ref_torch.homo_warping_3D_with_mask(fr[:, v], ref_torch.compose_projection(proj[:, v]), ref_P, hyp)
        vol_sum = vol_sum + ref_torch.group_correlation(fr[:, 0], warped, E.G) * wr[:, v - 1:v].unsqueeze(1)
    vol = vol_sum / (wr.sum(1, keepdim=True).unsqueeze(1) + 1e-6)
    (vol * R).sum().backward()
    mine = E.reference(name, torch.float32)
    for what, got, want in (("volume", mine.volume, vol.detach()), ("dfeat", mine.dfeat.permute(0, 1, 4, 2, 3), fr.grad),
                            ("dweight", mine.dweight, wr.grad)):
        err = (got.double() - want.double()).abs().max().item() / want.abs().max().item()
        print("oracle agreement %s %s %.2e" % (name, what, err))
        assert err < ORACLE_AGREEMENT, (name, what, err)
    # and float64 against the oracle: the reference is the same function, not merely close to itself
    r64 = E.reference(name)
    assert (r64.volume - vol.detach().double()).abs().max().item() / vol.abs().max().item() < ORACLE_AGREEMENT


def test_dev32_table_is_what_the_helper_measures():
    got = E.measure_dev32()
    assert sorted(got) == sorted(E.DEV32) == sorted(NAMES)
    for name in NAMES:
        for k, g, want in zip(E.OUTPUTS, got[name], E.DEV32[name]):
            assert math.isfinite(g) and 0.0 < g, (name, k, g)
            assert 0.5 * want <= g <= 2.0 * want, (name, k, g, want)
            assert 4.0 * want <= E.CAP[k], (name, k, want)                 # no case needs more than test_aggregate_fn_grads allows
            assert E.bounds(name)[k] >= 4.0 * want or E.bounds(name)[k] == E.CAP[k]
    for name in NAMES:
        r = E.reference(name)
        assert all(bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in (r.volume, r.dfeat, r.dweight)), name


def test_case_list_covers_the_tiling_edges():
    cs = E.CASES
    assert {2, 3, 5, 7} <= {c.V for c in cs} and {1, 2, 3} <= {c.B for c in cs} and {8, 16, 32, 64} == {c.C for c in cs}
    assert {1, 7, 8, 9, 17} <= {c.D for c in cs}
    assert {8, 64} <= {c.C for c in cs if c.V == 7}
    assert {(3, 5), (4, 8), (5, 9), (13, 19)} <= {(c.H, c.W) for c in cs} and {16, 17} <= {c.W for c in cs}
    assert sum(c.bf16 for c in cs) == 1 and E.CASE[E.AUTOGRAD_CASE] and E.CASE[E.MISSQ_CASE].geom == "wild"
    for c in cs:
        if c.B > 1:                                                       # another rt and other hypotheses per batch entry
            t = E.build_case(c.name)
            assert not torch.equal(t["rt"][0], t["rt"][1]) and not torch.equal(t["hyp"][0], t["hyp"][1]), c.name


def test_cases_avoid_z_near_zero():
    for name in NAMES:
        assert E.tap_census(name)["zmin"] > 0.25, name


def test_border_case_leaves_the_image_on_every_side():
    cen = E.tap_census("border-v3-c16-d9-13x19-b2")
    print("border case: footprint not wholly inside %.1f %%, wholly outside %.1f %%, beyond l/r/t/b %s" %
          (100 * cen["partial"], 100 * cen["outside"], cen["sides"]))
    assert abs(cen["partial"] - 0.505) < 0.002 and abs(cen["outside"] - 0.360) < 0.002          # the shares the case table states
    n = 2 * 2 * 9 * 13 * 19
    assert all(s > 0.05 * n for s in cen["sides"]), cen["sides"]
    assert cen["outside"] < cen["partial"] - 0.1                                                   # half-valid footprints exist


def _origins_per_tile(name, views=None):
    """Distinct footprint origins among the pixels of one 8 x 4 wavefront tile on one plane of one view: (min, max) over all of them."""
    c, t = E.CASE[name], E.build_case(name)
    lo, hi = 10 ** 9, 0
    for v in views or range(c.V - 1):
        _, _, x0, y0, _, _, _ = E.sweep_taps_ref(t["rt"][:, v], t["hyp"], c.H, c.W, torch.float32)
        key = (y0 * 4096 + x0).reshape(c.B, c.D, c.H, c.W)
        for ty in range(0, c.H, 4):
            for tx in range(0, c.W, 8):
                for b in range(c.B):
                    for d in range(c.D):
                        tile = key[b, d, ty:ty + 4, tx:tx + 8]
                        if tile.numel() == 32:
                            n = tile.unique().numel()
                            lo, hi = min(lo, n), max(hi, n)
    return lo, hi


def test_collision_cases_collide_inside_the_image():
    for name in ("minify-v3-c32-d8-8x17-b1", "degenerate-v4-c8-d9-6x10-b1"):
        cen = E.tap_census(name)
        assert cen["partial"] == 0.0 and cen["zmin"] >= 1.0, (name, cen)             # every sample inside, z = d in [1, 2]
    assert _origins_per_tile("degenerate-v4-c8-d9-6x10-b1", (0, 2)) == (1, 1)        # 32 pixels, one origin, the same on every plane
    assert _origins_per_tile("degenerate-v4-c8-d9-6x10-b1", (1,)) == (1, 2)          # moving with the plane; the +-3 % jitter may split it
    lo, hi = _origins_per_tile("minify-v3-c32-d8-8x17-b1")
    assert 2 <= lo and hi <= 9, (lo, hi)                                             # 32 pixels on ~3 x 2 origins
    assert E.tap_census("degenerate-v4-c8-d9-6x10-b1")["hits"] == 6 * 10 * 9         # the longest sum of the suite


# ------------------------------------------------------------------------------------------------ would a subtly wrong kernel fail?
def _manual_src_grad(name, drop_collisions):
    """d loss / d source features by hand (cost_volume_bwd.hip's formula: each sample adds wgt_k * R * w_v / (S * CPG) * ref to its four
    taps), in float64.  ``drop_collisions``: of the pixels of one 8 x 4 wavefront tile that share a footprint origin on one plane, only the
    last one's update survives - what a read-modify-write without the owner election would do."""
    c, t = E.CASE[name], E.build_case(name)
    B, V, H, W, C, D = c.B, c.V, c.H, c.W, c.C, c.D
    f, w, R = t["feat_cl"].double(), t["weight"].double(), t["R"].double()
    S = w.sum(1) + 1e-6
    out = torch.zeros(B, V, H * W, C, dtype=torch.float64)
    tile = ((torch.arange(H) // 4).view(H, 1) * 64 + (torch.arange(W) // 8).view(1, W)).reshape(-1)
    for v in range(V - 1):
        idx, wgt, x0, y0, _, _, _ = E.sweep_taps_ref(t["rt"][:, v], t["hyp"], H, W, torch.float64)
        coef = (R / (S.view(B, 1, 1, H, W) * (C // E.G)) * w[:, v].view(B, 1, 1, H, W)).reshape(B, E.G, D, H * W)
        coef = coef.repeat_interleave(C // E.G, dim=1).permute(0, 2, 3, 1) * f[:, 0].reshape(B, 1, H * W, C)       # [B,D,HW,C]
        keep = torch.ones(B, D, H * W, dtype=torch.bool)
        if drop_collisions:
            key = (tile.view(1, 1, -1) * 4096 + y0) * 4096 + x0
            for b in range(B):
                for d in range(D):
                    last = {}
                    for p, k in enumerate(key[b, d].tolist()):
                        last[k] = p
                    keep[b, d] = False
                    keep[b, d, list(last.values())] = True
        for k in range(4):
            val = coef * (wgt[k] * keep).unsqueeze(-1)
            for b in range(B):
                out[b, v + 1].index_add_(0, idx[k][b].reshape(-1), val[b].reshape(-1, C))
    return out.reshape(B, V, H, W, C)


@pytest.mark.parametrize("name", ["minify-v3-c32-d8-8x17-b1", "degenerate-v4-c8-d9-6x10-b1"])
def test_dropping_a_tap_where_origins_coincide_would_fail(name):
    r = E.reference(name)
    scale = E.scales(name)["dfeat"]
    right = _manual_src_grad(name, False)
    assert (right[:, 1:] - r.dfeat[:, 1:]).abs().max().item() / scale < 1e-13           # the hand formula is the autograd gradient
    wrong = _manual_src_grad(name, True)
    dev = (wrong[:, 1:] - r.dfeat[:, 1:]).abs().max().item() / scale
    print("wrong kernel: lost collisions   %-30s dfeat dev %.2e  bound %.2e" % (name, dev, E.bounds(name)["dfeat"]))
    assert dev > 100 * E.bounds(name)["dfeat"]


@pytest.mark.parametrize("name", NAMES)
def test_omitting_the_T_over_S_term_would_fail(name):
    t, r = E.build_case(name), E.reference(name)
    S = t["weight"].double().sum(1, keepdim=True) + 1e-6
    T = (t["R"].double() * r.volume).sum(dim=(1, 2)).unsqueeze(1)
    dev = E.deviation(name, r.volume, r.dfeat, r.dweight + T / S)["dweight"]
    print("wrong kernel: no -T/S           %-30s dweight dev %.2e  bound %.2e" % (name, dev, E.bounds(name)["dweight"]))
    assert dev > 100 * E.bounds(name)["dweight"]


@pytest.mark.parametrize("name", [c.name for c in E.CASES if c.C > 8])
def test_wrong_group_size_would_fail(name):
    """1 / CPG of the next narrower feature map (CPG / 2): every output is off by a factor 2."""
    r = E.reference(name)
    dev = E.deviation(name, 2 * r.volume, 2 * r.dfeat, 2 * r.dweight)
    print("wrong kernel: 1/(CPG/2)         %-30s dev %s" % (name, {k: "%.2e" % v for k, v in dev.items()}))
    assert all(dev[k] > 100 * E.bounds(name)[k] for k in ("volume", "dfeat")) and (E.CASE[name].V == 2 or dev["dweight"] > 100 * E.bounds(name)["dweight"])


@pytest.mark.parametrize("name", [c.name for c in E.CASES if c.D % 2 == 1 and c.D > 1])
def test_skipping_the_last_plane_of_an_odd_chunk_would_fail(name):
    """The backward without the last plane (the first half of the final plane pair when D is odd) = the backward of a gradient whose last
    plane is zero."""
    t, r = E.build_case(name), E.reference(name)
    R = t["R"].clone()
    R[:, :, -1] = 0
    wrong = E.cv_train_ref(t["feat_cl"], t["rt"], t["hyp"], t["weight"], R, torch.float64)
    dev = E.deviation(name, r.volume, wrong.dfeat, wrong.dweight)
    print("wrong kernel: last plane skipped %-30s dfeat dev %.2e (bound %.2e)  dweight dev %.2e (bound %.2e)" %
          (name, dev["dfeat"], E.bounds(name)["dfeat"], dev["dweight"], E.bounds(name)["dweight"]))
    assert dev["dfeat"] > 100 * E.bounds(name)["dfeat"] and dev["dweight"] > 100 * E.bounds(name)["dweight"]
