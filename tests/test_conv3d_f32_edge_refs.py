"""CPU checks of ``tests/conv3d_f32_edge_util.py``: the float64 references against naive loops, every case against the plan property it
claims (through the launchers' own planner, ``conv_plan_reader``), the coverage of tile forms / MT / SHW / CC / NT, and the bounds: the fp32-rounded reference
lies inside every bound with no element excluded, and each mutation - what a subtly wrong kernel would produce - violates it."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import conv3d_f32_edge_util as U


# ------------------------------------------------------------------------------------------------------------------- references
def _naive_conv(x, w, s):
    B, Ci, D, H, W = x.shape
    Co = w.shape[0]
    Do, Ho, Wo = (D - 1) // s[0] + 1, (H - 1) // s[1] + 1, (W - 1) // s[2] + 1
    y = torch.zeros(B, Co, Do, Ho, Wo, dtype=torch.float64)
    for b, o, od, oh, ow, i, kd, kh, kw in itertools.product(range(B), range(Co), range(Do), range(Ho), range(Wo), range(Ci), range(3), range(3), range(3)):
        d, h, v = od * s[0] - 1 + kd, oh * s[1] - 1 + kh, ow * s[2] - 1 + kw
        if 0 <= d < D and 0 <= h < H and 0 <= v < W:
            y[b, o, od, oh, ow] += x[b, i, d, h, v] * w[o, i, kd, kh, kw]
    return y


def _naive_deconv(x, w, s):
    B, Ci, D, H, W = x.shape
    Co = w.shape[1]
    y = torch.zeros(B, Co, D * s[0], H * s[1], W * s[2], dtype=torch.float64)
    for b, i, d, h, v, o, kd, kh, kw in itertools.product(range(B), range(Ci), range(D), range(H), range(W), range(Co), range(3), range(3), range(3)):
        od, oh, ow = d * s[0] - 1 + kd, h * s[1] - 1 + kh, v * s[2] - 1 + kw
        if 0 <= od < y.shape[2] and 0 <= oh < y.shape[3] and 0 <= ow < y.shape[4]:
            y[b, o, od, oh, ow] += x[b, i, d, h, v] * w[i, o, kd, kh, kw]
    return y


def _naive_wgrad(A, Bt, s):
    N, CA, Dp, Hp, Wp = A.shape
    _, CB, Db, Hb, Wb = Bt.shape
    dW = torch.zeros(CA, CB, 3, 3, 3, dtype=torch.float64)
    for n, a, b, d, h, v, kd, kh, kw in itertools.product(range(N), range(CA), range(CB), range(Dp), range(Hp), range(Wp), range(3), range(3), range(3)):
        z, y, x = d * s[0] - 1 + kd, h * s[1] - 1 + kh, v * s[2] - 1 + kw
        if 0 <= z < Db and 0 <= y < Hb and 0 <= x < Wb:
            dW[a, b, kd, kh, kw] += A[n, a, d, h, v] * Bt[n, b, z, y, x]
    return dW


@pytest.mark.parametrize("stride", U.STRIDES)
def test_references_match_naive_loops(stride):
    g = torch.Generator().manual_seed(11)
    s3 = (stride[0], stride[1], stride[1])
    x = torch.randn(1, 2, 3, 3, 4, generator=g, dtype=torch.float64)
    w = torch.randn(3, 2, 3, 3, 3, generator=g, dtype=torch.float64)
    y = F.conv3d(x, w, None, stride=s3, padding=1)
    assert (y - _naive_conv(x, w, s3)).abs().max() < 1e-12
    wt = torch.randn(2, 3, 3, 3, 3, generator=g, dtype=torch.float64)
    xs = x[:, :, :2, :2, :3]
    yt = F.conv_transpose3d(xs, wt, None, stride=s3, padding=1, output_padding=tuple(v - 1 for v in s3))
    assert (yt - _naive_deconv(xs, wt, s3)).abs().max() < 1e-12
    # both orientations of csrc/wgrad.hip against autograd and against the loop
    xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    F.conv3d(xg, wg, None, stride=s3, padding=1).backward(dy)
    assert (U.wgrad_sum(dy, x, stride) - wg.grad).abs().max() < 1e-12
    assert (U.wgrad_sum(dy, x, stride) - _naive_wgrad(dy, x, s3)).abs().max() < 1e-12
    xg, wg = xs.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    dyt = torch.randn(yt.shape, generator=g, dtype=torch.float64)
    F.conv_transpose3d(xg, wg, None, stride=s3, padding=1, output_padding=tuple(v - 1 for v in s3)).backward(dyt)
    assert (U.wgrad_sum(xs, dyt, stride) - wg.grad).abs().max() < 1e-12


@pytest.mark.parametrize("shape", [(1, 4, 1, 1, 4), (2, 8, 3, 7, 12), (1, 4, 2, 9, 36)])
def test_wino_pipeline_is_the_convolution(shape):
    g = torch.Generator().manual_seed(12)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    w = torch.randn(16, shape[1], 3, 3, 3, generator=g, dtype=torch.float64)
    want = F.conv3d(x, w, None, padding=1)
    assert (U.wino_pipeline(x, w) - want).abs().max() < 1e-12
    T, S = U.wino_pipeline(x, w, absolute=True), F.conv3d(x.abs(), w.abs(), None, padding=1)
    assert bool((T >= S * (1 - 1e-12)).all())
    print("T / S: median %.1f max %.1f" % (float((T / S).median()), float((T / S).max())))


def test_dgrad_kinds_are_the_gradient():
    """What the kernels run for a data gradient (the flipped, transposed weight) equals the transposed convolution the reference evaluates."""
    for c in (U.CASE["f22-int"]._replace(kind="dgrad", cin=24, cout=12), U.CASE["wn-int"]._replace(kind="wino-dgrad", cin=32, cout=12)):
        t = U.case_inputs(c)
        ran = F.conv3d(t["x"].double(), U.conv_weight(c, t["w"]).double(), None, padding=1)
        assert torch.equal(ran, U.raw_ref(c, t["x"], t["w"]))


# ------------------------------------------------------------------------------------------------------------------- claims and coverage
@pytest.mark.parametrize("c", U.ALL_CASES, ids=lambda c: c.name)
def test_layer_case_has_the_plan_property_it_claims(c):
    p = U.case_plan(c)._asdict()
    assert c.claim
    for k, v in c.want:
        assert p[k] == v, (c.name, c.claim, k, v, p)
    if c.kind == "deconv":
        Do, Ho, Wo = U.out_dims(c)
        assert Ho >= 2 and Wo >= 2 and (c.stride[0] == 1 or Do >= 2)                     # all four (eight) output parities exist
        assert p["route"] == "deconv3d_kernel"
    if c.kind in ("dgrad", "wino-dgrad"):
        assert c.cin != c.cout
    if c.kind in ("conv", "dgrad"):
        assert c.cin % 4 == 0 and c.cout % 8 == 0 and c.cout <= 64
    if c.kind in ("wino", "wino-dgrad"):
        assert U.wino_supported(c.cin, c.cout, c.D, c.H, c.W)


@pytest.mark.parametrize("c", U.WG_CASES, ids=lambda c: c.name)
def test_wgrad_case_has_the_plan_property_it_claims(c):
    p = U.wg_plan(c)._asdict()
    for k, v in c.want:
        assert p[k] == v, (c.name, c.claim, k, v, p)
    assert c.CA <= 64


def test_big_default_cases_leave_the_first_round():
    """On each of them the 32-voxel form would need more than 256 blocks, and the model picks a 64-voxel form by itself."""
    for name in U.BIG_DEFAULT:
        c = U.CASE[name]
        assert U.plan_conv(c.B, c.cin, c.cout, c.D, c.H, c.W, c.stride[0], c.stride[1], "22s").nblocks > 256, name
        assert U.case_plan(c).TW == 64
        assert c.cin <= 16
    assert {U.CASE[n].stride for n in U.BIG_DEFAULT} == set(U.STRIDES)


def test_coverage_of_conv_forms():
    default = [(U.case_plan(c), c) for c in U.DEFAULT_CASES]
    assert {p.form for p, _ in default} == set(U.FORMS)                                    # all four forms by the dispatcher's own choice
    forced = [(U.case_plan(c), c) for c in U.FORCED_CASES]
    for form, strides in (("22", U.STRIDES), ("42", U.STRIDES[:2]), ("22s", U.STRIDES)):
        mine = [(p, c) for p, c in forced if c.force == form and p.form == form]
        assert {c.stride for _, c in mine} == set(strides)
        TW = mine[0][0].TW
        for stride in strides:
            ms = [(p, c) for p, c in mine if c.stride == stride and c.data == "randn"]
            assert {p.Wo for p, _ in ms} >= {TW - 1, TW, TW + 1}
            assert {p.Ho for p, _ in ms} >= {1, 3}
            if stride[1] == 2:
                assert {c.W % 2 for _, c in ms} == {0, 1}                                  # odd and even input extents
        assert {c.cin for _, c in mine} >= {4, 8, 12, 16}
        assert {c.cout for _, c in mine} >= ({8, 16} if form == "42" else {8, 16, 24, 40, 48, 64})
        assert {p.Do for p, _ in mine} >= ({3, 5} if form == "42" else {1, 2, 3, 5})
        assert any(c.data == "int" for _, c in mine)
        dg = [(p, c) for p, c in mine if c.kind == "dgrad"]                               # the dgrad pack on the whole stride-(1,1) edge set
        s11 = [(p, c) for p, c in mine if c.kind == "conv" and c.stride == (1, 1) and c.data == "randn"]
        assert {(c.D, c.H, c.W, c.B, c.cin) for _, c in dg} == {(c.D, c.H, c.W, c.B, c.cin) for _, c in s11}
        assert {p.Ho for p, _ in dg} == {1, 3} and {c.cin for _, c in dg} == {4, 8, 12, 16} and {p.Wo for p, _ in dg} == {TW - 1, TW, TW + 1}
        assert all(c.cin != c.cout for _, c in dg)
        assert {(p.Ho, c.cin % 8 == 0) for p, c in dg} == {(1, False), (1, True), (3, False), (3, True)}   # full and half last chunks at both heights
        assert {(p.Ho, c.cin % 8 == 0) for p, c in mine} == {(1, False), (1, True), (3, False), (3, True)}
    every = default + forced
    assert {p.CC for p, _ in every if p.TW == 64} == {4, 8}
    assert {(p.form, p.CC) for p, _ in every} >= {("22", 8), ("22", 4), ("42", 8), ("42", 4), ("22s64", 8), ("22s64", 4), ("22s", 8)}
    assert {p.NT for p, _ in every if p.form == "22"} == {1, 2, 4}
    assert {p.nsplit for p, _ in every if p.form == "22s"} >= {1, 2, 4}
    # MVS_CONV_TILE=42 where the form is refused: the model decides
    assert any(c.force == "42" and p.form != "42" and p.Do == 2 for p, c in forced)
    epi = {(c.scale, c.relu, c.residual) for _, c in default}
    assert len(epi) == 8


def test_coverage_of_deconv_wino_wgrad():
    dc = U.DECONV_CASES
    for sd in (1, 2):
        mine = [c for c in dc if c.stride[0] == sd]
        assert {c.W for c in mine} >= {1, 31, 32, 33} and {c.D for c in mine} >= {1, 2, 3} and {c.H for c in mine} >= {1, 2, 3}
        assert {c.cout for c in mine} >= ({24, 48} if sd == 1 else {8, 16, 24, 48})
        assert any(c.scale and c.relu and c.residual for c in mine) and any(not (c.scale or c.relu or c.residual) for c in mine)
    assert {c.cin for c in dc} >= {8, 16, 24, 64}
    wn = [(U.case_plan(c), c) for c in U.WINO_CASES]
    assert {p.NT for p, _ in wn} == {1, 2}
    for nt in (1, 2):
        mine = [c for p, c in wn if p.NT == nt]
        assert {c.W for c in mine} >= {4, 28, 32, 36, 68} and {c.H for c in mine} >= {1, 2, 7, 8, 9}
        assert {c.D for c in mine} >= {1, 3}
        assert {c.B for c in mine} >= {1, 3}
        assert any(c.kind == "wino-dgrad" for c in mine)
    assert {c.cin for _, c in wn} >= {4, 8, 12, 64} and {c.cout for _, c in wn} >= {16, 32, 48, 64}
    assert any(not p.prefetch for p, _ in wn) and any(p.chunks % 2 == 1 and p.chunks > 1 for p, _ in wn)
    wg = [(U.wg_plan(c), c) for c in U.WG_EDGE_CASES + U.WG_MULTI_CASES]
    for mt, shw in itertools.product((1, 2, 3, 4), (1, 2)):
        mine = [(p, c) for p, c in wg if (p.MT, p.SHW) == (mt, shw)]
        assert any(p.tiles_max == 1 for p, _ in mine), (mt, shw)                           # every block one tile
        assert any(p.tiles_max >= 3 and p.tiles_min < p.tiles_max for p, _ in mine), (mt, shw)   # the prefetch loop, uneven last round
        assert any(c.data == "int" and p.tiles_max >= 3 for p, c in mine)
        edge = [(p, c) for p, c in mine if p.tiles_max == 1]
        assert {c.Wp - p.SEG for p, c in edge} >= {-1, 0, 1, 4}
        assert {p.vec_a for p, c in edge if c.Wp >= p.SEG} == {True, False}                # both A loads at a right tile edge
    edge = [(p, c) for p, c in wg if p.tiles_max == 1]
    assert {c.CA for _, c in edge} >= {8, 16, 24, 40, 48, 64} and {c.CB for _, c in edge} >= {1, 4, 5, 8, 64}
    assert {c.stride for _, c in edge} == {(1, 1), (1, 2), (2, 1), (2, 2)} and {c.orient for _, c in edge} == {"conv", "deconv"}
    assert {c.nb for _, c in edge} >= {1, 3} and any(c.Dp == 1 for _, c in edge) and any(c.short for _, c in edge)
    for p, c in edge:
        assert c.Hp in (1, p.TH, p.TH + 1)
    assert {(c.Hp > p.TH, c.Hp == p.TH, c.Hp == 1) for p, c in edge} >= {(True, False, False), (False, True, False), (False, False, True)}
    v1 = U.wgrad_v1_plan(*(getattr(U.WG_V1_ROWS_CASE, k) for k in ("nb", "CA", "CB", "Dp", "Hp")))
    assert v1.rows > 4 * v1.gy and v1.rows_per_wave >= 2
    # the first kernel runs the tiled kernel's whole table: stated here on its own set, so that thinning it cannot go unnoticed
    v1c = [c for c in U.WG_V1_CASES if c.data == "randn"]
    assert set(U.WG_EDGE_CASES + U.WG_MULTI_CASES) <= set(U.WG_V1_CASES) and U.WG_V1_ROWS_CASE in U.WG_V1_CASES
    assert {U.wgrad_v1_plan(c.nb, c.CA, c.CB, c.Dp, c.Hp).MT for c in v1c} == {1, 2, 3, 4}
    for shw in (1, 2):
        mine = [c for c in v1c if c.stride[1] == shw]
        assert 1 in {c.Hp for c in mine} and len({c.Hp for c in mine if c.Hp > 1}) >= 3          # kh = 0 / 2 on padding only, and on rows
        assert {c.Wp % 4 for c in mine} == {0, 1, 3}                                       # its K step is 4 voxels: whole and ragged last steps
        assert {c.CB % 4 for c in mine} >= {0, 1} and {c.CB for c in mine} >= {1, 4, 5, 8, 64}   # every tail of the 4-channel chunk
        assert {c.CA for c in mine} >= {8, 16, 24, 40, 48, 64} and {c.stride[0] for c in mine} == {1, 2}
    assert any(c.short and c.stride == (2, 2) for c in v1c) and any(c.short and c.stride == (1, 2) for c in v1c)   # odd Bt extents
    assert any(c.orient == "deconv" for c in v1c)


# ------------------------------------------------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("c", U.ALL_CASES + U.ROUTE_CASES[-2:], ids=lambda c: c.name)
def test_rounded_reference_is_inside_the_bound(c):
    ref, bound = U.expect(c)
    assert bound.shape == ref.shape and bool((bound >= 0).all())                           # one bound per element: none excluded
    assert U.share(ref.float(), ref, bound)[1] <= 1.0
    if c.data == "int":
        assert float(bound.max()) == 0 and torch.equal(ref.float().double(), ref)
    else:
        assert float(bound.min()) > 0 or c.relu


@pytest.mark.parametrize("c", U.WG_CASES, ids=lambda c: c.name)
def test_rounded_wgrad_reference_is_inside_the_bound(c):
    ref, bound = U.wg_expect(c.name)
    assert U.share(ref.float(), ref, bound)[1] <= 1.0
    if c.data == "int":
        assert float(bound.max()) == 0
    elif c.Dp == 1:                                                                        # kd = 0 and kd = 2 fall outside Bt when Db = 1
        if U.bt_dims(c)[0] == 1:
            assert float(bound[:, :, 0].max()) == 0 and float(bound[:, :, 2].max()) == 0 and float(ref[:, :, 0].abs().max()) == 0


def _caught(mut, c_or_name, wg=False):
    ref, bound = U.wg_expect(c_or_name) if wg else U.expect(c_or_name)
    return U.share(mut.float(), ref, bound)[1] > 1.0


def _raw(cases, kinds, n=6):
    out = [c for c in cases if c.kind in kinds and c.data == "randn" and not (c.scale or c.relu or c.residual)]
    return out[::max(1, len(out) // n)]


def test_mutations_of_the_conv_families_are_caught():
    """conv (every form), dgrad and Winograd (both NT): a dropped tap at one voxel, a shifted halo column of one tile, the last voxel of a
    tile row missing, two channels swapped across the 16 boundary."""
    fam = _raw(U.FORCED_CASES, ("conv", "dgrad"), 9) + _raw(U.DEFAULT_CASES, ("conv",), 6) + [U.CASE[n] for n in U.BIG_DEFAULT[::2]] + _raw(U.WINO_CASES, ("wino", "wino-dgrad"), 50)[::5] + _raw(U.WINO_CASES, ("wino", "wino-dgrad"), 50)[3::10]
    assert {U.case_plan(c).form for c in fam if c.kind in ("conv", "dgrad")} == set(U.FORMS)
    assert {U.case_plan(c).NT for c in fam if c.kind.startswith("wino")} == {1, 2}
    swapped = 0
    for c in fam:
        p = U.case_plan(c)
        Do, Ho, Wo = U.out_dims(c)
        TW = p.TW if c.kind in ("conv", "dgrad") else 32
        o = (Do - 1, Ho - 1, min(TW, Wo) - 1)                                              # the last voxel of the first tile's last row
        tap = next(tp for tp in itertools.product(range(3), repeat=3)
                   if all(0 <= ov * s - 1 + k < n for ov, s, k, n in zip(o, (c.stride[0], c.stride[1], c.stride[1]), tp, (c.D, c.H, c.W))))
        assert _caught(U.mutate_drop_tap(c, c.B - 1, o, tap), c), c.name
        assert _caught(U.mutate_drop_row_end(c, 0, TW), c), c.name
        if min(TW, Wo) * c.stride[1] < c.W and (min(TW, Wo) - 1) * c.stride[1] + 1 < c.W:
            assert _caught(U.mutate_shift_halo_column(c, 0, TW), c), c.name
        if c.cout > 16:
            swapped += 1
            assert _caught(U.mutate_swap_channels(U.expect(c)[0]), c), c.name
    assert swapped >= 4


def test_mutations_of_the_deconv_family_are_caught():
    fam = _raw(U.DECONV_CASES, ("deconv",), 8)
    assert {c.stride[0] for c in fam} == {1, 2}
    shifted = 0
    for c in fam:
        i = (c.D - 1, c.H - 1, min(32, c.W) - 1)
        assert _caught(U.mutate_drop_tap_deconv(c, c.B - 1, i, (1, 1, 1)), c), c.name
        assert _caught(U.mutate_drop_row_end(c, 0, 64), c), c.name
        if c.W > 1:
            shifted += 1
            assert _caught(U.mutate_shift_halo_column(c, 0, 32), c), c.name
        if c.cout > 16:
            assert _caught(U.mutate_swap_channels(U.expect(c)[0]), c), c.name
    assert shifted >= 4


def test_mutations_of_the_weight_gradient_are_caught():
    """Random cases of both orientations: a dropped tap, a tile's halo column shifted, the last voxel of a tile row missing, rows 15 / 16
    swapped.  The skipped second tile of a block: by the random multi-tile cases' bound, and exactly by the integer ones."""
    edge = [c for c in U.WG_EDGE_CASES if c.data == "randn"][::3]
    assert {c.orient for c in edge} == {"conv", "deconv"}
    for c in edge:
        assert _caught(U.mutate_wg_drop_tap(c.name, (1, 1, 1)), c.name, True), c.name
        assert _caught(U.mutate_wg_drop_row_end(c.name), c.name, True), c.name
        if (min(c.Wp, U.wg_plan(c).SEG) - 1) * c.stride[1] + 1 < U.bt_dims(c)[2] and c.Wp > 1:
            assert _caught(U.mutate_wg_shift_halo_column(c.name), c.name, True), c.name
        if c.CA > 16:
            assert _caught(U.mutate_swap_channels(U.wg_expect(c.name)[0]), c.name, True), c.name
    for c in U.WG_MULTI_CASES:
        assert _caught(U.mutate_wg_skip_second_tile(c.name), c.name, True), c.name
