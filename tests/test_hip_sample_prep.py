"""GPU tests of mvsformer_amd.sample_prep / csrc/sample_prep.hip against the numpy restatements of tests/sample_prep_util.py.

Shapes are the smallest that reach each edge.  The issue's 37x53 source at scale 0.45 resizes to 16x23, which cannot hold a 16x24 crop:
that one case uses a 16x16 crop (every other case uses 16x24)."""
import itertools

import numpy as np
import pytest
import torch

import sample_prep_util as u
from conftest import t

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _sp():
    from mvsformer_amd import sample_prep
    return sample_prep


def _sources(H0, W0, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H0, 0:W0]
    checker = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)
    ramp = np.stack([(xx * 255 // (W0 - 1)), (yy * 255 // (H0 - 1)), ((xx + yy) * 255 // (H0 + W0 - 2))], -1).astype(np.uint8)
    return np.stack([rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8), checker, ramp])


def _tables(sp, B, V, K, params, src_hw, dmin=None, dint=None):
    tb = sp.TrainTables(B, V, K, device=DEV)
    tb.write(params, src_hw, dmin or [1.0] * B, dint or [1.0] * B)
    return tb


def _params(sp, V, rs, cands, src_offsets=None):
    return sp.TrainParams(view_ids=list(range(V)), resize_scales=[rs] * V if not isinstance(rs, list) else rs, candidates=cands,
                          src_offsets=src_offsets if src_offsets is not None else [None] * (V - 1))


def test_module_and_abi():
    """Fails on the parent commit: no sample_prep module, no mvs_prep_* entries, ABI 50."""
    from mvsformer_amd import _lib
    sp = _sp()
    lib = _lib.load()
    assert lib.mvs_version() == _lib.ABI_VERSION == 51
    for n in ("mvs_prep_accept", "mvs_prep_geometry", "mvs_prep_area_crop", "mvs_prep_jitter_tail", "mvs_prep_eval_resize", "mvs_prep_pyramid_floats"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert callable(sp.prepare_train_batch) and callable(sp.prepare_eval_views) and callable(sp.draw_train_params)


AREA_CASES = [(37, 53, 1.0, 16, 24), (37, 53, 0.5, 16, 24), (37, 53, 0.45, 16, 16), (37, 53, 0.731, 16, 24), (64, 96, 0.5, 16, 24)]


@pytest.mark.parametrize("H0,W0,rs,h,w", AREA_CASES)
def test_area_resize_crop(H0, W0, rs, h, w):
    """Exact where the fp64 evaluation of the same weights is further than 2^-10 from a rounding boundary, within one level elsewhere; the
    2:1 case, scale 1 and the fp32 restatement are bit-equal.  0.731 on W0 = 53 gives int(38.74) = 38: actual and nominal scale differ."""
    from mvsformer_amd import ops
    sp = _sp()
    src = _sources(H0, W0)                                      # three "views"
    rh, rw = (int(H0 * rs), int(W0 * rs)) if rs != 1.0 else (H0, W0)
    want32 = np.stack([u.area_resize(s, rh, rw) for s in src])
    want64 = np.stack([u.area_resize_f64(s, rh, rw) for s in src]) if rs not in (1.0, 0.5) else want32.astype(np.float64)
    for oy, ox in ((0, 0), (rh - h, rw - w)):                     # the largest offset ends in the clipped last cell
        tb = _tables(sp, 1, 3, 1, [_params(sp, 3, rs, [(oy, ox)])], (H0, W0))
        chosen = ops.prep_accept(torch.zeros(1, H0, W0, dtype=torch.uint8, device=DEV), tb.ptab, tb.cand, (h, w), require_positive=False)
        got = ops.prep_area_crop(t(src, DEV)[None], tb.ptab, chosen, (h, w))[0].cpu().numpy()
        assert chosen.cpu().tolist() == [[oy, ox, 1, 0]]
        w32, w64 = want32[:, oy:oy + h, ox:ox + w], want64[:, oy:oy + h, ox:ox + w]
        near = np.abs(np.abs(w64 - np.floor(w64)) - 0.5) <= 2.0 ** -10
        diff = got.astype(np.int32) - np.clip(np.rint(w64), 0, 255).astype(np.int32)
        print("area %dx%d scale %g offset (%d,%d): %d near-ties, %d differ from fp64, %d from fp32" %
              (H0, W0, rs, oy, ox, near.sum(), (diff != 0).sum(), (got != w32).sum()))
        assert np.abs(diff).max() <= 1 and not (diff != 0)[~near].any()
        assert (diff != 0).sum() <= near.sum()
        assert np.array_equal(got, w32)
        # the count the fp64 oracle alone predicts: a pixel differs from round(fp64) exactly where the fp32 evaluation of the same
        # weights lands on the other side of the boundary, and only near-ties can
        assert (diff != 0).sum() == (w32.astype(np.int32) != np.clip(np.rint(w64), 0, 255).astype(np.int32)).sum()
        if (H0, W0, rs) == (37, 53, 0.731):
            assert int(near.sum()) == (22 if (oy, ox) == (0, 0) else 27)
        if rs in (1.0, 0.5):
            assert int(near.sum()) == 0


def _mask_cases(H0, W0, rs, h, w, cands):
    """raw PNG masks: positive (11) only at a pixel stage 1 samples / only at pixels it skips (10 elsewhere) / empty."""
    rh, rw = (int(H0 * rs), int(W0 * rs)) if rs != 1.0 else (H0, W0)
    iy, ix = u.nn_index(rh, H0), u.nn_index(rw, W0)
    oy, ox = cands[min(2, len(cands) - 1)]
    sampled = np.full((H0, W0), 10, np.uint8)
    sampled[iy[oy + 8], ix[ox + 8]] = 11                          # crop pixel (8, 8) is a stage-1 sample
    skipped = np.full((H0, W0), 10, np.uint8)
    skipped[iy[oy + 3], ix[ox + 5]] = 11
    return [sampled, skipped, np.full((H0, W0), 10, np.uint8)]


@pytest.mark.parametrize("H0,W0,rs,h,w", [(37, 53, 1.0, 16, 24), (37, 53, 0.731, 16, 24), (74, 100, 0.5, 32, 40), (64, 96, 1.0, 32, 40)])
@pytest.mark.parametrize("K", [1, 4])
def test_nearest_pyramid_acceptance_proj(H0, W0, rs, h, w, K):
    from mvsformer_amd import ops
    sp = _sp()
    rng = np.random.default_rng(3)
    rh, rw = (int(H0 * rs), int(W0 * rs)) if rs != 1.0 else (H0, W0)
    cands = [(0, 0), (rh - h, 0), (rh - h, rw - w), (1, 2)][:K] if K > 1 else [(rh - h, rw - w)]
    masks = _mask_cases(H0, W0, rs, h, w, cands)
    B, V = len(masks), 3
    depth = rng.uniform(400, 900, (B, H0, W0)).astype(np.float32)
    depth[:, ::5, ::3] = 0.0
    depth[:, 1, 1] = np.float32(3.0e38)
    intr = rng.uniform(0.5, 900, (B, V, 3, 3)).astype(np.float32)
    extr = rng.normal(size=(B, V, 4, 4)).astype(np.float32)
    src_off = [(1, 3), (rh - h, rw - w)]                           # consist_crop off: each view's own offsets
    rss = [rs, 1.0, rs]
    params = [_params(sp, V, rss, cands, src_off if b != 1 else [None, None]) for b in range(B)]
    dmin, dint, nd = [425.0, 0.5, 1.0], [2.65, 0.1, 0.3], 7
    lens = {sp.arange_length(a, b, nd) for a, b in zip(dmin, dint)}
    assert lens == {8} and sp.arange_length(425.0, 2.65, 192) == 192      # 0.1 and 0.3 * 7: arange's length rule yields 8, not 7
    tb = _tables(sp, B, V, K, params, (H0, W0), dmin, dint)
    chosen = ops.prep_accept(t(np.stack(masks), DEV), tb.ptab, tb.cand, (h, w))
    d, m, proj, dv = ops.prep_geometry(t(depth, DEV), t(np.stack(masks), DEV), tb.ptab, chosen, t(intr, DEV), t(extr, DEV), tb.drange, (h, w), 8)
    got_c = chosen.cpu().numpy()
    for b in range(B):
        want_c = u.accept(masks[b], rs, cands, h, w)
        assert tuple(got_c[b]) == want_c, (b, got_c[b], want_c)
        oy, ox = want_c[:2]
        wd, wm = u.crop_maps(depth[b], masks[b], rs, oy, ox, h, w)
        for s in ("stage1", "stage2", "stage3", "stage4"):
            assert np.array_equal(d[s][b].cpu().numpy(), wd[s]) and np.array_equal(m[s][b].cpu().numpy(), wm[s]), (b, s)
        offs = [(oy, ox)] + [(oy, ox) if o is None else o for o in params[b].src_offsets]
        wp = u.proj_matrices(intr[b], extr[b], rss, offs)
        for s in wp:
            assert np.array_equal(proj[s][b].cpu().numpy(), wp[s]), (b, s)
        assert np.array_equal(dv[b].cpu().numpy(), u.depth_values(dmin[b], dint[b], nd))
    assert got_c[0, 2] == 1 and got_c[0, 3] == min(2, K - 1)          # the third candidate (the only one with K = 1) holds the sampled pixel
    assert got_c[1, 2] == 0 and got_c[2, 2] == 0 and got_c[1, 3] == K - 1   # skipped-only and empty: rejected, last candidate used
    if K == 4:                                                     # first accepted: a mask that is positive everywhere
        full = np.full((1, H0, W0), 200, np.uint8)
        tb1 = _tables(sp, 1, V, K, params[:1], (H0, W0))
        assert ops.prep_accept(t(full, DEV), tb1.ptab, tb1.cand, (h, w)).cpu().tolist() == [[0, 0, 1, 0]]


def test_depth_values_192():
    from mvsformer_amd import ops
    sp = _sp()
    H0 = W0 = 16
    tb = _tables(sp, 1, 1, 1, [_params(sp, 1, 1.0, [(0, 0)])], (H0, W0), [425.0], [2.5 * 1.06])
    z = torch.zeros(1, H0, W0, device=DEV)
    chosen = ops.prep_accept(z.to(torch.uint8), tb.ptab, tb.cand, (16, 16), require_positive=False)
    dv = ops.prep_geometry(z, z.to(torch.uint8), tb.ptab, chosen, torch.eye(3, device=DEV).view(1, 1, 3, 3).contiguous(),
                           torch.eye(4, device=DEV).view(1, 1, 4, 4).contiguous(), tb.drange, (16, 16), sp.arange_length(425.0, 2.5 * 1.06, 192))[3]
    want = np.arange(425.0, 2.5 * 1.06 * 192 + 425.0, 2.5 * 1.06, dtype=np.float32)
    assert np.array_equal(dv[0].cpu().numpy(), want) and np.array_equal(want, u.depth_values(425.0, 2.5 * 1.06, 192))


def _jtab(sp, fn_idx, factors, enabled=(True, True, True, True), gamma=None):
    p = sp.TrainParams(view_ids=[0], resize_scales=[1.0], candidates=[(0, 0)], src_offsets=[], fn_idx=list(fn_idx), factors=tuple(factors),
                       gamma=gamma, enabled=tuple(enabled))
    tb = sp.TrainTables(1, 1, 1, device=DEV)
    tb.write([p], (8, 8), [1.0], [1.0])
    return tb.jtab


def _jitter_gpu(sp, img, fn_idx, factors, enabled=(True, True, True, True), gamma=None):
    from mvsformer_amd import ops
    out, lsum, u8 = ops.prep_jitter_tail(t(img, DEV)[None, None], _jtab(sp, fn_idx, factors, enabled, gamma), has_contrast=enabled[1], want_u8=True)
    return out[0, 0].cpu().numpy(), (None if lsum is None else int(lsum[0, 0])), u8[0, 0].cpu().numpy()


def test_jitter_24_orders_and_extremes():
    sp = _sp()
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    f = (0.8, 1.3, 0.7, 0.1)
    for order in itertools.permutations(range(4)):
        out, _, u8 = _jitter_gpu(sp, img, order, f)
        want = u.jitter(img, order, f)
        assert np.array_equal(u8, want), order
        assert np.array_equal(out, u.tail(want)), order
    half = img.copy()                                              # mean(L) ends in .5: 384 pixels, the sum of L is 384 * k + 192
    half[...] = 100
    half[:8] = 101
    assert int(u.luma(half).astype(np.int64).sum()) * 2 % half[..., 0].size == 0 and u.luma(half).mean() % 1 == 0.5
    for op, vals, im in ((0, (0.0, 2.5), img), (1, (0.0, 3.0), half), (1, (0.0, 3.0), img), (2, (0.0, 2.0), img), (3, (-0.5, 0.0, 0.5), img)):
        for v in vals:
            fac = [1.0, 1.0, 1.0, 0.0]
            fac[op] = v
            en = tuple(k == op for k in range(4))
            assert np.array_equal(_jitter_gpu(sp, im, (0, 1, 2, 3), fac, en)[2], u.jitter(im, (0, 1, 2, 3), fac, en)), (op, v)
    en = (False, True, True, True)                                 # brightness's range is None
    assert np.array_equal(_jitter_gpu(sp, img, (2, 0, 1, 3), (0.1, 1.4, 0.6, -0.2), en)[2], u.jitter(img, (2, 0, 1, 3), (0.1, 1.4, 0.6, -0.2), en))


def test_luma_sum_is_the_integer_sum():
    sp = _sp()
    img = np.random.default_rng(6).integers(0, 256, (33, 65, 3), dtype=np.uint8)
    _, lsum, _ = _jitter_gpu(sp, img, (0, 2, 1, 3), (1.2, 1.1, 0.9, 0.05))
    before = u.saturation(u.brightness(img, 1.2), 0.9)
    assert lsum == int(u.luma(before).astype(np.int64).sum())


@pytest.mark.parametrize("op", [3, 2])
def test_colour_cube(op):
    """All 2^24 colours as one 4096x4096 image through hue alone / saturation alone."""
    sp = _sp()
    c = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    cube = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8)
    fac = [1.0, 1.0, 1.0, 0.0]
    fac[op] = 0.3 if op == 3 else 1.7
    en = tuple(k == op for k in range(4))
    got = _jitter_gpu(sp, cube, (0, 1, 2, 3), fac, en)[2]
    assert np.array_equal(got, u.jitter(cube, (0, 1, 2, 3), fac, en))


def test_tail_exact_and_gamma():
    """Without gamma bit-equal to numpy fp32.  With gamma: torch-CPU's fp32 pow-clamp-normalize error against fp64 on these inputs is
    measured, and the kernel is allowed four times that (another powf of the same nominal accuracy)."""
    from mvsformer_amd import ops
    sp = _sp()
    img = np.arange(256 * 3, dtype=np.int64).reshape(16, 16, 3) % 256
    img = img.astype(np.uint8)
    out = ops.prep_jitter_tail(t(img, DEV)[None, None])[0][0, 0].cpu().numpy()
    assert np.array_equal(out, u.tail(img))
    for gamma in (0.7, 1.5):
        got = _jitter_gpu(sp, img, (0, 1, 2, 3), (1.0, 1.0, 1.0, 0.0), (False,) * 4, gamma=gamma)[0]
        w64 = u.tail_f64(img, gamma)
        e_torch = np.abs(u.tail(img, gamma).astype(np.float64) - w64).max()
        e_hip = np.abs(got.astype(np.float64) - w64).max()
        print("gamma %.1f: torch-CPU fp32 max abs err %.3e, kernel %.3e" % (gamma, e_torch, e_hip))
        assert e_hip <= 4 * e_torch


@pytest.mark.parametrize("H0,W0", [(37, 53), (75, 100)])
@pytest.mark.parametrize("H,W", [(64, 64), (64, 128)])
def test_eval_resize(H0, W0, H, W):
    sp = _sp()
    src = _sources(H0, W0, seed=9)
    intr = np.random.default_rng(1).uniform(1, 2000, (3, 3, 3)).astype(np.float32)
    for pad in (0, 4):
        got, k = sp.prepare_eval_views(t(src, DEV), intr, H, W, tt_pad=bool(pad))
        from mvsformer_amd import ops
        got_u8 = ops.prep_eval_resize(t(src, DEV), (H, W), pad_rows=pad, want="u8").cpu().numpy()
        for v in range(3):
            want = u.linear_resize(src[v], H, W, pad)
            assert np.array_equal(got_u8[v], want)
            assert np.abs(got_u8[v].astype(np.float64) - u.linear_resize_f64(src[v], H, W, pad)).max() <= 1.0
            assert np.array_equal(got[v].cpu().numpy(), u.tail(want))
            wk = intr[v].copy()
            wk[0, :] *= np.float32(1.0 * W / W0)
            wk[1, :] *= np.float32(1.0 * H / (H0 + 2 * pad))
            assert np.array_equal(k[v], wk)
    # the padding rows equal the edge rows: an identity-size resize of the padded image
    same = sp.ops.prep_eval_resize(t(src, DEV), (H0 + 8, W0), pad_rows=4, want="u8").cpu().numpy()
    assert np.array_equal(same, np.pad(src, ((0, 0), (4, 4), (0, 0), (0, 0)), "edge"))


def _batch_inputs(B, V, H0, W0, seed):
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (B, V, H0, W0, 3), dtype=np.uint8)
    depth = rng.uniform(400, 900, (B, H0, W0)).astype(np.float32)
    mask = rng.integers(0, 40, (B, H0, W0)).astype(np.uint8)
    intr = rng.uniform(0.5, 900, (B, V, 3, 3)).astype(np.float32)
    extr = rng.normal(size=(B, V, 4, 4)).astype(np.float32)
    return imgs, depth, mask, intr, extr


def _want_batch(inp, params, crop, dmin, dint, nd, augment):
    imgs, depth, mask, intr, extr = inp
    h, w = crop
    out = []
    for b, p in enumerate(params):
        oy, ox, ok, _ = u.accept(mask[b], p.resize_scales[0], p.candidates, h, w)
        offs = [(oy, ox)] + [(oy, ox) if o is None else o for o in p.src_offsets]
        views = []
        for v, rs in enumerate(p.resize_scales):
            H0, W0 = imgs.shape[2:4]
            rh, rw = (int(H0 * rs), int(W0 * rs)) if rs != 1.0 else (H0, W0)
            c = u.area_resize(imgs[b, v], rh, rw)[offs[v][0]:offs[v][0] + h, offs[v][1]:offs[v][1] + w]
            views.append(u.tail(u.jitter(c, p.fn_idx, p.factors, p.enabled), p.gamma) if augment else u.tail(c))
        wd, wm = u.crop_maps(depth[b], mask[b], p.resize_scales[0], oy, ox, h, w)
        out.append(dict(imgs=np.stack(views), depth=wd, mask=wm, proj=u.proj_matrices(intr[b], extr[b], p.resize_scales, offs),
                        dv=u.depth_values(dmin[b], dint[b], nd), ok=ok))
    return out


def _check_batch(got, want, augment):
    for b, wb in enumerate(want):
        gi = got["imgs"][b].cpu().numpy()
        if augment:
            # gamma: the kernel's powf against torch's.  Each is within 1 ulp of a value <= 1 (2^-23 at the most, two of them), the
            # subtraction and the division by std add as much again: 8 * 2^-23 over the smallest std
            assert np.abs(gi.astype(np.float64) - wb["imgs"]).max() <= 8 * 2.0 ** -23 / 0.224
        else:
            assert np.array_equal(gi, wb["imgs"])
        for s in ("stage1", "stage2", "stage3", "stage4"):
            assert np.array_equal(got["depth"][s][b].cpu().numpy(), wb["depth"][s])
            assert np.array_equal(got["mask"][s][b].cpu().numpy(), wb["mask"][s])
            assert np.array_equal(got["proj_matrices"][s][b].cpu().numpy(), wb["proj"][s])
        assert np.array_equal(got["depth_values"][b].cpu().numpy(), wb["dv"])
        assert int(got["offset"][b, 2]) == wb["ok"]


def _draw(sp, seed, crop, src_hw, augment, V, K):
    import random
    random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
    aug = dict(brightness=0.2, contrast=0.1, saturation=0.1, hue=0.05, min_gamma=0.7, max_gamma=1.5)
    return sp.draw_train_params(0, list(range(1, 8)), V, crop, src_hw=src_hw, augment=augment, aug_args=aug, resize_range=(1.0, 1.2), K=K)


@pytest.mark.parametrize("augment", [False, True])
def test_prepare_train_batch_eager_and_captured(augment):
    """B = 2, V = 3, 96x128 sources, 64x64 crop: equals the chain of restatements; under CapturedStep two replays with the parameter
    tables rewritten in between each equal the restatements for their parameters."""
    from mvsformer_amd.graphs import CapturedStep
    sp = _sp()
    B, V, K, crop, hw, nd = 2, 3, 4, (64, 64), (96, 128), 7
    inp = _batch_inputs(B, V, *hw, seed=11)
    dmin, dint = [425.0, 480.0], [2.65, 2.5 * 1.06]
    L = sp.arange_length(dmin[0], dint[0], nd)
    assert L == sp.arange_length(dmin[1], dint[1], nd)
    dev_in = [t(a, DEV) for a in inp]
    tb = sp.TrainTables(B, V, K, device=DEV)
    sets = [[_draw(sp, 10 * r + b, crop, hw, augment, V, K) for b in range(B)] for r in range(3)]
    tb.write(sets[0], hw, dmin, dint)
    got = sp.prepare_train_batch(*dev_in, tb, crop, L, augment=augment)
    _check_batch(got, _want_batch(inp, sets[0], crop, dmin, dint, nd, augment), augment)
    step = CapturedStep(lambda: sp.prepare_train_batch(*dev_in, tb, crop, L, augment=augment), warmup=2)
    for r in (1, 2):
        tb.write(sets[r], hw, dmin, dint)
        step.graph.replay()
        torch.cuda.synchronize()
        _check_batch(step.outputs, _want_batch(inp, sets[r], crop, dmin, dint, nd, augment), augment)


def test_eval_views_second_resize_to_the_standard_size():
    """fix_res (general_eval.py:187-205): a view whose scale_mvs_input result differs from the scene's standard size is resized again,
    8-bit to 8-bit, and its intrinsics are scaled a second time."""
    sp = _sp()
    src = _sources(75, 100, seed=12)
    intr = np.random.default_rng(2).uniform(1, 2000, (3, 3, 3)).astype(np.float32)
    got, k = sp.prepare_eval_views(t(src, DEV), intr, 64, 128, standard_hw=(64, 64))
    for v in range(3):
        want = u.linear_resize(u.linear_resize(src[v], 64, 128), 64, 64)
        assert np.array_equal(got[v].cpu().numpy(), u.tail(want))
        wk = intr[v].copy()
        wk[0, :] *= np.float32(1.0 * 128 / 100)
        wk[1, :] *= np.float32(1.0 * 64 / 75)
        wk[0, :] *= np.float32(1.0 * 64 / 128)
        wk[1, :] *= np.float32(1.0 * 64 / 64)
        assert np.array_equal(k[v], wk)
    same, k2 = sp.prepare_eval_views(t(src, DEV), intr, 64, 128, standard_hw=(64, 128))
    assert np.array_equal(same[0].cpu().numpy(), u.tail(u.linear_resize(src[0], 64, 128))) and np.array_equal(k2[0], sp.scale_intrinsics(intr[0], (75, 100), (64, 128)))


def _mvsformer_p_args():
    return dict(fix=True, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
                depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
                vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                              att_fusion=True, nhead=6, vit_path=""))


def _scene_batch(B, V, H0, W0, seed):
    """A renderable batch: textured fronto-parallel views of one scene, so that the projection matrices are those of real cameras."""
    from mvsformer_amd import synth
    sc = synth.make_scene(V, H0, W0, seed=seed)
    rng = np.random.default_rng(seed)
    imgs = rng.integers(0, 256, (B, V, H0, W0, 3), dtype=np.uint8)
    depth = np.stack([synth.plane_depth(sc, 1).to(torch.float32).numpy()] * B)
    mask = np.full((B, H0, W0), 255, np.uint8)
    intr = np.stack([np.stack([sc.K.to(torch.float32).numpy()] * V)] * B)
    extr = np.stack([sc.E.to(torch.float32).numpy()] * B)
    return (imgs, depth, mask, np.ascontiguousarray(intr), np.ascontiguousarray(extr)), float(depth.min()), float(depth.max())


def test_prepared_batch_feeds_dinomvsnet_and_the_loss():
    """The batch dict is what the existing entry points take: once through DINOMVSNet (training mode) and ce_loss_stage4, finite loss."""
    import mvsformer_amd as m
    from mvsformer_amd import losses
    from oracle.weights import load_model_shapes, make_model_state_dict
    sp = _sp()
    B, V, K, crop, hw, nd = 2, 3, 4, (64, 64), (96, 128), 192
    inp, dlo, dhi = _scene_batch(B, V, *hw, seed=4)
    dmin = [0.8 * dlo] * B
    dint = [(1.25 * dhi - 0.8 * dlo) / nd] * B
    L = sp.arange_length(dmin[0], dint[0], nd)
    tb = sp.TrainTables(B, V, K, device=DEV)
    tb.write([_draw(sp, 40 + b, crop, hw, True, V, K) for b in range(B)], hw, dmin, dint)
    batch = sp.prepare_train_batch(*[t(a, DEV) for a in inp], tb, crop, L, augment=True)
    assert batch["imgs"].shape == (B, V, 3, 64, 64) and batch["imgs"].dtype == torch.float32 and batch["imgs"].is_contiguous()
    for s, f in (("stage1", 8), ("stage2", 4), ("stage3", 2), ("stage4", 1)):
        assert batch["proj_matrices"][s].shape == (B, V, 2, 4, 4) and batch["proj_matrices"][s].is_contiguous()
        assert batch["depth"][s].shape == (B, 64 // f, 64 // f) == batch["mask"][s].shape and batch["depth"][s].is_contiguous()
    net = m.DINOMVSNet(_mvsformer_p_args())
    net.load_state_dict(make_model_state_dict(load_model_shapes(), 7), strict=True)
    net = net.to(DEV).train()
    out = net(batch["imgs"], batch["proj_matrices"], batch["depth_values"], tmp=[5.0, 5.0, 5.0, 1.0])
    ls = losses.ce_loss_stage4(out, batch["depth"], batch["mask"], [1.0, 1.0, 1.0, 1.0], inverse_depth=True)
    total = sum(ls.values())
    print("prepared batch -> DINOMVSNet -> ce_loss_stage4: %.6f" % float(total))
    assert torch.isfinite(total).all() and int(batch["offset"][:, 2].sum()) == B


def test_scan_tool_accepts_any_size_and_writes_scaled_cameras(tmp_path):
    """tools/infer_scan.py --max_h 64 --max_w 64 on a three-view 75x100 synthetic scan (neither side a multiple of 64) with a random
    checkpoint: it runs, and OUT/cams/*_cam.txt carry scale_mvs_input's intrinsics."""
    import importlib.util
    import os
    from PIL import Image
    from conftest import REPO
    from mvsformer_amd import data_io, synth
    from oracle.weights import load_model_shapes, make_model_state_dict
    sp = _sp()
    spec = importlib.util.spec_from_file_location("infer_scan_gpu", os.path.join(REPO, "tools", "infer_scan.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    H0, W0, NV = 75, 100, 3
    sc = synth.make_scene(NV, H0, W0, seed=6)
    scan, out = tmp_path / "scan", tmp_path / "out"
    (scan / "cams").mkdir(parents=True), (scan / "images").mkdir()
    rng = np.random.default_rng(8)
    depth = synth.plane_depth(sc, 1)
    dlo, dhi = 0.8 * float(depth.min()), 1.25 * float(depth.max())
    for v in range(NV):
        Image.fromarray(rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)).save(scan / "images" / ("%08d.png" % v))
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3], cam[1, 3, 3] = sc.E[v].numpy(), sc.K.numpy(), 1.0
        data_io.write_cam(str(scan / "cams" / ("%08d_cam.txt" % v)), cam)
        with open(scan / "cams" / ("%08d_cam.txt" % v)) as f:
            lines = f.read().split("\n")
        lines[11] = "%r %r" % (dlo, (dhi - dlo) / 192)
        with open(scan / "cams" / ("%08d_cam.txt" % v), "w") as f:
            f.write("\n".join(lines))
    with open(scan / "pair.txt", "w") as f:
        f.write("%d\n" % NV + "".join("%d\n2 %d 1.0 %d 1.0\n" % (v, (v + 1) % NV, (v + 2) % NV) for v in range(NV)))
    ckpt = tmp_path / "model.pth"
    torch.save({"state_dict": make_model_state_dict(load_model_shapes(), 7)}, ckpt)
    argv = ["--scan", str(scan), "--checkpoint", str(ckpt), "--out", str(out), "--num_view", "3", "--max_h", "64", "--max_w", "64"]
    tool.main(argv)
    for v in range(NV):
        k0, e0 = data_io.read_camera_parameters(str(scan / "cams" / ("%08d_cam.txt" % v)))
        k1, e1 = data_io.read_camera_parameters(str(out / "cams" / ("%08d_cam.txt" % v)))
        want = sp.scale_intrinsics(k0, (H0, W0), (64, 64))
        assert np.allclose(k1, want, rtol=1e-6, atol=0) and np.allclose(e1, e0, rtol=1e-6, atol=1e-7)       # one decimal round trip
        assert abs(k1[0, 0] / k0[0, 0] - 0.64) < 1e-6 and abs(k1[1, 1] / k0[1, 1] - 64 / 75) < 1e-6
        d, _ = data_io.read_pfm(str(out / "depth_est" / ("%08d.pfm" % v)))
        assert d.shape[:2] == (64, 64) and np.isfinite(d).all()
    with pytest.raises(SystemExit):                              # without the flags the tool still refuses a size it cannot take
        tool.main(argv[:-4])
