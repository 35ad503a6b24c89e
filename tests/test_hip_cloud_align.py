"""The cloud-alignment kernels and the ICP built on them (csrc/cloud_align.hip, mvsformer_amd/cloud_eval.py) against the numpy fp64
restatements of tests/cloud_align_util.py.  Transform and crop mask: bit for bit.  Pair sums: within the bound of any fp64 summation order,
and bit-identical from call to call.  ICP: an exact case against the known transform, a noisy case against the restated loop."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_align_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1025)
RINGS = {"triangle": U.TRIANGLE, "l_ring": U.L_RING, "star64": U.star_ring()}


def _ce():
    from mvsformer_amd import cloud_eval
    return cloud_eval


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dtype)


def _same_bits(got, want):
    """Bit for bit, except that a NaN matches any NaN (its sign and payload are the processor's choice)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ------------------------------------------------------------------------------------------------------------ transform
@pytest.mark.parametrize("n", SIZES)
def test_transform_is_the_restatement_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    p = (rng.normal(0.0, 50.0, (n, 3)) + [1000.0, -300.0, 20.0]).astype(np.float32)
    if n >= 63:
        p[5], p[17], p[40, 1] = [np.nan, 1.0, 2.0], [np.inf, -np.inf, 0.0], np.inf
    T = U.similarity(37.0, (1.0, -2.0, 0.5), 1.37, (12.5, -7.25, 3.0))
    got = _ce().transform(_dev(p), T).cpu().numpy()
    want = U.transform_ref(p, T)
    assert got.shape == (n, 3) and _same_bits(got, want)
    if n >= 63:
        assert np.isnan(got[5]).all() and not np.isfinite(got[17]).any() and not np.isfinite(got[40]).all()
    got = _ce().transform(_dev(p), T.tolist()).cpu().numpy()                  # nested lists
    assert _same_bits(got, want)


def test_transform_refuses_a_projective_matrix():
    from mvsformer_amd._lib import MvsHipError
    p = _dev(np.zeros((4, 3), np.float32))
    T = np.eye(4)
    T[3, 0] = 1e-3
    for bad in (T, np.eye(3), np.eye(4)[:3], np.full((4, 4), np.nan)):
        with pytest.raises(MvsHipError):
            _ce().transform(p, bad)


# ----------------------------------------------------------------------------------------------------------------- crop
@pytest.mark.parametrize("ring", sorted(RINGS))
@pytest.mark.parametrize("n", SIZES)
def test_crop_mask_is_the_restatement_exactly(n, ring):
    poly = np.asarray(RINGS[ring], np.float64)
    for axis in (0, 1, 2):
        p = U.crop_points(n, poly, axis, seed=7 * n + axis)
        if n >= 63:
            p[3, 0], p[9, 2], p[11, 1] = np.nan, np.inf, -np.inf
        want = U.crop_ref(p, axis, 0.0, 1.0, poly)
        got = _ce().crop_polygon(_dev(p), "XYZ"[axis], 0.0, 1.0, poly)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want), (axis, int((got.cpu().numpy() != want).sum()))
        poly3 = np.insert(poly, axis, 123.0, axis=1)                          # [K,3]: the orthogonal coordinate is ignored
        assert np.array_equal(_ce().crop_polygon(_dev(p), axis, 0.0, 1.0, poly3).cpu().numpy(), want)
        if n == 1025:
            assert 0 < want.sum() < n and not want[[3, 9, 11]].any()


def test_crop_refuses_more_vertices_than_are_built():
    from mvsformer_amd._lib import MvsHipError
    p = _dev(np.zeros((4, 3), np.float32))
    assert len(RINGS["star64"]) == U.MAX_K
    with pytest.raises(MvsHipError):
        _ce().crop_polygon(p, 2, 0.0, 1.0, U.star_ring(U.MAX_K + 1))
    with pytest.raises(MvsHipError):
        _ce().crop_polygon(p, "W", 0.0, 1.0, U.TRIANGLE)
    with pytest.raises(MvsHipError):
        _ce().crop_polygon(p, 2, 0.0, 1.0, U.TRIANGLE[:2])


# ------------------------------------------------------------------------------------------------------------ pair sums
BLOCK = 256
PAIR_SIZES = (1, 63, 64, 65, BLOCK + 1, 4 * BLOCK + 1, 1024 * BLOCK + BLOCK + 1)    # the last: more points than lanes (the grid-stride loop)


def _pair_record(src, dst, idx, dist, origin):
    from mvsformer_amd import ops
    rec = ops.align_pair_sums(_dev(src), _dev(dst), _dev(idx), _dev(dist), origin).cpu()
    return rec, _ce().PairSums.from_record(rec, origin)


@pytest.mark.parametrize("mix", ["none", "all", "every_other"])
@pytest.mark.parametrize("m", PAIR_SIZES)
def test_pair_sums_within_the_bound_of_any_summation_order(m, mix):
    rng = np.random.default_rng(m)
    offset = np.array([1000.0, -1000.0, 1000.0])
    n = 777
    dst = (rng.normal(0.0, 2.0, (n, 3)) + offset).astype(np.float32)
    idx = rng.integers(0, n, m)
    src = (dst[idx].astype(np.float64) + rng.normal(0.0, 0.05, (m, 3))).astype(np.float32)
    if mix == "all":
        idx[:] = -1
    elif mix == "every_other":
        idx[::2] = -1
    if m > 64:
        src[1] = [np.nan, 0.0, 0.0]
        idx[1] = -1
    dist = rng.uniform(0.0, 0.1, m).astype(np.float32)
    rec, got = _pair_record(src, dst, idx, dist, offset)
    rec2, _ = _pair_record(src, dst, idx, dist, offset)
    assert torch.equal(rec, rec2)                                             # bit-identical from call to call
    want, mags = U.pair_sums_ref(src, dst, idx, dist, offset)
    assert got.n == want["n"] and got.n_finite == want["n_finite"] and not rec[20:].any()
    if mix == "all":
        assert got.n == 0 and not rec[2:20].any()
    for key in ("sp", "sq", "sqp", "spp", "sqq", "sdd"):
        err = np.abs(np.asarray(getattr(got, key)) - np.asarray(want[key]))
        assert (err <= m * 2.0 ** -52 * np.asarray(mags[key])).all(), (key, err.max())
    if mix == "none" and m >= 63:
        # the origin is used: about it the covariance survives; about zero, with coordinates near 1e3, sum q p^T would have to carry it
        # in the last digits of numbers near 1e6 * m
        T = _ce().umeyama(got, True)
        ref = U.umeyama_ref(want)
        assert np.abs(T - ref).max() <= 1e-9 * 1e3
        zero, _ = U.pair_sums_ref(src, dst, idx, dist, (0.0, 0.0, 0.0))
        assert np.abs(zero["sqp"]).max() > 1e5 * np.abs(want["sqp"]).max() / 10


def test_pair_sums_skip_an_index_past_the_target():
    src = np.ones((5, 3), np.float32)
    dst = np.ones((3, 3), np.float32)
    idx = np.array([0, 3, 2, 1 << 40, -7], np.int64)
    _, got = _pair_record(src, dst, idx, np.ones(5, np.float32), (0.0, 0.0, 0.0))
    assert got.n == 2 and got.n_finite == 5 and got.sdd == 2.0


# ------------------------------------------------------------------------------------------------------------------ icp
def test_icp_exact_case_lands_within_four_roundings():
    """Identical points, every first correspondence the true one: fitness 1 and, after five iterations, every transformed point within
    ``2^-22 max|coord|`` of where the true transform puts it (one fp32 rounding of a transformed coordinate, times four).  The restated
    loop meets this on the CPU (tests/test_cloud_align_refs.py: 1.6e-8 against 9.3e-6)."""
    src, dst, T_true, s = U.exact_case()
    res = _ce().icp(_dev(src), _dev(dst), s, fitness_tol=0.0, rmse_tol=0.0, max_iter=5)
    err = np.abs(U.apply64(res.T, src) - U.apply64(T_true, src)).max()
    print("exact case: fitness %r, rmse %.3e, max |T x - T_true x| = %.3e (bound %.3e)" % (res.fitness, res.inlier_rmse, err, 2.0 ** -22 * np.abs(dst).max()))
    assert res.fitness == 1.0 and res.iterations == 5 and not res.converged
    assert err <= 2.0 ** -22 * np.abs(dst).max()


def test_icp_general_case_follows_the_restated_loop():
    """Noise, 20 % outliers, a start several spacings off.  The device differs from the restated loop (fp32 argmin, exact sums) by summation
    order only; the one other legitimate difference, an argmin taken on fp32 against fp64 distances, is measured here on the CPU as
    ``|T_ref32 - T_ref64|`` (0 on this fixture: no near-tie flips) and allowed four times.  The summation order may move each sum by
    ``M 2^-53`` of its terms' magnitudes; about the bounding-box centre those are within ~12 x the variances the solve divides by, the
    sheet's two large singular values are well separated from nothing they could be confused with, and iterations contract - allowed:
    ``100 M 2^-52 max|coord|`` in the Frobenius norm of ``T`` (4.4e-9 here)."""
    src, dst, T_true, init, threshold = U.general_case()
    a = U.icp_ref(src, dst, threshold, init=init, max_iter=40)
    b = U.icp_ref(src, dst, threshold, init=init, max_iter=40, fp32=False)
    argmin_term = float(np.linalg.norm(a[0] - b[0]))
    order_term = 100.0 * len(src) * 2.0 ** -52 * float(np.abs(dst).max())
    res = _ce().icp(_dev(src), _dev(dst), threshold, init=init, max_iter=40)
    diff = float(np.linalg.norm(res.T - a[0]))
    print("general case: iterations %d (restated %d), fitness %.6f (%.6f), |T_dev - T_ref| = %.3e, allowed 4 x %.3e + %.3e" % (
        res.iterations, a[3], res.fitness, a[1], diff, argmin_term, order_term))
    assert res.iterations == a[3] and res.converged and a[4]
    assert res.fitness == a[1] and abs(res.inlier_rmse - a[2]) <= 1e-9
    assert diff <= 4.0 * argmin_term + order_term


def test_icp_without_scaling_keeps_scale_one():
    dst, s = U.sheet()
    centre = dst.astype(np.float64).mean(0)
    R = U.similarity(0.3, (0.2, 0.1, 1.0), 1.0, (0.05, -0.04, 0.03), about=centre)
    src = U.apply64(np.linalg.inv(R), dst).astype(np.float32)
    res = _ce().icp(_dev(src), _dev(dst), 2.0 * s, with_scaling=False, max_iter=10)
    A = res.T[:3, :3]
    assert np.abs(A @ A.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(A) - 1.0) <= 1e-12
    assert np.abs(U.apply64(res.T, src) - dst).max() <= 1e-4


# -------------------------------------------------------------------------------------------------- the T&T protocol
def test_evaluate_tt_reaches_the_score_of_the_true_transform():
    """After the default stages the F-score at ``dtau`` is that of the true transform, up to the share of points that a residual of the
    exact case's size (``2^-22 max|coord|``) can carry across ``dtau`` - counted here from the distances under the true transform;
    with ``init`` alone it is lower."""
    ce = _ce()
    pred, gt, T_true, init, crop, dtau = U.tt_scene()
    dp, dg = _dev(pred), _dev(gt)
    truth = ce.evaluate_tt(dp, dg, T_true, crop, dtau, refine=False)
    rough = ce.evaluate_tt(dp, dg, init, crop, dtau, refine=False)
    fine = ce.evaluate_tt(dp, dg, init, crop, dtau)
    # the share: thinned clouds as evaluate sees them, distances both ways under the true transform
    moved = ce.transform(dp, T_true)
    pc = ce.voxel_downsample(moved[ce.crop_polygon(moved, crop["orthogonal_axis"], crop["axis_min"], crop["axis_max"], crop["bounding_polygon"])], 0.5 * dtau)
    gc = ce.voxel_downsample(dg[ce.crop_polygon(dg, crop["orthogonal_axis"], crop["axis_min"], crop["axis_max"], crop["bounding_polygon"])], 0.5 * dtau)
    r = 2.0 ** -22 * float(np.abs(gt).max())
    d_pg, d_gp = ce.nn_distance(pc, gc, 5.0 * dtau)[0], ce.nn_distance(gc, pc, 5.0 * dtau)[0]
    share_p = float(((d_pg - dtau).abs() <= r).float().mean())
    share_g = float(((d_gp - dtau).abs() <= r).float().mean())
    f_true, f_fine, f_rough = truth["fscore"][0], fine["fscore"][0], rough["fscore"][0]
    print("T&T scene: cropped %d / %d of %d / %d, F true %.6f, after ICP %.6f, init alone %.6f; shares within %.1e of dtau: %.2e %.2e; stages %s" % (
        fine["n_pred_cropped"], fine["n_gt_cropped"], len(pred), len(gt), f_true, f_fine, f_rough, r, share_p, share_g, fine["stages"]))
    assert 0 < truth["n_pred_cropped"] < len(pred) and 0 < truth["n_gt_cropped"] < len(gt)                 # the volume cuts part of it away
    assert 0.3 < f_true < 0.95 and len(fine["stages"]) == 3 and np.array(fine["T"]).shape == (4, 4)
    # F = 2PR / (P + R) moves by at most |dP| + |dR|
    assert abs(f_fine - f_true) <= share_p + share_g + 2.0 ** -50
    assert f_rough < f_true - 0.1
    T, results = ce.register_tt(dp, dg, init, crop, dtau, stages=[(("uniform", 1000), 8.0 * dtau, 3)])
    assert len(results) == 1 and results[0].iterations <= 3 and T.shape == (4, 4)


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from mvsformer_amd._lib import MvsHipError
    ce = _ce()
    cpu = torch.zeros(8, 3)
    dev = _dev(np.random.default_rng(0).normal(0, 1, (8, 3)).astype(np.float32))
    empty = torch.zeros(0, 3, device="cuda:0")
    for call in (lambda: ce.transform(cpu, np.eye(4)), lambda: ce.crop_polygon(cpu, 2, 0.0, 1.0, U.TRIANGLE), lambda: ce.icp(cpu, dev, 1.0),
                 lambda: ce.icp(dev, cpu, 1.0), lambda: ce.evaluate_tt(cpu, dev, np.eye(4), None, 0.1),
                 lambda: ce.icp(empty, dev, 1.0), lambda: ce.icp(dev, empty, 1.0),                          # empty clouds
                 lambda: ce.icp(dev + 100.0, dev, 1.0),                                                      # no correspondences
                 lambda: ce.icp(dev, dev, 0.0), lambda: ce.icp(dev, dev, 1.0, max_iter=0), lambda: ce.icp(dev, dev, 1.0, init=np.eye(3))):
        with pytest.raises(MvsHipError):
            call()
    assert ce.transform(empty, np.eye(4)).shape == (0, 3) and ce.crop_polygon(empty, 2, 0.0, 1.0, U.TRIANGLE).shape == (0,)
