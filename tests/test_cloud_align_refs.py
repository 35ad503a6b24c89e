"""The yardsticks of tests/test_hip_cloud_align.py (tests/cloud_align_util.py) against things that can be known, the host-side parts of the
feature (``umeyama``, the two file readers) and its plumbing (header, ctypes table, library).  No GPU."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_align_util as U  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvs_align_transform", "mvs_align_crop_polygon", "mvs_align_pair_sums_workspace_bytes", "mvs_align_pair_sums")


def _record(s):
    from mvsformer_amd import cloud_eval
    return cloud_eval.PairSums(s["n"], s["n_finite"], s["sp"], s["sq"], s["sqp"], s["spp"], s["sqq"], s["sdd"], s["origin"])


def _umeyama_pkg(s, with_scaling=True):
    from mvsformer_amd import cloud_eval
    return cloud_eval.umeyama(_record(s), with_scaling)


@pytest.mark.parametrize("solver", [U.umeyama_ref, _umeyama_pkg], ids=["restated", "package"])
def test_umeyama_recovers_a_random_similarity_from_exact_pairs(solver):
    rng = np.random.default_rng(0)
    for trial in range(5):
        p = rng.normal(0.0, 1.0, (200, 3))
        T = U.similarity(rng.uniform(-170, 170), rng.normal(size=3), rng.uniform(0.3, 3.0), rng.normal(size=3))
        got = solver(U.sums_of_pairs(p, U.apply64(T, p)))
        assert np.abs(got - T).max() <= 1e-12 * max(1.0, np.abs(T).max()), trial
        origin = p.mean(0) + 0.1
        got = solver(U.sums_of_pairs(p, U.apply64(T, p), origin))             # the origin drops out
        assert np.abs(got - T).max() <= 1e-12 * max(1.0, np.abs(T).max()), trial
    R = U.similarity(33.0, (1, 2, 3), 1.0, (0.5, -1.0, 2.0))
    got = solver(U.sums_of_pairs(p, U.apply64(R, p)), False)
    assert np.abs(got - R).max() <= 1e-12 and abs(np.linalg.det(got[:3, :3]) - 1.0) <= 1e-12


@pytest.mark.parametrize("solver", [U.umeyama_ref, _umeyama_pkg], ids=["restated", "package"])
def test_umeyama_planar_pairs_give_a_rotation_not_a_reflection(solver):
    """All points in one plane: the covariance has rank 2 and the SVD alone may return a reflection; S = diag(1, 1, -1) repairs it."""
    rng = np.random.default_rng(1)
    seen_negative = False
    for trial in range(20):
        p = np.concatenate([rng.normal(0.0, 1.0, (100, 2)), np.zeros((100, 1))], 1)
        T = U.similarity(rng.uniform(-170, 170), rng.normal(size=3), 1.3, rng.normal(size=3))
        s = U.sums_of_pairs(p, U.apply64(T, p))
        Usvd, _, Vt = np.linalg.svd(s["sqp"] / s["n"] - np.outer(s["sq"] / s["n"], s["sp"] / s["n"]))
        seen_negative |= np.linalg.det(Usvd) * np.linalg.det(Vt) < 0
        got = solver(s)
        assert np.linalg.det(got[:3, :3]) > 0 and np.abs(got - T).max() <= 1e-10, trial
    assert seen_negative                                                      # the case did occur


def test_umeyama_refuses_what_determines_no_transform():
    from mvsformer_amd import cloud_eval
    from mvsformer_amd._lib import MvsHipError
    line = np.outer(np.linspace(0, 1, 50), [1.0, 2.0, 3.0])
    for s in (U.sums_of_pairs(line[:2], line[:2]), U.sums_of_pairs(line, 2.0 * line), U.sums_of_pairs(np.ones((10, 3)), np.ones((10, 3)))):
        with pytest.raises(MvsHipError):
            cloud_eval.umeyama(_record(s), True)
        with pytest.raises(ValueError):
            U.umeyama_ref(s)
    bad = U.sums_of_pairs(np.eye(3), np.eye(3))
    bad["sqp"] = bad["sqp"] * np.nan
    with pytest.raises(MvsHipError):
        cloud_eval.umeyama(_record(bad), True)


def test_polygon_rule_on_hand_listed_points():
    tri = [((1, 1), True), ((3.5, 0.25), True), ((2.5, 2.5), False), ((-0.1, 1), False), ((1, -0.1), False), ((3, 3), False), ((0.5, 3.4), True)]
    ell = [((0.5, 0.5), True), ((3.5, 0.5), True), ((0.5, 3.5), True), ((2.0, 2.0), False), ((1.5, 1.5), False), ((3.9, 0.9), True),
           ((4.1, 0.5), False), ((0.9, 3.9), True), ((1.1, 3.9), False), ((3.9, 1.1), False)]
    for ring, cases in ((U.TRIANGLE, tri), (U.L_RING, ell)):
        for axis in (0, 1, 2):
            ua, va = U.OTHER_AXES[axis]
            for (u, v), want in cases:
                for w, in_slab in ((0.5, True), (0.0, True), (1.0, True), (np.nextafter(np.float32(0), np.float32(-1)), False),
                                   (np.nextafter(np.float32(1), np.float32(2)), False)):
                    p = np.zeros((1, 3), np.float32)
                    p[0, ua], p[0, va], p[0, axis] = u, v, w
                    assert bool(U.crop_ref(p, axis, 0.0, 1.0, ring)[0]) == (want and in_slab), (ring, axis, u, v, w)
    # v equal to a vertex's v: the edge ending there and the edge starting there count once together, not twice and not zero times
    assert bool(U.crop_ref(np.array([[0.5, 1.0, 0.5]], np.float32), 2, 0.0, 1.0, U.L_RING)[0])
    assert not bool(U.crop_ref(np.array([[2.0, 1.0, 0.5]], np.float32), 2, 0.0, 1.0, U.L_RING)[0])          # on the notch's lower edge: v > 1 is false for both ends
    assert not bool(U.crop_ref(np.array([[np.nan, 1.0, 0.5]], np.float32), 2, 0.0, 1.0, U.L_RING)[0])
    assert not bool(U.crop_ref(np.array([[-np.inf, 0.5, 0.5]], np.float32), 2, 0.0, 1.0, U.L_RING)[0])       # u = -inf is left of every crossing
    assert len(U.star_ring()) == U.MAX_K


def test_transform_restatement_rounds_once_in_the_stated_order():
    T = U.similarity(31.0, (1, 2, 3), 1.7, (0.1, 0.2, 0.3))
    p = np.random.default_rng(2).normal(0, 100, (500, 3)).astype(np.float32)
    got = U.transform_ref(p, T)
    assert got.dtype == np.float32 and np.abs(got - U.apply64(T, p)).max() <= 2.0 ** -24 * np.abs(got).max() * 1.001
    x, y, z = (np.float64(v) for v in p[7])
    assert got[7, 1] == np.float32(((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3])
    assert np.isnan(U.transform_ref(np.array([[np.nan, 0, 0]], np.float32), T)).all()


def test_pair_sums_restatement_against_plain_numpy():
    rng = np.random.default_rng(3)
    src, dst = rng.normal(0, 1, (300, 3)).astype(np.float32), rng.normal(0, 1, (200, 3)).astype(np.float32)
    idx = rng.integers(-1, 200, 300)
    dist = rng.uniform(0, 1, 300).astype(np.float32)
    s, mags = U.pair_sums_ref(src, dst, idx, dist, (0.1, 0.2, 0.3))
    ok = idx >= 0
    p, q = src[ok].astype(np.float64) - [0.1, 0.2, 0.3], dst[idx[ok]].astype(np.float64) - [0.1, 0.2, 0.3]
    assert s["n"] == ok.sum() and s["n_finite"] == 300
    assert np.allclose(s["sqp"], q.T @ p, rtol=1e-12, atol=1e-12) and np.allclose(s["sp"], p.sum(0), atol=1e-12) and np.allclose(s["sq"], q.sum(0), atol=1e-12)
    assert abs(s["spp"] - (p * p).sum()) < 1e-10 and abs(s["sqq"] - (q * q).sum()) < 1e-10 and abs(s["sdd"] - (dist[ok].astype(np.float64) ** 2).sum()) < 1e-10
    assert (mags["sqp"] >= np.abs(s["sqp"])).all()


def test_exact_fixture_meets_its_bound_under_the_restated_loop():
    """The fixture of the exact ICP case: every first correspondence is the true one, and five iterations of the restated loop land within
    four fp32 roundings of a transformed coordinate."""
    src, dst, T_true, s = U.exact_case()
    assert np.linalg.norm(src.astype(np.float64) - dst.astype(np.float64), axis=1).max() <= 0.45 * s
    T, fitness, rmse, it, converged = U.icp_ref(src, dst, s, max_iter=5, fitness_tol=0.0, rmse_tol=0.0)
    assert fitness == 1.0 and it == 5 and not converged
    err = np.abs(U.apply64(T, src) - U.apply64(T_true, src)).max()
    print("exact case: spacing %.4f, max |T x - T_true x| = %.3e, bound %.3e" % (s, err, 2.0 ** -22 * np.abs(dst).max()))
    assert err <= 2.0 ** -22 * np.abs(dst).max()


def test_general_fixture_converges_and_the_fp32_argmin_is_measured():
    """The restated loop on the noisy fixture converges near the truth; the same loop with fp64 distances differs from it by the amount the
    GPU test allows four times over (printed; DESIGN 8 f6 records it)."""
    src, dst, T_true, init, threshold = U.general_case()
    a = U.icp_ref(src, dst, threshold, init=init, max_iter=40)
    b = U.icp_ref(src, dst, threshold, init=init, max_iter=40, fp32=False)
    print("general case: iterations %d / %d, fitness %.4f, |T32 - T64| = %.3e, |T32 - T_true| = %.3e" % (
        a[3], b[3], a[1], np.linalg.norm(a[0] - b[0]), np.linalg.norm(a[0] - T_true)))
    assert a[4] and a[3] < 40 and 0.75 < a[1] < 0.85                          # converged; the outliers found no partner
    # the target is sampled at spacing 1 and the source lies between its points: a tenth of that spacing is "the known transform" here
    assert np.abs(U.apply64(a[0], src) - U.apply64(T_true, src)).max() < 0.1


def test_format_readers(tmp_path):
    from mvsformer_amd import data_io
    T = U.similarity(10.0, (0, 0, 1), 2.0, (1, 2, 3))
    good = tmp_path / "Barn_trans.txt"
    good.write_text("\n".join(" ".join("%.17e" % v for v in row) for row in T) + "\n")
    assert np.array_equal(data_io.read_alignment(str(good)), T)
    for name, text in (("3x4.txt", "\n".join(" ".join("%.17e" % v for v in row) for row in T[:3])), ("row.txt", "1 0 0 0 0 1 0 0 0 0 1 0 0 0 1 1"),
                       ("word.txt", "1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 one")):
        bad = tmp_path / name
        bad.write_text(text)
        with pytest.raises(ValueError):
            data_io.read_alignment(str(bad))
    doc = {"class_name": "SelectionPolygonVolume", "version_major": 1, "version_minor": 0, "orthogonal_axis": "Y", "axis_min": -1.5, "axis_max": 4.25,
           "bounding_polygon": [[0.0, 9.0, 0.0], [4.0, 9.0, 0.0], [0.0, 9.0, 4.0]]}
    path = tmp_path / "Barn.json"
    path.write_text(json.dumps(doc))
    got = data_io.read_crop_volume(str(path))
    assert got["orthogonal_axis"] == "Y" and got["axis_min"] == -1.5 and got["axis_max"] == 4.25
    assert got["bounding_polygon"].shape == (3, 3) and got["bounding_polygon"].dtype == np.float64
    for change in ({"class_name": "PointCloud"}, {"axis_min": None}, {"bounding_polygon": None}, {"orthogonal_axis": "W"}):
        d = {k: v for k, v in dict(doc, **change).items() if v is not None}
        path.write_text(json.dumps(d))
        with pytest.raises(ValueError):
            data_io.read_crop_volume(str(path))


def test_header_table_and_library_carry_the_entries():
    from mvsformer_amd import _lib, ops
    src = open(os.path.join(REPO, "include", "mvs_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, code) and n in _lib.SIGNATURES, n
    for name, value in (("MVS_ALIGN_CROP_MAX_K", ops.ALIGN_CROP_MAX_K), ("MVS_ALIGN_PAIR_RECORD_BYTES", ops.ALIGN_PAIR_RECORD_BYTES),
                        ("MVS_ALIGN_PAIR_MAX_ROWS", ops.ALIGN_PAIR_MAX_ROWS)):
        assert int(re.search(r"#define %s (\d+)" % name, code).group(1)) == value
    assert ops.ALIGN_CROP_MAX_K == U.MAX_K and _lib.ABI_VERSION == 51
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    row = 8 * 20
    assert lib.mvs_align_pair_sums_workspace_bytes(0) == row and lib.mvs_align_pair_sums_workspace_bytes(256) == row
    assert lib.mvs_align_pair_sums_workspace_bytes(257) == 2 * row and lib.mvs_align_pair_sums_workspace_bytes(1 << 30) == 1024 * row
    assert lib.mvs_align_pair_sums_workspace_bytes(-1) == -1
    # argument checks come before any launch: they can be exercised without a GPU
    import ctypes
    fake, EINVAL = ctypes.c_void_p(8), lib.mvs_align_transform(None, 1, None, None, None)
    assert EINVAL != 0 and b"mvs_align_transform" in lib.mvs_last_error()
    poly = (ctypes.c_double * (2 * 65))(*([0.0, 0.0, 1.0, 0.0, 0.0, 1.0] * 21 + [0.0] * 4))
    assert lib.mvs_align_crop_polygon(fake, 4, 2, 0.0, 1.0, ctypes.addressof(poly), 65, fake, None) == EINVAL and b"65" in lib.mvs_last_error()
    assert lib.mvs_align_crop_polygon(fake, 4, 3, 0.0, 1.0, ctypes.addressof(poly), 3, fake, None) == EINVAL and b"axis" in lib.mvs_last_error()
    assert lib.mvs_align_crop_polygon(fake, 4, 0, 0.0, 1.0, ctypes.addressof(poly), 2, fake, None) == EINVAL
    import mvsformer_amd
    from mvsformer_amd import cloud_eval
    assert mvsformer_amd.icp is cloud_eval.icp and mvsformer_amd.evaluate_tt is cloud_eval.evaluate_tt
