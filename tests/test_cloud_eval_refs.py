"""CPU checks of the point-cloud evaluation: the numpy yardstick (tests/cloud_eval_util.py) on hand-computed cases and against scipy's
KD-tree, the premises the GPU tests rest on (no distance within 8 ulp of a bound, targets well separated), and that the built library and
the package carry the feature."""
import math
import os
import re

import numpy as np
import pytest

import cloud_eval_util as U
from conftest import REPO

EINVAL = -22                                                                   # MVS_EINVAL
NEW_SYMBOLS = ("mvs_cloud_bounds", "mvs_cloud_grid_keys", "mvs_cloud_grid_workspace_bytes", "mvs_cloud_grid_build", "mvs_cloud_query_keys",
               "mvs_cloud_nn_query", "mvs_cloud_voxel_downsample_count", "mvs_cloud_voxel_downsample_write", "mvs_cloud_score_workspace_bytes",
               "mvs_cloud_score")


def test_brute_force_on_hand_computed_points():
    dst = [[0, 0, 0], [1, 0, 0], [0, 2, 0], [0, 0, -3], [10, 10, 10]]
    src = [[0.25, 0, 0], [0.75, 0, 0], [0, 1.5, 0], [0, 0, -2.5], [4, 4, 4]]
    d, i, raw = U.brute_nn(src, dst, 5.0)
    assert i.tolist() == [0, 1, 2, 3, -1]
    assert d.tolist() == [0.25, 0.25, 0.5, 0.5, 5.0]
    assert raw[4] == 6.0                                                      # (4,4,4) -> (0,2,0): sqrt(16 + 4 + 16), beyond the cap


def test_brute_force_cap_is_strict_and_ties_take_the_lowest_index():
    d, i, raw = U.brute_nn([[0, 0, 0]], [[3, 4, 0]], 5.0)                    # exactly at max_dist: capped
    assert raw[0] == 5.0 and d[0] == 5.0 and i[0] == -1
    d, i, _ = U.brute_nn([[0, 0, 0]], [[3, 4, 0]], 5.000001)
    assert d[0] == 5.0 and i[0] == 0
    d, i, _ = U.brute_nn([[0, 0, 0]], [[9, 9, 9], [0, 1, 0], [1, 0, 0], [0, 0, -1]], 2.0)
    assert d[0] == 1.0 and i[0] == 1
    d, i, _ = U.brute_nn([[0, 0, 0], [np.nan, 0, 0]], [[np.inf, 0, 0], [0, 0.5, 0]], 2.0)      # non-finite target skipped, query capped
    assert i.tolist() == [1, -1] and d.tolist() == [0.5, 2.0]
    d, i, _ = U.brute_nn(np.zeros((2, 3)), np.zeros((0, 3)), 2.0)
    assert i.tolist() == [-1, -1] and d.tolist() == [2.0, 2.0]


def test_cell_rule_and_two_voxel_centroid():
    assert U.cell_index([[-1.0, -0.5, 0.0], [0.49, 0.5, 1.0]], [-1.0, -0.5, 0.0], 0.5).tolist() == [[0, 0, 0], [2, 2, 2]]
    pts = [[0.0, 0.0, 0.0], [0.25, 0.25, 0.0], [1.5, 0.0, 0.0], [0.25, 0.0, 0.25], [1.25, 0.5, 0.75]]
    keys, (cen, col) = U.voxel_centroids(pts, 1.0, [np.asarray(pts) * 2.0])
    assert keys.tolist() == [0, 1]
    assert np.allclose(cen, [[0.5 / 3, 0.25 / 3, 0.25 / 3], [1.375, 0.25, 0.375]], rtol=0, atol=1e-15)
    assert np.allclose(col, 2.0 * cen, rtol=0, atol=1e-15)
    keys, (cen,) = U.voxel_centroids([[np.nan, 0, 0], [2.0, 2.0, 2.0]], 1.0)
    assert keys.tolist() == [0] and cen.tolist() == [[2.0, 2.0, 2.0]]


def test_evaluate_ref_on_hand_computed_clouds():
    pred, gt = [[0, 0, 0], [0, 0, 1], [50, 0, 0]], [[0, 0, 0.5], [0, 0, 3]]
    r = U.evaluate_ref(pred, gt, 4.0, taus=(1.0, 4.0))
    assert (r["n_pred"], r["n_gt"], r["pred_below_max"], r["gt_below_max"]) == (3, 2, 2, 2)
    assert r["accuracy"] == 0.5 and r["completeness"] == 1.25 and r["overall"] == 0.875
    assert r["pred_below_tau"] == [2, 2] and r["gt_below_tau"] == [1, 2]
    assert r["precision"] == [2 / 3, 2 / 3] and r["recall"] == [0.5, 1.0]
    assert r["fscore"][0] == pytest.approx(2 * (2 / 3) * 0.5 / (2 / 3 + 0.5))
    e = U.evaluate_ref(pred, gt, 4.0, taus=(1.0,), pred_mask=[False] * 3)
    assert e["n_pred"] == 0 and math.isnan(e["accuracy"]) and math.isnan(e["completeness"]) and math.isnan(e["precision"][0])
    assert e["recall"] == [0.0] and math.isnan(e["fscore"][0])


def test_brute_force_agrees_with_scipy():
    sp = pytest.importorskip("scipy.spatial")
    for name, case in U.geometry_cases().items():
        ok = np.isfinite(case["dst"]).all(axis=1)
        d, i, raw = U.reference("geometry", name)[1]
        qd, qi = sp.cKDTree(case["dst"][ok].astype(np.float64)).query(np.nan_to_num(case["src"].astype(np.float64), nan=1e9, posinf=1e9, neginf=-1e9))
        assert np.allclose(raw[np.isfinite(raw)], qd[np.isfinite(raw)], rtol=1e-12, atol=0), name
        hit = i >= 0
        assert np.allclose(np.linalg.norm(case["src"][hit].astype(np.float64) - case["dst"][i[hit]], axis=1), d[hit], rtol=1e-12, atol=0), name


@pytest.mark.parametrize("name", sorted(U.geometry_cases()))
def test_geometry_cases_keep_the_premises_of_the_gpu_test(name):
    """Coordinates within +-2^10, distinct targets more than 1e-3 apart, and no nearest distance within 8 fp32 ulp of max_dist - apart from
    the one deliberate entry at exactly max_dist."""
    case, (d, i, raw) = U.reference("geometry", name)
    for a in (case["src"], case["dst"]):
        assert np.abs(a[np.isfinite(a)]).max() <= 1024.0
    assert U.min_separation(case["dst"]) > 1e-3
    keep = np.ones(len(raw), bool)
    if "deliberate" in case:
        assert raw[case["deliberate"]] == float(np.float32(case["max_dist"]))
        keep[case["deliberate"]] = False
    assert U.clear_of(raw[keep], case["max_dist"])
    assert case["max_dist"] / (case["cell"] or case["max_dist"]) <= 16
    if "exact" in case:
        assert i[case["exact"][0]] == case["exact"][1]
    if name == "outliers":
        assert (raw[300:] > case["max_dist"]).all() and (i[300:] == -1).all()
    if name == "far_queries":
        assert (i[:200] == -1).all() and (i[200:] >= 0).any()
    if name == "one_cell":
        org = case["dst"].min(axis=0)
        assert (U.cell_index(case["dst"], org, case["cell"]) == 0).all()
    if name == "cell_faces":
        for a in (case["src"], case["dst"]):
            assert (a / np.float32(case["cell"]) == np.round(a / np.float32(case["cell"]))).all()


def test_size_cases_keep_the_premises_of_the_gpu_test():
    for n in U.SIZES:
        assert U.min_separation(U.size_case(0, n)["dst"]) > 1e-3
        for m in U.SIZES:
            case, (d, i, raw) = U.reference("size", (m, n))
            assert U.clear_of(raw, case["max_dist"]), (m, n)
    _, (d, i, raw) = U.reference("size", (5000, 5000))
    assert 0.1 < (i >= 0).mean() < 0.9                                       # both outcomes are exercised


def test_eval_clouds_have_no_distance_at_a_threshold():
    for name, (pred, gt, md) in U.eval_clouds().items():
        for voxel in (None, 1.0):
            r = U.evaluate_ref(pred, gt, md, taus=(0.5 * md, md), voxel=voxel)
            assert U.clear_of(r["all_dist"], md) and U.clear_of(r["all_dist"], 0.5 * md), (name, voxel)
            assert 0 < r["pred_below_max"] < r["n_pred"] or name != "cluster"


def test_library_and_package_carry_the_feature():
    """The built library exports every mvs_cloud_* entry the header declares, and the module imports.  Fails without the feature."""
    from mvsformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mvs_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mvs_cloud_\w+)\s*\(", src))
    assert declared == set(NEW_SYMBOLS)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.mvs_cloud_grid_workspace_bytes(256) == 2 * 8 + 4 and lib.mvs_cloud_grid_workspace_bytes(257) == 3 * 8 + 2 * 4
    assert lib.mvs_cloud_grid_workspace_bytes(0) == -1 and lib.mvs_cloud_score_workspace_bytes(0) == 8
    import mvsformer_amd
    from mvsformer_amd import cloud_eval
    assert mvsformer_amd.evaluate_cloud is cloud_eval.evaluate and mvsformer_amd.nn_distance is cloud_eval.nn_distance
    assert mvsformer_amd.voxel_downsample is cloud_eval.voxel_downsample


def test_host_side_refusals_launch_nothing():
    """Bad arguments are refused with MVS_EINVAL by the entry points' host code (no GPU here: a launch would fail differently)."""
    import ctypes
    from mvsformer_amd import _lib
    lib = _lib.load()
    fake = 0x1000                                                            # never dereferenced on the host
    b = (ctypes.c_float * 6)(0, 0, 0, 1, 1, 1)
    for cell in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.mvs_cloud_grid_keys(fake, 10, cell, ctypes.addressof(b), 0, fake, fake, None) == EINVAL and b"mvs_cloud_grid_keys" in lib.mvs_last_error()
    wide = (ctypes.c_float * 6)(0, 0, 0, 1, 2097152.0, 1)                   # 2^21 cells of 1 along y: at the limit
    assert lib.mvs_cloud_grid_keys(fake, 10, 1.0, ctypes.addressof(wide), 0, fake, fake, None) == EINVAL and b"2^21" in lib.mvs_last_error()
    t = (ctypes.c_float * 2)(1.0, 2.5)
    assert lib.mvs_cloud_score(fake, 10, 2.0, ctypes.addressof(t), 2, fake, fake, None) == EINVAL and b"exceeds max_dist" in lib.mvs_last_error()
    assert lib.mvs_cloud_score(fake, 10, 2.0, ctypes.addressof(t), 9, fake, fake, None) == EINVAL
    for md, cell in ((float("nan"), 1.0), (float("inf"), 1.0), (2.0, 0.0), (100.0, 1.0)):
        assert lib.mvs_cloud_nn_query(fake, 4, None, fake, cell, fake, fake, fake, fake, 4, md, fake, fake, None) == EINVAL
    assert lib.mvs_cloud_bounds(fake, 0, fake, fake, fake, None) == EINVAL
    from mvsformer_amd import cloud_eval
    from mvsformer_amd._lib import MvsHipError
    import torch
    with pytest.raises(MvsHipError):
        cloud_eval.nn_distance(torch.zeros(4, 3), torch.zeros(4, 3), 1.0)    # CPU tensors: no fallback
    assert cloud_eval.default_cell([0, 0, 0, 10, 10, 10], 1000, 4.0) == pytest.approx(1.0, rel=1e-5)
    assert cloud_eval.default_cell([0, 0, 0, 10, 10, 10], 10 ** 6, 4.0) == pytest.approx(0.25, rel=1e-5)       # max_dist / 16
    assert cloud_eval.default_cell([0, 0, 0, 10, 10, 0], 100, 4.0) == pytest.approx(1.0, rel=1e-5)            # flat: area / N
    assert cloud_eval.default_cell([1, 1, 1, 1, 1, 1], 1, 4.0) == pytest.approx(4.0, rel=1e-5)
