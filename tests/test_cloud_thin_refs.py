"""CPU checks of the greedy thinning: the numpy yardstick (tests/cloud_thin_util.py) against an independently written pass over
scikit-learn's radius search and against the two invariants of a valid result, the premise the GPU test rests on (no pair distance within
8 fp32 ulp of the radius, on every case), and that the built library and the package carry the feature."""
import os
import re

import numpy as np
import pytest

import cloud_eval_util as U
import cloud_thin_util as T
from conftest import REPO

EINVAL = -22                                                                   # MVS_EINVAL
NEW_SYMBOLS = ("mvs_greedy_thin_workspace_bytes", "mvs_greedy_thin")
CASES = sorted(T.cases())


def _radius_pass(xyz, dist, order):
    """The rule once more, written from its other end: neighbour lists first (scikit-learn's ball query over the finite points, inclusive
    radius), then the loop over ranks marking what each kept point removes."""
    nb = pytest.importorskip("sklearn.neighbors")
    p = U.f32(xyz)
    finite = np.nonzero(np.isfinite(p).all(axis=1))[0]
    state = np.zeros(len(p), np.int8)                                        # 0 unseen, 1 kept, -1 removed
    if finite.size:
        pts = p[finite].astype(np.float64)
        lists = nb.NearestNeighbors(radius=float(np.float32(dist)), algorithm="kd_tree").fit(pts).radius_neighbors(pts, return_distance=False)
        where = {int(i): k for k, i in enumerate(finite)}
        for i in (int(o) for o in order):
            if i in where and state[i] == 0:
                state[i] = 1
                for j in finite[lists[where[i]]]:
                    if j != i:
                        assert state[j] != 1                                 # a kept point within reach would have removed i
                        state[j] = -1
    return state == 1


@pytest.mark.parametrize("name", CASES)
def test_yardstick_equals_the_radius_search_pass(name):
    case, keep = T.reference(name)
    assert np.array_equal(keep, _radius_pass(case["xyz"], case["dist"], case["order"]))


@pytest.mark.parametrize("name", CASES)
def test_yardstick_output_keeps_the_invariants(name):
    case, keep = T.reference(name)
    assert T.invariants(case["xyz"], case["dist"], case["order"], keep)
    assert keep.dtype == bool and keep.shape == (len(case["xyz"]),)


def test_invariants_reject_wrong_sets():
    case, keep = T.reference("size_257")
    for flip in (np.nonzero(keep)[0][0], np.nonzero(~keep)[0][0]):           # one point too few, one too many
        bad = keep.copy()
        bad[flip] = ~bad[flip]
        assert not T.invariants(case["xyz"], case["dist"], case["order"], bad)
    other = T.reference("other_seed")[1]
    assert not np.array_equal(keep, other) and not T.invariants(case["xyz"], case["dist"], case["order"], other)     # valid under ITS order only


def test_yardstick_on_hand_computed_points():
    xyz = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [np.nan, 0, 0], [3, 4, 0]]
    assert T.greedy_ref(xyz, 1.0, [0, 1, 2, 3, 4, 5]).tolist() == [True, False, True, False, False, True]      # the bound is inclusive
    assert T.greedy_ref(xyz, 1.0, [1, 0, 2, 3, 4, 5]).tolist() == [False, True, False, True, False, True]
    assert T.greedy_ref(xyz, 0.999, [0, 1, 2, 3, 4, 5]).tolist() == [True, True, True, True, False, True]
    assert T.greedy_ref(xyz, 5.0, [4, 5, 0, 1, 2, 3]).tolist() == [False, False, False, False, False, True]     # (3,4,0) is exactly 5 from the origin
    assert T.greedy_ref(np.zeros((0, 3)), 1.0, []).tolist() == []


@pytest.mark.parametrize("name", CASES)
def test_no_pair_distance_is_within_8_ulp_of_the_radius(name):
    """The premise of the GPU test's exact equality, for every case it uses - none exempted."""
    case = T.cases()[name]
    assert T.clear_of_radius(case["xyz"], case["dist"])
    assert np.abs(case["xyz"][np.isfinite(case["xyz"])]).max(initial=0.0) <= 1024.0
    assert sorted(case["order"].tolist()) == list(range(len(case["xyz"])))


def test_cases_are_what_their_names_say():
    c, keep = T.reference("size_5000")
    nb = np.concatenate([(d <= c["dist"]).sum(axis=1) - 1 for _, d in T.pair_distances(c["xyz"])])
    assert 3.0 < nb.mean() < 6.0                                             # about 5 neighbours (fewer at the patch's rim)
    for n in T.LINE_SIZES:
        assert T.reference("line_%d_sorted" % n)[1].tolist() == [i % 2 == 0 for i in range(n)]       # every other point
    c, keep = T.reference("duplicates")
    rank = np.argsort(c["order"])
    for b in range(300):
        rows = np.nonzero(c["src"] == b)[0]
        assert len(rows) == 3 and keep[rows].sum() == 1 and keep[rows[rank[rows].argmin()]]          # the copy of lowest rank
    c, keep = T.reference("faces")
    origin, cell = T.thin_cell(c["xyz"], c["dist"])
    rank = np.argsort(c["order"])
    axes = {"face": 1, "edge": 2, "corner": 3}
    for kind, under, a, b in c["pairs"]:
        ca, cb = U.cell_index(c["xyz"][[a, b]], origin, cell)
        assert (np.abs(ca - cb) == 1).sum() == axes[kind] and np.abs(ca - cb).max() == 1            # straddles that many faces
        sep = np.linalg.norm(c["xyz"][a].astype(np.float64) - c["xyz"][b].astype(np.float64))
        assert (sep < c["dist"]) == under and abs(sep - c["dist"]) > 1e-5
        first, second = (a, b) if rank[a] < rank[b] else (b, a)
        assert keep[first] and keep[second] == (not under)
    c, keep = T.reference("non_finite")
    assert (~np.isfinite(c["xyz"]).all(axis=1)).sum() >= 16 and not keep[~np.isfinite(c["xyz"]).all(axis=1)].any()
    c, keep = T.reference("eval")
    assert not keep[~c["mask"]].any() and 0.3 * c["mask"].sum() < keep.sum() < 0.9 * c["mask"].sum()
    want = U.evaluate_ref(c["pred"][keep], c["gt"], c["max_dist"], c["taus"])
    for t in c["taus"]:
        assert U.clear_of(want["all_dist"], t)                               # the scores' own premise, after thinning


def test_library_and_package_carry_the_feature():
    """The header declares the thinning entry points, the built library exports them, the versions agree and the package exports the
    function.  Fails without the feature."""
    from mvsformer_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mvs_hip.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(mvs_greedy_thin\w*)\s*\(", src)) == set(NEW_SYMBOLS)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.mvs_version() == _lib.ABI_VERSION
    for n in NEW_SYMBOLS:
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert lib.mvs_greedy_thin_workspace_bytes(0) == -1
    assert lib.mvs_greedy_thin_workspace_bytes(1) == 128 + 32 + 8 and lib.mvs_greedy_thin_workspace_bytes(256) == 128 + 36 * 256
    import mvsformer_amd
    from mvsformer_amd import cloud_eval, ops
    assert mvsformer_amd.greedy_thin is cloud_eval.greedy_thin and "greedy_thin" in mvsformer_amd.__all__
    assert ops.GREEDY_THIN_BATCH == int(re.search(r"#define\s+MVS_GREEDY_THIN_BATCH\s+(\d+)", src).group(1))


def test_host_side_refusals_launch_nothing():
    """Bad arguments are refused with MVS_EINVAL by the entry point's host code, before any launch (there is no GPU here)."""
    import ctypes
    import torch
    from mvsformer_amd import _lib, cloud_eval
    from mvsformer_amd._lib import MvsHipError
    lib = _lib.load()
    fake = 0x1000                                                            # never dereferenced on the host
    rounds = ctypes.c_int64(0)
    args = lambda n, dist: (n, fake, fake, dist, fake, fake, fake, fake, fake, fake, ctypes.addressof(rounds), None)      # noqa: E731
    for dist in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.mvs_greedy_thin(*args(10, dist)) == EINVAL and b"mvs_greedy_thin" in lib.mvs_last_error()
    assert lib.mvs_greedy_thin(*args(0, 1.0)) == EINVAL
    assert lib.mvs_greedy_thin(10, None, fake, 1.0, fake, fake, fake, fake, fake, fake, ctypes.addressof(rounds), None) == EINVAL
    with pytest.raises(MvsHipError):
        cloud_eval.greedy_thin(torch.zeros(4, 3), 1.0)                       # a CPU tensor: no fallback
    # the cell rule: never below dist, and wide enough for what fp32 cell coordinates can be off by (include/mvs_hip.h)
    for ext, dist in ((0.0, 0.2), (600.0, 0.2), (1000.0, 1e-4), (2.0 ** 20, 1.0)):
        cell = cloud_eval.thin_cell([0, 0, 0, ext, 0.5 * ext, 0], dist)
        ncell = ext / cell + 1
        assert cell >= max(dist, ext / 2 ** 20) and ncell < 2 ** 21
        assert 0.99999 * (1.0 - 2.4082e-7 * (ncell + 4)) * cell >= dist
        assert cell == T.thin_cell([[0, 0, 0], [ext, 0.5 * ext, 0]], dist)[1]
