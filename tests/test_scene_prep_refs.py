"""The yardsticks of tests/test_hip_scene_prep.py (tests/scene_prep_util.py) against a case computed by hand, the host-side parts of the
feature (``write_pair_file``, the COLMAP text reader and writer) and its plumbing (header, ctypes table, source rules).  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_prep_util as U  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("mvs_scene_visibility", "mvs_scene_pair_scores", "mvs_scene_rank_sources", "mvs_scene_depth_ranges")


def test_restatements_agree_with_the_hand_computed_case():
    h = U.hand_case()
    seen, bad = U.visibility_ref(h["xyz"], h["obs_point"], h["obs_view"], 3)
    assert bad == 0 and seen.tolist() == [[True, True, True, False], [True, True, False, False], [True, False, True, False]]
    assert U.pack_bits(seen).tolist() == [[7], [3], [5]]
    C = U.centers_ref(h["R"], h["t"])
    assert np.array_equal(C, [[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    S = U.pair_scores_ref(seen, h["xyz"], h["R"], h["t"])
    assert np.abs(S - h["S"]).max() <= 1e-9 and np.array_equal(S, S.T) and not S.diagonal().any()
    P = h["xyz"].astype(np.float64)
    g, theta = U.term_ref(C[0], C[1], P[0])
    assert abs(theta - 45.0) <= 1e-12 and abs(g - np.exp(-8.0)) <= 1e-15
    assert abs(U.term_ref(C[1], C[2], P[0])[1] - 60.0) <= 1e-12
    # theta EXACTLY theta0 belongs to the sigma1 branch (theta <= theta0) and gives exp(0) = 1 whatever sigma1 is; the two sides of it
    # are told apart with a tiny sigma1: 1e-3 degrees below theta0 the term vanishes, 1e-3 above it is sigma2's
    _, theta = U.term_ref(C[0], C[1], P[1])
    assert abs(theta - 5.0) <= 1e-5
    assert U.term_ref(C[0], C[1], P[1], theta0=theta, sigma1=1e-9, sigma2=10.0)[0] == 1.0
    assert U.term_ref(C[0], C[1], P[1], theta0=theta + 1e-3, sigma1=1e-9, sigma2=10.0)[0] == 0.0
    assert abs(U.term_ref(C[0], C[1], P[1], theta0=theta - 1e-3, sigma1=1e-9, sigma2=10.0)[0] - np.exp(-1e-6 / 200.0)) <= 1e-12
    # a point ON a camera centre: theta = 0, a term, not a NaN
    g, theta = U.term_ref(C[0], C[2], P[2])
    assert theta == 0.0 and g == np.exp(-12.5)
    src, score = U.rank_ref(S, 2)
    assert np.array_equal(src, h["src"]) and np.array_equal(score[0], [S[0, 1], S[0, 2]])
    src, score = U.rank_ref(S, 4)                                  # k > V - 1
    assert np.array_equal(src[:, :2], h["src"]) and (src[:, 2:] == -1).all() and not score[:, 2:].any()
    rng, n = U.depth_ranges_ref(seen, h["xyz"], h["R"], h["t"])
    assert np.array_equal(rng, h["range"]) and np.array_equal(n, h["n"])


def test_rank_restatement_is_stable_on_ties():
    S = np.array([[0, 2, 1, 2, 0], [2, 0, 0, 0, 0], [1, 0, 0, 0, 0], [2, 0, 0, 0, 0], [0, 0, 0, 0, 0]], np.float64)
    src, score = U.rank_ref(S, 4)
    assert src[0].tolist() == [1, 3, 2, 4] and score[0].tolist() == [2, 2, 1, 0]
    assert src[4].tolist() == [0, 1, 2, 3] and src[1].tolist() == [0, 2, 3, 4]
    assert U.rank_gaps_ok(S, 4, tied=[(1, 3)]) and not U.rank_gaps_ok(S, 4)
    S2 = S.copy()
    S2[0, 3] = S2[3, 0] = 2 - 1e-9
    assert not U.rank_gaps_ok(S2, 4, tied=[(1, 3)])                # a near tie is refused


def test_depth_restatement_orders_negative_and_repeated_values():
    xyz = np.array([[0, 0, -2], [0, 0, 3], [0, 0, -2], [0, 0, 0.5], [0, 0, -7]], np.float32)
    R, t = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32)
    seen = np.ones((1, 5), bool)
    assert U.depths_ref(seen[0], xyz, R[0], t[0]).tolist() == [-2, 3, -2, 0.5, -7]
    for lo, hi, want in ((0.0, 1.0, (-7, 3)), (0.2, 0.8, (-2, 3)), (0.4, 0.79, (-2, 0.5))):
        assert U.depth_ranges_ref(seen, xyz, R, t, lo, hi)[0].tolist() == [list(want)]


def test_pair_file_round_trip(tmp_path):
    from mvsformer_amd import data_io
    pairs = [(0, [3, 1, 2]), (1, [0]), (2, [1, 3]), (3, [2, 0, 1])]
    scores = [[10.5, 2.25, 1e-3], [7.0], [3.0, 0.1], [9.0, 8.0, 1.0 / 3.0]]
    path = str(tmp_path / "pair.txt")
    assert data_io.write_pair_file(path, pairs, scores) == path
    assert data_io.read_pair_file(path) == pairs
    assert data_io.read_pair_file(data_io.write_pair_file(path, pairs)) == pairs
    lines = open(data_io.write_pair_file(path, pairs, scores)).read().split("\n")
    assert lines[0] == "4" and lines[1] == "0" and lines[2].split()[:3] == ["3", "3", "10.5"]
    assert [float(x) for x in lines[8].split()[2::2]] == scores[3]          # scores read back exactly
    # a view without sources is written, and dropped by the reader as the reference's reader drops it
    assert data_io.read_pair_file(data_io.write_pair_file(path, pairs + [(4, [])])) == pairs
    with pytest.raises(ValueError):
        data_io.write_pair_file(path, pairs, [[1.0]] * 4)


def _model(seed=3, V=5, N=40):
    s = U.ring_scene(V, N, seed, track=2.5)
    s["xyz"][7] = [np.nan, 1.0, np.inf]
    K = np.array([[[500.0 + v, 0, 320.5], [0, 505.25 + v, 240.0], [0, 0, 1]] for v in range(V)], np.float32)
    size = np.array([[640 + v, 480] for v in range(V)])
    return s, K, size


def test_colmap_text_round_trip(tmp_path):
    from mvsformer_amd import data_io
    s, K, size = _model()
    names = ["img %d.png" % v for v in range(5)]
    data_io.write_colmap_text(str(tmp_path), s["xyz"], s["obs_point"], s["obs_view"], s["R"], s["t"], K, size, names)
    got = data_io.read_colmap_text(str(tmp_path))
    assert got["xyz"].dtype == np.float32 and np.array_equal(got["xyz"], s["xyz"], equal_nan=True)
    assert np.array_equal(got["t"], s["t"]) and np.array_equal(got["K"], K) and np.array_equal(got["size"], size)
    assert np.abs(got["R"].astype(np.float64) - s["R"]).max() <= 4 * 2.0 ** -24          # through a quaternion: a few float32 ulp
    assert got["names"] == names and got["image_ids"].tolist() == [1, 2, 3, 4, 5] and got["point_ids"].tolist() == list(range(1, 41))
    assert got["obs_point"].dtype == np.int64 and got["obs_view"].dtype == np.int32
    # the observations come back grouped by point; as a set of (point, view) with multiplicity they are the input's
    key = lambda p, v: sorted(zip(np.asarray(p).tolist(), np.asarray(v).tolist()))  # noqa: E731
    assert key(got["obs_point"], got["obs_view"]) == key(s["obs_point"], s["obs_view"])
    # views are indexed in ascending IMAGE_ID whatever the order of the lines
    path = os.path.join(str(tmp_path), "images.txt")
    lines = open(path).read().split("\n")
    head = [ln for ln in lines if ln.startswith("#")]
    body = [ln for ln in lines if not ln.startswith("#")][:10]
    open(path, "w").write("\n".join(head + body[8:10] + body[0:8]) + "\n")
    again = data_io.read_colmap_text(str(tmp_path))
    assert again["names"] == names and np.array_equal(again["t"], s["t"]) and np.array_equal(again["obs_view"], got["obs_view"])
    data_io.write_colmap_text(str(tmp_path / "simple"), s["xyz"], s["obs_point"], s["obs_view"], s["R"], s["t"], K, size, model="SIMPLE_PINHOLE")
    simple = data_io.read_colmap_text(str(tmp_path / "simple"))
    assert np.array_equal(simple["K"][:, 0, 0], K[:, 0, 0]) and np.array_equal(simple["K"][:, 1, 1], K[:, 0, 0])
    assert np.array_equal(simple["K"][:, :2, 2], K[:, :2, 2])


@pytest.mark.parametrize("model", ["SIMPLE_RADIAL", "OPENCV", "RADIAL"])
def test_colmap_reader_refuses_a_model_with_distortion(tmp_path, model):
    from mvsformer_amd import data_io
    s, K, size = _model()
    data_io.write_colmap_text(str(tmp_path), s["xyz"], s["obs_point"], s["obs_view"], s["R"], s["t"], K, size, model=model)
    with pytest.raises(ValueError, match=model):
        data_io.read_colmap_text(str(tmp_path))


def test_quaternion_helpers_cover_every_branch():
    from mvsformer_amd import data_io
    rng = np.random.default_rng(0)
    mats = [np.eye(3), np.diag([1.0, -1, -1]), np.diag([-1.0, 1, -1]), np.diag([-1.0, -1, 1])]
    for _ in range(20):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        mats.append(q * np.sign(np.linalg.det(q)))
    for R in mats:
        q = data_io._rot_to_quat(R)
        assert abs(np.linalg.norm(q) - 1.0) <= 1e-15 and q[0] >= 0.0
        assert np.abs(data_io._quat_to_rot(q) - R).max() <= 1e-14


def test_synthetic_scenes_meet_the_ranking_condition():
    """The seeds tests/test_hip_scene_prep.py ranks: consecutive scores inside the first k are further apart than 1e-6 of the row maximum
    (the kernels are required to be within 1e-9), except the constructed exact ties."""
    import test_hip_scene_prep as T
    for name, (kw, k, tied) in T.RANK_SCENES.items():
        s = T._scene(**kw)                                         # pure numpy: the scene and its restated scores
        assert U.rank_gaps_ok(s["S"], k, tied), name
        counts = s["seen"].sum(0)
        assert (counts == 0).any() and (counts == 1).any(), name          # points seen by no view and by one view


def test_header_library_and_source_rules_know_the_entries():
    from mvsformer_amd import _lib, _sources
    src = open(os.path.join(REPO, "include", "mvs_scene_prep.h")).read()
    from ctypes import c_double as Dbl, c_int as I, c_int64 as L, c_void_p as P
    assert set(_lib.SCENE_SIGNATURES) == set(ENTRIES) and not set(ENTRIES) & set(_lib.SIGNATURES)      # a table of their own
    assert _lib.SCENE_SIGNATURES["mvs_scene_rank_sources"] == (I, [P, I, I, P, P, P])
    assert _lib.SCENE_SIGNATURES["mvs_scene_pair_scores"] == (I, [P, P, L, P, P, I, Dbl, Dbl, Dbl, P, P, P])
    assert _lib.SCENE_DEFINES == {"MVS_SCENE_MAX_VIEWS": 8192}
    lib = _lib.load()
    for e in ENTRIES:
        assert re.search(r"\b%s\s*\(" % e, src) and hasattr(lib, e) and getattr(lib, e).argtypes == _lib.SCENE_SIGNATURES[e][1]
        assert _sources.files_of(e)[0] == "scene_prep.hip" and _sources.SCENE_PUB in _sources.files_of(e)
    assert lib.mvs_scene_rank_sources(None, 1, 1, None, None, None) == -22 and b"mvs_scene_rank_sources" in lib.mvs_last_error()
    assert _sources.SCENE_PUB in _sources.file_digests()
    assert _sources.files_of("scene_pair_scores_kernel")[0] == "scene_prep.hip"
    assert _sources.files_of("mvs_prep_accept")[0] == "sample_prep.hip" and _sources.files_of("prep_jitter_tail")[0] == "sample_prep.hip"
    text = " ".join(src.split())
    assert "RESTATED" in text and "parity with the original script is UNVERIFIED" in text
    assert "scene_prep.hip" in open(os.path.join(REPO, "mvsformer_amd", "csrc", "Makefile")).read()
    import mvsformer_amd as m
    assert m.prepare_scene is m.scene_prep.prepare_scene
