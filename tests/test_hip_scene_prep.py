"""The scene-preparation kernels (csrc/scene_prep.hip, mvsformer_amd/scene_prep.py) against the numpy restatements of
tests/scene_prep_util.py.  Bitset, ranking and depth ranges: exactly.  Pair scores: to a relative 1e-9 of the row maximum (fp64 atan2 and
exp are good to a few ulp and the exponent is at most 180^2 / 2, so the true error is orders of magnitude smaller; the bound is in turn
far below any score gap that matters for ranking), symmetric, zero on the diagonal and bit-identical from call to call."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_prep_util as U  # noqa: E402

pytestmark = pytest.mark.gpu

EDGES = (1, 63, 64, 65, 4096, 4097)                 # word edges (64) and lane-stride edges (64 words = 4096 points)
# name -> (ring_scene arguments, k, constructed twin pairs); tests/test_scene_prep_refs.py checks the gap condition on these seeds.
# The cameras sit on a short arc so that every pair scores well above rounding (a view across a full ring scores exp(-36)).
RANK_SCENES = {
    "arc12": (dict(V=12, N=500, seed=21, arc=0.6), 5, ()),
    "twins": (dict(V=9, N=400, seed=22, arc=0.5, twins=((2, 7),)), 8, ((2, 7),)),
    "lonely_k_above_v": (dict(V=6, N=300, seed=23, arc=0.4, lonely=(4,)), 9, ()),
}


def _sp():
    from mvsformer_amd import scene_prep
    return scene_prep


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _u64(bits):
    return bits.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _scene(V, N, seed, **kw):
    """A scene and its restated visibility and scores, computed once and shared (read-only)."""
    kw = {k: v for k, v in kw.items()}
    s = U.ring_scene(V, N, seed, track=min(6.0, 0.6 * V + 0.5), **kw)
    seen, _ = U.visibility_ref(s["xyz"], s["obs_point"], s["obs_view"], V)
    s["seen"] = seen
    s["S"] = U.pair_scores_ref(seen, s["xyz"], s["R"], s["t"])
    return s


# ---------------------------------------------------------------------------------------------------------------- bitset
@pytest.mark.parametrize("n", EDGES)
def test_visibility_bits_are_numpy_s(n):
    V = 3
    rng = np.random.default_rng(n)
    m = 3 * n + 5
    obs_p, obs_v = rng.integers(0, n, m), rng.integers(0, V, m).astype(np.int32)
    obs_p[-5:], obs_v[-5:] = obs_p[:5], obs_v[:5]                        # duplicate observations collapse
    xyz = rng.normal(size=(n, 3)).astype(np.float32)
    bad = sorted({0, n // 2, n - 1}) if n >= 63 else []
    for i, p in enumerate(bad):
        xyz[p, i % 3] = (np.nan, np.inf, -np.inf)[i % 3]
    seen, n_bad = U.visibility_ref(xyz, obs_p, obs_v, V)
    bits, count, nonfinite = _sp().visibility(xyz, obs_p, obs_v, V)
    assert tuple(bits.shape) == (V, (n + 63) // 64) and bits.dtype == torch.int64 and count.dtype == torch.int32
    assert np.array_equal(_u64(bits), U.pack_bits(seen))
    assert count.cpu().tolist() == seen.sum(1).tolist() and nonfinite == n_bad == len(bad)
    if bad:
        assert not seen[:, bad].any() and seen.any()
    again, _, _ = _sp().visibility(_dev(xyz), _dev(obs_p), _dev(obs_v), V)   # device tensors, another atomic order: the same bits
    assert torch.equal(again, bits)


def test_visibility_without_observations_is_empty():
    bits, count, nonfinite = _sp().visibility(np.zeros((70, 3), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int32), 2)
    assert not bits.any() and not count.any() and nonfinite == 0


@pytest.mark.parametrize("p,v", [(-1, 0), (65, 0), (0, -1), (0, 3), (2 ** 40, 1)])
def test_a_bad_observation_is_einval(p, v):
    from mvsformer_amd._lib import MvsHipError
    s = U.ring_scene(3, 65, seed=1, track=2.0)
    obs_p, obs_v = np.append(s["obs_point"], p), np.append(s["obs_view"], v).astype(np.int32)
    with pytest.raises(MvsHipError, match=r"rc=-22.*1 observations"):
        _sp().visibility(s["xyz"], obs_p, obs_v, 3)
    with pytest.raises(MvsHipError, match="1 observations"):
        _sp().prepare_scene(s["xyz"], obs_p, obs_v, s["R"], s["t"], num_views=2)
    bits, _, _ = _sp().visibility(s["xyz"], s["obs_point"], s["obs_view"], 3)          # the library goes on working
    seen, _ = U.visibility_ref(s["xyz"], s["obs_point"], s["obs_view"], 3)
    assert np.array_equal(_u64(bits), U.pack_bits(seen))


# ---------------------------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize("V,N", [(1, 65), (2, 1), (2, 63), (2, 64), (5, 65), (5, 4096), (70, 64), (70, 4097)])
def test_pair_scores_match_the_fp64_restatement(V, N):
    s = _scene(V, N, seed=100 + V + N)
    if N > 1 and V > 1:
        per_point = s["seen"].sum(0)
        assert (per_point == 0).any() and (per_point == 1).any() and (per_point >= 2).any()
    bits, _, _ = _sp().visibility(s["xyz"], s["obs_point"], s["obs_view"], V)
    S = _sp().pair_scores(bits, s["xyz"], s["R"], s["t"])
    assert S.dtype == torch.float64 and tuple(S.shape) == (V, V)
    again = _sp().pair_scores(bits, s["xyz"], s["R"], s["t"])
    got = S.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), again.cpu().numpy().view(np.uint64))          # two runs: the same bits
    assert np.array_equal(got, got.T) and not got.diagonal().any()
    top = s["S"].max(1, keepdims=True)
    err = np.abs(got - s["S"])
    print("V=%d N=%d: max |S - ref| / row max = %.3e" % (V, N, (err / np.maximum(top, 1e-300)).max()))
    assert (err <= 1e-9 * top).all()
    assert np.array_equal(got == 0.0, s["S"] == 0.0)


def test_pair_scores_take_their_constants_as_arguments():
    s = _scene(5, 65, seed=170)
    bits, _, _ = _sp().visibility(s["xyz"], s["obs_point"], s["obs_view"], 5)
    got = _sp().pair_scores(bits, s["xyz"], s["R"], s["t"], theta0=20.0, sigma1=3.0, sigma2=0.5).cpu().numpy()
    want = U.pair_scores_ref(s["seen"], s["xyz"], s["R"], s["t"], 20.0, 3.0, 0.5)
    assert want.max() > 0 and (np.abs(got - want) <= 1e-9 * want.max(1, keepdims=True)).all()
    assert np.abs(want - s["S"]).max() > 1e-3                                        # the constants matter


def test_pair_scores_of_the_hand_case():
    """theta = theta0 up to rounding (the term is 1), a point ON a camera centre (atan2(0, 0) = 0: a term, not a NaN)."""
    h = U.hand_case()
    bits, count, _ = _sp().visibility(h["xyz"], h["obs_point"], h["obs_view"], 3)
    assert _u64(bits).tolist() == [[7], [3], [5]] and count.cpu().tolist() == [3, 2, 2]
    S = _sp().pair_scores(bits, h["xyz"], h["R"], h["t"]).cpu().numpy()
    assert np.isfinite(S).all() and (np.abs(S - h["S"]) <= 1e-9 * h["S"].max(1, keepdims=True)).all()
    src, _ = _sp().rank_sources(_dev(S), 2)
    assert np.array_equal(src.cpu().numpy(), h["src"])
    rng, n = _sp().depth_ranges(bits, count, h["xyz"], h["R"], h["t"])
    assert np.array_equal(rng.cpu().numpy(), h["range"]) and n.cpu().tolist() == h["n"].tolist()


# --------------------------------------------------------------------------------------------------------------- ranking
@pytest.mark.parametrize("name", sorted(RANK_SCENES))
def test_ranking_is_the_stable_sort(name):
    kw, k, tied = RANK_SCENES[name]
    s = _scene(**kw)
    V = kw["V"]
    assert U.rank_gaps_ok(s["S"], k, tied)                                # the condition under which rounding cannot excuse a difference
    want_src, want_score = U.rank_ref(s["S"], k)
    # the kernel on the restated scores: everything exact
    src, score = _sp().rank_sources(s["S"], k)
    assert src.dtype == torch.int32 and tuple(src.shape) == (V, k)
    assert np.array_equal(src.cpu().numpy(), want_src)
    assert np.array_equal(score.cpu().numpy().view(np.uint64), want_score.view(np.uint64))
    # the kernels end to end: the same order, the scores to 1e-9
    bits, _, _ = _sp().visibility(s["xyz"], s["obs_point"], s["obs_view"], V)
    S = _sp().pair_scores(bits, s["xyz"], s["R"], s["t"])
    src, score = _sp().rank_sources(S, k)
    assert np.array_equal(src.cpu().numpy(), want_src)
    assert (np.abs(score.cpu().numpy() - want_score) <= 1e-9 * s["S"].max(1, keepdims=True)).all()
    if tied:                                                              # the twins tie EXACTLY against every third view, on the device too
        (a, b), got = tied[0], S.cpu().numpy()
        others = [m for m in range(V) if m not in (a, b)]
        assert np.array_equal(got[others, a], got[others, b]) and got[others, a].max() > 0
        for m in others:
            row = want_src[m].tolist()
            assert row.index(a) + 1 == row.index(b)                       # the lower index first
    if k > V - 1:
        assert (want_src[:, V - 1:] == -1).all() and (want_src[:, :V - 1] >= 0).all()
    if "lonely" in kw:
        v = kw["lonely"][0]
        assert want_src[v, :V - 1].tolist() == [j for j in range(V) if j != v] and not want_score[v].any()


def test_ranking_of_all_equal_scores_and_one_view():
    src, score = _sp().rank_sources(np.zeros((1, 1)), 3)
    assert src.cpu().tolist() == [[-1, -1, -1]] and score.cpu().tolist() == [[0.0, 0.0, 0.0]]
    S = np.full((300, 300), 2.5)
    np.fill_diagonal(S, 0.0)
    src, score = _sp().rank_sources(S, 299)
    want, _ = U.rank_ref(S, 299)
    assert np.array_equal(src.cpu().numpy(), want) and (score.cpu().numpy() == 2.5).all()


# ---------------------------------------------------------------------------------------------------------- depth ranges
COUNTS = (0, 1, 2, 99, 100, 101, 257)


@functools.lru_cache(maxsize=None)
def _depth_scene():
    """Seven views that observe exactly COUNTS points of 300.  The blob is wider than the ring, so depths are negative for the points
    behind a camera; points 0..39 come in pairs with the same coordinates (repeated depths)."""
    rng = np.random.default_rng(7)
    s = U.ring_scene(len(COUNTS), 300, seed=7, radius=1.5, blob=2.0)
    s["xyz"][20:40] = s["xyz"][0:20]
    obs_p, obs_v = [], []
    for v, c in enumerate(COUNTS):
        pts = np.concatenate([np.arange(min(c, 40)), 40 + rng.choice(260, max(c - 40, 0), replace=False)])
        obs_p += pts.tolist()
        obs_v += [v] * c
    order = rng.permutation(len(obs_p))
    s["obs_point"], s["obs_view"] = np.array(obs_p, np.int64)[order], np.array(obs_v, np.int32)[order]
    s["seen"], _ = U.visibility_ref(s["xyz"], s["obs_point"], s["obs_view"], len(COUNTS))
    return s


def _same_bits32(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("lo,hi", [(0.01, 0.99), (0.0, 0.999), (0.5, 0.5), (0.0, 1.0), (0.25, 0.26)])
def test_depth_ranges_are_the_float32_restatement_bit_for_bit(lo, hi):
    s = _depth_scene()
    V = len(COUNTS)
    assert s["seen"].sum(1).tolist() == list(COUNTS)
    z = [U.depths_ref(s["seen"][v], s["xyz"], s["R"][v], s["t"][v]) for v in range(V)]
    assert all((zv < 0).any() and (zv > 0).any() for zv in z[3:]) and all(len(np.unique(zv)) < len(zv) for zv in z[3:])
    if hi == 0.999:
        assert all(int(c * hi) == c - 1 for c in COUNTS[1:])
    bits, count, _ = _sp().visibility(s["xyz"], s["obs_point"], s["obs_view"], V)
    assert count.cpu().tolist() == list(COUNTS)
    rng, n = _sp().depth_ranges(bits, count, s["xyz"], s["R"], s["t"], lo=lo, hi=hi)
    want, want_n = U.depth_ranges_ref(s["seen"], s["xyz"], s["R"], s["t"], lo, hi)
    assert n.cpu().tolist() == want_n.tolist() == list(COUNTS)
    assert _same_bits32(rng.cpu().numpy(), want)
    assert rng.cpu().numpy()[0].tolist() == [0.0, 0.0]                    # the view without points: (0, 0), reported in n, no error
    roomy, _ = _sp().depth_ranges(bits, count, s["xyz"], s["R"], s["t"], lo=lo, hi=hi, capacity=len(s["obs_point"]) + 1000)
    assert torch.equal(roomy, rng)


@pytest.mark.parametrize("V,N", [(2, 1), (3, 64), (5, 4097), (70, 4096)])
def test_depth_ranges_on_the_ring_scenes(V, N):
    s = _scene(V, N, seed=300 + V + N)
    bits, count, _ = _sp().visibility(s["xyz"], s["obs_point"], s["obs_view"], V)
    rng, n = _sp().depth_ranges(bits, count, s["xyz"], s["R"], s["t"])
    want, want_n = U.depth_ranges_ref(s["seen"], s["xyz"], s["R"], s["t"])
    assert n.cpu().tolist() == want_n.tolist() and _same_bits32(rng.cpu().numpy(), want)


def test_depth_ranges_report_a_workspace_that_is_too_small():
    s = _depth_scene()
    V = len(COUNTS)
    bits, count, _ = _sp().visibility(s["xyz"], s["obs_point"], s["obs_view"], V)
    rng, n = _sp().depth_ranges(bits, count, s["xyz"], s["R"], s["t"], capacity=sum(COUNTS[:5]))
    want, _ = U.depth_ranges_ref(s["seen"], s["xyz"], s["R"], s["t"])
    assert n.cpu().tolist() == list(COUNTS[:5]) + [-1, -1]
    assert _same_bits32(rng.cpu().numpy()[:5], want[:5]) and not rng.cpu().numpy()[5:].any()
    from mvsformer_amd._lib import MvsHipError
    for lo, hi in ((-0.1, 0.5), (0.6, 0.5), (0.1, 1.5), (float("nan"), 0.5)):
        with pytest.raises(MvsHipError):
            _sp().depth_ranges(bits, count, s["xyz"], s["R"], s["t"], lo=lo, hi=hi)


# ----------------------------------------------------------------------------------------------------------- whole scene
def test_prepare_scene_end_to_end(tmp_path):
    from mvsformer_amd import data_io
    kw, _, _ = RANK_SCENES["arc12"]
    s = _scene(**kw)
    V = kw["V"]
    want = U.prepare_ref(s, num_views=5, num_depth=48, interval_scale=1.06)
    assert U.rank_gaps_ok(want["S"], 5)
    got = _sp().prepare_scene(s["xyz"], s["obs_point"], s["obs_view"], s["R"], s["t"], num_views=5, num_depth=48, interval_scale=1.06)
    assert got["pairs"] == want["pairs"] and all(len(srcs) == 5 for _, srcs in got["pairs"])
    assert _same_bits32(got["depth_min"], want["depth_min"]) and _same_bits32(got["depth_max"], want["depth_max"])
    assert np.array_equal(got["depth_interval"], want["depth_interval"]) and got["n_points"].tolist() == want["n_points"].tolist()
    assert got["n_nonfinite"] == 0 and (got["depth_interval"] > 0).all()
    K = np.stack([np.array([[600.0 + v, 0, 320], [0, 600.0 + v, 240], [0, 0, 1]], np.float32) for v in range(V)])
    _sp().write_scan(str(tmp_path), got, s["R"], s["t"], K, num_depth=48)
    assert data_io.read_pair_file(str(tmp_path / "pair.txt")) == want["pairs"]
    for v in range(V):
        Kv, E = data_io.read_camera_parameters(str(tmp_path / "cams" / ("%08d_cam.txt" % v)))
        assert np.array_equal(Kv, K[v]) and np.array_equal(E[:3, :3], s["R"][v]) and np.array_equal(E[:3, 3], s["t"][v])
        assert E[3].tolist() == [0, 0, 0, 1]
        row = open(str(tmp_path / "cams" / ("%08d_cam.txt" % v))).read().split("\n")[11].split()
        assert np.float32(row[0]) == got["depth_min"][v] and np.float32(row[3]) == got["depth_max"][v] and float(row[2]) == 48.0
        assert abs(float(row[1]) - got["depth_interval"][v]) <= 1e-6 * got["depth_interval"][v]


def test_prepare_scene_leaves_out_sources_that_share_nothing():
    kw, _, _ = RANK_SCENES["lonely_k_above_v"]
    s = _scene(**kw)
    got = _sp().prepare_scene(s["xyz"], s["obs_point"], s["obs_view"], s["R"], s["t"], num_views=20)
    want = U.prepare_ref(s, num_views=20)
    assert got["pairs"] == want["pairs"]
    assert got["pairs"][4] == (4, []) and all(4 not in srcs and len(srcs) == 4 for v, srcs in got["pairs"] if v != 4)
    assert got["n_points"][4] == 0 and got["depth_min"][4] == 0.0 and got["depth_max"][4] == 0.0
    listed = _sp().prepare_scene(s["xyz"], s["obs_point"], s["obs_view"], s["R"], s["t"], num_views=20, keep_zero=True)
    assert listed["pairs"] == U.prepare_ref(s, num_views=20, keep_zero=True)["pairs"]
    assert listed["pairs"][4] == (4, [0, 1, 2, 3, 5]) and all(srcs[-1] == 4 and len(srcs) == 5 for v, srcs in listed["pairs"] if v != 4)
