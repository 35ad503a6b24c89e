"""CPU checks behind the sample-preparation kernels: the numpy restatement of PIL's colour steps is PIL bit for bit (and equals the
recorded fixture on a machine without PIL), the resize restatements hold what can be derived, ``draw_train_params`` consumes the
generators in the reference's order, and the header, ctypes table and library agree on the new entries."""
import itertools
import os
import random
import re

import numpy as np
import pytest
import torch

import sample_prep_util as u
from conftest import GOLDEN, REPO, load_golden


def _pil():
    return pytest.importorskip("PIL.Image")


def test_restatement_equals_the_recorded_pil_outputs():
    z = load_golden("sample_prep.npz")
    for o, want in zip(z["orders"], z["out"]):
        assert np.array_equal(u.jitter(z["img"], o, tuple(z["factors"])), want), o
    for (op, v), want in zip(z["singles"], z["single_out"]):
        f = [1.0, 1.0, 1.0, 0.0]
        f[int(op)] = float(v)
        assert np.array_equal(u.jitter(z["img"], [int(op)], tuple(f)), want), (op, v)


def test_hue_equals_pil_over_all_colours():
    _pil()
    c = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    cube = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8)
    assert np.array_equal(u.hue(cube, 0.3), u.jitter_pil(cube, [3], (1.0, 1.0, 1.0, 0.3)))


def test_blend_steps_equal_pil_at_the_clamps():
    _pil()
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    img[0, :3] = [[0, 0, 0], [255, 255, 255], [255, 0, 1]]
    half = np.full((16, 24, 3), 100, np.uint8)
    half[:8] = 101                                                # mean(L) = 100.5
    assert u.contrast_mean(half) == 101
    for im in (img, half):
        for f in (0.0, 0.3, 1.0, 1.7, 2.5, 3.0):
            assert np.array_equal(u.brightness(im, f), u.jitter_pil(im, [0], (f, 1.0, 1.0, 0.0))), f
            assert np.array_equal(u.contrast(im, f), u.jitter_pil(im, [1], (1.0, f, 1.0, 0.0))), f
            assert np.array_equal(u.saturation(im, f), u.jitter_pil(im, [2], (1.0, 1.0, f, 0.0))), f
    for hf in (-0.5, -0.2, 0.0, 0.5):
        assert np.array_equal(u.hue(img, hf), u.jitter_pil(img, [3], (1.0, 1.0, 1.0, hf))), hf
    for o in itertools.permutations(range(4)):
        assert np.array_equal(u.jitter(img, o, (0.8, 1.3, 0.7, 0.1)), u.jitter_pil(img, o, (0.8, 1.3, 0.7, 0.1))), o


def test_resize_restatements_hold_what_can_be_derived():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert np.array_equal(u.area_resize(img, 37, 53), img)
    for dh, dw in ((16, 23), (27, 38), (18, 26)):
        for tab, n in ((u.area_tab(37, dh), 37), (u.area_tab(53, dw), 53)):
            for taps in tab:
                assert abs(sum(w for _, w in taps) - 1.0) < 2.5e-3 and all(0 <= s < n for s, _ in taps)     # 1e-3 slivers are dropped
        a, f = u.area_resize(img, dh, dw), u.area_resize_f64(img, dh, dw)
        near = np.abs(np.abs(f - np.floor(f)) - 0.5) <= 2.0 ** -10
        d = a.astype(np.int64) - np.rint(f).astype(np.int64)
        assert np.abs(d).max() <= 1 and not (d != 0)[~near].any()
    even = rng.integers(0, 256, (64, 96, 3), dtype=np.uint8)
    assert np.array_equal(u.area_resize(even, 32, 48), np.floor(u.area_resize_f64(even, 32, 48) + 0.5).astype(np.uint8))
    for H, W in ((64, 64), (64, 128), (37, 53)):
        lin = u.linear_resize(img, H, W)
        assert np.abs(lin.astype(np.float64) - u.linear_resize_f64(img, H, W)).max() <= 1.0
    assert np.array_equal(u.linear_resize(img, 37, 53), img)
    assert np.array_equal(u.nn_index(16, 37), np.minimum(np.floor(np.arange(16) * (37 / 16)).astype(np.int64), 36))
    assert np.array_equal(u.stage_pyramid(img[:16, :24, 0])["stage1"], img[0:16:8, 0:24:8, 0])


def test_resize_restatements_equal_cv2_where_it_imports():
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    for dh, dw in ((16, 23), (27, 38), (18, 26), (37, 53)):
        assert np.array_equal(u.area_resize(img, dh, dw), cv2.resize(img, (dw, dh), interpolation=cv2.INTER_AREA))
        assert np.array_equal(u.nearest_resize(img, dh, dw), cv2.resize(img, (dw, dh), interpolation=cv2.INTER_NEAREST))
    for H, W in ((64, 64), (64, 128)):
        assert np.array_equal(u.linear_resize(img, H, W), cv2.resize(img, (W, H)))


def test_depth_values_equal_numpy_arange():
    from mvsformer_amd import sample_prep as sp
    for a, b, n in ((425.0, 2.65, 192), (425.0, 2.5 * 1.06, 192), (0.5, 0.1, 7), (1.0, 0.3, 7), (425.0, 2.65, 7), (0.0, 0.7, 7)):
        want = np.arange(a, b * n + a, b, dtype=np.float32)
        assert sp.arange_length(a, b, n) == len(want)
        assert np.array_equal(u.depth_values(a, b, n), want), (a, b, n)
    assert sp.arange_length(0.5, 0.1, 7) == 8                      # the length rule: 7 hypotheses asked for, arange yields 8


def test_draw_train_params_follows_the_reference_order():
    """A hand-written trace of the generator calls of dtu_dataset_ms.py::__getitem__ (:255-333), seeds fixed."""
    from mvsformer_amd import sample_prep as sp
    aug = dict(brightness=0.2, contrast=(0.9, 1.1), saturation=0.1, hue=0.05, min_gamma=0.7, max_gamma=1.5)
    crop, hw, V, K = (64, 64), (96, 128), 3, 2
    for consist in (False, True):
        random.seed(5), np.random.seed(6), torch.manual_seed(7)
        views = list(range(1, 8))
        got = sp.draw_train_params(0, views, V, crop, src_hw=hw, augment=True, aug_args=aug, resize_range=(1.0, 1.2), consist_crop=consist, K=K)
        random.seed(5), np.random.seed(6), torch.manual_seed(7)
        src = list(range(1, 8))
        np.random.shuffle(src)                                    # :256
        fn_idx = torch.randperm(4)                                # :268
        fac = [torch.tensor(1.0).uniform_(lo, hi).item() for lo, hi in ((0.8, 1.2), (0.9, 1.1), (0.9, 1.1), (-0.05, 0.05))]      # :269-272
        gamma = np.random.uniform(0.7, 1.5)                       # :273
        scales, cands, offs = [], [], []
        for i in range(V):
            enlarge = 1.0 + random.random() * (1.2 - 1.0)         # :298
            rs = max(np.clip(64 * enlarge / 96, 0.45, 1.0), np.clip(64 * enlarge / 128, 0.45, 1.0))
            scales.append(rs)
            rh, rw = (int(96 * rs), int(128 * rs)) if rs != 1.0 else (96, 128)
            if i == 0:
                for _ in range(K):                                # :313 with :226-227, once per candidate
                    oy = random.randint(0, rh - 64)
                    cands.append((oy, random.randint(0, rw - 64)))
            elif not consist:
                oy = random.randint(0, rh - 64)
                offs.append((oy, random.randint(0, rw - 64)))
            else:
                offs.append(None)
        assert views == src and got.view_ids == [0] + src[:V - 1]
        assert got.fn_idx == [int(i) for i in fn_idx] and list(got.factors) == fac and got.gamma == gamma
        assert got.resize_scales == [float(s) for s in scales] and got.candidates == cands and got.src_offsets == offs
        assert got.enabled == (True, True, True, True)
    assert sp.jitter_range(0, "brightness") is None and sp.jitter_range((1.0, 1.0), "contrast") is None and sp.jitter_range(0, "hue") is None
    val = sp.draw_train_params(0, [1, 2, 3], 3, crop, src_hw=hw, mode="val", resize_scale=0.75)
    assert val.fn_idx is None and val.resize_scales == [0.75] * 3 and val.candidates == [(4, 16)] and val.src_offsets == [(4, 16)] * 2
    assert sp.hue_shift(-0.5) == 129 and sp.hue_shift(0.5) == 127 and sp.hue_shift(0.0) == 0


def test_scaled_cameras_of_the_scan_tool(tmp_path):
    """tools/infer_scan.py --max_h 64 --max_w 64 on a three-view 75x100 synthetic scan: the camera files it writes carry the intrinsics
    of scale_mvs_input (rows 0 and 1 times 64 / 100 and 64 / 75 in fp32); without the flags the camera is passed through."""
    import importlib.util
    from mvsformer_amd import sample_prep as sp
    spec = importlib.util.spec_from_file_location("infer_scan", os.path.join(REPO, "tools", "infer_scan.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    scan = tmp_path / "scan"
    (scan / "cams").mkdir(parents=True)
    rng = np.random.default_rng(4)
    for v in range(3):
        k = np.array([[361.5 + v, 0, 50.2], [0, 360.25, 37.7], [0, 0, 1]], np.float32)
        e = np.eye(4, dtype=np.float32)
        e[:3, 3] = rng.normal(size=3)
        with open(scan / "cams" / ("%08d_cam.txt" % v), "w") as f:
            f.write("extrinsic\n" + "\n".join(" ".join(repr(float(x)) for x in r) for r in e) + "\n\nintrinsic\n" +
                    "\n".join(" ".join(repr(float(x)) for x in r) for r in k) + "\n\n425.0 2.5\n")
        cam = tool.scaled_camera(str(scan / "cams" / ("%08d_cam.txt" % v)), (75, 100), (64, 64))
        want = k.copy()
        want[0, :] *= np.float32(64 / 100)
        want[1, :] *= np.float32(64 / 75)
        assert cam.shape == (2, 4, 4) and np.array_equal(cam[1, :3, :3], want) and np.array_equal(cam[0], e)
        assert np.array_equal(cam[1, :3, :3], sp.scale_intrinsics(k, (75, 100), (64, 64)))
        same = tool.scaled_camera(str(scan / "cams" / ("%08d_cam.txt" % v)), (64, 128), None)
        assert np.array_equal(same[1, :3, :3], k)
    a = tool.parse_args(["--scan", str(scan), "--checkpoint", "x", "--out", "o", "--max_h", "64", "--max_w", "64"])
    assert (a.max_h, a.max_w) == (64, 64)
    assert tool.parse_args(["--scan", "s", "--checkpoint", "x", "--out", "o"]).max_h is None
    with pytest.raises(SystemExit):
        tool.parse_args(["--scan", "s", "--checkpoint", "x", "--out", "o", "--max_h", "100", "--max_w", "64"])


def test_header_table_and_library_agree_on_the_prep_entries():
    from mvsformer_amd import _lib, _sources
    src = open(os.path.join(REPO, "include", "mvs_hip.h")).read()
    names = set(re.findall(r"^(?:int|int64_t)\s+(mvs_prep_\w+)\s*\(", src, flags=re.M))
    assert names == {n for n in _lib.SIGNATURES if n.startswith("mvs_prep_")} and len(names) == 6
    assert "#define MVS_ABI_VERSION 51" in src and _lib.ABI_VERSION == 51
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    assert lib.mvs_prep_pyramid_floats(2, 64, 64) == 2 * (64 * 64 + 32 * 32 + 16 * 16 + 8 * 8) and lib.mvs_prep_pyramid_floats(1, 4, 64) == -1
    assert lib.mvs_prep_area_crop(None, None, None, 1, 1, 8, 8, 16, 16, None, None) < 0 and b"mvs_prep_area_crop" in lib.mvs_last_error()
    assert _sources.files_of("prep_area_crop_kernel")[0] == "sample_prep.hip" and _sources.files_of("mvs_prep_accept")[0] == "sample_prep.hip"
