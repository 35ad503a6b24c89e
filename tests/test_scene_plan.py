"""CPU checks of scene-resident inference: ``scene.plan`` (which image goes into which bank slot before which sample) on hand-made pair
lists, and the C-ABI declarations of the view-indexed sweeps and ``mvs_conf_stack`` (header and ctypes table agree)."""
import os
import re

import pytest

from conftest import REPO

# a 7-view scan in pair.txt form: every view with four sources, nearest first
PAIRS = [(0, [1, 2, 3, 4]), (1, [0, 2, 3, 5]), (2, [1, 3, 0, 4]), (3, [2, 4, 1, 5]), (4, [3, 5, 2, 6]), (5, [4, 6, 3, 2]), (6, [5, 4, 3, 0])]


def _simulate(steps, capacity):
    """Replay a plan on a model of the bank: -> extractions per view; asserts that every sample's table names slots holding its views."""
    bank = {}
    count = {}
    for st in steps:
        slots = [s for _, s in st["extract"]]
        assert len(set(slots)) == len(slots), "two images into one slot in one step"
        for v, s in st["extract"]:
            assert 0 <= s < capacity
            bank[s] = v
            count[v] = count.get(v, 0) + 1
        assert len(st["table"]) == len(st["views"]) and st["views"][0] == st["ref"]
        assert [bank.get(s) for s in st["table"]] == st["views"], (st, bank)
    return count


@pytest.mark.parametrize("num_views", [2, 3, 5])
@pytest.mark.parametrize("extract_batch", [1, 4])
def test_plan_full_capacity_extracts_every_image_once(num_views, extract_batch):
    from mvsformer_amd import scene
    for cap in (None, 7, 12):
        steps = scene.plan(PAIRS, num_views, cap, extract_batch=extract_batch)
        assert [st["ref"] for st in steps] == [r for r, _ in PAIRS]
        for st, (r, srcs) in zip(steps, PAIRS):
            assert st["views"] == [r] + srcs[:num_views - 1]
        count = _simulate(steps, cap or 7)
        used = {v for st in steps for v in st["views"]}
        assert set(count) == used and all(c == 1 for c in count.values()), count


@pytest.mark.parametrize("num_views", [2, 3, 5])
@pytest.mark.parametrize("extract_batch", [1, 4])
def test_plan_minimal_capacity_is_valid(num_views, extract_batch):
    """capacity = num_views: every table still valid, a view is extracted at most once per sample, and evicted views come back."""
    from mvsformer_amd import scene
    steps = scene.plan(PAIRS, num_views, num_views, extract_batch=extract_batch)
    count = _simulate(steps, num_views)
    for st in steps:
        ids = [v for v, _ in st["extract"]]
        assert len(set(ids)) == len(ids), st
        assert set(ids) <= set(st["views"])                     # no room to prefetch: only what the sample needs
    assert sum(count.values()) <= len(PAIRS) * num_views
    if num_views == 5:
        assert count[0] == 2                                    # view 0 leaves the five-slot bank after sample 2 and is needed again by sample 6


def test_plan_lru_eviction_order():
    from mvsformer_amd import scene
    pairs = [(0, [1]), (2, [3]), (0, [2]), (4, [0])]
    steps = scene.plan(pairs, 2, 3)
    assert steps[0]["extract"] == [(0, 0), (1, 1)] and steps[0]["table"] == [0, 1]
    # slot 2 is free for view 2; view 3 evicts the least recently used of {0, 1}: view 0 (slot 0; same step, lower slot)
    assert steps[1]["extract"] == [(2, 2), (3, 0)] and steps[1]["table"] == [2, 0]
    # view 0 comes back into the slot of the oldest view that is not part of the sample: view 1 (slot 1)
    assert steps[2]["extract"] == [(0, 1)] and steps[2]["table"] == [1, 2]
    # view 4 evicts view 3 (last used at step 1), views 0 and 2 were used at step 2
    assert steps[3]["extract"] == [(4, 0)] and steps[3]["table"] == [0, 1]


def test_plan_prefetch_fills_the_batch_from_following_samples():
    from mvsformer_amd import scene
    steps = scene.plan(PAIRS, 3, None, extract_batch=4)
    assert [v for v, _ in steps[0]["extract"]] == [0, 1, 2, 3]       # the sample's three views + the next new one (view 3 of sample 2)
    assert all(len(st["extract"]) <= 4 for st in steps)
    _simulate(steps, 7)


def test_plan_rejects_bad_input():
    from mvsformer_amd import scene
    with pytest.raises(ValueError):
        scene.plan(PAIRS, 5, 4)                                  # capacity < num_views
    with pytest.raises(ValueError):
        scene.plan(PAIRS, 5, 7, view_ids=[0, 1, 2, 3, 4, 5])     # source 6 is not among the images
    with pytest.raises(ValueError):
        scene.plan([(0, [])], 3, 3)
    with pytest.raises(ValueError):
        scene.plan(PAIRS, 1, 7)
    assert scene.plan(PAIRS, 5, 7, view_ids=range(7))


def test_scene_inference_refuses_cpu_and_training():
    import torch
    import mvsformer_amd as m
    from mvsformer_amd._lib import MvsHipError
    args = dict(fix=True, depth_type="ce", fusion_type="cnn", inverse_depth=True, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
                depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
                vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                              att_fusion=True, nhead=6))
    net = m.DINOMVSNet(args)
    with pytest.raises(MvsHipError):
        m.SceneInference(net.train())
    si = m.SceneInference(net.eval())
    with pytest.raises(MvsHipError):                            # no CPU fallback
        si.add_image(0, torch.zeros(3, 64, 64), torch.zeros(2, 4, 4), torch.ones(8))
    with pytest.raises(MvsHipError):
        net.train().forward_bank({}, [[0, 1]], {}, torch.ones(1, 8))
    with pytest.raises(MvsHipError):
        net.fusions[0].forward_bank(torch.zeros(2, 8, 8, 64), [[0, 1]], torch.zeros(1, 2, 2, 4, 4), torch.ones(1, 4, 8, 8))


NEW_SYMBOLS = {"mvs_cv_entropy_fwd_views": 15, "mvs_cv_aggregate_fwd_views": 17, "mvs_cv_corr_rows_fwd_views": 18, "mvs_conf_stack": 8}


def test_new_symbols_declared_in_header_and_ctypes_table():
    from mvsformer_amd import _lib
    src = open(os.path.join(REPO, "include", "mvs_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = {}
    for m in re.finditer(r"(mvs_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else len(args.split(","))
    for name, nargs in NEW_SYMBOLS.items():
        assert protos.get(name) == nargs, (name, protos.get(name))
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.I and len(args) == nargs, (name, len(args))
    # the dense entries next to them keep their argument lists: the indexed forms add (view_idx, N)
    assert protos["mvs_cv_entropy_fwd"] == 13 and protos["mvs_cv_aggregate_fwd"] == 15 and protos["mvs_cv_corr_rows_fwd"] == 16
    m = re.search(r"#define\s+MVS_ABI_VERSION\s+(\d+)", src)
    assert int(m.group(1)) == _lib.ABI_VERSION
