"""CPU-side checks of the training-recipe optimizer (mvsformer_amd/optim.py): the layer-wise ViT parameter groups against the reference's
own, the by-value table entry of the multi-group kernels against the C compiler's layout, the refusals, and ``state_dict()`` leaving the
live optimizer state alone."""
import json
import os

import pytest
import torch

from conftest import GOLDEN, REPO


def test_vit_param_groups_match_the_reference():
    """``vit_param_groups(vit_small())`` == the reference's ``param_groups_lrd`` on the same module (models/lr_decay.py:13-83), recorded by
    tools/gen_optim_golden.py as names and numbers: per group the parameter names, ``lr``, ``lr_scale``, ``weight_decay``, in order."""
    from mvsformer_amd.optim import vit_param_groups
    from mvsformer_amd.vit import vit_small
    gold = json.load(open(os.path.join(GOLDEN, "lrd_groups_vit_small.json")))
    assert len(gold["groups"]) == 27 and sum(len(g["params"]) for g in gold["groups"]) == 150
    vit = vit_small()
    names = {id(p): n for n, p in vit.named_parameters()}
    groups = vit_param_groups(vit, gold["vit_lr"], weight_decay=gold["weight_decay"], no_weight_decay_list=set(gold["no_weight_decay_list"]),
                              layer_decay=gold["layer_decay"])
    assert len(groups) == len(gold["groups"])
    for k, (mine, want) in enumerate(zip(groups, gold["groups"])):
        assert set(mine) == {"lr", "lr_scale", "weight_decay", "params", "vit_param"}, (k, sorted(mine))
        assert [names[id(p)] for p in mine["params"]] == want["params"], k
        assert mine["lr"] == want["lr"] and mine["lr_scale"] == want["lr_scale"] and mine["weight_decay"] == want["weight_decay"], (k, mine, want)
        assert mine["vit_param"] is True and want["vit_param"] is True
    # the groups go to the optimizer as they are: extra keys are carried, the scale is NOT applied (the reference never applies it)
    from mvsformer_amd.optim import FusedAdamW
    opt = FusedAdamW(groups + [dict(params=[torch.nn.Parameter(torch.ones(2))], lr=1e-3)], lr=1e-3, device_hyper=True)
    assert len(opt.param_groups) == 28 and opt.param_groups[0]["lr_scale"] == gold["groups"][0]["lr_scale"] and opt.param_groups[0]["lr"] == gold["vit_lr"]


def test_adam_entry_layout_matches_the_header(tmp_path):
    """``MvsAdamEntry`` (the by-value table entry of mvs_adamw_multi / mvs_grad_norm / mvs_grad_scale_) as the C compiler lays it out against
    its ctypes twin: size and every field offset; the hyper-parameter row stride too."""
    import ctypes
    import shutil
    import subprocess
    from mvsformer_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    ct = _lib.AdamEntry
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mvs_hip.h"', 'int main(void) {',
             'printf("%zu", sizeof(MvsAdamEntry));']
    for f, _ in ct._fields_:
        lines.append('printf(" %%zu", offsetof(MvsAdamEntry, %s));' % f)
    lines += ['printf(" %d %d\\n", MVS_ADAM_HYPER_STRIDE, MVS_ABI_VERSION);', 'return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    want = [int(v) for v in subprocess.check_output([str(exe)]).decode().split()]
    got = [ctypes.sizeof(ct)] + [getattr(ct, f).offset for f, _ in ct._fields_] + [_lib.ADAM_HYPER_STRIDE, _lib.ABI_VERSION]
    assert got == want, (got, want)
    assert [f for f, _ in ct._fields_] == ["p", "g", "m", "v", "n", "group", "reserved"] and ctypes.sizeof(ct) == 48
    for name in ("mvs_adamw_multi", "mvs_grad_norm_workspace_bytes", "mvs_grad_norm", "mvs_grad_scale_", "mvs_adamw_step"):
        assert name in _lib.SIGNATURES


def test_recipe_refusals():
    """No quiet other path: clipping and AMP scaling need the device table, CPU parameters and amsgrad are refused, bad table entries are
    refused by the library before any launch."""
    import ctypes
    from mvsformer_amd import _lib
    from mvsformer_amd._lib import MvsHipError
    from mvsformer_amd.optim import FusedAdamW, clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(3))
    with pytest.raises(MvsHipError):
        FusedAdamW([p], lr=1e-3, max_grad_norm=1.0)                     # needs device_hyper=True
    with pytest.raises(MvsHipError):
        FusedAdamW([p], lr=1e-3, device_hyper=True, amsgrad=True)
    opt = FusedAdamW([p], lr=1e-3, device_hyper=True, max_grad_norm=1.0)
    assert opt._step_supports_amp_scaling is True
    assert not hasattr(FusedAdamW([p], lr=1e-3), "_step_supports_amp_scaling")
    p.grad = torch.ones(3)
    with pytest.raises(MvsHipError):
        opt.step()                                                      # CPU parameters: there is no CPU path
    with pytest.raises(MvsHipError):
        opt.sync_hyper()
    with pytest.raises(MvsHipError):
        clip_grad_norm_([p], 1.0)
    plain = FusedAdamW([p], lr=1e-3)
    plain.grad_scale, plain.found_inf = torch.ones(()), torch.zeros(())   # what a GradScaler would set on an optimizer that declares support
    with pytest.raises(MvsHipError):
        plain.step()
    with pytest.raises(MvsHipError):
        plain.sync_hyper()                                              # no device table on the default path
    lib = _lib.load()
    fake = 0x1000                                                       # never dereferenced: the calls are refused on the host
    arr = (_lib.AdamEntry * 2)()
    for t in arr:
        t.p = t.g = t.m = t.v = fake
        t.n = 5
    arr[1].group = 3
    tab = ctypes.cast(arr, ctypes.c_void_p)
    assert lib.mvs_grad_norm_workspace_bytes(tab, 2) == 2 * 8 and lib.mvs_grad_norm_workspace_bytes(None, 2) < 0
    arr[1].n = 2049
    assert lib.mvs_grad_norm_workspace_bytes(tab, 2) == 3 * 8
    assert lib.mvs_adamw_multi(tab, 2, fake, 2, fake, None, None, None, None) < 0 and b"group 3 of 2" in lib.mvs_last_error()
    assert lib.mvs_adamw_multi(tab, 2, None, 4, fake, None, None, None, None) < 0 and b"mvs_adamw_multi" in lib.mvs_last_error()
    assert lib.mvs_adamw_multi(tab, 2, fake, 2000, fake, None, None, None, None) < 0
    assert lib.mvs_grad_norm(tab, 2, 1.0, None, None, None, fake, fake, None, None) < 0 and b"mvs_grad_norm" in lib.mvs_last_error()
    assert lib.mvs_grad_scale_(tab, 0, fake, None) < 0 and b"mvs_grad_scale_" in lib.mvs_last_error()
    arr[0].g = None
    assert lib.mvs_grad_norm_workspace_bytes(tab, 2) == 3 * 8


def test_state_dict_leaves_the_live_state_alone():
    """``state_dict()`` adds torch's per-parameter ``'step'`` to the checkpoint, not to ``opt.state[p]`` (it used to write a CPU tensor into
    the live state on every save).  The state is built by hand: ``step()`` has no CPU path."""
    from mvsformer_amd.optim import FusedAdamW
    ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]
    for device_hyper in (False, True):
        opt = FusedAdamW([dict(params=ps[:1], lr=1e-2), dict(params=ps[1:])], lr=1e-3, device_hyper=device_hyper)
        for p in ps:
            opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
        opt.param_groups[0]["step"], opt.param_groups[1]["step"] = torch.tensor(3.0), torch.tensor(5.0)
        for _ in range(2):
            sd = opt.state_dict()
            assert [float(sd["state"][k]["step"]) for k in (0, 1)] == [3.0, 5.0] and [float(g["step"]) for g in sd["param_groups"]] == [3.0, 5.0]
            for p in ps:
                assert sorted(opt.state[p]) == ["exp_avg", "exp_avg_sq"], sorted(opt.state[p])
        assert sd["state"][0]["exp_avg"] is opt.state[ps[0]]["exp_avg"]          # the moments themselves are shared, as torch shares them
        other = torch.optim.AdamW([dict(params=[torch.nn.Parameter(torch.ones(3))], lr=1e-2), dict(params=[torch.nn.Parameter(torch.ones(2, 2))])], lr=1e-3)
        other.load_state_dict(sd)                                               # still torch.optim.AdamW's layout
        assert float(other.state[other.param_groups[1]["params"][0]]["step"]) == 5.0
