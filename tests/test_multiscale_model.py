"""CPU-side checks of the ``multi_scale`` / ``att_fusion`` variants of ``DINOMVSNet``: construction, the reference's ``state_dict`` keys in the
reference's order (tests/golden/dinomvsnet_ms_shapes.json and the key lists in vit_decoder_ms_train.npz, tools/gen_multiscale_golden.py), the
refused combination, no CPU fallback, and ``install(features=True)``."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import multiscale_util as mu


def _shapes(net):
    return {k: list(v.shape) for k, v in net.state_dict().items()}


def test_multi_scale_model_has_the_reference_keys_in_order():
    import mvsformer_amd as m
    want = json.load(open(os.path.join(GOLDEN, "dinomvsnet_ms_shapes.json")))
    net = m.DINOMVSNet(mu.model_args(multi_scale=True))
    assert isinstance(net.decoder, m.FPNDecoderV2) and isinstance(net.decoder_vit, m.VITDecoderStage4)
    mine = _shapes(net)
    assert list(mine) == list(want) and mine == want
    assert [n for n, _ in net.named_children()] == ["encoder", "decoder", "vit", "decoder_vit", "fusions"]


@pytest.mark.parametrize("kind,cls,args", mu.DECODERS)
def test_decoders_have_the_reference_keys_in_order(kind, cls, args):
    import mvsformer_amd as m
    want = json.loads(str(np.load(os.path.join(GOLDEN, "vit_decoder_ms_train.npz"))[kind + ".keys"]))
    mine = _shapes(getattr(m, cls)(args))
    assert list(mine) == list(want) and mine == want
    if kind == "chain":                                      # decoder2.0 / decoder3.0 are BatchNorms in the chained form
        assert "decoder2.0.running_var" in mine and "decoder3.0.running_var" in mine


def test_att_fusion_false_builds_the_noatt_decoder():
    import mvsformer_amd as m
    net = m.DINOMVSNet(mu.model_args(multi_scale=False, att_fusion=False))
    assert isinstance(net.decoder, m.FPNDecoder) and isinstance(net.decoder_vit, m.VITDecoderStage4NoAtt)
    want = json.loads(str(np.load(os.path.join(GOLDEN, "vit_decoder_ms_train.npz"))["noatt.keys"]))
    assert [k[len("decoder_vit."):] for k in net.state_dict() if k.startswith("decoder_vit.")] == list(want)
    base = json.load(open(os.path.join(GOLDEN, "dinomvsnet_shapes.json")))
    other = lambda keys: [k for k in keys if not k.startswith("decoder_vit.")]
    assert other(net.state_dict()) == other(base)            # everything else as in the shipped config, same order


def test_impossible_combination_is_refused():
    import mvsformer_amd as m
    from mvsformer_amd._lib import MvsHipError
    with pytest.raises(MvsHipError, match="att_fusion"):
        m.DINOMVSNet(mu.model_args(multi_scale=True, att_fusion=False))


@pytest.mark.parametrize("kw", [dict(multi_scale=True), dict(multi_scale=False, att_fusion=False)])
def test_cpu_tensors_raise(kw):
    import mvsformer_amd as m
    from mvsformer_amd._lib import MvsHipError
    net = m.DINOMVSNet(mu.model_args(**kw)).eval()
    with pytest.raises(MvsHipError):
        net(torch.zeros(1, 3, 3, 64, 64), {"stage%d" % i: torch.zeros(1, 3, 2, 4, 4) for i in range(1, 5)}, torch.ones(1, 8))


def test_install_rebinds_a_class_that_accepts_the_flags(monkeypatch):
    import mvsformer_amd as m
    from mvsformer_amd.install import install
    names = json.load(open(os.path.join(GOLDEN, "reference_names.json")))
    monkeypatch.setitem(sys.modules, "models", types.ModuleType("models"))
    mods = {}
    for name, syms in names.items():
        mod = types.ModuleType(name)
        for s in syms:
            setattr(mod, s, object())
        mods[name] = mod
        monkeypatch.setitem(sys.modules, name, mod)
    done = install(features=True)
    mm = mods["models.mvsformer_model"]
    assert "DINOMVSNet" in done["models.mvsformer_model"] and mm.DINOMVSNet is m.DINOMVSNet
    for name in ("VITDecoderStage4", "VITDecoderStage4NoAtt", "FPNDecoderV2"):
        assert getattr(mods["models.module"], name) is getattr(m, name), name
    assert isinstance(mm.DINOMVSNet(mu.model_args(multi_scale=True)).decoder_vit, m.VITDecoderStage4)
    assert isinstance(mm.DINOMVSNet(mu.model_args(multi_scale=False, att_fusion=False)).decoder_vit, m.VITDecoderStage4NoAtt)
