"""CPU checks of the ViT fine-tuning plumbing (mvsformer_amd/mvsformer_model.py, mvsformer_amd/vit.py): ``vit_args['vit_path']`` loads the
pretrained DINO weights into ``model.vit`` as the reference does (mvsformer_model.py:182-193), and what training mode does not build is
refused before anything runs."""
import os

import pytest
import torch


def _args(vit_path):
    return dict(fix=False, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4], feat_chs=[8, 16, 32, 64],
                depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=False,
                vit_args=dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                              att_fusion=True, nhead=6, vit_path=vit_path))


def _vit_sd(seed):
    from oracle.weights import load_vit_shapes, make_vit_state_dict
    return make_vit_state_dict(load_vit_shapes("vit_small"), seed)


def _assert_loaded(net, sd):
    got = net.vit.state_dict()
    assert set(got) == set(sd)
    for k, v in sd.items():
        assert torch.equal(got[k], v.to(got[k].dtype)), k


def test_vit_path_plain_checkpoint(tmp_path, capsys):
    import mvsformer_amd as m
    sd = _vit_sd(21)
    path = os.path.join(str(tmp_path), "dino_deitsmall16_pretrain.pth")
    torch.save({"model": sd, "epoch": 3}, path)
    net = m.DINOMVSNet(_args(path))
    _assert_loaded(net, sd)
    out = capsys.readouterr().out
    assert "missing keys:[]" in out and "unexpected keys:[]" in out


def test_vit_path_model_best_with_vit_prefix(tmp_path):
    import mvsformer_amd as m
    sd = _vit_sd(22)
    full = {"vit." + k: v for k, v in sd.items()}
    full["encoder.conv0.0.weight"] = torch.zeros(1)              # other sub-modules' keys are not the ViT's
    path = os.path.join(str(tmp_path), "model_best.pth")
    torch.save({"state_dict": full, "epoch": 10}, path)
    net = m.DINOMVSNet(_args(path))
    _assert_loaded(net, sd)


def test_vit_path_partial_checkpoint_reports_missing_keys(tmp_path, capsys):
    import mvsformer_amd as m
    sd = _vit_sd(23)
    part = {k: v for k, v in sd.items() if not k.startswith("blocks.11.")}
    part["head.weight"] = torch.zeros(3)
    path = os.path.join(str(tmp_path), "vit.pth")
    torch.save(part, path)
    net = m.DINOMVSNet(_args(path))
    assert torch.equal(net.vit.blocks[0].attn.qkv.weight, sd["blocks.0.attn.qkv.weight"])
    out = capsys.readouterr().out
    assert "blocks.11.norm1.weight" in out and "head.weight" in out


def test_vit_path_missing_file_warns(tmp_path, capsys):
    import mvsformer_amd as m
    path = os.path.join(str(tmp_path), "nowhere.pth")
    net = m.DINOMVSNet(_args(path))
    assert "!!!No weight in %s testing should neglect this." % path in capsys.readouterr().out
    assert net.vit.pos_embed.shape == (1, 197, 384)


@pytest.mark.parametrize("kw", ["drop_rate", "attn_drop_rate", "drop_path_rate"])
def test_vit_training_refuses_dropout(kw):
    import mvsformer_amd as m
    from mvsformer_amd._lib import MvsHipError
    net = m.vit_small(patch_size=16, qk_scale="default", **{kw: 0.1}).train()
    with pytest.raises(MvsHipError, match=kw):
        net.forward_with_cls_att(torch.zeros(1, 3, 32, 32))


def test_vit_training_refuses_image_gradient():
    import mvsformer_amd as m
    from mvsformer_amd._lib import MvsHipError
    net = m.vit_small(patch_size=16, qk_scale="default").train()
    with pytest.raises(MvsHipError, match="no gradient"):
        net.forward_with_cls_att(torch.zeros(1, 3, 32, 32, requires_grad=True))


def test_vit_plain_forward_stays_eval_only():
    """The model calls only forward_with_last_att in training (mvsformer_model.py:216-220): the plain forward is not built there."""
    import mvsformer_amd as m
    from mvsformer_amd._lib import MvsHipError
    with pytest.raises(MvsHipError, match="eval only"):
        m.vit_small(patch_size=16, qk_scale="default").train()(torch.zeros(1, 3, 32, 32))
