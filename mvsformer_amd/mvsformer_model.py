"""``DINOMVSNet`` - the whole MVSFormer-P model (models/mvsformer_model.py:163-308) on the MI355X path, images -> depth map, with the reference's
constructor arguments (``configs/config_mvsformer-p.json`` ``arch.args``), sub-module names and therefore ``state_dict`` keys
(``encoder.`` / ``decoder.`` / ``vit.`` / ``decoder_vit.`` / ``fusions.<i>.``: a reference checkpoint loads with ``strict=True``) and
``forward(imgs [B,V,3,H,W], proj_matrices, depth_values, tmp)`` -> the reference's output dict.

Composition only: every piece is a HIP-backed module of this package (``FPNEncoder`` / ``FPNDecoder`` csrc/conv2d.hip + fpn.hip, the DINO
ViT-small branch csrc/vit_packed.hip, the four ``StageNet``s).  Eval mode runs the V views of all B samples as ONE batch through the 2-D
networks (the reference loops over views, mvsformer_model.py:238-271; with eval BatchNorm the results per image are the same) and hands the
feature maps to the cascade channel-last.  The constructor's variants are the reference's (mvsformer_model.py:173-176,195-201): ``multi_scale=True``
feeds the ViT into the three coarse pyramid levels (``VITDecoderStage4`` + ``FPNDecoderV2``, whose full-resolution tail is csrc/fpn_v2_tail.hip),
``att_fusion=False`` replaces the attention fusion by ``VITDecoderStage4NoAtt``; both together crash in the reference's forward and are refused
here at construction.  ``vit_arch='vit_small'`` only; Twins (``TwinMVSNet``) needs ``timm``.  ``"fix": false`` trains the ViT too (mvsformer_model.py:219), and
``vit_args['vit_path']`` loads the pretrained DINO weights (mvsformer_model.py:182-193).
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from . import _lib
from .cascade import CascadeMVS
from .fpn import FPNDecoder, FPNDecoderV2, FPNEncoder
from .vit import VITDecoderStage4, VITDecoderStage4NoAtt, VITDecoderStage4Single, vit_branch, vit_small


def _load_vit_weights(vit, path: str) -> None:
    """mvsformer_model.py:182-193: the pretrained DINO weights at ``vit_args['vit_path']`` when the file exists - a plain checkpoint (its
    ``'model'`` entry when there is one) or a trained ``model_best.pth`` (``state_dict`` with ``vit.``-prefixed keys) - loaded non-strictly
    with the missing / unexpected keys reported (utils.py torch_init_model); otherwise the reference's warning."""
    if not path or not os.path.exists(path):
        print('!!!No weight in', path, 'testing should neglect this.')
        return
    sd = torch.load(path, map_location="cpu")
    if os.path.basename(path) == "model_best.pth" and "state_dict" in sd:
        sd = {k[len("vit."):]: v for k, v in sd["state_dict"].items() if k.startswith("vit.")}
    if "model" in sd:
        sd = sd["model"]
    res = vit.load_state_dict(sd, strict=False)
    print("missing keys:{}".format(list(res.missing_keys)))
    print("unexpected keys:{}".format(list(res.unexpected_keys)))


class DINOMVSNet(CascadeMVS):
    def __init__(self, args: dict):
        super().__init__(args)                               # ndepths, depth_interals_ratio, fusions (mvsformer_model.py:166-170,203)
        a = self.args
        self.multi_scale = bool(a.get("multi_scale", False))
        va = dict(a["vit_args"])
        if va.get("vit_arch", "vit_small") != "vit_small" or va.get("twin", False):
            raise _lib.MvsHipError("DINOMVSNet: only vit_arch='vit_small' is built (configs/config_mvsformer-p.json)")
        att_fusion = bool(va.get("att_fusion", True))
        if self.multi_scale and not att_fusion:
            raise _lib.MvsHipError("DINOMVSNet: multi_scale=True with att_fusion=False is not a model: the reference builds VITDecoderStage4NoAtt, which "
                                   "returns one map, and its forward unpacks three (mvsformer_model.py:195-196,225,256)")
        self.vit_args = va
        self.encoder = FPNEncoder(feat_chs=a["feat_chs"])
        self.decoder = (FPNDecoderV2 if self.multi_scale else FPNDecoder)(feat_chs=a["feat_chs"])
        self.vit = vit_small(patch_size=va["patch_size"], qk_scale=va["qk_scale"])
        _load_vit_weights(self.vit, va.get("vit_path", ""))
        if not att_fusion:
            self.decoder_vit = VITDecoderStage4NoAtt(va)
        else:
            self.decoder_vit = (VITDecoderStage4 if self.multi_scale else VITDecoderStage4Single)(va)
        fusions = self.fusions                               # registered last, as the reference does (state_dict key ORDER too)
        del self.fusions
        self.fusions = fusions

    def train(self, mode: bool = True):
        """``"fix": true`` (MVSFormer-P): the ViT runs under ``no_grad`` in the reference (mvsformer_model.py:216-218); it has no dropout and no
        BatchNorm, so keeping it in eval mode changes nothing and lets it stay on the eval-only HIP path."""
        super().train(mode)
        if self.args.get("fix", False):
            self.vit.eval()
        return self

    def extract_features(self, imgs: torch.Tensor):
        """mvsformer_model.py:209-271 -> ``{stageK: [B,V,C,H/s,W/s]}`` (logical NCHW, channel-last memory in eval)."""
        B, V, _, H, W = imgs.shape
        x = imgs.reshape(B * V, 3, H, W)
        conv01, conv11, conv21, conv31 = self.encoder(x) if self.training else self.encoder(x, conv01_channels_last=True)
        if self.training and not self.args.get("fix", False):
            # fine-tuning the ViT (mvsformer_model.py:219): one autograd node (vit._ViTTrainFn) from the resized image to tokens + CLS attention
            vb = vit_branch(self.vit, None, x, self.vit_args["rescale"])
        else:
            with torch.no_grad():                            # the frozen ViT (mvsformer_model.py:216-218,248-250)
                vb = vit_branch(self.vit, self.decoder_vit if not self.training else None, x, self.vit_args["rescale"])
        if self.training:
            P = self.vit.patch_size
            hp, wp = int(H * self.vit_args["rescale"]) // P, int(W * self.vit_args["rescale"]) // P
            feat = vb["vit_feat"][:, 1:].reshape(B * V, hp, wp, self.vit.embed_dim).permute(0, 3, 1, 2)
            vit_out = self.decoder_vit(feat, vb["att_cls"].reshape(B * V, -1, hp, wp))
        else:
            vit_out = vb["vit_out"]
        if self.multi_scale:                                 # mvsformer_model.py:224-226,255-257: the three ViT maps join the decoder's levels
            feats = self.decoder(conv01, conv11, conv21, conv31, *vit_out)
        else:
            conv31 = conv31 + vit_out                        # mvsformer_model.py:229,263
            feats = self.decoder(conv01, conv11, conv21, conv31)
        return {"stage%d" % (i + 1): f.reshape(B, V, *f.shape[1:]) for i, f in enumerate(feats)}

    def forward(self, imgs, proj_matrices, depth_values, tmp=2.0):
        if not imgs.is_cuda:
            raise _lib.MvsHipError("DINOMVSNet: the MI355X HIP path is the only implementation (no CPU fallback)")
        if self.training:
            features = self.extract_features(imgs.to(torch.float32))
        else:
            with torch.no_grad():
                features = self.extract_features(imgs.to(torch.float32))
        return CascadeMVS.forward(self, features, proj_matrices, depth_values, tmp=tmp)
