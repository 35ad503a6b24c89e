"""The DINO ViT-small feature branch of MVSFormer-P on the MI355X path: ``vit_small`` / ``VisionTransformer`` with the
interface and the ``state_dict`` keys of the reference's ``models/vision_transformer.py`` (:340-451, ``vit_small`` :610-614) and
``VITDecoderStage4Single`` / ``AttentionFusionSimple`` of ``models/module.py`` (:353-368, :450-466), so the checkpoint of the shipped
``configs/config_mvsformer-p.json`` loads with ``strict=True``.  The ViT runs in eval mode and, for ``"fix": false``, in training mode
(``_ViTTrainFn``: one autograd node, the backward in ``csrc/vit_train.hip`` + ``mvs_gemm_x3``; DESIGN.md §8 "Fine-tuning the DINO ViT"); the
decoder also runs in training mode (batch-statistics BatchNorm, every gradient; ``_forward_train``).  In eval every
matrix product - patch embedding, QKV, attention scores, attention x V, projections, MLP, the decoder's 3x3 convolutions and transposed
convolutions as implicit GEMMs - runs in ``csrc/vit.hip`` on the bf16 matrix cores in three-term split form (fp32-equivalent), LayerNorm,
softmax and the bicubic resizes are HIP kernels too; torch only reshapes / concatenates / slices (no arithmetic beyond one broadcast
multiply and one mean over 6 heads).  ``mvsformer_amd.install(features=True)`` rebinds ``models.vision_transformer.vit_small`` and
``VITDecoderStage4Single``, and the decoders of the ``multi_scale`` / ``att_fusion: false`` variants: ``VITDecoderStage4`` (:305-350) and
``VITDecoderStage4NoAtt`` (:371-386).  Twins (``models/gvt.py``) needs ``timm`` and is not built.
"""
from __future__ import annotations

import math
from functools import partial
from typing import Optional

import torch
import torch.nn as nn

from . import _lib, ops, switches as sw
from .module import _publish_cache, _versions


def _f(t):
    return t.detach().to(torch.float32).contiguous()


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, qkv_bias, norm_layer):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads, qkv_bias)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class PatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.patch_size = patch_size
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


class VisionTransformer(nn.Module):
    """models/vision_transformer.py:340-451 (``cross_att=False``, ``qk_scale='default'``: what the shipped configs build)."""

    def __init__(self, img_size=(224,), patch_size=16, in_chans=3, num_classes=0, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0,
                 qkv_bias=False, qk_scale="default", norm_layer=nn.LayerNorm, **kwargs):
        super().__init__()
        if qk_scale != "default" or kwargs.get("cross_att", False) or num_classes:
            raise _lib.MvsHipError("VisionTransformer: only qk_scale='default', no cross attention, no classifier head is built (the shipped configs)")
        self.embed_dim, self.num_heads, self.patch_size = embed_dim, num_heads, patch_size
        self.patch_embed = PatchEmbed(img_size[0], patch_size, in_chans, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.patch_embed.num_patches + 1, embed_dim))
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias, norm_layer) for _ in range(depth)])
        self.norm = norm_layer(embed_dim)
        self._drop = tuple(float(kwargs.get(k, 0.0)) for k in ("drop_rate", "attn_drop_rate", "drop_path_rate"))
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        self._cache = None
        self._pos_cache = {}

    # ---- position table resized to the token grid (vision_transformer.py:394-416; prepare_tokens passes (h, w) as (w, h)) ----
    def _pos(self, hp: int, wp: int) -> torch.Tensor:
        # the weights epoch too: an optimizer step through raw pointers (FusedAdamW) does not move pos_embed._version
        key = (ops.weights_epoch(), self.pos_embed.data_ptr(), self.pos_embed._version, hp, wp)
        if self._pos_cache.get("key") != key:
            pe = _f(self.pos_embed)
            N = pe.shape[1] - 1
            n = int(math.sqrt(N))
            if hp * wp == N and hp == wp:
                pos = pe
            else:
                grid = pe[0, 1:].reshape(n, n, self.embed_dim).permute(2, 0, 1).contiguous()              # [C, n, n]
                sh, sw = (hp + 0.1) / n, (wp + 0.1) / n                                                  # the reference's scale factors
                if int(n * sh) != hp or int(n * sw) != wp:
                    raise _lib.MvsHipError("position table resize: %dx%d does not come out of scale factors %.4f, %.4f" % (hp, wp, sh, sw))
                grid = ops.bicubic_resize(grid, hp, wp, 1.0 / sh, 1.0 / sw)
                pos = torch.cat([pe[:, :1], grid.permute(1, 2, 0).reshape(1, hp * wp, self.embed_dim)], dim=1).contiguous()
            _publish_cache()
            self._pos_cache = {"key": key, "pos": pos}
        return self._pos_cache["pos"]

    def _prepared(self):
        packed_ok = self._packed_ok()
        key = (_versions(self), packed_ok)                   # MVS_VIT_PACKED as the operands were packed under it
        if self._cache is None or self._cache[0] != key:
            pw = _f(self.patch_embed.proj.weight).reshape(self.embed_dim, -1)
            blocks = []
            for b in self.blocks:
                blocks.append(tuple(_f(t) for t in (b.norm1.weight, b.norm1.bias, b.attn.qkv.weight, b.attn.qkv.bias, b.attn.proj.weight,
                                                    b.attn.proj.bias, b.norm2.weight, b.norm2.bias, b.mlp.fc1.weight, b.mlp.fc1.bias,
                                                    b.mlp.fc2.weight, b.mlp.fc2.bias)))
            # the linear layers' weights split once into (h, m, l) bf16 MFMA fragments (csrc/vit_packed.hip): no block of any GEMM splits them again
            packed = None
            if packed_ok:
                packed = [tuple(ops.x3p_pack(w) for w in (b[2], b[4], b[8], b[10])) for b in blocks]
            _publish_cache()
            self._cache = (key, pw, _f(self.patch_embed.proj.bias), blocks, _f(self.norm.weight), _f(self.norm.bias), _f(self.cls_token), packed)
        return self._cache[1:]

    def _packed_ok(self) -> bool:
        """The pre-split path (csrc/vit_packed.hip) covers heads of 64 with C a multiple of 128 up to 512 (ViT-small)."""
        C, NH = self.embed_dim, self.num_heads
        return C == NH * 64 and C % 128 == 0 and C <= 512 and sw.flag("MVS_VIT_PACKED")

    def _run_packed(self, x: torch.Tensor, want_cls: bool, prep):
        """The 12 blocks on pre-split operands: LayerNorm -> packed, qkv GEMM -> packed Q / K / V^T per head, flash attention -> packed,
        projection (+ residual) -> fp32 tokens, LayerNorm -> packed, fc1 (+ GELU) -> packed, fc2 (+ residual) -> fp32 tokens.  Token rows are
        laid out [B][Np] with Np = N rounded up to 32 (padding rows stay finite and are masked as keys).  ``want_cls``: also the CLS query's
        attention row of the last block, ``[B, heads, N]`` - the only part of the attention matrix the model reads (mvsformer_model.py:257)."""
        pw, pb, blocks, nw, nb, cls, packed = prep
        x = x.detach().to(torch.float32)
        B, nc, h, w = x.shape
        P, C, NH = self.patch_size, self.embed_dim, self.num_heads
        hp, wp = h // P, w // P
        n = hp * wp
        N = n + 1
        Np = (N + 31) // 32 * 32
        M = B * Np
        dev = x.device
        patches = x[:, :, :hp * P, :wp * P].reshape(B, nc, hp, P, wp, P).permute(0, 2, 4, 1, 3, 5).reshape(B * n, nc * P * P).contiguous()
        tok = torch.zeros(B, Np, C, device=dev, dtype=torch.float32)
        tok[:, 0] = cls[0, 0]
        ops.gemm_x3(patches, pw, tok, n, C, nc * P * P, nc * P * P, nc * P * P, C, nb1=B, sA=(n * nc * P * P, 0), sC=(Np * C, 0), shift=pb, c_off=C)
        tok[:, :N] += self._pos(hp, wp)
        t, t2 = tok.view(M, C), torch.empty(M, C, device=dev, dtype=torch.float32)
        hidden = blocks[0][8].shape[0]
        y_p, a_p, h_p = ops.Packed(M, C, dev), ops.Packed(M, C, dev), ops.Packed(M, hidden, dev)
        qkv_p = ops.QkvPacked(B, NH, Np, dev)
        eps = self.norm.eps
        att_cls = None
        for i, ((n1w, n1b, _, qb, _, prb, n2w, n2b, _, f1b, _, f2b), (wq, wpr, w1, w2)) in enumerate(zip(blocks, packed)):
            ops.layernorm_x3p(t, n1w, n1b, eps, Np, N, out=y_p)
            ops.gemm_x3p_qkv(y_p, wq, qb, B, Np, NH, (C // NH) ** -0.5, out=qkv_p)
            if want_cls and i == len(blocks) - 1:
                att_cls = ops.cls_attention_x3p(qkv_p, N)
            ops.attention_x3p(qkv_p, N, out=a_p)
            ops.gemm_x3p(a_p, wpr, C, C=t2, shift=prb, res=t)
            ops.layernorm_x3p(t2, n2w, n2b, eps, Np, N, out=y_p)
            ops.gemm_x3p(y_p, w1, hidden, shift=f1b, act=1, out=h_p)
            ops.gemm_x3p(h_p, w2, C, C=t, shift=f2b, res=t2)
        out = ops.layernorm(tok, nw, nb, eps)[:, :N].contiguous()
        return (out, att_cls) if want_cls else out

    def _run(self, x: torch.Tensor, want_att):
        """``want_att``: False, True (the last block's whole attention matrix, ``forward_with_last_att``'s contract) or ``"cls"`` (only the CLS
        query's row ``[B, heads, N]``: what ``vit_branch`` needs)."""
        if self.training:
            if not want_att:
                raise _lib.MvsHipError("VisionTransformer.forward: training mode is built for forward_with_last_att / forward_with_cls_att, what "
                                       "DINOMVSNet calls (mvsformer_model.py:216-220); the plain forward is eval only")
            return self._run_train(x, want_att)
        prep = self._prepared()
        if want_att is not True and prep[6] is not None:     # the pre-split operands exist: MVS_VIT_PACKED and a ViT they are built for
            return self._run_packed(x, want_att == "cls", prep)
        pw, pb, blocks, nw, nb, cls = prep[:6]
        x = x.detach().to(torch.float32)
        B, nc, h, w = x.shape
        P, C, NH = self.patch_size, self.embed_dim, self.num_heads
        hp, wp = h // P, w // P
        n = hp * wp
        N = n + 1
        hd = C // NH
        # patch embedding = GEMM over non-overlapping patches: [B*n, nc*P*P] x [C, nc*P*P]^T
        patches = x[:, :, :hp * P, :wp * P].reshape(B, nc, hp, P, wp, P).permute(0, 2, 4, 1, 3, 5).reshape(B * n, nc * P * P).contiguous()
        tok = torch.empty(B, N, C, device=x.device, dtype=torch.float32)
        tok[:, 0] = cls[0, 0]
        ops.gemm_x3(patches, pw, tok, n, C, nc * P * P, nc * P * P, nc * P * P, C, nb1=B, sA=(n * nc * P * P, 0), sC=(N * C, 0), shift=pb, c_off=C)
        t = (tok + self._pos(hp, wp)).contiguous()
        eps = self.norm.eps
        scores, vt_pad = None, None
        for i, (n1w, n1b, qw, qb, prw, prb, n2w, n2b, f1w, f1b, f2w, f2b) in enumerate(blocks):
            y = ops.layernorm(t, n1w, n1b, eps)
            qkv = torch.empty(B, N, 3 * C, device=x.device, dtype=torch.float32)
            ops.gemm_x3(y, qw, qkv, B * N, 3 * C, C, C, C, 3 * C, shift=qb)
            last = want_att and i == len(blocks) - 1
            if hd == 64 and not last and sw.flag("MVS_VIT_FLASH"):
                # flash form: softmax(Q K^T / sqrt(hd)) V without the N x N matrix (csrc/vit.hip attention_x3_kernel); V handed over
                # TRANSPOSED with 16-byte aligned rows ([B, heads, hd, N rounded up to 4], one strided copy into a buffer reused by all blocks)
                vt_pad = ops.attention_vt(qkv, NH, vt_pad)
                att_out = ops.attention_x3(qkv, vt_pad, NH, hd ** -0.5)
            else:
                # materialized form (the LAST block's attention matrix is an output: mvsformer_model.py:257 reads its CLS row): scores[b, h] =
                # Q . K^T (head slices of the packed qkv rows), softmax(scale * .), out[b, :, h] = P . V
                vt = qkv[:, :, 2 * C:].reshape(B, N, NH, hd).permute(0, 2, 3, 1).contiguous()     # the GEMM's B operand, read along K
                if scores is None:
                    scores = torch.empty(B, NH, N, N, device=x.device, dtype=torch.float32)
                ops.gemm_x3(qkv, qkv, scores, N, N, hd, 3 * C, 3 * C, N, nb1=B, nb2=NH, sA=(N * 3 * C, hd), sB=(N * 3 * C, hd), sC=(NH * N * N, N * N),
                            b_off=C)
                ops.softmax_rows_(scores, hd ** -0.5)
                att_out = torch.empty(B, N, C, device=x.device, dtype=torch.float32)
                ops.gemm_x3(scores, vt, att_out, N, hd, N, N, N, C, nb1=B, nb2=NH, sA=(NH * N * N, N * N), sB=(NH * hd * N, hd * N), sC=(N * C, hd))
            t2 = torch.empty_like(t)
            ops.gemm_x3(att_out, prw, t2, B * N, C, C, C, C, C, shift=prb, res=t)
            y = ops.layernorm(t2, n2w, n2b, eps)
            hid = torch.empty(B, N, f1w.shape[0], device=x.device, dtype=torch.float32)
            ops.gemm_x3(y, f1w, hid, B * N, f1w.shape[0], C, C, C, f1w.shape[0], shift=f1b, act=1)
            ops.gemm_x3(hid, f2w, t, B * N, C, f1w.shape[0], f1w.shape[0], f1w.shape[0], C, shift=f2b, res=t2)
        out = ops.layernorm(t, nw, nb, eps)
        if want_att == "cls":
            return out, scores[:, :, 0].contiguous()
        return (out, scores) if want_att else out

    def _train_params(self):
        """Every parameter in the order ``_ViTTrainFn`` takes them."""
        ps = [self.patch_embed.proj.weight, self.patch_embed.proj.bias, self.cls_token, self.pos_embed]
        for b in self.blocks:
            ps += [b.norm1.weight, b.norm1.bias, b.attn.qkv.weight, b.attn.qkv.bias, b.attn.proj.weight, b.attn.proj.bias, b.norm2.weight,
                   b.norm2.bias, b.mlp.fc1.weight, b.mlp.fc1.bias, b.mlp.fc2.weight, b.mlp.fc2.bias]
        return ps + [self.norm.weight, self.norm.bias]

    def _run_train(self, x: torch.Tensor, want_att):
        """Training mode (``"fix": false``, mvsformer_model.py:216-219): the whole ViT is ONE autograd node (``_ViTTrainFn``) whose forward
        keeps each block's activations and whose backward produces the gradient of every parameter.  Under bf16 autocast it stays
        fp32-equivalent: every matrix product is ``mvs_gemm_x3`` in split form on fp32 operands.  The image gets no gradient."""
        if any(self._drop):
            raise _lib.MvsHipError("VisionTransformer: training with drop_rate / attn_drop_rate / drop_path_rate %r is not built (vit_small uses 0)"
                                   % (self._drop,))
        if self.embed_dim // self.num_heads * self.num_heads != self.embed_dim or self.embed_dim > 1024:
            raise _lib.MvsHipError("VisionTransformer: training needs embed_dim <= 1024 divisible by the heads")
        if x.requires_grad:
            raise _lib.MvsHipError("VisionTransformer: training mode gives the image no gradient; pass it detached")
        return _ViTTrainFn.apply(self, want_att == "cls", x.detach().to(torch.float32).contiguous(), *self._train_params())

    def forward(self, x, src_epipoles=None):
        return self._run(x, False)

    def forward_with_last_att(self, x):
        """-> (tokens after the final LayerNorm ``[B, 1+hw, C]``, attention of the last block ``[B, heads, 1+hw, 1+hw]``)."""
        return self._run(x, True)

    def forward_with_cls_att(self, x):
        """-> (tokens ``[B, 1+hw, C]``, the CLS query's attention row of the last block ``[B, heads, 1+hw]``) = what mvsformer_model.py:246-257
        uses of ``forward_with_last_att`` (``vit_att[:, :, 0, 1:]``) without writing the other 1+hw rows."""
        return self._run(x, "cls")


def _pos_resize(vit: VisionTransformer, hp: int, wp: int):
    """The position table's resize as ``VisionTransformer._pos`` does it -> (n, rscale_h, rscale_w) or None when the table is used as is."""
    N = vit.pos_embed.shape[1] - 1
    n = int(math.sqrt(N))
    if hp * wp == N and hp == wp:
        return None
    sh, sw = (hp + 0.1) / n, (wp + 0.1) / n
    if int(n * sh) != hp or int(n * sw) != wp:
        raise _lib.MvsHipError("position table resize: %dx%d does not come out of scale factors %.4f, %.4f" % (hp, wp, sh, sw))
    return n, 1.0 / sh, 1.0 / sw


def attention_train_fwd(qkv: torch.Tensor, heads: int):
    """Attention (vision_transformer.py:139-150) of packed ``qkv [B,N,3C]`` in materialized form -> (P = softmax(Q K^T / sqrt(hd))
    ``[B,heads,N,N]``, P V ``[B,N,C]``): what the backward reads."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    p = torch.empty(B, heads, N, N, device=qkv.device, dtype=torch.float32)
    ops.gemm_x3(qkv, qkv, p, N, N, hd, C3, C3, N, nb1=B, nb2=heads, sA=(N * C3, hd), sB=(N * C3, hd), sC=(heads * N * N, N * N), b_off=C)
    ops.softmax_rows_(p, hd ** -0.5)
    out = torch.empty(B, N, C, device=qkv.device, dtype=torch.float32)
    ops.gemm_x3(p, qkv, out, N, hd, N, N, C3, C, nb1=B, nb2=heads, sA=(heads * N * N, N * N), sB=(N * C3, hd), sC=(N * C, hd), b_kn=True, b_off=2 * C)
    return p, out


def attention_train_bwd(qkv: torch.Tensor, p: torch.Tensor, dout: torch.Tensor, heads: int, da: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of :func:`attention_train_fwd` -> dqkv ``[B,N,3C]``: dP = dO V^T, dS = ``mvs_attention_softmax_bwd`` (with ``da``, the
    gradient of P itself: ``[B,heads,N,N]`` or its CLS row ``[B,heads,N]``; the softmax scale is inside dS), dQ = dS K, dK = dS^T Q (A
    transposed), dV = P^T dO (A transposed), each written into its third of dqkv."""
    B, N, C3 = qkv.shape
    C = C3 // 3
    hd = C // heads
    dev = qkv.device
    dp = torch.empty(B, heads, N, N, device=dev, dtype=torch.float32)
    sS, sQ = (heads * N * N, N * N), (N * C3, hd)
    ops.gemm_x3(dout, qkv, dp, N, N, hd, C, C3, N, nb1=B, nb2=heads, sA=(N * C, hd), sB=sQ, sC=sS, b_off=2 * C)
    ds = ops.attention_softmax_bwd(p, dp, hd ** -0.5, da)
    del dp
    dqkv = torch.empty(B, N, C3, device=dev, dtype=torch.float32)
    ops.gemm_x3(ds, qkv, dqkv, N, hd, N, N, C3, C3, nb1=B, nb2=heads, sA=sS, sB=sQ, sC=sQ, b_kn=True, b_off=C)
    ops.gemm_x3(ds, qkv, dqkv, N, hd, N, N, C3, C3, nb1=B, nb2=heads, sA=sS, sB=sQ, sC=sQ, b_kn=True, a_mode=3, c_off=C)
    ops.gemm_x3(p, dout, dqkv, N, hd, N, N, C, C3, nb1=B, nb2=heads, sA=sS, sB=(N * C, hd), sC=sQ, b_kn=True, a_mode=3, c_off=2 * C)
    return dqkv


def attention_flash_train_fwd(qkv: torch.Tensor, heads: int, want_cls: bool = False):
    """Attention of packed ``qkv [B,N,3C]`` in flash form (``mvs_attention_train_fwd_flash``, head dimension 64) -> (P V ``[B,N,C]``,
    ``lse [B,heads,N]`` = log sum_k exp(q . k_k / sqrt(hd))) and, with ``want_cls``, the CLS query's row of P ``[B,heads,N]``.  No N x N tensor."""
    return ops.attention_train_fwd_flash(qkv, heads, (qkv.shape[-1] // 3 // heads) ** -0.5, want_cls)


def attention_flash_train_bwd(qkv: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, dout: torch.Tensor, heads: int,
                              da_cls: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The backward of :func:`attention_flash_train_fwd` -> dqkv ``[B,N,3C]`` (``mvs_attention_train_bwd_flash``): P and dP are recomputed
    tile by tile from ``lse``, dS as in ``mvs_attention_softmax_bwd``; ``da_cls [B,heads,N]`` = the gradient of the returned CLS row.
    Deterministic: two runs are bitwise equal."""
    return ops.attention_train_bwd_flash(qkv, out, lse, dout, heads, (qkv.shape[-1] // 3 // heads) ** -0.5, da_cls)


def _train_flash_on() -> bool:
    return sw.flag("MVS_VIT_TRAIN_FLASH")


class _ViTTrainFn(torch.autograd.Function):
    """``VisionTransformer.forward_with_last_att`` / ``forward_with_cls_att`` in training mode and its backward
    (models/vision_transformer.py:104-154,194-214,394-451).

    Forward: ``mvs_gemm_x3`` for every linear layer, LayerNorm writing its row statistics (``mvs_layernorm_stats``), fc1's pre-activation kept
    for GELU's backward.  Attention with heads of 64 is the flash pair of csrc/vit_flash_train.hip (:func:`attention_flash_train_fwd` /
    ``_bwd``): a block keeps the row log-sum-exp ``[B,heads,N]`` and no N x N tensor; with ``cls_only`` the returned CLS row comes from the last
    block's forward.  The materialized form (:func:`attention_train_fwd`, P saved) remains for the last block when the WHOLE matrix is
    returned, for other head sizes, and for every block under ``MVS_VIT_TRAIN_FLASH=0``.  Saved per block: the block input, both
    LayerNorm outputs and statistics, qkv, lse (or P), the attention output, the mid-block tokens, fc1 before and after GELU.
    Backward, per block in reverse: linear data gradients = ``mvs_gemm_x3`` with ``b_kn = 1``, weight gradients dW = dY^T X with ``a_mode = 3``,
    bias / LayerNorm parameter gradients = ``mvs_colsum`` (fixed-order column sums), the attention backward dP = dO V^T, dS =
    ``mvs_attention_softmax_bwd`` (which folds in the gradient of the returned attention: all rows, or the CLS row only), dQ = dS K,
    dK = dS^T Q, dV = P^T dO written into one dqkv (flash blocks: the same quantities recomputed tile by tile).  The position table's gradient goes through ``mvs_bicubic_resize_bwd``.  No atomics: two
    runs give bitwise-equal gradients.

    ``cls_only``: return the last block's CLS query row ``[B, heads, N]`` instead of its whole attention matrix."""

    @staticmethod
    def forward(ctx, vit, cls_only, x, *params):
        f = [p.detach().to(torch.float32).contiguous() for p in params]
        pw, pb, cls, pe = f[0].reshape(f[0].shape[0], -1), f[1], f[2], f[3]
        blocks = [f[4 + 12 * i:16 + 12 * i] for i in range(len(vit.blocks))]
        nw, nb = f[-2], f[-1]
        B, nc, h, w = x.shape
        P, C, NH = vit.patch_size, vit.embed_dim, vit.num_heads
        hd = C // NH
        hp, wp = h // P, w // P
        n = hp * wp
        N, M, K0 = n + 1, B * (hp * wp + 1), nc * P * P
        scale = hd ** -0.5
        eps = vit.norm.eps
        dev = x.device
        patches = x[:, :, :hp * P, :wp * P].reshape(B, nc, hp, P, wp, P).permute(0, 2, 4, 1, 3, 5).reshape(B * n, K0).contiguous()
        tok = torch.empty(B, N, C, device=dev, dtype=torch.float32)
        tok[:, 0] = cls[0, 0]
        ops.gemm_x3(patches, pw, tok, n, C, K0, K0, K0, C, nb1=B, sA=(n * K0, 0), sC=(N * C, 0), shift=pb, c_off=C)
        rs = _pos_resize(vit, hp, wp)
        if rs is None:
            pos = pe
        else:
            nn_, rh, rw = rs
            grid = pe[0, 1:].reshape(nn_, nn_, C).permute(2, 0, 1).contiguous()
            grid = ops.bicubic_resize(grid, hp, wp, rh, rw)
            pos = torch.cat([pe[:, :1], grid.permute(1, 2, 0).reshape(1, n, C)], dim=1)
        t = (tok + pos).contiguous()
        saved, is_flash, att_out = [], [], None
        flash = hd == 64 and _train_flash_on()                # (hd != 64: the materialized form, as in eval)
        for (n1w, n1b, qw, qb, prw, prb, n2w, n2b, f1w, f1b, f2w, f2b) in blocks:
            hid = f1w.shape[0]
            y1, m1, r1 = ops.layernorm_stats(t, n1w, n1b, eps)
            qkv = torch.empty(B, N, 3 * C, device=dev, dtype=torch.float32)
            ops.gemm_x3(y1, qw, qkv, M, 3 * C, C, C, C, 3 * C, shift=qb)
            last = len(saved) == len(blocks) - 1
            if flash and not (last and not cls_only):
                # flash form: the block keeps lse [B,heads,N] instead of P [B,heads,N,N]; the last block also gives the CLS row
                if last:
                    att, p_att, att_out = attention_flash_train_fwd(qkv, NH, want_cls=True)
                else:
                    att, p_att = attention_flash_train_fwd(qkv, NH)
                is_flash.append(True)
            else:
                p_att, att = attention_train_fwd(qkv, NH)
                is_flash.append(False)
            t2 = torch.empty_like(t)
            ops.gemm_x3(att, prw, t2, M, C, C, C, C, C, shift=prb, res=t)
            y2, m2, r2 = ops.layernorm_stats(t2, n2w, n2b, eps)
            hpre = torch.empty(B, N, hid, device=dev, dtype=torch.float32)
            ops.gemm_x3(y2, f1w, hpre, M, hid, C, C, C, hid, shift=f1b)
            hact = ops.gelu(hpre)
            tn = torch.empty_like(t)
            ops.gemm_x3(hact, f2w, tn, M, C, hid, hid, hid, C, shift=f2b, res=t2)
            saved.append((t, y1, m1, r1, qkv, p_att, att, t2, y2, m2, r2, hpre, hact))
            t = tn
        out, mf, rf = ops.layernorm_stats(t, nw, nb, eps)
        if att_out is None:
            last = saved[-1][5]
            att_out = last[:, :, 0].contiguous() if cls_only else last.clone()
        ctx.cfg = ( B, N, C, NH, hd, n, hp, wp, K0, scale, rs, [tuple(p.shape) for p in params])
        ctx.is_flash = is_flash
        ctx.state = (f, patches, saved, t, mf, rf)
        return out, att_out

    @staticmethod
    def backward(ctx, dout, datt):
        B, N, C, NH, hd, n, hp, wp, K0, scale, rs, shapes = ctx.cfg
        f, patches, saved, t_last, mf, rf = ctx.state
        dev = dout.device
        M = B * N
        blocks = [f[4 + 12 * i:16 + 12 * i] for i in range(len(saved))]
        dout = dout.to(torch.float32).contiguous()
        da = datt.to(torch.float32).contiguous()
        gn = ops.colsum(dout, t_last, mf, rf)
        dt = ops.layernorm_bwd(dout, t_last, mf, rf, f[-2])
        block_grads = []
        for i in reversed(range(len(saved))):
            n1w, n1b, qw, qb, prw, prb, n2w, n2b, f1w, f1b, f2w, f2b = blocks[i]
            t, y1, m1, r1, qkv, p_att, att, t2, y2, m2, r2, hpre, hact = saved[i]
            hid = f1w.shape[0]
            # mlp.fc2 (+ the residual: dt flows on to t2 unchanged)
            dh = torch.empty(B, N, hid, device=dev, dtype=torch.float32)
            ops.gemm_x3(dt, f2w, dh, M, hid, C, C, hid, hid, b_kn=True)
            dw2 = torch.empty(C, hid, device=dev, dtype=torch.float32)
            ops.gemm_x3(dt, hact, dw2, C, hid, M, C, hid, hid, b_kn=True, a_mode=3)
            db2 = ops.colsum(dt)
            # GELU, mlp.fc1
            dhp = ops.gelu_bwd(dh, hpre)
            dy2 = torch.empty(B, N, C, device=dev, dtype=torch.float32)
            ops.gemm_x3(dhp, f1w, dy2, M, C, hid, hid, C, C, b_kn=True)
            dw1 = torch.empty(hid, C, device=dev, dtype=torch.float32)
            ops.gemm_x3(dhp, y2, dw1, hid, C, M, hid, C, C, b_kn=True, a_mode=3)
            db1 = ops.colsum(dhp)
            # norm2 (+ residual)
            g2 = ops.colsum(dy2, t2, m2, r2)
            dt2 = ops.layernorm_bwd(dy2, t2, m2, r2, n2w, res=dt)
            # attn.proj
            datt_o = torch.empty(B, N, C, device=dev, dtype=torch.float32)
            ops.gemm_x3(dt2, prw, datt_o, M, C, C, C, C, C, b_kn=True)
            dwp = torch.empty(C, C, device=dev, dtype=torch.float32)
            ops.gemm_x3(dt2, att, dwp, C, C, M, C, C, C, b_kn=True, a_mode=3)
            dbp = ops.colsum(dt2)
            da_i = da if i == len(saved) - 1 else None
            if ctx.is_flash[i]:                              # p_att holds lse
                dqkv = attention_flash_train_bwd(qkv, att, p_att, datt_o, NH, da_i)
            else:
                dqkv = attention_train_bwd(qkv, p_att, datt_o, NH, da_i)
            # attn.qkv
            dy1 = torch.empty(B, N, C, device=dev, dtype=torch.float32)
            ops.gemm_x3(dqkv, qw, dy1, M, C, 3 * C, 3 * C, C, C, b_kn=True)
            dwq = torch.empty(3 * C, C, device=dev, dtype=torch.float32)
            ops.gemm_x3(dqkv, y1, dwq, 3 * C, C, M, 3 * C, C, C, b_kn=True, a_mode=3)
            dbq = ops.colsum(dqkv)
            # norm1 (+ residual)
            g1 = ops.colsum(dy1, t, m1, r1)
            dt = ops.layernorm_bwd(dy1, t, m1, r1, n1w, res=dt2)
            block_grads.append((g1[:C], g1[C:], dwq, dbq, dwp, dbp, g2[:C], g2[C:], dw1, db1, dw2, db2))
        # tokens = [cls | patch embedding] + position table
        dpos = ops.colsum(dt, cols=N * C).view(N, C)
        if rs is None:
            dpe = dpos.view(1, N, C)
        else:
            nn_, rh, rw = rs
            dgrid = ops.bicubic_resize_bwd(dpos[1:].reshape(hp, wp, C).permute(2, 0, 1).contiguous(), nn_, nn_, rh, rw)
            dpe = torch.cat([dpos[:1], dgrid.permute(1, 2, 0).reshape(nn_ * nn_, C)], dim=0).view(1, nn_ * nn_ + 1, C)
        dcls = dpos[:1].reshape(1, 1, C).clone()
        dpatch = dt[:, 1:].reshape(B * n, C).contiguous()
        dwpe = torch.empty(C, K0, device=dev, dtype=torch.float32)
        ops.gemm_x3(dpatch, patches, dwpe, C, K0, B * n, C, K0, K0, b_kn=True, a_mode=3)
        dbpe = ops.colsum(dpatch)
        grads = [dwpe, dbpe, dcls, dpe]
        for g in reversed(block_grads):
            grads += list(g)
        grads += [gn[:C], gn[C:]]
        grads = [g.reshape(s) for g, s in zip(grads, shapes)]
        return (None, None, None) + tuple(grads)


def vit_small(patch_size=16, **kwargs):
    return VisionTransformer(patch_size=patch_size, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, qkv_bias=True,
                             norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)


class _Act(nn.Module):
    """Parameterless placeholder keeping ``nn.Sequential`` indices (and therefore checkpoint keys) as in the reference."""

    def forward(self, x):
        raise _lib.MvsHipError("structural placeholder: the activation runs in the GEMM epilogue")


class AttentionFusionSimple(nn.Module):
    def __init__(self, vit_ch, out_ch, nhead):
        super().__init__()
        self.conv_l = nn.Sequential(nn.Conv2d(vit_ch + nhead, vit_ch, kernel_size=3, padding=1), nn.BatchNorm2d(vit_ch))
        self.conv_r = nn.Sequential(nn.Conv2d(vit_ch, vit_ch, kernel_size=3, padding=1), nn.BatchNorm2d(vit_ch))
        self.act = _Act()
        self.proj = nn.Conv2d(vit_ch, out_ch, kernel_size=1)


def _fold(conv, bn):
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
    shift = bn.bias.detach().double() + (conv.bias.detach().double() - bn.running_mean.double()) * scale
    return scale.float().contiguous(), shift.float().contiguous()


def _conv3_matrix(w: torch.Tensor, cp: int) -> torch.Tensor:
    """``[Cout,Cin,3,3]`` -> ``[Cout, 9*cp]`` with k = tap*cp + c (channels zero-padded to ``cp``)."""
    cout, cin = w.shape[:2]
    m = torch.zeros(cout, 9, cp, device=w.device, dtype=torch.float32)
    m[:, :, :cin] = _f(w).permute(0, 2, 3, 1).reshape(cout, 9, cin)
    return m.reshape(cout, 9 * cp).contiguous()


def _convT_matrices(w: torch.Tensor) -> torch.Tensor:
    """ConvTranspose2d(k 4, s 2, p 1) weight ``[Cin,Cout,4,4]`` -> ``[4 classes, Cout, 4*Cin]``: class (ph, pw) = output parity, its 2x2 taps
    (th, tw) use ky = (1, 3) for ph = 0 and (0, 2) for ph = 1 (input rows y, y-1 and y+1, y), kx likewise; k = (th*2 + tw)*Cin + c."""
    cin, cout = w.shape[:2]
    wf = _f(w)
    ks = ((1, 3), (0, 2))
    out = torch.empty(4, cout, 4, cin, device=w.device, dtype=torch.float32)
    for ph in range(2):
        for pw in range(2):
            for th in range(2):
                for tw in range(2):
                    out[ph * 2 + pw, :, th * 2 + tw] = wf[:, :, ks[ph][th], ks[pw][tw]].t()
    return out.reshape(4, cout, 4 * cin).contiguous()


class ConvT2dFn(torch.autograd.Function):
    """Raw ``ConvTranspose2d`` (weight ``[Cin,Cout,KS,KS]``, no bias) in training, fp32 NCHW: the transposed convolution IS the data gradient of
    the convolution with the same weight read as ``[Cout_conv = Cin][Cin_conv = Cout]`` - forward = ``mvs_conv2d_gemm_x3`` mode 2, data
    gradient = mode 1, weight gradient = mode 3 with ``x`` in the role of the convolution's output gradient."""

    @staticmethod
    def forward(ctx, x, weight, stride, pad):
        x = x.to(torch.float32).contiguous()
        w = weight.detach().to(torch.float32).contiguous()
        ctx.save_for_backward(x, w)
        ctx.cfg = (int(stride), int(pad))
        KS = w.shape[2]
        Ho, Wo = (x.shape[2] - 1) * stride - 2 * pad + KS, (x.shape[3] - 1) * stride - 2 * pad + KS
        return ops.conv2d_dgrad_x3(x, w, int(stride), int(pad), Ho, Wo)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad = ctx.cfg
        dy = dy.contiguous()
        dx = ops.conv2d_fwd_x3(dy, w, stride, pad) if ctx.needs_input_grad[0] else None
        dw = ops.conv2d_wgrad_x3(x, dy, w.shape[2], stride, pad) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None


class MulFn(torch.autograd.Function):
    """``a * b`` (models/module.py:464) with both gradients through ``mvs_ewise_mul``."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        return ops.ewise_mul(a, b)

    @staticmethod
    def backward(ctx, dy):
        a, b = ctx.saved_tensors
        dy = dy.contiguous()
        return (ops.ewise_mul(dy, b) if ctx.needs_input_grad[0] else None), (ops.ewise_mul(dy, a) if ctx.needs_input_grad[1] else None)


ACT_GELU_BN = 4                          # GELU(erf) in the fp32 BatchNorm kernels (csrc/train.hip); 3 = Swish


def _fold_up(conv, bn):
    """(scale, shift) of a transposed convolution's epilogue: its bias, through the BatchNorm ``bn`` where one follows (None: the raw output)."""
    if bn is not None:
        return _fold(conv, bn)
    return torch.ones_like(conv.bias, dtype=torch.float32).contiguous(), _f(conv.bias)


class _DecoderBase(nn.Module):
    """What the ViT decoders of models/module.py:305-386 share on the HIP path: ``AttentionFusionSimple`` (:450-466) and chains of
    ``ConvTranspose2d(4, 2, 1)`` (+ BatchNorm + GELU), in eval as implicit GEMMs - on pre-split operands (``mvs_conv_x3p``) where the channel
    counts allow it, ``_up`` (``mvs_gemm_x3``) otherwise - and in training as autograd-tracked HIP ops."""

    def _ups(self):
        """The transposed convolutions of the module: ``[(name, conv, bn or None)]``, ``bn`` = the BatchNorm whose (+ GELU's) output the NEXT layer
        of that chain reads - folded into the epilogue of the layer's run that feeds it."""
        raise NotImplementedError

    def _mid_channels(self):
        """Channel counts of every map a transposed convolution READS (packed K) and of the fp32 outputs."""
        reads = [conv.in_channels for _, conv, _ in self._ups()]
        return reads, [conv.out_channels for _, conv, _ in self._ups()]

    def _packed_ok(self) -> bool:
        reads, outs = self._mid_channels()
        a = getattr(self, "attn", None)
        chans = list(reads) + ([a.conv_r[0].in_channels, a.proj.out_channels] if a is not None else [])
        return all(c % 32 == 0 for c in chans) and all(c % 4 == 0 for c in outs) and sw.flag("MVS_VIT_PACKED")

    def _prepared(self):
        packed = self._packed_ok()
        key = (_versions(self), packed)                      # MVS_VIT_PACKED as the operands were packed under it
        if self._cache is None or self._cache[0] != key:
            prep = dict(packed=packed)
            a = getattr(self, "attn", None)
            if a is not None:
                cl_in = a.conv_l[0].in_channels
                cp = (cl_in + 7) // 8 * 8
                prep.update(cp=cp, wl=_conv3_matrix(a.conv_l[0].weight, cp), fl=_fold(a.conv_l[0], a.conv_l[1]),
                            wr=_conv3_matrix(a.conv_r[0].weight, a.conv_r[0].in_channels), fr=_fold(a.conv_r[0], a.conv_r[1]),
                            wp=_f(a.proj.weight).reshape(a.proj.out_channels, -1), bp=_f(a.proj.bias))
                if packed:
                    # the same matrices split once into MFMA fragments (csrc/vit_packed.hip; channels of the [x | att] map padded to a multiple of 32)
                    cpp = (cl_in + 31) // 32 * 32
                    prep.update(cpp=cpp, wl_p=ops.x3p_pack(_conv3_matrix(a.conv_l[0].weight, cpp)), wr_p=ops.x3p_pack(prep["wr"]), wp_p=ops.x3p_pack(prep["wp"]))
            for name, conv, bn in self._ups():
                wm = _convT_matrices(conv.weight)
                u = dict(w=wm, raw=_fold_up(conv, None), fold=_fold_up(conv, bn) if bn is not None else None)
                if packed:
                    u["w_p"] = ops.x3p_pack_classes(wm, 128)
                prep[name] = u
            self._extra_prepare(prep)
            _publish_cache()
            self._cache = (key, prep)
        return self._cache[1]

    def _extra_prepare(self, prep):
        pass

    # ---- AttentionFusionSimple, eval
    @staticmethod
    def _attn_packed(p, xc, ac):
        """-> the fused map as a packed ``[M][out_ch]`` matrix with a zero row behind its pixels."""
        B, h, w, C = xc.shape
        M, nh, dev = B * h * w, ac.shape[-1], xc.device
        ra = (M + 128) // 128 * 128                           # rows allocated: the pixels + at least one zero row (taps outside the image)
        cat = torch.zeros(M, p["cpp"], device=dev, dtype=torch.float32)
        cat[:, :C] = xc.reshape(M, C)
        cat[:, C:C + nh] = ac.reshape(M, nh)
        x1 = torch.empty(M, C, device=dev, dtype=torch.float32)
        ops.conv_x3p(ops.x3p_pack(cat, ra), p["wl_p"], 1, B, h, w, C, C=x1, scale=p["fl"][0], shift=p["fl"][1], act=2)
        xr = (xc * ac.mean(dim=-1, keepdim=True)).reshape(M, C).contiguous()
        x12 = ops.Packed(M, C, dev)
        ops.conv_x3p(ops.x3p_pack(xr, ra), p["wr_p"], 1, B, h, w, C, scale=p["fr"][0], shift=p["fr"][1], act=2, mul=x1, out=x12)
        co = p["wp"].shape[0]
        y = ops.Packed(M, co, dev, rows_alloc=ra, zero=True)
        ops.gemm_x3p(x12, p["wp_p"], co, shift=p["bp"], out=y)
        return y

    @staticmethod
    def _attn_plain(p, xc, ac):
        """-> the fused map ``[B,h,w,out_ch]`` fp32 channel-last."""
        B, h, w, C = xc.shape
        nh = ac.shape[-1]
        cat = torch.zeros(B, h, w, p["cp"], device=xc.device, dtype=torch.float32)
        cat[..., :C] = xc
        cat[..., C:C + nh] = ac
        x1 = torch.empty(B, h * w, C, device=xc.device, dtype=torch.float32)
        ops.gemm_x3(cat, p["wl"], x1, h * w, C, 9 * p["cp"], 0, 9 * p["cp"], C, nb1=B, sA=(h * w * p["cp"], 0), sC=(h * w * C, 0), a_mode=1, H=h, W=w,
                    Cp=p["cp"], scale=p["fl"][0], shift=p["fl"][1], act=2)
        xr = (xc * ac.mean(dim=-1, keepdim=True)).contiguous()
        x12 = torch.empty_like(x1)
        ops.gemm_x3(xr, p["wr"], x12, h * w, C, 9 * C, 0, 9 * C, C, nb1=B, sA=(h * w * C, 0), sC=(h * w * C, 0), a_mode=1, H=h, W=w, Cp=C,
                    scale=p["fr"][0], shift=p["fr"][1], act=2, mul=x1)
        co = p["wp"].shape[0]
        y = torch.empty(B, h, w, co, device=xc.device, dtype=torch.float32)
        ops.gemm_x3(x12, p["wp"], y, B * h * w, co, C, C, C, co, shift=p["bp"])
        return y

    # ---- one ConvTranspose2d(4, 2, 1) in eval, either route: x = (map, B, h, w) with map a Packed or an fp32 [B,h,w,C] tensor
    @staticmethod
    def _up(x_cl, wm, fold, act):
        """One ConvTranspose2d(4, 2, 1) + folded BatchNorm + activation on a channel-last map ``[B,h,w,C]`` -> ``[B,2h,2w,Cout]``."""
        B, h, w, C = x_cl.shape
        cout = wm.shape[1]
        tmp = torch.empty(B, 4, h * w, cout, device=x_cl.device, dtype=torch.float32)
        ops.gemm_x3(x_cl, wm, tmp, h * w, cout, 4 * C, 0, 4 * C, cout, nb1=B, nb2=4, sA=(h * w * C, 0), sB=(0, cout * 4 * C), sC=(4 * h * w * cout, h * w * cout),
                    a_mode=2, H=h, W=w, Cp=C, scale=fold[0], shift=fold[1], act=act)
        return tmp.view(B, 2, 2, h, w, cout).permute(0, 3, 1, 4, 2, 5).reshape(B, 2 * h, 2 * w, cout).contiguous()

    def _up_layer(self, p, x, name, raw: bool, act: bool):
        """The layer ``name`` on ``x`` -> up to two maps of the doubled size: its raw output (bias only; fp32 ``[B,2h,2w,C]``: a module output) and
        ``GELU(BatchNorm(.))`` of it for the next layer (packed on the packed route).  Both come from the accumulators of the same product, each
        through its own epilogue: the BatchNorm + GELU act on the data BEFORE the next layer packs / gathers it, and the zero row that taps
        outside the image read stays zero (it would be GELU(shift) had the affine map been moved behind the gather)."""
        m, B, h, w = x
        u = p[name]
        cout = u["w"].shape[1]
        out_raw = out_act = None
        if p["packed"]:
            M4 = 4 * B * h * w
            if raw:
                out_raw = torch.empty(B, 2 * h, 2 * w, cout, device=m.buf.device, dtype=torch.float32)
                ops.conv_x3p(m, u["w_p"], 2, B, h, w, cout, C=out_raw.view(M4, cout), scale=u["raw"][0], shift=u["raw"][1], act=0)
            if act:
                out_act = ops.Packed(M4, cout, m.buf.device, rows_alloc=(M4 + 128) // 128 * 128, zero=True)
                ops.conv_x3p(m, u["w_p"], 2, B, h, w, cout, scale=u["fold"][0], shift=u["fold"][1], act=1, out=out_act)
        else:
            if raw:
                out_raw = self._up(m, u["w"], u["raw"], 0)
            if act:
                out_act = self._up(m, u["w"], u["fold"], 1)
        return out_raw, (out_act, B, 2 * h, 2 * w)

    def _final(self, p, x, name):
        """The chain's last layer with BatchNorm + GELU as a module output: fp32 ``[B,2h,2w,C]``."""
        m, B, h, w = x
        u = p[name]
        cout = u["w"].shape[1]
        if not p["packed"]:
            return self._up(m, u["w"], u["fold"], 1)
        out = torch.empty(B, 2 * h, 2 * w, cout, device=m.buf.device, dtype=torch.float32)
        ops.conv_x3p(m, u["w_p"], 2, B, h, w, cout, C=out.view(4 * B * h * w, cout), scale=u["fold"][0], shift=u["fold"][1], act=1)
        return out

    # ---- training
    @staticmethod
    def _attn_train(a, x, att):
        """models/module.py:459-466 with batch statistics: conv_l / conv_r / proj through ``Conv2dFn`` + ``BiasFn``, BatchNorm + Swish through
        ``BnActFn`` (SyncBatchNorm-aware), the gated product through ``MulFn``."""
        from .autograd import BnActFn
        from .fpn import ACT_SWISH, BiasFn, Conv2dFn

        def conv_bn(t, seq):
            y = BiasFn.apply(Conv2dFn.apply(t, seq[0].weight, 1, 1), seq[0].bias)
            return BnActFn.apply(y, seq[1].weight, seq[1].bias, None, seq[1], ACT_SWISH)

        x1 = conv_bn(torch.cat([x, att], dim=1), a.conv_l)
        gate = att.mean(dim=1, keepdim=True)                  # inputs come from the frozen ViT: no gradient flows through these two torch ops
        x2 = conv_bn(x * gate if not (x.requires_grad or att.requires_grad) else MulFn.apply(x, gate.expand_as(x)), a.conv_r)
        return BiasFn.apply(Conv2dFn.apply(MulFn.apply(x1, x2), a.proj.weight, 1, 0), a.proj.bias)

    @staticmethod
    def _convT_train(y, conv):
        from .fpn import BiasFn
        return BiasFn.apply(ConvT2dFn.apply(y, conv.weight, conv.stride[0], conv.padding[0]), conv.bias)

    @staticmethod
    def _bn_gelu_train(y, bn):
        from .autograd import BnActFn
        return BnActFn.apply(y, bn.weight, bn.bias, None, bn, ACT_GELU_BN)

    @staticmethod
    def _channels_last_inputs(x, att):
        # channel-last views ([B, vit_ch, h, w] made from tokens is a permuted view of [B, h*w, vit_ch]: contiguous() is free then)
        xc = x.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous()
        ac = att.detach().to(torch.float32).permute(0, 2, 3, 1).contiguous() if att is not None else None
        return xc, ac


class VITDecoderStage4Single(_DecoderBase):
    """models/module.py:353-368: ``forward(x [B,vit_ch,h,w], att [B,nhead,h,w]) -> [B,out_ch,4h,4w]`` (added to ``conv31``)."""

    def __init__(self, args):
        super().__init__()
        ch, vit_ch = args["out_ch"], args["vit_ch"]
        assert args["att_fusion"] is True
        self.attn = AttentionFusionSimple(vit_ch, ch * 4, args["nhead"])
        self.decoder = nn.Sequential(nn.ConvTranspose2d(ch * 4, ch * 2, 4, stride=2, padding=1), nn.BatchNorm2d(ch * 2), nn.GELU(),
                                     nn.ConvTranspose2d(ch * 2, ch, 4, stride=2, padding=1), nn.BatchNorm2d(ch), nn.GELU())
        self._cache = None

    def _ups(self):
        d = self.decoder
        return [("u1", d[0], d[1]), ("u2", d[3], d[4])]

    def _forward_train(self, x, att):
        """models/module.py:365-368 + :459-466 with batch statistics, every op an autograd-tracked HIP kernel (fp32 NCHW like the FPN's training
        path): the fusion through ``_attn_train``, the two ``ConvTranspose2d`` through ``ConvT2dFn``, BatchNorm + GELU through ``BnActFn``."""
        d = self.decoder
        y = self._attn_train(self.attn, x.to(torch.float32).contiguous(), att.to(torch.float32).contiguous())
        for conv, bn in ((d[0], d[1]), (d[3], d[4])):
            y = self._bn_gelu_train(self._convT_train(y, conv), bn)
        return y

    def forward(self, x, att):
        if self.training:
            return self._forward_train(x, att)
        p = self._prepared()
        with torch.no_grad():
            B, _, h, w = x.shape
            xc, ac = self._channels_last_inputs(x, att)
            y = (self._attn_packed if p["packed"] else self._attn_plain)(p, xc, ac)
            _, t = self._up_layer(p, (y, B, h, w), "u1", raw=False, act=True)
            return self._final(p, t, "u2").permute(0, 3, 1, 2)      # logical NCHW (channel-last memory); `conv31 + vit_out` broadcasts layouts


class VITDecoderStage4(_DecoderBase):
    """models/module.py:305-350 (``multi_scale=True``): ``forward(x [B,vit_ch,h,w], att [B,nhead,h,w]) -> (out1 [B,ch,4h,4w], out2 [B,ch/2,8h,8w],
    out3 [B,ch/4,16h,16w])``, the three transformer maps ``FPNDecoderV2`` concatenates.  Default: the chained form (``decoder2`` / ``decoder3`` start
    with the BatchNorm + GELU of the previous, un-normalised output); ``multi_scale_decoder=True``: three independent heads on the fused map."""

    def __init__(self, args):
        super().__init__()
        ch, vit_ch = args["out_ch"], args["vit_ch"]
        self.multi_scale_decoder = args.get("multi_scale_decoder", False)
        assert args["att_fusion"] is True
        self.attn = AttentionFusionSimple(vit_ch, ch * 4, args["nhead"])
        T, BN, G = (lambda i, o: nn.ConvTranspose2d(i, o, 4, stride=2, padding=1)), nn.BatchNorm2d, nn.GELU
        self.decoder1 = nn.Sequential(T(ch * 4, ch * 2), BN(ch * 2), G(), T(ch * 2, ch))
        if self.multi_scale_decoder:
            self.decoder2 = nn.Sequential(T(ch * 4, ch * 2), BN(ch * 2), G(), T(ch * 2, ch), BN(ch), G(), T(ch, ch // 2))
            self.decoder3 = nn.Sequential(T(ch * 4, ch * 2), BN(ch * 2), G(), T(ch * 2, ch), BN(ch), G(), T(ch, ch // 2), BN(ch // 2), G(),
                                          T(ch // 2, ch // 4))
        else:
            self.decoder2 = nn.Sequential(BN(ch), G(), T(ch, ch // 2))
            self.decoder3 = nn.Sequential(BN(ch // 2), G(), T(ch // 2, ch // 4))
        self._cache = None

    def _chains(self):
        """Per head ``[(name, conv, bn behind it or None)]``; in the chained form one chain runs through the three decoders."""
        d1, d2, d3 = self.decoder1, self.decoder2, self.decoder3
        if self.multi_scale_decoder:
            heads = []
            for k, d in ((1, d1), (2, d2), (3, d3)):
                convs = [i for i, m in enumerate(d) if isinstance(m, nn.ConvTranspose2d)]
                heads.append([("d%d_%d" % (k, i), d[i], d[i + 1] if i + 1 < len(d) else None) for i in convs])
            return heads
        return [[("d1_0", d1[0], d1[1]), ("d1_3", d1[3], d2[0]), ("d2_2", d2[2], d3[0]), ("d3_2", d3[2], None)]]

    def _ups(self):
        return [layer for chain in self._chains() for layer in chain]

    def _forward_train(self, x, att):
        """models/module.py:339-350 with batch statistics; every op an autograd-tracked HIP kernel, fp32 NCHW."""
        y = self._attn_train(self.attn, x.to(torch.float32).contiguous(), att.to(torch.float32).contiguous())
        outs = []
        for chain in self._chains():
            t = y
            for i, (_, conv, bn) in enumerate(chain):
                t = self._convT_train(t, conv)
                if not self.multi_scale_decoder and i >= 1:
                    outs.append(t)                            # out1, out2, out3 leave un-normalised
                if bn is not None:
                    t = self._bn_gelu_train(t, bn)
            if self.multi_scale_decoder:
                outs.append(t)
        return tuple(outs)

    def forward(self, x, att):
        if self.training:
            return self._forward_train(x, att)
        p = self._prepared()
        with torch.no_grad():
            B, _, h, w = x.shape
            xc, ac = self._channels_last_inputs(x, att)
            y = (self._attn_packed if p["packed"] else self._attn_plain)(p, xc, ac)
            outs = []
            for chain in self._chains():
                t = (y, B, h, w)
                for i, (name, _, bn) in enumerate(chain):
                    is_out = (i >= 1) if not self.multi_scale_decoder else (i == len(chain) - 1)
                    raw, t = self._up_layer(p, t, name, raw=is_out, act=bn is not None)
                    if is_out:
                        outs.append(raw)
            return tuple(o.permute(0, 3, 1, 2) for o in outs)


class VITDecoderStage4NoAtt(_DecoderBase):
    """models/module.py:371-386 (``att_fusion=False``): a 3x3 convolution ``vit_ch -> 4 ch`` + BatchNorm + GELU (implicit GEMM, ``a_mode=1``) in
    place of the attention fusion, then ``VITDecoderStage4Single``'s two-step decoder.  ``forward(x, att=None) -> [B,out_ch,4h,4w]``."""

    def __init__(self, args):
        super().__init__()
        ch, vit_ch = args["out_ch"], args["vit_ch"]
        self.down_sample = nn.Sequential(nn.Conv2d(vit_ch, ch * 4, kernel_size=3, padding=1), nn.BatchNorm2d(ch * 4), nn.GELU())
        self.decoder = nn.Sequential(nn.ConvTranspose2d(ch * 4, ch * 2, 4, stride=2, padding=1), nn.BatchNorm2d(ch * 2), nn.GELU(),
                                     nn.ConvTranspose2d(ch * 2, ch, 4, stride=2, padding=1), nn.BatchNorm2d(ch), nn.GELU())
        self._cache = None

    def _ups(self):
        d = self.decoder
        return [("u1", d[0], d[1]), ("u2", d[3], d[4])]

    def _packed_ok(self) -> bool:
        return self.down_sample[0].in_channels % 8 == 0 and super()._packed_ok()

    def _extra_prepare(self, prep):
        ds = self.down_sample
        prep.update(wd=_conv3_matrix(ds[0].weight, ds[0].in_channels), fd=_fold(ds[0], ds[1]))

    def _forward_train(self, x):
        from .fpn import BiasFn, Conv2dFn
        ds, d = self.down_sample, self.decoder
        y = BiasFn.apply(Conv2dFn.apply(x.to(torch.float32).contiguous(), ds[0].weight, 1, 1), ds[0].bias)
        y = self._bn_gelu_train(y, ds[1])
        for conv, bn in ((d[0], d[1]), (d[3], d[4])):
            y = self._bn_gelu_train(self._convT_train(y, conv), bn)
        return y

    def forward(self, x, att=None):
        if self.training:
            return self._forward_train(x)
        p = self._prepared()
        with torch.no_grad():
            B, C, h, w = x.shape
            if C % 8:
                raise _lib.MvsHipError("VITDecoderStage4NoAtt: vit_ch must be a multiple of 8 (got %d)" % C)
            xc, _ = self._channels_last_inputs(x, None)
            co = p["wd"].shape[0]
            y = torch.empty(B, h, w, co, device=x.device, dtype=torch.float32)
            ops.gemm_x3(xc, p["wd"], y, h * w, co, 9 * C, 0, 9 * C, co, nb1=B, sA=(h * w * C, 0), sC=(h * w * co, 0), a_mode=1, H=h, W=w, Cp=C,
                        scale=p["fd"][0], shift=p["fd"][1], act=1)
            if p["packed"]:
                M = B * h * w
                y = ops.x3p_pack(y.view(M, co), (M + 128) // 128 * 128)
            _, t = self._up_layer(p, (y, B, h, w), "u1", raw=False, act=True)
            return self._final(p, t, "u2").permute(0, 3, 1, 2)


def vit_branch(vit: VisionTransformer, dec: Optional[_DecoderBase], img: torch.Tensor, rescale: float = 0.5):
    """One view of mvsformer_model.py:243-262 up to ``vit_out``: bicubic resize, ViT with the last block's attention, reshapes, decoder - any of
    ``VITDecoderStage4Single`` / ``VITDecoderStage4NoAtt`` (one map) or ``VITDecoderStage4`` (``vit_out`` is then the tuple of its three maps)."""
    B, _, H, W = img.shape
    vh, vw = int(H * rescale), int(W * rescale)
    x = ops.bicubic_resize(img.detach().to(torch.float32).contiguous(), vh, vw, H / vh, W / vw)
    tok, att = vit.forward_with_cls_att(x)
    P = vit.patch_size
    hp, wp = vh // P, vw // P
    feat = tok[:, 1:].reshape(B, hp, wp, vit.embed_dim).permute(0, 3, 1, 2)
    att_cls = att[:, :, 1:].reshape(B, -1, hp, wp)
    return {"vit_imgs": x, "vit_feat": tok, "att_cls": att[:, :, 1:], "vit_out": dec(feat, att_cls) if dec is not None else None}
