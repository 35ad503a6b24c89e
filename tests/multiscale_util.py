"""Shared by tools/gen_multiscale_golden.py and the multi-scale tests: the model arguments, the fixed sampling of large tensors, the seeded
inputs of the decoder training golden and an fp64 torch restatement of the three ViT decoders (models/module.py:305-386, 450-466)."""
import torch
import torch.nn.functional as F

SAMPLE = 2048
VIT_ARGS = dict(twin=False, rescale=0.5, do_vit=True, patch_size=16, qk_scale="default", vit_arch="vit_small", vit_ch=384, out_ch=64,
                att_fusion=True, nhead=6, vit_path="")
DECODERS = (("chain", "VITDecoderStage4", dict(VIT_ARGS)), ("heads", "VITDecoderStage4", dict(VIT_ARGS, multi_scale_decoder=True)),
            ("noatt", "VITDecoderStage4NoAtt", dict(VIT_ARGS, att_fusion=False)))
TRAIN_SEEDS = {"chain": (51, 52), "heads": (53, 54), "noatt": (55, 56)}


def model_args(multi_scale=True, att_fusion=True, **vit):
    return dict(fix=True, depth_type="ce", fusion_type="cnn", inverse_depth=True, attn_temp=2.0, base_ch=8, ndepths=[32, 16, 8, 4],
                feat_chs=[8, 16, 32, 64], depth_interals_ratio=[4.0, 2.67, 1.5, 1.0], multi_scale=multi_scale,
                vit_args=dict(VIT_ARGS, att_fusion=att_fusion, **vit))


def sample_idx(numel: int, n: int = SAMPLE) -> torch.Tensor:
    """``n`` evenly spread flat indices (all of them for a small tensor): fixed by the size alone, so neither side stores them."""
    if numel <= n:
        return torch.arange(numel)
    return (torch.arange(n, dtype=torch.int64) * numel) // n


def sample(t: torch.Tensor, n: int = SAMPLE) -> torch.Tensor:
    flat = t.detach().reshape(-1)
    return flat[sample_idx(flat.numel(), n).to(flat.device)]


def train_inputs(seed: int):
    """The decoder training case: two 8 x 10 token maps (values exactly representable in fp16) and the generator that then draws the R's."""
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(2, 384, 8, 10, generator=g).to(torch.float16).to(torch.float32)
    att = (torch.rand(2, 6, 8, 10, generator=g) * 0.05).to(torch.float16).to(torch.float32)
    return feat, att, g


# ---------------------------------------------------------------------------------------------------------------------- fp64 restatement
def _bn(x, sd, pre, training):
    w, b = sd[pre + ".weight"].double(), sd[pre + ".bias"].double()
    if training:
        return F.batch_norm(x, None, None, w, b, True, 0.0, 1e-5)
    return F.batch_norm(x, sd[pre + ".running_mean"].double(), sd[pre + ".running_var"].double(), w, b, False, 0.0, 1e-5)


def _swish(x):
    return x * torch.sigmoid(x)


def _conv(x, sd, pre, pad):
    return F.conv2d(x, sd[pre + ".weight"].double(), sd[pre + ".bias"].double(), padding=pad)


def _convT(x, sd, pre):
    return F.conv_transpose2d(x, sd[pre + ".weight"].double(), sd[pre + ".bias"].double(), stride=2, padding=1)


def _seq(x, sd, pre, layout, training):
    """``layout``: per index of the nn.Sequential 'T' (ConvTranspose2d), 'B' (BatchNorm2d) or 'G' (GELU)."""
    for i, kind in enumerate(layout):
        if kind == "T":
            x = _convT(x, sd, "%s.%d" % (pre, i))
        elif kind == "B":
            x = _bn(x, sd, "%s.%d" % (pre, i), training)
        else:
            x = F.gelu(x)
    return x


def _attn(x, att, sd, training):
    x1 = _swish(_bn(_conv(torch.cat([x, att], dim=1), sd, "attn.conv_l.0", 1), sd, "attn.conv_l.1", training))
    x2 = _swish(_bn(_conv(x * att.mean(dim=1, keepdim=True), sd, "attn.conv_r.0", 1), sd, "attn.conv_r.1", training))
    return _conv(x1 * x2, sd, "attn.proj", 0)


def decoder_fp64(kind: str, sd, x, att, training=False):
    """``kind`` of :data:`DECODERS` -> the module's outputs (a tuple) in float64 from the ``state_dict`` ``sd``; autograd flows through."""
    x, att = x.double(), att.double()
    if kind == "noatt":
        y = F.gelu(_bn(_conv(x, sd, "down_sample.0", 1), sd, "down_sample.1", training))
        return (_seq(y, sd, "decoder", "TBGTBG", training),)
    y = _attn(x, att, sd, training)
    if kind == "heads":
        return (_seq(y, sd, "decoder1", "TBGT", training), _seq(y, sd, "decoder2", "TBGTBGT", training), _seq(y, sd, "decoder3", "TBGTBGTBGT", training))
    out1 = _seq(y, sd, "decoder1", "TBGT", training)
    out2 = _seq(out1, sd, "decoder2", "BGT", training)
    return out1, out2, _seq(out2, sd, "decoder3", "BGT", training)
