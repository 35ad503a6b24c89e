"""Flash attention for ViT fine-tuning (csrc/vit_flash_train.hip; mvsformer_amd/vit.py ``attention_flash_train_fwd`` / ``_bwd`` and the flash
blocks of ``_ViTTrainFn``) on the GPU: forward (out, row log-sum-exp, CLS row) and backward against fp64 torch autograd on the CPU, each
backward run twice for bitwise equality; key masking; agreement with the materialized path; the whole ViT with ``MVS_VIT_TRAIN_FLASH`` unset
against ``=0``; the peak-memory bound that the saved P matrices alone would break; graph capture.

Bars: relative L2 (``_l2``, as tests/test_hip_vit_train.py) 1e-5 on out, each third of dqkv and the CLS row - the bar the materialized split-form
path is held to, the flash form does the same arithmetic in another order; lse 1e-5 absolute against ``torch.logsumexp`` in fp64."""
import pytest
import torch

from mvsformer_amd.vit import attention_flash_train_bwd, attention_flash_train_fwd     # the feature's public functions: absent before it

pytestmark = pytest.mark.gpu

BAR = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _l2(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return ((got - want).norm() / max(1e-30, want.norm().item())).item()


def _rand(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _inputs(B, N, NH, seed, with_da, qk_scale=0.35):
    C = NH * 64
    g = torch.Generator().manual_seed(seed)
    qkv = _rand(g, B, N, 3 * C)
    qkv[..., :2 * C] *= qk_scale
    dout = _rand(g, B, N, C)
    da = _rand(g, B, NH, N, scale=float(N) ** 0.5) if with_da else None
    return qkv, dout, da


def _reference(qkv, dout, da, NH):
    """fp64 autograd on the CPU, as tests/test_hip_vit_train.py::test_attention_backward_vs_fp64 writes it -> (out, lse, att, dqkv)."""
    B, N, C3 = qkv.shape
    C, hd = C3 // 3, C3 // 3 // NH
    x = qkv.clone().requires_grad_(True)
    q, k, v = x.reshape(B, N, 3, NH, hd).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * hd ** -0.5
    att = s.softmax(-1)
    o = (att @ v).transpose(1, 2).reshape(B, N, C)
    loss = (o * dout).sum()
    if da is not None:
        loss = loss + (att[:, :, 0] * da).sum()                # the CLS row's gradient (mvsformer_model.py:223,253)
    loss.backward()
    return o.detach(), torch.logsumexp(s.detach(), -1), att.detach(), x.grad


def _run_flash(dev, qkv, dout, da, NH):
    f = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
    qkv_d, dout_d, da_d = f(qkv), f(dout), f(da)
    out, lse, cls_row = attention_flash_train_fwd(qkv_d, NH, want_cls=True)
    out2, lse2 = attention_flash_train_fwd(qkv_d, NH)
    dqkv = attention_flash_train_bwd(qkv_d, out, lse, dout_d, NH, da_d)
    dqkv2 = attention_flash_train_bwd(qkv_d, out, lse, dout_d, NH, da_d)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    assert torch.equal(dqkv, dqkv2)                            # deterministic: no atomics
    return out, lse, cls_row, dqkv


def _check(tag, got, ref, NH):
    out, lse, cls_row, dqkv = got
    o, rlse, att, grad = ref
    C = o.shape[-1]
    figs = {"out": _l2(out, o), "cls": _l2(cls_row, att[:, :, 0]), "lse_abs": (lse.double().cpu() - rlse).abs().max().item()}
    for j, name in enumerate("qkv"):
        figs["d" + name] = _l2(dqkv[..., j * C:(j + 1) * C], grad[..., j * C:(j + 1) * C])
    print(tag, " ".join("%s=%.3e" % kv for kv in figs.items()))
    for t in (out, lse, cls_row, dqkv):
        assert torch.isfinite(t).all()
    for name, v in figs.items():
        assert v < BAR, (tag, name, v)


@pytest.mark.parametrize("with_da", [False, True])
@pytest.mark.parametrize("N", [17, 50, 321, 1729])
def test_flash_forward_backward_vs_fp64(dev, N, with_da):
    B, NH = 2, 6
    qkv, dout, da = _inputs(B, N, NH, N * 2 + int(with_da), with_da)
    _check("N=%d da=%d" % (N, with_da), _run_flash(dev, qkv, dout, da, NH), _reference(qkv, dout, da, NH), NH)


def test_flash_forward_backward_vs_fp64_hires(dev):
    """3073 tokens: the ViT's token count in the 2048 x 1536 fine-tune (1024 x 768 after the rescale)."""
    B, NH, N = 1, 2, 3073
    qkv, dout, da = _inputs(B, N, NH, 3073, True)
    _check("N=3073", _run_flash(dev, qkv, dout, da, NH), _reference(qkv, dout, da, NH), NH)


@pytest.mark.parametrize("with_da", [False, True])
def test_flash_peaked_softmax(dev, with_da):
    """Logits spanning tens of units: the online maximum of the forward and exp(s - lse) of the backward.  Peaked, not degenerate: no row of
    the fp64 reference has a probability of exactly 1."""
    B, NH, N = 2, 6, 321
    qkv, dout, da = _inputs(B, N, NH, 77 + int(with_da), with_da, qk_scale=1.5)
    ref = _reference(qkv, dout, da, NH)
    q, k = qkv[..., :NH * 64].reshape(B, N, NH, 64), qkv[..., NH * 64:2 * NH * 64].reshape(B, N, NH, 64)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * 0.125
    assert (s.amax(-1) - s.amin(-1)).max() > 15.0                # (19.8 / 20.5 for these seeds)
    assert ref[2].amax(-1).max().item() < 1.0
    _check("peaked da=%d" % with_da, _run_flash(dev, qkv, dout, da, NH), ref, NH)


@pytest.mark.parametrize("N", [17, 50])
def test_flash_key_masking(dev, N):
    """The interface takes dense ``[B][N][3C]`` rows (no padding to fill), so the token counts that are no multiple of any tile are run embedded
    in a larger batch whose neighbouring images are NaN: a key, query or row read beyond an image's N tokens would land in them.  The embedded
    image's results are finite, within the bar of fp64 and bitwise those of the image run alone."""
    NH = 6
    qkv, dout, da = _inputs(1, N, NH, 900 + N, True)
    alone = _run_flash(dev, qkv, dout, da, NH)
    _check("masking N=%d" % N, alone, _reference(qkv, dout, da, NH), NH)
    nan = lambda t: torch.full_like(t, float("nan"))
    big = [torch.cat([nan(t), t, nan(t)], dim=0).to(dev, torch.float32).contiguous() for t in (qkv, dout, da)]
    out, lse, cls_row = attention_flash_train_fwd(big[0], NH, want_cls=True)
    dqkv = attention_flash_train_bwd(big[0], out, lse, big[1], NH, big[2])
    for got, want in zip((out, lse, cls_row, dqkv), alone):
        assert torch.isfinite(got[1]).all()
        assert torch.equal(got[1:2], want)


@pytest.mark.parametrize("with_da", [False, True])
def test_flash_agrees_with_materialized(dev, with_da):
    """Both paths are held to 1e-5 of fp64, so to 2e-5 of each other."""
    from mvsformer_amd import vit as V
    B, NH, N = 2, 6, 321
    C = NH * 64
    qkv, dout, da = _inputs(B, N, NH, 5, with_da)
    f = lambda t: None if t is None else t.to(dev, torch.float32).contiguous()
    qkv_d, dout_d, da_d = f(qkv), f(dout), f(da)
    p, out_m = V.attention_train_fwd(qkv_d, NH)
    dqkv_m = V.attention_train_bwd(qkv_d, p, dout_d, NH, da_d)
    out, lse, cls_row = attention_flash_train_fwd(qkv_d, NH, want_cls=True)
    dqkv = attention_flash_train_bwd(qkv_d, out, lse, dout_d, NH, da_d)
    figs = [_l2(out, out_m), _l2(cls_row, p[:, :, 0])] + [_l2(dqkv[..., j * C:(j + 1) * C], dqkv_m[..., j * C:(j + 1) * C]) for j in range(3)]
    print("flash vs materialized: out %.3e cls %.3e dq %.3e dk %.3e dv %.3e" % tuple(figs))
    assert max(figs) < 2e-5, figs


def test_flash_refuses_other_head_sizes_and_cpu(dev):
    from mvsformer_amd._lib import MvsHipError
    with pytest.raises(MvsHipError):
        attention_flash_train_fwd(torch.zeros(1, 8, 3 * 2 * 32, device=dev), 2)          # head dimension 32
    with pytest.raises(MvsHipError):
        attention_flash_train_fwd(torch.zeros(1, 8, 3 * 64), 1)                          # no CPU path


def _vit(dev, seed=11):
    import mvsformer_amd as m
    net = m.vit_small(patch_size=16, qk_scale="default")
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("norm1.weight") or name.endswith("norm2.weight") or name == "norm.weight":
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2 and "pos_embed" not in name and "cls_token" not in name:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p[0].numel()) ** 0.5)
            else:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    return net.to(dev).train()


def _vit_grads(net, img, wt, wa, entry):
    net.zero_grad()
    tok, att = getattr(net, entry)(img)
    ((tok * wt).sum() + (att * wa).sum()).backward()
    return tok.detach(), att.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


@pytest.mark.parametrize("entry", ["forward_with_cls_att", "forward_with_last_att"])
def test_vit_flash_vs_materialized(dev, monkeypatch, entry):
    """``vit_small`` in training mode, parameter gradients with ``MVS_VIT_TRAIN_FLASH`` unset against ``=0`` (read per call); the flash path twice:
    bitwise equal.  ``forward_with_last_att`` still returns the whole matrix (its last block stays materialized, the other 11 are flash)."""
    net = _vit(dev)
    g = torch.Generator().manual_seed(21)
    img = torch.rand(2, 3, 128, 160, generator=g).to(dev)
    N = 81
    wt = torch.randn(2, N, 384, generator=g).to(dev)
    wa = (torch.randn(2, 6, N, generator=g) if entry == "forward_with_cls_att" else torch.randn(2, 6, N, N, generator=g)).to(dev) * 9.0
    monkeypatch.delenv("MVS_VIT_TRAIN_FLASH", raising=False)
    tok, att, grads = _vit_grads(net, img, wt, wa, entry)
    tok2, att2, grads2 = _vit_grads(net, img, wt, wa, entry)
    assert tuple(att.shape) == tuple(wa.shape)
    assert torch.equal(tok, tok2) and torch.equal(att, att2) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    monkeypatch.setenv("MVS_VIT_TRAIN_FLASH", "0")
    tok0, att0, grads0 = _vit_grads(net, img, wt, wa, entry)
    worst = max((_l2(grads[k], grads0[k]), k) for k in grads)
    print("%s: tokens %.3e att %.3e worst gradient %.3e (%s)" % ((entry, _l2(tok, tok0), _l2(att, att0)) + worst))
    assert _l2(tok, tok0) < 2e-5 and _l2(att, att0) < 2e-5
    assert worst[0] < 2e-5, worst
    assert not torch.equal(grads["blocks.0.attn.qkv.weight"], grads0["blocks.0.attn.qkv.weight"])     # the switch did select another path


def test_vit_flash_peak_memory(dev, monkeypatch):
    """One training forward + backward at 2 views of 576 x 768 (1729 tokens) must stay below the size of the twelve saved P matrices alone,
    12 * B * heads * N^2 * 4 bytes (1.72 GB): the materialized path holds those plus every other saved activation and cannot pass; the flash
    path saves about 15 C floats per token and block and no N x N tensor."""
    monkeypatch.delenv("MVS_VIT_TRAIN_FLASH", raising=False)
    net = _vit(dev)
    B, NH = 2, 6
    img = torch.rand(B, 3, 576, 768, device=dev)
    N = (576 // 16) * (768 // 16) + 1
    assert N == 1729
    bound = 12 * B * NH * N * N * 4
    params = list(net.parameters())
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    tok, att = net.forward_with_cls_att(img)
    grads = torch.autograd.grad(tok.sum() + att.sum(), params)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - base
    print("peak %.1f MB over the level before the call; bound %.1f MB" % (delta / 2 ** 20, bound / 2 ** 20))
    assert all(torch.isfinite(g_).all() for g_ in grads)
    assert delta < bound, (delta, bound)


def test_flash_graph_capture(dev):
    """One flash forward + backward captured with ``torch.cuda.graph`` and replayed twice with fresh inputs copied into the static buffers:
    each replay equals the eager result bitwise."""
    B, NH, N = 2, 6, 321
    sets = [[t.to(dev, torch.float32).contiguous() for t in _inputs(B, N, NH, 40 + i, True)] for i in range(3)]

    def step(qkv, dout, da):
        out, lse, cls_row = attention_flash_train_fwd(qkv, NH, want_cls=True)
        return out, lse, cls_row, attention_flash_train_bwd(qkv, out, lse, dout, NH, da)

    eager = [[t.clone() for t in step(*s_)] for s_ in sets]
    static = [t.clone() for t in sets[0]]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(*static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(*static)
    for i in (1, 2):
        for dst, src in zip(static, sets[i]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager[i]))
