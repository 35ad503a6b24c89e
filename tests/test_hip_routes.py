"""Which kernels the eval paths launch under each switch set, on ONE live module with no cache reset between the sets, against the launch
orders recorded before the routing was gathered into pure functions (module.conv_route / deconv_route / tail_route for the regularizers;
fpn.encoder_route / decoder_route / v2_tail_route, stagenet.sweep_plan / stage_switches and the switch-keyed ViT caches for the rest).
test_hip_routes.json holds launch tags only, from a fresh module per switch set.  The "paths agree" tests elsewhere would pass if every
switch set took the same route; these would not."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

SETS = [{}, {"MVS_CONV_X3_MIN_VOXELS": "0"}, {"MVS_CONV_X3": "0"}, {"MVS_CONV_X3": "0", "MVS_CONV_WINO": "1"},
        {"MVS_CONV_X3_MIN_VOXELS": "0", "MVS_TAIL": "fp32"}, {"MVS_FUSE_PROB": "0"}]
SWITCHES = sorted({k for env in SETS for k in env})
CASES = {"costregnet": ("CostRegNet", lambda n, x: n(x), (1, 8, 8, 16, 24)),
         "costregnet3d_logits": ("CostRegNet3D", lambda n, x: n.logits(x), (1, 8, 4, 64, 96)),
         "costregnet3d_forward": ("CostRegNet3D", lambda n, x: n(x), (1, 8, 4, 64, 96))}


def _name(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_hip_routes.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", sorted(CASES))
def test_switch_sets_take_the_recorded_routes(dev, monkeypatch, recorded, case):
    import mvsformer_amd as m
    from mvsformer_amd import ops
    cls, run, shape = CASES[case]
    torch.manual_seed(3)
    net = getattr(m, cls)(8, 8).eval()
    m.randomize_bn_(net, 5)
    net = net.to(dev)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(11)).to(dev)
    orders, outs = {}, {}
    for env in SETS:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with torch.no_grad(), ops.kernel_timer() as kt:
            outs[_name(env)] = run(net, x)
        # on a live network the pack launches of a rebuild come before the layer launches: compared without them (as recorded)
        orders[_name(env)] = [t for t in kt.order if "pack" not in t and "prepare" not in t]
    for name, order in orders.items():
        print(case, name, order)
        assert order == recorded[case][name], (case, name)
    assert len({tuple(o) for o in orders.values()}) > 1, "every switch set took the same route"
    ref = outs["MVS_CONV_X3=0"]
    s = ref.abs().max().item()
    for name, y in outs.items():
        assert y.shape == ref.shape and (y - ref).abs().max().item() < 5e-6 * s, (case, name)


# ------------------------------------------------------------------------------------------- FPN, FPNDecoderV2, StageNet sweeps, ViT
# A case is ``case(dev) -> (sets, build)``: ``sets`` = [(recorded name, environment)] in the order they are applied, ``build()`` makes the
# module(s) and returns ``run() -> {output name: tensor}``; ``check(outs)`` gets the outputs per position of ``sets``.
def _scale_err(got, want):
    """Largest difference in units of the reference map's scale (tests/test_hip_fpn.py::scale_err, tests/test_hip_vit.py::_rel)."""
    want = want.double()
    return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-6))


def _fpn_case(dev):
    import mvsformer_amd as m
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(43)).to(dev)

    def build():
        torch.manual_seed(41)
        enc, dec = m.FPNEncoder([8, 16, 32, 64]).eval(), m.FPNDecoder([8, 16, 32, 64]).eval()
        m.randomize_bn_(enc, 5), m.randomize_bn_(dec, 6)
        enc, dec = enc.to(dev), dec.to(dev)

        def run():
            feats = enc(x)
            outs = dec(*feats)                                   # level 3 reads conv01's channel-last companion where fpn_cp runs
            return dict([("feat%d" % i, f) for i, f in enumerate(feats)] + [("out%d" % i, o) for i, o in enumerate(outs)])
        return run
    sets = [("default", {}), ("MVS_FPN_X3=0", {"MVS_FPN_X3": "0"}), ("MVS_FPN_X3=strip", {"MVS_FPN_X3": "strip"}), ("default", {})]
    return sets, build


def _fpn_check(sets, outs):
    """Every form of a layer is held within 2e-5 of the reference module's map (test_hip_fpn.py::test_fpn_encoder_vs_golden, all of x3 = 1 |
    0): two forms are within 4e-5 of each other.  The decoder behind its own set's encoder: 1e-4 of the map's scale, what
    test_hip_fpn.py::test_fpn_encoder_decoder_full_size_vs_torch_on_gpu allows the chain against the plain fp32 computation."""
    ref = outs[1]                                                # MVS_FPN_X3=0: fp32 matrix cores throughout
    for (name, _), o in zip(sets, outs):
        for k, v in o.items():
            e = _scale_err(v, ref[k])
            print("fpn", name, k, "%.3e" % e)
            assert v.shape == ref[k].shape and e < (4e-5 if k.startswith("feat") else 1e-4), (name, k, e)


def _v2_case(dev):
    import mvsformer_amd as m
    N, h, w = 1, 1, 1                                            # the smallest maps of test_hip_multiscale.py::test_decoder_v2_switch_routes_agree
    g = torch.Generator().manual_seed(5)
    c = [8, 16, 32, 64]
    convs = [torch.randn(N, c[i], h << (3 - i), w << (3 - i), generator=g).to(dev) for i in range(4)]
    vits = [torch.randn(N, c[3 - i], h << i, w << i, generator=g).to(dev) for i in range(3)]

    def build():
        torch.manual_seed(9)
        dec = m.FPNDecoderV2(c).eval()
        m.randomize_bn_(dec, 7)
        dec = dec.to(dev)
        return lambda: {"out%d" % (i + 1): o.clone() for i, o in enumerate(dec(*convs, *vits))}
    return [("default", {}), ("MVS_FPN_V2_TAIL=0", {"MVS_FPN_V2_TAIL": "0"}), ("default", {})], build


def _v2_check(sets, outs):
    """test_hip_multiscale.py::test_decoder_v2_switch_routes_agree: the first three maps bit for bit, the full-resolution map within TAIL_TOL."""
    ref = outs[1]
    for (name, _), o in zip(sets, outs):
        assert all(torch.equal(o["out%d" % k], ref["out%d" % k]) for k in (1, 2, 3)), name
        e = _scale_err(o["out4"], ref["out4"])
        print("fpn_v2", name, "%.3e" % e)
        assert e < 2e-5, (name, e)


STAGE_KEYS = ("depth", "prob_volume_pre", "photometric_confidence", "sim_depth")


def _stage_case(dev):
    import mvsformer_amd as m
    from mvsformer_amd import ops, stagenet, synth
    B, V, C, H, W, D, G = 1, 3, 32, 16, 24, 8, 8                 # C = 32: the stored-correlation sweeps are built for it
    scene = synth.make_scene(V, H * 4, W * 4, seed=C + H)
    feat = synth.render_features(scene, 4, C, batch=B, device=dev).contiguous()
    proj = synth.proj_matrices(scene, (4,), B, device=dev)["stage1"]
    z = synth.plane_depth(scene, 4, device=dev)
    hyp = (1.0 / (1.0 / z[None, None] + torch.linspace(1, -1, D, device=dev).view(1, D, 1, 1) * (1e-5 * D))).repeat(B, 1, 1, 1).contiguous()
    bank = ops.to_channels_last(feat)[0].contiguous()            # [V,H,W,C]: the same views, once each
    # a limit below the whole store under which two bands fit (as test_hip_parity.py::test_banded_stored_correlation_stage_equals_unbanded_exactly)
    full_mb = ops.cv_store_bytes(ops.to_channels_last(feat), D, G) / 2 ** 20
    assert full_mb > 0
    band_rows = -(-H // 2) + 2 * stagenet.VIS_HALO + 1
    banded = {"MVS_CV_STORE_MAX_MB": repr(full_mb * band_rows / H * 1.001), "MVS_CV_STORE_BANDS": "4"}

    def build():
        torch.manual_seed(C + H)
        net = m.StageNet(dict(base_ch=G, fusion_type="cnn", depth_type="ce"), D, 0).eval()
        m.randomize_bn_(net, 3)
        net = net.to(dev)

        def run():
            a, b = net(feat, proj, hyp, tmp=2.0), net.forward_bank(bank, [list(range(V))], proj, hyp, tmp=2.0)
            return dict([(k, a[k]) for k in STAGE_KEYS] + [("bank." + k, b[k]) for k in STAGE_KEYS])
        return run
    sets = [("default", {}), ("MVS_VIS=wino", {"MVS_VIS": "wino"}), ("MVS_VIS=valu", {"MVS_VIS": "valu"}),
            ("MVS_CV_STORE_MAX_MB=0", {"MVS_CV_STORE_MAX_MB": "0"}), ("banded", banded), ("MVS_CV_TILED=1", {"MVS_CV_TILED": "1"})]
    return sets, build


def _stage_check(sets, outs):
    """Logits of every set within 1e-4 of the default's: what test_hip_parity.py::test_stage_vs_oracle_mixed_kernel_paths asserts between the fast
    and the plain kernel paths of a stage.  The banded sweeps equal the one-store sweeps bit for bit
    (test_hip_parity.py::test_banded_stored_correlation_stage_equals_unbanded_exactly), and the bank form equals the dense form bit for bit
    wherever it exists (the LDS-tiled sweeps have none: there ``forward_bank`` takes the default route)."""
    ref = outs[0]
    for (name, _), o in zip(sets, outs):
        e = (o["prob_volume_pre"].double() - ref["prob_volume_pre"].double()).abs().max().item()
        print("stagenet", name, "%.3e" % e)
        assert e < 1e-4, (name, e)
        for k in STAGE_KEYS:
            if name != "MVS_CV_TILED=1":
                assert torch.equal(o["bank." + k], o[k]), (name, k)
            else:
                assert torch.equal(o["bank." + k], ref["bank." + k]), (name, k)
            if name == "banded":
                assert torch.equal(o[k], ref[k]), (name, k)


def _vit_case(dev):
    import mvsformer_amd as m
    g = torch.Generator().manual_seed(17)
    img = torch.randn(2, 3, 48, 64, generator=g).to(dev)
    x, att = torch.randn(2, 128, 3, 4, generator=g).to(dev), (torch.rand(2, 2, 3, 4, generator=g) * 0.05).to(dev)

    def build():
        torch.manual_seed(19)
        vit = m.VisionTransformer(img_size=(224,), patch_size=16, embed_dim=128, depth=2, num_heads=2, qkv_bias=True).eval()
        dec = m.VITDecoderStage4Single(dict(out_ch=16, vit_ch=128, att_fusion=True, nhead=2)).eval()
        m.randomize_bn_(dec, 23)
        vit, dec = vit.to(dev), dec.to(dev)

        def run():
            tok, cls_att = vit.forward_with_cls_att(img)
            return {"tokens": tok, "cls_att": cls_att, "decoder": dec(x, att)}
        return run
    return [("default", {}), ("MVS_VIT_PACKED=0", {"MVS_VIT_PACKED": "0"}), ("default", {})], build


def _vit_check(sets, outs):
    """Tokens and the CLS attention row: 2e-5 between the pre-split and the in-block split ViT (test_hip_vit.py, the test that sets
    MVS_VIT_PACKED=0).  The decoder (on inputs of its own, so that the ViT's difference does not enter): each route is held within 2e-5 of fp64
    (test_hip_multiscale.py::test_vit_decoders_eval_vs_fp64), so the two are within 4e-5 of each other."""
    ref = outs[1]
    for (name, _), o in zip(sets, outs):
        for k, bound in (("tokens", 2e-5), ("cls_att", 2e-5), ("decoder", 4e-5)):
            e = _scale_err(o[k], ref[k])
            print("vit", name, k, "%.3e" % e)
            assert o[k].shape == ref[k].shape and e < bound, (name, k, e)


# (case, check, tags of launches the module caches whatever the switches say): the ViT resizes its position table once per token grid
EVAL_CASES = {"fpn": (_fpn_case, _fpn_check, ()), "fpn_v2": (_v2_case, _v2_check, ()), "stagenet": (_stage_case, _stage_check, ()),
              "vit": (_vit_case, _vit_check, ("bicubic_resize",))}


def _layer_launches(order, cached=()):
    """Without what a live module launches only when a cache is rebuilt: the pack launches (as recorded) and the case's ``cached`` tags."""
    return [t for t in order if "pack" not in t and "prepare" not in t and t not in cached]


def run_sets(sets, build, setenv, delenv):
    """Apply ``sets`` in order to ONE module, no cache reset between them -> (launch orders, outputs), per position."""
    from mvsformer_amd import ops
    names = sorted({k for _, env in sets for k in env})
    run = build()
    orders, outs = [], []
    for _, env in sets:
        for k in names:
            delenv(k)
        for k, v in env.items():
            setenv(k, v)
        with torch.no_grad(), ops.kernel_timer() as kt:
            out = run()
        torch.cuda.synchronize()
        outs.append(out)
        orders.append(list(kt.order))
    for k in names:
        delenv(k)
    return orders, outs


@pytest.mark.parametrize("case", sorted(EVAL_CASES))
def test_eval_paths_take_the_recorded_routes(dev, monkeypatch, recorded, case):
    make, check, cached = EVAL_CASES[case]
    sets, build = make(dev)
    orders, outs = run_sets(sets, build, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    orders = [_layer_launches(o, cached) for o in orders]
    for (name, _), order in zip(sets, orders):
        print(case, name, order)
        assert order == _layer_launches(recorded[case][name], cached), (case, name)
    assert len({tuple(o) for o in orders}) > 1, "every switch set took the same route"
    check(sets, outs)
