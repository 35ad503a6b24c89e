#!/usr/bin/env python
"""Records the multi-scale goldens from the REAL reference classes (``models.mvsformer_model.DINOMVSNet`` with ``multi_scale=True``,
``models.module.VITDecoderStage4`` / ``VITDecoderStage4NoAtt``) on the CPU:

    python tools/gen_multiscale_golden.py /path/to/reference/checkout

* tests/golden/dinomvsnet_ms_shapes.json   ``state_dict`` key -> shape, in order
* tests/golden/dinomvsnet_ms_e2e.npz       eval, the images / cameras / depth range of dinomvsnet_e2e.npz (128 x 192, 3 views; named by digest,
                                           not stored twice): ``features_stage1`` whole, stages 2-4 as fixed samples + norms, every stage's
                                           depth, ``refined_depth``, ``photometric_confidence``
* tests/golden/vit_decoder_ms_train.npz    the three decoders in train(): outputs, loss, input / parameter gradients (fixed samples + norms),
                                           running statistics

Weights come from seeds (oracle/weights.py) and are rebuilt by the tests; large tensors are stored as ``tests/multiscale_util.sample`` of
them plus their L2 norm.
"""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
OUT = os.path.join(REPO, "tests", "golden")
SEED = 61


def _stub(name, **kw):
    m = types.ModuleType(name)
    m.__dict__.update(kw)
    sys.modules[name] = m


def np32(t):
    return t.detach().cpu().numpy().astype(np.float32)


def save(name, **arrs):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrs)
    print("%-28s %8.1f kB" % (name, os.path.getsize(path) / 1e3))


def _conditioning(net, real_forward, base, imgs, proj, dv, tmp, trials=3):
    """The REFERENCE's own answer to a feature error of 2e-6 of each map's scale (the project's bar for one fp32-equivalent layer): the largest
    change of ``photometric_confidence`` over ``trials`` random perturbations of the decoder's outputs."""
    worst = 0.0
    for trial in range(trials):
        g = torch.Generator().manual_seed(trial)
        net.decoder.forward = lambda *a: [o + 2e-6 * o.abs().max() * (torch.rand(o.shape, generator=g) * 2 - 1) for o in real_forward(*a)]
        with torch.no_grad():
            out = net(imgs, proj, dv, tmp=tmp)
        worst = max(worst, float((out["photometric_confidence"] - base["photometric_confidence"]).abs().max()))
    return worst


def gen_e2e(ref_mm):
    """The weight seed is the first from ``SEED`` on at which the reference model itself is a usable yardstick for the test's bars (depth 1e-3
    relative, confidence 2e-3): its stage depths vary over the image (a flat depth map would let 1e-3 hide a wrong feature map), and a feature
    error of 2e-6 moves its own confidence by less than a quarter of the confidence bar but by more than 5e-5 (random cascades exist at which
    one hypothesis takes all the probability everywhere and the output does not depend on the features at all).  Both criteria are
    properties of the reference on the CPU; nothing of the HIP path enters the choice."""
    import multiscale_util as mu
    from oracle.weights import make_model_state_dict
    cwd = os.getcwd()
    os.chdir(os.path.join(REPO, "tests"))                   # the constructor probes a relative weight path (absent: it only prints a notice)
    net = ref_mm.DINOMVSNet(mu.model_args(multi_scale=True))
    os.chdir(cwd)
    shapes = {k: list(v.shape) for k, v in net.state_dict().items()}
    with open(os.path.join(OUT, "dinomvsnet_ms_shapes.json"), "w") as f:
        json.dump(shapes, f, indent=0)
    net.eval()
    z = np.load(os.path.join(OUT, "dinomvsnet_e2e.npz"))
    imgs = torch.from_numpy(z["imgs"].astype(np.float32))
    proj = {"stage%d" % i: torch.from_numpy(z["proj_stage%d" % i]) for i in range(1, 5)}
    dv = torch.from_numpy(z["depth_range"])
    tmp = [float(t) for t in z["tmps"]]
    calls = []
    real_forward = net.decoder.forward                      # (the model calls decoder.forward(...) directly: a forward hook would not fire)

    def recording(*a):
        o = real_forward(*a)
        calls.append([t.detach().clone() for t in o])
        return o
    for seed in range(SEED, SEED + 16):
        net.load_state_dict(make_model_state_dict(shapes, seed), strict=True)
        del calls[:]
        net.decoder.forward = recording
        with torch.no_grad():
            out = net(imgs, proj, dv, tmp=tmp)
        spreads = [float((out["stage%d" % s]["depth"].max() - out["stage%d" % s]["depth"].min()) / out["stage%d" % s]["depth"].mean()) for s in range(1, 5)]
        moved = _conditioning(net, real_forward, out, imgs, proj, dv, tmp)
        print("seed %d: stage depth spreads %s of the mean, confidence moves %.2e under a 2e-6 feature error" % (seed, ["%.3f" % v for v in spreads], moved))
        if min(spreads) > 0.05 and 5e-5 < moved < 5e-4:
            break
    else:
        raise SystemExit("no usable seed")
    arrs = dict(inputs_sha256=np.array(hashlib.sha256(z["imgs"].tobytes() + z["depth_range"].tobytes()).hexdigest()), seed=np.int64(seed),
                tmps=np.array(tmp, dtype=np.float32), refined_depth=np32(out["refined_depth"]), reference_confidence_moves=np.float32(moved),
                photometric_confidence=np32(out["photometric_confidence"]))
    for s in range(4):
        f = torch.stack([c[s] for c in calls], dim=1)       # [1, V, C, H/s, W/s]
        if s == 0:
            arrs["features_stage1"] = np32(f)
        else:
            arrs["features_stage%d" % (s + 1)] = np32(mu.sample(f, 8192))
        arrs["norm_stage%d" % (s + 1)] = np.float64(f.double().norm())
        arrs["s%d_depth" % (s + 1)] = np32(out["stage%d" % (s + 1)]["depth"])
    save("dinomvsnet_ms_e2e.npz", **arrs)


def gen_decoder_train(ref_module):
    import multiscale_util as mu
    from oracle.weights import make_vit_state_dict
    arrs = {}
    for kind, cls, args in mu.DECODERS:
        wseed, iseed = mu.TRAIN_SEEDS[kind]
        dec = getattr(ref_module, cls)(args)
        shapes = {k: list(v.shape) for k, v in dec.state_dict().items()}
        dec.load_state_dict(make_vit_state_dict(shapes, wseed), strict=True)
        assert all(float(b.min()) > 0 for k, b in dec.named_buffers() if k.endswith("running_var"))
        dec.train()
        feat, att, g = mu.train_inputs(iseed)
        feat.requires_grad_(True), att.requires_grad_(True)
        outs = dec(feat, att)
        outs = outs if isinstance(outs, tuple) else (outs,)
        loss = sum((o * torch.randn(o.shape, generator=g)).sum() for o in outs)
        loss.backward()
        p = kind + "."
        arrs[p + "keys"] = np.array(json.dumps(shapes))
        arrs[p + "loss"] = np.float64(loss.detach().double())
        for i, o in enumerate(outs, start=1):
            arrs[p + "out%d" % i], arrs[p + "out%d.norm" % i] = np32(mu.sample(o)), np.float64(o.double().norm())
        arrs[p + "dfeat"], arrs[p + "dfeat.norm"] = np32(mu.sample(feat.grad)), np.float64(feat.grad.double().norm())
        if att.grad is not None:
            arrs[p + "datt"] = np32(att.grad)
        for k, prm in dec.named_parameters():
            arrs[p + "grad." + k], arrs[p + "norm." + k] = np32(mu.sample(prm.grad)), np.float64(prm.grad.double().norm())
        arrs.update({p + "buf." + k: np32(b) for k, b in dec.named_buffers() if b.dtype.is_floating_point})
    save("vit_decoder_ms_train.npz", **arrs)


def main(checkout):
    sys.path.insert(0, checkout)
    sys.dont_write_bytecode = True
    for name, kw in (("timm", {}), ("timm.models", {}),
                     ("timm.models.layers", dict(DropPath=nn.Identity, to_2tuple=lambda x: (x, x), trunc_normal_=nn.init.trunc_normal_)),
                     ("timm.models.vision_transformer", dict(Block=nn.Module)), ("torchvision", {}), ("torchvision.utils", {}),
                     ("omegaconf", dict(OmegaConf=object))):
        if name not in sys.modules:
            _stub(name, **kw)
    import warnings
    warnings.filterwarnings("ignore")
    import models.module as ref_module
    import models.mvsformer_model as ref_mm
    gen_decoder_train(ref_module)
    gen_e2e(ref_mm)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
