"""GPU tests of the argument checks of ``mvsformer_amd.ops`` that share a body: the 3-D conv-layer wrappers, the residual-shape check and
the pack / prepare wrappers, and (at the end) the checks the dense cost-volume sweeps share with the bank forms plus the sweep entries' null
checks straight through ctypes.  They allocate device tensors and launch NO kernel: ``ops._call`` is replaced by a recorder, so a refusal is
shown to come before anything reaches the library, and an accepted call is compared with the entry name, timer tag, work amount and
integer arguments written out here by hand (from the wrappers as they stood before they were folded, not computed by the code under test).
Shapes are the smallest each form's ``*_supported`` query accepts: B = 1, an 8 x 8 x 8 volume, the smallest channel pair."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture()
def calls(monkeypatch):
    from mvsformer_amd import ops
    seen = []
    monkeypatch.setattr(ops, "_call", lambda name, tag, *args: seen.append((name, tag, args)))
    return seen


def _t(*shape, dtype=torch.float32):
    return torch.empty(*shape, device=DEV, dtype=dtype)


def _layer(form, x, w, residual=None):
    from mvsformer_amd import ops
    return {
        "conv3d": lambda: ops.conv3d(x, w, 8, 8, (1, 1), residual=residual),
        "conv3d_s2": lambda: ops.conv3d(x, w, 8, 16, (2, 2), residual=residual),
        "conv3d_wino": lambda: ops.conv3d_wino(x, w, 16, 16, residual=residual),
        "conv3d_x3": lambda: ops.conv3d_x3(x, w, 16, 16, (1, 1), residual=residual),
        "conv3d_x3_s2": lambda: ops.conv3d_x3(x, w, 8, 16, (1, 2), residual=residual),
        "deconv3d_x3": lambda: ops.deconv3d_x3(x, w, 16, 8, 1, residual=residual),
        "deconv3d": lambda: ops.deconv3d(x, w, 16, 8, 1, residual=residual),
        "deconv3d_sd2": lambda: ops.deconv3d(x, w, 32, 16, 2, residual=residual, relu=False),
        "conv3d_small": lambda: ops.conv3d_small(x, w, 8, 16, 2, False, residual=residual),
        "conv3d_small_t": lambda: ops.conv3d_small(x, w, 16, 8, 2, True, residual=residual),
    }[form]()


# form: (cin, packed dtype, output shape, entry, tag name, FLOPs, the entry's integers from B to relu)
LAYERS = {
    "conv3d": (8, torch.float32, (1, 8, 8, 8, 8), "mvs_conv3d_fwd", "conv3d_kernel<1,1,1>", 2.0 * 27 * 8 * 8 * 512, (1, 8, 8, 8, 8, 8, 1, 1, 1)),
    "conv3d_s2": (8, torch.float32, (1, 16, 4, 4, 4), "mvs_conv3d_fwd", "conv3d_kernel<1,2,2>", 2.0 * 27 * 8 * 16 * 64, (1, 8, 16, 8, 8, 8, 2, 2, 1)),
    "conv3d_wino": (16, torch.float32, (1, 16, 8, 8, 8), "mvs_conv3d_wino_fwd", "wino_conv3d_kernel", 2.0 * 27 * 16 * 16 * 512, (1, 16, 16, 8, 8, 8, 1)),
    "conv3d_x3": (16, torch.uint8, (1, 16, 8, 8, 8), "mvs_conv3d_x3_fwd", "x3_conv_kernel<16,16,s1>", 2.0 * 27 * 16 * 16 * 512, (1, 16, 16, 8, 8, 8, 1, 1, 1)),
    "conv3d_x3_s2": (8, torch.uint8, (1, 16, 8, 4, 4), "mvs_conv3d_x3_fwd", "x3_conv_kernel<8,16,s2>", 2.0 * 27 * 8 * 16 * 128, (1, 8, 16, 8, 8, 8, 1, 2, 1)),
    "deconv3d_x3": (16, torch.uint8, (1, 8, 8, 16, 16), "mvs_deconv3d_x3_fwd", "x3_deconv_kernel<16,8>", 2.0 * 27 * 16 * 8 * 512, (1, 16, 8, 8, 8, 8, 1, 1)),
    "deconv3d": (16, torch.float32, (1, 8, 8, 16, 16), "mvs_deconv3d_fwd", "deconv3d_s1_kernel<8>", 2.0 * 27 * 16 * 8 * 512, (1, 16, 8, 8, 8, 8, 1, 1)),
    "deconv3d_sd2": (32, torch.float32, (1, 16, 16, 16, 16), "mvs_deconv3d_fwd", "deconv3d_kernel<1,2>", 2.0 * 27 * 32 * 16 * 512, (1, 32, 16, 8, 8, 8, 2, 0)),
    "conv3d_small": (8, torch.uint8, (1, 16, 4, 4, 4), "mvs_conv3d_small_fwd", "x3_small_kernel<conv,8,16,s2>", 2.0 * 27 * 8 * 16 * 64, (1, 8, 16, 8, 8, 8, 2, 0, 1)),
    "conv3d_small_t": (16, torch.uint8, (1, 8, 16, 16, 16), "mvs_conv3d_small_fwd", "x3_small_kernel<deconv,16,8,s2>", 2.0 * 27 * 16 * 8 * 512,
                       (1, 16, 8, 8, 8, 8, 2, 1, 1)),
}


def test_the_smallest_shapes_are_supported_ones():
    from mvsformer_amd import ops
    assert ops.conv3d_wino_supported(16, 16, 8, 8, 8) and not ops.conv3d_wino_supported(8, 8, 8, 8, 8)
    assert ops.conv3d_x3_supported(16, 16, (1, 1)) and ops.conv3d_x3_supported(8, 16, (1, 2)) and not ops.conv3d_x3_supported(8, 8, (1, 1))
    assert ops.deconv3d_x3_supported(16, 8, 1) and not ops.deconv3d_x3_supported(8, 8, 1)
    assert ops.conv3d_small_supported(8, 16, 2, False) and ops.conv3d_small_supported(16, 8, 2, True)


@pytest.mark.parametrize("form", sorted(LAYERS))
def test_layer_wrapper_checks_and_launch_arguments(form, calls):
    from mvsformer_amd._lib import MvsHipError
    cin, wdtype, oshape, entry, kernel, flops, ints = LAYERS[form]
    x, w = _t(1, cin, 8, 8, 8), _t(64, dtype=wdtype)
    bad = oshape[:-1] + (oshape[-1] - 1,)
    hint = {"deconv3d": " (stage H, W must be divisible by 8)", "deconv3d_sd2": " (stage H, W must be divisible by 8, D by 8)"}.get(form, "")
    with pytest.raises(MvsHipError) as e:
        _layer(form, x, w, _t(*bad))
    assert str(e.value) == "residual shape %s != output %s%s" % (bad, oshape, hint)
    with pytest.raises(MvsHipError) as e:
        _layer(form, x, w, _t(*oshape, dtype=torch.float64))
    assert str(e.value) == "residual must be torch.float32, got torch.float64"
    other = torch.float32 if wdtype == torch.uint8 else torch.uint8
    with pytest.raises(MvsHipError) as e:
        _layer(form, x, _t(64, dtype=other))
    assert str(e.value) == "packed weights must be %s, got %s" % (wdtype, other)
    with pytest.raises(MvsHipError) as e:
        _layer(form, x.cpu(), w)
    assert str(e.value) == "x must be a GPU tensor: the MI355X HIP path is the only implementation (no CPU fallback)"
    assert calls == []
    res = _t(*oshape)
    y = _layer(form, x, w, res)
    assert tuple(y.shape) == oshape and y.dtype == torch.float32 and y.device == x.device
    (name, tag, args), = calls
    assert name == entry and tag == (kernel, "flops", flops)
    assert args[:6] == (x.data_ptr(), w.data_ptr(), None, None, res.data_ptr(), y.data_ptr())
    assert args[6:-1] == ints and args[-1] == torch.cuda.current_stream().cuda_stream


def test_fused_tail_wrappers_check_the_residual(calls):
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    x, pw, pb = _t(1, 16, 8, 8, 8), _t(8), _t(1)
    good, bad = (1, 8, 8, 16, 16), (1, 8, 8, 16, 8)
    for run, wdtype in ((lambda w, r: ops.deconv3d_prob1(x, w, 16, None, None, r, pw, pb), torch.float32),
                        (lambda w, r: ops.tail_x3(x, w, None, None, r, pw, pb), torch.uint8)):
        with pytest.raises(MvsHipError) as e:
            run(_t(64, dtype=wdtype), _t(*bad))
        assert str(e.value) == "residual shape %s != %s" % (bad, good)
        other = torch.float32 if wdtype == torch.uint8 else torch.uint8
        with pytest.raises(MvsHipError) as e:
            run(_t(64, dtype=other), _t(*good))
        assert str(e.value) == "packed weights must be %s, got %s" % (wdtype, other)
    with pytest.raises(MvsHipError) as e:
        ops.tail_x3(_t(1, 8, 8, 8, 8), _t(64, dtype=torch.uint8), None, None, None, pw, pb)
    assert str(e.value) == "tail_x3: 8 input channels (built for 16)"
    assert calls == []
    w, r = _t(64, dtype=torch.uint8), _t(*good)
    logits = ops.tail_x3(x, w, None, None, r, pw, pb, relu=False)
    assert tuple(logits.shape) == (1, 8, 16, 16) and logits.dtype == torch.float32
    (name, tag, args), = calls
    assert name == "mvs_tail_x3_fwd" and tag == ("x3_tail_kernel<16,8,prob>", "flops", 2.0 * 27 * 16 * 8 * 512)
    assert args[:-1] == (x.data_ptr(), w.data_ptr(), None, None, r.data_ptr(), pw.data_ptr(), pb.data_ptr(), logits.data_ptr(), 1, 8, 8, 8, 0)


def test_bf16_layer_wrappers_check_the_residual(calls):
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    bf = torch.bfloat16
    x, w = _t(2, 8, 8, 8, 8, dtype=bf), _t(64, dtype=bf)
    good, bad = (2, 4, 4, 4, 16), (2, 4, 4, 4, 8)
    for run in (lambda r: ops.bf16_conv3d(x, w, 8, 16, 0, (2, 2), residual=r),
                lambda r: ops.bf16_conv3d_bn_fwd(x, w, 8, 16, 0, (2, 2), r, True, None, None, None, None, 0.1, 1e-5)):
        with pytest.raises(MvsHipError) as e:
            run(_t(*bad, dtype=bf))
        assert str(e.value) == "residual shape %s != output %s" % (bad, good)
        with pytest.raises(MvsHipError) as e:
            run(_t(*good))
        assert str(e.value) == "residual must be torch.bfloat16, got torch.float32"
    assert calls == []
    r = _t(*good, dtype=bf)
    y = ops.bf16_conv3d(x, w, 8, 16, 0, (2, 2), residual=r, relu=True)
    assert tuple(y.shape) == good and y.dtype == bf
    (name, tag, args), = calls
    assert name == "mvs_bf16_conv3d" and tag == ("bf16_conv_kernel<8,16,g0,s22>", "flops", 2.0 * 27 * 8 * 16 * 2 * 64)
    assert args[:-1] == (x.data_ptr(), w.data_ptr(), None, None, r.data_ptr(), y.data_ptr(), 2, 8, 16, 8, 8, 8, 0, 2, 2, 1)


W5 = (5, 5, 3, 3, 3)


def _refusals():
    """name -> (call, message): every pack / prepare wrapper at a channel count nothing is built for."""
    from mvsformer_amd import ops
    fold = (_t(8), _t(8))
    return {
        "conv3d_pack": (lambda: ops.conv3d_pack(_t(65, 65, 3, 3, 3), False), "unsupported conv channels Cin=65 Cout=65"),
        "conv3d_pack_shape": (lambda: ops.conv3d_pack(_t(8, 8, 3, 3), False), "conv weight must be [*,*,3,3,3], got (8, 8, 3, 3)"),
        "conv3d_wino_pack": (lambda: ops.conv3d_wino_pack(_t(*W5)), "conv3d_wino_pack: unsupported weight (5, 5, 3, 3, 3)"),
        "conv3d_wino_pack_shape": (lambda: ops.conv3d_wino_pack(_t(16, 16, 3, 3)), "conv3d_wino_pack: unsupported weight (16, 16, 3, 3)"),
        "conv3d_x3_pack": (lambda: ops.conv3d_x3_pack(_t(*W5)), "conv3d_x3_pack: unsupported weight (5, 5, 3, 3, 3) / stride (1, 1)"),
        "deconv3d_x3_pack": (lambda: ops.deconv3d_x3_pack(_t(*W5)), "deconv3d_x3_pack: unsupported weight (5, 5, 3, 3, 3) / sd 1"),
        "conv3d_small_pack": (lambda: ops.conv3d_small_pack(_t(*W5), 1, False),
                              "conv3d_small_pack: unsupported weight (5, 5, 3, 3, 3) / stride 1 / transposed False"),
        "tail_x3_pack": (lambda: ops.tail_x3_pack(_t(*W5)), "tail_x3_pack: weight (5, 5, 3, 3, 3) is not [16,8,3,3,3]"),
        "vis_wino_prepare": (lambda: ops.vis_wino_prepare(_t(5)), "vis params must hold 3689 floats"),
        "vis_x3_prepare": (lambda: ops.vis_x3_prepare(_t(5)), "vis params must hold 3689 floats"),
        "bf16_pack": (lambda: ops.bf16_pack(_t(*W5), 0, 5, 5), "bf16 conv: channels must be 8/16/32/64 (Cin=5 Cout=5, taps 27)"),
        "fpn_pack_weights": (lambda: ops.fpn_pack_weights(_t(5, 64, 3, 3)), "fpn 3x3 weight must be [8|16|32,64,3,3], got (5, 64, 3, 3)"),
        "fpn_level_x3s_prepare": (lambda: ops.fpn_level_x3s_prepare(_t(5, 64, 3, 3), _t(5)), "fpn_level_x3s_prepare: unsupported weight (5, 64, 3, 3)"),
        "fpn_level_x3s_prepare_scale": (lambda: ops.fpn_level_x3s_prepare(_t(16, 64, 3, 3), _t(5)),
                                        "fpn_level_x3s_prepare: unsupported weight (16, 64, 3, 3)"),
        "fpn_level_x3_prepare": (lambda: ops.fpn_level_x3_prepare(_t(5, 64, 3, 3), _t(64, 5), _t(64), _t(5), _t(5)),
                                 "fpn_level_x3_prepare: unsupported Ck=5 / weight (5, 64, 3, 3)"),
        "fpn_v2_tail_prepare": (lambda: ops.fpn_v2_tail_prepare(_t(5, 8, 4, 4), fold, _t(8, 8, 3, 3), fold),
                                "fpn_v2_tail_prepare: unsupported weights (5, 8, 4, 4), (8, 8, 3, 3)"),
        "conv2d_x3s_prepare": (lambda: ops.conv2d_x3s_prepare(_t(5, 5, 3, 3), _t(5), 1),
                               "conv2d_x3s_prepare: (5, 5, 3, 3) stride 1 is not a layer of the FPN encoder below full resolution"),
        "conv2d_x3_prepare": (lambda: ops.conv2d_x3_prepare(_t(5, 5, 3, 3), _t(5)), "conv2d_x3_prepare: (5, 5, 3, 3) is not conv00 / conv01 of the FPN encoder"),
        "conv2d_x3_prepare_scale": (lambda: ops.conv2d_x3_prepare(_t(8, 3, 7, 7), _t(5)),
                                    "conv2d_x3_prepare: (8, 3, 7, 7) is not conv00 / conv01 of the FPN encoder"),
        "conv2d_pack_weights": (lambda: ops.conv2d_pack_weights(_t(5, 5, 3, 3)), "conv2d weight (5, 5, 3, 3) is not an FPN encoder layer shape"),
    }


def test_pack_and_prepare_wrappers_refuse_unsupported_channels(calls):
    from mvsformer_amd._lib import MvsHipError
    for name, (run, message) in _refusals().items():
        with pytest.raises(MvsHipError) as e:
            run()
        assert str(e.value) == message, name
    assert calls == []


def test_pack_and_prepare_wrappers_allocate_what_the_size_query_says(calls):
    """An accepted weight: one launch of the entry with (weight, the form's integers, packed, stream); dtype and size of the result are the
    literal figures of the size queries (tests/test_abi.py pins those against the library)."""
    from mvsformer_amd import ops
    stream = torch.cuda.current_stream().cuda_stream
    w16, w168, scale8 = _t(16, 16, 3, 3, 3), _t(16, 8, 3, 3, 3), _t(8)
    w2d = _t(8, 3, 7, 7)
    cases = [
        (lambda: ops.conv3d_pack(w16, False), "mvs_conv3d_pack_weights", (w16.data_ptr(), 16, 16, 0), torch.float32, 6912),
        (lambda: ops.conv3d_pack(w168, True, 1), "mvs_conv3d_pack_weights", (w168.data_ptr(), 16, 8, 2), torch.float32, 3840),
        (lambda: ops.conv3d_wino_pack(w16), "mvs_conv3d_wino_pack_weights", (w16.data_ptr(), 16, 16), torch.float32, 12288),
        (lambda: ops.conv3d_x3_pack(w16), "mvs_conv3d_x3_pack_weights", (w16.data_ptr(), 16, 16, 1, 1), torch.uint8, 61440),
        (lambda: ops.deconv3d_x3_pack(w168), "mvs_deconv3d_x3_pack_weights", (w168.data_ptr(), 16, 8, 1), torch.uint8, 61440),
        (lambda: ops.conv3d_small_pack(w168, 2, True), "mvs_conv3d_small_pack_weights", (w168.data_ptr(), 16, 8, 2, 1), torch.uint8, 43008),
        (lambda: ops.conv2d_x3_prepare(w2d, scale8), "mvs_conv2d_x3_prepare", (w2d.data_ptr(), scale8.data_ptr(), 3, 8, 7), torch.uint8, 8 * 3 * 64 * 16),
        (lambda: ops.conv2d_pack_weights(w2d), "mvs_conv2d_pack_weights", (w2d.data_ptr(), 3, 8, 7), torch.float32, 3584),
    ]
    for run, entry, head, dtype, n in cases:
        del calls[:]
        packed = run()
        assert packed.dtype == dtype and tuple(packed.shape) == (n,) and packed.device == torch.device(DEV), entry
        assert calls == [(entry, None, head + (packed.data_ptr(), stream))], entry


# ----------------------------------------------------------------------------------------------- the cost-volume sweeps
def _sweep_args(C=8, H=24, W=40, D=4, B=1, V=3):
    """Dense sweep operands at the 8-channel 24 x 40 x 4 shape: channel-last features, rt, hypotheses, visibility weights."""
    return _t(B, V, H, W, C), _t(B, V - 1, 12), _t(B, D, H, W), _t(B, V - 1, H, W)


def test_dense_sweep_wrappers_share_the_bank_forms_checks(calls):
    """What the dense wrappers check since they share a body with the bank forms, each refused before anything reaches the library: hypotheses
    that are not ``[B,D,H,W]``, an ``rt`` that is not ``[B,V-1,12]``, visibility weights that are not ``[B,V-1,H,W]``, a band of rows outside
    the image (an empty one included)."""
    from mvsformer_amd import ops
    from mvsformer_amd._lib import MvsHipError
    feat, rt, depth, weight = _sweep_args()
    sweeps = {
        "cv_entropy": lambda rt=rt, depth=depth: ops.cv_entropy(feat, rt, depth, 8),
        "cv_aggregate": lambda rt=rt, depth=depth, weight=weight: ops.cv_aggregate(feat, rt, depth, weight, 8, True),
        "cv_corr": lambda rt=rt, depth=depth: ops.cv_corr(feat, rt, depth, 8),
        "cv_corr_rows": lambda rt=rt, depth=depth, y0=0, rows=24: ops.cv_corr_rows(feat, rt, depth, 8, y0, rows),
    }
    for name, run in sweeps.items():
        for bad in (_t(1, 4, 24, 39), _t(1, 4, 23, 40), _t(2, 4, 24, 40), _t(4, 24, 40)):
            with pytest.raises(MvsHipError, match=r"^%s: depth_values must be \[B,D,H,W\]" % name):
                run(depth=bad)
        for bad in (_t(1, 2, 16), _t(1, 3, 12), _t(2, 12)):
            with pytest.raises(MvsHipError, match=r"^%s: rt must be \[B,V-1,12\]" % name):
                run(rt=bad)
    for bad in (_t(1, 2, 24, 39), _t(1, 3, 24, 40), _t(1, 2, 23, 40), _t(2, 24, 40)):
        with pytest.raises(MvsHipError, match=r"^cv_aggregate: vis_weight must be \[B,V-1,H,W\]"):
            sweeps["cv_aggregate"](weight=bad)
    for y0, rows in ((-1, 4), (0, 25), (22, 3), (3, 0), (24, 1)):
        with pytest.raises(MvsHipError, match=r"^cv_corr_rows: rows \[-?\d+, \d+\) outside the image \(H = 24\)"):
            sweeps["cv_corr_rows"](y0=y0, rows=rows)
    assert calls == []
    ent = sweeps["cv_entropy"]()                               # the same operands unbroken: one launch of the dense entry, tag and work as before
    (name, tag, args), = calls
    assert name == "mvs_cv_entropy_fwd" and tag == ("cv_entropy_kernel<2>", "bytes", 4.0 * 24 * 40 * (3 * 8 + 4))
    assert args[:-1] == (feat.data_ptr(), rt.data_ptr(), depth.data_ptr(), 1, 3, 8, 8, 4, 24, 40, ent.data_ptr(), ops._cv_flags(None))


FAKE = 0x1000                                                  # a made-up address: the entries below return before reading any pointer
DENSE, BANK = (FAKE,), (FAKE, FAKE, 7)                         # feat | bank, view_idx, N
# entry -> (leading arguments up to the sizes, integers between W and the outputs, output pointers, which of them must not be null)
SWEEP_ENTRIES = {
    "mvs_cv_entropy_fwd": (DENSE + (FAKE, FAKE), (), 1, (0,)),
    "mvs_cv_entropy_fwd_views": (BANK + (FAKE, FAKE), (), 1, (0,)),
    "mvs_cv_aggregate_fwd": (DENSE + (FAKE, FAKE, FAKE), (), 2, (0,)),                 # volume; sim_depth is optional
    "mvs_cv_aggregate_fwd_bf16": (DENSE + (FAKE, FAKE, FAKE), (), 3, (0, 1)),          # volume, volume16
    "mvs_cv_aggregate_fwd_views": (BANK + (FAKE, FAKE, FAKE), (), 2, (0,)),
    "mvs_cv_corr_fwd": (DENSE + (FAKE, FAKE), (), 2, (0, 1)),                          # entropy, store
    "mvs_cv_corr_rows_fwd": (DENSE + (FAKE, FAKE), (0, 24), 2, (0, 1)),
    "mvs_cv_corr_rows_fwd_views": (BANK + (FAKE, FAKE), (0, 24), 2, (0, 1)),
}


@pytest.mark.parametrize("entry", sorted(SWEEP_ENTRIES))
def test_sweep_entries_refuse_a_null_output_under_their_own_name(entry):
    """Straight through ctypes: each of the eight sweep entries, called with one of its mandatory output pointers null, returns an error code
    and a message that begins with THAT entry's name (``mvs_cv_aggregate_fwd_bf16`` used to answer as ``mvs_cv_aggregate_fwd``).  The null
    check is every entry's first, so nothing is read and nothing is launched."""
    from mvsformer_amd import _lib
    lib = _lib.load()
    head, ints, nout, mandatory = SWEEP_ENTRIES[entry]
    for null_at in mandatory:
        outs = tuple(None if i == null_at else FAKE for i in range(nout))
        rc = getattr(lib, entry)(*head, 1, 3, 32, 8, 4, 24, 40, *ints, *outs, 0, None)        # B, V, C, G, D, H, W ... flags, stream
        assert rc != 0, (entry, null_at)
        assert lib.mvs_last_error().startswith(entry.encode() + b": null"), (entry, null_at, lib.mvs_last_error())
