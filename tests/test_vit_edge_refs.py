"""CPU-side check of the references of tests/test_hip_vit_edges.py: every parametrised case of that module is run through its fp64 ``want`` and
its fp32 twin ``ref32`` only (no GPU).  For the bound ``err(got) < 3 * err(ref32) + 2e-7`` to mean something, ``err(ref32)`` must be finite,
non-zero and small (< 1e-4) and no slice of ``want`` may be identically zero; the marked exceptions (``exact`` results, structurally unread
rows of the bicubic adjoint) are explained in that module's docstring and pinned here: an ``exact`` case has ``err(ref32) == 0``."""
import math

import torch

import test_hip_vit_edges as E


def test_every_case_has_a_meaningful_fp32_yardstick():
    n = exact = 0
    for out in E.all_case_outputs():
        n += 1
        assert out.want.dtype == torch.float64 and out.ref32.dtype == torch.float32, out.name
        assert bool(torch.isfinite(out.want).all()), out.name
        err32 = E.slice_err(out.ref32, out.want, out.kind)
        assert math.isfinite(err32) and err32 < 1e-4, (out.name, err32)
        zeros = E.zero_slices(out.want, out.kind)
        if out.exact:
            exact += 1
            assert err32 == 0.0, (out.name, err32)
        else:
            assert err32 > 0.0, out.name
            assert zeros == 0 or out.zero_ok, (out.name, zeros)
    assert n > 500 and exact * 6 < n                          # the marked cases stay the exception


def test_exact_cases_are_the_stated_closed_forms():
    for rows in E.LN_ROWS:                                    # LayerNorm over one feature: y = beta, dx = 0, dx + res = res
        d = E.ln_case(1, rows)
        assert torch.equal(d.y.want, d.beta.double().expand(rows, 1)) and not d.dx.want.any() and torch.equal(d.dx_res.want, d.res.double())
    for rows in E.SM_ROWS:
        for scale in E.SM_SCALES:
            for kind in E.SM_KINDS:
                assert bool((E.softmax_case(1, rows, scale, kind).want == 1).all())
    for BH in E.SB_BH:
        for da in E.SB_DA:
            assert not E.softmax_bwd_case(1, BH, da).out.want.any()
    for C in E.CS_C:
        d = E.colsum_case(1, C)
        assert torch.equal(d.plain.want, d.dy.double()[0]) and torch.equal(d.dbeta.want, d.dy.double()[0])
    for planes in E.BC_PLANES:
        d = E.bicubic_case(E.BC_CASES[0], planes)
        assert torch.equal(d.y.want.reshape(-1), d.x.double().reshape(-1)) and torch.equal(d.dx.want.reshape(-1), d.dy.double().reshape(-1))
    for B, NH in E.AT_BH:
        d = E.attention_case(B, NH, 1)
        C = NH * 64
        assert torch.equal(d.want.reshape(B, C), d.qkv[:, 0, 2 * C:].double())
    B, NH, N, _ = E.AT_PEAKED
    d = E.attention_case(*E.AT_PEAKED)
    v_last = d.qkv[:, N - 1, 2 * NH * 64:].double().reshape(B, NH, 1, 64)
    assert torch.equal(d.want, v_last.expand(B, NH, N, 64))


def test_gemm_cases_reach_all_four_instances():
    """``gemm_instance`` restates ``launch_gemm``; every case names the instance it reaches and all four are reached."""
    seen = set()
    for g in E.GEMM_CASES + E.EPILOGUE_CASES:
        assert E.gemm_instance(g) == g.inst, g.id()
        seen.add(g.inst)
    assert seen == {"fast<1>", "fast<2>", "general<1>", "general<2>"}
    ids = [g.id() for g in E.GEMM_CASES + E.EPILOGUE_CASES]
    assert len(set(ids)) == len(ids)


def test_epilogue_preactivations_cover_both_tails():
    """GELU (act 1) and Swish (act 2): pre-activations beyond +-12 on both sides."""
    for g in E.EPILOGUE_CASES:
        if g.act in (1, 2):
            pre = E.gemm_case(g).pre
            assert pre.min() < -12 and pre.max() > 12, (g.id(), float(pre.min()), float(pre.max()))


def test_cases_exercise_what_they_claim():
    # the bicubic adjoint at strong down-sampling really has inputs that no output reads, and nowhere else
    for case in E.BC_CASES:
        for planes in E.BC_PLANES:
            d = E.bicubic_case(case, planes)
            zeros = E.zero_slices(d.dx.want, "row")
            assert (zeros > 0) == (case[:4] in ((16, 16, 3, 5), (14, 14, 1, 37), (5, 4, 1, 1))), (case, zeros)
    # GELU: the special points are in, and x reaches both ends of [-12, 12]
    d = E.gelu_case(100003)
    assert all(bool((d.x == p).any()) for p in E.GELU_POINTS) and d.x[6:].min() < -11.99 and d.x[6:].max() > 11.99
    # the peaked attention row: the last key's logit is at least 45 above every other one
    B, NH, N, _ = E.AT_PEAKED
    q = E.attention_case(*E.AT_PEAKED).qkv.double()
    C = NH * 64
    for h in range(NH):
        s = q[:, :, h * 64:(h + 1) * 64] @ q[:, :, C + h * 64:C + (h + 1) * 64].transpose(-1, -2) / 8
        assert float((s[..., N - 1:] - s[..., :N - 1]).min()) > 45
    # the peaked / shifted softmax rows
    x = E.softmax_case(257, 5, 0.125, "peaked").x.double() * 0.125
    top = x.topk(2, -1).values
    assert float((top[:, 0] - top[:, 1]).min()) >= 60 - 1e-4
    assert float((E.softmax_case(257, 5, 1.0, "shifted").x).min()) > 70
