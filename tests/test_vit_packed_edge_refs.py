"""CPU-side check of the references of tests/test_hip_vit_packed_edges.py (no GPU): every case of tests/vit_packed_edge_util.py is run through
its fp64 ``want`` and its fp32 twin ``ref32``.  For ``err(got) < 3 * err(ref32) + floor`` to mean something, ``err(ref32)`` must be finite,
non-zero and small and no row of ``want`` may be identically zero; ``exact`` cases (results that are elements of the input: K and V of the
0 / 1 selection weights, the attention output under one dominant key, a softmax over one key) have ``err(ref32) == 0``, asserted instead.
The rest pins what the case lists claim: which kernel instance each case reaches, what the score patterns do to the lazily raised softmax
reference, how far the GELU / Swish pre-activations reach, and which pixels the convolution geometries contain."""
import math

import torch

import test_hip_vit_edges as E
import vit_packed_edge_util as U


def test_every_case_has_a_meaningful_fp32_yardstick():
    n = exact = 0
    for out in U.all_case_outputs():
        n += 1
        assert out.want.dtype == torch.float64 and out.ref32.dtype == torch.float32, out.name
        assert bool(torch.isfinite(out.want).all()), out.name
        err32 = E.slice_err(out.ref32, out.want, out.kind)
        assert math.isfinite(err32) and err32 < 1e-4, (out.name, err32)
        assert E.zero_slices(out.want, out.kind) == 0, out.name
        if out.exact:
            exact += 1
            assert err32 == 0.0, (out.name, err32)
        else:
            assert err32 > 0.0, out.name
    assert n > 250 and exact * 6 < n, (n, exact)             # the marked cases stay the exception


def test_exact_cases_are_the_stated_closed_forms():
    for c in U.QA_CASES + U.QA_SWEEP:
        d = U.qa_case_cached(c)
        if c.pattern:                                        # k and v are columns of x; under pattern b every output row is the last key's V
            x = d.x[:, :c.N].double()
            assert torch.equal(d.k.want[:, 0, :, :32], x[..., 32:64]) and not d.k.want[..., 32:].any()
            assert torch.equal(d.v.want[:, 0], x[..., 64:]) and torch.equal(d.v.want[:, 1], x[..., 64:].flip(-1))
        if c.pattern == "b":
            assert torch.equal(d.att.want, d.v.want[:, :, c.N - 1:].expand_as(d.att.want))
            assert bool((d.cls.want[..., c.N - 1] == 1).all()) and float(d.cls.want[..., :c.N - 1].max()) < 1e-19      # one-hot
        if c.N == 1:
            assert bool((d.cls.want == 1).all())


def test_pack_values_and_the_split_model():
    """The round trip's claim on the CPU model of csrc/split3.h: h + m + l is v bit for bit from 2^-110 on, within 2^-126 below."""
    for R, K, ra in U.PACK_CASES:
        assert ra % 16 == 0 and ra >= R
        x = U.pack_case(R, K)
        for s in U.PACK_SPECIALS:
            assert bool((x == torch.tensor(s, dtype=torch.float64).float()).any()), s
        h, m, l = U.split3_model(x)
        assert bool(torch.isfinite(h).all())
        U.check_roundtrip(h + (m + l), x)
    assert {r for r, _, _ in U.PACK_CASES} == set(U.PACK_R) and {k for _, k, _ in U.PACK_CASES} == set(U.PACK_K)
    # below 2^-110 the l term really cannot hold the remainder: the bound of the header is not a formality
    v = torch.tensor([1.2345 * 2.0 ** -111], dtype=torch.float64).float()
    h, m, l = U.split3_model(v)
    assert not torch.equal(h + (m + l), v)
    # the order of the sum matters at the top of the range: for FLT_MAX h is the largest bf16, m rounds up to 2^120 and h + m is 2^128
    v = torch.tensor([3.4028234663852886e38], dtype=torch.float64).float()
    h, m, l = U.split3_model(v)
    assert torch.equal(h + (m + l), v) and bool(torch.isinf((h + m) + l).all())


def test_cases_name_the_instances_they_reach():
    seen, why = set(), set()
    for g in U.PG_CASES + U.CV_CASES:
        inst, reason = g.inst()
        assert inst in U.X3P_INSTANCES
        seen.add(inst), why.add(reason)
    for c in U.QA_CASES + [U.QA_BIG]:
        inst, _ = c.inst()
        assert inst in U.X3P_INSTANCES
        seen.add(inst)
    assert why == {"N<=64", "gelu+packed", "default", "fill"}
    assert {(0, 8, 64, 4, 2), (0, 8, 128, 8, 4), (0, 7, 128, 8, 1), (1, 8, 128, 8, 4), (1, 7, 128, 8, 1)} <= seen
    # the issue's 112-row shape: 120 blocks against 96, the last row block holds one row
    assert U.x3p_instance(0, 1009, 1536) == ((0, 7, 128, 8, 1), "fill") and 1009 % 112 == 1
    assert any(g.act == 1 and "P" in g.outs and g.N > 64 for g in U.PG_CASES)
    # the children's configurations and the defaults cover all thirteen instances
    parse = lambda mode, s: (mode,) + tuple(int(v) for v in s.split(","))
    for c0, c1 in U.CHILD_CFGS:
        assert parse(0, c0) in U.X3P_INSTANCES and parse(1, c1) in U.X3P_INSTANCES
        seen.add(parse(0, c0)), seen.add(parse(1, c1))
    assert len(U.X3P_INSTANCES) == 13
    assert seen == U.X3P_INSTANCES, U.X3P_INSTANCES - seen
    assert parse(0, U.NO_INSTANCE_CFG) not in U.X3P_INSTANCES
    for lst in (U.PG_CASES, U.PG_SWEEP, U.CV_CASES, U.CV_SWEEP, U.QA_CASES + U.QA_SWEEP):
        ids = [c.id() for c in lst]
        assert len(set(ids)) == len(ids)
    # the reduced sweeps cross the 112- or the 128-row seam in every case but the two smallest
    assert sum(g.M > 112 for g in U.PG_SWEEP) >= 7 and sum(c.M > 112 for c in U.CV_SWEEP) >= 7 and sum(c.images * c.Np > 112 for c in U.QA_SWEEP) >= 9


def test_case_lists_cover_the_stated_edges():
    assert {g.M for g in U.PG_CASES} >= set(U.PG_M) and {g.N for g in U.PG_CASES} >= set(U.PG_N) and {g.K for g in U.PG_CASES} >= set(U.PG_K) | {1536}
    for outs in ("C", "P", "CP"):
        assert any(g.outs == outs for g in U.PG_CASES) and any(c.outs == outs for c in U.CV_CASES)
    assert all(not g.res or "C" in g.outs for g in U.PG_CASES + U.PG_SWEEP)
    assert {(g.ss, g.act, g.res) for g in U.PG_CASES} == {(s, a, r) for s in (False, True) for a in (0, 1) for r in (False, True)}
    assert {(C, Np) for C, Np, _, _ in U.LNP_CASES} == {(C, Np) for C in U.LNP_C for Np, _ in U.LNP_NP_N} and {i for _, _, _, i in U.LNP_CASES} == {1, 3}
    plain = [c for c in U.QA_CASES if not c.pattern]
    assert {c.N for c in plain} >= set(U.QA_N) and {c.heads for c in plain} == {2, 4, 6} and {c.images for c in plain} >= {1, 3}
    assert {(c.N, c.Np) for c in plain} >= {(5, 64), (33, 128)} and {(c.images, c.Np) for c in plain} >= {(5, 32), (7, 32)}
    assert [c.pattern for c in U.QA_CASES if c.pattern] == list(U.QA_PATTERNS)
    for mode in (1, 2):
        cs = [c for c in U.CV_CASES if c.mode == mode]
        assert {(c.images, c.h, c.w) for c in cs} == set(U.CV_GEOM) and {c.Cp for c in cs} == {32, 64, 128} and {c.N for c in cs} == set(U.CV_N)
        assert {c.act for c in cs} == {0, 1, 2, 3} and {c.mul for c in cs} == {False, True}
    assert all(c.cin < c.Cp and c.rows_alloc() > c.M for c in U.CV_CASES + U.CV_SWEEP)


def test_score_patterns_do_what_they_claim():
    """In base-2 units, the units of the kernel's reference (it is raised when a score exceeds it by more than 8)."""
    case = {c.pattern: U.qa_case_cached(c) for c in U.QA_CASES if c.pattern}
    N = U.QA_PATTERN_N
    assert N % 32 == 1                                        # the last key alone in a partial tile
    s = case["b"].logits
    assert float((s[..., N - 1:] - s[..., :N - 1]).min()) >= 45
    rise = U.step_maxima(case["c"].logits).diff(dim=-1)
    assert float(rise.min()) > 6 and float(rise.max()) < 8
    assert float(U.step_maxima(case["d"].logits).diff(dim=-1).min()) > 8
    s = case["e"].logits
    assert bool((s.argmax(-1) == 0).all()) and float(U.step_maxima(s).diff(dim=-1).max()) < 0
    assert float(case["f"].logits.min()) > 70
    # the ordinary cases stay ordinary: no logit beyond +-60
    assert float(case["a"].logits.abs().max()) < 60


def test_epilogue_preactivations_cover_both_tails():
    """GELU (act 1) and Swish (act 2): pre-activations beyond +-12 on both sides."""
    n = 0
    for d in [U.pg_case(g) for g in U.PG_CASES + U.PG_SWEEP] + [U.cv_case(c) for c in U.CV_CASES + U.CV_SWEEP]:
        act = d.g.act if hasattr(d, "g") else d.c.act
        if act in (1, 2):
            n += 1
            assert d.pre.min() < -12 and d.pre.max() > 12, (d.out.name, float(d.pre.min()), float(d.pre.max()))
    assert n >= 20


def test_conv_geometries_contain_the_claimed_pixels():
    geoms = {(c.images, c.h, c.w) for c in U.CV_CASES}
    # a pixel whose eight neighbour taps all lie outside the image (the centre tap never does): the one-pixel map
    assert (1, 1, 1) in geoms
    # tap by tap: within ONE geometry, a pixel with that tap outside the image and a pixel with it inside (the x = 0 / x = w - 1 and y = 0 /
    # y = h - 1 edges: a gather that wrapped to the neighbouring row, or read the neighbouring image, would return a real pixel there)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dy, dx) == (0, 0):
                continue
            both = [g for g in geoms if {0 <= y + dy < g[1] and 0 <= x + dx < g[2] for y in range(g[1]) for x in range(g[2])} == {False, True}]
            assert any(w >= 2 and i >= 2 for i, _, w in both) if dx else both, (dy, dx)
    # a 128-row block seam strictly inside an image, not at a row start; and M = 128 exactly (the zero row is then row 128)
    inside = [(i, h, w) for i, h, w in geoms if i * h * w > 128 and 128 % (h * w) != 0 and (128 % (h * w)) % w != 0]
    assert (2, 12, 12) in inside and (3, 4, 11) in inside
    assert any(i * h * w == 128 for i, h, w in geoms)
    # the same for the 112-row seam of the forced instances
    assert any(c.M > 112 and 112 % (c.h * c.w) != 0 for c in U.CV_SWEEP)
