"""The packed ViT inference kernels (csrc/vit_packed.hip: ``x3p_pack`` / ``x3p_unpack``, ``layernorm_x3p``, ``gemm_x3p`` in its default
instances, ``gemm_x3p_qkv`` -> ``attention_x3p`` / ``cls_attention_x3p``, ``conv_x3p``, and in child processes the instances the default never
picks) against fp64 at tile, block and image edges, with the PER-ROW metric and the bound of tests/test_hip_vit_edges.py:
``err(got) < 3 * err(ref32) + 2e-7`` (``+ 5e-7`` for the attention output and the CLS row), a slice = one token / pixel / CLS row.

The cases and their fp64 / fp32 references are built on the CPU by tests/vit_packed_edge_util.py and checked without a GPU by
tests/test_vit_packed_edge_refs.py.  Besides the values every test checks the memory a kernel does not own: fp32 outputs have a row stride of
N + 4 and are pre-filled with 777.25, packed outputs are pre-filled with the byte 0x5A, and the gap columns, the rows beyond M and the rows
beyond the last image must come back untouched; inputs that must not be read (LayerNorm's padding rows, the attention's padding keys) hold
NaN / 1e30 / values of magnitude 1e3.

``layernorm_x3p`` and ``cls_attention_x3p`` are held to the same per-row contract as the GEMMs (before this module they had whole-tensor
bounds of 2e-6 and 5e-6 only); the ratios ``check`` prints are the record."""
import os
import subprocess
import sys

import pytest
import torch

import vit_packed_edge_util as U
from test_hip_vit_edges import FACTOR, FLOOR, FLOOR_ATT, Out, check, slice_err, zero_slices          # noqa: F401

pytestmark = pytest.mark.gpu
HERE = os.path.abspath(__file__)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ops():
    from mvsformer_amd import ops
    return ops


def _err():
    from mvsformer_amd import _lib
    return _lib.MvsHipError


def _opt(t, dev):
    return None if t is None else t.to(dev)


SLACK = 4096                                                 # bytes behind a sentinel-filled packed matrix that must stay untouched as well


def _packed_sentinel(rows, K, dev, rows_alloc):
    p = _ops().Packed(rows, K, dev, rows_alloc=rows_alloc)
    p.buf = torch.full((p.buf.numel() + SLACK,), U.SENTINEL_BYTE, device=dev, dtype=torch.uint8)
    return p


def _assert_rows_untouched(p, first, what):
    raw = U.packed_rows(p.buf, p.rows_alloc, p.K)
    assert bool((raw[first:] == U.SENTINEL_BYTE).all()), "%s: wrote packed rows >= %d" % (what, first)
    tail = p.buf.cpu()[p.rows_alloc // 16 * (p.K // 32) * 3072:]
    assert tail.numel() == SLACK and bool((tail == U.SENTINEL_BYTE).all()), "%s: wrote behind the packed matrix" % what


def _check_outputs(ops, C, outp, rows, N, out, what):
    """The tail gemm_x3p and conv_x3p share: C's gap columns and spare row keep the sentinel, packed rows >= ``rows`` are untouched, the
    unpacked packed output is C (the same bits; a GELU's -0 comes back from the split as +0), and the values meet the bound."""
    got = None
    if C is not None:
        Cc = C.cpu()
        assert bool((Cc[:, N:] == U.SENTINEL).all()) and bool((Cc[rows] == U.SENTINEL).all()), "%s wrote outside C (gap columns / past the last row)" % what
        got = Cc[:rows, :N]
    if outp is not None:
        _assert_rows_untouched(outp, rows, what)
        unp = ops.x3p_unpack(outp).cpu()
        if got is not None:
            assert torch.equal(unp, got), "%s: packed output differs from C" % what
            assert torch.equal(unp[got != 0].view(torch.int32), got[got != 0].view(torch.int32))
        got = unp
    check(got, out)


# ---------------------------------------------------------------------------------------------------------------- 1. pack / unpack
@pytest.mark.parametrize("R,K,ra", U.PACK_CASES)
def test_x3p_pack_unpack_roundtrip(dev, R, K, ra):
    """Bit-exact for every |v| >= 2^-110 (FLT_MAX and the values around the largest bf16 included), within 2^-126 below; rows R .. rows_alloc
    are zero bytes in all three terms; the terms themselves are the CPU model's, bit for bit."""
    ops = _ops()
    x = U.pack_case(R, K)
    p = ops.x3p_pack(x.to(dev), rows_alloc=ra)
    assert p.rows_alloc == ra and p.buf.numel() == ra // 16 * (K // 32) * 3072
    got = ops.x3p_unpack(p).cpu()
    U.check_roundtrip(got, x)
    raw = U.packed_rows(p.buf, ra, K)
    assert not raw[R:].any(), "rows beyond R are not zero bytes"
    terms = raw[:R].reshape(R, K // 32, 3, 4, 16).contiguous().view(torch.bfloat16).reshape(R, K // 32, 3, 4, 8).permute(2, 0, 1, 3, 4).reshape(3, R, K)
    normal = x.abs() >= 2.0 ** -100                          # (every term a normal bf16 or zero: no dependence on how subnormals convert)
    for got_t, want_t in zip(terms.float(), U.split3_model(x)):
        assert torch.equal(got_t[normal], want_t[normal])


# ---------------------------------------------------------------------------------------------------------------- 2. LayerNorm -> packed
@pytest.mark.parametrize("C,Np,N,images", U.LNP_CASES)
def test_layernorm_x3p_rows_vs_fp64(dev, C, Np, N, images):
    ops = _ops()
    d = U.lnp_case(C, Np, N, images)
    rows = images * Np
    out = _packed_sentinel(rows, C, dev, rows + 16)
    x, g, b = d.x.to(dev), d.gamma.to(dev), d.beta.to(dev)
    ops.layernorm_x3p(x, g, b, U.LNP_EPS, Np, N, out=out)
    got = ops.x3p_unpack(out).cpu()
    check(got[d.valid], d.y)
    raw = U.packed_rows(out.buf, out.rows_alloc, C)
    assert not raw[:rows][~d.valid].any(), "padding rows t >= N are not zero bytes"
    _assert_rows_untouched(out, rows, "layernorm_x3p")
    again = ops.layernorm_x3p(x, g, b, U.LNP_EPS, Np, N)
    assert torch.equal(ops.x3p_unpack(again).cpu(), got)


# ---------------------------------------------------------------------------------------------------------------- 3. gemm_x3p
def _run_pgemm(dev, g):
    ops = _ops()
    d = U.pg_case(g)
    M, N = g.M, g.N
    Ap = ops.x3p_pack(d.A.to(dev), rows_alloc=U.up(M, 16) if g.tight else None)
    Bp = ops.x3p_pack(d.B.to(dev), rows_alloc=U.up(N, 16) if g.tight else None)
    C = torch.full((M + 1, N + 4), U.SENTINEL, device=dev) if "C" in g.outs else None
    outp = _packed_sentinel(M, N, dev, Ap.rows_alloc + 16) if "P" in g.outs else None      # (the contract: at least A's allocation)
    ops.gemm_x3p(Ap, Bp, N, C=None if C is None else C[:M], scale=_opt(d.scale, dev), shift=_opt(d.shift, dev), act=g.act, res=_opt(d.res, dev), out=outp)
    _check_outputs(ops, C, outp, M, N, d.out, "gemm_x3p")


@pytest.mark.parametrize("g", U.PG_CASES, ids=U.PG.id)
def test_gemm_x3p_edges_vs_fp64(dev, g):
    """The default instances of ``launch_pgemm`` (the id names the one each case reaches and why; see ``x3p_instance``)."""
    assert os.environ.get("MVS_X3P_CFG") is None and os.environ.get("MVS_X3P_CFG_QKV") is None       # x3p_instance() describes the defaults
    _run_pgemm(dev, g)


# ---------------------------------------------------------------------------------------------------------------- 4. qkv -> attention, CLS row
def _qkv_attention(dev, c, x, W, bias):
    """One zero-copy pass: returns (q, k, v, att, cls) on the CPU: q / k / v ``[images][heads][Np][64]`` in key order, att ``[images][Np][C]``."""
    ops = _ops()
    B, NH, Np, C = c.images, c.heads, c.Np, c.heads * 64
    xp, wp = ops.x3p_pack(x.reshape(B * Np, C).to(dev), rows_alloc=B * Np), ops.x3p_pack(W.to(dev))
    qkv = ops.gemm_x3p_qkv(xp, wp, _opt(bias, dev), B, Np, NH, U.SCALE)

    def unpack(buf, rows, K):
        p = ops.Packed(rows, K, dev, rows_alloc=rows)
        assert p.buf.numel() == buf.numel()
        p.buf = buf
        return ops.x3p_unpack(p).cpu()

    q, k = unpack(qkv.q, B * NH * Np, 64).reshape(B, NH, Np, 64), unpack(qkv.k, B * NH * Np, 64).reshape(B, NH, Np, 64)
    v = U.vt_unpermute(unpack(qkv.vt, B * NH * 64, Np).reshape(B, NH, 64, Np)).transpose(-1, -2)
    out = _packed_sentinel(B * Np, C, dev, B * Np + 16)
    ops.attention_x3p(qkv, c.N, out=out)
    _assert_rows_untouched(out, B * Np, "attention_x3p")
    att = ops.x3p_unpack(out).cpu().reshape(B, Np, C)
    got_cls = ops.cls_attention_x3p(qkv, c.N).cpu()
    assert got_cls.shape == (B, NH, c.N)
    return q, k, v, att, got_cls


def _heads(att, c):
    return att.reshape(c.images, c.Np, c.heads, 64).permute(0, 2, 1, 3)


def _run_qa(dev, d, mask_check=True):
    c = d.c
    N = c.N
    q, k, v, att, cls = _qkv_attention(dev, c, d.x, d.W, d.bias)
    check(q[:, :, :N], d.q), check(k[:, :, :N], d.k), check(v[:, :, :N], d.v)
    if c.pattern:                                             # a 0 / 1 W: K and V are elements of x, exactly
        assert torch.equal(k[:, :, :N].double(), d.k.want) and torch.equal(v[:, :, :N].double(), d.v.want)
    a = _heads(att, c)
    assert bool(torch.isfinite(att).all()), "output rows in [N, Np) must be finite"
    check(a[:, :, :N] if d.rows is None else a[:, :, d.rows], d.att, floor=FLOOR_ATT)
    check(cls, d.cls, floor=FLOOR_ATT)
    assert float((cls.double().sum(-1) - 1).abs().max()) < 1e-5
    if c.pattern == "b":                                      # one key 50 above the rest: that key's V, and a one-hot CLS row
        assert torch.equal(a[:, :, :N].double(), d.att.want)
        assert bool((cls[..., N - 1] == 1).all()) and float(cls[..., :N - 1].max()) < 1e-19
    if mask_check and N < c.Np:                               # what lies in the padding rows cannot reach rows < N
        gen = torch.Generator().manual_seed(N)
        x2 = d.x.clone()
        x2[:, N:] = (torch.rand(x2[:, N:].shape, generator=gen) + 0.5) * 1e3 * torch.sign(torch.randn(x2[:, N:].shape, generator=gen))
        q2, k2, v2, att2, cls2 = _qkv_attention(dev, c, x2, d.W, d.bias)
        assert float(k2[:, :, N:].abs().max()) > 10            # (the padding keys really differ)
        assert torch.equal(att2[:, :N].view(torch.int32), att[:, :N].view(torch.int32)), "padding keys leak into rows < N"
        assert torch.equal(cls2.view(torch.int32), cls.view(torch.int32)), "padding keys leak into the CLS row"
        assert torch.equal(q2[:, :, :N], q[:, :, :N]) and torch.equal(k2[:, :, :N], k[:, :, :N]) and torch.equal(v2[:, :, :N], v[:, :, :N])


@pytest.mark.parametrize("c", U.QA_CASES, ids=U.QA.id)
def test_qkv_attention_cls_edges_vs_fp64(dev, c):
    assert os.environ.get("MVS_X3P_CFG_QKV") is None
    _run_qa(dev, U.qa_case_cached(c))


def test_attention_cls_at_the_cls_kernel_limit(dev):
    """N = Np = 8192, the CLS kernel's score array full: the CLS row and 32 query rows (first, last, random) against fp64; N = 8193 is refused."""
    ops = _ops()
    d = U.qa_big_case()
    _run_qa(dev, d, mask_check=False)
    big = ops.QkvPacked(1, 2, 8192 + 32, dev)
    with pytest.raises(_err()):
        ops.cls_attention_x3p(big, 8193)


# ---------------------------------------------------------------------------------------------------------------- 5. conv_x3p
def _run_conv(dev, c):
    ops = _ops()
    d = U.cv_case(c)
    M, N, R = c.M, c.N, c.rows_out()
    xp = ops.x3p_pack(d.xcl.to(dev), rows_alloc=c.rows_alloc())
    wra = U.up(N, 16) if c.spare16 else U.up(N, 128)
    wp = ops.x3p_pack(d.Wm.to(dev), rows_alloc=wra) if c.mode == 1 else ops.x3p_pack_classes(d.Wm.to(dev), wra)
    C = torch.full((R + 1, N + 4), U.SENTINEL, device=dev) if "C" in c.outs else None
    outp = _packed_sentinel(R, N, dev, U.up(R, 16) + 16) if "P" in c.outs else None
    mul = _opt(d.mul, dev)
    if mul is not None and C is None:                         # without C the kernel's row stride is N
        mul = mul[:, :N].contiguous()
    ops.conv_x3p(xp, wp, c.mode, c.images, c.h, c.w, N, C=None if C is None else C[:R], scale=_opt(d.scale, dev), shift=_opt(d.shift, dev), act=c.act,
                 mul=mul, out=outp)
    _check_outputs(ops, C, outp, R, N, d.out, "conv_x3p")


@pytest.mark.parametrize("c", U.CV_CASES, ids=U.CV.id)
def test_conv_x3p_edges_vs_fp64(dev, c):
    assert os.environ.get("MVS_X3P_CFG") is None
    _run_conv(dev, c)


# ---------------------------------------------------------------------------------------------------------------- 6. instances the default never picks
# MVS_X3P_CFG / MVS_X3P_CFG_QKV are read once per process: the reduced sweeps below run here under the default instances and once more per
# forced configuration in a fresh child pytest process (one after another; a child that hangs or dies on a signal ends the series).
@pytest.mark.parametrize("g", U.PG_SWEEP, ids=U.PG.id)
def test_sweep_gemm(dev, g):
    _run_pgemm(dev, g)


@pytest.mark.parametrize("c", U.CV_SWEEP, ids=U.CV.id)
def test_sweep_conv(dev, c):
    _run_conv(dev, c)


@pytest.mark.parametrize("c", U.QA_SWEEP, ids=U.QA.id)
def test_sweep_qkv_attention(dev, c):
    _run_qa(dev, U.qa_case_cached(c))


_CHILD_TROUBLE = []
CHILD_TIMEOUT = 300                                          # 30 small cases and the imports take about 20 s


def _child(args, cfg0, cfg1):
    if _CHILD_TROUBLE:
        pytest.skip("an earlier child process hung or died (%s): no further children are started" % _CHILD_TROUBLE[0])
    env = dict(os.environ, MVS_X3P_CFG=cfg0, MVS_X3P_CFG_QKV=cfg1)
    try:
        r = subprocess.run([sys.executable] + args, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _CHILD_TROUBLE.append("%s timed out" % cfg0)
        pytest.fail("child %s / %s timed out" % (cfg0, cfg1))
    if r.returncode < 0 or r.returncode >= 128:
        _CHILD_TROUBLE.append("%s ended with status %d" % (cfg0, r.returncode))
        pytest.fail("child %s / %s ended with status %d\n%s" % (cfg0, cfg1, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return r


@pytest.mark.parametrize("cfg0,cfg1", U.CHILD_CFGS)
def test_forced_instances_in_a_child(dev, cfg0, cfg1):
    r = _child(["-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", HERE, "-k", "test_sweep_"], cfg0, cfg1)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "%d passed" % (len(U.PG_SWEEP) + len(U.CV_SWEEP) + len(U.QA_SWEEP)) in r.stdout, r.stdout[-1000:]


def _no_instance_body():
    """Runs in a child with MVS_X3P_CFG = MVS_X3P_CFG_QKV = "8,32,4,1": both forms must refuse, and launch nothing."""
    ops, dev = _ops(), torch.device("cuda:0")
    A, B = ops.x3p_pack(torch.ones(16, 32, device=dev)), ops.x3p_pack(torch.ones(128, 32, device=dev))
    C = torch.full((16, 128), U.SENTINEL, device=dev)
    for call in (lambda: ops.gemm_x3p(A, B, 128, C=C), lambda: ops.gemm_x3p_qkv(ops.x3p_pack(torch.ones(32, 128, device=dev)), ops.x3p_pack(torch.ones(384, 128, device=dev)), None, 1, 32, 2, 0.125)):
        try:
            call()
        except _err() as e:
            assert "no kernel instance" in str(e), e
        else:
            raise AssertionError("a configuration without an instance was accepted")
    assert bool((C == U.SENTINEL).all())
    print("refused-ok")


def test_configuration_without_an_instance_is_refused(dev):
    code = "import sys; sys.path[:0] = [%r, %r]; import test_hip_vit_packed_edges as T; T._no_instance_body()" % (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE)))
    r = _child(["-c", code], U.NO_INSTANCE_CFG, U.NO_INSTANCE_CFG)
    assert r.returncode == 0 and "refused-ok" in r.stdout, (r.stdout + r.stderr)[-3000:]


# ---------------------------------------------------------------------------------------------------------------- 7. refusals (no kernel is launched)
def test_refusals(dev):
    ops, E = _ops(), _err()
    ones = lambda *s: torch.ones(*s, device=dev)
    A, B = ops.x3p_pack(ones(16, 32)), ops.x3p_pack(ones(64, 32))
    C = torch.full((16, 64), U.SENTINEL, device=dev)

    def forged(rows, K, like):                               # a Packed whose stated K the constructor would refuse
        p = ops.Packed(rows, like, dev)
        p.K = K
        return p

    refused = [
        lambda: ops.x3p_pack(ones(16, 40)),                                                   # K % 32 != 0
        lambda: ops.gemm_x3p(forged(16, 40, 64), forged(64, 40, 64), 64, C=C),                # ... at the entry point itself
        lambda: ops.gemm_x3p(A, B, 62, C=C),                                                  # N % 4 != 0
        lambda: ops.gemm_x3p(A, B, 36, C=C, out=forged(16, 36, 64)),                          # a packed output with N % 32 != 0
        lambda: ops.gemm_x3p(A, B, 64, res=ones(16, 64), out=ops.Packed(16, 64, dev)),        # res without C
        lambda: ops.gemm_x3p(A, B, 64, C=C, act=2),                                           # act 2 belongs to conv_x3p
        lambda: ops.layernorm_x3p(ones(16, 16), ones(16), ones(16), 1e-6, 16, 16, out=forged(16, 16, 32)),        # C = 16
        lambda: ops.layernorm_x3p(ones(16, 544), ones(544), ones(544), 1e-6, 16, 16),         # C = 544
        lambda: ops.layernorm_x3p(ones(48, 64), ones(64), ones(64), 1e-6, 24, 20),            # Np = 24
        lambda: ops.layernorm_x3p(ones(32, 64), ones(64), ones(64), 1e-6, 32, 33),            # N > Np
        lambda: ops.gemm_x3p_qkv(ops.x3p_pack(ones(32, 192)), ops.x3p_pack(ones(576, 192)), None, 1, 32, 3, 0.125),       # C = 192
        lambda: ops.gemm_x3p_qkv(ops.x3p_pack(ones(48, 128)), ops.x3p_pack(ones(384, 128)), None, 1, 48, 2, 0.125),       # Np = 48
        lambda: ops.attention_x3p(ops.QkvPacked(1, 2, 48, dev), 40),                          # Np = 48
        lambda: ops.conv_x3p(ops.x3p_pack(ones(16, 32), rows_alloc=16), ops.x3p_pack(ones(16, 288)), 1, 1, 4, 4, 16, C=ones(16, 16)),   # no spare row
    ]
    for i, call in enumerate(refused):
        with pytest.raises(E):
            call()
            pytest.fail("refusal %d was accepted" % i)
    torch.cuda.synchronize()
    assert bool((C == U.SENTINEL).all())
