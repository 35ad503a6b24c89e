"""The fp32 training convolutions - ``conv3d_kernel`` in its four tile forms (csrc/conv3d_fwd.hip), ``deconv3d_kernel`` (csrc/conv3d.hip),
``wino_conv3d_kernel`` with one and two N tiles (csrc/conv3d_wino.hip), ``wgrad_tiled_kernel`` with single-tile and multi-tile blocks and the
first ``wgrad_kernel`` (csrc/wgrad.hip) - through ``mvsformer_amd.ops`` against float64, element by element, at tile edges.  Cases, plans
(read from the launchers' planner), references and the derivation of the bounds: ``tests/conv3d_f32_edge_util.py``; that the cases reach what they claim and that the
bounds reject the mutations: ``tests/test_conv3d_f32_edge_refs.py`` (CPU); the runner and the guard planes: ``tests/conv3d_f32_edge_child.py``.

MVS_CONV_TILE is read once per process: the forms it forces run in one fresh child process each; everything else runs here, where the
dispatcher's own choice (read back by ``plan_conv``) reaches all four forms.  MVS_WINO_NT and MVS_WGRAD_V1 are read per call.

Every check prints ``F32EDGE family case max|err| ratio`` (ratio = the largest |err| / bound over ALL elements).  Largest ratio per family
when recorded on an MI355X:
    conv3d_kernel   2x2x64 0.021 (forced) / 0.014 (by the model), 4x2x64 0.023 / 0.016, 2x2x64 split 0.017 (model only), 2x2x32 split 0.014 / 0.020
    deconv3d_kernel sd 1 0.090, sd 2 0.317 (even-parity voxels sum Cin terms only: the bound is tightest there)
    Winograd        NT 1 0.014, NT 2 0.014
    dW              tiled 0.029, first kernel 0.045
    ConvFn / DeconvFn through autograd: y 0.077, dX 0.054 (deconv3d_kernel; 0.005 through the direct and Winograd kernels), dW 0.006
    every integer-operand case exact; no guard plane written, no NaN read.
The bounds are worst-case (every rounding at its maximum, all of one sign) while the errors of K random roundings grow like sqrt(K): a
ratio of 0.01 .. 0.3 is what a correct kernel shows, and every mutation of the refs test lies above 1."""
import os
import subprocess
import sys

import pytest
import torch

import conv3d_f32_edge_child as R
import conv3d_f32_edge_util as U

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv3d_f32_edge_child.py")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert os.environ.get("MVS_CONV_TILE") is None             # plan_conv(force=None) describes what runs in this process
    return torch.device("cuda:0")


def _ops():
    from mvsformer_amd import ops
    return ops


def _names(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------------------------- direct conv
@pytest.mark.parametrize("name", _names(U.DEFAULT_CASES))
def test_conv_default_dispatch_vs_fp64(dev, name):
    """The dispatcher's own choice: the 32-voxel form at its edges, the three 64-voxel forms where the model picks them by itself, the
    epilogue in all eight combinations, the "dgrad" pack, integer operands exact."""
    R.run_layer(_ops(), dev, U.CASE[name])


_CHILD_TROUBLE = []
CHILD_TIMEOUT = 240                                          # ~50 small cases and the imports take about 15 s


def _child(force):
    if _CHILD_TROUBLE:
        pytest.skip("an earlier child process hung or died (%s): no further children are started" % _CHILD_TROUBLE[0])
    env = dict(os.environ, MVS_CONV_TILE=force)
    try:
        r = subprocess.run([sys.executable, CHILD], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _CHILD_TROUBLE.append("%s timed out" % force)
        pytest.fail("child MVS_CONV_TILE=%s timed out" % force)
    if r.returncode not in (0, 1):                            # 1 = a case outside its bound; anything else (a signal, a HIP error: 3) = died
        _CHILD_TROUBLE.append("%s ended with status %d" % (force, r.returncode))
        pytest.fail("child MVS_CONV_TILE=%s ended with status %d\n%s" % (force, r.returncode, (r.stdout + r.stderr)[-3000:]))
    return r


@pytest.mark.parametrize("force", U.CHILD_FORMS)
def test_conv_forced_form_in_a_child(dev, force):
    """All cases of one forced tile form (its Wo / Ho / Do / stride / channel edges, the "dgrad" twins, the integer case; for 42 also
    the two fall-backs to the model) in one fresh process."""
    r = _child(force)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "%d cases ok (MVS_CONV_TILE=%s)" % (len(U.forced_cases(force)), force) in r.stdout, r.stdout[-1000:]


# ------------------------------------------------------------------------------------------------------------------- deconv
@pytest.mark.parametrize("name", _names(U.DECONV_CASES))
def test_deconv_vs_fp64(dev, name):
    R.run_layer(_ops(), dev, U.CASE[name])


# ------------------------------------------------------------------------------------------------------------------- Winograd
@pytest.mark.parametrize("name", _names(U.WINO_CASES))
def test_wino_vs_fp64(dev, monkeypatch, name):
    c = U.CASE[name]
    if c.force is None:
        monkeypatch.delenv("MVS_WINO_NT", raising=False)
    else:
        monkeypatch.setenv("MVS_WINO_NT", c.force)
    R.run_layer(_ops(), dev, c)


# ------------------------------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("name", _names(U.WG_EDGE_CASES + U.WG_MULTI_CASES))
def test_wgrad_tiled_vs_fp64(dev, monkeypatch, name):
    monkeypatch.delenv("MVS_WGRAD_V1", raising=False)
    R.run_wgrad(_ops(), dev, U.WG_CASE[name], "dW-tiled")


@pytest.mark.parametrize("name", _names(U.WG_V1_CASES))
def test_wgrad_v1_vs_fp64(dev, monkeypatch, name):
    monkeypatch.setenv("MVS_WGRAD_V1", "1")
    R.run_wgrad(_ops(), dev, U.WG_CASE[name], "dW-v1")


# ------------------------------------------------------------------------------------------------------------------- autograd routing
def _route_check(family, name, got, ref, bound):
    err, ratio = U.share(got.detach().cpu(), ref, bound)
    print("F32EDGE %-12s %-44s err %.3e  ratio %.3f" % (family, name, err, ratio))
    assert ratio <= 1.0, (name, ratio, err)


def _spy(ops, monkeypatch):
    seen = []
    for fn in ("conv3d", "conv3d_wino", "deconv3d"):
        orig = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, (lambda o, f: lambda *a, **k: (seen.append(f), o(*a, **k))[1])(orig, fn))
    return seen


@pytest.mark.parametrize("name", [c.name for c in U.ROUTE_CASES if c.kind == "conv"])
def test_conv_fn_routes_vs_fp64(dev, monkeypatch, name):
    """``ConvFn`` forward, dX and dW against float64 autograd within the kernels' bounds; which wrapper ran is observed, not assumed."""
    from mvsformer_amd import autograd as A
    ops, F = _ops(), torch.nn.functional
    monkeypatch.delenv("MVS_WINO_NT", raising=False)
    monkeypatch.delenv("MVS_WGRAD_V1", raising=False)
    monkeypatch.delenv("MVS_CONV_WINO", raising=False)
    c = U.CASE[name]
    t = U.case_inputs(c)
    seen = _spy(ops, monkeypatch)
    x, w = t["x"].to(dev).requires_grad_(True), t["w"].to(dev).requires_grad_(True)
    y = A.ConvFn.apply(x, w, c.stride)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
    y.backward(dy.to(dev))
    x64, w64 = t["x"].double().requires_grad_(True), t["w"].double().requires_grad_(True)
    s3 = (c.stride[0], c.stride[1], c.stride[1])
    y64 = F.conv3d(x64, w64, None, stride=s3, padding=1)
    y64.backward(dy.double())
    assert seen == list(U.ROUTES[name]), seen
    if seen[0] == "conv3d_wino":
        Ky, Sy = U.terms(c._replace(kind="wino")), U.wino_pipeline(t["x"], t["w"], absolute=True)
    else:
        Ky, Sy = 27.0 * c.cin, F.conv3d(t["x"].double().abs(), t["w"].double().abs(), None, stride=s3, padding=1)
    _route_check("ConvFn", name + " y", y, y64.detach(), U.C_ACC * Ky * U.U32 * Sy)
    Do, Ho, Wo = y.shape[2:]
    back = c._replace(cin=c.cout, cout=c.cin, D=Do, H=Ho, W=Wo)          # the layer the data gradient runs: dY in, Cin channels out
    if seen[1] == "conv3d_wino":
        Kx, Sx = U.terms(back._replace(kind="wino")), U.wino_pipeline(dy, t["w"].flip(2, 3, 4).transpose(0, 1), absolute=True)
    else:                                                     # direct "dgrad": 27 Cout; deconv3d_kernel: the taps of the voxel's parities
        Kx = U.terms(back._replace(kind="deconv" if seen[1] == "deconv3d" else "dgrad"))
        Sx = F.conv_transpose3d(dy.double().abs(), t["w"].double().abs(), None, stride=s3, padding=1, output_padding=tuple(s - 1 for s in s3))
    _route_check("ConvFn", name + " dX", x.grad, x64.grad, U.C_ACC * Kx * U.U32 * Sx)
    Sw = U.wgrad_sum(dy.abs(), t["x"].abs(), c.stride)
    _route_check("ConvFn", name + " dW", w.grad, w64.grad, U.C_ACC * dy[:, 0].numel() * U.U32 * Sw)


@pytest.mark.parametrize("name", [c.name for c in U.ROUTE_CASES if c.kind == "deconv"])
def test_deconv_fn_routes_vs_fp64(dev, monkeypatch, name):
    """``DeconvFn``: forward ``deconv3d``, dX the strided ``conv3d`` with the weight read as ``[out = cin, in = cout]``, dW with ``A = X``."""
    from mvsformer_amd import autograd as A
    ops, F = _ops(), torch.nn.functional
    monkeypatch.delenv("MVS_WGRAD_V1", raising=False)
    c = U.CASE[name]
    t = U.case_inputs(c)
    seen = _spy(ops, monkeypatch)
    x, w = t["x"].to(dev).requires_grad_(True), t["w"].to(dev).requires_grad_(True)
    sd = c.stride[0]
    y = A.DeconvFn.apply(x, w, sd)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6))
    y.backward(dy.to(dev))
    x64, w64 = t["x"].double().requires_grad_(True), t["w"].double().requires_grad_(True)
    y64 = F.conv_transpose3d(x64, w64, None, stride=(sd, 2, 2), padding=1, output_padding=(sd - 1, 1, 1))
    y64.backward(dy.double())
    assert seen == list(U.ROUTES[name]), seen
    _route_check("DeconvFn", name + " y", y, *U.expect(c))
    Sx = F.conv3d(dy.double().abs(), t["w"].double().abs(), None, stride=(sd, 2, 2), padding=1)
    _route_check("DeconvFn", name + " dX", x.grad, x64.grad, U.C_ACC * 27.0 * c.cout * U.U32 * Sx)
    Sw = U.wgrad_sum(t["x"].abs(), dy.abs(), c.stride)
    _route_check("DeconvFn", name + " dW", w.grad, w64.grad, U.C_ACC * t["x"][:, 0].numel() * U.U32 * Sw)


def test_print_worst_ratios(dev):
    """Runs last in this module: the record of the largest ratio per family seen in this process (the children print their own)."""
    for fam in sorted(R.WORST):
        print("WORST %-12s %.3f" % (fam, R.WORST[fam]))
