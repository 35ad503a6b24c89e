"""Runs the cases of ``tests/conv3d_f32_edge_util.py`` through ``mvsformer_amd.ops`` on the GPU and holds each output to its float64
reference and per-element bound.  Imported by ``tests/test_hip_conv3d_f32_edges.py``; run as a script it is the child process of one
forced tile form: MVS_CONV_TILE is read once per process by ``dispatch_tile`` (csrc/conv3d_fwd.hip), so
``MVS_CONV_TILE=22|42|22s python conv3d_f32_edge_child.py`` runs all of that form's cases and exits 0 only if every one is inside its bound
(1: some case is outside its bound; 3: a call raised something else, e.g. a HIP error, and the run ended there).

Memory a kernel does not own: every 5-D output the wrappers allocate is placed between two guard planes (one D plane, H W elements, of
777.25 before and behind it), ``dW`` between two guards of 9 elements; inputs and residuals lie between NaN planes, so a read that escapes a
buffer descriptor's range shows up in the values."""
import contextlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch                                   # noqa: E402

import conv3d_f32_edge_util as U               # noqa: E402

WORST = {}                                     # family -> largest |err| / bound seen in this process


@contextlib.contextmanager
def guarded_outputs(ops):
    """While active, ``ops._new`` (5-D outputs) and ``torch.zeros`` (``dW``; the wrapper owns the zeroing) allocate between guard planes;
    yields the list of ``(buffer, numel, plane)``."""
    made = []
    new0, zeros0 = ops._new, torch.zeros

    def alloc(shape, device, dtype, zero):
        numel, plane = 1, shape[-1] * shape[-2]
        for s in shape:
            numel *= s
        buf = torch.full((numel + 2 * plane,), U.GUARD, device=device, dtype=dtype)
        view = buf[plane:plane + numel].view(shape)
        if zero:
            view.zero_()
        made.append((buf, numel, plane))
        return view

    def new(on, *shape, dtype=torch.float32):
        if len(shape) != 5:
            return new0(on, *shape, dtype=dtype)
        return alloc(shape, getattr(on, "device", on), dtype, False)

    def zeros(*shape, **kw):
        if len(shape) != 5 or kw.get("dtype") != torch.float32:
            return zeros0(*shape, **kw)
        return alloc(shape, kw["device"], torch.float32, True)

    ops._new, torch.zeros = new, zeros
    try:
        yield made
    finally:
        ops._new, torch.zeros = new0, zeros0


def _in(t, dev):
    return None if t is None else U.guarded(t.to(dev), float("nan"))[0]


def check(family, name, got, ref, bound, made):
    """Prints ``F32EDGE family case max|err| ratio``, records the family's worst ratio, and requires: finite, every element inside its bound
    (bound 0: equal), the guards of every output untouched."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    err, ratio = U.share(got, ref, bound)
    print("F32EDGE %-12s %-44s err %.3e  ratio %.3f" % (family, name, err, ratio))
    if float(bound.max()) > 0:
        WORST[family] = max(WORST.get(family, 0.0), ratio)
    assert len(made) >= 1
    for buf, numel, plane in made:
        assert U.guards_intact(buf, numel, plane), "%s %s: a guard plane of an output was written" % (family, name)
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite output (an input guard was read?)" % (family, name)
    if float(bound.max()) == 0:
        assert torch.equal(got.double(), ref), "%s %s: integer operands must come out exact (max err %.3e)" % (family, name, err)
    assert ratio <= 1.0, "%s %s: |got - float64| reaches %.3f of its bound (max err %.3e)" % (family, name, ratio, err)
    return ratio


def family_of(c):
    p = U.case_plan(c)
    if c.kind in ("conv", "dgrad"):
        return "conv-" + p.form
    if c.kind == "deconv":
        return "deconv-sd%d" % c.stride[0]
    return "wino-nt%d" % p.NT


def run_layer(ops, dev, c):
    """One case of ``U.ALL_CASES`` through the wrapper ``ConvFn`` / ``DeconvFn`` would use -> the ratio."""
    t = U.case_inputs(c)
    x, w = _in(t["x"], dev), t["w"].to(dev)
    epi = dict(scale=t["scale"].to(dev) if c.scale else None, shift=t["shift"].to(dev) if c.scale else None,
               residual=_in(t["residual"], dev) if c.residual else None, relu=c.relu)
    with guarded_outputs(ops) as made:
        if c.kind == "conv":
            y = ops.conv3d(x, ops.conv3d_pack(w, False), c.cin, c.cout, c.stride, **epi)
        elif c.kind == "dgrad":
            y = ops.conv3d(x, ops.conv3d_pack(w, "dgrad"), c.cin, c.cout, (1, 1), **epi)
        elif c.kind == "deconv":
            y = ops.deconv3d(x, ops.conv3d_pack(w, True, c.stride[0]), c.cin, c.cout, c.stride[0], **epi)
        else:
            wk = w if c.kind == "wino" else w.flip(2, 3, 4).transpose(0, 1).contiguous()
            y = ops.conv3d_wino(x, ops.conv3d_wino_pack(wk), c.cin, c.cout, **epi)
        torch.cuda.synchronize()
    assert len(made) == 1
    return check(family_of(c), c.name, y, *U.expect(c), made)


def run_wgrad(ops, dev, c, family):
    """``ops.conv3d_wgrad`` twice on the same inputs: both results inside the bound (a sum of atomics: no bit equality between them)."""
    A, Bt = U.wg_inputs(c.name)
    A, Bt = _in(A, dev), _in(Bt, dev)
    ref, bound = U.wg_expect(c.name)
    worst = 0.0
    for rep in range(2):
        with guarded_outputs(ops) as made:
            dW = ops.conv3d_wgrad(A, Bt, c.stride)
            torch.cuda.synchronize()
        assert len(made) == 1
        worst = max(worst, check(family, c.name + "#%d" % rep, dW, ref, bound, made))
        zero = (bound == 0) & (ref == 0)
        assert bool((dW.cpu()[zero] == 0).all())
    return worst


def main():
    force = os.environ.get("MVS_CONV_TILE")
    cases = U.forced_cases(force)
    assert force in U.CHILD_FORMS and cases, "MVS_CONV_TILE must name a forced form"
    from mvsformer_amd import ops
    dev = torch.device("cuda:0")
    failed = []
    for c in cases:
        try:
            run_layer(ops, dev, c)
        except AssertionError as e:
            failed.append(c.name)
            print("FAILED %s: %s" % (c.name, e))
        except Exception as e:                 # a HIP error, not a wrong value: start nothing more on the GPU; the parent counts 3 as died
            print("DIED in %s: %s: %s" % (c.name, type(e).__name__, e))
            return 3
    for fam in sorted(WORST):
        print("WORST %-12s %.3f" % (fam, WORST[fam]))
    if failed:
        print("%d of %d cases failed: %s" % (len(failed), len(cases), " ".join(failed)))
        return 1
    print("%d cases ok (MVS_CONV_TILE=%s)" % (len(cases), force))
    return 0


if __name__ == "__main__":
    sys.exit(main())
