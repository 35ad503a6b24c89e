"""Greedy radius thinning on the MI355X (csrc/cloud_eval.hip, ``cloud_eval.greedy_thin``) against the sequential rule of
tests/cloud_thin_util.py: the keep mask and the output points are equal, bit for bit.  tests/test_cloud_thin_refs.py checks on the CPU
that no case has a pair distance within 8 fp32 ulp of its radius, so the kernel's fp32 comparison and the yardstick's fp64 one agree."""
import numpy as np
import pytest
import torch

import cloud_eval_util as U
import cloud_thin_util as T
from test_hip_cloud_eval import _check_scores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _run(name, dev):
    """-> ``(case, yardstick keep, kernel keep)`` after checking mask and points against the yardstick."""
    from mvsformer_amd import cloud_eval
    case, want = T.reference(name)
    xyz = case["xyz"]
    out, keep = cloud_eval.greedy_thin(_t(xyz, dev), case["dist"], order=_t(case["order"], dev), return_mask=True)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (len(xyz),) and out.dtype == torch.float32 and out.is_cuda
    keep = keep.cpu().numpy()
    assert np.array_equal(keep, want), np.nonzero(keep != want)[0][:8]
    assert out.cpu().numpy().tobytes() == xyz[want].tobytes()                # the kept points themselves, in original index order
    return case, want, keep


@pytest.mark.parametrize("n", T.SIZES)
def test_sizes(dev, n):
    _run("size_%d" % n, dev)


def test_duplicates_leave_the_copy_of_lowest_rank(dev):
    case, want, keep = _run("duplicates", dev)
    rank = np.argsort(case["order"])
    for b in range(300):
        rows = np.nonzero(case["src"] == b)[0]
        assert keep[rows].sum() == 1 and keep[rows[rank[rows].argmin()]]


def test_pairs_across_cell_faces_edges_and_corners(dev):
    case, want, keep = _run("faces", dev)
    rank = np.argsort(case["order"])
    for kind, under, a, b in case["pairs"]:
        first, second = (a, b) if rank[a] < rank[b] else (b, a)
        assert keep[first] and keep[second] == (not under), (kind, under)


@pytest.mark.parametrize("how", ["sorted", "reverse", "shuffle"])
@pytest.mark.parametrize("n", T.LINE_SIZES)
def test_a_chain_of_decisions_finishes(dev, n, how):
    """Sorted order: every decision waits for the previous point's, about n rounds (each its own launch); it ends and is right."""
    from mvsformer_amd import cloud_eval, ops
    case, want, _ = _run("line_%d_%s" % (n, how), dev)
    with torch.cuda.device(dev):
        keep, rounds = cloud_eval._greedy(_t(case["xyz"], dev), case["dist"], _t(case["order"], dev), 0)
    assert np.array_equal(keep.cpu().numpy(), want) and 1 <= rounds <= n
    if how == "sorted":
        # the lanes of a wavefront read their neighbours before any of them writes, so a round moves the chain on by about one point per
        # wavefront (5 at most here): far more rounds than one batch, so the host has read the counter and launched again
        assert rounds > ops.GREEDY_THIN_BATCH and want.tolist() == [i % 2 == 0 for i in range(n)]


def test_non_finite_points_are_never_kept_and_shield_nothing(dev):
    case, want, keep = _run("non_finite", dev)
    bad = ~np.isfinite(case["xyz"]).all(axis=1)
    assert bad.sum() >= 16 and not keep[bad].any()
    assert T.invariants(case["xyz"], case["dist"], case["order"], keep)


def test_order_and_seed(dev):
    from mvsformer_amd import cloud_eval
    from mvsformer_amd._lib import MvsHipError
    case, want, _ = _run("size_257", dev)
    _run("other_seed", dev)                                                  # the same points under another explicit order
    xyz, d = _t(case["xyz"], dev), case["dist"]
    masks = {}
    for seed in (0, 1, 2):
        a, ka = cloud_eval.greedy_thin(xyz, d, seed=seed, return_mask=True)
        b, kb = cloud_eval.greedy_thin(xyz, d, seed=seed, return_mask=True)
        assert torch.equal(a, b) and torch.equal(ka, kb)                     # the same seed: the same points
        gen = torch.Generator(device=dev)
        gen.manual_seed(seed)
        order = torch.randperm(len(case["xyz"]), generator=gen, device=dev)  # the documented default
        masks[seed] = ka.cpu().numpy()
        assert np.array_equal(masks[seed], T.greedy_ref(case["xyz"], d, order.cpu().numpy()))
        assert T.invariants(case["xyz"], d, order.cpu().numpy(), masks[seed])
    assert torch.equal(cloud_eval.greedy_thin(xyz, d), cloud_eval.greedy_thin(xyz, d, seed=0))
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])
    n = len(case["xyz"])
    twice = torch.arange(n, device=dev)
    twice[5] = 6                                                             # 6 twice, 5 missing
    past = torch.arange(n, device=dev)
    past[0] = n
    for bad in (twice, past, -torch.arange(n, device=dev), torch.arange(n - 1, device=dev), torch.arange(n, device=dev).int(),
                torch.arange(n), list(range(n))):
        with pytest.raises(MvsHipError):
            cloud_eval.greedy_thin(xyz, d, order=bad)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_rgb_rows_pass_through(dev, dtype):
    from mvsformer_amd import cloud_eval
    case, want = T.reference("size_5000")
    rgb = (np.random.default_rng(8).uniform(0, 255, case["xyz"].shape)).astype(dtype)
    out, col = cloud_eval.greedy_thin(_t(case["xyz"], dev), case["dist"], order=_t(case["order"], dev), rgb=_t(rgb, dev))
    assert col.dtype == _t(rgb, dev).dtype and col.cpu().numpy().tobytes() == rgb[want].tobytes()
    assert out.cpu().numpy().tobytes() == case["xyz"][want].tobytes()
    o2, c2, keep = cloud_eval.greedy_thin(_t(case["xyz"], dev), case["dist"], order=_t(case["order"], dev), rgb=_t(rgb, dev), return_mask=True)
    assert torch.equal(o2, out) and torch.equal(c2, col) and np.array_equal(keep.cpu().numpy(), want)


def test_empty_and_all_non_finite(dev):
    from mvsformer_amd import cloud_eval, ops
    with ops.kernel_timer() as timer:
        e = torch.empty(0, 3, device=dev)
        assert tuple(cloud_eval.greedy_thin(e, 0.5).shape) == (0, 3)
        x, c, k = cloud_eval.greedy_thin(e, 0.5, rgb=torch.empty(0, 3, dtype=torch.uint8, device=dev), return_mask=True)
        assert tuple(x.shape) == (0, 3) and tuple(c.shape) == (0, 3) and c.dtype == torch.uint8 and tuple(k.shape) == (0,)
        assert timer.order == []
        x, k = cloud_eval.greedy_thin(torch.full((5, 3), float("nan"), device=dev), 0.5, return_mask=True)
        assert tuple(x.shape) == (0, 3) and k.tolist() == [False] * 5
        assert timer.order == ["cloud_bounds"]                               # that no point is finite is a device result; no index, no round


def test_inside_evaluate(dev):
    from mvsformer_amd import cloud_eval
    from mvsformer_amd._lib import MvsHipError
    c, keep = T.reference("eval")
    pred, gt, order, mask = _t(c["pred"], dev), _t(c["gt"], dev), _t(c["order"], dev), _t(c["mask"], dev)
    want = U.evaluate_ref(c["pred"][keep], c["gt"], c["max_dist"], c["taus"])
    for t in c["taus"]:
        assert U.clear_of(want["all_dist"], t)
    got = cloud_eval.evaluate(pred, gt, c["max_dist"], c["taus"], pred_mask=mask, greedy=c["dist"], greedy_order=order)
    assert got["n_pred"] == int(keep.sum()) and got["n_gt"] == len(c["gt"])  # the prediction only
    _check_scores(got, want)
    seeded = cloud_eval.evaluate(pred, gt, c["max_dist"], c["taus"], greedy=c["dist"], greedy_seed=3)
    again = cloud_eval.evaluate(pred, gt, c["max_dist"], c["taus"], greedy=c["dist"], greedy_seed=3)
    assert {k: str(v) for k, v in seeded.items()} == {k: str(v) for k, v in again.items()} and seeded["n_pred"] < len(c["pred"])
    with pytest.raises(MvsHipError):
        cloud_eval.evaluate(pred, gt, c["max_dist"], c["taus"], voxel=1.0, greedy=c["dist"])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(MvsHipError):
            cloud_eval.evaluate(pred, gt, c["max_dist"], c["taus"], greedy=bad)
    plain = cloud_eval.evaluate(pred, gt, c["max_dist"], c["taus"], pred_mask=mask)
    none = cloud_eval.evaluate(pred, gt, c["max_dist"], c["taus"], pred_mask=mask, greedy=None, greedy_seed=5)
    assert {k: str(v) for k, v in plain.items()} == {k: str(v) for k, v in none.items()}             # str: nan equals nan
    _check_scores(plain, U.evaluate_ref(c["pred"], c["gt"], c["max_dist"], c["taus"], pred_mask=c["mask"]))


def test_bad_arguments_are_refused(dev):
    from mvsformer_amd import cloud_eval, ops
    from mvsformer_amd._lib import MvsHipError
    p = _t(U.plane_patch(100, 1), dev)
    with ops.kernel_timer() as timer:
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(MvsHipError):
                cloud_eval.greedy_thin(p, bad)
        with pytest.raises(MvsHipError):
            cloud_eval.greedy_thin(p.cpu(), 1.0)
        with pytest.raises(MvsHipError):
            cloud_eval.greedy_thin(p.view(-1, 2), 1.0)
        with pytest.raises(MvsHipError):
            cloud_eval.greedy_thin(p.view(-1), 1.0)
        with pytest.raises(MvsHipError):
            cloud_eval.greedy_thin(p, 1.0, rgb=torch.zeros(99, 3, device=dev))
        with pytest.raises(MvsHipError):
            cloud_eval.greedy_thin(p, 1.0, rgb=torch.zeros(100, 3))
        assert timer.order == []                                             # none of these reached the library
    with pytest.raises(MvsHipError, match="too small"):                      # the entry itself refuses a grid whose cells are smaller than dist
        idx = cloud_eval._Index(p, 0.5, None)
        ops.greedy_thin(torch.arange(100, device=dev), idx.grid, 1.0, idx.sorted_pts, idx.perm, idx.cell_keys, idx.cell_start)
