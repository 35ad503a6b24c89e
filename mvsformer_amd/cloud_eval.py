"""Point-cloud evaluation on the device: DTU's accuracy / completeness / overall and Tanks-and-Temples' precision / recall / F-score between
a reconstructed cloud and a ground-truth cloud (csrc/cloud_eval.hip).  The reference leaves this step to the DTU MATLAB code and the T&T
site; here the clouds stay where ``SceneFusion.fuse(on_device=True)`` left them.

* :func:`nn_distance`: exact nearest-neighbour distances, capped at ``max_dist``, over a uniform grid of the target.
* :func:`voxel_downsample`: one point per occupied voxel, the centroid of the voxel's points (the Open3D / T&T rule).
* :func:`greedy_thin`: DTU's own thinning (0.2 mm there) - a greedy pass over a shuffle of the points: a visited point that has not been
  removed is kept and removes every other point within ``dist``.  The rule is reproduced exactly for a given visiting order; the order is
  an input (default: a seeded device permutation).  MATLAB's shuffle is not reproduced, so scores after thinning are those of the same
  protocol under another shuffle, not the MATLAB numbers bit for bit; the distances themselves are exact.
* :func:`evaluate`: both directions, the means and the shares under every threshold, read back in ONE 256-byte record at the end.
* :func:`transform`, :func:`crop_polygon`, :func:`icp`, :func:`register_tt`, :func:`evaluate_tt`: what Tanks and Temples does before the
  distances - bring the reconstruction into the scanner's frame, refine that by point-to-point ICP with a scale factor, cut both clouds to
  the crop volume (csrc/cloud_align.hip; one 192-byte record read per ICP iteration).
* :func:`in_box`, :func:`in_volume`, :func:`above_plane`: DTU's bounding-box, observation-mask and above-plane filters as boolean masks
  (elementwise torch code).

Host reads: the scores are one record.  Before that each grid build reads its 32-byte bounds record (``mvs_cloud_grid_keys`` refuses a grid
of 2^21 cells or more per axis on the host, and the default cell size is derived from the bounds), a voxel thinning reads its voxel count
to size its output, and a greedy thinning reads its counter of undecided points once per batch of rounds.  The key sort is
``torch.sort(stable=True)``; everything else is the HIP path, and a CPU tensor is refused.

The default cell (``cell=None``): ``cbrt(V / N)`` with ``V`` the target's bounding-box volume over the axes that have an extent (the square
or the length itself for a flat or a straight cloud) and ``N`` its finite points - about one point per cell of a filled box, a handful per
occupied cell of a surface - then raised to ``max_dist / 16`` (at most 16 shells are walked before the cap ends the search) and to
``extent / 2^20`` (the grid indexes fewer than 2^21 cells per axis).
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import MvsHipError

MAX_DEFAULT_SHELLS = 16


def _cloud(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise MvsHipError("%s must be a GPU tensor: the MI355X HIP path is the only implementation (no CPU fallback)" % name)
    if t.dim() != 2 or t.shape[1] != 3:
        raise MvsHipError("%s must be [N,3], got %s" % (name, tuple(t.shape)))
    return t.detach().to(torch.float32).contiguous()


def _positive(v, name: str) -> float:
    v = float(v)
    if not math.isfinite(v) or v <= 0.0:
        raise MvsHipError("%s=%r must be positive and finite" % (name, v))
    return v


def default_cell(bounds: Sequence[float], n_finite: int, max_dist: float) -> float:
    """The rule of the module docstring on the host: ``bounds`` = (min xyz, max xyz)."""
    ext = [float(bounds[3 + a]) - float(bounds[a]) for a in range(3)]
    pos = [e for e in ext if e > 0.0]
    cell = (math.prod(pos) / max(1, n_finite)) ** (1.0 / len(pos)) if pos else max_dist
    cell = max(cell, max_dist / MAX_DEFAULT_SHELLS, max(ext) / float(1 << 20))
    return float(np.float32(cell) * np.float32(1.0 + 2.0 ** -20))          # rounded to fp32, never below the two floors


class _Index:
    """The grid of one target cloud: what ``mvs_cloud_grid_build`` left on the device.  ``cell``: the edge, a rule ``(bounds, n_valid) ->
    edge``, or None for :func:`default_cell` with ``max_dist``.  ``skip_empty``: no finite point -> nothing is launched after the bounds."""

    def __init__(self, pts: torch.Tensor, cell, max_dist: Optional[float] = None, want_sorted: bool = True, skip_empty: bool = False):
        self.pts, self.n = pts, pts.shape[0]
        self.grid, self.bounds, self.n_bad = ops.cloud_bounds(pts)
        self.n_valid = self.n - self.n_bad
        if skip_empty and self.n_valid == 0:
            return
        if cell is None:
            cell = default_cell(self.bounds, self.n_valid, max_dist)
        self.cell = cell(self.bounds, self.n_valid) if callable(cell) else cell
        keys = ops.cloud_grid_keys(pts, self.cell, self.grid, self.bounds, self.n_bad)
        skeys, self.perm = torch.sort(keys, stable=True)                   # plumbing: the one step of the index that is not HIP
        self.sorted_pts, self.cell_keys, self.cell_start = ops.cloud_grid_build(pts, skeys, self.perm, self.grid, want_sorted)

    def query(self, src: torch.Tensor, max_dist: float):
        qperm = torch.sort(ops.cloud_query_keys(src, self.grid), stable=True)[1]
        return ops.cloud_nn_query(src, qperm, self.grid, self.cell, self.sorted_pts, self.perm, self.cell_keys, self.cell_start, max_dist)


def _capped(m: int, max_dist: float, device):
    return (torch.full((m,), max_dist, dtype=torch.float32, device=device), torch.full((m,), -1, dtype=torch.int64, device=device))


def _nn(src: torch.Tensor, dst: torch.Tensor, max_dist: float, cell: Optional[float]):
    if src.shape[0] == 0 or dst.shape[0] == 0:
        return _capped(src.shape[0], max_dist, src.device)                 # nothing to launch
    index = _Index(dst, cell, max_dist)
    if index.n_valid == 0:
        return _capped(src.shape[0], max_dist, src.device)
    return index.query(src, max_dist)


@torch.no_grad()
def nn_distance(src, dst, max_dist: float, cell: Optional[float] = None):
    """For every point of ``src [M,3]`` the Euclidean distance to the nearest point of ``dst [N,3]`` and that point's index:
    ``(dist float32 [M], idx int64 [M])``; where no target is closer than ``max_dist`` (strictly), ``max_dist`` and ``-1``.  Exact - the
    minimum a brute-force scan finds in fp32; equidistant targets resolve to the lowest index.  Non-finite targets are not indexed, a
    non-finite query comes back capped.  ``cell``: the grid's cell edge (default: see the module docstring); ``max_dist / cell <= 32``."""
    src, dst = _cloud(src, "src"), _cloud(dst, "dst")
    max_dist = _positive(max_dist, "max_dist")
    cell = None if cell is None else _positive(cell, "cell")
    if cell is not None and max_dist / cell > ops.CLOUD_MAX_SHELLS:
        raise MvsHipError("max_dist / cell = %g: at most %d shells are walked" % (max_dist / cell, ops.CLOUD_MAX_SHELLS))
    with torch.cuda.device(src.device):
        return _nn(src, dst, max_dist, cell)


def _thin(xyz: torch.Tensor, voxel: float, attrs: Sequence[torch.Tensor] = ()):
    """-> ``[centroids] + [mean of each attr]`` per occupied voxel, ascending key order."""
    empty = [torch.empty(0, 3, dtype=torch.float32, device=xyz.device) for _ in range(1 + len(attrs))]
    if xyz.shape[0] == 0:
        return empty
    index = _Index(xyz, voxel, want_sorted=False)
    count = ops.cloud_voxel_count(index.grid) if index.n_valid else 0
    if count == 0:
        return empty
    return [ops.cloud_voxel_write(a, index.perm, index.grid, index.cell_start, count) for a in [xyz] + list(attrs)]


@torch.no_grad()
def voxel_downsample(xyz, voxel: float, rgb=None):
    """One point per occupied voxel of edge ``voxel`` (cells counted from the cloud's per-axis minimum): the centroid of the voxel's points,
    accumulated in fp64 in original order - bit-identical from run to run.  Output order: ascending cell key (x fastest).  ``rgb [N,3]``
    (uint8 or float32) is averaged the same way and returned in its own dtype (uint8: rounded to nearest): ``xyz`` or ``(xyz, rgb)``.
    Non-finite points are dropped."""
    xyz = _cloud(xyz, "xyz")
    voxel = _positive(voxel, "voxel")
    if rgb is None:
        with torch.cuda.device(xyz.device):
            return _thin(xyz, voxel)[0]
    if not isinstance(rgb, torch.Tensor) or not rgb.is_cuda or rgb.shape != xyz.shape:
        raise MvsHipError("rgb must be a GPU tensor of xyz's shape %s" % (tuple(xyz.shape),))
    with torch.cuda.device(xyz.device):
        out, col = _thin(xyz, voxel, [rgb.detach().to(torch.float32).contiguous()])
    if rgb.dtype == torch.uint8:
        col = (col + 0.5).floor().clamp_(0, 255).to(torch.uint8)
    return out, col


def thin_cell(bounds: Sequence[float], dist: float) -> float:
    """The cell edge of a greedy thinning's grid: ``max(dist, extent / 2^20)`` widened by what fp32 cell coordinates can be off by, so that
    two points within ``dist`` always lie in cells that differ by at most 1 per axis (``mvs_greedy_thin`` checks it; include/mvs_hip.h):
    ``max(1.0001 * dist + extent * 2^-21, extent * 2^-20)``, ``extent`` = the largest axis extent."""
    ext = max(float(bounds[3 + a]) - float(bounds[a]) for a in range(3))
    cell = max(1.0001 * dist + ext * 2.0 ** -21, ext * 2.0 ** -20)
    return float(np.float32(cell) * np.float32(1.0 + 2.0 ** -20))          # rounded to fp32, never below the rule


def _order(order, n: int, seed: int, device) -> torch.Tensor:
    if order is None:
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        return torch.randperm(n, generator=gen, device=device)
    if not isinstance(order, torch.Tensor) or order.device != device or order.dtype != torch.int64 or order.shape != (n,):
        raise MvsHipError("order must be an int64 tensor [%d] on the cloud's device (a permutation of 0..%d)" % (n, n - 1))
    return order.contiguous()


def _greedy(xyz: torch.Tensor, dist: float, order, seed: int):
    """-> ``(keep bool [N], rounds)``; ``xyz`` is fp32 ``[N,3]`` on the current device."""
    n = xyz.shape[0]
    order = _order(order, n, seed, xyz.device)
    none = torch.zeros(n, dtype=torch.bool, device=xyz.device)
    if n == 0:
        return none, 0
    index = _Index(xyz, lambda bounds, n_valid: thin_cell(bounds, dist), skip_empty=True)
    if index.n_valid == 0:
        return none, 0                                                     # nothing finite: no index, no round
    return ops.greedy_thin(order, index.grid, dist, index.sorted_pts, index.perm, index.cell_keys, index.cell_start)       # refuses an order that is no permutation


@torch.no_grad()
def greedy_thin(xyz, dist: float, order=None, seed: int = 0, rgb=None, return_mask: bool = False):
    """DTU's thinning: visit the points in ``order``; a visited point that has not been removed is kept and removes every other point at
    distance ``<= dist`` (``(dx*dx + dy*dy) + dz*dz <= dist*dist`` in fp32).  -> the kept points ``[K,3]`` in their original index order
    (a subset of the input, pairwise farther apart than ``dist``), ``(xyz, rgb)`` with ``rgb [N,3]`` (any dtype: rows are selected, not
    averaged), and with ``return_mask`` also ``keep`` bool ``[N]`` as the last item.  Non-finite points are never kept and remove nothing.

    ``order``: int64 ``[N]`` on the cloud's device, a permutation of ``0..N-1`` (checked; anything else is refused).  Default:
    ``torch.randperm(N, generator=<device generator seeded with seed>)`` - the same seed gives the same points.  The shuffle is this
    function's, not MATLAB's.

    The kept set is the lexicographically first maximal independent set under ``order``; the kernel finds it in rounds (a point decides
    once every neighbour of lower rank has), which gives exactly what the sequential loop gives.  The keep mask is the kernel's; the
    compaction is ``torch`` indexing with that mask (``xyz[keep]``), which preserves index order."""
    xyz = _cloud(xyz, "xyz")
    dist = _positive(dist, "dist")
    if rgb is not None and (not isinstance(rgb, torch.Tensor) or not rgb.is_cuda or rgb.shape != xyz.shape):
        raise MvsHipError("rgb must be a GPU tensor of xyz's shape %s" % (tuple(xyz.shape),))
    with torch.cuda.device(xyz.device):
        keep = _greedy(xyz, dist, order, seed)[0]
        out = [xyz[keep]]
        if rgb is not None:
            out.append(rgb[keep])
    if return_mask:
        out.append(keep)
    return out[0] if len(out) == 1 else tuple(out)


def _valid(xyz: torch.Tensor, mask) -> torch.Tensor:
    ok = torch.isfinite(xyz).all(dim=1)
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != xyz.device or mask.shape != (xyz.shape[0],):
            raise MvsHipError("a mask must be a boolean tensor [%d] on the cloud's device" % xyz.shape[0])
        ok = ok & mask.to(torch.bool)
    return ok


@torch.no_grad()
def evaluate(pred_xyz, gt_xyz, max_dist: float, taus: Sequence[float] = (), voxel: Optional[float] = None, pred_mask=None, gt_mask=None,
             cell: Optional[float] = None, greedy: Optional[float] = None, greedy_seed: int = 0, greedy_order=None) -> Dict[str, object]:
    """Scores of ``pred_xyz [M,3]`` against ``gt_xyz [N,3]`` (device tensors; ``SceneFusion.fuse(on_device=True)['xyz']`` as it is):

    * ``n_pred``, ``n_gt``: points after the masks (boolean ``[M]`` / ``[N]``; non-finite points are dropped too) and the thinning
      (``voxel``: :func:`voxel_downsample` of both clouds first; or ``greedy``: :func:`greedy_thin` with that radius of the PREDICTION
      only, as DTU does - its ground truth is sampled already - in the order ``greedy_order`` ``[M]`` or a shuffle seeded with
      ``greedy_seed``; a masked-out point is never kept and removes nothing; ``voxel`` and ``greedy`` together are refused);
    * ``accuracy``: the mean of the pred -> gt distances that are ``< max_dist`` (DTU: ``d[d < max_dist].mean()``), ``completeness``: the
      same for gt -> pred, ``overall``: their mean; ``pred_below_max`` / ``gt_below_max``: how many distances those means are over;
    * per ``tau`` (``taus``, each ``<= max_dist``; lists in that order): ``precision`` = the share of pred points closer than ``tau`` to the
      ground truth, ``recall`` = the same for gt points, ``fscore = 2PR / (P + R)`` (0 when ``P + R == 0``), and the counts
      ``pred_below_tau`` / ``gt_below_tau``.

    A mean or a share over an empty set is ``nan``.  Masked-out points never leave the device: they are turned into non-finite points,
    which the index skips and the score does not count."""
    pred, gt = _cloud(pred_xyz, "pred_xyz"), _cloud(gt_xyz, "gt_xyz")
    if pred.device != gt.device:
        raise MvsHipError("pred_xyz is on %s, gt_xyz on %s" % (pred.device, gt.device))
    max_dist = _positive(max_dist, "max_dist")
    taus = [float(t) for t in taus]
    if len(taus) > ops.CLOUD_SCORE_MAX_K:
        raise MvsHipError("%d thresholds, at most %d are built" % (len(taus), ops.CLOUD_SCORE_MAX_K))
    for t in taus:
        if not t <= max_dist:
            raise MvsHipError("tau=%r exceeds max_dist=%r" % (t, max_dist))
    cell = None if cell is None else _positive(cell, "cell")
    if cell is not None and max_dist / cell > ops.CLOUD_MAX_SHELLS:
        raise MvsHipError("max_dist / cell = %g: at most %d shells are walked" % (max_dist / cell, ops.CLOUD_MAX_SHELLS))
    voxel = None if voxel is None else _positive(voxel, "voxel")
    greedy = None if greedy is None else _positive(greedy, "greedy")
    if voxel is not None and greedy is not None:
        raise MvsHipError("voxel and greedy are two thinning rules: pass one of them")
    nan = float("nan")
    with torch.cuda.device(pred.device):
        clouds = []
        for xyz, mask in ((pred, pred_mask), (gt, gt_mask)):
            ok = _valid(xyz, mask)
            xyz = torch.where(ok[:, None], xyz, torch.full((), nan, dtype=torch.float32, device=xyz.device))
            if voxel is not None:
                xyz = _thin(xyz, voxel)[0]
                ok = torch.ones(xyz.shape[0], dtype=torch.bool, device=xyz.device)
            elif greedy is not None and not clouds:                        # the prediction only; its dropped points are non-finite by now
                ok = _greedy(xyz, greedy, greedy_order, greedy_seed)[0]
                xyz = torch.where(ok[:, None], xyz, torch.full((), nan, dtype=torch.float32, device=xyz.device))
            clouds.append((xyz, ok))
        rec = torch.zeros(2, ops.CLOUD_SCORE_RECORD_BYTES // 8, dtype=torch.int64, device=pred.device)
        for i, ((src, ok), (dst, _)) in enumerate((clouds, clouds[::-1])):
            dist = _nn(src, dst, max_dist, cell)[0]
            dist = torch.where(ok, dist, torch.full((), nan, dtype=torch.float32, device=dist.device))      # a dropped point scores nothing
            ops.cloud_score(dist, max_dist, taus, rec[i])
            rec[i, 12] = ok.sum()                                          # a reserved slot: the points that count
        host = rec.cpu()                                                   # the one read of the scores
    out: Dict[str, object] = {}
    sides = []
    for i in range(2):
        r = host[i]
        n, below = int(r[12]), int(r[1])
        counts = [int(c) for c in r[2:2 + len(taus)]]
        sides.append((n, below, float(r[11:12].view(torch.float64)[0]), counts, [c / n if n else nan for c in counts]))
    (n_pred, pb, acc, pc, prec), (n_gt, gb, comp, gc, rcl) = sides
    out.update(n_pred=n_pred, n_gt=n_gt, accuracy=acc, completeness=comp, overall=0.5 * (acc + comp), pred_below_max=pb, gt_below_max=gb,
               taus=taus, precision=prec, recall=rcl, pred_below_tau=pc, gt_below_tau=gc,
               fscore=[(2.0 * p * r / (p + r) if p + r > 0.0 else 0.0) if p == p and r == r else nan for p, r in zip(prec, rcl)])
    return out


# ------------------------------------------------------------------------- alignment: Tanks and Temples (csrc/cloud_align.hip)
# The T&T toolbox brings a reconstruction into the scanner's frame with a given 4 x 4 matrix, refines it by point-to-point ICP with a scale
# factor on three progressively finer down-samples, cuts both clouds to the scene's crop volume and only then measures distances.  It does
# so with Open3D on the host.  Neither Open3D nor the toolbox was available to compare with: the crop rule is the one written out in
# include/mvs_hip.h (UNVERIFIED against Open3D's SelectionPolygonVolume), and the default stages of register_tt are recalled, not checked
# (UNVERIFIED against the toolbox) - which is why they are arguments.  The toolbox's trajectory-based initial alignment is not here: the
# initial transform is an input.
_AXES = {"X": 0, "Y": 1, "Z": 2, 0: 0, 1: 1, 2: 2}


def _matrix(T, name: str = "T") -> np.ndarray:
    try:
        T = np.array(T, dtype=np.float64)
    except (TypeError, ValueError):
        raise MvsHipError("%s must be a 4x4 matrix of numbers" % name)
    if T.shape != (4, 4) or not np.isfinite(T).all():
        raise MvsHipError("%s must be a finite 4x4 matrix, got shape %s" % (name, T.shape))
    if not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise MvsHipError("%s: the last row must be 0 0 0 1, got %s" % (name, T[3].tolist()))
    return T


@torch.no_grad()
def transform(xyz, T) -> torch.Tensor:
    """``xyz [N,3]`` moved by the 4 x 4 ``T`` (numpy float64 or nested lists; last row ``0 0 0 1``): per coordinate
    ``(r0 x + r1 y) + r2 z + t`` in fp64, in this order, rounded to fp32 once.  Non-finite points pass through as the arithmetic leaves
    them."""
    xyz = _cloud(xyz, "xyz")
    T = _matrix(T)
    with torch.cuda.device(xyz.device):
        return ops.align_transform(xyz, list(T[:3, :3].reshape(-1)) + list(T[:3, 3]))


@torch.no_grad()
def crop_polygon(xyz, axis, axis_min: float, axis_max: float, polygon) -> torch.Tensor:
    """The test of Open3D's ``SelectionPolygonVolume`` as restated in include/mvs_hip.h (parity with Open3D itself is unverified: it was not
    available) -> bool ``[N]``.  ``axis``: the orthogonal axis, ``"X" / "Y" / "Z"`` or ``0 / 1 / 2``; the polygon lives in the plane of the
    other two, ``(u, v)`` = (Y, Z) / (X, Z) / (X, Y).  A point is kept iff ``axis_min <= p[axis] <= axis_max`` and the even-odd crossing
    rule over the ring of vertices says inside, all in fp64 from the fp32 coordinates; a non-finite point is out.  ``polygon``: ``[K,3]``
    (the orthogonal coordinate is ignored, as in the T&T json files) or ``[K,2]`` = ``(u, v)``; ``3 <= K <= 64``."""
    xyz = _cloud(xyz, "xyz")
    if axis not in _AXES:
        raise MvsHipError("axis=%r: 'X', 'Y', 'Z' or 0, 1, 2" % (axis,))
    axis = _AXES[axis]
    poly = np.array(polygon, dtype=np.float64)
    if poly.ndim != 2 or poly.shape[1] not in (2, 3) or poly.shape[0] < 3:
        raise MvsHipError("polygon must be [K,3] or [K,2] with K >= 3, got %s" % (poly.shape,))
    if poly.shape[1] == 3:
        poly = poly[:, [a for a in range(3) if a != axis]]
    with torch.cuda.device(xyz.device):
        return ops.align_crop_polygon(xyz, axis, float(axis_min), float(axis_max), poly.tolist())


class PairSums:
    """The record of ``ops.align_pair_sums`` on the host: ``n`` pairs, ``n_finite`` source points, ``sp``, ``sq`` (3), ``sqp`` (3 x 3, row =
    q's axis), ``spp``, ``sqq``, ``sdd`` - sums over the pairs of ``p = src - origin``, ``q = dst - origin`` and ``dist^2`` - and the
    ``origin`` they were taken about."""

    def __init__(self, n, n_finite, sp, sq, sqp, spp, sqq, sdd, origin=(0.0, 0.0, 0.0)):
        self.n, self.n_finite = int(n), int(n_finite)
        self.sp, self.sq = np.array(sp, dtype=np.float64).reshape(3), np.array(sq, dtype=np.float64).reshape(3)
        self.sqp = np.array(sqp, dtype=np.float64).reshape(3, 3)
        self.spp, self.sqq, self.sdd = float(spp), float(sqq), float(sdd)
        self.origin = np.array(origin, dtype=np.float64).reshape(3)

    @classmethod
    def from_record(cls, record: torch.Tensor, origin) -> "PairSums":
        host = record.cpu()                                                # the one read of an ICP iteration
        s = host[2:20].view(torch.float64).numpy()
        return cls(int(host[0]), int(host[1]), s[0:3], s[3:6], s[6:15], s[15], s[16], s[17], origin)


def umeyama(record: PairSums, with_scaling: bool = True) -> np.ndarray:
    """The least-squares similarity ``q ~ c R p + t`` from the sums of the pairs (Umeyama 1991) -> 4 x 4 float64.  Means ``mu_p, mu_q``,
    covariance ``Sigma = (1/n) sum (q - mu_q)(p - mu_p)^T``, SVD ``Sigma = U D V^T``, ``S = diag(1, 1, sign(det U det V))``,
    ``R = U S V^T``, ``c = tr(D S) / var_p`` (1 without scaling), ``t = mu_q - c R mu_p``, then the origin is added back.  Fewer than 3
    pairs, non-finite sums, or a covariance of rank below 2 (all pairs on a line) raise: a NaN matrix is never returned."""
    n = record.n
    if n < 3:
        raise MvsHipError("umeyama: %d pairs, at least 3 are needed" % n)
    mp, mq = record.sp / n, record.sq / n
    cov = record.sqp / n - np.outer(mq, mp)
    var_p = record.spp / n - float(mp @ mp)
    if not (np.isfinite(cov).all() and math.isfinite(var_p)):
        raise MvsHipError("umeyama: the sums are not finite")
    U, D, Vt = np.linalg.svd(cov)
    if not (var_p > 0.0 and D[0] > 0.0 and D[1] > 1e-12 * D[0]):
        raise MvsHipError("umeyama: the pairs do not span a plane (singular values %s, var_p %g): the rotation is undetermined" % (D.tolist(), var_p))
    S = np.diag([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0.0 else -1.0])
    R = U @ S @ Vt
    c = float((D * np.diag(S)).sum()) / var_p if with_scaling else 1.0
    A = c * R
    T = np.eye(4)
    T[:3, :3] = A
    T[:3, 3] = (mq - A @ mp) + record.origin - A @ record.origin
    if not np.isfinite(T).all():
        raise MvsHipError("umeyama: the solution is not finite")
    return T


class IcpResult:
    """``T`` 4 x 4 float64; ``fitness`` = pairs / finite source points and ``inlier_rmse`` = sqrt(sum dist^2 / pairs) as measured in the
    last iteration (before its update, unless that iteration found the loop converged and applied none); ``iterations`` = evaluations made
    (one record read each); ``converged``."""

    def __init__(self, T, fitness, inlier_rmse, iterations, converged):
        self.T, self.fitness, self.inlier_rmse, self.iterations, self.converged = T, fitness, inlier_rmse, iterations, converged

    def __repr__(self):
        return "IcpResult(fitness=%r, inlier_rmse=%r, iterations=%d, converged=%r, T=\n%r)" % (
            self.fitness, self.inlier_rmse, self.iterations, self.converged, self.T)


@torch.no_grad()
def icp(src, dst, threshold: float, init=None, with_scaling: bool = True, max_iter: int = 20, fitness_tol: float = 1e-6,
        rmse_tol: float = 1e-6, cell: Optional[float] = None) -> IcpResult:
    """Open3D's point-to-point ICP loop (``TransformationEstimationPointToPoint(with_scaling)``) of ``src [M,3]`` onto ``dst [N,3]``.  The
    target's grid is built once.  Per iteration: the ORIGINAL source moved by the accumulated fp64 ``T`` (:func:`transform`; roundings do
    not pile up), the nearest target within ``threshold`` of every point, the pair sums about the target's bounding-box centre, ONE
    record read, ``fitness`` and ``inlier_rmse``, the update (:func:`umeyama` on the pairs (moved source, target)), ``T = update @ T``.
    The loop ends before the update when both ``|fitness - previous| < fitness_tol`` and ``|inlier_rmse - previous| < rmse_tol``
    (absolute differences, as in Open3D despite its "relative" names), or after ``max_iter`` iterations.  No pair at all, or pairs that
    determine no transform, raise."""
    src, dst = _cloud(src, "src"), _cloud(dst, "dst")
    if src.device != dst.device:
        raise MvsHipError("src is on %s, dst on %s" % (src.device, dst.device))
    threshold = _positive(threshold, "threshold")
    T = np.eye(4) if init is None else _matrix(init, "init")
    max_iter = int(max_iter)
    if max_iter < 1:
        raise MvsHipError("max_iter=%d: at least one iteration" % max_iter)
    if src.shape[0] == 0 or dst.shape[0] == 0:
        raise MvsHipError("icp: an empty cloud (%d source, %d target points)" % (src.shape[0], dst.shape[0]))
    cell = None if cell is None else _positive(cell, "cell")
    if cell is not None and threshold / cell > ops.CLOUD_MAX_SHELLS:
        raise MvsHipError("threshold / cell = %g: at most %d shells are walked" % (threshold / cell, ops.CLOUD_MAX_SHELLS))
    with torch.cuda.device(src.device):
        index = _Index(dst, cell, threshold)
        if index.n_valid == 0:
            raise MvsHipError("icp: the target has no finite point")
        origin = [0.5 * (float(index.bounds[a]) + float(index.bounds[3 + a])) for a in range(3)]
        record = torch.empty(ops.ALIGN_PAIR_RECORD_BYTES // 8, dtype=torch.int64, device=src.device)
        prev, fitness, rmse, converged, it = None, 0.0, 0.0, False, 0
        while it < max_iter:
            moved = ops.align_transform(src, list(T[:3, :3].reshape(-1)) + list(T[:3, 3]))
            dist, idx = index.query(moved, threshold)
            sums = PairSums.from_record(ops.align_pair_sums(moved, dst, idx, dist, origin, record), origin)
            it += 1
            if sums.n == 0:
                raise MvsHipError("icp: no source point has a target within threshold=%g at iteration %d" % (threshold, it))
            fitness, rmse = sums.n / max(1, sums.n_finite), math.sqrt(sums.sdd / sums.n)
            if prev is not None and abs(fitness - prev[0]) < fitness_tol and abs(rmse - prev[1]) < rmse_tol:
                converged = True
                break
            prev = (fitness, rmse)
            T = umeyama(sums, with_scaling) @ T
    return IcpResult(T, fitness, rmse, it, converged)


def default_tt_stages(dtau: float):
    """``(downsample, threshold, max_iter)`` per stage, as the T&T toolbox's three registrations are RECALLED (the toolbox was not available
    to check them against, hence an argument of :func:`register_tt`): voxels of ``dtau`` with threshold ``80 dtau``, voxels of ``dtau / 2``
    with ``20 dtau``, every k-th point up to about 4 M points with ``2 dtau``; 20 iterations each."""
    return [(("voxel", dtau), 80.0 * dtau, 20), (("voxel", 0.5 * dtau), 20.0 * dtau, 20), (("uniform", 4e6), 2.0 * dtau, 20)]


def _crop(xyz: torch.Tensor, crop) -> torch.Tensor:
    if crop is None:
        return xyz
    try:
        axis, lo, hi, poly = crop["orthogonal_axis"], crop["axis_min"], crop["axis_max"], crop["bounding_polygon"]
    except (KeyError, TypeError):
        raise MvsHipError("crop must be None or a mapping with orthogonal_axis, axis_min, axis_max, bounding_polygon (data_io.read_crop_volume)")
    return xyz[crop_polygon(xyz, axis, lo, hi, poly)]


def _downsample(xyz: torch.Tensor, how) -> torch.Tensor:
    kind, value = how
    if kind == "voxel":
        return voxel_downsample(xyz, value)
    if kind == "uniform":
        return xyz[::max(1, int(round(xyz.shape[0] / float(value))))] if xyz.shape[0] else xyz
    raise MvsHipError("downsample %r: ('voxel', size) or ('uniform', max_points)" % (how,))


@torch.no_grad()
def register_tt(pred, gt, init, crop, dtau: float, stages=None):
    """The registration of the Tanks-and-Temples protocol -> ``(T 4 x 4 float64, [IcpResult per stage])``.  ``init``: the 4 x 4 that brings
    ``pred`` roughly into ``gt``'s frame (the ``*_trans.txt`` of a training scene); ``crop``: ``data_io.read_crop_volume``'s mapping or
    None.  A stage is ``(downsample, threshold, max_iter)`` with ``downsample`` = ``("voxel", size)`` (:func:`voxel_downsample`) or
    ``("uniform", max_points)`` (every k-th point, ``k = max(1, round(N / max_points))``).  Each stage moves ``pred`` by the current
    ``T``, crops it and ``gt``, down-samples both, runs :func:`icp` from identity with scaling and composes the result into ``T``.
    ``stages=None``: :func:`default_tt_stages` - recalled, not checked against the toolbox."""
    pred, gt = _cloud(pred, "pred"), _cloud(gt, "gt")
    T = _matrix(init, "init")
    dtau = _positive(dtau, "dtau")
    stages = default_tt_stages(dtau) if stages is None else list(stages)
    results = []
    gt_c = _crop(gt, crop)
    for how, threshold, max_iter in stages:
        src = _downsample(_crop(transform(pred, T), crop), how)
        dst = _downsample(gt_c, how)
        res = icp(src, dst, threshold, with_scaling=True, max_iter=max_iter)
        T = res.T @ T
        results.append(res)
    return T, results


@torch.no_grad()
def evaluate_tt(pred, gt, init, crop, dtau: float, max_dist: Optional[float] = None, taus: Optional[Sequence[float]] = None, stages=None,
                refine: bool = True) -> Dict[str, object]:
    """The Tanks-and-Temples score of ``pred`` against ``gt``: :func:`register_tt` (skipped with ``refine=False``: ``init`` as it is), then
    ``pred`` moved and cropped, ``gt`` cropped, and :func:`evaluate` with ``voxel = dtau / 2``, ``taus = (dtau,)`` unless given, and
    ``max_dist`` (default ``5 dtau``; it caps the accuracy / completeness means only).  -> :func:`evaluate`'s dict plus ``T`` (nested
    lists), ``stages`` (fitness, inlier_rmse, iterations, converged per stage) and ``n_pred_cropped`` / ``n_gt_cropped``."""
    dtau = _positive(dtau, "dtau")
    if refine:
        T, results = register_tt(pred, gt, init, crop, dtau, stages)
    else:
        T, results = _matrix(init, "init"), []
    pred_c, gt_c = _crop(transform(pred, T), crop), _crop(_cloud(gt, "gt"), crop)
    out = evaluate(pred_c, gt_c, 5.0 * dtau if max_dist is None else max_dist, (dtau,) if taus is None else taus, voxel=0.5 * dtau)
    out.update(T=T.tolist(), n_pred_cropped=int(pred_c.shape[0]), n_gt_cropped=int(gt_c.shape[0]),
               stages=[dict(fitness=r.fitness, inlier_rmse=r.inlier_rmse, iterations=r.iterations, converged=r.converged) for r in results])
    return out


# ------------------------------------------------------------------------------------------------ DTU's filters (elementwise torch)
def in_box(xyz: torch.Tensor, lo, hi) -> torch.Tensor:
    """``lo <= xyz <= hi`` on every axis -> bool ``[N]`` (DTU's bounding box ``BB``)."""
    lo = torch.as_tensor(lo, dtype=xyz.dtype, device=xyz.device)
    hi = torch.as_tensor(hi, dtype=xyz.dtype, device=xyz.device)
    return ((xyz >= lo) & (xyz <= hi)).all(dim=1)


def in_volume(xyz: torch.Tensor, occupancy: torch.Tensor, origin, res: float) -> torch.Tensor:
    """DTU's observation mask: voxel ``round((xyz - origin) / res)`` of ``occupancy [X,Y,Z]`` (uint8 / bool) is set; a point outside the
    volume is outside the mask -> bool ``[N]``."""
    origin = torch.as_tensor(origin, dtype=xyz.dtype, device=xyz.device)
    occ = occupancy.to(xyz.device)
    q = torch.round((xyz - origin) / float(res))
    shape = torch.tensor(occ.shape, dtype=xyz.dtype, device=xyz.device)
    inside = ((q >= 0) & (q < shape)).all(dim=1)                            # NaN compares false
    qi = torch.where(inside[:, None], q, torch.zeros_like(q)).long()
    return inside & (occ[qi[:, 0], qi[:, 1], qi[:, 2]] != 0)


def above_plane(xyz: torch.Tensor, plane4) -> torch.Tensor:
    """``[x y z 1] . plane4 > 0`` -> bool ``[N]`` (DTU's table plane)."""
    p = torch.as_tensor(plane4, dtype=xyz.dtype, device=xyz.device)
    return (xyz * p[:3]).sum(dim=1) + p[3] > 0
