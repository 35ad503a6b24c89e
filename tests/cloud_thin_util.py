"""The yardstick of the greedy-thinning tests, numpy only: DTU's sequential rule as include/mvs_hip.h states it, brute force with fp64
distances over the fp32 inputs, seeded case builders, and the premise that lets an fp32 kernel be held to exact equality
(``clear_of_radius``: no pair distance within 8 fp32 ulp of the radius, the margin of tests/cloud_eval_util.py)."""
import functools

import numpy as np

from cloud_eval_util import ULPS, cell_index, eval_clouds, f32, min_separation, plane_patch

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 5000)
LINE_SIZES = (65, 257)


def greedy_ref(xyz, dist, order):
    """Visit the points in ``order``; a visited point that has not been removed is kept and removes every other point at distance
    ``<= float(np.float32(dist))``.  Non-finite points are never kept and remove nothing.  -> keep bool ``[N]``."""
    p = f32(xyz).astype(np.float64)
    n = len(p)
    order = np.asarray(order, dtype=np.int64)
    assert sorted(order.tolist()) == list(range(n))
    d = float(np.float32(dist))
    good = np.isfinite(p).all(axis=1)
    keep, removed = np.zeros(n, bool), np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        for i in order:
            if not good[i] or removed[i]:
                continue
            keep[i] = True
            near = np.sqrt(((p - p[i]) ** 2).sum(axis=1)) <= d             # a non-finite row gives nan or inf: never near
            near[i] = False
            removed |= near
    return keep


def pair_distances(xyz, chunk=512):
    """Yields ``(first row, float64 [rows, N])`` blocks of the distance matrix over the finite points' rows (non-finite: inf)."""
    p = f32(xyz).astype(np.float64)
    good = np.isfinite(p).all(axis=1)
    q = np.where(good[:, None], p, 0.0)
    for a in range(0, len(p), chunk):
        d = np.sqrt(((q[a:a + chunk, None, :] - q[None, :, :]) ** 2).sum(axis=2))
        d[~good[a:a + chunk], :] = np.inf
        d[:, ~good] = np.inf
        yield a, d


def clear_of_radius(xyz, dist, ulps=ULPS):
    """No pair distance within ``ulps`` fp32 ulp of ``dist``: ``d2 <= dist*dist`` in fp32 and ``d <= dist`` in fp64 then agree (the fp32
    path: three subtractions, three squares, two adds and the rounding of ``dist*dist`` - under 3 ulp of the distance)."""
    d32 = float(np.float32(dist))
    band = ulps * float(np.spacing(np.float32(dist)))
    return all(bool((np.abs(d - d32) > band).all()) for _, d in pair_distances(xyz))


def invariants(xyz, dist, order, keep):
    """The two properties of a valid result: kept points are pairwise farther apart than ``dist``; every removed finite point has a kept
    neighbour of lower rank within ``dist``; non-finite points are not kept."""
    p = f32(xyz)
    n = len(p)
    d32 = float(np.float32(dist))
    rank = np.empty(n, np.int64)
    rank[np.asarray(order, np.int64)] = np.arange(n)
    good = np.isfinite(p).all(axis=1)
    if keep[~good].any():
        return False
    for a, d in pair_distances(p):
        rows = np.arange(a, a + len(d))
        near = d <= d32
        near[np.arange(len(d)), rows] = False
        if (near & keep[rows][:, None] & keep[None, :]).any():
            return False
        shield = (near & keep[None, :] & (rank[None, :] < rank[rows][:, None])).any(axis=1)
        if (shield != (good[rows] & ~keep[rows])).any():
            return False
    return True


def thin_cell(xyz, dist):
    """``cloud_eval.thin_cell`` restated: -> ``(origin float32 [3], cell)`` of the grid a thinning of ``xyz`` with ``dist`` builds."""
    p = f32(xyz)
    p = p[np.isfinite(p).all(axis=1)]
    lo, hi = p.min(axis=0), p.max(axis=0)
    ext = max(float(hi[a]) - float(lo[a]) for a in range(3))
    cell = max(1.0001 * dist + ext * 2.0 ** -21, ext * 2.0 ** -20)
    return lo, float(np.float32(cell) * np.float32(1.0 + 2.0 ** -20))


# ------------------------------------------------------------------------------------------------------------ builders
def shuffle(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def plane_case(n, seed=0):
    """A noisy plane patch of ``n`` points and the radius at which a point has about 5 neighbours."""
    size = 60.0
    dist = float(np.sqrt(5.0 * size * size / (np.pi * max(n, 1))))
    return dict(xyz=plane_patch(n, 4000 + 10 * n + seed, size=size), dist=dist, order=shuffle(n, 5000 + n))


def line_case(n, how):
    """``n`` points on a line, 0.6 * dist apart: only adjacent points are neighbours.  In sorted order every other point is kept and the
    parallel form needs about ``n`` rounds (each decision waits for the previous point's)."""
    xyz = np.zeros((n, 3))
    xyz[:, 0] = np.arange(n) * 0.6
    order = {"sorted": np.arange(n), "reverse": np.arange(n)[::-1], "shuffle": shuffle(n, 600 + n)}[how]
    return dict(xyz=f32(xyz), dist=1.0, order=np.ascontiguousarray(order, dtype=np.int64))


FACE_KINDS = (("face", (1.0, 0.0, 0.0)), ("edge", (1.0, 1.0, 0.0)), ("corner", (1.0, 1.0, 1.0)))


def faces_case():
    """Pairs that straddle a face, an edge and a corner of the thinning's grid, 1e-4 (relative) under and over ``dist`` apart - a thousand
    times the 8-ulp band - three cells from the next pair.  ``pairs``: (kind, under, index a, index b)."""
    dist, ext = 1.0, 20.0
    anchors = [[0.0, 0.0, 0.0], [ext, ext, ext]]
    _, cell = thin_cell(anchors, dist)
    pts, pairs, k = list(anchors), [], 2
    for kind, u in FACE_KINDS:
        u = np.asarray(u) / np.linalg.norm(u)
        for under in (True, False):
            s = dist * (1.0 - 1e-4 if under else 1.0 + 1e-4)
            c = np.where(np.asarray(u) > 0, k * cell, (k + 0.5) * cell)   # on the face(s) the pair straddles, mid-cell on the other axes
            pairs.append((kind, under, len(pts), len(pts) + 1))
            pts += [c - 0.05 * s * u, c + 0.95 * s * u]
            k += 3
    xyz = f32(pts)
    return dict(xyz=xyz, dist=dist, order=shuffle(len(xyz), 77), pairs=pairs)


def duplicates_case():
    """The same 300 points three times over, at a radius below their smallest separation: one copy of each survives."""
    base = plane_patch(300, 41)
    r = np.random.default_rng(42)
    src = np.tile(np.arange(300), 3)[r.permutation(900)]                    # src[i]: the base point row i repeats
    return dict(xyz=f32(base[src]), dist=0.5 * min_separation(base), order=shuffle(900, 43), src=src)


def non_finite_case():
    c = plane_case(500, seed=3)
    xyz = c["xyz"].copy()
    xyz[::37, 0] = np.nan
    xyz[5, 1] = np.inf
    xyz[11, 2] = -np.inf
    xyz[12] = np.nan
    return dict(xyz=xyz, dist=c["dist"], order=c["order"])


def eval_case():
    """A prediction to thin inside ``evaluate`` (with a mask that drops a third of it) against a ground truth."""
    pred, gt, md = eval_clouds()["plane"]
    mask = np.random.default_rng(44).uniform(size=len(pred)) > 1.0 / 3.0
    xyz = np.where(mask[:, None], pred, np.float32(np.nan))                 # what evaluate thins: masked-out points are non-finite
    return dict(xyz=f32(xyz), dist=0.8, order=shuffle(len(pred), 45), pred=pred, gt=gt, max_dist=md, taus=(0.5 * md, md), mask=mask)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(xyz, dist, order, ...); built once per process, not to be written to."""
    out = {"size_%d" % n: plane_case(n) for n in SIZES}
    for n in LINE_SIZES:
        for how in ("sorted", "reverse", "shuffle"):
            out["line_%d_%s" % (n, how)] = line_case(n, how)
    out["faces"] = faces_case()
    out["duplicates"] = duplicates_case()
    out["non_finite"] = non_finite_case()
    out["other_seed"] = dict(plane_case(257), order=shuffle(257, 9))         # the points of size_257 in another order
    out["eval"] = eval_case()
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> ``(case, keep)``: the yardstick of one case, computed once per process and not to be written to."""
    case = cases()[name]
    keep = greedy_ref(case["xyz"], case["dist"], case["order"])
    keep.setflags(write=False)
    return case, keep
