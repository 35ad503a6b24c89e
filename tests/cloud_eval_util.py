"""The yardstick of the point-cloud evaluation tests, numpy only: brute-force nearest neighbours in fp64 over the fp32 inputs, the cell rule
in ``np.float32`` (the kernel's two IEEE operations), centroids and means in fp64, seeded cloud builders and the shared test cases."""
import functools

import numpy as np

AXIS_BITS = 21
ULPS = 8                                   # fp32 path: three subtractions, three squares, two adds, a square root: ~3 ulp worst case
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 5000)


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3))


def brute_nn(src, dst, max_dist, chunk=512):
    """-> ``(dist float64 [M] capped, idx int64 [M], raw float64 [M])``: the fp64 distance to the nearest finite target (``raw``; inf when
    there is none or the query is not finite), ``dist`` = ``raw`` where ``raw < max_dist`` else ``max_dist`` with index -1; ties -> lowest
    index (``argmin`` returns the first minimum)."""
    src, dst = f32(src).astype(np.float64), f32(dst).astype(np.float64)
    md = float(np.float32(max_dist))
    M = src.shape[0]
    raw, idx = np.full(M, np.inf), np.full(M, -1, dtype=np.int64)
    good = np.isfinite(dst).all(axis=1)
    if good.any():
        with np.errstate(invalid="ignore"):
            for a in range(0, M, chunk):
                d = src[a:a + chunk, None, :] - dst[None, :, :]
                d2 = (d * d).sum(axis=2)
                d2[:, ~good] = np.inf
                d2[~np.isfinite(d2)] = np.inf
                j = d2.argmin(axis=1)
                raw[a:a + chunk] = np.sqrt(d2[np.arange(j.size), j])
                idx[a:a + chunk] = j
    hit = raw < md
    return np.where(hit, raw, md), np.where(hit, idx, -1), raw


def cell_index(xyz, origin, cell):
    """``floorf((x - origin) / cell)`` in fp32 -> int64 ``[N,3]``."""
    xyz = f32(xyz)
    return np.floor((xyz - np.asarray(origin, np.float32)) / np.float32(cell)).astype(np.int64)


def voxel_centroids(xyz, voxel, attrs=()):
    """-> ``(keys int64 [C] ascending, [centroids float64 [C,3]] + [attr means])`` over the finite points; sums run in original order."""
    xyz = f32(xyz)
    good = np.isfinite(xyz).all(axis=1)
    if not good.any():
        return np.zeros(0, np.int64), [np.zeros((0, 3)) for _ in range(1 + len(attrs))]
    origin = xyz[good].min(axis=0)
    c = cell_index(xyz[good], origin, voxel)
    assert c.min() >= 0 and c.max() < (1 << AXIS_BITS)
    key = c[:, 0] | (c[:, 1] << AXIS_BITS) | (c[:, 2] << (2 * AXIS_BITS))
    keys, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    outs = []
    for a in [xyz] + [np.asarray(t) for t in attrs]:
        s = np.zeros((keys.size, 3))
        np.add.at(s, inv, a[good].astype(np.float64))                      # unbuffered: adds in index order
        outs.append(s / cnt[:, None])
    return keys, outs


def evaluate_ref(pred, gt, max_dist, taus=(), voxel=None, pred_mask=None, gt_mask=None):
    """The scores ``cloud_eval.evaluate`` returns, and ``all_dist``: every uncapped fp64 distance that was scored."""
    clouds = []
    for xyz, m in ((pred, pred_mask), (gt, gt_mask)):
        xyz = f32(xyz)
        ok = np.isfinite(xyz).all(axis=1)
        if m is not None:
            ok &= np.asarray(m, bool)
        xyz = xyz[ok]
        if voxel is not None:
            xyz = voxel_centroids(xyz, voxel)[1][0].astype(np.float32)     # the function returns fp32 points
        clouds.append(xyz)
    md = float(np.float32(max_dist))
    out, raws = dict(n_pred=len(clouds[0]), n_gt=len(clouds[1]), taus=[float(t) for t in taus]), []
    for name, mean, cnt, share, src, dst in (("pred", "accuracy", "pred_below_tau", "precision", clouds[0], clouds[1]),
                                             ("gt", "completeness", "gt_below_tau", "recall", clouds[1], clouds[0])):
        raw = brute_nn(src, dst, max_dist)[2]
        raws.append(raw)
        below = raw[raw < md]
        out[name + "_below_max"] = int(below.size)
        out[mean] = float(below.mean()) if below.size else float("nan")
        out[cnt] = [int((raw < float(np.float32(t))).sum()) for t in taus]
        out[share] = [c / len(src) if len(src) else float("nan") for c in out[cnt]]
    out["overall"] = 0.5 * (out["accuracy"] + out["completeness"])
    out["fscore"] = [(2 * p * r / (p + r) if p + r > 0 else 0.0) if p == p and r == r else float("nan")
                     for p, r in zip(out["precision"], out["recall"])]
    out["all_dist"] = np.concatenate(raws) if raws else np.zeros(0)
    return out


def clear_of(raw, bound, ulps=ULPS):
    """No finite distance within ``ulps`` fp32 ulp of ``bound``: the fp32 and the fp64 comparison then agree."""
    raw = raw[np.isfinite(raw)]
    return bool((np.abs(raw - float(np.float32(bound))) > ulps * float(np.spacing(np.float32(bound)))).all())


# ------------------------------------------------------------------------------------------------------------ builders
def plane_patch(n, seed, size=60.0, noise=0.05, centre=(-20.0, 5.0, -30.0)):
    """A noisy, tilted plane patch around ``centre`` (negative coordinates included)."""
    r = np.random.default_rng(seed)
    u, v = r.uniform(-0.5, 0.5, n) * size, r.uniform(-0.5, 0.5, n) * size
    p = np.stack([u, v, 0.3 * u - 0.2 * v], axis=1) + r.normal(0.0, noise, (n, 3)) + np.asarray(centre)
    return f32(p)


def sphere_shell(n, seed, radius=25.0, noise=0.05, centre=(10.0, -15.0, 40.0)):
    r = np.random.default_rng(seed)
    d = r.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True) + 1e-30
    return f32(d * (radius + r.normal(0.0, noise, (n, 1))) + np.asarray(centre))


def cluster_outliers(n, n_out, seed, spread=3.0, far=400.0):
    """A Gaussian cluster at the origin and ``n_out`` outliers on a shell ``far`` away from it (and from each other's cells)."""
    r = np.random.default_rng(seed)
    c = r.normal(0.0, spread, (n, 3)).clip(-4 * spread, 4 * spread)
    d = r.normal(size=(n_out, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True) + 1e-30
    return f32(np.concatenate([c, d * far]))


def min_separation(dst):
    """The smallest distance between two DISTINCT finite targets (inf for fewer than two)."""
    d = np.unique(f32(dst)[np.isfinite(f32(dst)).all(axis=1)], axis=0).astype(np.float64)
    best = np.inf
    for a in range(0, len(d), 512):
        d2 = ((d[a:a + 512, None, :] - d[None, :, :]) ** 2).sum(axis=2)
        d2[np.arange(min(512, len(d) - a)), np.arange(a, min(a + 512, len(d)))] = np.inf
        best = min(best, float(np.sqrt(d2.min()))) if d2.size else best
    return best


# --------------------------------------------------------------------------------------------------------------- cases
def size_case(m, n):
    """M queries against N targets on the same noisy patch (negative coordinates, targets about 0.85 apart): some capped, some not."""
    return dict(src=plane_patch(m, 1000 + m, noise=0.3), dst=plane_patch(n, 2000 + n), max_dist=0.6, cell=None)


def geometry_cases():
    """name -> dict(src, dst, max_dist, cell[, exact=(query, expected index)])."""
    r = np.random.default_rng(7)
    cases = {}
    cases["negative"] = dict(src=plane_patch(257, 11, centre=(-300.0, -200.0, -100.0), noise=0.3),
                             dst=plane_patch(5000, 12, centre=(-300.0, -200.0, -100.0)), max_dist=2.0, cell=None)
    lat = 0.5                                                                # every coordinate an integer multiple of the cell
    cases["cell_faces"] = dict(src=f32(r.integers(-40, 40, (300, 3)) * lat), dst=f32(r.integers(-40, 40, (5000, 3)) * lat), max_dist=2.9, cell=lat)   # 2.9 is no lattice distance
    cases["one_cell"] = dict(src=f32(r.uniform(-2.0, 5.0, (257, 3))), dst=f32(r.uniform(0.05, 3.5, (5000, 3))), max_dist=4.0, cell=4.0)
    base = sphere_shell(700, 13)
    dup = np.concatenate([base, base, base[:100]])[r.permutation(1500)]
    cases["duplicates"] = dict(src=sphere_shell(257, 14, noise=0.5), dst=f32(dup), max_dist=3.0, cell=None)
    cases["outliers"] = dict(src=cluster_outliers(300, 20, 15), dst=cluster_outliers(1000, 30, 16), max_dist=5.0, cell=None)
    cases["far_queries"] = dict(src=f32(np.concatenate([plane_patch(100, 17) + 900.0, plane_patch(100, 18) - np.float32(800.0), plane_patch(57, 19)])),
                                dst=plane_patch(2000, 20), max_dist=2.0, cell=None)
    # a 3-4-5 triangle: the nearest target of query 0 sits at exactly max_dist (in fp32 and in fp64) -> capped; query 1 has one at 2.5
    dst = f32(np.concatenate([[[3.0, 4.0, 0.0], [40.0, 0.0, 0.0], [1.5, 2.0, 20.0]], plane_patch(200, 21, centre=(200.0, 200.0, 0.0))]))
    cases["at_max_dist"] = dict(src=f32([[0.0, 0.0, 0.0], [1.5, 2.0, 17.5]]), dst=dst, max_dist=5.0, cell=None, exact=(0, -1), deliberate=0)
    # query 0 is 1 away from targets 2, 5 and 6: the lowest index wins
    dst = f32(np.concatenate([[[9.0, 9.0, 9.0], [-7.0, 3.0, 2.0], [1.0, 0.0, 0.0], [5.0, 5.0, -5.0], [0.0, 6.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]],
                              plane_patch(100, 22, centre=(100.0, 0.0, 0.0))]))
    cases["exact_tie"] = dict(src=f32([[0.0, 0.0, 0.0], [4.0, 4.0, -4.0]]), dst=dst, max_dist=3.0, cell=None, exact=(0, 2))
    src, dst = plane_patch(257, 23, noise=0.3), plane_patch(5000, 24)
    cases["cell_is_max_dist"] = dict(src=src, dst=dst, max_dist=2.0, cell=2.0)
    cases["cell_is_16th"] = dict(src=src, dst=dst, max_dist=2.0, cell=2.0 / 16)
    cases["default_cell"] = dict(src=src, dst=dst, max_dist=2.0, cell=None)
    nf = dst.copy()
    nf[::97, 1] = np.nan
    nf[5, 0] = np.inf
    qn = src.copy()
    qn[3, 2] = np.nan
    cases["non_finite"] = dict(src=qn, dst=nf, max_dist=2.0, cell=None)
    return cases


def eval_clouds():
    """name -> (pred, gt, max_dist): a reconstruction with noise and outliers against a cleaner ground truth."""
    return {"plane": (plane_patch(3000, 31, noise=0.4), plane_patch(4000, 32), 2.0),
            "sphere": (sphere_shell(2500, 33, noise=0.5), sphere_shell(3000, 34), 2.5),
            "cluster": (cluster_outliers(1500, 40, 35), cluster_outliers(2000, 10, 36, spread=2.5), 1.5)}


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    """The brute force of one case, computed once per process: ('size', (m, n)) or ('geometry', name)."""
    case = size_case(*name) if kind == "size" else geometry_cases()[name]
    return case, brute_nn(case["src"], case["dst"], case["max_dist"])
