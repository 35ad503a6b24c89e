"""numpy fp64 restatements of the cloud-alignment entries (include/mvs_hip.h, mvsformer_amd/cloud_eval.py) and the fixtures their tests
share.  Nothing here imports the package: tests/test_cloud_align_refs.py checks these restatements against things that can be known, and
tests/test_hip_cloud_align.py holds the kernels to them."""
import math

import numpy as np

MAX_K = 64                                                                   # MVS_ALIGN_CROP_MAX_K
OTHER_AXES = {0: (1, 2), 1: (0, 2), 2: (0, 1)}                                # X: (Y, Z)   Y: (X, Z)   Z: (X, Y)


# ------------------------------------------------------------------------------------------------------------ transform
def transform_ref(xyz32, T):
    """``round_fp32(((r0 x + r1 y) + r2 z) + t)`` per row, every operation in fp64 in this order."""
    p, T = np.asarray(xyz32, np.float32).astype(np.float64), np.asarray(T, np.float64)
    with np.errstate(all="ignore"):
        cols = [((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)]
        return np.stack(cols, 1).astype(np.float32)


def similarity(angle_deg, axis, scale, shift, about=(0.0, 0.0, 0.0)):
    """4 x 4: rotate by ``angle_deg`` about ``axis`` through ``about``, scale about it, then shift."""
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = math.radians(angle_deg)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    c = np.asarray(about, np.float64)
    T = np.eye(4)
    T[:3, :3] = scale * R
    T[:3, 3] = c - scale * R @ c + np.asarray(shift, np.float64)
    return T


def apply64(T, p):
    return np.asarray(p, np.float64) @ T[:3, :3].T + T[:3, 3]


# ----------------------------------------------------------------------------------------------------------------- crop
def crop_ref(xyz32, axis, axis_min, axis_max, poly_uv):
    """The slab and the even-odd crossing rule, in fp64 from the fp32 coordinates; a non-finite point is out."""
    p = np.asarray(xyz32, np.float32).astype(np.float64).reshape(-1, 3)
    poly = np.asarray(poly_uv, np.float64)
    ua, va = OTHER_AXES[axis]
    u, v, w = p[:, ua], p[:, va], p[:, axis]
    inside = np.zeros(len(p), bool)
    with np.errstate(all="ignore"):
        for k in range(len(poly)):
            (au, av), (bu, bv) = poly[k], poly[(k + 1) % len(poly)]
            straddles = (av > v) != (bv > v)
            cross = (bu - au) * (v - av) / (bv - av) + au
            inside ^= straddles & (u < cross)
        return np.isfinite(p).all(1) & (axis_min <= w) & (w <= axis_max) & inside


TRIANGLE = [(0.0, 0.0), (4.0, 0.0), (0.0, 4.0)]
L_RING = [(0.0, 0.0), (4.0, 0.0), (4.0, 1.0), (1.0, 1.0), (1.0, 4.0), (0.0, 4.0)]            # concave: the notch is x > 1 and y > 1


def star_ring(k=MAX_K, seed=3):
    """A ring of ``k`` vertices, alternately near and far from (2, 2): concave at every other vertex."""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = np.where(np.arange(k) % 2 == 0, 2.5, 1.0) + rng.uniform(-0.2, 0.2, k)
    return np.stack([2.0 + rad * np.cos(ang), 2.0 + rad * np.sin(ang)], 1)


def crop_points(n, poly_uv, axis, seed):
    """``n`` fp32 points around the ring: uniform over its box and beyond, some with ``v`` EQUAL to a vertex's ``v`` (the ``>`` against ``>=``
    edge of the rule), some with ``u`` equal to a vertex's ``u``, some exactly on the slab faces 0 and 1 and one ulp outside them."""
    rng = np.random.default_rng(seed)
    poly = np.asarray(poly_uv, np.float64)
    ua, va = OTHER_AXES[axis]
    p = np.empty((n, 3), np.float32)
    p[:, ua] = rng.uniform(poly[:, 0].min() - 1, poly[:, 0].max() + 1, n)
    p[:, va] = rng.uniform(poly[:, 1].min() - 1, poly[:, 1].max() + 1, n)
    p[:, axis] = rng.uniform(-0.5, 1.5, n)
    i = np.arange(n)
    sel = i % 5 == 1
    p[sel, va] = poly[i[sel] % len(poly), 1].astype(np.float32)
    sel = i % 7 == 2
    p[sel, ua] = poly[i[sel] % len(poly), 0].astype(np.float32)
    faces = np.array([0.0, 1.0, np.nextafter(np.float32(0), np.float32(-1)), np.nextafter(np.float32(1), np.float32(2))], np.float32)
    sel = i % 3 == 0
    p[sel, axis] = faces[(i[sel] // 3) % 4]
    return p


# ------------------------------------------------------------------------------------------------------------ pair sums
def pair_sums_ref(src32, dst32, idx, dist32, origin):
    """-> ``(dict n, n_finite, sp, sq, sqp, spp, sqq, sdd, origin; abs: the same sums over |terms|)``.  Terms are formed as the kernel forms
    them (fp64 differences and products of the fp32 inputs); they are added with ``math.fsum``, i.e. exactly."""
    src, dst = np.asarray(src32, np.float32).astype(np.float64).reshape(-1, 3), np.asarray(dst32, np.float32).astype(np.float64).reshape(-1, 3)
    idx, o = np.asarray(idx, np.int64), np.asarray(origin, np.float64)
    ok = (idx >= 0) & (idx < len(dst))
    p, q, d = src[ok] - o, dst[idx[ok]] - o, np.asarray(dist32, np.float32).astype(np.float64)[ok]
    terms = dict(sp=[p[:, a] for a in range(3)], sq=[q[:, a] for a in range(3)], sqp=[q[:, a] * p[:, b] for a in range(3) for b in range(3)],
                 spp=[(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]], sqq=[(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]],
                 sdd=[d * d])
    sums = {k: np.array([math.fsum(t) for t in v]) for k, v in terms.items()}
    mags = {k: np.array([math.fsum(np.abs(t)) for t in v]) for k, v in terms.items()}
    for s in (sums, mags):
        s["sqp"] = s["sqp"].reshape(3, 3)
        for k in ("spp", "sqq", "sdd"):
            s[k] = float(s[k][0])
    sums.update(n=int(ok.sum()), n_finite=int(np.isfinite(src).all(1).sum()), origin=o)
    return sums, mags


def umeyama_ref(s, with_scaling=True):
    """Umeyama's closed form from the sums ``s`` (a dict as ``pair_sums_ref`` returns); ValueError where it is undetermined."""
    n = s["n"]
    if n < 3:
        raise ValueError("fewer than 3 pairs")
    mp, mq = s["sp"] / n, s["sq"] / n
    cov = s["sqp"] / n - np.outer(mq, mp)
    var_p = s["spp"] / n - mp @ mp
    U, D, Vt = np.linalg.svd(cov)
    if not (np.isfinite(D).all() and var_p > 0 and D[1] > 1e-12 * D[0]):
        raise ValueError("rank-deficient")
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    A = (np.trace(np.diag(D) @ S) / var_p if with_scaling else 1.0) * (U @ S @ Vt)
    T = np.eye(4)
    T[:3, :3] = A
    T[:3, 3] = (mq - A @ mp) + s["origin"] - A @ s["origin"]
    return T


def sums_of_pairs(p, q, origin=(0.0, 0.0, 0.0)):
    """Exact-pair sums in fp64 (no fp32 rounding of the inputs): for the tests of ``umeyama`` itself."""
    o = np.asarray(origin, np.float64)
    p, q = np.asarray(p, np.float64) - o, np.asarray(q, np.float64) - o
    return dict(n=len(p), n_finite=len(p), sp=p.sum(0), sq=q.sum(0), sqp=q.T @ p, spp=float((p * p).sum()), sqq=float((q * q).sum()), sdd=0.0, origin=o)


# ------------------------------------------------------------------------------------------------------------------ icp
def nearest_ref(tree, dst32, moved32, threshold, fp32):
    """-> ``(dist, idx)``: the nearest target strictly within ``threshold`` (else ``threshold``, -1).  ``fp32``: the library's distance
    contract - ``sqrtf((dx*dx + dy*dy) + dz*dz)`` in fp32, ties to the lowest index - over the kd-tree's 8 nearest candidates;
    otherwise the kd-tree's own fp64 distances."""
    k = min(8, len(dst32))
    dd, ii = tree.query(moved32.astype(np.float64), k=k, distance_upper_bound=float(threshold) * (1 + 1e-5))
    dd, ii = dd.reshape(len(moved32), k), ii.reshape(len(moved32), k)
    miss = ii >= len(dst32)
    safe = np.where(miss, 0, ii)
    if fp32:
        d = moved32[:, None, :].astype(np.float32) - dst32[safe].astype(np.float32)
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        dd = np.where(miss, np.float32(np.inf), np.sqrt(d2)).astype(np.float32)
        best = dd.min(1)
        idx = np.where(dd == best[:, None], safe, np.iinfo(np.int64).max).min(1)
        hit = best < np.float32(threshold)
        return np.where(hit, best, np.float32(threshold)).astype(np.float32), np.where(hit, idx, -1)
    hit = dd[:, 0] < threshold
    return np.where(hit, dd[:, 0], threshold), np.where(hit, safe[:, 0], -1)


def icp_ref(src32, dst32, threshold, init=None, with_scaling=True, max_iter=20, fitness_tol=1e-6, rmse_tol=1e-6, fp32=True):
    """``cloud_eval.icp`` restated over ``scipy.spatial.cKDTree``: the moved source rounded to fp32 as the device rounds it, the search capped
    at ``threshold``, the sums about the target's bounding-box centre -> ``(T, fitness, rmse, iterations, converged)``."""
    from scipy.spatial import cKDTree
    src32, dst32 = np.asarray(src32, np.float32), np.asarray(dst32, np.float32)
    tree = cKDTree(dst32.astype(np.float64))
    origin = 0.5 * (dst32.min(0).astype(np.float64) + dst32.max(0).astype(np.float64))
    T = np.eye(4) if init is None else np.array(init, np.float64)
    prev, it, converged = None, 0, False
    while it < max_iter:
        moved = transform_ref(src32, T)
        dist, idx = nearest_ref(tree, dst32, moved, threshold, fp32)
        s, _ = pair_sums_ref(moved, dst32, idx, dist, origin) if fp32 else _sums64(moved, dst32, idx, dist, origin)
        it += 1
        if s["n"] == 0:
            raise ValueError("no correspondences")
        fitness, rmse = s["n"] / s["n_finite"], math.sqrt(s["sdd"] / s["n"])
        if prev is not None and abs(fitness - prev[0]) < fitness_tol and abs(rmse - prev[1]) < rmse_tol:
            converged = True
            break
        prev = (fitness, rmse)
        T = umeyama_ref(s, with_scaling) @ T
    return T, fitness, rmse, it, converged


def _sums64(moved, dst32, idx, dist64, origin):
    s, m = pair_sums_ref(moved, dst32, idx, np.zeros(len(idx), np.float32), origin)
    d = np.asarray(dist64, np.float64)[idx >= 0]
    s["sdd"] = math.fsum(d * d)
    return s, m


# ------------------------------------------------------------------------------------------------------------- fixtures
def height(x, y):
    return 3.0 * np.sin(0.5 * x + 0.4) * np.cos(0.45 * y) + 0.004 * x * y + 0.6 * np.sin(0.05 * x * x / 8.0)


def sheet(n=40, seed=11):
    """A jittered ``n x n`` grid on a bumpy sheet without a symmetry -> ``(fp32 [n*n,3], its smallest point spacing)``."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    x, y = i.ravel() + rng.uniform(-0.2, 0.2, n * n), j.ravel() + rng.uniform(-0.2, 0.2, n * n)
    pts = np.stack([x, y, height(x, y)], 1).astype(np.float32)
    s = float(cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=2)[0][:, 1].min())
    return pts, s


BASE_SIMILARITY = dict(angle_deg=2.0, axis=(0.3, -0.2, 1.0), scale_minus_1=0.01, shift=(0.02, -0.015, 0.01))


def exact_case(n=40, seed=11):
    """-> ``(src, dst, T_true, s)``: ``dst`` = the sheet, ``src`` = ``inverse(T_true) dst`` rounded to fp32.  ``T_true`` is BASE_SIMILARITY
    about the sheet's centre with angle, scale - 1 and shift multiplied by one factor, chosen so that the largest displacement
    ``|src_i - dst_i|`` is 0.45 of the smallest spacing: every first correspondence is then the true one (another target is at least
    0.55 spacings away).  (At the full 2 degrees and 1.01 a corner of a 40 x 40 grid moves by more than a spacing.)"""
    dst, s = sheet(n, seed)
    centre = dst.astype(np.float64).mean(0)

    def make(f):
        b = BASE_SIMILARITY
        T = similarity(f * b["angle_deg"], b["axis"], 1.0 + f * b["scale_minus_1"], f * np.asarray(b["shift"]), about=centre)
        src = apply64(np.linalg.inv(T), dst).astype(np.float32)
        return T, src, float(np.linalg.norm(src.astype(np.float64) - dst.astype(np.float64), axis=1).max())

    f = 1.0
    for _ in range(60):                                                      # the displacement is close to linear in f
        f *= 0.45 * s / make(f)[2]
    while make(f)[2] > 0.45 * s:
        f *= 1.0 - 1e-6
    T, src, _ = make(f)
    return src, dst, T, s


def general_case(m=5000, seed=5, outliers=0.2, noise=0.03, threshold=2.5):
    """-> ``(src, dst, T_true, init, threshold)``: ``dst`` = the sheet; ``src`` = ``m`` points sampled between its points with Gaussian
    noise, 20 % of them lifted off the sheet by more than 3 thresholds, all moved by ``inverse(T_true)``; ``init`` is off by several
    spacings (a shift of about 2 and a degree of rotation)."""
    dst, _ = sheet()
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(1.0, 38.0, m), rng.uniform(1.0, 38.0, m)
    p = np.stack([x, y, height(x, y)], 1) + rng.normal(0.0, noise, (m, 3))
    out = rng.random(m) < outliers
    p[out, 2] += rng.choice([-1.0, 1.0], int(out.sum())) * rng.uniform(3.0 * threshold + 2.0, 6.0 * threshold, int(out.sum()))
    centre = dst.astype(np.float64).mean(0)
    T_true = similarity(2.0, (0.3, -0.2, 1.0), 1.01, (0.3, -0.2, 0.1), about=centre)
    src = apply64(np.linalg.inv(T_true), p).astype(np.float32)
    init = similarity(1.0, (0.1, 0.2, 1.0), 1.0, (1.4, -1.2, 0.5), about=centre) @ T_true
    return src, dst, T_true, init, threshold


def tt_scene(n=30000, seed=9):
    """-> ``(pred, gt, T_true, init, crop, dtau)``.  ``gt`` (the scanner's frame): ``n`` points on the bumpy sheet over 40 x 40 without the
    strip 28 <= x < 30.  ``pred``: the ground-truth points with x < 28 - the same points, so that under the true transform their
    distances are fp32 roundings and no distance lies near ``dtau`` - moved into an arbitrary frame by ``inverse(T_true)`` (25 degrees,
    scale 2.5).  The part x >= 30 is missing from the reconstruction: recall < 1.  ``crop``: the L-shaped ring scaled to the sheet and a
    slab in z, which cut most of both clouds away.  ``init`` = ``T_true`` off by 0.4 degrees, 0.4 % of scale and a shift of
    (0.12, -0.1, 0.6): 0.6 along z is more than 2 ``dtau`` off the surface.  (Gross outliers in ``pred`` - tried: a fifth as many points
    3 to 4 off the sheet - pull the first two stages, whose thresholds of 80 and 20 ``dtau`` admit them, far enough that the third
    stage ends in a local optimum 0.02 from the truth, in the restated loop exactly as on the device; that is a property of the
    protocol, not of the kernels, and is left out of this fixture.)"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0.0, 40.0, n), rng.uniform(0.0, 40.0, n)
    keep = (x < 28.0) | (x >= 30.0)
    gt = np.stack([x, y, height(x, y)], 1)[keep].astype(np.float32)
    seen = gt[gt[:, 0] < 28.0].astype(np.float64)
    centre = np.array([20.0, 20.0, 0.0])
    T_true = similarity(25.0, (0.2, 0.1, 1.0), 2.5, (3.0, -2.0, 1.0), about=centre)
    pred = apply64(np.linalg.inv(T_true), seen).astype(np.float32)
    init = similarity(0.4, (0.1, -0.3, 1.0), 1.004, (0.12, -0.1, 0.6), about=centre) @ T_true
    poly = np.array([(8.0 * u + 4.0, 8.0 * v + 4.0, 0.0) for u, v in L_RING])
    crop = dict(orthogonal_axis="Z", axis_min=-8.0, axis_max=8.0, bounding_polygon=poly)
    return pred, gt, T_true, init, crop, 0.25
