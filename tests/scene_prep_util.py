"""Yardsticks of the scene-preparation tests: numpy restatements of the rule in include/mvs_scene_prep.h ("Scene preparation") and a seeded
synthetic scene.  The scores are restated in float64 by the plain double loop over view pairs and common points, the ranking by Python's
stable ``sorted(..., reverse=True)``, the depths in float32 operation by operation with ``np.sort`` for the order statistics.  Nothing
here imports the package."""
import numpy as np

THETA0, SIGMA1, SIGMA2, LO, HI = 5.0, 1.0, 10.0, 0.01, 0.99
DEG = 180.0 / np.pi


# ------------------------------------------------------------------------------------------------------------------ scenes
def look_at(C, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """World-to-camera (R, t) float64 of a camera at C whose +z axis points at ``target``."""
    C = np.asarray(C, np.float64)
    z = np.asarray(target, np.float64) - C
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ C


def ring_scene(V, N, seed, track=6.0, radius=4.0, blob=0.6, twins=(), lonely=(), arc=2.0 * np.pi):
    """V cameras on a ring (on its first ``arc`` radians) looking at a Gaussian blob of N points; per point a track length drawn from Poisson(track) clipped to
    [0, V] (so some points are seen by 0 and by 1 view) and that many distinct views.  ``twins``: pairs (a, b) - view b gets view a's pose
    AND its observations (tied scores against every third view).  ``lonely``: views that observe nothing.  float32 xyz / R / t."""
    rng = np.random.default_rng(seed)
    ang = np.sort(rng.uniform(0.0, arc, V))
    R = np.zeros((V, 3, 3))
    t = np.zeros((V, 3))
    for v in range(V):
        r = radius * rng.uniform(0.9, 1.1)
        R[v], t[v] = look_at((r * np.cos(ang[v]), r * np.sin(ang[v]), rng.uniform(-0.5, 0.5)))
    for a, b in twins:
        R[b], t[b] = R[a], t[a]
    xyz = rng.normal(0.0, blob, (N, 3))
    skip = set(lonely) | {b for _, b in twins}
    views = [v for v in range(V) if v not in skip]
    obs_p, obs_v = [], []
    lengths = np.minimum(rng.poisson(track, N), len(views))
    if N >= 3:
        lengths[-2:] = (1, 0)                                     # always present: a point seen by one view and one seen by none
    for p in range(N):
        n = int(lengths[p])
        for v in rng.choice(views, n, replace=False) if n else ():
            obs_p.append(p)
            obs_v.append(int(v))
    for a, b in twins:
        obs_p += [p for p, v in zip(obs_p, obs_v) if v == a]
        obs_v += [b] * (len(obs_p) - len(obs_v))
    order = rng.permutation(len(obs_p))
    return {"xyz": xyz.astype(np.float32), "obs_point": np.array(obs_p, np.int64)[order], "obs_view": np.array(obs_v, np.int32)[order],
            "R": R.astype(np.float32), "t": t.astype(np.float32)}


# ------------------------------------------------------------------------------------------------------------ restatements
def visibility_ref(xyz, obs_point, obs_view, V):
    """-> (seen [V,N] bool, number of non-finite points); raises ValueError on an index out of range."""
    N = len(xyz)
    obs_point, obs_view = np.asarray(obs_point, np.int64), np.asarray(obs_view, np.int64)
    if ((obs_point < 0) | (obs_point >= N) | (obs_view < 0) | (obs_view >= V)).any():
        raise ValueError("observation out of range")
    seen = np.zeros((V, N), bool)
    seen[obs_view, obs_point] = True
    finite = np.isfinite(np.asarray(xyz, np.float32)).all(1)
    seen[:, ~finite] = False
    return seen, int((~finite).sum())


def pack_bits(seen):
    """[V,N] bool -> [V, ceil(N/64)] uint64, bit p % 64 of word p // 64."""
    V, N = seen.shape
    W = (N + 63) // 64
    pad = np.zeros((V, W * 64), bool)
    pad[:, :N] = seen
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    return (pad.reshape(V, W, 64).astype(np.uint64) * weights).sum(2, dtype=np.uint64)


def centers_ref(R, t):
    R, t = np.asarray(R, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    return -((R[:, 0, :] * t[:, 0:1] + R[:, 1, :] * t[:, 1:2]) + R[:, 2, :] * t[:, 2:3])


def term_ref(Ci, Cj, p, theta0=THETA0, sigma1=SIGMA1, sigma2=SIGMA2):
    """g(theta_ij(p)) and theta for ONE point, scalar float64 arithmetic in the header's order."""
    a, b = Ci - p, Cj - p
    c = np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    theta = np.arctan2(np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) * DEG
    d, s = theta - theta0, (sigma1 if theta <= theta0 else sigma2)
    return float(np.exp(-(d * d) / (2.0 * s * s))), float(theta)


def pair_scores_ref(seen, xyz, R, t, theta0=THETA0, sigma1=SIGMA1, sigma2=SIGMA2):
    """S [V,V] float64 by the plain double loop over pairs; the common points of a pair are evaluated as arrays and added in index order."""
    V = len(R)
    C = centers_ref(R, t)
    P = np.asarray(xyz, np.float32).astype(np.float64)
    S = np.zeros((V, V))
    for i in range(V):
        for j in range(i + 1, V):
            p = P[seen[i] & seen[j]]
            if not len(p):
                continue
            a, b = C[i] - p, C[j] - p
            c0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
            c1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
            c2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
            theta = np.arctan2(np.sqrt((c0 * c0 + c1 * c1) + c2 * c2), (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]) * DEG
            d, s = theta - theta0, np.where(theta <= theta0, sigma1, sigma2)
            total = 0.0
            for g in np.exp(-(d * d) / (2.0 * s * s)):
                total += float(g)
            S[i, j] = S[j, i] = total
    return S


def rank_ref(S, k):
    """-> (src [V,k] int32, score [V,k] float64) by a stable descending sort; -1 / 0 past V - 1 sources."""
    V = len(S)
    src, score = np.full((V, k), -1, np.int32), np.zeros((V, k))
    for i in range(V):
        ranked = sorted(((S[i, j], j) for j in range(V) if j != i), key=lambda e: e[0], reverse=True)[:k]
        for r, (s, j) in enumerate(ranked):
            src[i, r], score[i, r] = j, s
    return src, score


def rank_gaps_ok(S, k, tied=(), rel=1e-6):
    """The condition of the ranking tests on a restated S: inside the first k ranks (and at the boundary to rank k) consecutive scores
    differ by more than ``rel`` of the row maximum, unless they are EXACTLY equal and either both 0 (views that share no point) or the two
    views are a constructed twin pair.  With it, no disagreement in the order can be put down to rounding."""
    V = len(S)
    twins = {frozenset(p) for p in tied}
    for i in range(V):
        ranked = sorted(((S[i, j], j) for j in range(V) if j != i), key=lambda e: e[0], reverse=True)
        top = max(S[i].max(), 1e-300)
        for (s0, j0), (s1, j1) in zip(ranked[:k], ranked[1:k + 1]):
            if s0 == s1 and (s0 == 0.0 or frozenset((j0, j1)) in twins):
                continue
            if not s0 - s1 > rel * top:
                return False
    return True


def depths_ref(seen_row, xyz, R_v, t_v):
    """float32 z of the points of one view in ascending point order, each operation rounded on its own: ((r20 x + r21 y) + r22 z) + t2."""
    p = np.asarray(xyz, np.float32)[seen_row]
    r, t2 = np.asarray(R_v, np.float32)[2], np.float32(np.asarray(t_v, np.float32)[2])
    return ((r[0] * p[:, 0] + r[1] * p[:, 1]) + r[2] * p[:, 2]) + t2


def depth_ranges_ref(seen, xyz, R, t, lo=LO, hi=HI):
    """-> (range [V,2] float32, n [V] int64): sorted[min(int(n lo), n - 1)], sorted[min(int(n hi), n - 1)]; (0, 0) for a view without points."""
    V = len(R)
    rng, n = np.zeros((V, 2), np.float32), np.zeros(V, np.int64)
    for v in range(V):
        z = np.sort(depths_ref(seen[v], xyz, R[v], t[v]))
        n[v] = len(z)
        if len(z):
            rng[v] = z[min(int(len(z) * lo), len(z) - 1)], z[min(int(len(z) * hi), len(z) - 1)]
    return rng, n


def prepare_ref(scene, num_views=20, num_depth=192, interval_scale=1.0, keep_zero=False):
    V = len(scene["R"])
    seen, _ = visibility_ref(scene["xyz"], scene["obs_point"], scene["obs_view"], V)
    S = pair_scores_ref(seen, scene["xyz"], scene["R"], scene["t"])
    src, score = rank_ref(S, num_views)
    rng, n = depth_ranges_ref(seen, scene["xyz"], scene["R"], scene["t"])
    pairs = [(v, [int(j) for j, s in zip(src[v], score[v]) if j >= 0 and (keep_zero or s > 0.0)]) for v in range(V)]
    interval = (rng[:, 1].astype(np.float64) - rng[:, 0].astype(np.float64)) / (num_depth - 1) / interval_scale
    return {"pairs": pairs, "S": S, "depth_min": rng[:, 0], "depth_max": rng[:, 1], "depth_interval": interval, "n_points": n}


# ------------------------------------------------------------------------------------------------------- the hand-computed case
def hand_case():
    """3 views, 4 points, every number known in closed form.  Cameras with R = I: C0 = (0,0,0), C1 = (1,0,0), C2 = (0,1,0).
      p0 = (0, 0, 1): seen by 0, 1, 2.  Rays to C0, C1: (0,0,-1), (1,0,-1): 45 degrees.  C0, C2: 45.  C1, C2: (1,0,-1), (0,1,-1): 60.
      p1 = (0.5, h, 0), h = 0.5 / tan(2.5 deg): seen by 0, 1.  The isosceles triangle C0 p1 C1 has the apex angle 2 * 2.5 = 5 = theta0:
           the term takes the sigma1 branch and is 1 up to rounding.
      p2 = (0, 0, 0) = C0: seen by 0, 2.  a = 0: atan2(0, 0) = 0 degrees, the term is exp(-25 / 2), not a NaN.
      p3 = (3, 3, 3): seen by nobody.
    S01 = g(45) + g(5), S02 = g(45) + g(0), S12 = g(60), with g(x) = exp(-(x-5)^2 / 200) above 5 and exp(-(x-5)^2 / 2) up to 5."""
    h = 0.5 / np.tan(np.radians(2.5))
    xyz = np.array([[0, 0, 1], [0.5, h, 0], [0, 0, 0], [3, 3, 3]], np.float32)
    R = np.stack([np.eye(3)] * 3).astype(np.float32)
    t = -np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    obs = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0), (2, 2)]
    g = lambda x: float(np.exp(-(x - 5.0) ** 2 / (200.0 if x > 5.0 else 2.0)))  # noqa: E731
    S = np.zeros((3, 3))
    S[0, 1] = S[1, 0] = g(45.0) + 1.0
    S[0, 2] = S[2, 0] = g(45.0) + g(0.0)
    S[1, 2] = S[2, 1] = g(60.0)
    return {"xyz": xyz, "obs_point": np.array([o[0] for o in obs], np.int64), "obs_view": np.array([o[1] for o in obs], np.int32),
            "R": R, "t": t, "S": S, "src": np.array([[1, 2], [0, 2], [0, 1]], np.int32),
            # depths: R = I, t_z = 0: z is the point's z.  view 0 sees z = (1, 0, 0), view 1 (1, 0), view 2 (1, 0)
            "range": np.array([[0, 1], [0, 1], [0, 1]], np.float32), "n": np.array([3, 2, 2])}
