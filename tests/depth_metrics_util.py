"""Helpers of the depth-metrics tests: a numpy restatement of the reference's ``Thres_metrics`` / ``AbsDepthError_metrics`` (utils.py:148-182;
the error |est - gt| in fp32 as the reference forms it, everything after it in fp64 with exact integer counts), of ``DictAverageMeter``
(utils.py:119-145, Python floats), and the builder of the cases that tests/golden/depth_metrics.npz was recorded on
(tools/gen_depth_metrics_golden.py runs the REAL utils.py on them)."""
import numpy as np

F32 = np.float32
ABS_KEY = "abs_depth_error"
# 2.5 mm x interval_scale 1.06: not exact in fp32, the DTU interval of every shipped config
DTU_INTERVAL = float(F32(2.5) * F32(1.06))
VALID_MULT = (2, 4, 8, 14)
TEST_MULT = (1, 2, 4, 8, 14, 20)


def make_case(B, H, W, seed, mask="half", poison=False, nan_valid=None, integer=False, offset=0.0):
    """-> ``est, gt`` fp32 ``[B,H,W]`` and a bool ``mask``.  ``mask``: 'all', 'half' (random, about half), 'last' (exactly one valid pixel per
    image: the last one), 'none1' (like 'half', but image ``min(1, B-1)`` has none).  ``poison``: NaN and +-Inf in est and gt at invalid pixels.
    ``nan_valid = (b, flat index)``: a NaN in est at that pixel, which is made valid.  ``integer``: integer-valued gt, est = gt + ``offset`` on
    the first half of every map and gt elsewhere."""
    rng = np.random.RandomState(seed)
    gt = (425.0 + 500.0 * rng.rand(B, H, W)).astype(F32)
    est = (gt + 10.0 * rng.randn(B, H, W).astype(F32) * rng.rand(B, H, W).astype(F32) ** 2).astype(F32)
    if integer:
        gt = np.floor(gt).astype(F32)
        est = gt.copy()
        est.reshape(B, -1)[:, :(H * W + 1) // 2] += F32(offset)
    if mask == "all":
        m = np.ones((B, H, W), dtype=bool)
    elif mask == "last":
        m = np.zeros((B, H, W), dtype=bool)
        m.reshape(B, -1)[:, -1] = True
    else:
        m = rng.rand(B, H, W) < 0.5
        if mask == "none1":
            m[min(1, B - 1)] = False
    if poison:
        inv = np.argwhere(~m)
        for j, (b, y, x) in enumerate(inv[::3]):
            (est if j % 2 else gt)[b, y, x] = (np.nan, np.inf, -np.inf)[j % 3]
    if nan_valid is not None:
        b, i = nan_valid
        est.reshape(B, -1)[b, i] = np.nan
        m.reshape(B, -1)[b, i] = True
    return est, gt, m


def np_metrics(est, gt, mask, thr=None, band=None):
    """fp64 restatement.  ``thr``: ``[B,K]`` (or ``[K]``) fp32 thresholds.  -> dict: ``n [B]``, ``n_band [B]``, ``above [B,K]`` (exact ints),
    ``per_image [B,1+K]`` and ``batch [1+K]`` (fp64; NaN for an image with no valid pixel, 0 for an empty band)."""
    est, gt = np.asarray(est, dtype=F32), np.asarray(gt, dtype=F32)
    B = est.shape[0]
    valid = np.asarray(mask).reshape(B, -1)
    valid = valid > 0.5 if valid.dtype != bool else valid
    thr = np.zeros((B, 0), F32) if thr is None else np.broadcast_to(np.asarray(thr, dtype=F32), (B, np.asarray(thr).shape[-1]))
    K = thr.shape[1]
    n, nb, above, per = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros((B, K), np.int64), np.zeros((B, 1 + K))
    with np.errstate(all="ignore"):
        for b in range(B):
            e = np.abs(est[b].reshape(-1)[valid[b]] - gt[b].reshape(-1)[valid[b]])        # fp32 - fp32, abs: fp32
            assert e.dtype == F32
            n[b] = e.size
            sel = e if band is None else e[(e >= F32(band[0])) & (e <= F32(band[1]))]
            nb[b] = sel.size
            if band is not None and sel.size == 0:
                per[b, 0] = 0.0
            else:
                per[b, 0] = np.sum(sel.astype(np.float64)) / sel.size if sel.size else np.nan
            for k in range(K):
                above[b, k] = int(np.count_nonzero(e > thr[b, k]))                        # fp32 against fp32; NaN > t is False
                per[b, 1 + k] = above[b, k] / n[b] if n[b] else np.nan
        batch = per.mean(axis=0)                              # a NaN image makes its column's mean NaN
    return dict(n=n, n_band=nb, above=above, per_image=per, batch=batch)


def thresholds_host(interval, multipliers, per_sample=False):
    """The reference's host arithmetic: ``float32(mult * (float(interval[0]) / 2.65))`` or ``float32(mult * float(interval[j]))`` -> ``[B,K]``."""
    interval = np.asarray(interval, dtype=F32)
    rows = []
    for j in range(interval.size):
        di = float(interval[j]) if per_sample else float(interval[0]) / 2.65
        rows.append([F32(di * m) for m in multipliers])
    return np.array(rows, dtype=F32)


class MeterRef:
    """utils.py:119-145 in Python floats."""

    def __init__(self):
        self.data, self.count = {}, 0

    def update(self, new_input, n=1.0):
        self.count += n
        for k, v in new_input.items():
            assert isinstance(v, float)
            self.data[k] = self.data[k] + v if k in self.data else v

    def mean(self):
        return {k: v / self.count for k, v in self.data.items()}


def ulps32(got, want64):
    """|got - want| in units of the fp32 spacing at ``want`` (both NaN: 0; one NaN: inf)."""
    got, want64 = np.asarray(got, dtype=np.float64), np.asarray(want64, dtype=np.float64)
    with np.errstate(all="ignore"):
        sp = np.spacing(np.abs(want64).astype(F32)).astype(np.float64)
        u = np.abs(got - want64) / sp
    both = np.isnan(got) & np.isnan(want64)
    one = np.isnan(got) ^ np.isnan(want64)
    return np.where(both, 0.0, np.where(one, np.inf, u))


# The cases of tests/golden/depth_metrics.npz: name -> make_case arguments.  Thresholds: the DTU set of test.py on DTU_INTERVAL and two
# plain Python numbers; bands: none, one that holds something, one that holds nothing.
FIXTURE_CASES = {
    "b1_5x51_half": dict(B=1, H=5, W=51, seed=1, mask="half"),
    "b3_5x51_all": dict(B=3, H=5, W=51, seed=2, mask="all"),
    "b3_37x113_half": dict(B=3, H=37, W=113, seed=3, mask="half"),
    "b3_1x257_last": dict(B=3, H=1, W=257, seed=4, mask="last"),
    "b3_5x51_none1": dict(B=3, H=5, W=51, seed=5, mask="none1"),
    "b1_3x85_none": dict(B=1, H=3, W=85, seed=6, mask="none1"),
    "b3_4x64_poison": dict(B=3, H=4, W=64, seed=7, mask="half", poison=True),
    "b3_1x65_nanvalid": dict(B=3, H=1, W=65, seed=8, mask="half", nan_valid=(1, 17)),
}
FIXTURE_THRES = [float(F32(DTU_INTERVAL)) / 2.65 * m for m in TEST_MULT] + [0.1, 2]
FIXTURE_BANDS = [None, (0.5, 4.0), (1e6, 2e6)]
