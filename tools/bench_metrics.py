#!/usr/bin/env python
"""Depth metrics, two routes on the same maps (needs the GPU):

    python tools/bench_metrics.py [--views 20] [--repeats 5] [--out profiles/depth_metrics_bench.json]

* ``reference``: test.py:310-320's seven entries written as the reference writes them - a plain-torch restatement of ``utils.py:148-182``
  inside this tool (boolean-mask gathers per image, ``torch.stack(...).mean()``), ``depth_interval[0].item()``, one ``.item()`` per entry
  (``tensor2float``) and a Python-float meter;
* ``fused``: one ``mvsformer_amd.metrics.depth_metrics`` call per view (thresholds built on the device, meter advanced by the same call)
  and ONE ``mean()`` at the end.

At 1536x1152 and 640x512, B = 1 and B = 4: milliseconds per view (host clock around ``--views`` calls, synchronised at the end of each
route's turn), the routes alternating, every repeat kept; beside them the kernel launches of one view (torch.profiler, outside the timed
region) and the host synchronisations of one turn (counted ``.item()`` / ``.cpu()`` / ``.tolist()`` calls).
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvsformer_amd import metrics  # noqa: E402

MULT = metrics.TEST_MULTIPLIERS


def ref_thres(depth_est, depth_gt, mask, thres):
    res = []
    for i in range(depth_gt.shape[0]):
        e, g = depth_est[i][mask[i]], depth_gt[i][mask[i]]
        res.append(torch.mean((torch.abs(e - g) > thres).float()))
    return torch.stack(res).mean()


def ref_abs(depth_est, depth_gt, mask):
    res = []
    for i in range(depth_gt.shape[0]):
        e, g = depth_est[i][mask[i]], depth_gt[i][mask[i]]
        res.append(torch.mean((e - g).abs()))
    return torch.stack(res).mean()


def route_reference(views, interval):
    data, count = {}, 0
    for est, gt, mask in views:
        di = interval[0].item() / 2.65
        out = {"abs_depth_error": ref_abs(est, gt, mask > 0.5)}
        for m in MULT:
            out["thres%dmm_error" % m] = ref_thres(est, gt, mask > 0.5, di * m)
        out = {k: v.item() for k, v in out.items()}
        count += 1
        for k, v in out.items():
            data[k] = data.get(k, 0.0) + v
    return {k: v / count for k, v in data.items()}


def route_fused(views, interval):
    meter = metrics.DeviceAverageMeter([metrics.ABS_KEY] + metrics.threshold_names(MULT), views[0][0].device)
    for est, gt, mask in views:
        metrics.depth_metrics(est, gt, mask, depth_interval=interval, multipliers=MULT, meter=meter)
    return meter.mean()


class SyncCounter:
    """Counts the calls that make the host wait for the device."""
    names = ("item", "cpu", "tolist")

    def __enter__(self):
        self.n, self.saved = 0, {k: getattr(torch.Tensor, k) for k in self.names}
        for k, fn in self.saved.items():
            def wrapped(t, *a, _fn=fn, **kw):
                if t.is_cuda:
                    self.n += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(torch.Tensor, k, fn)


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if "cuda" in str(getattr(e, "device_type", "")).lower() and "mem" not in e.name.lower())
    except Exception as e:                                   # noqa: BLE001 - a profiler that does not load leaves the count unmeasured
        print("launch count unavailable: %s" % e, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "depth_metrics_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py runs the MI355X path: no GPU")
    dev = torch.device("cuda:0")
    interval = torch.tensor([2.5 * 1.06], device=dev)
    res = dict(device=torch.cuda.get_device_name(0), views_per_turn=a.views, multipliers=list(MULT), cases=[])
    for H, W in ((1152, 1536), (512, 640)):
        for B in (1, 4):
            g = torch.Generator(device=dev).manual_seed(H + B)
            views = []
            for _ in range(a.views):
                gt = 425.0 + 500.0 * torch.rand(B, H, W, device=dev, generator=g)
                est = gt + 6.0 * torch.randn(B, H, W, device=dev, generator=g)
                views.append((est, gt, (torch.rand(B, H, W, device=dev, generator=g) < 0.7).float()))
            itv = interval.expand(B).contiguous()
            routes = {"reference": route_reference, "fused": route_fused}
            means = {k: fn(views, itv) for k, fn in routes.items()}        # untimed pass; the two routes must agree
            worst = max(abs(means["reference"][k] - means["fused"][k]) / max(abs(means["reference"][k]), 1e-30) for k in means["fused"])
            case = dict(height=H, width=W, batch=B, largest_relative_difference=worst, ms_per_view={k: [] for k in routes}, launches_per_view={},
                        host_syncs_per_turn={})
            for k, fn in routes.items():
                case["launches_per_view"][k] = launches(lambda: fn(views[:1], itv))
                with SyncCounter() as sc:
                    fn(views, itv)
                case["host_syncs_per_turn"][k] = sc.n
            for _ in range(a.repeats):
                for k, fn in routes.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(views, itv)
                    torch.cuda.synchronize()
                    case["ms_per_view"][k].append(1e3 * (time.perf_counter() - t0) / a.views)
            res["cases"].append(case)
            print(json.dumps(case))
            del views
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
