#!/usr/bin/env python
"""Records tests/golden/depth_metrics.npz from the REAL reference ``utils.py`` on the CPU:

    python tools/gen_depth_metrics_golden.py /path/to/reference/checkout

For every case of tests/depth_metrics_util.py::FIXTURE_CASES: the inputs, ``Thres_metrics`` at every threshold of ``FIXTURE_THRES`` and
``AbsDepthError_metrics`` at every band of ``FIXTURE_BANDS`` (fp32, as the reference returns them), and a ``DictAverageMeter`` trace: the
validation set of entries (abs error + four thresholds) of every case whose results are finite, fed in case order through
``tensor2float`` as ``_valid_epoch`` feeds them - the meter's sums and count after every update and its final means.
``utils.py`` imports torchvision, yaml and omegaconf at its top; they are stubbed (nothing recorded here touches them).
"""
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import depth_metrics_util as du  # noqa: E402


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    if "." in name:
        setattr(sys.modules[name.rsplit(".", 1)[0]], name.rsplit(".", 1)[1], mod)
    return mod


def main(checkout):
    sys.path.insert(0, checkout)
    sys.dont_write_bytecode = True
    for name, kw in (("torchvision", {}), ("torchvision.utils", {}), ("yaml", {}), ("omegaconf", dict(OmegaConf=object))):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                _stub(name, **kw)
    import utils as ref
    arrs, meter = {}, ref.DictAverageMeter()
    trace_in, trace_data, trace_count, trace_cases = [], [], [], []
    keys = [du.ABS_KEY] + ["thres%dmm_error" % m for m in du.VALID_MULT]
    di = float(du.F32(du.DTU_INTERVAL)) / 2.65
    for name, kw in du.FIXTURE_CASES.items():
        est, gt, mask = du.make_case(**kw)
        e, g, m = torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mask)
        arrs[name + ".est"], arrs[name + ".gt"], arrs[name + ".mask"] = est, gt, mask.astype(np.uint8)
        arrs[name + ".thres"] = np.array([ref.Thres_metrics(e, g, m, t).item() for t in du.FIXTURE_THRES], dtype=np.float32)
        arrs[name + ".abs"] = np.array([(ref.AbsDepthError_metrics(e, g, m) if b is None else ref.AbsDepthError_metrics(e, g, m, b)).item()
                                        for b in du.FIXTURE_BANDS], dtype=np.float32)
        # per image too (the wrapper applied to a batch of one): what the per-image outputs are compared with
        arrs[name + ".thres_img"] = np.array([[ref.Thres_metrics(e[b:b + 1], g[b:b + 1], m[b:b + 1], t).item() for t in du.FIXTURE_THRES]
                                              for b in range(est.shape[0])], dtype=np.float32)
        arrs[name + ".abs_img"] = np.array([[(ref.AbsDepthError_metrics(e[b:b + 1], g[b:b + 1], m[b:b + 1]) if bd is None else
                                              ref.AbsDepthError_metrics(e[b:b + 1], g[b:b + 1], m[b:b + 1], bd)).item() for bd in du.FIXTURE_BANDS]
                                            for b in range(est.shape[0])], dtype=np.float32)
        scalars = {keys[0]: ref.AbsDepthError_metrics(e, g, m)}
        for k, mult in zip(keys[1:], du.VALID_MULT):
            scalars[k] = ref.Thres_metrics(e, g, m, di * mult)
        scalars = ref.tensor2float(scalars)
        print(name, arrs[name + ".abs"], arrs[name + ".thres"])
        if all(np.isfinite(v) for v in scalars.values()):
            meter.update(scalars)
            trace_cases.append(name)
            trace_in.append([scalars[k] for k in keys])
            trace_data.append([meter.data[k] for k in keys])
            trace_count.append(meter.count)
    mean = meter.mean()
    arrs.update(meter_keys=np.array(keys), meter_cases=np.array(trace_cases), meter_in=np.array(trace_in, dtype=np.float64),
                meter_data=np.array(trace_data, dtype=np.float64), meter_count=np.array(trace_count, dtype=np.float64),
                meter_mean=np.array([mean[k] for k in keys], dtype=np.float64))
    out = os.path.join(REPO, "tests", "golden", "depth_metrics.npz")
    np.savez_compressed(out, **arrs)
    print("wrote %s (%d bytes), meter over %s" % (out, os.path.getsize(out), trace_cases))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
