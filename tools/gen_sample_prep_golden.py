#!/usr/bin/env python
"""Writes tests/golden/sample_prep.npz with PIL: a 16x24 image, fixed factors, and PIL's output for the 24 orders of the four colour
operations (ImageEnhance.Brightness / Contrast / Color and the HSV hue shift, which is all torchvision's PIL branch does), plus single
operations at their extremes.  Data only; a machine without PIL checks tests/sample_prep_util.py against it."""
import itertools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import sample_prep_util as u  # noqa: E402


def main():
    rng = np.random.default_rng(2024)
    img = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    img[0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [1, 254, 128]]
    factors = np.array([0.8, 1.3, 0.7, 0.1])
    orders = np.array(list(itertools.permutations(range(4))), np.int64)
    out = np.stack([u.jitter_pil(img, o, tuple(factors)) for o in orders])
    singles = np.array([(0, 0.0), (0, 2.5), (1, 0.0), (1, 3.0), (2, 0.0), (2, 2.0), (3, -0.5), (3, 0.0), (3, 0.5)])
    single_out = []
    for op, v in singles:
        f = [1.0, 1.0, 1.0, 0.0]
        f[int(op)] = float(v)
        single_out.append(u.jitter_pil(img, [int(op)], tuple(f)))
    np.savez_compressed(os.path.join(REPO, "tests", "golden", "sample_prep.npz"), img=img, factors=factors, orders=orders, out=out,
                        singles=singles, single_out=np.stack(single_out))


if __name__ == "__main__":
    main()
