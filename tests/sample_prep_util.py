"""numpy restatements of the sample-preparation arithmetic, the yardsticks of tests/test_sample_prep_refs.py and test_hip_sample_prep.py.

Colour steps: PIL itself is the oracle.  ``brightness`` / ``contrast`` / ``saturation`` / ``hue`` restate, operation for operation in
PIL's C float arithmetic, what ``ImageEnhance.Brightness / Contrast / Color(img).enhance(f)`` and ``convert('HSV')`` / ``convert('RGB')``
compute; that is all torchvision's PIL branch of ``adjust_brightness / contrast / saturation / hue`` does, and torchvision itself is not
needed.  test_sample_prep_refs.py pins them to PIL bit for bit, and tests/golden/sample_prep.npz carries PIL's outputs for a machine
without PIL.

Resizes: OpenCV's INTER_AREA, INTER_NEAREST and 8-bit INTER_LINEAR restated from their definition; parity with an installed cv2 is
not verified (only where cv2 imports).  ``area_resize_f64`` / ``linear_resize_f64`` evaluate the same weights in fp64 without rounding.
"""
import math

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


# ------------------------------------------------------------------------------------------------------------------ PIL colour steps
def _blend(d, s, alpha):
    """Image.blend(degenerate, image, alpha) on int arrays (ImagingBlend)."""
    a = np.float32(alpha)
    t = d.astype(np.float32) + a * (s.astype(np.int32) - d.astype(np.int32)).astype(np.float32)
    if 0.0 <= alpha <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def luma(img):
    i = img.astype(np.int64)
    return ((i[..., 0] * 19595 + i[..., 1] * 38470 + i[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def brightness(img, f):
    return _blend(np.zeros_like(img), img, f)


def contrast_mean(img):
    """int(ImageStat.Stat(img.convert('L')).mean[0] + 0.5)"""
    l = luma(img)
    return int(int(l.astype(np.int64).sum()) / l.size + 0.5)


def contrast(img, f):
    return _blend(np.full_like(img, contrast_mean(img)), img, f)


def saturation(img, f):
    return _blend(np.repeat(luma(img)[..., None], 3, axis=-1), img, f)


def hue_shift(hue_factor):
    """np.uint8(hue_factor * 255) as torchvision forms it: truncation toward zero, then modulo 256."""
    return int(hue_factor * 255) & 0xFF


def hue(img, hue_factor):
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(np.float32)
        s = cr / maxc.astype(np.float32)
        rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))
        h = np.where(r == maxc, bc - gc,
                     np.where(g == maxc, (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32),
                              (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)))
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
        uh = np.clip(np.nan_to_num(h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        us = np.clip(np.nan_to_num(s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    uh, us, uv = np.where(grey, 0, uh), np.where(grey, 0, us), maxc
    uh = (uh + hue_shift(hue_factor)) & 0xFF
    h6 = uh.astype(np.float32).astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = (h6 - i.astype(np.float32).astype(np.float64)).astype(np.float32).astype(np.float64)
    fs = (us.astype(np.float32).astype(np.float64) / 255.0).astype(np.float32).astype(np.float64)
    v = uv.astype(np.float64)

    def rnd(x):                                                   # C round(): halves away from zero (x >= 0 here)
        return np.clip(np.floor(x + 0.5).astype(np.int64), 0, 255)
    p, q, t = rnd(v * (1.0 - fs)), rnd(v * (1.0 - fs * f)), rnd(v * (1.0 - fs * (1.0 - f)))
    k = i % 6
    out = np.empty(img.shape, np.uint8)
    for c, sel in enumerate(((uv, q, p, p, t, uv), (t, uv, uv, q, p, p), (p, p, t, uv, uv, q))):
        ch = np.choose(k, sel)
        out[..., c] = np.where(us == 0, uv, ch)
    return out


def jitter(img, fn_idx, factors, enabled=(True, True, True, True)):
    """color_jittor.py:53-83 on one HxWx3 uint8 image; ``factors`` = (brightness, contrast, saturation, hue)."""
    ops = (brightness, contrast, saturation, hue)
    for k in fn_idx:
        if enabled[int(k)]:
            img = ops[int(k)](img, factors[int(k)])
    return img


def jitter_pil(img, fn_idx, factors, enabled=(True, True, True, True)):
    """The same through PIL (what torchvision's functional_pil does)."""
    from PIL import Image, ImageEnhance
    im = Image.fromarray(img)
    for k in fn_idx:
        k = int(k)
        if not enabled[k]:
            continue
        if k == 0:
            im = ImageEnhance.Brightness(im).enhance(factors[0])
        elif k == 1:
            im = ImageEnhance.Contrast(im).enhance(factors[1])
        elif k == 2:
            im = ImageEnhance.Color(im).enhance(factors[2])
        else:
            h, s, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(all="ignore"):                       # torchvision's own lines: numpy's uint8 cast and wrap-around addition
                np_h += np.array(factors[3] * 255).astype(np.uint8)
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return np.array(im)


def tail(img_u8, gamma=None):
    """ToTensor, RandomGamma(clip_image=True), Normalize: HxWx3 uint8 -> 3xHxW fp32, every step in fp32 (gamma through torch.pow)."""
    x = img_u8.astype(np.float32) / np.float32(255.0)
    if gamma is not None:
        import torch
        x = torch.pow(torch.from_numpy(x), float(gamma)).clamp_(0.0, 1.0).numpy()
    return np.ascontiguousarray(((x - MEAN) / STD).transpose(2, 0, 1))


def tail_f64(img_u8, gamma):
    x = img_u8.astype(np.float64) / 255.0
    x = np.clip(np.power(x, float(np.float32(gamma))), 0.0, 1.0)
    return ((x - MEAN.astype(np.float64)) / STD.astype(np.float64)).transpose(2, 0, 1)


# ------------------------------------------------------------------------------------------------------------------ resizes
def nn_index(dst, src):
    """cv2.INTER_NEAREST source indices of a dst-long axis over a src-long one."""
    d = np.arange(dst, dtype=np.float64)
    return np.minimum(np.floor(d * (float(src) / float(dst))).astype(np.int64), src - 1)


def nearest_resize(a, dst_h, dst_w):
    return a[nn_index(dst_h, a.shape[0])][:, nn_index(dst_w, a.shape[1])]


def area_tab(ssize, dsize):
    """OpenCV's computeResizeAreaTab: per destination index a list of (source index, weight in double)."""
    scale = float(ssize) / float(dsize)
    tab = []
    for d in range(dsize):
        fsx1 = d * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = math.ceil(fsx1), math.floor(fsx2)
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        taps = []
        if sx1 - fsx1 > 1e-3:
            taps.append((sx1 - 1, (sx1 - fsx1) / cell))
        for sx in range(sx1, sx2):
            taps.append((sx, 1.0 / cell))
        if fsx2 - sx2 > 1e-3:
            taps.append((sx2, min(min(fsx2 - sx2, 1.0), cell) / cell))
        tab.append(taps)
    return tab


def _area(img, dst_h, dst_w, ft):
    H0, W0 = img.shape[:2]
    xt, yt = area_tab(W0, dst_w), area_tab(H0, dst_h)
    src = img.astype(ft)
    hor = np.zeros((H0, dst_w, img.shape[2]), ft)
    for d, taps in enumerate(xt):
        for sx, wgt in taps:
            hor[:, d] = hor[:, d] + src[:, sx] * ft(np.float32(wgt) if ft is np.float32 else wgt)
    out = np.zeros((dst_h, dst_w, img.shape[2]), ft)
    for d, taps in enumerate(yt):
        for sy, wgt in taps:
            out[d] = out[d] + ft(np.float32(wgt) if ft is np.float32 else wgt) * hor[sy]
    return out


def area_resize_f64(img, dst_h, dst_w):
    """The same weights evaluated in fp64, not rounded."""
    return _area(img, dst_h, dst_w, np.float64)


def area_resize(img, dst_h, dst_w):
    """cv2.resize(img, (dst_w, dst_h), interpolation=cv2.INTER_AREA) of an HxWx3 uint8 image."""
    H0, W0 = img.shape[:2]
    if (dst_h, dst_w) == (H0, W0):
        return img.copy()
    if H0 == 2 * dst_h and W0 == 2 * dst_w:
        i = img.astype(np.int32)
        return ((i[0::2, 0::2] + i[0::2, 1::2] + i[1::2, 0::2] + i[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    return np.clip(np.rint(_area(img, dst_h, dst_w, np.float32)), 0, 255).astype(np.uint8)


def _linear_coef(dsize, ssize):
    scale = float(ssize) / float(dsize)
    fx = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(np.float32)
    fx = np.where((sx < 0) | (sx >= ssize - 1), np.float32(0), fx).astype(np.float32)
    sx = np.clip(sx, 0, ssize - 1)
    return sx, fx


def linear_resize(img, dst_h, dst_w, pad_rows=0):
    """cv2.resize(img, (dst_w, dst_h)) (INTER_LINEAR, 8-bit fixed point) of np.pad(img, pad_rows rows, 'edge')."""
    if pad_rows:
        img = np.pad(img, ((pad_rows, pad_rows), (0, 0), (0, 0)), "edge")
    H0, W0 = img.shape[:2]
    if H0 == 2 * dst_h and W0 == 2 * dst_w:
        return area_resize(img, dst_h, dst_w)
    sx, fx = _linear_coef(dst_w, W0)
    sy, fy = _linear_coef(dst_h, H0)
    a0, a1 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64), np.rint(fx * np.float32(2048)).astype(np.int64)
    b0, b1 = np.rint((np.float32(1) - fy) * np.float32(2048)).astype(np.int64), np.rint(fy * np.float32(2048)).astype(np.int64)
    i = img.astype(np.int64)
    hor = i[:, sx] * a0[None, :, None] + i[:, np.minimum(sx + 1, W0 - 1)] * a1[None, :, None]
    r0, r1 = hor[sy], hor[np.minimum(sy + 1, H0 - 1)]
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def linear_resize_f64(img, dst_h, dst_w, pad_rows=0):
    if pad_rows:
        img = np.pad(img, ((pad_rows, pad_rows), (0, 0), (0, 0)), "edge")
    H0, W0 = img.shape[:2]
    if H0 == 2 * dst_h and W0 == 2 * dst_w:
        return area_resize_f64(img, dst_h, dst_w)

    def coef(dsize, ssize):
        f = np.clip((np.arange(dsize, dtype=np.float64) + 0.5) * (float(ssize) / dsize) - 0.5, 0, ssize - 1)
        s = np.minimum(np.floor(f).astype(np.int64), ssize - 1)
        return s, f - s
    sx, fx = coef(dst_w, W0)
    sy, fy = coef(dst_h, H0)
    i = img.astype(np.float64)
    hor = i[:, sx] * (1 - fx)[None, :, None] + i[:, np.minimum(sx + 1, W0 - 1)] * fx[None, :, None]
    return hor[sy] * (1 - fy)[:, None, None] + hor[np.minimum(sy + 1, H0 - 1)] * fy[:, None, None]


# ------------------------------------------------------------------------------------------------------------------ geometry
def stage_pyramid(a):
    """generate_stage_depth"""
    h, w = a.shape
    return {"stage1": nearest_resize(a, h // 8, w // 8), "stage2": nearest_resize(a, h // 4, w // 4),
            "stage3": nearest_resize(a, h // 2, w // 2), "stage4": a}


def resized_size(H0, W0, resize_scale):
    return int(H0 * resize_scale), int(W0 * resize_scale)


def accept(mask_raw, resize_scale, cands, crop_h, crop_w, require_positive=True):
    """The retry loop over given candidates: -> (offset_y, offset_x, accepted, index)."""
    m = (mask_raw.astype(np.float32) > 10).astype(np.float32)
    if resize_scale != 1.0:
        m = nearest_resize(m, *resized_size(*m.shape, resize_scale))
    for k, (oy, ox) in enumerate(cands):
        s1 = stage_pyramid(m[oy:oy + crop_h, ox:ox + crop_w])["stage1"]
        if not require_positive or np.any(s1 > 0.0):
            return int(oy), int(ox), 1, k
    return int(cands[-1][0]), int(cands[-1][1]), 0, len(cands) - 1


def crop_maps(depth_hr, mask_raw, resize_scale, oy, ox, crop_h, crop_w):
    m = (mask_raw.astype(np.float32) > 10).astype(np.float32)
    d = depth_hr
    if resize_scale != 1.0:
        rh, rw = resized_size(*m.shape, resize_scale)
        m, d = nearest_resize(m, rh, rw), nearest_resize(d, rh, rw)
    return stage_pyramid(d[oy:oy + crop_h, ox:ox + crop_w]), stage_pyramid(m[oy:oy + crop_h, ox:ox + crop_w])


def proj_matrices(intr, extr, resize_scales, offsets):
    """intr [V,3,3], extr [V,4,4] fp32, per view resize_scale and (offset_y, offset_x) -> {stage: [V,2,4,4]} as __getitem__ builds them."""
    mats = []
    for v in range(intr.shape[0]):
        k = intr[v].astype(np.float32).copy()
        if resize_scales[v] != 1.0:
            k[0, :] *= np.float32(resize_scales[v])
            k[1, :] *= np.float32(resize_scales[v])
        k[0, 2] -= np.float32(offsets[v][1])
        k[1, 2] -= np.float32(offsets[v][0])
        pm = np.zeros((2, 4, 4), np.float32)
        pm[0] = extr[v]
        pm[1, :3, :3] = k
        mats.append(pm)
    pm = np.stack(mats)
    out = {"stage4": pm}
    for name, f in (("stage1", 0.125), ("stage2", 0.25), ("stage3", 0.5)):
        c = pm.copy()
        c[:, 1, :2, :] = pm[:, 1, :2, :] * np.float32(f)
        out[name] = c
    return out


def depth_values(depth_min, depth_interval, ndepths):
    """np.arange(depth_min, depth_interval * ndepths + depth_min, depth_interval, dtype=float32), restated: length by arange's rule, the
    first two elements from double, the rest by numpy's fp32 fill loop."""
    stop = depth_interval * ndepths + depth_min
    n = int(math.ceil((stop - depth_min) / depth_interval))
    f0, f1 = np.float32(depth_min), np.float32(depth_min + depth_interval)
    out = np.empty(n, np.float32)
    out[0] = f0
    if n > 1:
        out[1] = f1
    delta = np.float32(f1 - f0)
    for i in range(2, n):
        out[i] = f0 + np.float32(i) * delta
    return out
