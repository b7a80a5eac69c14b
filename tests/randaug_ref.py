"""Pillow's uint8 arithmetic for the ops of the reference's RandAugment, restated in numpy per op from PIL's C and Python sources (Geometry.c, Blend.c, Filter.c,
Convert.c, ImageOps.py, ImageEnhance.py, Image.rotate), independently of devias_amd.randaug: the op is taken by the reference's NAME and its level argument, the frame is
one [H, W, 3] image at a time, tables are built as the Python lists ImageOps builds, and the bicubic rows outside the frame repeat the previous row's VALUE as
BICUBIC_BODY does (not a clamped index).  tests/golden/randaug_vectors.npz holds what Pillow itself returned; test_randaug_cpu.py holds this file and
devias_amd.randaug.randaug_cpu to it bitwise."""
import math

import numpy as np

FILL = np.array([128, 128, 128], dtype=np.uint8)
BILINEAR, BICUBIC = 2, 3


def to_l(im):
    r, g, b = (im[..., k].astype(np.int64) for k in range(3))
    return ((r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(im1, im2, alpha):
    alpha = np.float32(alpha)
    if alpha == 0:
        return im1.copy()
    if alpha == 1:
        return im2.copy()
    a, b = im1.astype(np.int32), im2.astype(np.int32)
    t = a.astype(np.float32) + alpha * (b - a).astype(np.float32)
    if 0 <= alpha <= 1:
        return t.astype(np.uint8)
    out = np.zeros(t.shape, dtype=np.uint8)
    mid = (t > 0) & (t < 255)
    out[mid] = t[mid].astype(np.uint8)
    out[t >= 255] = 255
    return out


def smooth(im):
    H, W, _ = im.shape
    out = im.copy()
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)).reshape(3, 3)
    if H < 3 or W < 3:
        return out                                       # nothing but border
    p = im.astype(np.float32)
    ss = np.full((H - 2, W - 2, 3), 0.5, dtype=np.float32)
    for ky, dy in enumerate((2, 1, 0)):                  # KERNEL1x3 on the rows y + 1, y, y - 1 of inner pixel (y, x)
        row = p[dy:dy + H - 2]
        ss = ss + ((row[:, 0:W - 2] * k[ky, 0] + row[:, 1:W - 1] * k[ky, 1]) + row[:, 2:W] * k[ky, 2])
    out[1:H - 1, 1:W - 1] = np.clip(ss.astype(np.int64), 0, 255).astype(np.uint8)
    return out


def _poly(v1, v2, v3, v4, d):
    return v2 + d * ((-v1 + v3) + d * ((2 * (v1 - v2) + v3 - v4) + d * (-v1 + v2 - v3 + v4)))


def transform_affine(im, a, resample):
    H, W, _ = im.shape
    out = np.empty_like(im)
    out[...] = FILL
    src = im.astype(np.float64)
    for yo in range(H):
        xs, ys = np.arange(W) + 0.5, yo + 0.5
        xin = a[0] * xs + a[1] * ys + a[2]
        yin = a[3] * xs + a[4] * ys + a[5]
        xo = np.nonzero((xin >= 0) & (xin < W) & (yin >= 0) & (yin < H))[0]            # the output pixels of this row whose source lies inside
        if not len(xo):
            continue
        xi, yi = xin[xo] - 0.5, yin[xo] - 0.5
        x, y = np.floor(xi).astype(np.int64), np.floor(yi).astype(np.int64)
        dx, dy = (xi - x)[:, None], (yi - y)[:, None]
        yclip = lambda r: np.clip(r, 0, H - 1)                                         # noqa: E731
        if resample == BICUBIC:
            cols = [np.clip(x - 1 + k, 0, W - 1) for k in range(4)]
            v = [_poly(*(src[yclip(y - 1), c] for c in cols), dx)]
            for k in (1, 2, 3):                                                        # a row outside the frame: the previous row's value
                inside = ((y - 1 + k >= 0) & (y - 1 + k < H))[:, None]
                v.append(np.where(inside, _poly(*(src[yclip(y - 1 + k), c] for c in cols), dx), v[k - 1]))
            r = _poly(v[0], v[1], v[2], v[3], dy)
        else:
            x0, x1 = np.clip(x, 0, W - 1), np.clip(x + 1, 0, W - 1)
            v1 = src[yclip(y), x0] + (src[yclip(y), x1] - src[yclip(y), x0]) * dx
            inside = ((y + 1 >= 0) & (y + 1 < H))[:, None]
            v2 = np.where(inside, src[yclip(y + 1), x0] + (src[yclip(y + 1), x1] - src[yclip(y + 1), x0]) * dx, v1)
            r = v1 + (v2 - v1) * dy
        out[yo, xo] = np.where(r <= 0, 0, np.where(r >= 255, 255, r)).astype(np.uint8)
    return out


def rotate(im, degrees, resample):
    H, W, _ = im.shape
    angle = degrees % 360.0
    if angle == 0:
        return im.copy()
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return transform_affine(im, m, resample)


def point(im, luts):
    return np.stack([np.asarray(luts[c], dtype=np.int64).clip(0, 255).astype(np.uint8)[im[..., c]] for c in range(3)], axis=-1)


def autocontrast(im):
    luts = []
    for c in range(3):
        h = np.bincount(im[..., c].ravel(), minlength=256).tolist()
        lo = next(i for i in range(256) if h[i])
        hi = next(i for i in range(255, -1, -1) if h[i])
        if hi <= lo:
            luts.append(list(range(256)))
        else:
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            luts.append([min(255, max(0, int(ix * scale + offset))) for ix in range(256)])
    return point(im, luts)


def equalize(im):
    luts = []
    for c in range(3):
        h = np.bincount(im[..., c].ravel(), minlength=256).tolist()
        histo = [f for f in h if f]
        step = (sum(histo) - histo[-1]) // 255 if len(histo) > 1 else 0
        if not step:
            luts.append(list(range(256)))
        else:
            lut, n = [], step // 2
            for i in range(256):
                lut.append(n // step)
                n = n + h[i]
            luts.append(lut)
    return point(im, luts)


def apply(name, im, arg, resample=BICUBIC):
    """the reference's NAME_TO_OP[name](img, *level_args) on one uint8 [H, W, 3] image"""
    H, W, _ = im.shape
    base = name[:-10] if name.endswith("Increasing") else name
    if name == "AutoContrast":
        return autocontrast(im)
    if name == "Equalize":
        return equalize(im)
    if name == "Invert":
        return point(im, [list(range(255, -1, -1))] * 3)
    if name == "Rotate":
        return rotate(im, arg, resample)
    if name == "ShearX":
        return transform_affine(im, (1, arg, 0, 0, 1, 0), resample)
    if name == "ShearY":
        return transform_affine(im, (1, 0, 0, arg, 1, 0), resample)
    if name == "TranslateXRel":
        return transform_affine(im, (1, 0, arg * W, 0, 1, 0), resample)
    if name == "TranslateYRel":
        return transform_affine(im, (1, 0, 0, 0, 1, arg * H), resample)
    if base == "Posterize":
        bits = int(arg)
        return im.copy() if bits >= 8 else point(im, [[i & ~(2 ** (8 - bits) - 1) for i in range(256)]] * 3)
    if base == "Solarize":
        return point(im, [[i if i < int(arg) else 255 - i for i in range(256)]] * 3)
    if name == "SolarizeAdd":
        return point(im, [[min(255, i + int(arg)) if i < 128 else i for i in range(256)]] * 3)
    if base == "Color":
        return blend(np.repeat(to_l(im)[..., None], 3, axis=-1), im, arg)
    if base == "Contrast":
        l = to_l(im)
        mean = int(float(np.bincount(l.ravel(), minlength=256) @ np.arange(256)) / l.size + 0.5)
        return blend(np.full_like(im, mean), im, arg)
    if base == "Brightness":
        return blend(np.zeros_like(im), im, arg)
    if base == "Sharpness":
        return blend(smooth(im), im, arg)
    raise ValueError(name)


def randaug_ref(frames, layers, resample=BICUBIC):
    """uint8 [T, H, W, 3] through the applied layers (name, applied, arg or None)"""
    out = []
    for im in frames:
        for name, applied, arg in layers:
            if applied:
                im = apply(name, im, arg, resample)
        out.append(im)
    return np.stack(out)
