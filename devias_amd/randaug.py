"""RandAugment on the device: the reference's `--aa rand-m7-n4-mstd0.5-inc1 --train_interpolation bicubic` (dataset/kinetics.py:_aug_frame ->
video_transforms.create_random_augment -> utils/transform/rand_augment.py; the same lines in ssv2.py, hvu.py, activitynet.py, hat_decode.py) on uint8 clips, bit for bit
what PIL computes: integer tables, fp32 blends, fp64 bicubic / bilinear taps, truncating conversions.

The draws are the reference's, on the host, from numpy's global state and Python's `random` in the reference's order and amount (RandAugment.draw); the arguments reach
the device as kernel arguments, turned into the values PIL hands to C with PIL's own Python arithmetic (lower).  One launch (devias_randaug_apply) applies one layer to
every clip of the batch whose layer was applied and is no identity; a layer with AutoContrast, Equalize or Contrast in it is preceded by one launch of
devias_randaug_stats.  Point ops work in place; the affine ops and Sharpness write to the other half of a double-sized buffer and the clip's offset flips.

Out of scope: interpolation="random" (a per-frame random.choice) and the `w` section (weighted choice without replacement): NotImplementedError; AugMix and
AutoAugment policies."""
from __future__ import annotations

import math
import random
import re
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MAX_LEVEL = 10.0
FILL = (128, 128, 128)
RAND_TRANSFORMS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness", "Sharpness", "ShearX",
                   "ShearY", "TranslateXRel", "TranslateYRel")
RAND_INCREASING_TRANSFORMS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd", "ColorIncreasing",
                              "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
# DEVIAS_RA_* (include/devias_amd.h)
OP_NONE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_COLOR, OP_CONTRAST, OP_BRIGHTNESS, OP_SHARPNESS, OP_AFFINE = range(12)
BILINEAR, BICUBIC = 2, 3                       # PIL's resampling codes, as the affine row carries them
NEIGHBOURHOOD = (OP_SHARPNESS, OP_AFFINE)      # ops that read other pixels than the one they write: out of place
NEEDS_STATS = (OP_AUTOCONTRAST, OP_EQUALIZE, OP_CONTRAST)
Layer = Tuple[str, bool, tuple]                # op name, applied, the level_fn's arguments
Lowered = Tuple[int, Tuple[float, ...], float, int, int]      # op code, six doubles, one float, two integers

_SIGNED = {"Rotate": 30.0, "ShearX": 0.3, "ShearY": 0.3, "TranslateXRel": 0.45, "TranslateYRel": 0.45}
_ENHANCE = {"Color": OP_COLOR, "Contrast": OP_CONTRAST, "Brightness": OP_BRIGHTNESS, "Sharpness": OP_SHARPNESS}


def parse_config(config_str: str):
    """rand_augment_transform's reading of the string: (magnitude, num_layers, weight_idx, magnitude_std, increasing).  As there, a section without a digit is skipped,
    an unknown key is ignored, and `inc` selects the increasing set whenever it carries a value: bool() of a non-empty string, so "inc0" selects it too."""
    magnitude, num_layers, weight_idx, mstd, increasing = MAX_LEVEL, 2, None, None, False
    config = config_str.split("-")
    if config[0] != "rand":
        raise ValueError(f"RandAugment: the config string starts with 'rand', got {config_str!r}")
    for c in config[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        if key == "mstd":
            if mstd is None:                   # hparams.setdefault: the first one holds
                mstd = float(val)
        elif key == "inc":
            increasing = increasing or bool(val)
        elif key == "m":
            magnitude = int(val)
        elif key == "n":
            num_layers = int(val)
        elif key == "w":
            weight_idx = int(val)
    return magnitude, num_layers, weight_idx, mstd, increasing


def _randomly_negate(v):
    return -v if random.random() > 0.5 else v


def level_args(name: str, level: float, hparams: dict) -> tuple:
    """LEVEL_TO_ARG[name](level, hparams): the signed ops draw one random.random()"""
    if name in ("AutoContrast", "Equalize", "Invert"):
        return ()
    if name in _SIGNED:
        if name.startswith("Translate"):
            return (_randomly_negate((level / MAX_LEVEL) * hparams.get("translate_pct", 0.45)),)
        return (_randomly_negate((level / MAX_LEVEL) * _SIGNED[name]),)
    if name == "Posterize":
        return (int((level / MAX_LEVEL) * 4),)
    if name == "PosterizeIncreasing":
        return (4 - int((level / MAX_LEVEL) * 4),)
    if name == "Solarize":
        return (int((level / MAX_LEVEL) * 256),)
    if name == "SolarizeIncreasing":
        return (256 - int((level / MAX_LEVEL) * 256),)
    if name == "SolarizeAdd":
        return (int((level / MAX_LEVEL) * 110),)
    if name in _ENHANCE:
        return ((level / MAX_LEVEL) * 1.8 + 0.1,)
    if name.endswith("Increasing") and name[:-10] in _ENHANCE:
        return (1.0 + _randomly_negate((level / MAX_LEVEL) * 0.9),)
    raise ValueError(f"RandAugment: unknown op {name!r}")


def rotation_matrix(degrees: float, W: int, H: int) -> Optional[Tuple[float, ...]]:
    """Image.rotate's matrix about the centre (w / 2, h / 2), in its Python arithmetic; None where it returns a copy (angle % 360 == 0)"""
    angle = degrees % 360.0
    if angle == 0:
        return None
    if angle in (90, 180, 270):
        raise NotImplementedError("RandAugment: Image.rotate serves right angles by a transpose; the recipe's angles stay within 30 degrees")
    cx, cy = W / 2.0, H / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def lower(name: str, args: tuple, H: int, W: int, resample: int = BICUBIC) -> Lowered:
    """the values PIL hands to C for op `name` with the level_fn's `args` on an H x W frame: (op code, six doubles, one float, two integers).  OP_NONE for the
    identities the reference returns the image for: a rotation by 0, an enhance factor of 1.0 (Image.blend returns its second image), a posterize that keeps 8 bits."""
    z = (0.0,) * 6
    if name == "AutoContrast":
        return OP_AUTOCONTRAST, z, 0.0, 0, 0
    if name == "Equalize":
        return OP_EQUALIZE, z, 0.0, 0, 0
    if name == "Invert":
        return OP_INVERT, z, 0.0, 0, 0
    if name == "Rotate":
        m = rotation_matrix(args[0], W, H)
        return (OP_NONE, z, 0.0, 0, 0) if m is None else (OP_AFFINE, m, 0.0, resample, 0)
    if name == "ShearX":
        return OP_AFFINE, (1.0, float(args[0]), 0.0, 0.0, 1.0, 0.0), 0.0, resample, 0
    if name == "ShearY":
        return OP_AFFINE, (1.0, 0.0, 0.0, float(args[0]), 1.0, 0.0), 0.0, resample, 0
    if name == "TranslateXRel":
        return OP_AFFINE, (1.0, 0.0, float(args[0] * W), 0.0, 1.0, 0.0), 0.0, resample, 0
    if name == "TranslateYRel":
        return OP_AFFINE, (1.0, 0.0, 0.0, 0.0, 1.0, float(args[0] * H)), 0.0, resample, 0
    if name.startswith("Posterize"):
        bits = int(args[0])
        return (OP_NONE, z, 0.0, 0, 0) if bits >= 8 else (OP_POSTERIZE, z, 0.0, ~(2 ** (8 - bits) - 1) & 0xff, 0)
    if name in ("Solarize", "SolarizeIncreasing"):
        return OP_SOLARIZE, z, 0.0, int(args[0]), 0
    if name == "SolarizeAdd":
        return OP_SOLARIZE_ADD, z, 0.0, int(args[0]), 128
    base = name[:-10] if name.endswith("Increasing") else name
    if base in _ENHANCE:
        f = float(np.float32(args[0]))         # Image.blend takes the factor as a C float
        return (OP_NONE, z, 0.0, 0, 0) if f == 1.0 else (_ENHANCE[base], z, f, 0, 0)
    raise ValueError(f"RandAugment: unknown op {name!r}")


# ---- the arithmetic on the host: numpy, one operation per rounding ------------------------------------------------------------------------------------------
def _luminance(f: np.ndarray) -> np.ndarray:
    """Image.convert("L") of uint8 [..., 3]"""
    v = f.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def _blend(d: np.ndarray, i: np.ndarray, alpha: float) -> np.ndarray:
    """Image.blend(d, i, alpha): fl32(d + fl32(alpha * (i - d))), truncated; clamped first where alpha lies outside [0, 1]"""
    a = np.float32(alpha)
    d32 = d.astype(np.float32)
    t = d32 + a * (i.astype(np.float32) - d32)
    if not (0.0 <= a <= 1.0):
        t = np.where(t <= 0, np.float32(0), np.where(t >= 255, np.float32(255), t))
    return t.astype(np.uint8)


def _smooth(f: np.ndarray) -> np.ndarray:
    """ImageFilter.SMOOTH of uint8 [T, H, W, 3]: the 3 x 3 kernel (1, 1, 1, 1, 5, 1, 1, 1, 1) / 13 in fp32 from 0.5, the row below first; border pixels are copied"""
    T, H, W, _ = f.shape
    out = f.copy()
    if H < 3 or W < 3:
        return out
    k1, k5 = np.float32(1.0) / np.float32(13.0), np.float32(5.0) / np.float32(13.0)
    v = f.astype(np.float32)
    ss = np.full((T, H - 2, W - 2, 3), 0.5, dtype=np.float32)
    for r, mid in ((2, k1), (1, k5), (0, k1)):               # rows y + 1, y, y - 1
        row = v[:, r:r + H - 2]
        ss = ss + ((row[:, :, 0:W - 2] * k1 + row[:, :, 1:W - 1] * mid) + row[:, :, 2:W] * k1)
    out[:, 1:H - 1, 1:W - 1] = np.clip(ss.astype(np.int32), 0, 255).astype(np.uint8)
    return out


def _cubic(v1, v2, v3, v4, d):
    p1, p2, p3, p4 = v2, -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def _affine(f: np.ndarray, a: Sequence[float], resample: int) -> np.ndarray:
    """Image.transform(size, AFFINE, a, resample, fillcolor=FILL) of uint8 [T, H, W, 3]"""
    T, H, W, _ = f.shape
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5)
    xin = a[0] * X + a[1] * Y + a[2]
    yin = a[3] * X + a[4] * Y + a[5]
    inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x, y = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x)[None, :, :, None], (yin - y)[None, :, :, None]
    v = f.astype(np.float64)
    if resample == BICUBIC:
        cols = [np.clip(x + k, 0, W - 1) for k in (-1, 0, 1, 2)]
        rows = [np.clip(y + k, 0, H - 1) for k in (-1, 0, 1, 2)]            # a row outside the frame repeats the previous value: the clamped row's
        r = [_cubic(*[v[:, ry, cx, :] for cx in cols], dx) for ry in rows]
        o = _cubic(r[0], r[1], r[2], r[3], dy)
    elif resample == BILINEAR:
        cols = [np.clip(x + k, 0, W - 1) for k in (0, 1)]
        rows = [np.clip(y + k, 0, H - 1) for k in (0, 1)]
        r = [v[:, ry, cols[0], :] + (v[:, ry, cols[1], :] - v[:, ry, cols[0], :]) * dx for ry in rows]
        o = r[0] + (r[1] - r[0]) * dy
    else:
        raise ValueError(f"RandAugment: resample {resample}")
    o = np.where(o <= 0.0, 0.0, np.where(o >= 255.0, 255.0, o)).astype(np.uint8)
    return np.where(inside[None, :, :, None], o, np.array(FILL, dtype=np.uint8))


def _autocontrast_lut(h: np.ndarray) -> np.ndarray:
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(ix * scale + offset))) for ix in range(256)], dtype=np.uint8)


def _equalize_lut(h: np.ndarray) -> np.ndarray:
    histo = [int(c) for c in h if c]
    step = (sum(histo) - histo[-1]) // 255 if len(histo) > 1 else 0
    if not step:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, dtype=np.uint8)


def apply_lowered(f: np.ndarray, low: Lowered) -> np.ndarray:
    """one lowered op on uint8 [T, H, W, 3] (numpy)"""
    op, a, fac, i0, i1 = low
    if op == OP_NONE:
        return f
    if op in (OP_AUTOCONTRAST, OP_EQUALIZE):
        out = np.empty_like(f)
        make = _autocontrast_lut if op == OP_AUTOCONTRAST else _equalize_lut
        for t in range(f.shape[0]):
            for c in range(3):
                out[t, ..., c] = make(np.bincount(f[t, ..., c].reshape(-1), minlength=256))[f[t, ..., c]]
        return out
    if op in (OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD):
        i = np.arange(256)
        lut = {OP_INVERT: 255 - i, OP_POSTERIZE: i & i0, OP_SOLARIZE: np.where(i < i0, i, 255 - i), OP_SOLARIZE_ADD: np.where(i < i1, np.minimum(255, i + i0), i)}[op]
        return lut.astype(np.uint8)[f]
    if op == OP_BRIGHTNESS:
        return _blend(np.zeros_like(f), f, fac)
    if op == OP_COLOR:
        return _blend(np.broadcast_to(_luminance(f)[..., None], f.shape), f, fac)
    if op == OP_CONTRAST:
        lum = _luminance(f).astype(np.int64).reshape(f.shape[0], -1)
        grey = np.array([int(float(s) / lum.shape[1] + 0.5) for s in lum.sum(axis=1)], dtype=np.uint8)
        return _blend(np.broadcast_to(grey[:, None, None, None], f.shape), f, fac)
    if op == OP_SHARPNESS:
        return _blend(_smooth(f), f, fac)
    if op == OP_AFFINE:
        return _affine(f, a, i0)
    raise ValueError(f"RandAugment: op code {op}")


def randaug_cpu(frames, plan: Sequence[Layer], resample: int = BICUBIC):
    """the kernels' arithmetic restated on the host for ONE clip: uint8 [T, H0, W0, 3] (a torch tensor or a numpy array; the same kind is returned) through the
    applied layers of `plan`"""
    is_t = isinstance(frames, torch.Tensor)
    f = frames.cpu().numpy() if is_t else np.asarray(frames)
    if f.dtype != np.uint8 or f.ndim != 4 or f.shape[3] != 3:
        raise ValueError("randaug_cpu: uint8 frames [T, H0, W0, 3] expected")
    for name, applied, args in plan:
        if applied:
            f = apply_lowered(f, lower(name, args, f.shape[1], f.shape[2], resample))
    f = np.ascontiguousarray(f)
    return torch.from_numpy(f.copy()) if is_t else f


class RandAugment:
    """The reference's RandAugment for clips of uint8 frames, on the device.

    draw()                               the plan for one clip: n layers (op name, applied, level arguments), from numpy's global state and `random` as the reference
                                         consumes them
    __call__(frames, plans=None)         frames as ClipIngest takes them; returns the augmented uint8 clips in the same form, on the device (the input is not written)
    augment_buffer(buf, T, layout, plans)   the same on a flat staged device buffer, IN PLACE; returns (buffer, layout) for ClipIngest.ingest_buffer
    On a CPU device the clips are computed by randaug_cpu."""

    def __init__(self, config_str: str = "rand-m7-n4-mstd0.5-inc1", interpolation: str = "bicubic", input_size=224, device=None):
        if interpolation == "random":
            raise NotImplementedError("RandAugment: interpolation='random' draws random.choice per FRAME and op; no recipe uses it and a clip's layer is one launch here")
        if interpolation not in ("bicubic", "bilinear"):
            raise ValueError(f"RandAugment: interpolation 'bicubic' or 'bilinear', got {interpolation!r}")
        self.magnitude, self.num_layers, weight_idx, mstd, increasing = parse_config(config_str)
        if weight_idx is not None:
            raise NotImplementedError("RandAugment: a 'w' section means weighted choice WITHOUT replacement; no recipe uses it")
        self.config_str, self.interpolation = config_str, interpolation
        self.resample = BICUBIC if interpolation == "bicubic" else BILINEAR
        size_min = min(input_size) if isinstance(input_size, (tuple, list)) else input_size
        self.hparams = {"translate_const": int(size_min * 0.45), "interpolation": self.resample, "img_mean": FILL}
        if mstd is not None:
            self.hparams["magnitude_std"] = mstd
        self.transforms = RAND_INCREASING_TRANSFORMS if increasing else RAND_TRANSFORMS
        self.prob = 0.5
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self._stats = {}

    # ---- the plan (host only) --------------------------------------------------------------------------------------------------------------------------
    def draw(self) -> List[Layer]:
        """RandAugment.__call__ and AugmentOp.__call__: one np.random.choice over the ops (size n, with replacement); per layer random.random() against prob, then
        random.gauss(m, mstd) clipped to [0, 10], then the level_fn (one more random.random() for the signed ops).  A skipped layer draws nothing more."""
        idx = np.random.choice(len(self.transforms), self.num_layers)
        plan = []
        for k in idx:
            name = self.transforms[int(k)]
            if self.prob < 1.0 and random.random() > self.prob:
                plan.append((name, False, ()))
                continue
            magnitude = self.magnitude
            mstd = self.hparams.get("magnitude_std", 0)
            if mstd and mstd > 0:
                magnitude = random.gauss(magnitude, mstd)
            magnitude = min(MAX_LEVEL, max(0, magnitude))
            plan.append((name, True, level_args(name, magnitude, self.hparams)))
        return plan

    # ---- the device side -------------------------------------------------------------------------------------------------------------------------------
    def _stats_on(self, device, nbytes: int) -> torch.Tensor:
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        s = self._stats.get(key)
        if s is None or s.numel() < nbytes:
            s = self._stats[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return s

    @staticmethod
    def half_of(nbytes: int) -> int:
        """the distance between a clip's two homes in a double-sized buffer whose first half holds `nbytes` of frames: the next multiple of 16"""
        return (int(nbytes) + 15) // 16 * 16

    def augment_buffer(self, buf: torch.Tensor, T: int, layout: Sequence[Tuple[int, int, int]], plans: Sequence[Sequence[Layer]]):
        """buf: a flat uint8 device buffer; layout[b] = (byte offset, H0, W0) of clip b's [T, H0, W0, 3] frames; plans[b]: clip b's layers.  The clips are augmented IN
        the buffer.  Where some layer needs the other half (an affine op, Sharpness) the buffer must hold every clip below half = numel // 2 (a multiple of 16), the
        upper half being scratch: ClipIngest.stage(..., double=True) makes such a buffer; any other buffer is copied into one first.  Returns (buffer, layout): where
        each clip lives after its last layer."""
        from . import ops
        B = len(layout)
        if len(plans) != B:
            raise ValueError(f"RandAugment: {len(plans)} plans for {B} clips")
        if buf.dim() != 1 or buf.dtype != torch.uint8 or not buf.is_cuda:
            raise ValueError("RandAugment.augment_buffer: a flat uint8 device buffer expected")
        T = int(T)
        lows = [[lower(n, a, H0, W0, self.resample) if ap else (OP_NONE, (0.0,) * 6, 0.0, 0, 0) for n, ap, a in plan] for plan, (_, H0, W0) in zip(plans, layout)]
        layers = max((len(l) for l in lows), default=0)
        span = max(int(off) + T * int(H0) * int(W0) * 3 for off, H0, W0 in layout)
        half = buf.numel() // 2
        if any(l[0] in NEIGHBOURHOOD for ls in lows for l in ls) and (half % 16 != 0 or span > half):
            half = self.half_of(span)
            big = torch.empty(2 * half, dtype=torch.uint8, device=buf.device)
            big[:span].copy_(buf[:span])
            buf = big
        where = [int(off) for off, _, _ in layout]
        stats = self._stats_on(buf.device, B * T * _lib.RANDAUG_STATS_BYTES)
        for k in range(layers):
            rows = (_lib.RandaugRow * B)()
            active = stats_needed = False
            for b, (ls, (_, H0, W0)) in enumerate(zip(lows, layout)):
                op, a, fac, i0, i1 = ls[k] if k < len(ls) else (OP_NONE, (0.0,) * 6, 0.0, 0, 0)
                r = rows[b]
                r.src, r.dst, r.H0, r.W0, r.op, r.i0, r.i1, r.f = where[b], where[b], int(H0), int(W0), op, i0, i1, fac
                for q in range(6):
                    r.a[q] = a[q]
                if op in NEIGHBOURHOOD:
                    r.dst = where[b] = where[b] + half if where[b] < half else where[b] - half
                active = active or op != OP_NONE
                stats_needed = stats_needed or op in NEEDS_STATS
            if stats_needed:
                ops.randaug_stats(buf, rows, T, stats)
            if active:
                ops.randaug_apply(buf, rows, T, stats)
        return buf, [(w, int(H0), int(W0)) for w, (_, H0, W0) in zip(where, layout)]

    def __call__(self, frames, plans: Optional[Sequence[Sequence[Layer]]] = None):
        from .ingest import check_clips
        clips, T = check_clips(frames, "RandAugment")
        if plans is None:
            plans = [self.draw() for _ in clips]
        if len(plans) != len(clips):
            raise ValueError(f"RandAugment: {len(plans)} plans for {len(clips)} clips")
        src_dev = clips[0].device
        device = src_dev if src_dev.type != "cpu" else self.device
        batched = isinstance(frames, torch.Tensor)
        if device.type == "cpu":
            out = [randaug_cpu(c, p, self.resample) for c, p in zip(clips, plans)]
            return torch.stack(out) if batched else out
        sizes = [c.numel() for c in clips]
        offsets = [0] + [int(v) for v in np.cumsum(sizes)[:-1]]
        half = self.half_of(sum(sizes))
        buf = torch.empty(2 * half, dtype=torch.uint8, device=device)           # the input is never written: its clips are copied into the lower half
        for c, o, n in zip(clips, offsets, sizes):
            buf[o:o + n].view(c.shape).copy_(c, non_blocking=True)
        buf, layout = self.augment_buffer(buf, T, [(o, c.shape[1], c.shape[2]) for o, c in zip(offsets, clips)], plans)
        out = [buf[o:o + n].view(c.shape) for (o, _, _), n, c in zip(layout, sizes, clips)]
        return torch.stack(out) if batched else out
