#!/usr/bin/env python3
"""Generate tests/golden/randaug_vectors.npz by RUNNING THE REAL REFERENCE (build container only): utils/transform/rand_augment.py, which needs only numpy and PIL,
on small uint8 clips (T = 2).

  per-op cases   every op of _RAND_INCREASING_TRANSFORMS and the non-increasing variants (Posterize, Solarize, Color, Contrast, Brightness, Sharpness) through
                 AugmentOp's own call at forced magnitudes 0, 10 and the recipe's 7 (prob = 1, no magnitude noise); the signed ops with both signs (random.random is
                 pinned for the call); the affine ops with bicubic and bilinear resampling.  The level arguments are captured by wrapping NAME_TO_OP.
                 Frame sets: 20 x 27 (every case), 37 x 23 (magnitude 7, bicubic), and every case on 1 x 9, 9 x 1, 2 x 2 (so small that Equalize's step is 0),
                 a constant 5 x 4 frame (AutoContrast sees hi <= lo, Equalize a single bin) and a 6 x 5 frame that touches 0 and 255 in every channel.
                 PIL refused no size for any op (the script would print it, and the case would be left out).
  chain cases    video_transforms.create_random_augment's transform (rand_augment_transform with its hparams) on a clip after random.seed / np.random.seed: the
                 seeds, the chosen ops, which were applied and with what arguments, the output, and the next draw of each generator after the call.  Seeds are
                 taken in order while they add coverage; the script asserts that every op is applied in some chain, that some chain has a skipped layer and some
                 chain the same op twice.

Layout: "frames.<set>"; per set "op.<set>.name / .mag / .neg / .interp / .arg / .out" (one row per case; arg is NaN where the op has none, interp is PIL's code);
"chain.config / .interp / .set / .seeds / .ops / .applied / .args / .next" (one row per chain) and "chain.out.<k>"; "parse.config / .values" what rand_augment_transform reads from a config string (magnitude, layers, magnitude_std or NaN, increasing, weighted);
"pillow" the Pillow version.

Usage (in the build container):  python tests/golden/make_randaug_goldens.py
This script never runs on the GPU box and nothing under tests/ imports it."""
from __future__ import annotations

import importlib.util
import os
import random

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("DEVIAS_REFERENCE", "/root/reference")
T = 2
FRAMES = {"f20x27": (20, 27), "f37x23": (37, 23), "f1x9": (1, 9), "f9x1": (9, 1), "f2x2": (2, 2), "const5x4": (5, 4), "ext6x5": (6, 5), "c14x11": (14, 11)}
SIGNED = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing")
AFFINE = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
NON_INCREASING = ("Posterize", "Solarize", "Color", "Contrast", "Brightness", "Sharpness")
MAGNITUDES = (0, 10, 7)
RECIPE = "rand-m7-n4-mstd0.5-inc1"
PARSE = (RECIPE, "rand", "rand-m9-n3-mstd0.5", "rand-mstd1-w0", "rand-m5-n2", "rand-inc0-m3", "rand-n1-inc1-mstd0.25-mstd2", "rand-m12-x3-n-inc", "rand-m7-n4-mstd0-inc1")


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_rand_augment", os.path.join(REF, "utils", "transform", "rand_augment.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def frames_of(name):
    H0, W0 = FRAMES[name]
    if name == "const5x4":
        return np.broadcast_to(np.array([77, 200, 13], dtype=np.uint8), (T, H0, W0, 3)).copy()
    f = np.random.RandomState(1000 * H0 + W0).randint(0, 256, size=(T, H0, W0, 3)).astype(np.uint8)
    if name == "ext6x5":
        f[:, 0, 0, :], f[:, -1, -1, :] = 0, 255
    return f


def hparams_of(input_size, interp):
    # video_transforms.create_random_augment's aa_params
    return {"translate_const": int(input_size * 0.45), "interpolation": interp}


def run_frames(fn, frames):
    out = fn([Image.fromarray(f) for f in frames])
    return np.stack([np.asarray(im) for im in out])


def main():
    ra = load_reference()
    fx, log = {"pillow": np.array(PIL.__version__)}, []
    for n in FRAMES:
        fx["frames." + n] = frames_of(n)
    orig_ops = dict(ra.NAME_TO_OP)

    def wrap(name):
        def f(img, *args, **kw):
            log.append((name, args))
            return orig_ops[name](img, *args, **kw)
        return f

    for n in orig_ops:
        ra.NAME_TO_OP[n] = wrap(n)

    # ---- per-op cases
    variants = []
    for name in tuple(ra._RAND_INCREASING_TRANSFORMS) + NON_INCREASING:
        for interp in ((Image.BICUBIC, Image.BILINEAR) if name in AFFINE else (Image.BICUBIC,)):
            if name in ("AutoContrast", "Equalize", "Invert"):
                variants.append((name, 7, 0, interp))
                continue
            for mag in MAGNITUDES:
                for neg in ((0, 1) if name in SIGNED and mag else (0,)):
                    variants.append((name, mag, neg, interp))
    real_random = random.random
    for fset in FRAMES:
        if fset == "c14x11":
            continue
        rows = []
        for name, mag, neg, interp in variants:
            if fset == "f37x23" and (mag != 7 or interp != Image.BICUBIC):
                continue
            op = ra.AugmentOp(name, prob=1.0, magnitude=mag, hparams=hparams_of(224, interp))
            del log[:]
            random.random = (lambda: 0.75) if neg else (lambda: 0.25)
            try:
                out = run_frames(op, fx["frames." + fset])
            except Exception as e:                                        # PIL refuses this size for this op: outside the op's domain
                print(f"[randaug_vectors] PIL refused {name} on {fset}: {e!r}")
                continue
            finally:
                random.random = real_random
            assert len(log) == T and all(l == log[0] for l in log) and len(log[0][1]) <= 1
            rows.append((name, mag, neg, interp, float(log[0][1][0]) if log[0][1] else np.nan, out))
        for k, (key, dt) in enumerate((("name", None), ("mag", np.int32), ("neg", np.int32), ("interp", np.int32), ("arg", np.float64), ("out", np.uint8))):
            fx[f"op.{fset}.{key}"] = np.array([r[k] for r in rows], dtype=dt)

    # ---- chain cases
    chains, applied_ops, skipped, twice = [], set(), False, False

    def run_chain(config, interp_name, fset, seeds):
        tf = ra.rand_augment_transform(config, hparams_of(224, {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}[interp_name]))
        names = {id(op): n for op, n in zip(tf.ops, ra._RAND_INCREASING_TRANSFORMS if "inc" in config else ra._RAND_TRANSFORMS)}
        chosen = []

        class Spy:
            def __init__(self, op):
                self.op = op

            def __call__(self, imgs):
                chosen.append([names[id(self.op)], len(log)])
                return self.op(imgs)

        tf.ops = [Spy(op) for op in tf.ops]
        del log[:]
        random.seed(seeds[0])
        np.random.seed(seeds[1])
        out = run_frames(tf, fx["frames." + fset])
        nxt = (random.random(), np.random.uniform())
        layers = []
        for k, (n, at) in enumerate(chosen):
            end = chosen[k + 1][1] if k + 1 < len(chosen) else len(log)
            if end == at:
                layers.append((n, False, np.nan))
            else:
                assert end - at == T and log[at][0] == n
                layers.append((n, True, float(log[at][1][0]) if log[at][1] else np.nan))
        return layers, out, nxt

    def keep(config, interp_name, fset, seeds, layers, out, nxt):
        nonlocal skipped, twice
        chains.append((config, interp_name, fset, seeds, layers, out, nxt))
        applied_ops.update(n for n, ap, _ in layers if ap)
        skipped = skipped or any(not ap for _, ap, _ in layers)
        ns = [n for n, ap, _ in layers if ap]
        twice = twice or len(set(ns)) < len(ns)

    for fset, seeds in (("f20x27", (1, 2)), ("f37x23", (3, 4))):
        keep(RECIPE, "bicubic", fset, seeds, *run_chain(RECIPE, "bicubic", fset, seeds))
    keep("rand-m9-n3-mstd0.5", "bilinear", "c14x11", (5, 6), *run_chain("rand-m9-n3-mstd0.5", "bilinear", "c14x11", (5, 6)))
    keep("rand-m5-n2", "bicubic", "c14x11", (7, 8), *run_chain("rand-m5-n2", "bicubic", "c14x11", (7, 8)))
    for s in range(100, 400):
        if set(ra._RAND_INCREASING_TRANSFORMS) <= applied_ops and skipped and twice:
            break
        seeds = (s, 7000 + s)
        layers, out, nxt = run_chain(RECIPE, "bicubic", "c14x11", seeds)
        ns = [n for n, ap, _ in layers if ap]
        if (set(ns) - applied_ops) or (not twice and len(set(ns)) < len(ns)) or (not skipped and len(ns) < len(layers)):
            keep(RECIPE, "bicubic", "c14x11", seeds, layers, out, nxt)
    assert set(ra._RAND_INCREASING_TRANSFORMS) <= applied_ops, set(ra._RAND_INCREASING_TRANSFORMS) - applied_ops
    assert skipped and twice
    nmax = max(len(c[4]) for c in chains)
    fx["chain.config"] = np.array([c[0] for c in chains])
    fx["chain.interp"] = np.array([c[1] for c in chains])
    fx["chain.set"] = np.array([c[2] for c in chains])
    fx["chain.seeds"] = np.array([c[3] for c in chains], dtype=np.int64)
    fx["chain.ops"] = np.array([[l[0] for l in c[4]] + [""] * (nmax - len(c[4])) for c in chains])
    fx["chain.applied"] = np.array([[l[1] for l in c[4]] + [False] * (nmax - len(c[4])) for c in chains])
    fx["chain.args"] = np.array([[l[2] for l in c[4]] + [np.nan] * (nmax - len(c[4])) for c in chains], dtype=np.float64)
    fx["chain.next"] = np.array([c[6] for c in chains], dtype=np.float64)
    for k, c in enumerate(chains):
        fx[f"chain.out.{k}"] = c[5]
    # ---- the config parser: what rand_augment_transform makes of a string (magnitude, layers, magnitude_std or NaN, increasing set, weighted choice)
    parsed = []
    for config in PARSE:
        tf = ra.rand_augment_transform(config, hparams_of(224, Image.BICUBIC))
        op = tf.ops[4]                                                    # Posterize or PosterizeIncreasing
        parsed.append((op.magnitude, tf.num_layers, op.hparams.get("magnitude_std", np.nan), float(op.level_fn is ra.LEVEL_TO_ARG["PosterizeIncreasing"]),
                       float(tf.choice_weights is not None)))
    fx["parse.config"], fx["parse.values"] = np.array(PARSE), np.array(parsed, dtype=np.float64)
    path = os.path.join(HERE, "randaug_vectors.npz")
    np.savez_compressed(path, **fx)
    ncase = sum(len(fx[f"op.{s}.name"]) for s in FRAMES if s != "c14x11")
    print(f"[randaug_vectors] Pillow {PIL.__version__}: {ncase} per-op cases, {len(chains)} chains, wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


if __name__ == "__main__":
    main()
