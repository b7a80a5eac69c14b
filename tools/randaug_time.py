#!/usr/bin/env python3
"""Timing of RandAugment on the device on MI355X, one call:

  (1) per op: every op of the recipe's set at magnitude 7 as ONE layer applied to all B clips (B = 32, T = 16, frames 256 x 340): device-event time per layer,
      kernel launches, bytes moved (a point op reads and writes the clips once; an op that needs statistics reads them once more; a neighbourhood op reads
      and writes once, to the other half) and the resulting rate.
  (2) batches drawn from the recipe's distribution (rand-m7-n4-mstd0.5-inc1, bicubic; at least 20 batches under fixed seeds): device time, launches and bytes per batch.
  (3) the same drawn plans through PIL itself -- the operations the reference's workers run, per frame -- on 16 worker processes, as clips/s; empty where PIL is
      not installed.  Measured first, before this process opens the GPU (the workers never do).
  (4) the LayerNorm forward stream on a bf16 [B * 1568, 768] tensor: the project's yardstick for streaming kernels.
  (5) with --parent-tree DIR (a built checkout of the parent commit): `python bench.py --gpus 1` here and there in alternating child processes.

    python tools/randaug_time.py [--out profiles/randaug.txt] [--batch 32] [--batches 20] [--iters 5] [--pil-clips 64] [--parent-tree DIR] [--bench-steps 20] [--bench-runs 2]

Nothing is gated: nobody had measured any of this before."""
from __future__ import annotations

import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

from region_timing import block, med

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
T, H0, W0 = 16, 256, 340
RECIPE = "rand-m7-n4-mstd0.5-inc1"
CLIP_BYTES = T * H0 * W0 * 3


def pil_clip(job):
    """one clip through its plan with PIL: what a worker of the reference does (16 frames per applied layer)"""
    from PIL import Image, ImageEnhance, ImageOps
    seed, plan = job
    frames = np.random.RandomState(seed).randint(0, 256, size=(T, H0, W0, 3)).astype(np.uint8)
    imgs = [Image.fromarray(f) for f in frames]
    kw = dict(resample=Image.BICUBIC, fillcolor=(128, 128, 128))
    t0 = time.perf_counter()
    for name, applied, args in plan:
        if not applied:
            continue
        a = args[0] if args else None
        fn = {"AutoContrast": lambda im: ImageOps.autocontrast(im), "Equalize": lambda im: ImageOps.equalize(im), "Invert": lambda im: ImageOps.invert(im),
              "Rotate": lambda im: im.rotate(a, **kw), "PosterizeIncreasing": lambda im: im if a >= 8 else ImageOps.posterize(im, a),
              "SolarizeIncreasing": lambda im: ImageOps.solarize(im, a), "SolarizeAdd": lambda im: im.point([min(255, i + a) if i < 128 else i for i in range(256)] * 3),
              "ColorIncreasing": lambda im: ImageEnhance.Color(im).enhance(a), "ContrastIncreasing": lambda im: ImageEnhance.Contrast(im).enhance(a),
              "BrightnessIncreasing": lambda im: ImageEnhance.Brightness(im).enhance(a), "SharpnessIncreasing": lambda im: ImageEnhance.Sharpness(im).enhance(a),
              "ShearX": lambda im: im.transform(im.size, Image.AFFINE, (1, a, 0, 0, 1, 0), **kw), "ShearY": lambda im: im.transform(im.size, Image.AFFINE, (1, 0, 0, a, 1, 0), **kw),
              "TranslateXRel": lambda im: im.transform(im.size, Image.AFFINE, (1, 0, a * im.size[0], 0, 1, 0), **kw),
              "TranslateYRel": lambda im: im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, a * im.size[1]), **kw)}[name]
        imgs = [fn(im) for im in imgs]
    return time.perf_counter() - t0


def pil_lines(plans, procs=16):
    try:
        import PIL
    except ImportError:
        return ["(3) the drawn plans through PIL on %d worker processes: PIL is not installed on this machine; clips/s: (not measured)" % procs]
    import multiprocessing as mp
    jobs = list(enumerate(plans))
    with mp.get_context("fork").Pool(procs) as pool:
        pool.map(pil_clip, jobs[:procs])                     # warm the workers
        t0 = time.perf_counter()
        busy = pool.map(pil_clip, jobs, chunksize=1)
        wall = time.perf_counter() - t0
    return ["(3) the same drawn plans through PIL %s on %d worker processes, %d clips of %d frames %d x %d: %.1f clips/s over %.2f s of wall time (the workers also make their frames: "
            "%.1f clips/s counting only the time inside the PIL operations, %.1f ms of them per clip on one CPU)"
            % (PIL.__version__, procs, len(jobs), T, H0, W0, len(jobs) / wall, wall, procs * len(jobs) / sum(busy), 1e3 * statistics.mean(busy))]


def moved(ra, plans):
    """(bytes moved, apply rows, stats rows) of the plans of one batch"""
    from devias_amd import randaug as R
    n = a = s = 0
    for p in plans:
        for name, applied, args in p:
            op = R.lower(name, args, H0, W0, ra.resample)[0] if applied else R.OP_NONE
            if op != R.OP_NONE:
                a += 1
                n += 2 * CLIP_BYTES
            if op in R.NEEDS_STATS:
                s += 1
                n += CLIP_BYTES
    return n, a, s


def device_lines(B, plans_of, iters):
    from devias_amd import ops
    from devias_amd.randaug import RAND_INCREASING_TRANSFORMS, RandAugment, level_args
    ra = RandAugment(RECIPE, "bicubic", device=DEV)
    half = ra.half_of(B * CLIP_BYTES)
    g = torch.Generator().manual_seed(7)
    buf = torch.empty(2 * half, dtype=torch.uint8, device=DEV)
    buf[:B * CLIP_BYTES].copy_(torch.randint(0, 256, (B * CLIP_BYTES,), dtype=torch.uint8, generator=g))
    layout = [(b * CLIP_BYTES, H0, W0) for b in range(B)]

    def timed(plans):
        fn = lambda: ra.augment_buffer(buf, T, layout, plans)    # noqa: E731
        fn()
        ops.counters(reset=True)
        fn()
        launches = ops.randaug_launches()
        v = [block(fn, iters) for _ in range(3)]
        return statistics.median(a for a, _ in v), statistics.median(h for _, h in v), launches

    lines = ["(1) one layer, the same op on all %d clips (magnitude 7, positive sign), %.0f MB of uint8 frames:" % (B, B * CLIP_BYTES / 1e6)]
    random.seed(0)
    for name in RAND_INCREASING_TRANSFORMS:
        real, random.random = random.random, lambda: 0.25
        try:
            args = level_args(name, 7, ra.hparams)
        finally:
            random.random = real
        plans = [[(name, True, args)]] * B
        ms, host, launches = timed(plans)
        nbytes = moved(ra, plans)[0]
        lines.append("    %-22s %8.4f ms per layer (host issue %.3f ms), %d launch%s, %4.0f MB moved -> %5.2f TB/s" % (name, ms, host, launches, "" if launches == 1 else "es", nbytes / 1e6,
                                                                                                                  nbytes / (ms * 1e-3) / 1e12))
    lines += ["", "(2) batches of %d clips with plans drawn from %s (seeds 100 + k / 200 + k), all four layers:" % (B, RECIPE)]
    per = []
    for k, plans in enumerate(plans_of):
        ms, host, launches = timed(plans)
        nbytes, a, s = moved(ra, plans)
        per.append((ms, host, launches, nbytes))
        lines.append("    batch %2d: %7.4f ms, host issue %.3f ms, %d launches (%d clip-layers applied, %d with statistics), %4.0f MB moved" % (k, ms, host, launches, a, s, nbytes / 1e6))
    tot = [p[0] for p in per]
    lines.append("    per batch: device %s; launches %.1f on average; %.0f MB moved on average; %.0f clips/s of device time"
                 % (med(tot), statistics.mean(p[2] for p in per), statistics.mean(p[3] for p in per) / 1e6, B / (statistics.median(tot) * 1e-3)))
    x = torch.randn((B * 1568, 768), generator=g).to(torch.bfloat16).to(DEV)
    gw, gb = torch.ones(768, device=DEV), torch.zeros(768, device=DEV)
    ln = lambda: ops.layernorm_fwd(x, gw, gb, 1e-6)              # noqa: E731
    for _ in range(5):
        ln()
    tl = statistics.median(block(ln, 10)[0] for _ in range(6))
    lines += ["", "(4) LayerNorm forward bf16 [%d, 768] in the same call: %.0f MB over %.4f ms -> %.2f TB/s" % (x.shape[0], 4 * x.numel() / 1e6, tl, 4 * x.numel() / (tl * 1e-3) / 1e12)]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randaug.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pil-clips", type=int, default=64)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    from devias_amd.randaug import RandAugment
    ra = RandAugment(RECIPE, "bicubic", device="cpu")
    plans_of = []
    for k in range(a.batches):
        random.seed(100 + k)
        np.random.seed(200 + k)
        plans_of.append([ra.draw() for _ in range(a.batch)])
    # child and worker processes first: this process has not opened the GPU yet
    flat = [p for plans in plans_of for p in plans][:a.pil_clips]
    third = pil_lines(flat)
    if a.parent_tree:
        from multitask_time import bench_pair
        bench_lines = bench_pair(os.path.abspath(a.parent_tree), a.bench_steps, a.bench_runs)
        bench_lines[0] = bench_lines[0].replace("(4)", "(5)")
    else:
        bench_lines = ["(5) python bench.py against the parent commit: not measured in this call (no --parent-tree)"]
    if not torch.cuda.is_available():
        sys.exit("randaug_time.py measures on an MI355X: no GPU, no number")
    lines = ["RandAugment on the device, B = %d, T = %d, frames %d x %d, %s; device-event time, median of 3 blocks of %d calls" % (a.batch, T, H0, W0, torch.cuda.get_device_name(0), a.iters), ""]
    lines += device_lines(a.batch, plans_of, a.iters) + [""] + third + [""] + bench_lines
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
