#!/usr/bin/env python3
"""Timing of mixup / cutmix on the device and of the soft-target loss on MI355X, one process, alternating blocks, every comparison with an A/A spread taken in the same
call (tools/region_timing.py):

  (1) the clip mix in place at [B, 3, 16, 224, 224], fp32 and bf16, batch-mode mixup and batch-mode cutmix at lam = 0.5 (the box the reference draws around the centre of
      the plane): ops.mixup_clips against the reference's ATen sequence on the same device (flip copy, two mul_, add_; the slice assignment from a flip copy).  Device-event
      time per call, host time to issue one call, kernels and their device time in one profiled call, and the bytes the kernel has to move over the device-event time of a call.
      With --nt-lib PATH (a build of the library with -DDEVIAS_MIXUP_NT, e.g. tools/build_variant_file.sh nt mixup -DDEVIAS_MIXUP_NT) the same section is measured
      again with non-temporal loads and stores, in a child process that loads that library.
  (2) at B, C = 400: mixup.mixup_target against the reference's mixup_target composed from ATen, and SoftTargetCrossEntropy forward + backward against timm's two-line
      loss composed from ATen with autograd; for each also the host time per call in one uninterrupted loop of 300 calls.
  (3) with --parent-tree DIR (a built checkout of the parent commit): `python bench.py --gpus 1` here and there, alternating child processes started before this
      process opens the GPU (tools/multitask_time.bench_pair).

    python tools/mixup_time.py [--out profiles/mixup.txt] [--batch 32] [--rounds 6] [--iters 10] [--nt-lib PATH] [--parent-tree DIR] [--bench-steps 20] [--bench-runs 2]

Nothing is gated: the yardsticks are the ATen sequence and the parent commit, the reader judges the differences against the A/A spreads."""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

from region_timing import block, compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
SHAPE = (3, 16, 224, 224)
C = 400
LAM = 0.5


def centre_box():
    H, W = SHAPE[-2:]
    bh, bw = int(H * np.sqrt(1 - LAM)), int(W * np.sqrt(1 - LAM))
    return H // 2 - bh // 2, H // 2 + bh // 2, W // 2 - bw // 2, W // 2 + bw // 2


def clip_pair(B, dtype, cutmix):
    from devias_amd import _lib, ops
    g = torch.Generator().manual_seed(7)
    x = torch.randn((B,) + SHAPE, generator=g).to(dtype).to(DEV)
    yl, yh, xl, xh = centre_box()
    row = _lib.MixupRow(_lib.MIX_CUTMIX, 1.0, 0.0, yl, yh, xl, xh, 0) if cutmix else _lib.MixupRow(_lib.MIX_MIXUP, LAM, 1.0 - LAM, 0, 0, 0, 0, 0)
    table = (_lib.MixupRow * B)(*([row] * B))

    def fused():
        ops.mixup_clips(x, table)

    def aten_mixup():          # mixup.py:205-206
        x_flipped = x.flip(0).mul_(1. - LAM)
        x.mul_(LAM).add_(x_flipped)

    def aten_cutmix():         # mixup.py:203
        x[..., yl:yh, xl:xh] = x.flip(0)[..., yl:yh, xl:xh]

    H, W = SHAPE[-2:]
    size = x.numel() * x.element_size()
    moved = size * ((yh - yl) / H + (yh - yl) * (xh - xl) / (H * W)) if cutmix else 2.0 * size          # rows [yl, yh) read, the box written; everything read and written
    return fused, (aten_cutmix if cutmix else aten_mixup), moved, size


def clip_lines(B, rounds, iters, label):
    lines = []
    for dtype, dn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        for cutmix in (False, True):
            fused, aten, moved, size = clip_pair(B, dtype, cutmix)
            name = "(1%s) %s clips [%d, 3, 16, 224, 224] (%.0f MB), batch-mode %s at lam = 0.5" % (label, dn, B, size / 1e6, "cutmix" if cutmix else "mixup")
            lines += compare(name, fused, aten, rounds, iters)
            t = statistics.median(block(fused, iters)[0] for _ in range(rounds))          # ms per call by device events, launches back to back
            lines.append("    the clip kernel: %.0f MB to move (%.2f clip-passes) over %.4f ms per call -> %.2f TB/s" % (moved / 1e6, moved / size, t, moved / (t * 1e-3) / 1e12))
            del fused, aten
            torch.cuda.empty_cache()
    return lines


def target_pair(B):
    from devias_amd import mixup as mx
    g = torch.Generator().manual_seed(9)
    y = torch.randint(0, C, (B,), generator=g).to(DEV)

    def fused():
        mx.mixup_target(y, C, LAM, 0.1, DEV)

    def one_hot(t, on, off):          # mixup.py:17-19
        return torch.full((t.size()[0], C), off, device=DEV).scatter_(1, t.long().view(-1, 1), on)

    def aten():                       # mixup.py:22-27
        off = 0.1 / C
        on = 1. - 0.1 + off
        return one_hot(y, on, off) * LAM + one_hot(y.flip(0), on, off) * (1. - LAM)

    return fused, aten


def loss_pair(B, dtype):
    from devias_amd import mixup as mx
    from devias_amd.losses import SoftTargetCrossEntropy
    g = torch.Generator().manual_seed(11)
    z = (torch.randn((B, C), generator=g) * 3.0).to(dtype).to(DEV).requires_grad_(True)
    t = mx.mixup_target(torch.randint(0, C, (B,), generator=g).to(DEV), C, LAM, 0.1, DEV)
    crit = SoftTargetCrossEntropy()

    def fused():
        z.grad = None
        crit(z, t).backward()

    def aten():                       # timm.loss.SoftTargetCrossEntropy
        z.grad = None
        torch.sum(-t * torch.nn.functional.log_softmax(z, dim=-1), dim=-1).mean().backward()

    return fused, aten


def host_loop(fn, n=300):
    """host microseconds to issue one call in ONE loop of n calls (the device queue stays full: no synchronise between blocks of ten, as in a training step)"""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixup.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--nt-lib", default=None)
    ap.add_argument("--clips-only", default=None, help="print section (1) under this label and stop (the child of --nt-lib)")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    if a.clips_only is not None:
        print("\n".join(clip_lines(a.batch, a.rounds, a.iters, a.clips_only)))
        return
    # child processes first: this process has not opened the GPU yet
    if a.parent_tree:
        from multitask_time import bench_pair
        bench_lines = bench_pair(os.path.abspath(a.parent_tree), a.bench_steps, a.bench_runs)
        bench_lines[0] = bench_lines[0].replace("(4)", "(3)")
    else:
        bench_lines = ["(3) python bench.py against the parent commit: not measured in this call (no --parent-tree)"]
    nt_lines = []
    if a.nt_lib:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--clips-only", ", non-temporal loads and stores", "--batch", str(a.batch), "--rounds", str(a.rounds),
                              "--iters", str(a.iters)], env=dict(os.environ, DEVIAS_LIB_PATH=os.path.abspath(a.nt_lib)), capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise RuntimeError("the non-temporal run failed: %s" % out.stderr[-2000:])
        nt_lines = [""] + [ln for ln in out.stdout.splitlines() if ln.startswith(("(1", "    "))]
    if not torch.cuda.is_available():
        sys.exit("mixup_time.py measures on an MI355X: no GPU, no number")
    B = a.batch
    lines = ["mixup / cutmix on the device and the soft-target loss, B = %d, %s; rounds = %d alternating blocks of %d calls; `fused` = this library, `eager ATen` = the reference's tensor expressions"
             % (B, torch.cuda.get_device_name(0), a.rounds, a.iters), ""]
    lines += clip_lines(B, a.rounds, a.iters, "")
    lines += nt_lines + [""]
    fused, aten = target_pair(B)
    lines += compare("(2) soft target [%d, %d] from int64 labels" % (B, C), fused, aten, a.rounds, a.iters)
    lines.append("    host time to issue one call in one loop of 300 calls: fused %.1f us, eager ATen %.1f us" % (host_loop(fused), host_loop(aten)))
    for dtype, dn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        fused, aten = loss_pair(B, dtype)
        lines += compare("(2) SoftTargetCrossEntropy forward + backward, %s logits [%d, %d]" % (dn, B, C), fused, aten, a.rounds, a.iters)
        lines.append("    host time to issue one call in one loop of 300 calls: fused %.1f us, eager ATen %.1f us" % (host_loop(fused), host_loop(aten)))
    lines += [""] + bench_lines
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
