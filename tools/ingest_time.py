#!/usr/bin/env python3
"""Timing of the clip ingest on MI355X, one process, alternating blocks, every comparison with an A/A spread taken in the same call (tools/region_timing.py):

  (1) devias_clip_ingest at B = 32, T = 16, S = 224 on 256 x 340 uint8 frames, fp32 and bf16 output, with boxes drawn from the recipe's distribution under a fixed seed
      (ClipIngest.draw) and with the identity box (the validation centre crop), against the same transform composed from ATen on the device (float, / 255, normalise,
      per-clip slice, F.interpolate(bilinear, align_corners=False), flip, stack).  Device-event time per call after a warm-up, the kernels of one profiled call, the bytes
      read and written computed from the boxes (every source row the box's output rows touch, the box's columns, 3 bytes a pixel; the clip written once), and the
      resulting rate beside the project's LayerNorm forward stream on a bf16 [B * 1568, 768] tensor measured in the same call.
  (2) host to device: the uint8 batch through ClipIngest's pinned staging ring (pack + one non_blocking copy) and as a plain pinned copy, against the pinned fp32 clip
      it replaces.
  (3) with --parent-tree DIR (a built checkout of the parent commit): `python bench.py --gpus 1` here and there, alternating child processes started before this
      process opens the GPU (tools/multitask_time.bench_pair).

    python tools/ingest_time.py [--out profiles/ingest.txt] [--batch 32] [--rounds 6] [--iters 10] [--parent-tree DIR] [--bench-steps 20] [--bench-runs 2]

Nothing is gated: the yardsticks are the ATen composition, the LayerNorm stream and the parent commit; the reader judges the differences against the A/A spreads."""
from __future__ import annotations

import argparse
import os
import random
import statistics
import sys

import numpy as np
import torch

from region_timing import block, compare, med

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda"
T, H0, W0, S = 16, 256, 340, 224


def bytes_moved(boxes, B, esize):
    """(read, written): the source rows and columns under every box, T frames, 3 bytes a pixel (a downscaling box skips no row at these sizes: every row of the box
    is a tap of some output row or lies between two that are); the clip written once"""
    read = sum(T * h * w * 3 for (_, _, h, w, _) in boxes)
    return read, B * 3 * T * S * S * esize


def aten_ingest(frames, boxes, mean, std, dtype):
    x = frames.float() / 255.0
    x = ((x - mean) / std).permute(0, 4, 1, 2, 3)                       # B C T H W
    out = []
    for b, (i, j, h, w, fl) in enumerate(boxes):
        y = torch.nn.functional.interpolate(x[b][:, :, i:i + h, j:j + w], size=(S, S), mode="bilinear", align_corners=False)
        out.append(y.flip(-1) if fl else y)
    return torch.stack(out).to(dtype)


def ingest_lines(B, rounds, iters):
    from devias_amd import ops
    from devias_amd.ingest import ClipIngest
    lines = []
    g = torch.Generator().manual_seed(7)
    frames = torch.randint(0, 256, (B, T, H0, W0, 3), dtype=torch.uint8, generator=g).to(DEV)
    x = torch.randn((B * 1568, 768), generator=g).to(torch.bfloat16).to(DEV)
    gw, gb = torch.ones(768, device=DEV), torch.zeros(768, device=DEV)
    ln = lambda: ops.layernorm_fwd(x, gw, gb, 1e-6)                    # noqa: E731
    for _ in range(5):
        ln()
    ln_bytes = 2 * x.numel() * 2
    for dtype, dn in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        m = ClipIngest(S, out_dtype=dtype, device=DEV)
        random.seed(11)
        np.random.seed(12)
        drawn = [m.draw(H0, W0) for _ in range(B)]
        for boxes, what in ((drawn, "boxes drawn from the recipe's distribution (seeds 11 / 12)"), ([m.center_box(H0, W0)] * B, "the identity box (centre crop)")):
            mean, std = (torch.tensor(v, device=DEV) for v in (m.mean, m.std))
            fused = lambda: m(frames, boxes)                            # noqa: E731
            aten = lambda: aten_ingest(frames, boxes, mean, std, dtype)  # noqa: E731
            lines += compare("(1) %s clip [%d, 3, %d, %d, %d] from uint8 [%d, %d, %d, %d, 3], %s" % (dn, B, T, S, S, B, T, H0, W0, what), fused, aten, rounds, iters)
            t = statistics.median(block(fused, iters)[0] for _ in range(rounds))
            tl = statistics.median(block(ln, iters)[0] for _ in range(rounds))
            rd, wr = bytes_moved(boxes, B, 2 if dtype == torch.bfloat16 else 4)
            lines.append("    the ingest kernel: %.0f MB read + %.0f MB written over %.4f ms per call -> %.2f TB/s; LayerNorm forward bf16 [%d, 768] in the same call: %.0f MB over %.4f ms -> %.2f TB/s"
                         % (rd / 1e6, wr / 1e6, t, (rd + wr) / (t * 1e-3) / 1e12, x.shape[0], ln_bytes / 1e6, tl, ln_bytes / (tl * 1e-3) / 1e12))
            torch.cuda.empty_cache()
    return lines


def h2d_lines(B, rounds, iters):
    from devias_amd.ingest import ClipIngest
    g = torch.Generator().manual_seed(8)
    u8 = torch.randint(0, 256, (B, T, H0, W0, 3), dtype=torch.uint8, generator=g)
    u8_pinned = u8.pin_memory()
    clip = torch.empty((B, 3, T, S, S), dtype=torch.float32).normal_(generator=g).pin_memory()
    m = ClipIngest(S, device=DEV)
    clips = list(u8.unbind(0))
    d_u8, d_clip = torch.empty_like(u8, device=DEV), torch.empty_like(clip, device=DEV)
    fns = (("uint8 batch through the staging ring (pack into pinned memory + one non_blocking copy), %.0f MB" % (u8.numel() / 1e6), lambda: m._stage(clips, u8.numel(), torch.device(DEV))),
           ("uint8 batch, already pinned, one copy, %.0f MB" % (u8.numel() / 1e6), lambda: d_u8.copy_(u8_pinned, non_blocking=True)),
           ("the fp32 clip it replaces, pinned, one copy, %.0f MB" % (clip.numel() * 4 / 1e6), lambda: d_clip.copy_(clip, non_blocking=True)))
    lines = ["(2) host to device, per batch of %d clips:" % B]
    for name, fn in fns:
        for _ in range(3):
            fn()
        v = [block(fn, iters) for _ in range(rounds)]
        lines.append("    %s: device-event %s; host %s" % (name, med([a for a, _ in v]), med([b for _, b in v])))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    # child processes first: this process has not opened the GPU yet
    if a.parent_tree:
        from multitask_time import bench_pair
        bench_lines = bench_pair(os.path.abspath(a.parent_tree), a.bench_steps, a.bench_runs)
        bench_lines[0] = bench_lines[0].replace("(4)", "(3)")
    else:
        bench_lines = ["(3) python bench.py against the parent commit: not measured in this call (no --parent-tree)"]
    if not torch.cuda.is_available():
        sys.exit("ingest_time.py measures on an MI355X: no GPU, no number")
    B = a.batch
    lines = ["clip ingest on the device, B = %d, T = %d, S = %d, frames %d x %d, %s; rounds = %d alternating blocks of %d calls; `fused` = devias_clip_ingest, `eager ATen` = the same "
             "transform composed from ATen on the device" % (B, T, S, H0, W0, torch.cuda.get_device_name(0), a.rounds, a.iters), ""]
    lines += ingest_lines(B, a.rounds, a.iters) + [""]
    lines += h2d_lines(B, a.rounds, a.iters) + [""]
    lines += bench_lines
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
