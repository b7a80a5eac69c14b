#!/usr/bin/env python3
"""Timing of the two-token multi-task baseline on MI355X (bf16, B = 32, Nt = 1570, D = 768, 400 + 365 classes), one process, alternating blocks, every comparison
with an A/A spread taken in the same call (the SAME function measured in two interleaved slots: what the method itself cannot tell apart):

  (1) forward + backward of the head region (regions.TwoTokenHeadRegionFn: devias_two_token_head_fwd / _bwd) against the same computation composed from ATen with
      autograd (tests/multitask_ref.two_token_head, eager, same dtype: it normalises all B * Nt rows).  Three figures each: the time per call by device events around
      a loop of calls, the HOST time to issue one call (host clock around the loop, before the synchronise), and, from one profiled call, the number of kernels and
      the SUM of their device durations (copies and memsets not counted).
  (2) forward + backward of the distillation loss (multi_task_loss.DistillFn: devias_distill_fwd / _bwd; KL on [B, 365], and on [B, 765] with the unified head's
      pad) against the ATen composition (tests/multitask_ref.distill).
  (3) forward + backward of the two-token model + TrainLoss next to the plain cls-token ViT + label-smoothing CE (1569 tokens), in the same call.
  (4) with --parent-tree DIR (a built checkout of the parent commit): `python bench.py --gpus 1` here and there, alternating, as child processes started before this
      process opens the GPU; the headline `value` of each run, and the spread between this tree's own runs.

    python tools/multitask_time.py [--out profiles/multitask.txt] [--batch 32] [--rounds 6] [--iters 10] [--parent-tree DIR] [--bench-steps 20] [--bench-runs 2]

Medians over `rounds` alternating blocks of `iters` calls after warm-up are reported with min and max.  Nothing is gated: the yardsticks are the ATen composition
and the parent commit, the reader judges the differences against the A/A spreads."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

from region_timing import compare, med

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda"
NT, D, CA, CS = 1570, 768, 400, 365


def region_pair(B, unified, dtype=torch.bfloat16):
    import multitask_ref as mr
    from devias_amd.regions import TwoTokenHeadRegionFn
    g = torch.Generator().manual_seed(7)
    h = torch.randn((B * NT, D), generator=g).to(DEV, dtype).requires_grad_(True)
    ca, cs = (CA + CS, CA + CS) if unified else (CA, CS)
    dza, dzs = ((torch.randn((B, c), generator=g) * 0.05).to(DEV, dtype) for c in (ca, cs))
    prm = {"norm.weight": 1.0 + 0.1 * torch.randn(D, generator=g), "norm.bias": 0.1 * torch.randn(D, generator=g),
           "head.weight": 0.02 * torch.randn((ca, D), generator=g), "head.bias": torch.zeros(ca)}
    if not unified:
        prm.update({"scene_head.weight": 0.02 * torch.randn((cs, D), generator=g), "scene_head.bias": torch.zeros(cs)})
    master = {k: v.to(DEV).requires_grad_(True) for k, v in prm.items()}
    P = {k: v.to(DEV, dtype).requires_grad_(True) for k, v in prm.items()}
    meta = (B, NT, 1e-6, dtype, True)

    def fused():
        h.grad = None
        for p in master.values():
            p.grad = None
        _, za, _, zs = TwoTokenHeadRegionFn.apply(h, master["norm.weight"], master["norm.bias"], master["head.weight"], master["head.bias"],
                                                  master.get("scene_head.weight"), master.get("scene_head.bias"), meta)
        torch.autograd.backward([za, zs], [dza, dzs])

    def eager():
        h.grad = None
        for p in P.values():
            p.grad = None
        (_, za), (_, zs) = mr.two_token_head(h.view(B, NT, D), P)
        torch.autograd.backward([za, zs], [dza, dzs])

    return fused, eager


def distill_pair(B, pad, dtype=torch.bfloat16):
    import multitask_ref as mr
    from devias_amd import _lib
    from devias_amd.multi_task_loss import DistillFn
    g = torch.Generator().manual_seed(9)
    z = (torch.randn((B, pad + CS), generator=g) * 3.0).to(DEV, dtype).requires_grad_(True)
    t = (torch.randn((B, CS), generator=g) * 3.0).to(DEV)

    def fused():
        z.grad = None
        DistillFn.apply(z, t, _lib.DISTILL_KL, 2.0).backward()

    def eager():
        z.grad = None
        mr.distill(z.float(), t, "KL", pad, 2.0).backward()

    return fused, eager


def model_steps(B):
    from devias_amd import synth
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.modeling_finetune import vit_base_patch16_224
    from devias_amd.modeling_multi_task import disentangle_vit_base_patch16_224
    from devias_amd.multi_task_loss import TrainLoss
    two = disentangle_vit_base_patch16_224(num_classes=CA, num_scene_classes=CS, all_frames=16, tubelet_size=2, init_scale=1e-3, compute_dtype="bf16")
    plain = vit_base_patch16_224(num_classes=CA, all_frames=16, tubelet_size=2, init_scale=1e-3, use_mean_pooling=False, compute_dtype="bf16")
    for m in (two, plain):
        synth.fill_module_(m, seed=0)
        m.to(DEV).train()
    x = synth.video(B, 16, 224, seed=1000).to(DEV)
    y = synth.targets(B, CA, seed=1000).to(DEV)
    tl = synth.teacher_logits(B, CS, seed=1000).to(DEV)
    ccrit = LabelSmoothingCrossEntropy(0.1)
    tcrit = TrainLoss(ccrit, "KL", logit_criterion_weight=1.0, num_action_classes=CA, sync_loss_dict=False)

    def two_step():
        two.zero_grad(set_to_none=True)
        tcrit(two(x), (None, tl), y)[0].backward()

    def plain_step():
        plain.zero_grad(set_to_none=True)
        ccrit(plain(x)[1], y).backward()

    return two_step, plain_step


def bench_pair(parent, steps, runs):
    """`python bench.py` in this tree and in `parent`, alternating, each a child process of its own -> report lines"""
    def run(tree):
        out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "5"], cwd=tree, capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise RuntimeError("bench.py failed in %s: %s" % (tree, out.stderr[-2000:]))
        return float(json.loads(out.stdout.strip().splitlines()[-1])["value"])
    here, there = [], []
    for _ in range(runs):
        here.append(run(ROOT)); there.append(run(parent))
    lines = ["(4) python bench.py --gpus 1 --steps %d --warmup 5, alternating child processes, %d runs each" % (steps, runs),
             "    this tree     %s" % med(here, "clips/s"), "    parent commit %s" % med(there, "clips/s"),
             "    this / parent = %.4f; spread between this tree's own runs %.2f clips/s (%.2f %%)" % (
                 statistics.median(here) / statistics.median(there), max(here) - min(here), 100.0 * (max(here) - min(here)) / statistics.median(here))]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multitask.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-runs", type=int, default=2)
    a = ap.parse_args()
    bench_lines = bench_pair(os.path.abspath(a.parent_tree), a.bench_steps, a.bench_runs) if a.parent_tree else \
        ["(4) python bench.py against the parent commit: not measured in this call (no --parent-tree)"]
    if not torch.cuda.is_available():
        sys.exit("multitask_time.py measures on an MI355X: no GPU, no number")
    B = a.batch
    lines = ["two-token multi-task baseline, bf16, B = %d, Nt = %d, D = %d, %d + %d classes, %s; rounds = %d alternating blocks of %d calls"
             % (B, NT, D, CA, CS, torch.cuda.get_device_name(0), a.rounds, a.iters), ""]
    for unified in (False, True):
        fused, eager = region_pair(B, unified)
        lines += compare("(1) head region forward + backward, %s" % ("unified head [2B, 765]" if unified else "separate heads"), fused, eager, a.rounds, a.iters)
        del fused, eager
        torch.cuda.empty_cache()
    lines.append("")
    for pad in (0, CA):
        fused, eager = distill_pair(B, pad)
        lines += compare("(2) distillation KL forward + backward, student [B, %d]%s" % (pad + CS, " (unified head's pad)" if pad else ""), fused, eager, a.rounds, a.iters)
    lines.append("")
    two_step, plain_step = model_steps(B)
    lines += compare("(3) forward + backward, ViT-B/16 16x224^2, B = %d: two-token model (1570 tokens) + TrainLoss" % B, two_step, plain_step, a.rounds, max(1, a.iters // 2),
                     warm=3, old_name="plain cls ViT+CE", profiled=False)
    lines += [""] + bench_lines
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
