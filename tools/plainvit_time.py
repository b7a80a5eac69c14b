#!/usr/bin/env python3
"""Timing of the plain video ViT's pooled-head region on MI355X (bf16, B = 32, Nt = 1568, D = 768, C = 365), one process, alternating blocks:

  (a) forward + backward of the region (regions.PoolHeadRegionFn: devias_pool_head_fwd / _bwd) against the same computation composed from ATen with autograd
      (tests/plainvit_ref.pool_head, eager, same dtype).  Three figures each, named for what they are: the time per call by device events around a loop of calls,
      the HOST time to issue one call (host clock around the loop, before the synchronise), and, from one profiled call, the number of kernels and the SUM of their
      device durations (copies and memsets not counted).  The region must not be slower than the ATen composition in device-event time or in kernel time: the tool
      exits 1 otherwise.  Every other figure is reported, not gated.
  (b) the bytes per second of the two streaming kernels (pool_partial_kernel reads h once and writes the chunk sums; head_dx_kernel writes dx once), from their
      durations in that profiled call and byte counts computed from the shapes, beside the project's LayerNorm forward on the same [B * Nt, D] tensor in this
      process (reads and writes it once: the one-pass stream the other two are judged by).
  (c) forward + backward of the plain ViT (mean pooling, LabelSmoothingCrossEntropy) next to the slot model's (TrainLoss with precomputed teacher logits).

    python tools/plainvit_time.py [--out profiles/plainvit.txt] [--batch 32] [--rounds 6] [--iters 10]

Medians over `rounds` alternating blocks of `iters` calls after warm-up are reported with min and max."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

from region_timing import block, kernel_summary as fmt, kernels, med

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda"
NT, D, C = 1568, 768, 365


def region_pair(B, dtype=torch.bfloat16):
    import plainvit_ref as pr
    from devias_amd import _lib
    from devias_amd.regions import PoolHeadRegionFn
    g = torch.Generator().manual_seed(7)
    h = torch.randn((B * NT, D), generator=g).to(DEV, dtype).requires_grad_(True)
    dz = (torch.randn((B, C), generator=g) * 0.05).to(DEV, dtype)
    prm = {"fc_norm.weight": 1.0 + 0.1 * torch.randn(D, generator=g), "fc_norm.bias": 0.1 * torch.randn(D, generator=g),
           "head.weight": 0.02 * torch.randn((C, D), generator=g), "head.bias": torch.zeros(C)}
    master = {k: v.to(DEV).requires_grad_(True) for k, v in prm.items()}
    P = {k: v.to(DEV, dtype).requires_grad_(True) for k, v in prm.items()}
    meta = (B, NT, _lib.POOL_MEAN, 1e-6, dtype, True)

    def fused():
        h.grad = None
        for p in master.values():
            p.grad = None
        _, z = PoolHeadRegionFn.apply(h, master["fc_norm.weight"], master["fc_norm.bias"], master["head.weight"], master["head.bias"], meta)
        z.backward(dz)

    def eager():
        h.grad = None
        for p in P.values():
            p.grad = None
        _, z = pr.pool_head(h.view(B, NT, D), P, True)
        z.backward(dz)

    return fused, eager, h


def model_steps(B):
    import devias_amd
    from devias_amd import synth
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.modeling_finetune import vit_base_patch16_224
    from devias_amd.train_loss import TrainLoss
    slot = devias_amd.create_model("slot_vit_base_patch16_224", slot_matching_method="matching", init_scale=1e-3, compute_dtype="bf16", num_classes=400,
                                   num_scene_classes=365, all_frames=16, num_latents=2, agg_weights_tie=True, agg_depth=8)
    plain = vit_base_patch16_224(num_classes=C, all_frames=16, tubelet_size=2, init_scale=1e-3, use_mean_pooling=True, compute_dtype="bf16")
    for m in (slot, plain):
        synth.fill_module_(m, seed=0)
        m.to(DEV).train()
    x = synth.video(B, 16, 224, seed=1000).to(DEV)
    y, ys = synth.targets(B, 400, seed=1000).to(DEV), synth.targets(B, C, seed=1000).to(DEV)
    tl = synth.teacher_logits(B, 365, seed=1000).to(DEV)
    fg = tuple(t.to(DEV) for t in synth.fg_masks(B, 1568, 196, seed=1000))
    tcrit = TrainLoss(scene_criterion="KL", num_action_classes=400, slot_matching_method="matching", mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0,
                      scene_loss_weight=4000, sync_loss_dict=False)
    ccrit = LabelSmoothingCrossEntropy(0.1)

    def slot_step():
        slot.zero_grad(set_to_none=True)
        total, _, _ = tcrit(slot, slot(x), (None, tl), y, fg_mask=fg)
        total.backward()

    def plain_step():
        plain.zero_grad(set_to_none=True)
        ccrit(plain(x)[1], ys).backward()

    return slot_step, plain_step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plainvit.txt"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("plainvit_time.py measures on an MI355X: no GPU, no number")
    from devias_amd import ops
    B = a.batch
    lines = ["plain video ViT, pooled-head region, bf16, B = %d, Nt = %d, D = %d, C = %d, %s; rounds = %d alternating blocks of %d calls"
             % (B, NT, D, C, torch.cuda.get_device_name(0), a.rounds, a.iters)]
    fused, eager, h = region_pair(B)
    for fn in (fused, eager):
        for _ in range(5):
            fn()
    f, e = [], []
    for _ in range(a.rounds):
        f.append(block(fused, a.iters)); e.append(block(eager, a.iters))
    kf, ke = kernels(fused), kernels(eager)
    fd, ed = statistics.median(v[0] for v in f), statistics.median(v[0] for v in e)
    ok = fd <= ed
    if kf and ke:
        ok &= sum(t for _, t in kf) <= sum(t for _, t in ke)
    lines += ["", "(a) region forward + backward: fused      per call %s; host issue %s; %s" % (med([v[0] for v in f]), med([v[1] for v in f]), fmt(kf)),
              "                               eager ATen per call %s; host issue %s; %s" % (med([v[0] for v in e]), med([v[1] for v in e]), fmt(ke)),
              "    the region is %s the ATen composition (device-event time %.2fx%s)" % ("not slower than" if ok else "SLOWER THAN", ed / fd,
              ", kernel time %.2fx" % (sum(t for _, t in ke) / sum(t for _, t in kf)) if kf and ke else "")]
    # (b) the streams
    x = h.detach()
    gw, gb = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    ln = lambda: ops.layernorm_fwd(x, gw, gb, 1e-6)      # noqa: E731
    for _ in range(5):
        ln()
    kl = kernels(ln)
    es, rows = x.element_size(), B * NT
    chunks = (NT + 63) // 64
    want = {"pool_partial_kernel": rows * D * es + B * chunks * D * 4, "head_dx_kernel": rows * D * es + B * D * es}
    lines += ["", "(b) one-pass streams over the [%d, %d] bf16 tensor (bytes from the shapes over the kernel's duration in one profiled call)" % (rows, D)]
    for name, nbytes in want.items():
        t = [ms for n, ms in (kf or []) if name in n]
        lines.append("    %-22s %s" % (name, "%.1f us, %.2f TB/s (%d bytes)" % (t[0] * 1e3, nbytes / (t[0] * 1e-3) / 1e12, nbytes) if t else "not measured"))
    if kl:
        t = max(ms for _, ms in kl)
        nbytes = 2 * rows * D * es + 2 * rows * 4
        lines.append("    %-22s %.1f us, %.2f TB/s (%d bytes: read + write + the row statistics)" % ("layernorm forward", t * 1e3, nbytes / (t * 1e-3) / 1e12, nbytes))
    else:
        lines.append("    layernorm forward      not measured")
    if kf:
        lines.append("    the region's kernels: " + ", ".join("%s %.1f us" % (n.split("(")[0][-40:], t * 1e3) for n, t in kf))
    del fused, eager, h, x
    torch.cuda.empty_cache()
    # (c) the steps
    slot_step, plain_step = model_steps(B)
    for fn in (slot_step, plain_step):
        for _ in range(3):
            fn()
    s, p = [], []
    for _ in range(a.rounds):
        s.append(block(slot_step, a.iters)[0]); p.append(block(plain_step, a.iters)[0])
    lines += ["", "(c) forward + backward, ViT-B/16 16x224^2, B = %d: slot model + TrainLoss %s" % (B, med(s)),
              "                                                   plain ViT (mean pooling) + label-smoothing CE %s" % med(p)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
