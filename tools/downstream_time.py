#!/usr/bin/env python3
"""Timing of the downstream recipe on MI355X (bf16, ViT-B/16 16x224^2, B = 12 -- the recipe's batch -- and B = 32), one process, alternating blocks:

  (a) forward + backward of the downstream step (slot-fusion model + LabelSmoothingCrossEntropy) against the slot recipe's forward + backward (slot model + TrainLoss
      with precomputed teacher logits), which this tool's subject does not change and which therefore is the yardstick.  The slot step is timed as TWO interleaved
      series (S1, D, S2, D, ...): the difference of their medians is the A/A spread of this very call.  The downstream step runs the same patch embed, encoder and
      aggregation block and strictly less arithmetic behind them, so it must be no slower than the slot step plus that spread: the tool exits 1 otherwise.
  (b) the fused head region + cross-entropy, forward and backward (devias_fusion_head_* + devias_softmax_ce_*), against tests/downstream_ref.py run eagerly on the
      GPU in the same dtype (ATen kernels; it computes the selection alone, with device-side indices).  Two figures each, named for what they are: the ISSUE time per
      call (device events around a host loop of calls: at these sizes mostly the host that issues the launches) and, from one profiled call, the number of kernels
      and the SUM of their device durations (torch.profiler's device events; copies and memsets are not counted).  The region must be faster in both.
  (c) peak memory of both steps (torch.cuda.max_memory_allocated over one step after a reset).

    python tools/downstream_time.py [--out profiles/downstream.txt] [--batches 12 32] [--rounds 6] [--iters 10]

Block times are device-event times over `iters` steps after warm-up; medians over `rounds` blocks are reported with min and max."""
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
ENC = dict(num_classes=400, num_scene_classes=365, all_frames=16, num_latents=2, agg_weights_tie=True, agg_depth=8)


def steps(B):
    import devias_amd
    from devias_amd import synth
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.train_loss import TrainLoss
    slot = devias_amd.create_model("slot_vit_base_patch16_224", slot_matching_method="matching", init_scale=1e-3, compute_dtype="bf16", **ENC)
    fus = devias_amd.create_model("slot_fusion_vit_base_patch16_224", head_type="mlp", downstream_nb_classes=48, use_input_ln=True, compute_dtype="bf16", **ENC)
    for m in (slot, fus):
        synth.fill_module_(m, seed=0)
        m.to(DEV).train()
    x = synth.video(B, 16, 224, seed=1000).to(DEV)
    y = synth.targets(B, 400, seed=1000).to(DEV)
    yd = synth.targets(B, 48, seed=1000).to(DEV)
    tl = synth.teacher_logits(B, 365, seed=1000).to(DEV)
    fg = tuple(t.to(DEV) for t in synth.fg_masks(B, 1568, 196, seed=1000))
    tcrit = TrainLoss(scene_criterion="KL", num_action_classes=400, slot_matching_method="matching", mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0,
                      scene_loss_weight=4000, sync_loss_dict=False)
    ccrit = LabelSmoothingCrossEntropy(0.1)

    def slot_step():
        slot.zero_grad(set_to_none=True)
        total, _, _ = tcrit(slot, slot(x), (None, tl), y, fg_mask=fg)
        total.backward()

    def fus_step():
        fus.zero_grad(set_to_none=True)
        ccrit(fus(x)[1], yd).backward()

    return slot_step, fus_step, fus


def head_pair(fus, B, dtype=torch.bfloat16):
    """the fused region + CE and the eager restatement on the same slots and parameters"""
    import downstream_ref as dr
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.regions import FusionHeadFn
    S, D = 2, 768
    g = torch.Generator().manual_seed(7)
    slots = (torch.randn((B * S, D), generator=g) * 0.5).to(DEV, dtype).requires_grad_(True)
    y = torch.randint(0, 48, (B,), generator=g).to(DEV)
    fh = fus.fusion_head
    names = ("head.weight", "head.bias", "action_norm.weight", "action_norm.bias", "scene_norm.weight", "scene_norm.bias", "fusion_head.fc_action_down.weight",
             "fusion_head.fc_action_down.bias", "fusion_head.fc_action_ln.weight", "fusion_head.fc_action_ln.bias", "fusion_head.fc_input_ln.weight",
             "fusion_head.fc_input_ln.bias", "fusion_head.classifier.weight", "fusion_head.classifier.bias")
    prm = dict(fus.named_parameters())
    args = [prm[n] for n in names]
    meta = (B, S, 400, fus.action_norm.eps, fh.fc_action_ln.eps, dtype, True)
    crit = LabelSmoothingCrossEntropy(0.1)
    P = {n: p.detach().to(dtype).requires_grad_(True) for n, p in prm.items() if n.startswith(("head.", "action_norm.", "scene_norm.", "fusion_head."))}

    def fused():
        slots.grad = None
        for p in args:
            p.grad = None
        _, out, _ = FusionHeadFn.apply(slots, *args, meta)
        crit(out, y).backward()

    def eager():
        slots.grad = None
        for p in P.values():
            p.grad = None
        o = dr.fusion_forward(slots.view(B, S, D), P, 400, use_input_ln=True)
        dr.label_smoothing_ce(o["out"].float(), y, 0.1).backward()

    return fused, eager


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "downstream.txt"))
    ap.add_argument("--batches", type=int, nargs="+", default=[12, 32])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("downstream_time.py measures on an MI355X: no GPU, no number")
    lines, ok = ["downstream recipe, bf16, ViT-B/16 16x224^2, %s; rounds = %d blocks of %d steps, alternating" % (torch.cuda.get_device_name(0), a.rounds, a.iters)], True
    for B in a.batches:
        slot_step, fus_step, fus = steps(B)
        for fn in (slot_step, fus_step):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        s1, s2, d = [], [], []
        for _ in range(a.rounds):
            s1.append(block(slot_step, a.iters)[0]); d.append(block(fus_step, a.iters)[0])
            s2.append(block(slot_step, a.iters)[0]); d.append(block(fus_step, a.iters)[0])
        spread = abs(statistics.median(s1) - statistics.median(s2))
        slot_ms, down_ms = statistics.median(s1 + s2), statistics.median(d)
        verdict = down_ms <= slot_ms + spread
        ok &= verdict
        lines += ["", "B = %d" % B,
                  "(a) forward + backward: slot recipe %s" % med(s1 + s2),
                  "                        slot series 1 %.3f ms, series 2 %.3f ms: A/A spread %.3f ms" % (statistics.median(s1), statistics.median(s2), spread),
                  "                        downstream  %s" % med(d),
                  "    downstream - slot = %+.3f ms (%s the slot step + the A/A spread)" % (down_ms - slot_ms, "within" if verdict else "SLOWER THAN")]
        peaks = []
        for fn in (slot_step, fus_step):
            torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peaks.append(torch.cuda.max_memory_allocated() / 2 ** 20)
        fused, eager = head_pair(fus, B)
        for fn in (fused, eager):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        f, e = [], []
        for _ in range(a.rounds):
            f.append(block(fused, 5 * a.iters)[0]); e.append(block(eager, 5 * a.iters)[0])
        kf, ke = kernels(fused), kernels(eager)
        tf, te = (sum(t for _, t in k) if k else None for k in (kf, ke))
        faster = statistics.median(f) < statistics.median(e) and (tf is None or te is None or tf < te)
        ok &= faster
        lines += ["(b) head region + cross-entropy, forward + backward: fused      issue time per call %s; %s" % (med(f), fmt(kf)),
                  "                                                     eager ATen issue time per call %s; %s" % (med(e), fmt(ke)),
                  "    the region is %s (issue time %.2fx%s)" % ("faster" if faster else "NOT FASTER", statistics.median(e) / statistics.median(f),
                                                                  ", kernel time %.2fx" % (te / tf) if tf and te else ""),
                  "(c) peak memory of one step: slot recipe %.1f MiB, downstream %.1f MiB (both models and their inputs resident)" % tuple(peaks)]
        del slot_step, fus_step, fus, fused, eager
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
