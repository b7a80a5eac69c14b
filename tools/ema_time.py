#!/usr/bin/env python3
"""Device time of the optimizer step with and without the model EMA, over the real parameter list of slot_vit_base_patch16_224 (98.4 M fp32 values, the layer-decay
groups of devias_amd.optim_factory), in one process on one GPU:

    python tools/ema_time.py [--iters 20] [--rounds 9] [--other-lib PATH]

  adamw          devias_adamw_multi alone                                       28 bytes per parameter
  adamw_aa       the same launch again: the A/A spread a difference has to beat
  fused          devias_adamw_ema_multi: the shadow written by the AdamW launch  36
  two_launch     devias_adamw_multi, then devias_ema_multi                      40
  torch_loop     devias_adamw_multi, then timm's loop: per state_dict entry `ema_v.copy_(ema_v * decay + (1. - decay) * model_v)`
  adamw_other    (--other-lib) devias_adamw_multi of another build of the library, the parent commit's for one, on the same table: must agree with `adamw`

All variants are timed in alternating windows of `--iters` repetitions between device events, `--rounds` windows each; a line gives the median window in microseconds
per repetition, the spread (min..max) of the windows, and bytes moved over the median against the achievable HBM rate of MI355X_MICROARCH.md (6.3 TB/s).
Before timing, fused, two_launch and torch_loop are checked to leave the same bits in the shadows."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import devias_amd  # noqa: E402
from devias_amd import _lib, ops, optim_factory as of  # noqa: E402
from devias_amd.ema import ModelEma  # noqa: E402

HBM_ACHIEVABLE = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--other-lib", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    model = devias_amd.create_model("slot_vit_base_patch16_224", num_classes=400, all_frames=16, num_latents=2, slot_matching="matching",
                                    agg_weights_tie=True, agg_depth=8, drop_block_rate=None).cuda()
    assigner = of.LayerDecayValueAssigner.from_decay(0.75, model.get_num_layers())
    args = types.SimpleNamespace(opt="adamw", lr=1e-6, weight_decay=0.05, opt_eps=1e-8, opt_betas=[0.9, 0.999])
    opt = of.create_optimizer(args, model, get_num_layer=assigner.get_layer_id, get_layer_scale=assigner.get_scale)
    g = torch.Generator(device="cuda").manual_seed(1)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device="cuda", generator=g) * 0.01
    me = ModelEma(model, decay=a.decay)
    opt.step(ema=me)                                   # builds the plan: one table for the whole list, the shadow pointers in it
    (key, plan), = opt._plans.items()
    betas, eps = key[0], key[1]
    n_params = sum(p.numel() for p in model.parameters())
    T = (plan.table, plan.chunk_tensor, plan.chunk_index)
    msd, esd = model.state_dict(), me.state_dict()
    entries = sum(v.numel() for v in esd.values())

    def adamw():
        ops.adamw_multi(*T, betas[0], betas[1], eps)

    def fused():
        ops.adamw_ema_multi(*T, betas[0], betas[1], eps, a.decay)

    def two_launch():
        adamw()
        ops.ema_multi(*T, a.decay)

    def torch_loop():
        adamw()
        for k, ema_v in esd.items():
            ema_v.copy_(ema_v * a.decay + (1. - a.decay) * msd[k])

    paths = {"adamw": (adamw, 28 * n_params), "adamw_aa": (adamw, 28 * n_params), "fused": (fused, 36 * n_params),
             "two_launch": (two_launch, 40 * n_params), "torch_loop": (torch_loop, 28 * n_params + 12 * entries)}
    if a.other_lib:
        other = ctypes.CDLL(a.other_lib)
        other.devias_adamw_multi.restype, other.devias_adamw_multi.argtypes = _lib.PROTOTYPES["devias_adamw_multi"]
        if other.devias_version() < 174:                       # before ABI 174 the betas crossed as floats
            other.devias_adamw_multi.argtypes = [ctypes.c_float if t is ctypes.c_double else t for t in other.devias_adamw_multi.argtypes]

        def adamw_other():
            rc = other.devias_adamw_multi(T[0].data_ptr(), T[1].data_ptr(), T[2].data_ptr(), T[1].numel(), betas[0], betas[1], eps, 1.0, None,
                                          torch.cuda.current_stream().cuda_stream)
            assert rc == 0
        paths["adamw_other"] = (adamw_other, 28 * n_params)

    # the three EMA forms leave the same bits (the tied aggregator tensors are listed once per layer by state_dict: the loop updates them once per listing, so
    # they are compared for the parameters the optimizer launch covers exactly once)
    once = [k for k, v in esd.items() if sum(1 for w in esd.values() if w.data_ptr() == v.data_ptr()) == 1]
    snap = {k: esd[k].clone() for k in once}
    state = [t for p in model.parameters() for t in (p.data, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]
    state0 = [t.clone() for t in state]
    results = []
    for f in (fused, two_launch, torch_loop):
        for k in once:
            esd[k].copy_(snap[k])
        for t, t0 in zip(state, state0):               # every form starts from the same parameters and moments
            t.copy_(t0)
        f()
        results.append({k: esd[k].clone() for k in once})
    assert all(torch.equal(results[0][k], results[1][k]) and torch.equal(results[0][k], results[2][k]) for k in once), "the EMA forms disagree"
    del state0, snap, results

    times = {k: [] for k in paths}
    for f, _ in paths.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, (f, _) in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    out = {"what": "optimizer step (+ model EMA), microseconds per repetition between device events", "parameters": n_params, "state_dict_values": entries,
           "tensors": len(list(model.parameters())), "chunks": plan.n_chunks, "decay": a.decay, "iters": a.iters, "rounds": a.rounds}
    print(json.dumps(out))
    for k, v in times.items():
        med = statistics.median(v)
        print("%-12s median %8.1f us  (%8.1f .. %8.1f)  %6.1f MB  %5.2f TB/s = %4.1f %% of 6.3 TB/s" %
              (k, med, min(v), max(v), paths[k][1] / 1e6, paths[k][1] / med / 1e6, 100.0 * paths[k][1] / (med * 1e-6) / HBM_ACHIEVABLE))
    aa = abs(statistics.median(times["adamw"]) - statistics.median(times["adamw_aa"]))
    d = statistics.median(times["two_launch"]) - statistics.median(times["fused"])
    print("A/A spread of adamw: %.1f us; two_launch - fused: %.1f us" % (aa, d))
    if a.other_lib:
        print("adamw - adamw_other: %.1f us" % (statistics.median(times["adamw"]) - statistics.median(times["adamw_other"])))


if __name__ == "__main__":
    main()
