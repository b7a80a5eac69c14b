#!/usr/bin/env python3
"""Generate the downstream-recipe fixtures by RUNNING THE REAL REFERENCE (build container only):

  downstream_t8.npz                 one fp32 step of the reference's slot_fusion_vit_base_patch16_224 (8 frames, B = 2, num_latents=2, tied depth 8, head_type='mlp',
                                    downstream_nb_classes=48, use_input_ln) under LabelSmoothingCrossEntropy(0.1): input, out, idx, the loss, parameter names, gradient
                                    norms and 16 sampled elements per parameter (make_goldens.generate's format), and the names of the parameters without a gradient
  downstream_state_dict_keys.json   names and shapes of that model's state_dict
  downstream_optim.json             utils/optim_factory.get_parameter_groups with LayerDecayValueAssigner on that model

While generating, tests/downstream_ref.py (the plain-PyTorch restatement the tests use at other shapes) is checked against the reference on the slots the reference
computed; a mismatch aborts, and so does a selection whose relative gap to the runner-up slot is below 0.05 in float64.  The fixtures are data only.

timm is not importable in the build container: its LabelSmoothingCrossEntropy is downstream_ref.label_smoothing_ce (timm/loss/cross_entropy.py, five lines).

Usage (in the build container):  python tests/golden/make_downstream_goldens.py [--only step|keys|optim]
This script never runs on the GPU box and nothing under tests/ imports it.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_goldens as mg  # noqa: E402  (puts the repository root and tests/ on sys.path)

from devias_amd import synth  # noqa: E402
import downstream_ref as dr  # noqa: E402

ROOT = mg.ROOT
CFG = dict(num_classes=400, num_scene_classes=365, all_frames=8, num_latents=2, agg_weights_tie=True, agg_depth=8, head_type="mlp", slot_fusion_method="concat",
           downstream_nb_classes=48, use_input_ln=True)
B, SMOOTHING, MIN_GAP = 2, 0.1, 0.05


def install():
    ref = mg.install_reference()
    import model.modeling_slot_fusion  # noqa: F401  (registers slot_fusion_vit_base_patch16_224 in ref[0])
    return ref


def build(reg):
    with contextlib.redirect_stdout(io.StringIO()):
        m = reg["slot_fusion_vit_base_patch16_224"](**CFG)
    return m


def generate_step(reg):
    torch.manual_seed(0)
    model = build(reg)
    model.train()
    synth.fill_module_(model, seed=0)
    names = [n for n, _ in model.named_parameters()]
    assert len(names) == 196, len(names)
    x = synth.video(B, CFG["all_frames"], 224, seed=1000)
    y = synth.targets(B, CFG["downstream_nb_classes"], seed=1000)
    taps = {}
    model.agg_block.register_forward_hook(lambda m, i, o: taps.__setitem__("slots", o[0]))
    inp, out = model(x)
    loss = dr.label_smoothing_ce(out, y, SMOOTHING)
    model.zero_grad()
    taps["slots"].retain_grad()
    loss.backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    no_grad = [n for n in names if grads[n] is None]
    assert sorted(no_grad) == sorted(dr.NO_GRAD_NAMES), no_grad
    # ---- downstream_ref on the reference's slots: float32 against the reference, float64 for the selection gap
    S, D, nb = CFG["num_latents"], 768, CFG["num_classes"]
    slots = taps["slots"].detach()
    P = {n: p.detach().clone().requires_grad_(True) for n, p in model.named_parameters() if not n.startswith(("blocks.", "patch_embed.", "agg_block.", "norm."))}
    sl = slots.clone().requires_grad_(True)
    o = dr.fusion_forward(sl, P, nb, use_input_ln=True)
    oloss = dr.label_smoothing_ce(o["out"], y, SMOOTHING)
    oloss.backward()
    checks = {"input": mg.rel_err(o["input"], inp), "out": mg.rel_err(o["out"], out), "loss": mg.rel_err(oloss, loss), "dslots": mg.rel_err(sl.grad, taps["slots"].grad)}
    for n in P:
        if n in no_grad:
            assert P[n].grad is None, n
        else:
            checks["d" + n] = mg.rel_err(P[n].grad, grads[n])
    print("[downstream_t8] downstream_ref vs reference: " + ", ".join(f"{k}={v:.1e}" for k, v in checks.items()))
    assert max(checks.values()) < 2e-5, checks
    Z64 = torch.nn.functional.linear(slots.double().reshape(B * S, D), P["head.weight"].detach().double(), P["head.bias"].detach().double())
    idx64, gaps = dr.select(Z64, B, S, nb)
    print(f"[downstream_t8] selection {idx64.tolist()}, relative gaps to the runner-up slot {gaps.tolist()}")
    assert float(gaps.min()) >= MIN_GAP, gaps
    assert torch.equal(idx64, o["idx"])
    rows = slots[torch.arange(B), idx64[:, 0]]
    assert mg.rel_err(torch.nn.functional.layer_norm(rows, (D,), P["action_norm.weight"].detach(), P["action_norm.bias"].detach(), 1e-6), inp[:, :D]) < 2e-5
    zero = lambda n: torch.zeros_like(dict(model.named_parameters())[n])      # noqa: E731
    g = {n: (grads[n].detach() if grads[n] is not None else zero(n)) for n in names}
    fx = {
        "config": np.array(repr(CFG)), "batch": np.array(B), "smoothing": np.array(SMOOTHING),
        "input": inp.detach().numpy(), "out": out.detach().numpy(), "idx": idx64.numpy().astype(np.int32), "gaps": gaps.numpy(),
        "slots": slots.numpy(), "dslots": taps["slots"].grad.numpy(),
        "loss": np.array(float(loss.detach().double())),
        "param_names": np.array(names), "no_grad_names": np.array(no_grad),
        "grad_norms": np.array([float(g[n].double().norm()) for n in names], dtype=np.float64),
        "grad_samples": np.stack([g[n].reshape(-1)[torch.from_numpy(mg.sample_idx(n, g[n].numel()))].numpy() for n in names]),
    }
    path = os.path.join(ROOT, "tests", "golden", "downstream_t8.npz")
    np.savez_compressed(path, **fx)
    print(f"[downstream_t8] wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB) loss={float(loss):.9f}")


def generate_keys(reg):
    m = build(reg)
    out = {"slot_fusion_vit_base_patch16_224.tied_s2_d8_cd48": {k: list(v.shape) for k, v in m.state_dict().items()},
           "named_parameters": len(list(m.named_parameters()))}
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "downstream_state_dict_keys.json"), "w"))
    print("[downstream keys]", len(out["slot_fusion_vit_base_patch16_224.tied_s2_d8_cd48"]), out["named_parameters"])


def generate_optim(reg):
    for mod, names in (("adafactor", ["Adafactor"]), ("adahessian", ["Adahessian"]), ("adamp", ["AdamP"]), ("lookahead", ["Lookahead"]), ("nadam", ["Nadam"]),
                       ("nvnovograd", ["NvNovoGrad"]), ("radam", ["RAdam"]), ("rmsprop_tf", ["RMSpropTF"]), ("sgdp", ["SGDP"])):
        m = types.ModuleType("timm.optim." + mod)
        for n in names:
            setattr(m, n, object)
        sys.modules["timm.optim." + mod] = m
    sys.modules.setdefault("timm.optim", types.ModuleType("timm.optim"))
    import utils.optim_factory as rof
    m = build(reg)
    nl = m.get_num_layers()
    out = {"groups": {}}
    for tag, decay, agg_scale in (("ld0.75", 0.75, 0.1), ("flat", 1.0, 0.1)):
        assigner = rof.LayerDecayValueAssigner([decay ** (nl + 1 - i) for i in range(nl + 2)]) if decay < 1.0 else None
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            rof.get_parameter_groups(m, 0.05, m.no_weight_decay(), assigner.get_layer_id if assigner else None, assigner.get_scale if assigner else None,
                                     agg_block_scale=agg_scale)
        txt = buf.getvalue()
        names = json.loads(txt[txt.index("{"):])
        out["groups"][tag] = {"num_layers": nl, "layer_decay": decay, "agg_block_scale": agg_scale, "weight_decay": 0.05,
                              "groups": [[k, v["weight_decay"], v["lr_scale"], v["params"]] for k, v in names.items()]}
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "downstream_optim.json"), "w"))
    print("[downstream optim]", {k: len(v["groups"]) for k, v in out["groups"].items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=[None, "step", "keys", "optim"])
    args = ap.parse_args()
    torch.set_num_threads(os.cpu_count() or 8)
    reg = install()[0]
    if args.only in (None, "keys"):
        generate_keys(reg)
    if args.only in (None, "optim"):
        generate_optim(reg)
    if args.only in (None, "step"):
        generate_step(reg)


if __name__ == "__main__":
    main()
