#!/usr/bin/env python3
"""Generate the plain video ViT's fixtures by RUNNING THE REAL REFERENCE (build container only):

  plainvit_mean_t8.npz / plainvit_cls_t8.npz   one fp32 training step of the reference's vit_base_patch16_224 (8 frames, B = 2, 365 classes, use_mean_pooling True /
                                               False) under LabelSmoothingCrossEntropy(0.1): token, logits, the loss, parameter names, gradient norms and 16
                                               sampled elements per parameter (make_goldens.generate's format)
  plainvit_state_dict_keys.json                names and shapes of both models' state_dicts
  plainvit_optim.json                          utils/optim_factory.get_parameter_groups with LayerDecayValueAssigner (0.75) and without, on both models

While generating, tests/plainvit_ref.py (the plain-PyTorch restatement the tests use at other shapes) is checked against the reference; a mismatch aborts.  The
fixtures are data only.  timm is not importable in the build container: its LabelSmoothingCrossEntropy is plainvit_ref.label_smoothing_ce.

Usage (in the build container):  python tests/golden/make_plainvit_goldens.py [--only step|keys|optim]
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
from oracle import ref_cpu  # noqa: E402
import plainvit_ref as pr  # noqa: E402

ROOT = mg.ROOT
CFG = dict(num_classes=365, all_frames=8, tubelet_size=2, init_scale=1.0)
B, SMOOTHING = 2, 0.1
MODES = (("mean", True), ("cls", False))


def build(reg, mean_pooling):
    with contextlib.redirect_stdout(io.StringIO()):
        return reg["vit_base_patch16_224"](use_mean_pooling=mean_pooling, **CFG)


def generate_step(reg, tag, mean_pooling):
    torch.manual_seed(0)
    model = build(reg, mean_pooling)
    model.train()
    synth.fill_module_(model, seed=0)
    names = [n for n, _ in model.named_parameters()]
    x = synth.video(B, CFG["all_frames"], 224, seed=1000)
    y = synth.targets(B, CFG["num_classes"], seed=1000)
    token, logits = model(x)
    loss = pr.label_smoothing_ce(logits, y, SMOOTHING)
    model.zero_grad()
    loss.backward()
    grads = {n: p.grad.detach() for n, p in model.named_parameters()}
    # ---- plainvit_ref against the reference
    cfg = ref_cpu.SlotViTConfig(all_frames=CFG["all_frames"])
    P = {n: p.detach().clone().requires_grad_(True) for n, p in model.named_parameters()}
    otok, ologits = pr.forward(P, cfg, x, mean_pooling)
    oloss = pr.label_smoothing_ce(ologits, y, SMOOTHING)
    oloss.backward()
    checks = {"token": mg.rel_err(otok, token), "logits": mg.rel_err(ologits, logits), "loss": mg.rel_err(oloss, loss)}
    checks.update({"d" + n: mg.rel_err(P[n].grad, grads[n]) for n in names})
    worst = sorted(checks.items(), key=lambda kv: -kv[1])[:4]
    print(f"[plainvit_{tag}_t8] plainvit_ref vs reference, worst: " + ", ".join(f"{k}={v:.1e}" for k, v in worst))
    assert max(checks.values()) < 2e-5, worst
    fx = {
        "config": np.array(repr(dict(CFG, use_mean_pooling=mean_pooling))), "batch": np.array(B), "smoothing": np.array(SMOOTHING),
        "token": token.detach().numpy(), "logits": logits.detach().numpy(), "loss": np.array(float(loss.detach().double())),
        "param_names": np.array(names),
        "grad_norms": np.array([float(grads[n].double().norm()) for n in names], dtype=np.float64),
        "grad_samples": np.stack([grads[n].reshape(-1)[torch.from_numpy(mg.sample_idx(n, grads[n].numel()))].numpy() for n in names]),
    }
    path = os.path.join(ROOT, "tests", "golden", f"plainvit_{tag}_t8.npz")
    np.savez_compressed(path, **fx)
    print(f"[plainvit_{tag}_t8] wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB) loss={float(loss.detach()):.9f}, {len(names)} parameters")


def generate_keys(reg):
    out = {}
    for tag, mp in MODES:
        m = reg["vit_base_patch16_224"](use_mean_pooling=mp, num_classes=365, all_frames=16, tubelet_size=2)
        out[tag] = {"state_dict": {k: list(v.shape) for k, v in m.state_dict().items()}, "named_parameters": [n for n, _ in m.named_parameters()],
                    "pos_embed": list(m.pos_embed.shape)}
    import inspect
    sig = inspect.signature(reg["vit_base_patch16_224"].__globals__["VisionTransformer"].__init__)
    out["defaults"] = {k: (v.default if isinstance(v.default, (int, float, bool, str, type(None))) else repr(v.default)) for k, v in sig.parameters.items()
                       if k != "self" and v.default is not inspect.Parameter.empty}
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "plainvit_state_dict_keys.json"), "w"))
    print("[plainvit keys]", {k: len(v["state_dict"]) for k, v in out.items() if k != "defaults"}, out["defaults"])


def generate_optim(reg):
    for mod, names in (("adafactor", ["Adafactor"]), ("adahessian", ["Adahessian"]), ("adamp", ["AdamP"]), ("lookahead", ["Lookahead"]), ("nadam", ["Nadam"]),
                       ("nvnovograd", ["NvNovoGrad"]), ("radam", ["RAdam"]), ("rmsprop_tf", ["RMSpropTF"]), ("sgdp", ["SGDP"])):
        m = types.ModuleType("timm.optim." + mod)
        for n in names:
            setattr(m, n, object)
        sys.modules["timm.optim." + mod] = m
    sys.modules.setdefault("timm.optim", types.ModuleType("timm.optim"))
    import utils.optim_factory as rof
    out = {"groups": {}}
    for tag, mp in MODES:
        m = build(reg, mp)
        nl = m.get_num_layers()
        for dtag, decay in (("ld0.75", 0.75), ("flat", 1.0)):
            assigner = rof.LayerDecayValueAssigner([decay ** (nl + 1 - i) for i in range(nl + 2)]) if decay < 1.0 else None
            with contextlib.redirect_stdout(io.StringIO()) as buf:
                rof.get_parameter_groups(m, 0.05, m.no_weight_decay(), assigner.get_layer_id if assigner else None, assigner.get_scale if assigner else None)
            txt = buf.getvalue()
            groups = json.loads(txt[txt.index("{"):])
            out["groups"][f"{tag}.{dtag}"] = {"num_layers": nl, "layer_decay": decay, "weight_decay": 0.05, "use_mean_pooling": mp,
                                              "groups": [[k, v["weight_decay"], v["lr_scale"], v["params"]] for k, v in groups.items()]}
    json.dump(out, open(os.path.join(ROOT, "tests", "golden", "plainvit_optim.json"), "w"))
    print("[plainvit optim]", {k: len(v["groups"]) for k, v in out["groups"].items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=[None, "step", "keys", "optim"])
    args = ap.parse_args()
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    reg = mg.install_reference()[0]
    if args.only in (None, "keys"):
        generate_keys(reg)
    if args.only in (None, "optim"):
        generate_optim(reg)
    if args.only in (None, "step"):
        for tag, mp in MODES:
            generate_step(reg, tag, mp)


if __name__ == "__main__":
    main()
