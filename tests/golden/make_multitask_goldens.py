#!/usr/bin/env python3
"""Generate the two-token multi-task baseline's fixtures by RUNNING THE REAL REFERENCE (build container only):

  multitask_t8.npz / multitask_unified_t8.npz   one fp32 training step of the reference's disentangle_vit_base_patch16_224 (8 frames, B = 2, 400 action + 365 scene
                                                classes, separate heads / unified head) under the driver's TrainLoss(LabelSmoothingCrossEntropy(0.1), 'KL') with weight
                                                1.0 / 2.0 against a stored synthetic teacher [2, 365]: both tokens, both logits, the three losses, parameter names,
                                                gradient norms and 16 sampled elements per parameter (make_goldens.generate's format)
  multitask_loss.npz                            the driver's TrainLoss alone: {KL, CE} x {separate, unified} at a few (B, Ca, Cs), peaked logits, one teacher row
                                                with a duplicated maximum: inputs, the three losses, the gradients of both student logits
  multitask_state_dict_keys.json                names and shapes of both head modes' state_dicts
  multitask_optim.json                          utils/optim_factory.get_parameter_groups with LayerDecayValueAssigner (0.75) and without, on both head modes

While generating, tests/multitask_ref.py (the plain-PyTorch restatement the tests use at other shapes) is checked against the reference; a mismatch aborts.  The
fixtures are data only.  timm is not importable in the build container: its LabelSmoothingCrossEntropy is multitask_ref.label_smoothing_ce, and the driver's heavy
imports (datasets, engines, optimizers, mixup) are stand-in modules.

Usage (in the build container):  python tests/golden/make_multitask_goldens.py [--only step|loss|keys|optim]
This script never runs on the GPU box and nothing under tests/ imports it.
"""
from __future__ import annotations

import argparse
import contextlib
import inspect
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
import multitask_ref as mr  # noqa: E402

ROOT = mg.ROOT
GOLD = os.path.join(ROOT, "tests", "golden")
CFG = dict(num_classes=400, num_scene_classes=365, all_frames=8, tubelet_size=2, init_scale=1.0)
B, SMOOTHING = 2, 0.1
MODES = (("multitask", False, 1.0), ("multitask_unified", True, 2.0))          # (file tag, unified_head, logit_criterion_weight)
LOSS_SHAPES = ((1, 5, 7), (3, 101, 365), (4, 400, 365))                         # (B, Ca, Cs)
LOSS_WEIGHT, LOSS_STD = 2.0, 6.0


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install_driver():
    """the reference's registry with the multi-task model in it, the driver's TrainLoss and the reference's utils.optim_factory"""
    reg = mg.install_reference()[0]
    for mod, names in (("adafactor", ["Adafactor"]), ("adahessian", ["Adahessian"]), ("adamp", ["AdamP"]), ("lookahead", ["Lookahead"]), ("nadam", ["Nadam"]),
                       ("nvnovograd", ["NvNovoGrad"]), ("radam", ["RAdam"]), ("rmsprop_tf", ["RMSpropTF"]), ("sgdp", ["SGDP"])):
        _mod("timm.optim." + mod, **{n: object for n in names})
    sys.modules.setdefault("timm.optim", types.ModuleType("timm.optim"))
    sys.modules["timm.models"].create_model = None
    _mod("timm.loss", LabelSmoothingCrossEntropy=object, SoftTargetCrossEntropy=object)
    _mod("utils.transform.mixup", Mixup=object)
    _mod("dataset"); _mod("dataset.datasets", build_dataset=None)
    _mod("engine"); _mod("engine.engine_for_multi_task", train_one_epoch=None, validation_one_epoch=None, final_test=None, merge=None, final_test_with_scene_label=None)
    import utils as ref_utils
    ref_utils.utils = _mod("utils.utils", NativeScalerWithGradNormCount=object, multiple_samples_collate=None)
    import utils.optim_factory as rof
    import run_multi_task_finetuning as drv          # (registers disentangle_vit_base_patch16_224 through model.modeling_multi_task)
    return reg, drv.TrainLoss, rof


def build(reg, unified):
    with contextlib.redirect_stdout(io.StringIO()):
        return reg["disentangle_vit_base_patch16_224"](unified_head=unified, **CFG)


def teacher_logits(b, cs, seed, std=3.0):
    return (torch.randn((b, cs), generator=torch.Generator().manual_seed(seed)) * std).contiguous()


def generate_step(reg, TrainLoss, tag, unified, weight):
    torch.manual_seed(0)
    model = build(reg, unified)
    model.train()
    synth.fill_module_(model, seed=0)
    names = [n for n, _ in model.named_parameters()]
    x = synth.video(B, CFG["all_frames"], 224, seed=1000)
    y = synth.targets(B, CFG["num_classes"], seed=1000)
    teacher = teacher_logits(B, CFG["num_scene_classes"], 77)
    crit = TrainLoss(lambda z, t: mr.label_smoothing_ce(z, t, SMOOTHING), "KL", unified_head=unified, num_action_classes=CFG["num_classes"], logit_criterion_weight=weight)
    out = model(x)
    (ta, za), (ts, zs) = out
    total, action_logit, ld = crit(out, (None, teacher), y)
    assert action_logit is za
    model.zero_grad()
    total.backward()
    grads = {n: p.grad.detach() for n, p in model.named_parameters()}
    # ---- multitask_ref against the reference
    cfg = ref_cpu.SlotViTConfig(all_frames=CFG["all_frames"])
    P = {n: p.detach().clone().requires_grad_(True) for n, p in model.named_parameters()}
    (ota, oza), (ots, ozs) = mr.forward(P, cfg, x)
    ototal, oaction, ologit = mr.train_loss(oza, ozs, teacher, y, SMOOTHING, "KL", unified, CFG["num_classes"], weight)
    ototal.backward()
    checks = {"action_token": mg.rel_err(ota, ta), "scene_token": mg.rel_err(ots, ts), "action_logits": mg.rel_err(oza, za), "scene_logits": mg.rel_err(ozs, zs),
              "loss": mg.rel_err(ototal, total), "action_loss": abs(float(oaction.detach()) - ld["action_loss"]) / abs(ld["action_loss"]),
              "logit_loss": abs(float(ologit.detach()) - ld["logit_loss"]) / abs(ld["logit_loss"])}
    checks.update({"d" + n: mg.rel_err(P[n].grad, grads[n]) for n in names})
    worst = sorted(checks.items(), key=lambda kv: -kv[1])[:4]
    print(f"[{tag}_t8] multitask_ref vs reference, worst: " + ", ".join(f"{k}={v:.1e}" for k, v in worst))
    assert max(checks.values()) < 2e-5, worst
    fx = {
        "config": np.array(repr(dict(CFG, unified_head=unified))), "batch": np.array(B), "smoothing": np.array(SMOOTHING), "logit_criterion": np.array("KL"),
        "logit_criterion_weight": np.array(weight), "teacher": teacher.numpy(),
        "action_token": ta.detach().numpy(), "scene_token": ts.detach().numpy(), "action_logits": za.detach().numpy(), "scene_logits": zs.detach().numpy(),
        "loss": np.array(float(total.detach().double())), "action_loss": np.array(ld["action_loss"]), "logit_loss": np.array(ld["logit_loss"]),
        "param_names": np.array(names),
        "grad_norms": np.array([float(grads[n].double().norm()) for n in names], dtype=np.float64),
        "grad_samples": np.stack([grads[n].reshape(-1)[torch.from_numpy(mg.sample_idx(n, grads[n].numel()))].numpy() for n in names]),
    }
    path = os.path.join(GOLD, f"{tag}_t8.npz")
    np.savez_compressed(path, **fx)
    print(f"[{tag}_t8] wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB) loss={float(total.detach()):.9f} "
          f"(action {ld['action_loss']:.6f}, logit {ld['logit_loss']:.6f}), {len(names)} parameters")


def generate_loss(TrainLoss):
    fx, worst_all = {"cases": []}, 0.0
    for i, (b, ca, cs) in enumerate(LOSS_SHAPES):
        for unified in (False, True):
            g = torch.Generator().manual_seed(500 + 10 * i + int(unified))
            wa, ws = (ca + cs, ca + cs) if unified else (ca, cs)
            za0 = torch.randn((b, wa), generator=g) * LOSS_STD
            zs0 = torch.randn((b, ws), generator=g) * LOSS_STD
            teacher = torch.randn((b, cs), generator=g) * LOSS_STD
            top = float(teacher[0].max()) + 1.0
            teacher[0, min(3, cs - 1)] = top          # a duplicated maximum in row 0: argmax takes the FIRST of the two
            teacher[0, 1] = top
            y = torch.randint(0, ca, (b,), generator=g)
            for crit_name in ("KL", "CE"):
                key = f"{crit_name}.{'unified' if unified else 'separate'}.B{b}_Ca{ca}_Cs{cs}"
                za, zs = za0.clone().requires_grad_(True), zs0.clone().requires_grad_(True)
                crit = TrainLoss(lambda z, t: mr.label_smoothing_ce(z, t, SMOOTHING), crit_name, unified_head=unified, num_action_classes=ca,
                                 logit_criterion_weight=LOSS_WEIGHT)
                total, _, ld = crit(((None, za), (None, zs)), (None, teacher), y)
                total.backward()
                oza, ozs = za0.clone().requires_grad_(True), zs0.clone().requires_grad_(True)
                ototal, oaction, ologit = mr.train_loss(oza, ozs, teacher, y, SMOOTHING, crit_name, unified, ca, LOSS_WEIGHT)
                ototal.backward()
                errs = [mg.rel_err(ototal, total), abs(float(oaction.detach()) - ld["action_loss"]) / abs(ld["action_loss"]), abs(float(ologit.detach()) - ld["logit_loss"]) / abs(ld["logit_loss"]),
                        mg.rel_err(oza.grad, za.grad), mg.rel_err(ozs.grad, zs.grad)]
                worst_all = max(worst_all, max(errs))
                assert max(errs) < 2e-5, (key, errs)
                fx["cases"].append(key)
                fx.update({key + ".action_logit": za0.numpy(), key + ".scene_logit": zs0.numpy(), key + ".teacher": teacher.numpy(), key + ".target": y.numpy(),
                           key + ".losses": np.array([float(total.detach().double()), ld["action_loss"], ld["logit_loss"]], dtype=np.float64),
                           key + ".d_action_logit": za.grad.numpy(), key + ".d_scene_logit": zs.grad.numpy()})
    fx["cases"] = np.array(fx["cases"])
    fx["smoothing"], fx["logit_criterion_weight"] = np.array(SMOOTHING), np.array(LOSS_WEIGHT)
    path = os.path.join(GOLD, "multitask_loss.npz")
    np.savez_compressed(path, **fx)
    print(f"[multitask_loss] multitask_ref.train_loss vs the driver's TrainLoss, worst {worst_all:.1e}; wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB), "
          f"{len(fx['cases'])} cases")


def generate_keys(reg):
    out = {}
    for tag, unified, _ in MODES:
        m = reg["disentangle_vit_base_patch16_224"](unified_head=unified, num_classes=400, all_frames=16, tubelet_size=2)
        out[tag] = {"state_dict": {k: list(v.shape) for k, v in m.state_dict().items()}, "named_parameters": [n for n, _ in m.named_parameters()],
                    "pos_embed": list(m.pos_embed.shape), "no_weight_decay": sorted(m.no_weight_decay())}
    sig = inspect.signature(reg["disentangle_vit_base_patch16_224"].__globals__["VisionTransformer"].__init__)
    out["defaults"] = {k: (v.default if isinstance(v.default, (int, float, bool, str, type(None))) else repr(v.default)) for k, v in sig.parameters.items()
                       if k != "self" and v.default is not inspect.Parameter.empty}
    json.dump(out, open(os.path.join(GOLD, "multitask_state_dict_keys.json"), "w"))
    print("[multitask keys]", {k: len(v["state_dict"]) for k, v in out.items() if k != "defaults"}, out["defaults"])


def generate_optim(reg, rof):
    out = {"groups": {}}
    for tag, unified, _ in MODES:
        m = build(reg, unified)
        nl = m.get_num_layers()
        for dtag, decay in (("ld0.75", 0.75), ("flat", 1.0)):
            assigner = rof.LayerDecayValueAssigner([decay ** (nl + 1 - i) for i in range(nl + 2)]) if decay < 1.0 else None
            with contextlib.redirect_stdout(io.StringIO()) as buf:
                rof.get_parameter_groups(m, 0.05, m.no_weight_decay(), assigner.get_layer_id if assigner else None, assigner.get_scale if assigner else None)
            txt = buf.getvalue()
            groups = json.loads(txt[txt.index("{"):])
            out["groups"][f"{tag}.{dtag}"] = {"num_layers": nl, "layer_decay": decay, "weight_decay": 0.05, "unified_head": unified,
                                              "groups": [[k, v["weight_decay"], v["lr_scale"], v["params"]] for k, v in groups.items()]}
    json.dump(out, open(os.path.join(GOLD, "multitask_optim.json"), "w"))
    print("[multitask optim]", {k: len(v["groups"]) for k, v in out["groups"].items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=[None, "step", "loss", "keys", "optim"])
    args = ap.parse_args()
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    reg, TrainLoss, rof = install_driver()
    if args.only in (None, "keys"):
        generate_keys(reg)
    if args.only in (None, "optim"):
        generate_optim(reg, rof)
    if args.only in (None, "loss"):
        generate_loss(TrainLoss)
    if args.only in (None, "step"):
        for tag, unified, weight in MODES:
            generate_step(reg, TrainLoss, tag, unified, weight)


if __name__ == "__main__":
    main()
