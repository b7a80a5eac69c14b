#!/usr/bin/env python3
"""Generate the mixup / cutmix fixtures by RUNNING THE REAL REFERENCE (build container only):

  mixup_vectors.npz            utils/transform/mixup.py's Mixup on small CPU clips: per case the numpy seed, the input clip and labels, the reference's output clip and
                               soft target, and the table it drew -- lam per clip, use_cutmix and the boxes, captured by wrapping cutmix_bbox_and_lam, the two
                               _params_* methods and mixup_target.  The three modes; mixup only, cutmix only, both, cutmix_minmax = (0.2, 0.8); prob 1 and 0.5;
                               mixup_enabled False; label_smoothing 0 and 0.1; fp32 and bf16 clips; [B, C, T, H, W] from B in {2, 4, 6} and (C, T, H, W) in
                               {(3, 2, 8, 8), (3, 2, 10, 14), (1, 1, 5, 7)}.  The script asserts that the set holds a box touching each border, an empty box
                               (the corrected lam becomes 1) and a pair whose two clips differ in kind.
  plainvit_mean_mixup_t8.npz   plainvit_mean_t8.npz's fp32 step of the reference's vit_base_patch16_224 under batch-mode Mixup(0.8, 1.0, label_smoothing=0.1,
                               num_classes=365) with a recorded seed and timm's SoftTargetCrossEntropy (restated here: timm is not importable in the build
                               container); make_goldens.generate's format plus the seed and the soft target.

'pair' mode on video clips: the reference's `x[i][:, yl:yh, xl:xh]` (mixup.py:187-188) is written for [C, H, W] images; on a [C, T, H, W] clip it would cut frames
yl:yh and rows xl:xh.  The box belongs to the H x W plane, as in the other two modes, so in 'pair' mode the reference is handed the [B, C*T, H, W] view of the same
storage: the same draws (only the last two dimensions are read), the box applied where 'elem' and 'batch' mode apply it.
The reference spells numpy's boolean type `np.bool`, which numpy 2 no longer has: the script restores the alias before it imports the module.

Usage (in the build container):  python tests/golden/make_mixup_goldens.py [--only vectors|step]
This script never runs on the GPU box and nothing under tests/ imports it.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_goldens as mg  # noqa: E402  (puts the repository root and tests/ on sys.path)

from devias_amd import synth  # noqa: E402

ROOT = mg.ROOT
SHAPES = ((3, 2, 8, 8), (3, 2, 10, 14), (1, 1, 5, 7))
BATCHES = (2, 4, 6)
CONFIGS = (("mixup", dict(mixup_alpha=0.8, cutmix_alpha=0.0)), ("cutmix", dict(mixup_alpha=0.0, cutmix_alpha=1.0)), ("both", dict(mixup_alpha=0.8, cutmix_alpha=1.0)),
           ("minmax", dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8))))
MODES = ("batch", "pair", "elem")
NUM_CLASSES = 11
STEP_SEED = 7


def load_reference_mixup():
    if not hasattr(np, "bool"):
        np.bool = bool
    spec = importlib.util.spec_from_file_location("reference_mixup", os.path.join(mg.REF, "utils", "transform", "mixup.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_reference(rm, case, seed):
    """one call of the reference's Mixup -> dict of arrays (the fixture's entries for this case)"""
    B, shape, dtype = case["B"], case["shape"], torch.bfloat16 if case["dtype"] == "bf16" else torch.float32
    g = torch.Generator().manual_seed(1000 + seed)
    x0 = torch.randn((B,) + shape, generator=g).to(dtype)
    y = torch.randint(0, NUM_CLASSES, (B,), generator=g)
    m = rm.Mixup(prob=case["prob"], mode=case["mode"], label_smoothing=case["smoothing"], num_classes=NUM_CLASSES, **case["kw"])
    m.mixup_enabled = case["enabled"]
    log = {"boxes": [], "params": None, "lam": None}
    orig_box, orig_target = rm.cutmix_bbox_and_lam, rm.mixup_target
    orig_elem, orig_batch = m._params_per_elem, m._params_per_batch

    def box(*a, **k):
        out = orig_box(*a, **k)
        log["boxes"].append(([int(v) for v in out[0]], float(out[1])))
        return out

    def params_elem(n):
        lam, cut = orig_elem(n)
        log["params"] = (np.array(lam, dtype=np.float32).copy(), np.array(cut, dtype=bool).copy())
        return lam, cut

    def params_batch():
        lam, cut = orig_batch()
        log["params"] = (np.full(B, lam, dtype=np.float64), np.full(B, bool(cut)))
        return lam, cut

    def target(t, nc, lam=1., smoothing=0.0, device="cpu"):
        log["lam"] = lam
        return orig_target(t, nc, lam, smoothing, device)

    rm.cutmix_bbox_and_lam, rm.mixup_target, m._params_per_elem, m._params_per_batch = box, target, params_elem, params_batch
    try:
        np.random.seed(seed)
        x = x0.clone()
        xin = x.view(B, shape[0] * shape[1], shape[2], shape[3]) if case["mode"] == "pair" else x
        xo, t = m(xin, y)
        assert xo.data_ptr() == x.data_ptr()
    finally:
        rm.cutmix_bbox_and_lam, rm.mixup_target = orig_box, orig_target
    lam_drawn, cut = log["params"]
    n = len(lam_drawn)
    kind, boxes, k = np.zeros(B, dtype=np.int32), np.zeros((B, 4), dtype=np.int32), 0
    for i in range(n):
        if lam_drawn[i] != 1.:
            kind[i] = 2 if cut[i] else 1
            if cut[i] and (case["mode"] != "batch" or i == 0):
                boxes[i] = log["boxes"][k][0]
                k += 1
            elif cut[i]:
                boxes[i] = boxes[0]
    assert k == len(log["boxes"])
    lam_drawn = np.asarray(lam_drawn, dtype=np.float64)
    if case["mode"] == "pair":
        kind[B // 2:], boxes[B // 2:] = kind[:B // 2][::-1], boxes[:B // 2][::-1]
        lam_drawn, cut = np.concatenate((lam_drawn, lam_drawn[::-1])), np.concatenate((cut, cut[::-1]))
    lam_t = log["lam"]
    lam_target = lam_t.float().reshape(-1).numpy().astype(np.float64) if isinstance(lam_t, torch.Tensor) else np.full(B, float(lam_t), dtype=np.float64)
    return {"seed": np.array(seed), "x": x0.float().numpy(), "y": y.numpy(), "out_x": x.float().numpy(), "out_target": t.numpy(), "kind": kind,
            "use_cutmix": np.asarray(cut, dtype=bool), "lam_drawn": lam_drawn, "lam_target": lam_target, "boxes": boxes}


def properties(case, r):
    """what a case contributes to the coverage the set must have"""
    H, W = case["shape"][-2:]
    p = set()
    B = case["B"]
    for i in range(B):
        if r["kind"][i] == 2:
            yl, yh, xl, xh = (int(v) for v in r["boxes"][i])
            if yl == yh or xl == xh:
                p.add("empty_box")
                assert r["lam_target"][i] == 1.0
            else:
                p |= {n for n, hit in (("top", yl == 0), ("bottom", yh == H), ("left", xl == 0), ("right", xh == W)) if hit}
                if 0 < yl and yh < H and 0 < xl and xh < W:
                    p.add("inner_box")
        if r["kind"][i] == 0 and case["enabled"]:
            p.add("unmixed_clip")
        if r["kind"][i] != r["kind"][B - 1 - i]:
            p.add("pair_differs_in_kind")
        if r["kind"][i] == 2 and r["kind"][B - 1 - i] == 2 and not np.array_equal(r["boxes"][i], r["boxes"][B - 1 - i]):
            p.add("pair_differs_in_box")
    return p


def generate_vectors():
    rm = load_reference_mixup()
    cases = []
    k = 0
    for mode in MODES:
        for tag, kw in CONFIGS:
            for dtype in ("fp32", "bf16"):
                cases.append(dict(mode=mode, tag=tag, kw=kw, dtype=dtype, shape=SHAPES[k % 3], B=BATCHES[(k // 3 + k) % 3], smoothing=(0.1, 0.0)[k % 2],
                                  prob=0.5 if k % 4 == 3 else 1.0, enabled=True, want=None))
                k += 1
    for i, mode in enumerate(MODES):          # mixing switched off by the training loop
        cases.append(dict(mode=mode, tag="both", kw=CONFIGS[2][1], dtype="fp32", shape=SHAPES[i], B=BATCHES[i], smoothing=0.1, prob=1.0, enabled=False, want=None))
    # cases whose seed is searched for one property, so that the set has it whatever the first draws gave
    for want, mode, tag, dtype, shape, B, prob in (
            ("empty_box", "batch", "cutmix", "fp32", SHAPES[2], 2, 1.0), ("empty_box", "elem", "cutmix", "bf16", SHAPES[2], 4, 1.0),
            ("pair_differs_in_kind", "elem", "both", "fp32", SHAPES[1], 4, 1.0), ("pair_differs_in_kind", "elem", "both", "bf16", SHAPES[0], 6, 0.5),
            ("inner_box", "pair", "cutmix", "bf16", SHAPES[1], 4, 1.0), ("top", "batch", "cutmix", "bf16", SHAPES[0], 4, 1.0),
            ("bottom", "elem", "cutmix", "fp32", SHAPES[0], 2, 1.0), ("left", "pair", "both", "fp32", SHAPES[2], 6, 1.0), ("right", "elem", "cutmix", "fp32", SHAPES[1], 6, 1.0),
            ("unmixed_clip", "elem", "mixup", "bf16", SHAPES[2], 6, 0.5), ("unmixed_clip", "batch", "both", "fp32", SHAPES[1], 2, 0.5)):
        cases.append(dict(mode=mode, tag=tag, kw=dict(CONFIGS)[tag], dtype=dtype, shape=shape, B=B, smoothing=0.1, prob=prob, enabled=True, want=want))
    fx, seen, names = {}, set(), []
    for ci, case in enumerate(cases):
        for seed in range(100 * ci, 100 * ci + 100):
            r = run_reference(rm, case, seed)
            p = properties(case, r)
            if case["want"] is None or case["want"] in p:
                break
        else:
            raise AssertionError(f"no seed gives {case['want']} for case {ci}")
        seen |= p
        name = f"c{ci:02d}"
        names.append(name)
        cfg = {k: case[k] for k in ("mode", "tag", "dtype", "shape", "B", "smoothing", "prob", "enabled")}
        cfg["kw"] = dict(case["kw"])
        fx[name + ".config"] = np.array(repr(cfg))
        for key, v in r.items():
            fx[f"{name}.{key}"] = v
    need = {"top", "bottom", "left", "right", "inner_box", "empty_box", "pair_differs_in_kind", "pair_differs_in_box", "unmixed_clip"}
    assert need <= seen, need - seen
    fx["cases"] = np.array(names)
    fx["num_classes"] = np.array(NUM_CLASSES)
    path = os.path.join(ROOT, "tests", "golden", "mixup_vectors.npz")
    np.savez_compressed(path, **fx)
    print(f"[mixup_vectors] {len(names)} cases, coverage {sorted(seen)}, wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


def soft_target_ce(logits, target):
    """timm.loss.SoftTargetCrossEntropy"""
    return torch.sum(-target * torch.nn.functional.log_softmax(logits, dim=-1), dim=-1).mean()


def generate_step():
    import make_plainvit_goldens as mp
    rm = load_reference_mixup()
    reg = mg.install_reference()[0]
    torch.manual_seed(0)
    model = mp.build(reg, True)
    model.train()
    synth.fill_module_(model, seed=0)
    names = [n for n, _ in model.named_parameters()]
    x = synth.video(mp.B, mp.CFG["all_frames"], 224, seed=1000)
    y = synth.targets(mp.B, mp.CFG["num_classes"], seed=1000)
    mix = rm.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=mp.SMOOTHING, num_classes=mp.CFG["num_classes"])
    np.random.seed(STEP_SEED)
    x, t = mix(x, y)
    assert not torch.equal(x, synth.video(mp.B, mp.CFG["all_frames"], 224, seed=1000)), "the recorded seed must mix the batch"
    token, logits = model(x)
    loss = soft_target_ce(logits, t)
    model.zero_grad()
    loss.backward()
    grads = {n: p.grad.detach() for n, p in model.named_parameters()}
    fx = {
        "config": np.array(repr(dict(mp.CFG, use_mean_pooling=True))), "batch": np.array(mp.B), "smoothing": np.array(mp.SMOOTHING), "mixup_seed": np.array(STEP_SEED),
        "mixup": np.array(repr(dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode="batch"))), "soft_target": t.numpy(),
        "token": token.detach().numpy(), "logits": logits.detach().numpy(), "loss": np.array(float(loss.detach().double())),
        "param_names": np.array(names),
        "grad_norms": np.array([float(grads[n].double().norm()) for n in names], dtype=np.float64),
        "grad_samples": np.stack([grads[n].reshape(-1)[torch.from_numpy(mg.sample_idx(n, grads[n].numel()))].numpy() for n in names]),
    }
    path = os.path.join(ROOT, "tests", "golden", "plainvit_mean_mixup_t8.npz")
    np.savez_compressed(path, **fx)
    print(f"[plainvit_mean_mixup_t8] wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB) loss={float(loss.detach()):.9f}, {len(names)} parameters")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=[None, "vectors", "step"])
    args = ap.parse_args()
    torch.set_num_threads(min(os.cpu_count() or 8, 32))
    if args.only in (None, "vectors"):
        generate_vectors()
    if args.only in (None, "step"):
        generate_step()


if __name__ == "__main__":
    main()
