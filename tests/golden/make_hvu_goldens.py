#!/usr/bin/env python3
"""Generate the HVU-recipe fixtures by RUNNING THE REAL REFERENCE (build container only):

  hvu_loss.npz      utils/loss/hvu_train_loss.py TrainLoss on seeded student outputs, S in {2, 3, 4}, both scene criteria, 739 + 248 classes
  vitb_t8_hvu.npz   one fp32 step of the reference model (num_classes=739, num_scene_classes=248, 8 frames, B = 2) under that loss,
                    in the format of make_goldens.generate() (golden_util.load / check_against_golden read it unchanged)
  fame_hvu_t8.npz   utils/transform/fame_hvu.py FAME on the inputs, `rand` and `perm` of fame_t8.npz

While generating, tests/hvu_ref.py (the plain-PyTorch restatement the tests use at other shapes) is checked against the reference on the
same data; a mismatch aborts.  The fixtures are data only.

Usage (in the build container):  python tests/golden/make_hvu_goldens.py [--only loss|step|fame]
This script never runs on the GPU box and nothing under tests/ imports it.
"""
from __future__ import annotations

import argparse
import itertools
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
import make_goldens as mg  # noqa: E402  (puts the repository root and tests/ on sys.path)

from devias_amd import synth  # noqa: E402
from oracle import ref_cpu  # noqa: E402
import hvu_ref  # noqa: E402

ROOT = mg.ROOT
NB, NS = 739, 248          # run_slot_finetuning_hvu.py:35-36


def install_hvu_reference():
    ref = mg.install_reference()
    # utils/loss/hvu_train_loss.py:6 imports its two constants from the whole training driver: stand in for that module
    drv = types.ModuleType("run_slot_finetuning_hvu")
    drv.HVU_NUM_ACTION_CLASSES, drv.HVU_NUM_SCENE_CLASSES = NB, NS
    sys.modules["run_slot_finetuning_hvu"] = drv
    # TrainLoss force-casts the fg masks to fp16 (hvu_train_loss.py:75-76) which breaks fp32 backward;
    # masks are k/256 (exact in fp16) so making .half() the identity is value-preserving (SURVEY §8c caveat 1)
    torch.Tensor.half = lambda self: self
    from utils.loss.hvu_train_loss import TrainLoss
    assert TrainLoss(None, "CE").num_action_classes == NB and TrainLoss(None, "CE").num_scene_classes == NS
    return ref, TrainLoss


def assignment_gap(Z, ya, ys, B, S):
    """per sample: the best ordered slot pair and the relative gap of its cost to the runner-up's"""
    p = Z.float().softmax(-1).view(B, S, -1)
    out, gaps = [], []
    for b in range(B):
        cs = sorted((-(p[b, i, ya[b]] + p[b, j, NB + ys[b]]).item(), i, j) for i, j in itertools.permutations(range(S), 2))
        out.append([cs[0][1], cs[0][2]])
        gaps.append((cs[1][0] - cs[0][0]) / abs(cs[0][0]) if len(cs) > 1 else float("inf"))
    return out, gaps


def generate_loss(TrainLoss):
    """The reference's HVU TrainLoss itself on seeded student outputs whose assignment is decisive (so that a bf16 run has the same match):
    randn * 2 logits with 9 planted on the action class of a chosen slot and 8 on the scene class of a chosen slot (the largest of 987 such noise values is
    about 6.5).  Odd samples choose the SAME slot for both (the assignment's conflict branch); there a second-choice scene slot gets 7, else the runner-up
    would differ only by noise."""
    fx = {}
    for S in (2, 3, 4):
        B, D, G, N, nh = 4, 768, 196, 392, 4
        g = torch.Generator().manual_seed(5100 + S)
        # values on dyadic grids finer than bf16's (1/1024 for logits of magnitude <= 9): the same tests, a fixture half the size
        q = lambda t, steps: torch.round(t * steps) / steps
        base = dict(slots_head=q(torch.randn(B * S, NB + NS, generator=g) * 2.0, 1024), slots=q(torch.randn(B * S, D, generator=g), 64),
                    maskp=q(torch.rand(B * S, G, generator=g), 256), attn=q(torch.rand(B * nh, S, N, generator=g), 256),
                    target=torch.randint(0, NB, (B,), generator=g), scene_target=torch.randint(0, NS, (B,), generator=g),
                    fg=torch.randint(0, 257, (B, G), generator=g).float() / 256.0, fgN=torch.randint(0, 257, (B, N), generator=g).float() / 256.0)
        ya, ys, Z = base["target"], base["scene_target"], base["slots_head"]
        for b in range(B):
            ia = (b + S // 2) % S
            conflict = b % 2 == 1
            js = ia if conflict else (ia + 1) % S
            Z[b * S + ia, ya[b]] = 9.0
            Z[b * S + js, NB + ys[b]] = 8.0
            if conflict:
                Z[b * S + (ia + 1) % S, NB + ys[b]] = 7.0
        match32, gaps = assignment_gap(Z, ya, ys, B, S)
        match16, gaps16 = assignment_gap(Z.bfloat16(), ya, ys, B, S)
        print(f"[hvu_loss S={S}] match {match32}, relative cost gap to the runner-up: fp32 min {min(gaps):.3f}, bf16-rounded logits min {min(gaps16):.3f}")
        assert min(gaps) >= 1e-2 and min(gaps16) >= 1e-2 and match16 == match32, (gaps, gaps16, match32, match16)
        for k, v in base.items():
            fx[f"s{S}.{k}"] = v.numpy()
        totals, first = {}, None
        for crit_name in ("KL", "CE"):
            leaves = {k: base[k].clone().requires_grad_(True) for k in ("slots_head", "slots", "maskp", "attn")}
            out = (None, (None, None, leaves["attn"]), (leaves["slots_head"], leaves["slots"], leaves["maskp"]))
            crit = TrainLoss(criterion=None, scene_criterion=crit_name, slot_matching_method="matching",
                             mask_prediction_loss_weight=1.0, mask_distill_loss_weight=3.0)
            ys_in = base["scene_target"].clone()               # the reference offsets its argument in place (hvu_train_loss.py:45-46)
            total, logits, ld = crit(out, base["target"], ys_in, fg_mask=(base["fg"], base["fgN"]))
            assert torch.equal(ys_in, base["scene_target"] + NB)
            total.backward()
            ol = {k: base[k].clone().requires_grad_(True) for k in leaves}
            oout = (None, (None, None, ol["attn"]), (ol["slots_head"], ol["slots"], ol["maskp"]))
            ys_keep = base["scene_target"].clone()
            ototal, ologits, old, oidx = hvu_ref.hvu_train_loss(oout, base["target"], ys_keep, (base["fg"], base["fgN"]), num_action_classes=NB,
                                                                scene_criterion=crit_name, mask_prediction_loss_weight=1.0, mask_distill_loss_weight=3.0)
            assert torch.equal(ys_keep, base["scene_target"])
            ototal.backward()
            errs = {"total": mg.rel_err(ototal, total), "logits": mg.rel_err(ologits, logits)}
            errs.update({"d" + k: mg.rel_err(ol[k].grad, leaves[k].grad) for k in leaves})
            errs.update({k: abs(old[k] - ld[k]) / max(abs(ld[k]), 1e-30) for k in ld})
            print(f"[hvu_loss S={S} {crit_name}] hvu_ref vs reference: " + ", ".join(f"{k}={v:.1e}" for k, v in errs.items()), ld)
            assert max(errs.values()) < 2e-6, errs
            match = np.stack([oidx[0].numpy(), oidx[1].numpy()], axis=1)
            assert match.tolist() == match32
            Zv = base["slots_head"].view(B, S, -1)
            assert [int(torch.argmin((Zv[b] - logits[b]).abs().sum(-1))) for b in range(B)] == match[:, 0].tolist()      # the rows the reference returned
            pre = f"s{S}.{crit_name}."
            totals[crit_name] = float(total.detach().double())
            fx[pre + "total"] = np.array(totals[crit_name])
            fx[pre + "losses"] = np.array([float(ld[k]) for k in hvu_ref.LOSS_NAMES])
            fx[pre + "match"] = match
            # against a one-hot target the two criteria are the same arithmetic: matched logits and gradients are stored once per S
            got = dict({"d" + k: leaves[k].grad for k in leaves}, logits=logits.detach())
            if first is None:
                first = got
                for k, v in got.items():
                    fx[f"s{S}.{k}"] = v.numpy()
            else:
                err = {k: mg.rel_err(got[k], first[k]) for k in got}
                print(f"[hvu_loss S={S}] 'CE' against 'KL' (logits, gradients): " + ", ".join(f"{k}={v:.1e}" for k, v in err.items()))
                assert max(err.values()) <= 1e-6, err
        assert abs(totals["KL"] - totals["CE"]) <= 1e-6 * abs(totals["CE"]), totals
    path = os.path.join(ROOT, "tests", "golden", "hvu_loss.npz")
    np.savez_compressed(path, **fx)
    print(f"[hvu_loss] wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)")


STEP_NAME, STEP_CFG, STEP_B = "vitb_t8_hvu", dict(all_frames=8, num_classes=NB, num_scene_classes=NS), 2


def generate_step(ref, TrainLoss):
    """make_goldens.generate() with the HVU loss: weights and inputs are devias_amd.synth formulae, scene labels synth.scene_targets"""
    reg, ms, mf, AggregationBlock, _ = ref
    name, B = STEP_NAME, STEP_B
    cfg = ref_cpu.SlotViTConfig(**STEP_CFG)
    torch.manual_seed(0)
    model = mg.build_reference_student(cfg, reg, ms, AggregationBlock)
    model.train()
    synth.fill_module_(model, seed=0)
    names = [n for n, _ in model.named_parameters()]
    shapes = ref_cpu.param_shapes(cfg)
    assert names == list(shapes.keys()) and all(tuple(p.shape) == shapes[n] for n, p in model.named_parameters())
    assert tuple(model.head.weight.shape) == (NB + NS, cfg.embed_dim)
    x = synth.video(B, cfg.all_frames, cfg.img_size, seed=1000)
    y = synth.targets(B, NB, seed=1000)
    ys = synth.scene_targets(B, NS, seed=1000)
    fg = synth.fg_masks(B, cfg.num_patches, cfg.grid * cfg.grid, seed=1000)
    taps = {}
    model.blocks[0].register_forward_hook(lambda m, i, o: taps.__setitem__("block0", o.detach()))
    model.blocks[-1].register_forward_hook(lambda m, i, o: taps.__setitem__(f"block{cfg.depth - 1}", o.detach()))
    model.norm.register_forward_hook(lambda m, i, o: taps.__setitem__("feats", o.detach()))
    crit = TrainLoss(criterion=None, scene_criterion="KL", slot_matching_method="matching", mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0)
    out = model(x)
    total, logits, ld = crit(out, y, ys.clone(), fg_mask=fg)
    model.zero_grad()
    total.backward()
    (af, sf), (al, sl, attn), (slots_head, slots, maskp) = out
    grads = {n: p.grad.detach() for n, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    # ---- oracle forward + hvu_ref loss vs the reference on identical data
    Pg = {k: v.clone().requires_grad_(True) for k, v in synth.fill_params(shapes, seed=0).items()}
    oout = ref_cpu.student_forward(Pg, cfg, x, {}, None)
    ototal, ologits, old, oidx = hvu_ref.hvu_train_loss(oout, y, ys, fg, num_action_classes=NB)
    ototal.backward()
    checks = {"slots_head": mg.rel_err(oout[2][0], slots_head), "slots": mg.rel_err(oout[2][1], slots), "mask_predictions": mg.rel_err(oout[2][2], maskp),
              "attn": mg.rel_err(oout[1][2], attn), "action_logit": mg.rel_err(oout[1][0], al), "scene_logit": mg.rel_err(oout[1][1], sl),
              "total": mg.rel_err(ototal, total), "logits": mg.rel_err(ologits, logits)}
    for k in ld:
        checks["loss." + k] = abs(old[k] - ld[k]) / max(abs(ld[k]), 1e-30)
    gmax = max(float(g.abs().max()) for g in grads.values())
    gerr = {n: float((Pg[n].grad.double() - grads[n].double()).abs().max() / max(float(grads[n].abs().max()), 1e-6 * gmax)) for n in names}
    checks["grads(worst)"] = max(gerr.values())
    print(f"[{name}] oracle + hvu_ref vs reference: " + ", ".join(f"{k}={v:.2e}" for k, v in checks.items()))
    bad = {k: v for k, v in checks.items() if v > (1e-3 if k.startswith("grads") else 5e-5)}
    assert not bad, f"oracle disagrees with the reference: {bad}"
    Z = slots_head.view(B, cfg.num_latents, -1)
    assert [int(torch.argmin((Z[b] - logits[b]).abs().sum(-1))) for b in range(B)] == oidx[0].tolist()
    fx = {
        "config": np.array(repr(STEP_CFG)), "batch": np.array(B),
        "slots_head": slots_head.detach().numpy(), "slots": slots.detach().numpy(),
        "mask_predictions": maskp.detach().numpy(), "attn": attn.detach().numpy(),
        "action_feat": af.detach().numpy(), "scene_feat": sf.detach().numpy(),
        "action_logit": al.detach().numpy(), "scene_logit": sl.detach().numpy(),
        "matched_logits": logits.detach().numpy(),
        "match_action_slot": oidx[0].numpy(), "match_scene_slot": oidx[1].numpy(),
        "total_loss": np.array(float(total.detach().double())),
        "loss_names": np.array(list(ld.keys())), "loss_values": np.array([float(ld[k]) for k in ld], dtype=np.float64),
        "param_names": np.array(names),
        "grad_norms": np.array([float(grads[n].double().norm()) for n in names], dtype=np.float64),
        "grad_samples": np.stack([grads[n].reshape(-1)[torch.from_numpy(mg.sample_idx(n, grads[n].numel()))].numpy() for n in names]),
        "tap_names": np.array(sorted(taps.keys())),
        "taps": np.stack([mg.tap_summary(taps[k]) for k in sorted(taps.keys())]),
    }
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **fx)
    print(f"[{name}] wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB) total_loss={float(total):.9f} {ld}")


def generate_fame():
    """utils/transform/fame_hvu.py FAME, run like make_goldens.generate_fame runs fame.py (oracle/fame_cpu.py's restatements of the two kornia
    functions injected as the `kornia` module, the two random draws replaced by fixed tensors), on the inputs of fame_t8.npz"""
    from oracle import fame_cpu

    class _Blur(nn.Module):
        def __init__(self, ks, sg):
            super().__init__()
            self.ks, self.sg = ks, sg

        def forward(self, x):
            return fame_cpu.gaussian_blur2d(x, self.ks[0], self.sg[0])

    def _mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    _mod("kornia", filters=_mod("kornia.filters", GaussianBlur2d=_Blur), color=_mod("kornia.color", rgb_to_hsv=fame_cpu.rgb_to_hsv))
    _mod("kornia.augmentation"); _mod("kornia.augmentation.container", VideoSequential=object)
    _mod("torchvision", transforms=_mod("torchvision.transforms")); _mod("torchvision.datasets")
    _mod("torchvision.datasets.video_utils", VideoClips=object)
    sys.path.insert(0, mg.REF)
    import utils.transform.fame_hvu as rfh
    t8 = dict(np.load(os.path.join(ROOT, "tests", "golden", "fame_t8.npz")))
    cases = {"fame_hvu_t8": (t8, True)}
    t16 = dict(np.load(os.path.join(ROOT, "tests", "golden", "fame_t16_all.npz")))
    cases["(fame_t16_all inputs, prob_aug = 1: checked, not committed)"] = (t16, False)
    for name, (src, commit) in cases.items():
        B, T, size, beta, prob = int(src["B"]), int(src["T"]), int(src["size"]), float(src["beta"]), float(src["prob_aug"])
        x = synth.scene_video(B, T, size)
        action = torch.from_numpy(src["label"])
        scene = torch.arange(B) * 5 + 2
        perm_t, rand_t = torch.from_numpy(src["perm"]), torch.from_numpy(src["rand"])
        model = rfh.FAME(beta=beta, prob_aug=prob)
        orig = (torch.randperm, torch.rand)
        torch.randperm = lambda n, device=None: perm_t
        torch.rand = lambda n: rand_t
        try:
            with torch.no_grad():
                vids, a_out, s_out, (m, mpf) = model(x.clone(), action, scene)
        finally:
            torch.randperm, torch.rand = orig
        assert np.array_equal(m.numpy(), src["mask"]) and np.array_equal(mpf.numpy(), src["masks_per_frame"]), name     # bit for bit fame.py's masks
        assert np.array_equal(a_out.numpy(), src["out_label"]), name
        assert np.array_equal(vids.flatten()[torch.from_numpy(src["video_sample_idx"])].numpy(), src["video_sample"]), name
        # the restatements the tests use: hvu_ref's routing, and the routing of devias_amd.fame on hvu_ref's (src, partner, aug) table
        oa, os_ = hvu_ref.fame_hvu_labels(action, scene, perm_t, rand_t, prob)
        assert torch.equal(oa, a_out) and torch.equal(os_, s_out), name
        from devias_amd.fame import route_hvu_labels
        ra, rs = route_hvu_labels(action, scene, *hvu_ref.fame_route_table(perm_t, rand_t, prob), prob)
        assert torch.equal(ra, a_out) and torch.equal(rs, s_out), name
        print(f"[{name}] reference == hvu_ref == devias_amd.fame.route_hvu_labels; scene labels {scene.tolist()} -> {s_out.tolist()}")
        if commit:
            np.savez_compressed(os.path.join(ROOT, "tests", "golden", name + ".npz"),
                                B=B, T=T, size=size, beta=beta, prob_aug=prob, rand=src["rand"], perm=src["perm"],
                                action_label=action.numpy(), scene_label=scene.numpy(), out_action_label=a_out.numpy(), out_scene_label=s_out.numpy(),
                                mask=m.numpy(), masks_per_frame=mpf.numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=[None, "loss", "step", "fame"])
    args = ap.parse_args()
    torch.set_num_threads(os.cpu_count() or 8)
    ref, TrainLoss = install_hvu_reference()
    if args.only in (None, "loss"):
        generate_loss(TrainLoss)
    if args.only in (None, "step"):
        generate_step(ref, TrainLoss)
    if args.only in (None, "fame"):
        generate_fame()


if __name__ == "__main__":
    main()
