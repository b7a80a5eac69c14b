"""The bounds of tests/multitask_loss_bounds.py proven without a GPU (the float64 reference is torch's own kl_div / cross_entropy on the materialised pad; the CPU
emulation stays under HALF the slack; every seeded mutant exceeds a bound), and tests/multitask_ref.train_loss against the fixture the driver's TrainLoss wrote
(tests/golden/multitask_loss.npz)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import multitask_loss_bounds as lb
import multitask_ref as mr

DTYPES = (torch.float32, torch.bfloat16)
FX = dict(np.load(gu.GOLDEN_DIR + "/multitask_loss.npz", allow_pickle=False))


def _all():
    for B, C, pad in lb.CASES:
        for mode in lb.MODES:
            for dtype in DTYPES:
                yield B, C, pad, mode, dtype


def test_reference_is_torchs_own_loss_on_the_materialised_pad():
    for B, C, pad, mode, dtype in _all():
        I = lb.inputs(B, C, pad, dtype)
        ref, _ = lb.bounds(I, mode, dtype)
        z = I["z"].double().requires_grad_(True)
        want = mr.distill(z, I["t"].double(), mode, pad, I["w"])
        (want * float(I["g"])).backward()
        assert abs(float(ref["loss"]) - float(want.detach())) <= 1e-12 * abs(float(want.detach())), (B, C, pad, mode)
        assert float((ref["dz"] - z.grad).abs().max()) <= 1e-13, (B, C, pad, mode)
        # the tie: the one-hot of row 0 sits on the FIRST of the two maxima
        if mode == "CE":
            hot = int(torch.argmin(ref["dz"][0] / float(I["g"])))
            assert hot == pad + I["first"] and I["t"][0, I["first"]] == I["t"][0].max() and int((I["t"][0] == I["t"][0].max()).sum()) == 2


def test_emulation_stays_under_half_of_the_slack(capsys):
    worst = {}
    for B, C, pad, mode, dtype in _all():
        I = lb.inputs(B, C, pad, dtype)
        ref, bnd = lb.bounds(I, mode, dtype)
        for k, r in lb.ratios(lb.emulate(I, mode, dtype), ref, bnd).items():
            key = (k, mode, "bf16" if dtype == torch.bfloat16 else "fp32")
            worst[key] = max(worst.get(key, 0.0), r * lb.SLACK)
            assert r <= 0.5, (B, C, pad, mode, dtype, k, r)
    with capsys.disabled():
        for key in sorted(worst):
            print("distill emulation, worst ratio at slack 1:", key, round(worst[key], 4))


@pytest.mark.parametrize("mutant", lb.MUTANTS)
def test_every_mutant_exceeds_a_bound(mutant):
    failed = []
    for B, C, pad, mode, dtype in _all():
        I = lb.inputs(B, C, pad, dtype)
        ref, bnd = lb.bounds(I, mode, dtype)
        bad = {k: r for k, r in lb.ratios(lb.emulate(I, mode, dtype, mutant=mutant), ref, bnd).items() if r > 1.0}
        if bad:
            failed.append((B, C, pad, mode, dtype, bad))
    assert failed, f"no case tells the mutant {mutant} from the kernel: the bounds show nothing about it"


@pytest.mark.parametrize("case", [str(c) for c in FX["cases"]])
def test_restated_train_loss_matches_the_drivers(case):
    crit, head, shape = case.split(".")
    ca = int(shape.split("_")[1][2:])
    za = torch.from_numpy(FX[case + ".action_logit"]).requires_grad_(True)
    zs = torch.from_numpy(FX[case + ".scene_logit"]).requires_grad_(True)
    total, action, logit = mr.train_loss(za, zs, torch.from_numpy(FX[case + ".teacher"]), torch.from_numpy(FX[case + ".target"]), float(FX["smoothing"]), crit,
                                         head == "unified", ca, float(FX["logit_criterion_weight"]))
    total.backward()
    got = np.array([float(total.detach()), float(action.detach()), float(logit.detach())])
    assert np.abs(got - FX[case + ".losses"]).max() <= 2e-5 * np.abs(FX[case + ".losses"]).max()
    assert gu.rel(za.grad, FX[case + ".d_action_logit"]) <= 2e-5 and gu.rel(zs.grad, FX[case + ".d_scene_logit"]) <= 2e-5
