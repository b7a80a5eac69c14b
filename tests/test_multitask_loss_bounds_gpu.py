"""devias_distill_fwd / _bwd on the GPU against the float64 bounds of tests/multitask_loss_bounds.py (every element of the gradient, the loss; both modes, fp32 and
bf16 student logits, with and without the unified head's pad, the first-index tie), and devias_amd.multi_task_loss.TrainLoss against the fixture the driver's
TrainLoss wrote (tests/golden/multitask_loss.npz)."""
import numpy as np
import pytest
import torch

import golden_util as gu
import multitask_loss_bounds as lb

pytestmark = pytest.mark.gpu
DEV = "cuda"
FX = dict(np.load(gu.GOLDEN_DIR + "/multitask_loss.npz", allow_pickle=False))
TOL = 1e-3          # the project's parity gate (fp32 logits against the driver's fp32 CPU run)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode", lb.MODES)
@pytest.mark.parametrize("case", lb.CASES, ids=lambda c: "B%d_C%d_pad%d" % c)
def test_distill_kernels_within_bounds(case, mode, dtype):
    from devias_amd import _lib, ops
    B, C, pad = case
    I = lb.inputs(B, C, pad, dtype)
    ref, bnd = lb.bounds(I, mode, dtype)
    code = _lib.DISTILL_CE if mode == "CE" else _lib.DISTILL_KL
    z, t, g = I["z"].to(DEV), I["t"].to(DEV), I["g"].to(DEV)
    loss, tmin = ops.distill_fwd(z, t, code, I["w"])
    dz = ops.distill_bwd(z, t, tmin, g, code, I["w"])
    torch.cuda.synchronize()
    assert (tmin is None) == (pad == 0)
    if pad and mode == "KL":
        assert float(tmin) == float(I["t"].min())          # a minimum has no rounding
    out = {"loss": loss.cpu(), "dz": dz.float().cpu()}
    r = lb.ratios(out, ref, bnd)
    print("distill", case, mode, dtype, {k: round(v, 4) for k, v in r.items()})
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    if mode == "CE":          # the tie of row 0: the one-hot sits on the FIRST of the two maxima
        assert int(torch.argmin(out["dz"][0])) == pad + I["first"]
    loss2, tmin2 = ops.distill_fwd(z, t, code, I["w"])
    assert torch.equal(loss2, loss) and torch.equal(ops.distill_bwd(z, t, tmin2, g, code, I["w"]), dz)


@pytest.mark.parametrize("case", [str(c) for c in FX["cases"]])
def test_train_loss_matches_the_drivers(case):
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.multi_task_loss import TrainLoss
    crit, head, shape = case.split(".")
    ca = int(shape.split("_")[1][2:])
    za = torch.from_numpy(FX[case + ".action_logit"]).to(DEV).requires_grad_(True)
    zs = torch.from_numpy(FX[case + ".scene_logit"]).to(DEV).requires_grad_(True)
    teacher, target = torch.from_numpy(FX[case + ".teacher"]).to(DEV), torch.from_numpy(FX[case + ".target"]).to(DEV)
    tl = TrainLoss(LabelSmoothingCrossEntropy(float(FX["smoothing"])), crit, unified_head=head == "unified", num_action_classes=ca,
                   logit_criterion_weight=float(FX["logit_criterion_weight"]))
    total, action_logit, ld = tl(((None, za), (None, zs)), (None, teacher), target)
    assert action_logit is za and set(ld) == {"action_loss", "logit_loss"} and all(isinstance(v, float) for v in ld.values())
    total.backward()
    got = np.array([float(total.detach()), ld["action_loss"], ld["logit_loss"]])
    want = FX[case + ".losses"]
    errs = {"losses": float(np.abs(got - want).max() / np.abs(want).max()), "d_action_logit": gu.rel(za.grad.cpu(), FX[case + ".d_action_logit"]),
            "d_scene_logit": gu.rel(zs.grad.cpu(), FX[case + ".d_scene_logit"])}
    print("[multitask TrainLoss vs the driver]", case, {k: "%.2e" % v for k, v in errs.items()})
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
    # sync_loss_dict=False: 0-d device tensors, the same numbers
    tl.sync_loss_dict = False
    _, _, ld2 = tl(((None, za.detach()), (None, zs.detach())), (None, teacher), target)
    assert all(torch.is_tensor(v) and v.is_cuda and v.dim() == 0 for v in ld2.values()) and float(ld2["logit_loss"]) == ld["logit_loss"]
