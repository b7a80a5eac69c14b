"""devias_mixup_target and devias_soft_ce_fwd / _bwd on the GPU against the float64 bounds of tests/soft_ce_bounds.py: every element of the target and of the
gradient, and the loss; fp32 and bf16 logits; rows made by a mixup, an exact one-hot, a row scaled by 0.5 and an all-zero row."""
import pytest
import torch

import soft_ce_bounds as sb

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", sb.CASES, ids=lambda c: "B%d_C%d" % c)
def test_target_and_soft_ce_kernels_within_bounds(case, dtype):
    from devias_amd import ops
    B, C = case
    I = sb.inputs(B, C, dtype)
    ref, bnd = sb.bounds(I, dtype)
    z, g = I["z"].to(DEV), I["g"].to(DEV)
    t = ops.mixup_target(I["y"].to(DEV), C, I["on"], I["off"], I["ws"].tolist(), I["wo"].tolist())
    t = sb.override_rows(t, I["y"]).contiguous()          # exact edits: a one-hot row, a row times 0.5, a zero row
    loss = ops.soft_ce_fwd(z, t)
    dz = ops.soft_ce_bwd(z, t, g)
    torch.cuda.synchronize()
    assert dz.dtype == dtype and loss.dtype == torch.float32
    out = {"t": t.cpu(), "loss": loss.cpu(), "dz": dz.float().cpu()}
    r = sb.ratios(out, ref, bnd)
    print("soft-target CE", case, dtype, {k: round(v, 4) for k, v in r.items()})
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    assert torch.equal(ops.soft_ce_fwd(z, t), loss) and torch.equal(ops.soft_ce_bwd(z, t, g), dz)          # fixed-order sums: the same bits again


def test_autograd_function_carries_the_device_scalar():
    """SoftTargetCrossEntropy under loss / update_freq: the gradient is the kernel's with g = 1 / 2, and no host sync is needed to get it there"""
    from devias_amd import ops
    from devias_amd.losses import SoftTargetCrossEntropy
    I = sb.inputs(8, 400, torch.bfloat16)
    z = I["z"].to(DEV).requires_grad_(True)
    t = ops.mixup_target(I["y"].to(DEV), 400, I["on"], I["off"], I["ws"].tolist(), I["wo"].tolist())
    loss = SoftTargetCrossEntropy()(z, t)
    (loss / 2).backward()
    assert loss.dim() == 0 and torch.equal(loss.reshape(1), ops.soft_ce_fwd(z.detach(), t))
    assert torch.equal(z.grad, ops.soft_ce_bwd(z.detach(), t, torch.tensor([0.5], device=DEV)))
