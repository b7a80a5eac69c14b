"""The bounds of tests/soft_ce_bounds.py proven without a GPU: the float64 reference is timm's SoftTargetCrossEntropy (two lines of torch) on the reference's mixup_target
formula with the rows the cases override; the CPU emulation stays under HALF the slack; every seeded mutant exceeds a bound."""
import pytest
import torch

import soft_ce_bounds as sb

DTYPES = (torch.float32, torch.bfloat16)


def _all():
    for B, C in sb.CASES:
        for dtype in DTYPES:
            yield B, C, dtype


def test_the_entries_the_bounds_are_for_exist():
    """what tests/test_soft_ce_bounds_gpu.py calls: the wrappers, their C entries, the criterion"""
    from devias_amd import _lib, losses, ops
    assert all(n in _lib.PROTOTYPES for n in ("devias_mixup_target", "devias_soft_ce_fwd", "devias_soft_ce_bwd", "devias_soft_ce_workspace_bytes"))
    assert callable(ops.mixup_target) and callable(ops.soft_ce_fwd) and callable(ops.soft_ce_bwd)
    with pytest.raises(RuntimeError, match="GPU tensor"):          # no CPU fallback
        losses.SoftTargetCrossEntropy()(torch.zeros(2, 5), torch.full((2, 5), 0.2))


def test_reference_is_timms_loss_on_the_reference_target():
    for B, C, dtype in _all():
        I = sb.inputs(B, C, dtype)
        ref, _ = sb.bounds(I, dtype)
        on, off = I["on"], I["off"]
        y1 = torch.full((B, C), off, dtype=torch.float64).scatter_(1, I["y"].view(-1, 1), on)                 # mixup.py:17-27 in float64
        y2 = torch.full((B, C), off, dtype=torch.float64).scatter_(1, I["y"].flip(0).view(-1, 1), on)
        t = sb.override_rows(y1 * I["ws"].double().view(-1, 1) + y2 * I["wo"].double().view(-1, 1), I["y"])
        assert torch.equal(t, ref["t"])
        z = I["z"].double().requires_grad_(True)
        want = torch.sum(-t * torch.nn.functional.log_softmax(z, dim=-1), dim=-1).mean()                  # timm.loss.SoftTargetCrossEntropy
        (want * float(I["g"])).backward()
        assert abs(float(ref["loss"]) - float(want.detach())) <= 1e-12 * abs(float(want.detach())), (B, C)
        assert float((ref["dz"] - z.grad).abs().max()) <= 1e-13, (B, C)
        # the rows the cases are about
        sums = ref["t"].sum(1)
        for b in range(B):
            kind = sb.ROW_KINDS[b % 4]
            assert abs(float(sums[b]) - {"mixed": 1.0, "one_hot": 1.0, "half": 0.5, "zero": 0.0}[kind]) <= 1e-6
            if kind == "one_hot":
                assert float(ref["t"][b].max()) == 1.0 and int((ref["t"][b] != 0).sum()) == 1


def test_emulation_stays_under_half_of_the_slack(capsys):
    worst = {}
    for B, C, dtype in _all():
        I = sb.inputs(B, C, dtype)
        ref, bnd = sb.bounds(I, dtype)
        for k, r in sb.ratios(sb.emulate(I, dtype), ref, bnd).items():
            key = (k, "bf16" if dtype == torch.bfloat16 else "fp32")
            worst[key] = max(worst.get(key, 0.0), r * sb.SLACK)
            assert r <= 0.5, (B, C, dtype, k, r)
    with capsys.disabled():
        for key in sorted(worst):
            print("soft-target CE emulation, worst ratio at slack 1:", key, round(worst[key], 4))


@pytest.mark.parametrize("mutant", sb.MUTANTS)
def test_every_mutant_exceeds_a_bound(mutant):
    failed = []
    for B, C, dtype in _all():
        I = sb.inputs(B, C, dtype)
        ref, bnd = sb.bounds(I, dtype)
        bad = {k: r for k, r in sb.ratios(sb.emulate(I, dtype, mutant=mutant), ref, bnd).items() if r > 1.0}
        if bad:
            failed.append((B, C, dtype, bad))
    assert failed, f"no case tells the mutant {mutant} from the kernel: the bounds show nothing about it"
