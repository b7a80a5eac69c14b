"""The bounds of tests/fusion_bounds.py against the CPU emulation of the kernels (no GPU): the float64 reference plus exactly the kernels' roundings must stay under
every bound at HALF its slack (that is how the slacks are set), the bounds' stage-by-stage float64 values must be the autograd reference's, the planted selection must
hold its margin, and every seeded mutant must exceed 1."""
import itertools

import pytest
import torch

import fusion_bounds as fb

NB, NS = 5, 3
f = fb.f


def _case(kind, B, S, D, Cd, dtype, use_in, masked, seed=0):
    P = fb.make_params(D, NB, NS, Cd, use_in, seed)
    slots, P, dout, dinp, picks = fb.head_inputs(kind, B, S, D, dtype, P, seed)
    mask = fb.drop_mask(B, D, 0.5, seed) if masked else None
    return slots, P, dout, dinp, picks, mask


def _ratios(em, slots, P, use_in, mask, dout, dinp, dtype):
    ref, bnd = fb.bounds(slots, P, NB, use_in, mask, dout, dinp, em["idx"], em["r"] > 0, dtype)
    out = {"input": fb.excess(em["input"], ref["input"], bnd["input"])[0], "out": fb.excess(em["out"], ref["out"], bnd["out"])[0],
           "dslots": fb.excess(em["dslots"], ref["dslots"], bnd["dslots"])[0]}
    for n, g in em["grads"].items():
        out[n] = fb.excess(g, ref[n], bnd[n])[0]
    return out, ref


CASES = [(k, B, S, D, Cd, dt, ui, mk) for k, (B, S, D, Cd), dt, (ui, mk) in itertools.product(
    fb.GENERATORS, ((3, 3, 384, 48), (1, 1, 384, 2), (12, 4, 768, 101), (3, 2, 384, 200), (3, 3, 1024, 48)), (torch.float32, torch.bfloat16), ((True, False), (False, True), (True, True)))]


def test_emulation_stays_under_half_the_slack_and_selection_is_decisive():
    worst = {}
    for kind, B, S, D, Cd, dtype, use_in, masked in CASES:
        slots, P, dout, dinp, picks, mask = _case(kind, B, S, D, Cd, dtype, use_in, masked)
        idx, gap = fb.selection_gap(slots, P, NB)
        assert gap >= fb.MATCH_MARGIN and torch.equal(idx, picks), (kind, B, S, gap, idx, picks)
        em = fb.emulate(slots, P, NB, use_in, mask, dout, dinp, dtype)
        assert torch.equal(em["idx"], picks)
        ratios, _ = _ratios(em, slots, P, use_in, mask, dout, dinp, dtype)
        for n, v in ratios.items():
            grp = ("fwd" if n in ("input", "out") else "bwd", "bf16" if dtype == torch.bfloat16 else "fp32", "dslots/act" if n in ("input", "out", "dslots") else "params")
            if v > worst.get(grp, (0, None))[0]:
                worst[grp] = (v, (n, kind, B, S, D, Cd, use_in, masked))
    for k in sorted(worst):
        print("fusion emulation, worst ratio at slack 1:", k, "%.4f" % worst[k][0], worst[k][1])
    for (d, _, _), (v, where) in worst.items():
        assert v <= (fb.SLACK_FWD if d == "fwd" else fb.SLACK_BWD) / 2, (v, where)


def test_bounds_reference_is_the_autograd_reference():
    for kind, use_in, masked in (("diffuse", True, True), ("collide", False, False), ("last", True, False)):
        slots, P, dout, dinp, picks, mask = _case(kind, 3, 3, 384, 48, torch.float32, use_in, masked)
        ref, _ = fb.bounds(slots, P, NB, use_in, mask, dout, dinp, picks, None, torch.float32)
        ag = fb.reference(slots, P, NB, use_in, mask, dout, dinp)
        assert torch.equal(ag["idx"], picks)
        for n in ("input", "out", "dslots"):
            assert torch.allclose(ref[n], ag[n], rtol=1e-11, atol=1e-13), n
        for n, g in ag["grads"].items():
            assert torch.allclose(ref[n], g, rtol=1e-10, atol=1e-13), n
        # unselected rows are exactly zero; a collided row holds the sum
        sel = torch.zeros(3, 3, dtype=torch.bool)
        sel[torch.arange(3), picks[:, 0]] = True
        sel[torch.arange(3), picks[:, 1]] = True
        assert (~sel).any() and float(ag["dslots"][~sel].abs().max()) == 0.0


@pytest.mark.parametrize("mutant", [m for m in fb.MUTANTS if m != "no_smooth_term"])
def test_seeded_mutants_exceed_the_bounds(mutant):
    """each fault must push some output over its bound (slack included) on the generator built to show it, in fp32"""
    kind = {"no_sum": "collide", "eps_swap": "faint"}.get(mutant, "diffuse")
    dtype = torch.float32
    slots, P, dout, dinp, picks, mask = _case(kind, 3, 3, 384, 48, dtype, True, True)
    em = fb.emulate(slots, P, NB, True, mask, dout, dinp, dtype, mutant=mutant)
    ratios, _ = _ratios(em, slots, P, True, mask, dout, dinp, dtype)
    worst = max(v / (fb.SLACK_FWD if n in ("input", "out") else fb.SLACK_BWD) for n, v in ratios.items())
    print("mutant", mutant, "worst excess %.3g" % worst)
    assert worst > 1.0, ratios


CE_CASES = [(C, B, eps, kind, dt) for C, B, eps, kind, dt in itertools.product((2, 48, 101, 1000), (1, 5), (0.0, 0.1), ("plain", "last", "peaked"),
                                                                            (torch.float32, torch.bfloat16))]


def test_cross_entropy_emulation_and_mutant():
    worst = {}
    for C, B, eps, kind, dtype in CE_CASES:
        z, y = fb.ce_inputs(C, B, kind, dtype)
        g = 0.5
        loss, dz = fb.emulate_ce(z, y, eps, g, dtype)
        rl, rdz = fb.ce_reference(z, y, eps, g)
        bl, bdz = fb.ce_bounds(z, y, eps, g, dtype)
        k = "bf16" if dtype == torch.bfloat16 else "fp32"
        worst[k, "loss"] = max(worst.get((k, "loss"), 0), fb.excess(loss, rl, bl)[0])
        worst[k, "dz"] = max(worst.get((k, "dz"), 0), fb.excess(dz, rdz, bdz)[0])
        if eps > 0 and kind == "plain":
            _, dzm = fb.emulate_ce(z, y, eps, g, dtype, mutant="no_smooth_term")
            assert fb.excess(dzm, rdz, bdz * fb.SLACK_CE)[0] > 1.0, (C, B, dtype)
    print("cross-entropy emulation, worst ratio at slack 1:", {k: "%.4f" % v for k, v in worst.items()})
    assert max(worst.values()) <= fb.SLACK_CE / 2, worst
