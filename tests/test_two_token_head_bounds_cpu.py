"""The bounds of tests/two_token_head_bounds.py proven without a GPU: from the inside (the CPU emulation of the kernels' documented roundings stays under HALF of
every slack, over every generator, both dtypes, both head modes) and from the outside (every seeded mutant exceeds a bound on at least one case)."""
import pytest
import torch

import two_token_head_bounds as tb

# (Nt, B, D, Ca, Cs, unified, masks, dtoken): no patch rows between the tokens, one, a few, around one chunk of the dx kernel, two chunks with a ragged tail
SHAPES = [(2, 1, 384, 2, 2, False, False, False), (2, 3, 384, 2, 2, True, True, True), (3, 3, 384, 101, 365, False, True, True), (7, 1, 768, 400, 365, True, True, False),
          (63, 3, 384, 101, 365, True, False, True), (64, 1, 768, 400, 365, False, True, True), (65, 3, 384, 101, 365, False, True, False),
          (131, 3, 1024, 101, 365, True, True, True)]
DTYPES = (torch.bfloat16, torch.float32)


def _cases():
    for kind in tb.GENERATORS:
        for shape in SHAPES:
            for dtype in DTYPES:
                yield kind, shape, dtype


def test_stagewise_reference_is_the_autograd_reference():
    for kind, (Nt, B, D, Ca, Cs, uni, mask, dtok), dtype in _cases():
        if dtype != torch.float32:
            continue
        I = tb.inputs(kind, B, Nt, D, Ca, Cs, dtype, uni, mask, dtok)
        ref, _ = tb.bounds(I, dtype)
        auto = tb.reference(I)
        assert set(auto) == set(ref)
        for k, v in auto.items():
            scale = float(v.abs().max()) + 1e-300
            assert float((ref[k] - v).abs().max()) <= 1e-11 * scale, (kind, Nt, uni, k)


def test_emulation_stays_under_half_of_every_slack(capsys):
    worst = {}
    for kind, (Nt, B, D, Ca, Cs, uni, mask, dtok), dtype in _cases():
        I = tb.inputs(kind, B, Nt, D, Ca, Cs, dtype, uni, mask, dtok)
        ref, bnd = tb.bounds(I, dtype)
        out = tb.emulate(I, dtype)
        assert set(out) == set(ref)
        for k, r in tb.ratios(out, ref, bnd).items():
            r1 = r * tb.SLACKS[k]                      # the ratio at slack 1
            key = (k, "bf16" if dtype == torch.bfloat16 else "fp32")
            if r1 > worst.get(key, (0.0,))[0]:
                worst[key] = (r1, kind, Nt, uni)
            limit = 1.0 if k == "a" else 0.5
            assert r <= limit, (kind, Nt, B, D, Ca, Cs, uni, dtype, k, r)
    with capsys.disabled():
        for key in sorted(worst):
            print("two_token_head emulation, worst ratio at slack 1:", key, worst[key])


def test_tail_rows_differ_by_far_more_than_the_bound():
    """the generator `tail`: the token of row Nt - 2 lies at least 1000 bounds away from the token of row Nt - 1 somewhere, in both dtypes"""
    for dtype in DTYPES:
        I = tb.inputs("tail", 3, 7, 384, 101, 365, dtype, False, False, False)
        ref, bnd = tb.bounds(I, dtype)
        other = torch.nn.functional.layer_norm(I["h"].double()[:, -2], (384,), I["gamma"].double(), I["beta"].double(), tb.EPS)
        assert tb.excess(other, ref["token_s"], bnd["token_s"] * tb.SLACK_FWD)[0] > 1000.0


@pytest.mark.parametrize("mutant", tb.MUTANTS)
def test_every_mutant_exceeds_a_bound(mutant):
    failed = []
    for kind, (Nt, B, D, Ca, Cs, uni, mask, dtok), dtype in _cases():
        I = tb.inputs(kind, B, Nt, D, Ca, Cs, dtype, uni, mask, dtok)
        ref, bnd = tb.bounds(I, dtype)
        out = tb.emulate(I, dtype, mutant=mutant)
        bad = {k: r for k, r in tb.ratios(out, ref, bnd).items() if r > 1.0}
        if bad:
            failed.append((kind, Nt, uni, dtype, bad))
    assert failed, f"no case tells the mutant {mutant} from the kernel: the bounds show nothing about it"
