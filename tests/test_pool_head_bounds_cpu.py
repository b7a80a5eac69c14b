"""The bounds of tests/pool_head_bounds.py proven without a GPU: from the inside (the CPU emulation of the kernels' documented roundings stays under HALF of every
slack, over every generator, both dtypes, both pool modes) and from the outside (every seeded mutant exceeds a bound on at least one case)."""
import pytest
import torch

import pool_head_bounds as pb

# (Nt, B, D, C, mask, dtoken): one, few, around one chunk, three chunks with a ragged tail
SHAPES = [(1, 1, 384, 2, False, False), (7, 3, 384, 101, True, True), (pb.CHUNK - 1, 3, 384, 365, True, False), (pb.CHUNK, 1, 768, 400, False, True),
          (pb.CHUNK + 1, 3, 384, 365, True, True), (2 * pb.CHUNK + 3, 3, 1024, 101, True, True)]
DTYPES = (torch.bfloat16, torch.float32)


def _cases():
    for kind in pb.GENERATORS:
        for shape in SHAPES:
            for pool in (pb.MEAN, pb.CLS):
                for dtype in DTYPES:
                    yield kind, shape, pool, dtype


def test_stagewise_reference_is_the_autograd_reference():
    for kind, (Nt, B, D, C, mask, dtok), pool, dtype in _cases():
        if dtype != torch.float32:
            continue
        I = pb.inputs(kind, B, Nt, D, C, dtype, mask, dtok)
        ref, _ = pb.bounds(I, pool, dtype)
        auto = pb.reference(I, pool)
        for k, v in auto.items():
            scale = float(v.abs().max()) + 1e-300
            assert float((ref[k] - v).abs().max()) <= 1e-11 * scale, (kind, Nt, pool, k)


def test_emulation_stays_under_half_of_every_slack(capsys):
    worst = {}
    for kind, (Nt, B, D, C, mask, dtok), pool, dtype in _cases():
        I = pb.inputs(kind, B, Nt, D, C, dtype, mask, dtok)
        ref, bnd = pb.bounds(I, pool, dtype)
        out = pb.emulate(I, pool, dtype)
        for k, r in pb.ratios(out, ref, bnd).items():
            r1 = r * pb.SLACKS[k]                      # the ratio at slack 1
            key = (k, "bf16" if dtype == torch.bfloat16 else "fp32")
            if r1 > worst.get(key, (0.0,))[0]:
                worst[key] = (r1, kind, Nt, pool)
            limit = 1.0 if k == "a" else 0.5
            assert r <= limit, (kind, Nt, B, D, C, pool, dtype, k, r)
    with capsys.disabled():
        for key in sorted(worst):
            print("pool_head emulation, worst ratio at slack 1:", key, worst[key])


@pytest.mark.parametrize("mutant", pb.MUTANTS)
def test_every_mutant_exceeds_a_bound(mutant):
    failed = []
    for kind, (Nt, B, D, C, mask, dtok), pool, dtype in _cases():
        I = pb.inputs(kind, B, Nt, D, C, dtype, mask, dtok)
        ref, bnd = pb.bounds(I, pool, dtype)
        out = pb.emulate(I, pool, dtype, mutant=mutant)
        bad = {k: r for k, r in pb.ratios(out, ref, bnd).items() if r > 1.0}
        if bad:
            failed.append((kind, Nt, pool, dtype, bad))
    assert failed, f"no case tells the mutant {mutant} from the kernel: the bounds show nothing about it"
