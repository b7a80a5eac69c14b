"""tests/grad_compare.py flags the errors a gradient-norm comparison lets through: a permutation of 64-row blocks, two same-shape gradients
swapped, a 20 % perturbation orthogonal to the gradient."""
import torch

import grad_compare as gc


def _grads(seed=0):
    g = torch.Generator().manual_seed(seed)
    shapes = {"blocks.0.attn.qkv.weight": (192, 64), "blocks.0.attn.q_bias": (64,), "blocks.0.attn.v_bias": (64,),
              "blocks.0.attn.proj.weight": (64, 64), "blocks.1.attn.proj.weight": (64, 64), "blocks.0.mlp.fc1.weight": (256, 64),
              "blocks.0.norm1.weight": (64,), "agg_block.latents": (2, 64), "head.weight": (101, 64)}
    return {n: torch.randn(s, generator=g, dtype=torch.float64) for n, s in shapes.items()}


def _norm_rel(a, b):
    return max(abs(float(a[n].norm()) - float(b[n].norm())) / float(b[n].norm()) for n in b)


BOUNDS = {f: 1e-2 for f in gc.FAMILY_NAMES}


def test_identical_and_small_noise_pass():
    ref = _grads()
    errs = gc.compare({n: t.clone() for n, t in ref.items()}, ref)
    assert all(e.rel == 0 and e.blk == 0 and abs(e.cos - 1) < 1e-12 for e in errs.values())
    g = torch.Generator().manual_seed(1)
    noisy = {n: t * (1 + 1e-3 * torch.randn(t.shape, generator=g, dtype=torch.float64)) for n, t in ref.items()}
    assert not gc.violations(gc.compare(noisy, ref), BOUNDS)


def test_row_block_permutation_is_flagged():
    ref = _grads()
    bad = dict(ref)
    w = ref["blocks.0.mlp.fc1.weight"]
    bad["blocks.0.mlp.fc1.weight"] = torch.cat((w[64:128], w[:64], w[128:]))
    assert _norm_rel(bad, ref) < 1e-12                       # invisible to a norm check
    v = gc.violations(gc.compare(bad, ref), BOUNDS)
    assert list(v) == ["blocks.0.mlp.fc1.weight"] and v["blocks.0.mlp.fc1.weight"][0] == "fc1"
    # a head's q rows swapped with its k rows inside the qkv weight
    q = ref["blocks.0.attn.qkv.weight"]
    bad = dict(ref, **{"blocks.0.attn.qkv.weight": torch.cat((q[64:128], q[:64], q[128:]))})
    e = gc.compare(bad, ref)["blocks.0.attn.qkv.weight"]
    assert e.blk > 1.0 and e.rel > 0.5


def test_swap_of_same_shape_tensors_is_flagged():
    ref = _grads()
    for a, b in (("blocks.0.attn.q_bias", "blocks.0.attn.v_bias"), ("blocks.0.attn.proj.weight", "blocks.1.attn.proj.weight")):
        bad = dict(ref, **{a: ref[b], b: ref[a]})
        assert _norm_rel(bad, ref) < 0.3
        v = gc.violations(gc.compare(bad, ref), BOUNDS)
        assert set(v) == {a, b}, v


def test_orthogonal_perturbation_is_flagged():
    ref = _grads()
    g = torch.Generator().manual_seed(2)
    bad = {}
    for n, r in ref.items():
        e = torch.randn(r.shape, generator=g, dtype=torch.float64)
        e -= (e * r).sum() / (r * r).sum() * r                # orthogonal to r
        bad[n] = r + 0.2 * r.norm() / e.norm() * e
    assert _norm_rel(bad, ref) < 2.1e-2                       # a 20 % error moves the norm by 2 %
    errs = gc.compare(bad, ref)
    assert all(abs(e.rel - 0.2) < 1e-9 and abs(e.cos - 1 / (1.04 ** 0.5)) < 1e-9 for e in errs.values())
    assert set(gc.violations(errs, BOUNDS)) == set(ref)
    assert not gc.violations(errs, {f: 0.25 for f in gc.FAMILY_NAMES})


def test_zero_reference_uses_the_global_floor():
    ref = _grads()
    ref["blocks.0.norm1.weight"] = torch.zeros(64, dtype=torch.float64)
    got = dict(ref, **{"blocks.0.norm1.weight": torch.full((64,), 1e-9, dtype=torch.float64)})
    e = gc.compare(got, ref)["blocks.0.norm1.weight"]
    assert e.rel < 1e-2 and e.blk < 1e-2


def test_every_model_parameter_has_a_family():
    from oracle import ref_cpu
    for cfg in (ref_cpu.SlotViTConfig(all_frames=16), ref_cpu.SlotViTConfig(head_type="mlp", num_latents=4, agg_weights_tie=False, agg_depth=4)):
        fams = {gc.family(n) for n in ref_cpu.param_shapes(cfg)}
        assert fams == set(gc.FAMILY_NAMES), fams
