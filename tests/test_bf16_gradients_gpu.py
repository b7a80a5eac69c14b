"""Element-wise gradients of the bf16 training step (the measured one) against fp32, per parameter family (tests/grad_compare.py: relative
Frobenius error, cosine, worst 64-row block), where every earlier bf16 check compared gradient NORMS, or only finiteness and run-to-run equality.

The reference is the fp32 parity mode of the same library on the same weights and inputs (pinned to the CPU oracle here and to the real
reference by the goldens).  bf16-only wiring is what these tests reach and the fp32 parity tests do not: the transposed weight copies of the
dgrad GEMMs, the q-prescaled qkv copy and DEVIAS_ATTN_Q_PRESCALED attention, the one-wave dK / dV kernel, the q / v bias gradients from dO,
the dGELU + column-sum epilogue, the 256^2 persistent kernel with split tail tiles at M = 50176, bf16 weight-gradient split-K.

Family bounds are about 2x the worst value measured on MI355X (written next to each bound).  rel / blk of a family is the worst over its
parameters of max(relative Frobenius error, worst 64-row block error)."""
from functools import partial
from types import SimpleNamespace

import pytest
import torch

import golden_util as gu
import grad_compare as gc
from devias_amd import ops, synth
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

# bound per family; (measured on MI355X) = the worst of rel / blk64 over the family's parameters, in the run that set the bound.
# agg_block: its worst is agg_block.layers.0.0.norm.bias, a gradient that is mathematically zero (cos ~ 0: round-off against round-off, measured
#   against the 1e-6 global floor); the family's other parameters stay under 2e-2.
# head (> 5e-2): the mask predictor's and the action / scene head's gradients are sums over only B x 2 slot rows of bf16-rounded slot features
#   and of loss gradients behind the scene KL of weight 4000 -- no averaging over tokens: a few 64-row blocks of mask_predictor.decoder reach 0.1.
def _fam(latents, patch_embed, qkv_weight, qv_bias, proj, fc1, fc2, norm, agg_block, head):
    return dict(latents=latents, patch_embed=patch_embed, qkv_weight=qkv_weight, qv_bias=qv_bias, proj=proj, fc1=fc1, fc2=fc2, norm=norm,
                agg_block=agg_block, head=head)


# ViT-B/16 16x224^2, B = 32 (the bench step), bf16 vs the fp32 mode; also every option of BOUNDED below (worst over default and options):
# measured 6.6e-3, 1.10e-2, 8.9e-3, 1.63e-2, 8.8e-3, 9.95e-3, 8.4e-3, 1.30e-2, 2.57e-2, 1.00e-1
TOL_B32 = _fam(1.5e-2, 2.5e-2, 2e-2, 3.5e-2, 2e-2, 2e-2, 2e-2, 3e-2, 5e-2, 2e-1)
# ViT-L/16, 24 blocks x 1568 tokens, B = 8: measured 7.9e-3, 1.33e-2, 1.07e-2, 1.72e-2, 1.06e-2, 1.28e-2, 1.05e-2, 1.39e-2, 2.95e-2, 9.7e-2
TOL_VITL = _fam(1.6e-2, 3e-2, 2.5e-2, 3.5e-2, 2.5e-2, 2.6e-2, 2.5e-2, 3e-2, 6e-2, 2e-1)
# ViT-B/16 32x320^2 (6400 tokens), B = 2: measured 9.0e-3, 1.14e-2, 1.16e-2, 1.94e-2, 1.0e-2, 1.09e-2, 1.01e-2, 1.39e-2, 3.37e-2, 5.5e-2
TOL_6400 = _fam(1.8e-2, 2.5e-2, 2.5e-2, 4e-2, 2e-2, 2.2e-2, 2.2e-2, 3e-2, 7e-2, 1.2e-1)
# training-mode regularisers and heads at ViT-B/16 8x224^2, B = 2, bf16 vs the fp32 mode with the same masks
TOL_REG = {
    # measured 8.3e-3, 1.23e-2, 1.02e-2, 1.90e-2, 9.1e-3, 1.08e-2, 9.0e-3, 1.57e-2, 5.4e-2, 9.7e-2
    "dropout": _fam(1.7e-2, 2.5e-2, 2.1e-2, 4e-2, 2e-2, 2.2e-2, 2e-2, 3.2e-2, 1.1e-1, 2e-1),
    # measured 8.9e-3, 1.18e-2, 1.06e-2, 2.09e-2, 9.7e-3, 1.08e-2, 1.02e-2, 1.30e-2, 1.71e-2, 1.53e-1
    "drop_path": _fam(1.8e-2, 2.4e-2, 2.2e-2, 4.2e-2, 2e-2, 2.2e-2, 2.1e-2, 2.6e-2, 3.5e-2, 3.1e-1),
    # measured 6.3e-2, 9.7e-2, 1.02e-1, 1.67e-1, 1.06e-1, 1.14e-1, 1.01e-1, 1.40e-1, 1.01e-1, 1.64e-1: every family ~8x the linear head's.  The
    # MLP head puts two more bf16 GEMMs and a ReLU between the slots and the logits; the head kernels alone are within 3e-2 of fp32 autograd
    # (test_recipe_gpu.py::test_mlp_head_with_and_without_fc_dropout).  Bounded as measured; the cause is not established.
    "mlp_head": _fam(1.3e-1, 2e-1, 2.1e-1, 3.4e-1, 2.2e-1, 2.3e-1, 2.1e-1, 2.8e-1, 2.1e-1, 3.3e-1),
    # measured 8.8e-3, 1.30e-2, 1.20e-2, 2.06e-2, 1.03e-2, 1.26e-2, 1.01e-2, 1.44e-2, 2.75e-2, 2.41e-1 (head: mask_predictor.decoder.0.weight)
    "classes101_fc_drop": _fam(1.8e-2, 2.6e-2, 2.4e-2, 4.2e-2, 2.1e-2, 2.6e-2, 2.1e-2, 2.9e-2, 5.5e-2, 4.8e-1),
}
# the fp32 mode itself vs the CPU oracle must be at least this much tighter than the bf16 bounds it serves as reference for (measured: 1.5e-6
# at worst, 3.8e-5 for the zero agg_block.layers.0.0.norm.bias gradient)
ANCHOR_FACTOR = 10.0


def _build(cfg, dtype, **kw):
    from devias_amd.modeling_slot import VisionTransformer
    m = VisionTransformer(img_size=cfg.img_size, patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4,
                          qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_classes=cfg.num_classes,
                          all_frames=cfg.all_frames, tubelet_size=cfg.tubelet_size, init_scale=1e-3,
                          num_latents=cfg.num_latents, head_type=cfg.head_type, slot_matching_method="matching",
                          agg_weights_tie=cfg.agg_weights_tie, agg_depth=cfg.agg_depth,
                          num_scene_classes=cfg.num_scene_classes, compute_dtype=dtype, **kw)
    synth.fill_module_(m, seed=0)
    return m.cuda().train()


def _crit(num_classes=400):
    from devias_amd.train_loss import TrainLoss
    return TrainLoss(criterion=None, scene_criterion="KL", num_action_classes=num_classes, slot_matching_method="matching",
                     mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0, scene_loss_weight=4000)


def _data(cfg, B):
    x, y, tl, fg = gu.inputs(cfg, B)
    return x.cuda(), y.cuda(), tl.cuda(), (fg[0].cuda(), fg[1].cuda())


def _flat(out):
    return [t for grp in out for t in grp if t is not None]


def _step(model, crit, data, seed=None):
    """one training step; returns every forward output, the loss, the slot match and a copy of every gradient"""
    x, y, tl, fg = data
    model.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)                       # fc dropout draws from torch's generator: the same mask in both modes
    out = model(x)
    total, _, _ = crit(model, out, (None, tl), y, fg_mask=fg)
    total.backward()
    torch.cuda.synchronize()
    return SimpleNamespace(out=[t.detach().clone() for t in _flat(out)], total=total.detach().clone(), match=crit.last_match.clone(),
                           grads={n: p.grad.detach().clone() for n, p in model.named_parameters()})


def _same_bits(a, b):
    """names of what differs between two _step results (empty: bitwise equal)"""
    diff = [] if torch.equal(a.total, b.total) else ["loss"]
    diff += [f"out{i}" for i, (u, v) in enumerate(zip(a.out, b.out)) if not torch.equal(u, v)]
    diff += [n for n in a.grads if not torch.equal(a.grads[n], b.grads[n])]
    return diff


# ------------------------------------------------------------------------------------------------ B = 32, the bench step
@pytest.fixture(scope="module")
def b32():
    """ViT-B/16 16x224^2, B = 32: the fp32-mode reference step (computed once for the module), the bf16 model and its default-option step"""
    cfg = ref_cpu.SlotViTConfig(all_frames=16)
    data = _data(cfg, 32)
    crit = _crit()
    m32 = _build(cfg, "fp32")
    ref = _step(m32, crit, data)
    del m32
    torch.cuda.empty_cache()
    model = _build(cfg, "bf16")
    base = _step(model, crit, data)
    return SimpleNamespace(cfg=cfg, data=data, crit=crit, ref=ref, model=model, base=base)


@pytest.fixture
def knobs():
    """set_(name, value): a library option for this test only; the scope restores every option when the test ends"""
    with ops.options():
        yield ops.set_option


def test_fp32_mode_anchor_vs_oracle():
    """the reference of this file, the fp32 mode, against the CPU oracle in the same metric (vitb_t16, B = 2): every family at least
    ANCHOR_FACTOR x tighter than the bf16 bounds"""
    fx, cfg, B = gu.load("vitb_t16")
    model = _build(cfg, "fp32")
    res = _step(model, _crit(), _data(cfg, B))
    x, y, tl, fg = gu.inputs(cfg, B)
    P = synth.fill_params(ref_cpu.param_shapes(cfg), seed=0)
    _, _, _, ograds, _, oidx = ref_cpu.train_step(P, cfg, x, y, tl, fg)
    assert res.match[:, 0].cpu().tolist() == oidx[0].tolist() and res.match[:, 1].cpu().tolist() == oidx[1].tolist()
    gc.check(res.grads, ograds, TOL_B32, "fp32-mode vs oracle vitb_t16 B=2", scale=1.0 / ANCHOR_FACTOR)


def test_bf16_b32_step_gradients_vs_fp32_mode(b32):
    """the bench step with default options: every one of the 186 gradients element-wise against the fp32 mode"""
    cnt_ok = b32.base.match.shape == b32.ref.match.shape and torch.equal(b32.base.match, b32.ref.match)
    assert cnt_ok, "a flipped slot match makes the gradients incomparable"
    assert len(b32.base.grads) == 186
    gc.check(b32.base.grads, b32.ref.grads, TOL_B32, "bf16 B=32 default")


# options documented or tested as the same arithmetic: loss, outputs and all 186 gradients bitwise equal to the default step
SAME_BITS = [
    {"gemm_wt": 0}, {"gemm_aux_nt": 0}, {"gemm_epi_spec": 0}, {"gemm_splitk_xcd": 0},
    {"gemm_dynamic": 1, "gemm_concurrent": 1},
    {"gemm_tail_split": 0}, {"gemm_tail_split": 1}, {"gemm_tail_split": 2}, {"gemm_tail_split": 4}, {"gemm_persistent": 0},
    {"attn_dkdv": 2}, {"attn_xcd": 0},
]
# options that change a summation order (or the kernel): within the B = 32 bounds of the fp32 mode
BOUNDED = [
    {"gemm_reserve_cus": 8}, {"gemm_reserve_cus": 16}, {"gemm_reserve_cus": 64},
    {"attn_qpre": 0}, {"attn_dkdv": 0}, {"attn_bias_fused": 0}, {"gemm_w4": 15},
    {"gemm_epi": 0}, {"gemm_groupm": 2}, {"gemm256": 0}, {"gemm_ss": 1}, {"gemm_smallm": 2}, {"attn_cfg": 6}, {"attn_cfg": 7},
]
_ID = lambda d: "+".join(f"{k}={v}" for k, v in d.items())      # noqa: E731


@pytest.mark.parametrize("opts", SAME_BITS, ids=_ID)
def test_b32_option_gives_the_same_bits(b32, knobs, opts):
    """The gemm_* and attn_* options of the library's table (csrc/common.h) are each in SAME_BITS, BOUNDED, or excluded here:
    gemm_debug (ablation bits, honoured only by a -DDEVIAS_GEMM_DEBUG build) and gemm_concurrent alone (it only announces concurrent
    kernels to gemm_dynamic = -1, which then takes the dynamic queues: the gemm_dynamic = 1 case)."""
    for k, v in opts.items():
        knobs(k, v)
    res = _step(b32.model, b32.crit, b32.data)
    diff = _same_bits(res, b32.base)
    assert not diff, f"{_ID(opts)} changed {len(diff)} results: {diff[:8]}"


@pytest.mark.parametrize("opts", BOUNDED, ids=_ID)
def test_b32_option_within_bounds(b32, knobs, opts):
    for k, v in opts.items():
        knobs(k, v)
    res = _step(b32.model, b32.crit, b32.data)
    assert torch.equal(res.match, b32.ref.match)
    if "gemm_reserve_cus" in opts:
        # the forward's tiles are whole-K on any grid: only the backward reductions follow the CU count
        assert torch.equal(res.total, b32.base.total) and all(torch.equal(u, v) for u, v in zip(res.out, b32.base.out))
    same = not _same_bits(res, b32.base)
    print(f"{_ID(opts)}: {'bitwise equal to' if same else 'differs from'} the default step")
    gc.check(res.grads, b32.ref.grads, TOL_B32, f"bf16 B=32 {_ID(opts)}")


# ------------------------------------------------------------------------------------------------ other geometries
@pytest.mark.parametrize("geom", ["vitl_1568_B8", "vitb_6400_B2"])
def test_bf16_gradients_vs_fp32_mode_at_baseline_geometry(geom):
    """BASELINE configs 4 (ViT-L/16, 24 blocks x 1568 tokens, B = 8) and 5 (ViT-B/16 32x320^2: 6400 tokens, B = 2)"""
    if geom == "vitl_1568_B8":
        cfg, B, tol = ref_cpu.SlotViTConfig(embed_dim=1024, num_heads=16, depth=24, all_frames=16), 8, TOL_VITL
    else:
        cfg, B, tol = ref_cpu.SlotViTConfig(all_frames=32, img_size=320), 2, TOL_6400
    data = _data(cfg, B)
    crit = _crit()
    m = _build(cfg, "fp32")
    ref = _step(m, crit, data)
    del m
    torch.cuda.empty_cache()
    res = _step(_build(cfg, "bf16"), crit, data)
    assert torch.equal(res.match, ref.match)
    gc.check(res.grads, ref.grads, tol, f"bf16 {geom}")


REG_CASES = {
    # the dropout golden's configuration: nn.Dropout (pos / proj / mlp), attention dropout and drop_path at 0.1, the golden's masks
    "dropout": (lambda: gu.load(gu.DROPOUT_GOLDEN)[1], lambda: gu.load(gu.DROPOUT_GOLDEN)[0]["_rates"]),
    # drop_path 0.2 alone (the UCF-101 recipe's rate)
    "drop_path": (lambda: gu.load("vitb_t8")[1], lambda: {"drop_path_rate": 0.2}),
    # the MLP head (the mlp-head golden's configuration)
    "mlp_head": (lambda: gu.load("vitb_t8_mlphead")[1], lambda: {}),
    # 101 action classes (head width 466, ragged) behind fc dropout 0.5
    "classes101_fc_drop": (lambda: ref_cpu.SlotViTConfig(all_frames=8, num_classes=101), lambda: {"fc_drop_rate": 0.5}),
}


@pytest.mark.parametrize("case", list(REG_CASES))
def test_bf16_regularised_step_vs_fp32_mode_same_masks(case):
    """training-mode dropout / drop_path / MLP head / 101 classes, B = 2: bf16 against the fp32 mode with the SAME masks (FormulaDropoutSource;
    fc dropout from torch's generator under one seed)"""
    cfg, rates = REG_CASES[case][0](), dict(REG_CASES[case][1]())
    crit = _crit(cfg.num_classes)
    data = _data(cfg, 2)
    res = {}
    for mode in ("fp32", "bf16"):
        m = _build(cfg, mode, **rates)
        m.dropout_source = gu.FormulaDropoutSource()
        res[mode] = _step(m, crit, data, seed=7)
        del m
    assert torch.equal(res["bf16"].match, res["fp32"].match)
    gc.check(res["bf16"].grads, res["fp32"].grads, TOL_REG[case], f"bf16 {case}")


# ------------------------------------------------------------------------------------------------ weight copies after an optimizer step
def test_weight_copies_follow_the_optimizer_step():
    """One FusedAdamW step over every parameter of a bf16 model, then a second training step; against a FRESHLY built bf16 model holding the
    updated values (every cached copy -- bf16, transposed, q-scaled, qkv bias -- made anew): loss, outputs and every gradient bitwise equal.
    A copy the update failed to refresh (a transposed weight read only by the backward's dgrad GEMMs, the q-scaled qkv weight) breaks the equality.
    M = 8 x 1568 = 49 x 256 rows: the 256^2 kernels serve the encoder GEMMs."""
    from devias_amd.weight_cache import _WCACHE
    from devias_amd.optim import FusedAdamW
    cfg = ref_cpu.SlotViTConfig(all_frames=16, depth=4)
    data = _data(cfg, 8)
    crit = _crit()
    m = _build(cfg, "bf16")
    opt = FusedAdamW(list(m.parameters()), lr=1e-3, weight_decay=0.05)
    _step(m, crit, data)
    opt.step()
    t0, q0 = _WCACHE.transposes, _WCACHE.qscaled
    after = _step(m, crit, data)
    # every encoder weight was transposed anew (4 per block) and the q-scaled qkv weight and bias re-made (2 per block)
    assert _WCACHE.transposes >= t0 + 4 * cfg.depth and _WCACHE.qscaled >= q0 + 2 * cfg.depth, (_WCACHE.transposes - t0, _WCACHE.qscaled - q0)
    fresh = _build(cfg, "bf16")
    with torch.no_grad():
        for (n, p), (n2, q) in zip(fresh.named_parameters(), m.named_parameters()):
            assert n == n2
            p.copy_(q)
    again = _step(fresh, crit, data)
    diff = _same_bits(after, again)
    assert not diff, f"{len(diff)} results differ after the optimizer step: {diff[:8]}"
