"""Mixup / CutMix on the GPU: devias_amd.mixup.Mixup against what the real reference computed for every case of tests/golden/mixup_vectors.npz (clip and soft target,
BITWISE), in place, repeatable; larger batches and clips against the same table applied with ATen; labels out of range; one step of each engine with a Mixup against
the hand-composed sequence; the plain ViT's fp32 step under mixup against tests/golden/plainvit_mean_mixup_t8.npz."""
import ast
from functools import partial

import numpy as np
import pytest
import torch

import golden_util as gu
from devias_amd import synth
from test_mixup_cpu import CASES, FX, build, case

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3          # the project's parity gate (tests/test_plainvit_gpu.py holds the unmixed step to it)


def _bits(t):
    return t.detach().float().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _on_device(x_np, dtype, offset):
    """the clip on the device; offset 1: its storage starts one element into an allocation, so the base is not 16-byte aligned (the scalar kernel)"""
    x = torch.from_numpy(x_np).to(dtype)
    buf = torch.empty(x.numel() + offset, dtype=dtype, device=DEV)
    out = buf[offset:].view(x.shape)
    out.copy_(x)
    assert out.is_contiguous() and (out.data_ptr() % 16 == 0) == (offset == 0)
    return out


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("name", CASES)
def test_clip_and_target_are_bitwise_the_references(name, offset):
    cfg, r = case(name)
    dtype = torch.bfloat16 if cfg["dtype"] == "bf16" else torch.float32
    m = build(cfg, int(FX["num_classes"]))
    x = _on_device(r["x"], dtype, offset)
    y = torch.from_numpy(r["y"]).to(DEV)
    before = x.clone()
    np.random.seed(int(r["seed"]))
    out, target = m(x, y)
    torch.cuda.synchronize()
    assert out is x and out.data_ptr() == x.data_ptr()                                   # in place: the same storage
    assert target.dtype == torch.float32 and tuple(target.shape) == (cfg["B"], int(FX["num_classes"]))
    assert _same_bits(x, torch.from_numpy(r["out_x"])), name
    assert _same_bits(target, torch.from_numpy(r["out_target"])), name
    for i in np.nonzero(r["kind"] == 0)[0]:                                              # an unmixed clip is untouched
        assert _same_bits(x[int(i)], before[int(i)])
    x2 = before.clone()                                                                  # the same seed again: the same bits
    np.random.seed(int(r["seed"]))
    _, target2 = m(x2, y)
    assert _same_bits(x2, x) and _same_bits(target2, target)


def _aten_apply(x0, table):
    """the table applied with ATen, one op per rounding: what the reference's tensor expressions compute for these rows"""
    B = x0.shape[0]
    out = x0.clone()
    for i, row in enumerate(table.rows):
        j = B - 1 - i
        if row.kind == 1:
            out[i] = x0[i] * row.w_self + x0[j] * row.w_other
        elif row.kind == 2:
            out[i][..., row.yl:row.yh, row.xl:row.xh] = x0[j][..., row.yl:row.yh, row.xl:row.xh]
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("mode,kw,shape", [
    ("batch", dict(mixup_alpha=0.8, cutmix_alpha=0.0), (4, 3, 4, 40, 36)),          # several workgroups of 16-byte pieces
    ("batch", dict(mixup_alpha=0.0, cutmix_alpha=1.0), (4, 3, 4, 40, 36)),          # rows [yl, yh) of every plane
    ("elem", dict(mixup_alpha=0.8, cutmix_alpha=1.0), (6, 3, 4, 40, 36)),
    ("elem", dict(mixup_alpha=0.8, cutmix_alpha=1.0), (6, 3, 2, 25, 18)),           # a plane of 450 elements: fp32 pieces straddle planes (bf16: the scalar kernel)
    ("elem", dict(mixup_alpha=0.8, cutmix_alpha=1.0), (6, 3, 4, 30, 18)),           # a plane of 540 elements: bf16 pieces straddle planes
    ("elem", dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.7), (70, 1, 1, 5, 7)),  # 35 pairs: more than one launch's worth, misaligned clips
], ids=["batch_mixup", "batch_cutmix", "elem_both", "elem_straddle_fp32", "elem_straddle_bf16", "elem_70_clips"])
def test_larger_batches_against_the_table_applied_with_aten(mode, kw, shape, dtype):
    from devias_amd.mixup import Mixup
    m = Mixup(mode=mode, num_classes=7, **kw)
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(shape, generator=g).to(dtype).to(DEV)
    y = torch.randint(0, 7, (shape[0],), generator=g).to(DEV)
    for seed in (0, 1, 2):
        np.random.seed(seed)
        table = m.draw(shape)
        x = x0.clone()
        m.apply(x, y, table)
        assert _same_bits(x, _aten_apply(x0, table)), (mode, seed)


def test_target_of_many_rows_and_labels_out_of_range():
    from devias_amd import mixup as mx
    from devias_amd.losses import SoftTargetCrossEntropy
    B, C = 258, 5                                                                        # more rows than one launch carries weights for
    g = torch.Generator().manual_seed(3)
    y = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    t = mx.mixup_target(y.to(DEV), C, lam, 0.1, DEV)
    off = 0.1 / C
    on = 1. - 0.1 + off
    y1 = torch.full((B, C), off).scatter_(1, y.view(-1, 1), on)
    y2 = torch.full((B, C), off).scatter_(1, y.flip(0).view(-1, 1), on)
    assert _same_bits(t, y1 * lam.view(-1, 1) + y2 * (1. - lam).view(-1, 1))
    # a label outside [0, C) is never an index: its row and the partner row that reads it are NaN, and so is the loss
    y = torch.tensor([1, 10 ** 6, 2, 0, 4, 3], dtype=torch.int64, device=DEV)
    t = mx.mixup_target(y, C, 0.3, 0.1, DEV).cpu()
    nan_rows = torch.isnan(t).all(1).tolist()
    assert nan_rows == [False, True, False, False, True, False] and torch.isfinite(t[[0, 2, 3, 5]]).all()
    assert torch.isnan(mx.mixup_target(torch.tensor([-1, 2], dtype=torch.int64, device=DEV), C, 1., 0.0, DEV)).all()
    z = torch.randn(6, C, device=DEV, requires_grad=True)
    loss = SoftTargetCrossEntropy()(z, t.to(DEV))
    assert torch.isnan(loss)


# ---- the engines ---------------------------------------------------------------------------------------------------------------------------------
SMALL = dict(embed_dim=384, depth=2, num_heads=6, qkv_bias=True, all_frames=2, init_scale=1.0, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
NC, NS = 17, 9


def _plain(num_classes, seed, **kw):
    from devias_amd.modeling_finetune import VisionTransformer
    m = VisionTransformer(num_classes=num_classes, compute_dtype="fp32", **dict(SMALL, **kw))
    synth.fill_module_(m, seed=seed)
    return m.to(DEV).train()


def _loader():
    return [(synth.video(2, 2, 224, seed=40), synth.targets(2, NC, seed=40), None, None)]


def _mix():
    from devias_amd.mixup import Mixup
    return Mixup(0.8, 1.0, label_smoothing=0.1, num_classes=NC)


def _sgd(model):
    return torch.optim.SGD(model.parameters(), lr=0.0)


@pytest.mark.parametrize("seed", [11, 12])
def test_downstream_engine_step_is_the_hand_composed_sequence(seed):
    from devias_amd import engine_for_finetuning as eng
    from devias_amd.losses import SoftTargetCrossEntropy
    model, crit, mix = _plain(NC, 0), SoftTargetCrossEntropy(), _mix()
    (x, y, _, _), = _loader()
    np.random.seed(seed)
    xm, t = mix(x.to(DEV), y.to(DEV))
    want, _ = eng.train_class_batch(model, xm, t, crit)
    np.random.seed(seed)
    stats = eng.train_one_epoch(model, crit, _loader(), _sgd(model), DEV, 0, mixup_fn=mix, check_finite_every=1)
    assert np.isfinite(stats["loss"]) and stats["loss"] == float(want.detach())


def test_scene_engine_mixes_after_the_teachers_argmax():
    from devias_amd import engine_for_finetuning_scene as eng
    from devias_amd.losses import SoftTargetCrossEntropy
    model, teacher, crit, mix = _plain(NC, 0), _plain(NC, 1).eval(), SoftTargetCrossEntropy(), _mix()
    (x, _, _, _), = _loader()
    x = x.to(DEV)
    labels = eng.scene_targets(teacher, x)                      # on the UNMIXED clip
    np.random.seed(21)
    xm, t = mix(x.clone(), labels)
    want, _ = eng.train_class_batch(model, xm, t, crit)
    np.random.seed(21)
    stats = eng.train_one_epoch(model, teacher, crit, _loader(), _sgd(model), DEV, 0, mixup_fn=mix, check_finite_every=1)
    assert np.isfinite(stats["loss"]) and stats["loss"] == float(want.detach())
    assert not _same_bits(xm, x)                                 # the seed mixes: the order of argmax and mix is what the equality above shows


def test_multi_task_engine_feeds_student_and_teacher_the_mixed_clip():
    from devias_amd import engine_for_multi_task as eng
    from devias_amd.losses import SoftTargetCrossEntropy
    from devias_amd.modeling_multi_task import VisionTransformer
    from devias_amd.multi_task_loss import TrainLoss
    model = VisionTransformer(num_classes=NC, num_scene_classes=NS, compute_dtype="fp32", **SMALL)
    synth.fill_module_(model, seed=0)
    model = model.to(DEV).train()
    teacher = _plain(NS, 1).eval()
    crit = TrainLoss(SoftTargetCrossEntropy(), "KL", num_action_classes=NC)
    mix = _mix()
    (x, y, _, _), = _loader()
    np.random.seed(31)
    xm, t = mix(x.to(DEV), y.to(DEV))
    want, _, parts = eng.train_class_batch(model, teacher, xm, t, crit)
    np.random.seed(31)
    stats = eng.train_one_epoch(model, teacher, crit, _loader(), _sgd(model), DEV, 0, mixup_fn=mix, check_finite_every=1)
    assert np.isfinite(stats["loss"]) and stats["loss"] == float(want.detach()) and stats["action_loss"] == parts["action_loss"] and stats["logit_loss"] == parts["logit_loss"]


# ---- the plain ViT's fp32 step under mixup against the step the reference ran ---------------------------------------------------------------------
def test_plainvit_fp32_step_under_mixup_against_the_reference():
    from devias_amd.losses import SoftTargetCrossEntropy
    from devias_amd.mixup import Mixup
    from devias_amd.modeling_finetune import vit_base_patch16_224
    fx = dict(np.load(gu.GOLDEN_DIR + "/plainvit_mean_mixup_t8.npz", allow_pickle=False))
    cfg, B, mk = ast.literal_eval(str(fx["config"])), int(fx["batch"]), ast.literal_eval(str(fx["mixup"]))
    model = vit_base_patch16_224(**dict(cfg, compute_dtype="fp32"))
    synth.fill_module_(model, seed=0)
    model = model.to(DEV).train()
    x = synth.video(B, cfg["all_frames"], 224, seed=1000).to(DEV)
    y = synth.targets(B, cfg["num_classes"], seed=1000).to(DEV)
    mix = Mixup(label_smoothing=float(fx["smoothing"]), num_classes=cfg["num_classes"], **mk)
    np.random.seed(int(fx["mixup_seed"]))
    x, t = mix(x, y)
    assert _same_bits(t, torch.from_numpy(fx["soft_target"]))
    token, logits = model(x)
    loss = SoftTargetCrossEntropy()(logits, t)
    loss.backward()
    torch.cuda.synchronize()
    errs = {"token": gu.rel(token.detach().float().cpu(), fx["token"]), "logits": gu.rel(logits.detach().float().cpu(), fx["logits"]),
            "loss": abs(float(loss.detach()) - float(fx["loss"])) / abs(float(fx["loss"]))}
    names = [str(n) for n in fx["param_names"]]
    grads = {n: p.grad.detach() for n, p in model.named_parameters()}
    assert names == list(grads)
    nmax = float(fx["grad_norms"].max())
    for i, n in enumerate(names):
        g = grads[n].float().cpu()
        ref_norm = float(fx["grad_norms"][i])
        errs[n + ".norm"] = abs(float(g.double().norm()) - ref_norm) / max(ref_norm, 1e-6 * nmax)
        smp = g.reshape(-1)[torch.from_numpy(gu.sample_idx(n, g.numel()))].double().numpy()
        ref_s = fx["grad_samples"][i].astype(np.float64)
        errs[n + ".samples"] = float(np.abs(smp - ref_s).max() / max(np.abs(ref_s).max(), 1e-6 * nmax, 1e-30))
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print("[plainvit mean fp32 under mixup vs reference] token %.2e logits %.2e loss %.2e; worst: %s" % (errs["token"], errs["logits"], errs["loss"],
                                                                                                        ", ".join("%s %.2e" % kv for kv in worst)))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad
