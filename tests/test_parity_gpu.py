"""End-to-end parity of the HIP path (through the C ABI) against the golden fixtures produced by the real reference
and against the CPU oracle, on the same formula weights / inputs.  fp32 kernel mode carries the 1e-3 gate of
BASELINE.json's north_star; bf16 mode deviation is measured and bounded loosely."""
import os
import numpy as np
import pytest
import torch

import golden_util as gu
from devias_amd import synth
from oracle import ref_cpu

pytestmark = pytest.mark.gpu

TOL_FP32 = 1e-3          # north_star: per-slot logits and total loss within 1e-3 relative (fp32)


def build(cfg, dtype, rates=None):
    from devias_amd.modeling_slot import VisionTransformer
    from functools import partial
    m = VisionTransformer(patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4, **(rates or {}),
                          qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_classes=cfg.num_classes,
                          all_frames=cfg.all_frames, tubelet_size=cfg.tubelet_size, init_scale=1e-3,
                          num_latents=cfg.num_latents, head_type=cfg.head_type, slot_matching_method="matching",
                          agg_weights_tie=cfg.agg_weights_tie, agg_depth=cfg.agg_depth,
                          num_scene_classes=cfg.num_scene_classes, compute_dtype=dtype)
    synth.fill_module_(m, seed=0)
    return m.cuda().train()


def run_step(model, cfg, B):
    from devias_amd.train_loss import TrainLoss
    x, y, tl, fg = gu.inputs(cfg, B)
    crit = TrainLoss(criterion=None, scene_criterion="KL", num_action_classes=cfg.num_classes, slot_matching_method="matching",
                     mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0, scene_loss_weight=4000)
    out = model(x.cuda())
    total, logits, ld = crit(model, out, (None, tl.cuda()), y.cuda(), fg_mask=(fg[0].cuda(), fg[1].cuda()))
    model.zero_grad()
    total.backward()
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    return out, total, logits, ld, grads, crit.last_match


@pytest.mark.parametrize("name", gu.STUDENT_GOLDENS)
def test_fp32_step_matches_reference_golden(name):
    fx, cfg, B = gu.load(name)
    model = build(cfg, "fp32")
    out, total, logits, ld, grads, match = run_step(model, cfg, B)
    idx = (match[:, 0].cpu().tolist(), match[:, 1].cpu().tolist())
    errs, gerrs = gu.check_against_golden(fx, out, float(total), logits, ld, grads, tol_out=TOL_FP32, tol_grad=5e-3, idx=idx)
    print(name, "max output err", max(errs.values()), "max grad err", max(gerrs.values()))
    # intermediate taps are not exposed by the fused path; outputs + 186 gradient norms pin every parameter's path


@pytest.mark.parametrize("dtype,tol_out,tol_grad", [("fp32", TOL_FP32, 5e-3), ("bf16", 5e-2, None)])
def test_dropout_step_matches_reference_golden(dtype, tol_out, tol_grad):
    """nn.Dropout inside the encoder (pos_drop, attn_drop, proj_drop, Mlp.drop: model/modeling_slot.py:280,356 / 90,110 / 92,114 / 58,66) + drop_path,
    training mode, rates 0.1: the golden is the REAL reference run with its dropout modules multiplying by given masks; the HIP model draws the same masks
    through its DropoutSource (element masks: devias_amd.synth formulae; attention-matrix mask: the kernels' hash of the same seeds).  fp32: the north_star
    gate on outputs, loss and every gradient; bf16: bounded."""
    fx, cfg, B = gu.load(gu.DROPOUT_GOLDEN)
    model = build(cfg, dtype, fx["_rates"])
    model.dropout_source = gu.FormulaDropoutSource()
    from devias_amd import ops
    ops.counters(reset=True)
    out, total, logits, ld, grads, match = run_step(model, cfg, B)
    cnt = ops.counters()
    assert cnt["mhsa_fwd_" + ("f32" if dtype == "fp32" else "bf16")] == cfg.depth            # every block's attention ran in the library
    if dtype == "fp32":
        idx = (match[:, 0].cpu().tolist(), match[:, 1].cpu().tolist())
        errs, gerrs = gu.check_against_golden(fx, out, float(total.detach()), logits, ld, grads, tol_out=tol_out, tol_grad=tol_grad, idx=idx)
        print("dropout golden fp32: max output err", max(errs.values()), "max grad err", max(gerrs.values()))
    else:
        e_logit = gu.rel(out[2][0].detach().float().cpu(), fx["slots_head"])
        e_total = abs(float(total) - float(fx["total_loss"])) / abs(float(fx["total_loss"]))
        names = [str(n) for n in fx["param_names"]]
        gn = np.array([float(grads[n].double().norm()) for n in names])
        e_gn = np.abs(gn - fx["grad_norms"]) / np.maximum(fx["grad_norms"], 1e-6 * fx["grad_norms"].max())
        print(f"dropout golden bf16: logits rel {e_logit:.3e}, total loss rel {e_total:.3e}, grad-norm rel median {np.median(e_gn):.3e}")
        assert e_logit < tol_out and e_total < 2e-2 and np.median(e_gn) < 5e-2
    # eval mode draws nothing and is the un-dropped model
    model.eval()
    x, _, _, _ = gu.inputs(cfg, B)
    with torch.no_grad():
        a = model(x.cuda())[2][0]
        b = model(x.cuda())[2][0]
    assert torch.equal(a, b)


def test_dropout_default_source_draws_from_torch_generators():
    """without an installed source the masks come from torch's generators (as nn.Dropout's do): reproducible under torch.manual_seed, different across
    draws; rates reach the modules as in the reference (modeling_slot.py:280-289)"""
    fx, cfg, B = gu.load("vits_t8")
    model = build(cfg, "fp32", dict(drop_rate=0.2, attn_drop_rate=0.3))
    assert model.pos_drop.p == 0.2 and model.blocks[0].attn.attn_drop.p == 0.3 and model.blocks[0].attn.proj_drop.p == 0.2 and model.blocks[0].mlp.drop.p == 0.2
    x, _, _, _ = gu.inputs(cfg, B)
    x = x.cuda()
    torch.manual_seed(5); a = model(x)[2][0].detach().clone()
    b = model(x)[2][0].detach().clone()
    torch.manual_seed(5); c = model(x)[2][0].detach().clone()
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_fp32_forward_is_deterministic():
    fx, cfg, B = gu.load("vitb_t8")
    model = build(cfg, "fp32")
    o1, t1, l1, _, g1, _ = run_step(model, cfg, B)
    o2, t2, l2, _, g2, _ = run_step(model, cfg, B)
    assert torch.equal(o1[2][0], o2[2][0]) and torch.equal(t1, t2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n          # split-K / LN / colsum reductions have a fixed order (no atomics)


@pytest.mark.parametrize("name", ["vitb_t8", "vits_t8"])
def test_bf16_step_close_to_reference(name):
    """bf16 storage / fp32 accumulate: not gated at 1e-3; bound the deviation and check the matching agrees."""
    fx, cfg, B = gu.load(name)
    model = build(cfg, "bf16")
    out, total, logits, ld, grads, match = run_step(model, cfg, B)
    e_logit = gu.rel(out[2][0].detach().float().cpu(), fx["slots_head"])
    e_total = abs(float(total) - float(fx["total_loss"])) / abs(float(fx["total_loss"]))
    names = [str(n) for n in fx["param_names"]]
    gn = np.array([float(grads[n].double().norm()) for n in names])
    e_gn = np.abs(gn - fx["grad_norms"]) / np.maximum(fx["grad_norms"], 1e-6 * fx["grad_norms"].max())
    print(f"{name} bf16: logits rel {e_logit:.3e}, total loss rel {e_total:.3e}, grad-norm rel median {np.median(e_gn):.3e} max {e_gn.max():.3e}")
    assert e_logit < 5e-2 and e_total < 2e-2 and np.median(e_gn) < 5e-2
    assert torch.isfinite(total).all()


def test_surface_attributes_used_by_the_reference_driver():
    """attributes run_slot_finetuning.py reads (:433,475-479,532,541) and the misspelt kwarg it passes (:386)"""
    from devias_amd import create_model
    m = create_model("slot_vit_base_patch16_224", pretrained=False, num_classes=400, all_frames=16, tubelet_size=2, fc_drop_rate=0.0,
                     drop_rate=0.0, drop_path_rate=0.0, attn_drop_rate=0.0, drop_block_rate=None, use_checkpoint=False,
                     init_scale=0.001, num_latents=2, head_type="linear", slot_matching="matching", agg_weights_tie=True,
                     agg_depth=8, num_scene_classes=365)
    assert m.patch_embed.patch_size == (16, 16) and m.patch_embed.num_patches == 1568 and m.patch_embed.tubelet_size == 2
    assert tuple(m.pos_embed.shape) == (1, 1568, 768) and m.get_num_layers() == 12
    assert m.no_weight_decay() == {"pos_embed", "cls_token"} and m.slot_matching_method == "matching"
    with pytest.raises(ValueError):
        create_model("slot_vit_base_patch16_224", slot_matching_method="bogus")
    with pytest.raises(AssertionError):
        m.cuda()(torch.zeros(1, 3, 16, 112, 112, device="cuda"))


def test_teacher_forward_matches_reference_golden():
    """frozen cls-token scene teacher (model/modeling_finetune.py), N+1 = 785 tokens: fp32 within 1e-3, bf16 loosely"""
    from devias_amd.modeling_finetune import vit_base_patch16_224
    fx = dict(np.load(gu.GOLDEN_DIR + "/teacher_vitb_t8.npz"))
    x = synth.video(2, 8, 224, seed=1000).cuda()
    for mode, tol in (("fp32", 1e-3), ("bf16", 5e-2)):
        m = vit_base_patch16_224(num_classes=365, all_frames=8, tubelet_size=2, use_mean_pooling=False, init_scale=1e-3,
                                 compute_dtype=mode)
        synth.fill_module_(m, seed=1)
        m = m.cuda().eval()
        names = sorted(n for n, _ in m.named_parameters())
        assert names == sorted(ref_cpu.teacher_param_shapes(ref_cpu.SlotViTConfig(all_frames=8)).keys())
        tok, logits = m(x, return_attn=False)
        e1, e2 = gu.rel(tok.float().cpu(), fx["token"]), gu.rel(logits.float().cpu(), fx["logits"])
        print(f"teacher {mode}: token {e1:.2e} logits {e2:.2e}")
        assert e1 < tol and e2 < tol


def test_train_class_batch_with_teacher_and_fused_adamw():
    """engine.train_class_batch with a teacher MODULE + one FusedAdamW step == torch.optim.AdamW on the same gradients"""
    from devias_amd.engine_for_slot import train_class_batch
    from devias_amd.modeling_finetune import vit_base_patch16_224
    from devias_amd.optim import FusedAdamW
    from devias_amd.train_loss import TrainLoss
    fx, cfg, B = gu.load("vitb_t8")
    model = build(cfg, "fp32")
    teacher = vit_base_patch16_224(num_classes=365, all_frames=8, use_mean_pooling=False, init_scale=1e-3, compute_dtype="fp32")
    synth.fill_module_(teacher, seed=1)
    teacher = teacher.cuda().eval()
    x, y, tl, fg = gu.inputs(cfg, B)
    crit = TrainLoss(scene_criterion="KL", num_action_classes=400, slot_matching_method="matching", scene_loss_weight=4000,
                     mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0)
    loss, out, ld = train_class_batch(model, teacher, x.cuda(), y.cuda(), crit, fg_mask=(fg[0].cuda(), fg[1].cuda()))
    assert torch.isfinite(loss).all() and out.shape == (B, 765) and all(isinstance(v, float) for v in ld.values())
    loss.backward()
    ref = [p.detach().clone().requires_grad_(True) for p in model.parameters()]
    for r, p in zip(ref, model.parameters()):
        r.grad = p.grad.clone()
    topt = torch.optim.AdamW(ref, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    fopt = FusedAdamW(model.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    topt.step(); fopt.step()
    worst = max(gu.rel(p.detach().cpu(), r.detach().cpu()) for p, r in zip(model.parameters(), ref))
    assert worst < 1e-6, worst


def test_drop_path_matches_oracle_with_the_same_masks():
    """stochastic depth (timm drop_path): with the SAME per-sample masks the fused row-scale epilogue path must equal the oracle
    block evaluated with those masks, forward and backward (fp32)"""
    from devias_amd.functions import EncoderBlockFn
    from devias_amd.weight_cache import _f32
    cfg = ref_cpu.SlotViTConfig(all_frames=2, embed_dim=384, num_heads=6, depth=1)
    B, N, D = 3, cfg.num_patches, cfg.embed_dim
    shapes = {k: v for k, v in ref_cpu.param_shapes(cfg).items() if k.startswith("blocks.0.")}
    P = synth.fill_params(shapes, seed=5)
    x = synth.param_values("dp.x", (B, N, D), seed=6) * 20
    ds = torch.tensor([[0.0, 1 / 0.8, 1 / 0.8], [1 / 0.8, 0.0, 1 / 0.8]])
    # oracle with masks
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xg = x.clone().requires_grad_(True)
    p = "blocks.0."
    import torch.nn.functional as F
    u = F.layer_norm(xg, (D,), Pg[p + "norm1.weight"], Pg[p + "norm1.bias"], 1e-6)
    bias = torch.cat([Pg[p + "attn.q_bias"], torch.zeros(D), Pg[p + "attn.v_bias"]])
    qkv = F.linear(u, Pg[p + "attn.qkv.weight"], bias).reshape(B, N, 3, 6, 64).permute(2, 0, 3, 1, 4)
    att = ((qkv[0] * 0.125) @ qkv[1].transpose(-2, -1)).softmax(-1)
    o = (att @ qkv[2]).transpose(1, 2).reshape(B, N, D)
    x1 = xg + ds[0].view(B, 1, 1) * F.linear(o, Pg[p + "attn.proj.weight"], Pg[p + "attn.proj.bias"])
    h = F.gelu(F.linear(F.layer_norm(x1, (D,), Pg[p + "norm2.weight"], Pg[p + "norm2.bias"], 1e-6), Pg[p + "mlp.fc1.weight"], Pg[p + "mlp.fc1.bias"]))
    x2 = x1 + ds[1].view(B, 1, 1) * F.linear(h, Pg[p + "mlp.fc2.weight"], Pg[p + "mlp.fc2.bias"])
    w = synth.param_values("dp.w", (B, N, D), seed=7)
    (x2 * w).sum().backward()
    # HIP path
    order = ["norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.q_bias", "attn.v_bias", "attn.proj.weight", "attn.proj.bias",
             "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"]
    Pc = [P[p + k].cuda().requires_grad_(True) for k in order]
    xc = x.reshape(B * N, D).cuda().requires_grad_(True)
    dsc = ds.cuda().contiguous()
    y = EncoderBlockFn.apply(xc, *Pc, (B, N, 6, 1e-6, torch.float32), dsc[0], dsc[1])
    (y * w.reshape(B * N, D).cuda()).sum().backward()
    assert gu.rel(y.detach().cpu().view(B, N, D), x2.detach()) < 1e-5
    assert gu.rel(xc.grad.cpu().view(B, N, D), xg.grad) < 1e-4
    for k, t_ in zip(order, Pc):
        assert gu.rel(t_.grad.cpu(), Pg[p + k].grad) < 2e-4, k
    # and the module-level switch draws masks only in training mode
    from devias_amd.modeling_slot import VisionTransformer
    m = VisionTransformer(embed_dim=384, num_heads=6, depth=2, qkv_bias=True, num_classes=400, all_frames=2, num_latents=2,
                          agg_weights_tie=True, agg_depth=2, slot_matching_method="matching", drop_path_rate=0.5, compute_dtype="fp32").cuda()
    xin = synth.video(2, 2, 224).cuda()
    m.eval(); a = m(xin)[2][1]; b_ = m(xin)[2][1]          # slots (the head is zero-initialised with init_scale=0)
    assert torch.equal(a, b_)
    m.train(); torch.manual_seed(0); c = m(xin)[2][1]; d = m(xin)[2][1]
    assert not torch.equal(c, d)


@pytest.mark.parametrize("kw", [dict(embed_dim=1024, num_heads=16, depth=2, all_frames=4),            # ViT-L width (BASELINE config 4)
                                dict(embed_dim=768, num_heads=12, depth=1, all_frames=4, img_size=320),   # 320^2 frames (config 5 geometry)
                                dict(embed_dim=384, num_heads=6, depth=2, all_frames=2, num_latents=3, agg_depth=3),
                                dict(embed_dim=384, num_heads=6, depth=2, all_frames=2, num_latents=5, agg_depth=2),       # 5 slots: the unfolded AggBlockFn, tied ...
                                dict(embed_dim=384, num_heads=6, depth=2, all_frames=2, num_latents=5, agg_depth=2, agg_weights_tie=False)])   # ... and one weight set per layer
def test_fp32_step_matches_oracle_other_geometries(kw):
    """geometries the goldens do not cover (ViT-L width, 320x320 frames -> 400-cell mask grid, 3 slots, 5 slots: more than the folded slot attention
    takes, so the unfolded form runs): HIP fp32 vs the CPU oracle on the same formula weights/inputs, outputs + loss + every gradient"""
    from functools import partial
    from devias_amd.modeling_slot import VisionTransformer
    from devias_amd.train_loss import TrainLoss
    cfg = ref_cpu.SlotViTConfig(**kw)
    B = 2
    m = VisionTransformer(img_size=cfg.img_size, patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads,
                          mlp_ratio=4, qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_classes=400,
                          all_frames=cfg.all_frames, init_scale=1e-3, num_latents=cfg.num_latents, slot_matching_method="matching",
                          agg_weights_tie=cfg.agg_weights_tie, agg_depth=cfg.agg_depth, compute_dtype="fp32")
    synth.fill_module_(m, seed=0)
    m = m.cuda().train()
    x, y, tl, fg = gu.inputs(cfg, B)
    crit = TrainLoss(scene_criterion="KL", num_action_classes=400, slot_matching_method="matching", scene_loss_weight=4000,
                     mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0)
    out = m(x.cuda())
    total, logits, ld = crit(m, out, (None, tl.cuda()), y.cuda(), fg_mask=(fg[0].cuda(), fg[1].cuda()))
    total.backward()
    P = synth.fill_params(ref_cpu.param_shapes(cfg), seed=0)
    ototal, ologits, old, ograds, oout, oidx = ref_cpu.train_step(P, cfg, x, y, tl, fg)
    assert gu.rel(out[2][0].detach().cpu(), oout[2][0].detach()) < 1e-3
    assert gu.rel(out[2][2].detach().cpu(), oout[2][2].detach()) < 1e-3 and out[2][2].shape[1] == cfg.grid ** 2
    assert gu.rel(out[1][2].detach().cpu(), oout[1][2].detach()) < 1e-3
    assert abs(float(total) - float(ototal)) / abs(float(ototal)) < 1e-3
    assert crit.last_match.cpu().tolist() == [[int(a), int(b)] for a, b in zip(oidx[0], oidx[1])]
    gmax = max(float(g.abs().max()) for g in ograds.values())
    for n, p in m.named_parameters():
        e = float((p.grad.cpu().double() - ograds[n].double()).abs().max() / max(float(ograds[n].abs().max()), 1e-6 * gmax))
        assert e < 5e-3, (n, e)


def test_validation_one_epoch_and_final_test(tmp_path):
    """engine/engine_for_slot.py:215-303: eval forward, CE on the selected action logits, top-1/5; compared with the same
    metrics computed from the ORACLE's forward of the same clips (fp32)"""
    from devias_amd.engine_for_slot import final_test, validation_one_epoch
    fx, cfg, B = gu.load("vits_t8")
    model = build(cfg, "fp32")
    x, y, tl, fg = gu.inputs(cfg, B)
    P = synth.fill_params(ref_cpu.param_shapes(cfg), seed=0)
    with torch.no_grad():
        out = ref_cpu.student_forward(P, cfg, x)
    logits = out[1][0].float()
    ce = float(torch.nn.functional.cross_entropy(logits, y, reduction="mean"))
    top = logits.topk(5, dim=1).indices
    acc1 = 100.0 * float((top[:, :1] == y[:, None]).any(1).float().mean())
    acc5 = 100.0 * float((top == y[:, None]).any(1).float().mean())
    loader = [(x, y), (x, y)]
    st = validation_one_epoch(loader, model, "cuda")
    assert abs(st["loss"] - ce) < 1e-4 * abs(ce) and st["acc1"] == acc1 and st["acc5"] == acc5
    f = tmp_path / "final.txt"
    ids = ["vid%d" % i for i in range(B)]
    st2 = final_test([(x, y, ids, torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.int64))], model, "cuda", str(f))
    lines = f.read_text().splitlines()
    assert len(lines) == 1 + B and lines[1].startswith("vid0 [") and lines[1].endswith(" %d 0 1" % int(y[0]))
    assert abs(st2["loss"] - ce) < 1e-4 * abs(ce)


def test_knn_classifier_matches_reference():
    """utils/eval/run_knn.py:123-163 on formula features: top-1/top-5 of the reference function (tests/golden/knn.json)"""
    import json
    from devias_amd.eval_knn import knn_classifier
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "knn.json")))
    n_train, n_test, D, C = g["n_train"], g["n_test"], g["D"], g["C"]
    lab_tr = torch.from_numpy((synth.hash_u64(5, "knn.lab.train", n_train) % np.uint64(C)).astype(np.int64))
    lab_te = torch.from_numpy((synth.hash_u64(5, "knn.lab.test", n_test) % np.uint64(C)).astype(np.int64))
    cent = synth.param_values("knn.centroids.weight", (C, D), seed=5) * 20
    f_tr = torch.nn.functional.normalize(cent[lab_tr] + synth.param_values("knn.noise.train.weight", (n_train, D), seed=5) * 110, dim=1)
    f_te = torch.nn.functional.normalize(cent[lab_te] + synth.param_values("knn.noise.test.weight", (n_test, D), seed=5) * 110, dim=1)
    for case in g["cases"]:
        t1, t5 = knn_classifier(f_tr.cuda(), lab_tr.cuda(), f_te.cuda(), lab_te.cuda(), case["k"], case["T"], num_classes=C)
        assert abs(t1 - case["top1"]) <= 0.9 and abs(t5 - case["top5"]) <= 0.9, (case, t1, t5)     # <= 2 of 230 borderline votes (fp32 summation order)


def test_short_training_run_decreases_the_loss():
    """integration: train_one_epoch (FAME masks, teacher logits as a tensor, layer-decay groups, cosine LR with warm-up, clipped fused
    AdamW) on a fixed batch of 4 clips for 12 steps in bf16 -- the loss must stay finite and fall at every step"""
    import types
    import devias_amd
    from devias_amd import optim_factory as of
    from devias_amd.engine_for_slot import train_class_batch
    from devias_amd.train_loss import TrainLoss
    model = devias_amd.create_model("slot_vit_small_patch16_224", num_classes=400, all_frames=4, num_latents=2, slot_matching_method="matching",
                                    agg_weights_tie=True, agg_depth=2, num_scene_classes=365, compute_dtype="bf16")
    synth.fill_module_(model, seed=0)
    model = model.cuda().train()
    B = 4
    x = synth.scene_video(B, 4, 224).cuda()
    y = synth.targets(B, 400).cuda()
    tl = synth.teacher_logits(B, 365).cuda()
    fg = tuple(m.cuda() for m in synth.fg_masks(B, model.patch_embed.num_patches))
    crit = TrainLoss(scene_criterion="KL", num_action_classes=400, slot_matching_method="matching", scene_loss_weight=4000,
                     mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0)
    assigner = of.LayerDecayValueAssigner.from_decay(0.75, model.get_num_layers())
    args = types.SimpleNamespace(opt="adamw", lr=2e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=[0.9, 0.999])
    opt = of.create_optimizer(args, model, get_num_layer=assigner.get_layer_id, get_layer_scale=assigner.get_scale)
    sched = of.cosine_scheduler(2e-3, 1e-5, epochs=1, niter_per_ep=12, warmup_epochs=1, warmup_steps=2)
    losses = []
    for it in range(12):
        for g in opt.param_groups:
            g["lr"] = sched[it] * g["lr_scale"]
        opt.zero_grad(set_to_none=True)
        loss, out, ld = train_class_batch(model, tl, x, y, crit, fg_mask=fg)
        loss.backward()
        opt.step(max_norm=5.0)
        losses.append(float(loss.detach().float().sum()))
        assert np.isfinite(losses[-1]) and float(opt.last_grad_norm) > 0
    assert losses[-1] < losses[0] - 0.3 and all(b <= a + 1e-3 for a, b in zip(losses[1:], losses[2:])), losses     # falls every step after the lr = 0 warm-up step
