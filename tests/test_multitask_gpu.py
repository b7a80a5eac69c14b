"""The two-token multi-task baseline end to end on the GPU, both head modes: the fp32 step against the step the real reference ran (tests/golden/multitask_t8.npz,
multitask_unified_t8.npz; 1e-3 relative with golden_util's floor convention), the bf16 step against the fp32 mode element-wise (tests/grad_compare.py), the forward
without a graph, fc_dropout under two given masks, the optimizer through the engine and the evaluation loops."""
import ast
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden_util as gu
import grad_compare as gc
import multitask_ref as mr
from devias_amd import synth
from oracle import ref_cpu
from test_bf16_gradients_gpu import TOL_6400

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3          # the project's parity gate
# bf16 against the fp32 mode, ViT-B/16 8x224^2, B = 2: every family test_bf16_gradients_gpu.py bounds carries its bound for its plain B = 2 configuration (TOL_6400).
# The parameters outside its families borrow the bound of the family that sums the same kind of quantity -- none is taken from a run of this model:
#   cls_token, scene_token   the sum over the clips of the first block's input gradient at one row -- what patch_embed.proj.bias sums over all rows: 'patch_embed'
#   scene_head.*             a linear head on a normalised token, as head.* is: the 'head' family
BORROWED = {"cls_token": "patch_embed", "scene_token": "patch_embed", "scene_head.weight": "head", "scene_head.bias": "head"}
MODES = ("multitask", "multitask_unified")


def _fx(mode):
    fx = dict(np.load(gu.GOLDEN_DIR + f"/{mode}_t8.npz", allow_pickle=False))
    return fx, ast.literal_eval(str(fx["config"])), int(fx["batch"])


def _build(cfg, dtype, **kw):
    from devias_amd.modeling_multi_task import disentangle_vit_base_patch16_224
    m = disentangle_vit_base_patch16_224(**dict(cfg, compute_dtype=dtype, **kw))
    synth.fill_module_(m, seed=0)
    return m.to(DEV).train()


def _criterion(fx, cfg, **kw):
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.multi_task_loss import TrainLoss
    return TrainLoss(LabelSmoothingCrossEntropy(float(fx["smoothing"])), str(fx["logit_criterion"]), unified_head=cfg["unified_head"],
                     num_action_classes=cfg["num_classes"], logit_criterion_weight=float(fx["logit_criterion_weight"]), **kw)


def _step(model, crit, x, y, teacher):
    model.zero_grad(set_to_none=True)
    out = model(x)
    (ta, za), (ts, zs) = out
    total, action_logit, ld = crit(out, (None, teacher), y)
    assert action_logit is za
    total.backward()
    torch.cuda.synchronize()
    return SimpleNamespace(ta=ta.detach().clone(), ts=ts.detach().clone(), za=za.detach().clone(), zs=zs.detach().clone(), loss=total.detach().clone(), ld=ld,
                           graph=za.grad_fn is not None and zs.grad_fn is not None, grads={n: p.grad.detach().clone() for n, p in model.named_parameters()})


@pytest.fixture(scope="module", params=MODES)
def steps(request):
    """the fp32-mode step, its forwards without a graph, and the bf16 step of one head mode's fixture, computed once"""
    from devias_amd import ops
    fx, cfg, B = _fx(request.param)
    x = synth.video(B, cfg["all_frames"], 224, seed=1000).to(DEV)
    y = synth.targets(B, cfg["num_classes"], seed=1000).to(DEV)
    teacher = torch.from_numpy(fx["teacher"]).to(DEV)
    out = SimpleNamespace(mode=request.param, fx=fx, cfg=cfg, B=B, x=x, y=y, teacher=teacher)
    for dtype in ("fp32", "bf16"):
        m = _build(cfg, dtype)
        ops.counters(reset=True)
        s = _step(m, _criterion(fx, cfg), x, y, teacher)
        s.launches = ops.two_token_head_launches()          # the forward, the backward
        m.eval()
        ops.counters(reset=True)
        ev = m(x)                                   # eval(), autograd ON: tensors without a graph
        s.eval = ([t.clone() for pair in ev for t in pair], all(t.grad_fn is None and not t.requires_grad for pair in ev for t in pair), ops.two_token_head_launches())
        m.train()
        with torch.no_grad():
            ng = m(x)
        s.nograd = [t.clone() for pair in ng for t in pair]
        setattr(out, "s" + dtype[-2:], s)
        del m
        torch.cuda.empty_cache()
    return out


def test_fp32_step_against_the_reference(steps):
    fx, s = steps.fx, steps.s32
    assert s.graph
    errs = {"action_token": gu.rel(s.ta.float().cpu(), fx["action_token"]), "scene_token": gu.rel(s.ts.float().cpu(), fx["scene_token"]),
            "action_logits": gu.rel(s.za.float().cpu(), fx["action_logits"]), "scene_logits": gu.rel(s.zs.float().cpu(), fx["scene_logits"]),
            "loss": abs(float(s.loss) - float(fx["loss"])) / abs(float(fx["loss"])),
            "action_loss": abs(s.ld["action_loss"] - float(fx["action_loss"])) / abs(float(fx["action_loss"])),
            "logit_loss": abs(s.ld["logit_loss"] - float(fx["logit_loss"])) / abs(float(fx["logit_loss"]))}
    names = [str(n) for n in fx["param_names"]]
    assert names == list(s.grads)
    nmax = float(fx["grad_norms"].max())
    for i, n in enumerate(names):
        g = s.grads[n].float().cpu()
        ref_norm = float(fx["grad_norms"][i])
        errs[n + ".norm"] = abs(float(g.double().norm()) - ref_norm) / max(ref_norm, 1e-6 * nmax)
        smp = g.reshape(-1)[torch.from_numpy(gu.sample_idx(n, g.numel()))].double().numpy()
        ref_s = fx["grad_samples"][i].astype(np.float64)
        errs[n + ".samples"] = float(np.abs(smp - ref_s).max() / max(np.abs(ref_s).max(), 1e-6 * nmax, 1e-30))
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print("[%s fp32 vs reference] tokens %.2e %.2e logits %.2e %.2e loss %.2e; worst: %s" % (
        steps.mode, errs["action_token"], errs["scene_token"], errs["action_logits"], errs["scene_logits"], errs["loss"], ", ".join("%s %.2e" % kv for kv in worst)))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


def test_bf16_step_against_the_fp32_mode(steps):
    a, r = steps.s16, steps.s32
    own = [n for n in r.grads if n not in BORROWED]
    gc.check({n: a.grads[n] for n in own}, {n: r.grads[n] for n in own}, TOL_6400, f"{steps.mode} bf16 B=2")
    new = [n for n in r.grads if n in BORROWED]
    assert new == ["cls_token", "scene_token"] + ([] if steps.cfg["unified_head"] else ["scene_head.weight", "scene_head.bias"])
    errs = gc.compare({n: a.grads[n] for n in new}, {n: r.grads[n] for n in new})
    for n, e in errs.items():
        print(f"[grad] {steps.mode} bf16 B=2  rel {e.rel:.2e}  cos {e.cos:.8f}  blk64 {e.blk:.2e}  ({n}; bound {TOL_6400[BORROWED[n]]:.1e} of '{BORROWED[n]}')")
    bad = {n: e.worst for n, e in errs.items() if not e.worst <= TOL_6400[BORROWED[n]]}
    assert not bad, bad


def test_forward_without_a_graph(steps):
    """zero drop rates: no_grad in training mode and eval() with autograd on both give the training forward's bits (the forward-only blocks, the region without a
    save arena); the region's counter moves once per call"""
    for s in (steps.s32, steps.s16):
        outs, graphless, launches = s.eval
        assert s.launches == 2 and graphless and launches == 1
        for got, got2, want in zip(outs, s.nograd, (s.ta, s.za, s.ts, s.zs)):
            assert torch.equal(got, want) and torch.equal(got2, want)


class _GivenMasks:
    """a DropoutSource that hands out the two fc_dropout masks it was given"""

    def __init__(self, masks):
        self.masks, self.asked = masks, []

    def element_mask(self, kind, block, shape, keep, device):
        self.asked.append((kind, block, tuple(shape), keep))
        return self.masks[kind].to(device)


@pytest.mark.parametrize("unified", [False, True], ids=["separate", "unified"])
def test_fc_dropout_under_two_given_masks_matches_the_restatement(unified):
    """a small model (D = 384, depth 2, 2 frames): fc_drop_rate = 0.5 with the SAME two masks in multitask_ref, fp32, forward and every gradient"""
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.modeling_multi_task import VisionTransformer
    from devias_amd.multi_task_loss import TrainLoss
    from functools import partial
    B, Ca, Cs = 3, 101, 37
    cfg = ref_cpu.SlotViTConfig(all_frames=2, embed_dim=384, num_heads=6, depth=2)
    m = VisionTransformer(embed_dim=384, num_heads=6, depth=2, qkv_bias=True, num_classes=Ca, num_scene_classes=Cs, all_frames=2, fc_drop_rate=0.5, init_scale=1.0,
                          norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), unified_head=unified, compute_dtype="fp32")
    synth.fill_module_(m, seed=3)
    g = torch.Generator().manual_seed(11)
    masks = {k: ((torch.rand((B, 384), generator=g) < 0.5).float() * 2.0).contiguous() for k in ("head", "scene_head")}
    assert not torch.equal(masks["head"], masks["scene_head"])
    x, y = synth.video(B, 2, 224, seed=5), synth.targets(B, Ca, seed=5)
    teacher = torch.randn((B, Cs), generator=g) * 3.0
    P = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    (rta, rza), (rts, rzs) = mr.forward(P, cfg, x, masks["head"], masks["scene_head"])
    mr.train_loss(rza, rzs, teacher, y, 0.1, "KL", unified, Ca, 2.0)[0].backward()
    m = m.to(DEV).train()
    m.dropout_source = _GivenMasks(masks)
    out = m(x.to(DEV))
    (ta, za), (ts, zs) = out
    TrainLoss(LabelSmoothingCrossEntropy(0.1), "KL", unified_head=unified, num_action_classes=Ca, logit_criterion_weight=2.0)(out, (None, teacher.to(DEV)), y.to(DEV))[0].backward()
    assert m.dropout_source.asked == [("head", -2, (B, 384), 0.5), ("scene_head", -3, (B, 384), 0.5)]
    errs = {"action_token": gu.rel(ta.detach().cpu(), rta.detach()), "scene_token": gu.rel(ts.detach().cpu(), rts.detach()),
            "action_logits": gu.rel(za.detach().cpu(), rza.detach()), "scene_logits": gu.rel(zs.detach().cpu(), rzs.detach())}
    errs.update({n: gu.rel(p.grad.cpu(), P[n].grad) for n, p in m.named_parameters()})
    print("[multitask fc_dropout %s] worst: %s" % ("unified" if unified else "separate", ", ".join("%s %.2e" % kv for kv in sorted(errs.items(), key=lambda kv: -kv[1])[:4])))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


def test_two_optimizer_steps_through_the_engine(steps):
    """train_one_epoch(model, scene_model, TrainLoss, ...) over a four-batch loader with update_freq = 2 and the fused AdamW: two optimizer steps, every parameter
    moves, the frozen cls-token teacher does not"""
    from devias_amd import engine_for_multi_task as eng
    from devias_amd.modeling_finetune import vit_base_patch16_224
    from devias_amd.optim import FusedAdamW
    model = _build(steps.cfg, "bf16")
    teacher = vit_base_patch16_224(num_classes=steps.cfg["num_scene_classes"], all_frames=steps.cfg["all_frames"], tubelet_size=2, init_scale=1.0, use_mean_pooling=False,
                                   compute_dtype="bf16")
    synth.fill_module_(teacher, seed=1)
    teacher = teacher.to(DEV)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    t_before = {n: p.detach().clone() for n, p in teacher.named_parameters()}
    opt = FusedAdamW(list(model.parameters()), lr=1e-3, weight_decay=0.05)
    loader = [(synth.video(steps.B, steps.cfg["all_frames"], 224, seed=2000 + i), synth.targets(steps.B, steps.cfg["num_classes"], seed=2000 + i), None, None) for i in range(4)]
    stats = eng.train_one_epoch(model, teacher, _criterion(steps.fx, steps.cfg), loader, opt, DEV, 0, max_norm=5.0, update_freq=2, check_finite_every=4)
    assert np.isfinite(stats["loss"]) and np.isfinite(stats["action_loss"]) and np.isfinite(stats["logit_loss"]) and stats["logit_loss"] > 0
    assert not teacher.training and model.training
    still = [n for n, p in model.named_parameters() if torch.equal(p.detach(), before[n])]
    assert not still, still
    assert all(torch.equal(p.detach(), t_before[n]) for n, p in teacher.named_parameters())


def test_evaluation_loops_score_the_right_logits(steps, tmp_path):
    """validation_one_epoch / final_test on the action logits, final_test_with_scene_label on the scene logits (cut to the scene classes under the unified head)
    against the teacher's argmax: the returned means against values computed directly from the model's outputs, the file lines against merge"""
    from devias_amd import engine_for_multi_task as eng
    cfg, B, unified = steps.cfg, steps.B, steps.cfg["unified_head"]
    model = _build(cfg, "bf16")

    class Teacher(torch.nn.Module):          # a frozen scene model with known logits per clip: (token, logits)
        def forward(self, x, return_attn=False):
            m = x.float().mean(dim=(1, 2, 3, 4))
            return m[:, None], torch.sin(m[:, None] * 50.0 + torch.arange(cfg["num_scene_classes"], device=x.device)[None, :])

    teacher = Teacher()
    clips = [synth.video(B, cfg["all_frames"], 224, seed=3000 + i) for i in range(2)]
    targets = [synth.targets(B, cfg["num_classes"], seed=3000 + i) for i in range(2)]
    loader = [(c, t, ["vid%d_%d" % (i, j) for j in range(B)], torch.zeros(B, dtype=torch.int64), torch.arange(B)) for i, (c, t) in enumerate(zip(clips, targets))]
    model.eval()
    with torch.no_grad():
        outs = [model(c.to(DEV)) for c in clips]
        za = torch.cat([o[0][1] for o in outs]).float().cpu()
        zs = torch.cat([o[1][1] for o in outs]).float().cpu()[:, (cfg["num_classes"] if unified else 0):]
        ys = torch.cat([teacher(c.to(DEV))[1].argmax(1) for c in clips]).cpu()
    y = torch.cat(targets)

    def want(z, t):
        return {"loss": float(torch.nn.functional.cross_entropy(z, t)), "acc1": 100.0 * float((z.argmax(1) == t).float().mean()),
                "acc5": 100.0 * float((z.topk(5, 1)[1] == t[:, None]).any(1).float().mean())}

    val = eng.validation_one_epoch(loader, model, DEV)
    assert set(val) == {"loss", "acc1", "acc5"} and all(abs(val[k] - v) <= 1e-4 * max(1.0, abs(v)) for k, v in want(za, y).items()), (val, want(za, y))
    fin = eng.final_test(loader, model, DEV, str(tmp_path / "0.txt"))
    assert fin == val
    rows = (tmp_path / "0.txt").read_text().splitlines()
    assert len(rows) == 1 + 2 * B and rows[1] == "vid0_0 {} {} 0 0".format(str(za[0].numpy().tolist()), int(y[0]))
    top1, top5 = eng.merge(str(tmp_path), 1)[:2]
    assert abs(top1 - fin["acc1"]) < 1e-9 and abs(top5 - fin["acc5"]) < 1e-9
    sdir = tmp_path / "scene"
    sdir.mkdir()
    sc = eng.final_test_with_scene_label(loader, model, teacher, DEV, str(sdir / "0.txt"), num_labels=cfg["num_classes"], unified_head=unified)
    assert all(abs(sc[k] - v) <= 1e-4 * max(1.0, abs(v)) for k, v in want(zs, ys).items()), (sc, want(zs, ys))
    srows = (sdir / "0.txt").read_text().splitlines()
    assert len(srows) == 1 + 2 * B and srows[1] == "vid0_0 {} {} 0 0".format(str(zs[0].numpy().tolist()), int(ys[0]))
    assert zs.shape[1] == cfg["num_scene_classes"] and abs(eng.merge(str(sdir), 1)[0] - sc["acc1"]) < 1e-9
