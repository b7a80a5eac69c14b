"""The plain video ViT end to end on the GPU, both pool modes: the fp32 step against the step the real reference ran (tests/golden/plainvit_{mean,cls}_t8.npz, 1e-3
relative with golden_util's floor convention), the bf16 step against the fp32 mode element-wise (tests/grad_compare.py), the forward without a graph, fc_dropout under
a given mask, the optimizer and the scene engine."""
import ast
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden_util as gu
import grad_compare as gc
import plainvit_ref as pr
from devias_amd import synth
from oracle import ref_cpu
from test_bf16_gradients_gpu import TOL_6400

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3          # the project's parity gate
# bf16 against the fp32 mode, ViT-B/16 8x224^2, B = 2: every family test_bf16_gradients_gpu.py bounds carries its bound for its plain B = 2 configuration (TOL_6400).
# The parameters outside its families borrow the bound of the family that sums the same kind of quantity -- none is taken from a run of this model:
#   fc_norm.*   a LayerNorm's weight / bias gradient, summed over rows: the 'norm' family
#   cls_token   the sum over the clips of the first block's input gradient at one row -- what patch_embed.proj.bias sums over all rows: the 'patch_embed' family
BORROWED = {"fc_norm.weight": "norm", "fc_norm.bias": "norm", "cls_token": "patch_embed"}
MODES = ("mean", "cls")


def _fx(mode):
    fx = dict(np.load(gu.GOLDEN_DIR + f"/plainvit_{mode}_t8.npz", allow_pickle=False))
    return fx, ast.literal_eval(str(fx["config"])), int(fx["batch"])


def _build(cfg, dtype, **kw):
    from devias_amd.modeling_finetune import vit_base_patch16_224
    m = vit_base_patch16_224(**dict(cfg, compute_dtype=dtype, **kw))
    synth.fill_module_(m, seed=0)
    return m.to(DEV).train()


def _step(model, x, y, smoothing):
    from devias_amd.losses import LabelSmoothingCrossEntropy
    model.zero_grad(set_to_none=True)
    token, logits = model(x)
    loss = LabelSmoothingCrossEntropy(smoothing)(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return SimpleNamespace(token=token.detach().clone(), logits=logits.detach().clone(), loss=loss.detach().clone(), graph=logits.grad_fn is not None,
                           grads={n: p.grad.detach().clone() for n, p in model.named_parameters()})


@pytest.fixture(scope="module", params=MODES)
def steps(request):
    """the fp32-mode step, its forward without a graph, and the bf16 step of one pool mode's fixture, computed once"""
    from devias_amd import ops
    fx, cfg, B = _fx(request.param)
    x = synth.video(B, cfg["all_frames"], 224, seed=1000).to(DEV)
    y = synth.targets(B, cfg["num_classes"], seed=1000).to(DEV)
    out = SimpleNamespace(mode=request.param, fx=fx, cfg=cfg, B=B, x=x, y=y)
    for dtype in ("fp32", "bf16"):
        m = _build(cfg, dtype)
        s = _step(m, x, y, float(fx["smoothing"]))
        m.eval()
        ops.counters(reset=True)
        ev = m(x)                                   # eval(), autograd ON: tensors without a graph
        s.eval = (ev[0].clone(), ev[1].clone(), ev[1].grad_fn is None and not ev[1].requires_grad, ops.pool_head_launches())
        m.train()
        with torch.no_grad():
            ng = m(x)
        s.nograd = (ng[0].clone(), ng[1].clone())
        setattr(out, "s" + dtype[-2:], s)
        del m
        torch.cuda.empty_cache()
    return out


def test_fp32_step_against_the_reference(steps):
    fx, s = steps.fx, steps.s32
    assert s.graph
    errs = {"token": gu.rel(s.token.float().cpu(), fx["token"]), "logits": gu.rel(s.logits.float().cpu(), fx["logits"]),
            "loss": abs(float(s.loss) - float(fx["loss"])) / abs(float(fx["loss"]))}
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
    print("[plainvit %s fp32 vs reference] token %.2e logits %.2e loss %.2e; worst: %s" % (steps.mode, errs["token"], errs["logits"], errs["loss"],
                                                                                         ", ".join("%s %.2e" % kv for kv in worst)))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


def test_bf16_step_against_the_fp32_mode(steps):
    a, r = steps.s16, steps.s32
    own = [n for n in r.grads if n not in BORROWED]
    gc.check({n: a.grads[n] for n in own}, {n: r.grads[n] for n in own}, TOL_6400, f"plainvit {steps.mode} bf16 B=2")
    new = [n for n in r.grads if n in BORROWED]
    assert new == (["fc_norm.weight", "fc_norm.bias"] if steps.mode == "mean" else ["cls_token"])
    errs = gc.compare({n: a.grads[n] for n in new}, {n: r.grads[n] for n in new})
    for n, e in errs.items():
        print(f"[grad] plainvit {steps.mode} bf16 B=2  rel {e.rel:.2e}  cos {e.cos:.8f}  blk64 {e.blk:.2e}  ({n}; bound {TOL_6400[BORROWED[n]]:.1e} of '{BORROWED[n]}')")
    bad = {n: e.worst for n, e in errs.items() if not e.worst <= TOL_6400[BORROWED[n]]}
    assert not bad, bad


def test_forward_without_a_graph(steps):
    """zero drop rates: no_grad in training mode and eval() with autograd on both give the training forward's bits in mean-pooling mode (the forward-only blocks,
    the region without a save arena); an eval() cls model takes the frozen teacher's path: no graph, the new counter untouched"""
    for s in (steps.s32, steps.s16):
        tok, logits, graphless, launches = s.eval
        assert graphless
        if steps.mode == "mean":
            assert torch.equal(s.nograd[0], s.token) and torch.equal(s.nograd[1], s.logits)
            assert torch.equal(tok, s.token) and torch.equal(logits, s.logits)
            assert launches == 1
        else:
            assert launches == 0
            assert torch.equal(s.nograd[0], tok) and torch.equal(s.nograd[1], logits)          # no_grad: the frozen path too
            if s is steps.s32:          # padded full-tile kernels against the unpadded training path: other kernels, the same arithmetic, at the parity gate
                assert gu.rel(tok.float().cpu(), s.token.float().cpu()) <= TOL and gu.rel(logits.float().cpu(), s.logits.float().cpu()) <= TOL


class _GivenMasks:
    """a DropoutSource that hands out the fc_dropout mask it was given"""

    def __init__(self, mask):
        self.mask, self.asked = mask, []

    def element_mask(self, kind, block, shape, keep, device):
        self.asked.append((kind, block, tuple(shape), keep))
        return self.mask.to(device)


@pytest.mark.parametrize("mean_pooling", [True, False], ids=MODES)
def test_fc_dropout_under_a_given_mask_matches_the_restatement(mean_pooling):
    """a small model (D = 384, depth 2, 2 frames): fc_drop_rate = 0.5 with the SAME mask in plainvit_ref, fp32, forward and every gradient"""
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.modeling_finetune import VisionTransformer
    from functools import partial
    B, C = 3, 101
    cfg = ref_cpu.SlotViTConfig(all_frames=2, embed_dim=384, num_heads=6, depth=2)
    m = VisionTransformer(embed_dim=384, num_heads=6, depth=2, qkv_bias=True, num_classes=C, all_frames=2, fc_drop_rate=0.5, init_scale=1.0,
                          norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), use_mean_pooling=mean_pooling, compute_dtype="fp32")
    synth.fill_module_(m, seed=3)
    g = torch.Generator().manual_seed(11)
    mask = ((torch.rand((B, 384), generator=g) < 0.5).float() * 2.0).contiguous()
    x, y = synth.video(B, 2, 224, seed=5), synth.targets(B, C, seed=5)
    P = {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters()}
    rtok, rlogits = pr.forward(P, cfg, x, mean_pooling, mask)
    pr.label_smoothing_ce(rlogits, y, 0.1).backward()
    m = m.to(DEV).train()
    m.dropout_source = _GivenMasks(mask)
    tok, logits = m(x.to(DEV))
    LabelSmoothingCrossEntropy(0.1)(logits, y.to(DEV)).backward()
    assert m.dropout_source.asked == [("head", -2, (B, 384), 0.5)]
    errs = {"token": gu.rel(tok.detach().cpu(), rtok.detach()), "logits": gu.rel(logits.detach().cpu(), rlogits.detach())}
    errs.update({n: gu.rel(p.grad.cpu(), P[n].grad) for n, p in m.named_parameters()})
    print("[plainvit fc_dropout %s] worst: %s" % (MODES[not mean_pooling], ", ".join("%s %.2e" % kv for kv in sorted(errs.items(), key=lambda kv: -kv[1])[:4])))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


def test_five_adamw_steps_lower_the_loss(steps):
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.optim import FusedAdamW
    model = _build(steps.cfg, "bf16")
    crit = LabelSmoothingCrossEntropy(0.1)
    opt = FusedAdamW(list(model.parameters()), lr=1e-4, weight_decay=0.05)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = crit(model(steps.x)[1], steps.y)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        after = float(crit(model(steps.x)[1], steps.y))
    losses = [float(v) for v in losses]
    print("[plainvit %s] loss over five steps %s -> %.4f" % (steps.mode, ["%.4f" % v for v in losses], after))
    assert np.isfinite(after) and after < losses[0]


def test_scene_engine_epoch_with_a_frozen_teacher(steps):
    """train_one_epoch(model, scene_model, ...) over a four-batch list with update_freq = 2 and ModelEma: two optimizer steps, every parameter with a gradient moves,
    the teacher does not"""
    from devias_amd import engine_for_finetuning_scene as eng
    from devias_amd.ema import ModelEma
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.optim import FusedAdamW
    model = _build(steps.cfg, "bf16")
    teacher = _build(dict(steps.cfg, use_mean_pooling=False), "bf16").eval()
    synth.fill_module_(teacher, seed=1)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    t_before = {n: p.detach().clone() for n, p in teacher.named_parameters()}
    opt = FusedAdamW(list(model.parameters()), lr=1e-3, weight_decay=0.05)
    ema = ModelEma(model, decay=0.9)
    bogus = torch.full((steps.B,), 10 ** 6, dtype=torch.int64)          # the caller's targets are never read: as an index they would be out of range
    loader = [(synth.video(steps.B, steps.cfg["all_frames"], 224, seed=2000 + i), bogus) for i in range(4)]
    stats = eng.train_one_epoch(model, teacher, LabelSmoothingCrossEntropy(0.1), loader, opt, DEV, 0, max_norm=5.0, model_ema=ema, update_freq=2, check_finite_every=4)
    assert np.isfinite(stats["loss"])
    assert not teacher.training
    still = [n for n, p in model.named_parameters() if torch.equal(p.detach(), before[n])]
    assert not still, still
    assert all(torch.equal(p.detach(), t_before[n]) for n, p in teacher.named_parameters())
