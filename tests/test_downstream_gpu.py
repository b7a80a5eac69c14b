"""The downstream model end to end on the GPU: the fp32 step against the step the real reference ran (tests/golden/downstream_t8.npz, 1e-3 relative with
golden_util's floor convention), the bf16 step against the fp32 mode element-wise (tests/grad_compare.py), evaluation under no_grad, and the fine-tuning engine."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import downstream_ref as dr
import golden_util as gu
import grad_compare as gc
from devias_amd import synth
from test_bf16_gradients_gpu import TOL_6400

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3          # the project's parity gate
# bf16 against the fp32 mode, ViT-B/16 8x224^2, B = 2.  Families test_bf16_gradients_gpu.py already bounds carry its bound for its plain B = 2 configuration
# (TOL_6400; that file has no plain 8x224^2 one).  The new family -- action_norm.*, scene_norm.*, fusion_head.* -- had no measurement: bound = twice the worst of
# rel / blk64 measured on MI355X in the run that set it (written beside it).
TOL_FUSION = 4e-2          # measured 1.94e-2 (action_norm.weight, a 64-row block; its rel 9.9e-3); scene_norm.weight 1.04e-2, every fusion_head.* at most 8.4e-3


def _cfg():
    fx = dict(np.load(gu.GOLDEN_DIR + "/downstream_t8.npz", allow_pickle=False))
    import ast
    return fx, ast.literal_eval(str(fx["config"])), int(fx["batch"])


def _build(cfg, dtype, **kw):
    import devias_amd
    m = devias_amd.create_model("slot_fusion_vit_base_patch16_224", **dict(cfg, compute_dtype=dtype, **kw))
    synth.fill_module_(m, seed=0)
    return m.to(DEV).train()


def _step(model, x, y, smoothing):
    from devias_amd.losses import LabelSmoothingCrossEntropy
    model.zero_grad(set_to_none=True)
    inp, out = model(x)
    loss = LabelSmoothingCrossEntropy(smoothing)(out, y)
    loss.backward()
    torch.cuda.synchronize()
    return SimpleNamespace(input=inp.detach().clone(), out=out.detach().clone(), idx=model.last_idx.clone(), loss=loss.detach().clone(),
                           grads={n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in model.named_parameters()})


@pytest.fixture(scope="module")
def steps():
    """the fp32-mode step and the bf16 step of the fixture's configuration, computed once"""
    fx, cfg, B = _cfg()
    x = synth.video(B, cfg["all_frames"], 224, seed=1000).to(DEV)
    y = synth.targets(B, cfg["downstream_nb_classes"], seed=1000).to(DEV)
    m32 = _build(cfg, "fp32")
    s32 = _step(m32, x, y, float(fx["smoothing"]))
    with torch.no_grad():
        m32.eval()
        ev = m32(x)
        ev_idx = m32.last_idx.clone()
    del m32
    torch.cuda.empty_cache()
    m16 = _build(cfg, "bf16")
    s16 = _step(m16, x, y, float(fx["smoothing"]))
    return SimpleNamespace(fx=fx, cfg=cfg, B=B, x=x, y=y, s32=s32, s16=s16, m16=m16, eval32=(ev[0].clone(), ev[1].clone(), ev_idx))


def test_fp32_step_against_the_reference(steps):
    fx, s = steps.fx, steps.s32
    assert s.idx.cpu().tolist() == fx["idx"].tolist()
    errs = {"input": gu.rel(s.input.float().cpu(), fx["input"]), "out": gu.rel(s.out.float().cpu(), fx["out"]), "loss": abs(float(s.loss) - float(fx["loss"])) / abs(float(fx["loss"]))}
    names = [str(n) for n in fx["param_names"]]
    none = sorted(n for n in names if s.grads[n] is None)
    assert none == sorted(str(n) for n in fx["no_grad_names"]) == sorted(dr.NO_GRAD_NAMES)
    nmax = float(fx["grad_norms"].max())
    for i, n in enumerate(names):
        if s.grads[n] is None:
            continue
        g = s.grads[n].float().cpu()
        ref_norm = float(fx["grad_norms"][i])
        errs[n + ".norm"] = abs(float(g.double().norm()) - ref_norm) / max(ref_norm, 1e-6 * nmax)
        smp = g.reshape(-1)[torch.from_numpy(gu.sample_idx(n, g.numel()))].double().numpy()
        ref_s = fx["grad_samples"][i].astype(np.float64)
        errs[n + ".samples"] = float(np.abs(smp - ref_s).max() / max(np.abs(ref_s).max(), 1e-6 * nmax, 1e-30))
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print("[downstream fp32 vs reference] input %.2e out %.2e loss %.2e; worst: %s" % (errs["input"], errs["out"], errs["loss"], ", ".join("%s %.2e" % kv for kv in worst)))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, bad


def test_bf16_step_against_the_fp32_mode(steps):
    a, r = steps.s16, steps.s32
    assert torch.equal(a.idx, r.idx), "a flipped selection makes the gradients incomparable"
    assert sorted(n for n, g in a.grads.items() if g is None) == sorted(dr.NO_GRAD_NAMES)
    live = [n for n, g in r.grads.items() if g is not None]
    new = [n for n in live if n.startswith(("action_norm.", "scene_norm.", "fusion_head."))]
    old = [n for n in live if n not in new]
    assert len(old) + len(new) + 6 == 196
    gc.check({n: a.grads[n] for n in old}, {n: r.grads[n] for n in old}, TOL_6400, "downstream bf16 B=2")
    errs = gc.compare({n: a.grads[n] for n in new}, {n: r.grads[n] for n in new})
    for n, e in errs.items():
        print(f"[grad] downstream bf16 B=2 fusion      rel {e.rel:.2e}  cos {e.cos:.8f}  blk64 {e.blk:.2e}  ({n})")
    print("[grad] downstream bf16 B=2 fusion worst %.3e; out rel %.2e, loss rel %.2e" % (max(e.worst for e in errs.values()), gu.rel(a.out.float().cpu(), r.out.float().cpu()),
                                                                                      abs(float(a.loss) - float(r.loss)) / abs(float(r.loss))))
    bad = {n: e.worst for n, e in errs.items() if not e.worst <= TOL_FUSION}
    assert not bad, bad


def test_eval_under_no_grad_is_the_training_forward(steps):
    """no dropout, no stochastic depth: the forward-only encoder blocks and the region without a save arena give the training forward's bits"""
    inp, out, idx = steps.eval32
    assert torch.equal(out, steps.s32.out) and torch.equal(inp, steps.s32.input) and torch.equal(idx, steps.s32.idx)
    m = steps.m16
    m.eval()
    with torch.no_grad():
        i16, o16 = m(steps.x)
    m.train()
    assert torch.equal(o16, steps.s16.out) and torch.equal(i16, steps.s16.input)


def test_twenty_steps_of_the_engine_lower_the_loss(steps):
    from devias_amd import engine_for_finetuning as eng
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.optim import FusedAdamW
    model = _build(steps.cfg, "bf16")
    crit = LabelSmoothingCrossEntropy(0.1)
    x, y = steps.x.cpu(), steps.y.cpu()
    with torch.no_grad():
        before = float(crit(model(steps.x)[1], steps.y))
    opt = FusedAdamW([p for p in model.parameters()], lr=1e-4, weight_decay=0.05)
    stats = eng.train_one_epoch(model, crit, [(x, y, None, None)] * 20, opt, DEV, 0, max_norm=5.0, check_finite_every=20)
    with torch.no_grad():
        after = float(crit(model(steps.x)[1], steps.y))
    print("[downstream engine] loss %.4f -> %.4f after 20 steps; last step's loss %.4f, grad norm %.3f" % (before, after, stats["loss"], stats["grad_norm"]))
    assert after < before and np.isfinite(stats["loss"])
    # the six gradient-less parameters never moved
    fresh = dict(_build(steps.cfg, "bf16").named_parameters())
    for n in dr.NO_GRAD_NAMES:
        assert torch.equal(dict(model.named_parameters())[n], fresh[n]), n


def test_validation_final_test_and_merge(steps, tmp_path):
    from devias_amd import engine_for_finetuning as eng
    model = steps.m16
    Cd = steps.cfg["downstream_nb_classes"]
    loader = []
    for b in range(2):
        x = synth.video(2, steps.cfg["all_frames"], 224, first=2 * b)
        loader.append((x, synth.targets(2, Cd, first=2 * b), ["clip[%d]" % (2 * b + i) for i in range(2)], torch.tensor([b, b + 1]), torch.tensor([0, 1])))
    val = eng.validation_one_epoch(loader, model, DEV)
    stats = eng.final_test(loader, model, DEV, str(tmp_path / "0.txt"))
    assert not model.training
    model.train()
    assert set(val) == {"loss", "acc1", "acc5"} == set(stats) and val == stats and np.isfinite(val["loss"])
    rows = (tmp_path / "0.txt").read_text().splitlines()
    assert len(rows) == 5 and all(" output : [" in r and "] : output " in r for r in rows[1:])
    hit1 = hit5 = 0
    with torch.no_grad():
        model.eval()
        for x, t, *_ in loader:
            out = model(x.to(DEV))[1].float().cpu()
            top = out.topk(5, dim=1).indices
            hit1 += int((top[:, 0] == t).sum())
            hit5 += int((top == t[:, None]).any(1).sum())
        model.train()
    assert stats["acc1"] == 100.0 * hit1 / 4 and stats["acc5"] == 100.0 * hit5 / 4
    top1, top5 = eng.merge(str(tmp_path), 1)
    assert top1 == pytest.approx(100.0 * hit1 / 4, abs=1e-9) and top5 == pytest.approx(100.0 * hit5 / 4, abs=1e-9)
