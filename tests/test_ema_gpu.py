"""Model EMA on the GPU: the shadow weights written inside the fused AdamW launch (devias_adamw_ema_multi), the stand-alone stream (devias_ema_multi), the host-side
refusals, and the two things a user would notice: the evaluated `.ema` model follows the update although it was forwarded before (weight-copy cache), and nothing
changes when no shadow is given.  The arithmetic contract is that of tests/test_ema_cpu.py: bit-equal to torch's `ema_v * decay + (1. - decay) * model_v`."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import golden_util as gu
from test_kernels_gpu import _opt_setup, rnd
from test_parity_gpu import build

pytestmark = pytest.mark.gpu

DECAY = 0.9


@pytest.fixture(autouse=True)
def _global_rng_untouched():
    with torch.random.fork_rng():
        yield


class Holder(nn.Module):
    """the tensor set of test_kernels_gpu._opt_setup as a model: lengths 3, 1, 16384, 16385, 32768, 40000, 257x129, 765x768 and a 5x7x11 tensor"""

    def __init__(self, tensors):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(t.clone()) for t in tensors])


def _torch_ema(shadow, value, decay):
    return shadow * decay + (1. - decay) * value


def _offset_storage(t):
    """the same values in storage that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _grads(shapes, step):
    return [rnd(*s, seed=100 * step + i, scale=0.3 * step) for i, s in enumerate(shapes)]


def _run(max_norm, ema_fused=True, with_ema=True, offset=()):
    from devias_amd.ema import ModelEma
    from devias_amd.optim import FusedAdamW
    shapes, ps, groups = _opt_setup()
    model = Holder(ps)
    params = list(model.ps)
    opt = FusedAdamW(groups(params), lr=1e-3, betas=(0.9, 0.95), eps=1e-8, ema_fused=ema_fused)
    me = ModelEma(model, decay=DECAY) if with_ema else None
    for i in offset:
        me.ema.ps[i].data = _offset_storage(me.ema.ps[i].data)
    ref = [p.detach().clone() for p in params]                 # the shadows by the torch expression, from this run's own parameters
    for step in range(1, 6):
        lr = 1e-3 * (1.0 - 0.1 * step)
        for g in opt.param_groups:
            g["lr"] = lr * g["lr_scale"]
        skip = 4 if step == 3 else -1                          # a parameter without a gradient in one step
        for i, (p, g) in enumerate(zip(params, _grads(shapes, step))):
            p.grad = None if i == skip else g
        opt.step(max_norm=max_norm, ema=me) if with_ema else opt.step(max_norm=max_norm)
        ref = [_torch_ema(r, p.detach(), DECAY) for r, p in zip(ref, params)]
    return params, opt, me, ref


@pytest.fixture(scope="module")
def plain_runs():
    """FusedAdamW without a shadow, once per max_norm, shared by the cases below and left unchanged"""
    return {mn: _run(mn, with_ema=False) for mn in (None, 0.5)}


@pytest.mark.parametrize("ema_fused", [True, False])
@pytest.mark.parametrize("max_norm", [None, 0.5])
def test_step_with_shadow_equals_step_without_and_torch_ema(max_norm, ema_fused, plain_runs):
    params0, opt0, _, ref = plain_runs[max_norm]
    params, opt, me, _ = _run(max_norm, ema_fused=ema_fused)
    for i, (p0, p) in enumerate(zip(params0, params)):
        assert torch.equal(p.detach(), p0.detach()), i
        assert torch.equal(opt.state[p]["exp_avg"], opt0.state[p0]["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], opt0.state[p0]["exp_avg_sq"]), i
    for i, (e, r) in enumerate(zip(me.ema.ps, ref)):
        assert not torch.equal(e, params[i].detach()) and torch.equal(e, r), (i, float((e - r).abs().max()))


def test_shadow_in_unaligned_storage_takes_the_scalar_path(plain_runs):
    params0, _, _, ref = plain_runs[0.5]
    params, _, me, _ = _run(0.5, offset=(0, 1, 4, 5, 6))
    assert all(me.ema.ps[i].data_ptr() % 16 == 4 for i in (0, 1, 4, 5, 6))
    for i, (p, p0) in enumerate(zip(params, params0)):           # the shadow's alignment must not change the update itself
        assert torch.equal(p.detach(), p0.detach()), (i, float((p.detach() - p0.detach()).abs().max()))
    for i, (e, r) in enumerate(zip(me.ema.ps, ref)):
        assert torch.equal(e, r), (i, float((e - r).abs().max()))


def test_stand_alone_launch_reads_only_param_and_ema():
    """devias_ema_multi over a hand-made table whose grad / exp_avg / exp_avg_sq words are 0; one record without a shadow is left alone"""
    from devias_amd import ops
    from devias_amd.optim import _REC, chunk_lists
    shapes, ps, _ = _opt_setup(seed=90)
    es = [rnd(*s, seed=190 + i) for i, s in enumerate(shapes)]
    es[1], ps[7] = _offset_storage(es[1]), _offset_storage(ps[7])
    e0 = [e.clone() for e in es]
    rec = np.zeros(len(ps), _REC)
    for i, (p, e) in enumerate(zip(ps, es)):
        rec[i]["param"], rec[i]["n"], rec[i]["ema"] = p.data_ptr(), p.numel(), 0 if i == 2 else e.data_ptr()
    table = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    ct, ci = chunk_lists([p.numel() for p in ps], "cuda")
    p0 = [p.clone() for p in ps]
    for decay in (0.9999, 0.5):
        before = [e.clone() for e in es]
        ops.ema_multi(table, ct, ci, decay)
        for i, (p, e, b) in enumerate(zip(ps, es, before)):
            if i == 2:
                assert torch.equal(e, e0[i])
                continue
            assert torch.equal(e, _torch_ema(b, p, decay)), (decay, i)
            bound = 3.1 * 2.0 ** -24 * (decay * b.double().abs() + (1.0 - decay) * p.double().abs())
            err = (e.double() - (decay * b.double() + (1.0 - decay) * p.double())).abs()
            assert bool((err <= bound).all()), (decay, i, float((err / bound.clamp_min(1e-300)).max()))
    assert all(torch.equal(p, q) for p, q in zip(ps, p0))
    with pytest.raises(ValueError):
        ops.ema_multi(table, ct, ci, 1.5)


def test_fused_path_refuses_shadows_it_cannot_write():
    from devias_amd.ema import ModelEma
    from devias_amd.optim import FusedAdamW
    shapes, ps, groups = _opt_setup()

    def setup(**kw):
        model = Holder(ps)
        for p, g in zip(model.ps, _grads(shapes, 1)):
            p.grad = g
        return model, FusedAdamW(groups(list(model.ps)), lr=1e-3), ModelEma(model, decay=DECAY, **kw)

    model, opt, me = setup()
    me.ema.ps[2].data = model.ps[2].data
    with pytest.raises(RuntimeError, match="aliases"):
        opt.step(ema=me)
    model, opt, me = setup()
    me.ema.ps[2].data = me.ema.ps[2].data.flatten()[:-1].contiguous()
    with pytest.raises(RuntimeError, match="shadow of ps.2"):
        opt.step(ema=me)
    model, opt, me = setup(device="cpu")
    assert not me.on_device_of(model)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        opt.step(ema=me)
    before = [p.detach().clone() for p in model.ps]
    me.update(model)                                           # the way such a shadow is kept: the torch expression on the host
    assert all(torch.equal(e, _torch_ema(b.cpu(), p.detach().cpu(), DECAY)) for e, b, p in zip(me.ema.ps, before, model.ps))
    assert all(torch.equal(p.detach(), b) for p, b in zip(model.ps, before))          # and no refused call stepped anything


@pytest.mark.parametrize("name", ["devias_amd.engine_for_slot", "devias_amd.engine_for_slot_hvu"])
def test_train_one_epoch_steps_the_fused_optimizer_with_the_shadow(name):
    """the toy loop of tests/test_engine_cpu.py on the GPU with FusedAdamW: two windows of two micro-batches, the shadow goes through step(ema=...) (update() is never
    called), equals the torch expression applied after each of the two steps, and the model ends where the run without a shadow ends"""
    import copy
    import importlib
    import test_engine_cpu as te
    from devias_amd.ema import ModelEma
    from devias_amd.optim import FusedAdamW
    eng, hvu = importlib.import_module(name), name.endswith("_hvu")
    cpu_model, batches = te._setup(hvu)

    def run(with_ema):
        model = copy.deepcopy(cpu_model).cuda()
        opt = FusedAdamW([{"params": [model.weight], "weight_decay": 0.1, "lr_scale": 0.5}, {"params": [model.bias], "weight_decay": 0.0}], lr=1.0)
        me = ModelEma(model, decay=0.75) if with_ema else None
        after, step = [], opt.step
        opt.step = lambda **kw: (step(**kw), after.append(({k: v.clone() for k, v in model.state_dict().items()}, set(kw))))[0]
        if me is not None:
            me.update = None                                   # calling it would raise
        head = (model, te.Criterion(hvu)) if hvu else (model, te.TEACHER, te.Criterion(hvu))
        eng.train_one_epoch(*head, batches, opt, "cuda", 0, max_norm=0.5, start_steps=3, lr_schedule_values=te.LR, wd_schedule_values=te.WD,
                            num_training_steps_per_epoch=2, update_freq=2, check_finite_every=0, **({"model_ema": me} if with_ema else {}))
        return model, me, after

    plain, _, after = run(False)
    model, me, seen = run(True)
    assert [kw for _, kw in after] == [{"max_norm"}] * 2 and [kw for _, kw in seen] == [{"max_norm", "ema"}] * 2
    shadow = {k: v.cuda() for k, v in cpu_model.state_dict().items()}
    for sd, _ in after:
        shadow = {k: _torch_ema(shadow[k], sd[k], 0.75) for k in shadow}
    assert all(torch.equal(v, shadow[k]) for k, v in me.state_dict().items())
    assert torch.equal(model.weight, plain.weight) and torch.equal(model.bias, plain.bias) and not torch.equal(me.ema.weight, model.weight)


# ------------------------------------------------------------------------------------------------ the model
def _flat(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _flat(o)]
    return []


def _backward(model, cfg, B, x):
    from devias_amd.train_loss import TrainLoss
    _, y, tl, fg = gu.inputs(cfg, B)
    crit = TrainLoss(criterion=None, scene_criterion="KL", num_action_classes=cfg.num_classes, slot_matching_method="matching",
                     mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0, scene_loss_weight=4000)
    total, _, _ = crit(model, model(x), (None, tl.cuda()), y.cuda(), fg_mask=(fg[0].cuda(), fg[1].cuda()))
    model.zero_grad(set_to_none=True)
    total.backward()


def test_evaluated_shadow_model_follows_the_update():
    """ViT-S, 8 frames, B = 2, bf16: `.ema` is forwarded (its compute-dtype weight copies are cached), two fused steps move the shadows through raw pointers, and the
    next forward of `.ema` must be that of a fresh model carrying the shadow weights"""
    from devias_amd.ema import ModelEma
    from devias_amd.optim import FusedAdamW
    fx, cfg, B = gu.load("vits_t8")
    model = build(cfg, "bf16")
    me = ModelEma(model, decay=0.5)
    assert not me.ema.training and len(me.state_dict()) == len(model.state_dict()) and me.on_device_of(model)
    x = gu.inputs(cfg, B)[0].cuda()
    with torch.no_grad():
        first = [t.clone() for t in _flat(me.ema(x))]
    opt = FusedAdamW(model.parameters(), lr=2e-3)
    for _ in range(2):
        _backward(model, cfg, B, x)
        opt.step(max_norm=5.0, ema=me)
    with torch.no_grad():
        second = [t.clone() for t in _flat(me.ema(x))]
    fresh = build(cfg, "bf16").eval()
    fresh.load_state_dict(me.state_dict())
    with torch.no_grad():
        want = _flat(fresh(x))
    assert len(first) == len(second) == len(want) >= 3
    assert all(torch.equal(a, b) for a, b in zip(second, want))
    assert any(not torch.equal(a, b) for a, b in zip(first, second))
    # the stand-alone launch, with no optimizer step before it that would have invalidated the weight copies for it: torch moves the model, update() moves the shadows
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(1.25)
    me.update(model)
    with torch.no_grad():
        third = [t.clone() for t in _flat(me.ema(x))]
    fresh.load_state_dict(me.state_dict())
    with torch.no_grad():
        want = _flat(fresh(x))
    assert all(torch.equal(a, b) for a, b in zip(third, want)) and any(not torch.equal(a, b) for a, b in zip(second, third))
    msd = model.state_dict()
    differs = [not torch.equal(v, msd[k]) for k, v in me.state_dict().items()]
    assert sum(differs) > len(differs) // 2


def test_no_shadow_no_change():
    """one training step with ema=None against the step taken through step() as the other tests call it: same gradients in, same bits out"""
    from devias_amd.optim import FusedAdamW
    fx, cfg, B = gu.load("vits_t8")
    a, b = build(cfg, "bf16"), build(cfg, "bf16")
    x = gu.inputs(cfg, B)[0].cuda()
    _backward(a, cfg, B, x)
    for p, q in zip(a.parameters(), b.parameters()):
        q.grad = None if p.grad is None else p.grad.clone()
    oa, ob = FusedAdamW(a.parameters(), lr=2e-3), FusedAdamW(b.parameters(), lr=2e-3)
    oa.step(max_norm=5.0, ema=None)
    ob.step(max_norm=5.0)
    assert float(oa.last_grad_norm) == float(ob.last_grad_norm) > 0
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
        if p.grad is not None:
            assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]) and torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"]), n
