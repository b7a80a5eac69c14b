"""train_one_epoch of both recipes (engine_for_slot, engine_for_slot_hvu) without a GPU: the loop is plain torch apart from the criterion, so a
stub criterion on a Linear model pins what the two loops share -- the skip past num_training_steps_per_epoch, the LR / WD schedule poke, gradient
accumulation with the grad_sync calls, clip + step, the finite check and the returned stats -- and what each recipe does with its own batch tuple."""
import copy
import importlib

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

RECIPES = ("devias_amd.engine_for_slot", "devias_amd.engine_for_slot_hvu")
LR = [0.9, 0.8, 0.7, 0.4, 0.2, 0.1]
WD = [0.5, 0.4, 0.3, 0.05, 0.02, 0.01]
TEACHER = torch.linspace(-1.0, 1.0, 10).view(2, 5)              # the Kinetics recipe's `scene_model`, given as precomputed logits


def _value(out, target, scene, fg_mask):
    """depends on every input the engine routes: the action target, the scene source and the first mask"""
    return (F.cross_entropy(out, target) * (1.0 + scene.float().mean()) * fg_mask[0].mean()).reshape(1)


class Criterion:
    """the recipe's call signature; returns (loss[1], out, {"action_loss": tensor})"""

    def __init__(self, hvu, bad=False):
        self.hvu, self.bad, self.masks_seen = hvu, bad, []

    def __call__(self, *args, fg_mask=None):
        if self.hvu:
            (_, (out, _, _), _), target, scene = args
        else:
            model, (_, (out, _, _), _), (token, scene), target = args
            assert isinstance(model, nn.Module) and token is None and scene is TEACHER
        self.masks_seen.append(fg_mask)
        loss = _value(out, target, scene, fg_mask)
        if self.bad:
            loss = loss * 0 + float("inf")
        return loss, out, {"action_loss": loss.detach()[0] * 0.5}


class Model(nn.Linear):
    def forward(self, x):
        return None, (super().forward(x), None, None), None


class GradSync:
    def __init__(self):
        self.events = []

    def set_accumulate(self, flag):
        self.events.append("acc %s" % flag)

    def finish(self):
        self.events.append("finish")


def _setup(hvu):
    g = torch.Generator().manual_seed(7)
    model = Model(4, 3)
    with torch.no_grad():
        model.weight.copy_(torch.randn(3, 4, generator=g))
        model.bias.copy_(torch.randn(3, generator=g))
    batches = []
    for _ in range(5):
        x, y = torch.randn(2, 4, generator=g), torch.randint(0, 3, (2,), generator=g)
        masks = (torch.rand(2, 6, generator=g), torch.rand(2, 8, generator=g))
        batches.append((x, y, torch.randint(0, 5, (2,), generator=g), masks) if hvu else (x, y, masks))
    return model, batches


def _optimizer(model):
    return torch.optim.SGD([{"params": [model.weight], "weight_decay": 0.1, "lr_scale": 0.5}, {"params": [model.bias], "weight_decay": 0.0}], lr=1.0)


def _run(name, model, batches, criterion, **kw):
    eng = importlib.import_module(name)
    opt, sync = _optimizer(model), GradSync()
    head = (model, criterion) if name.endswith("_hvu") else (model, TEACHER, criterion)
    stats = eng.train_one_epoch(*head, batches, opt, "cpu", 0, max_norm=0.5, start_steps=3, lr_schedule_values=LR, wd_schedule_values=WD,
                                num_training_steps_per_epoch=2, update_freq=2, grad_sync=sync, check_finite_every=1, **kw)
    return stats, opt, sync


def _restated(model, batches, hvu, prep=lambda x, masks: (x, masks)):
    """two windows of two micro-batches each scaled by 1/2, clip_grad_norm_, SGD step"""
    opt = _optimizer(model)
    for w in range(2):
        opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = LR[3 + w] * 0.5, LR[3 + w]
        opt.param_groups[0]["weight_decay"] = WD[3 + w]
        for batch in batches[2 * w:2 * w + 2]:
            x, masks = prep(batch[0], batch[-1])
            (_value(model(x)[1][0], batch[1], batch[2] if hvu else TEACHER, masks) / 2).backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 0.5)
        opt.step()
        opt.zero_grad(set_to_none=True)
    return model


@pytest.mark.parametrize("name", RECIPES)
def test_train_one_epoch_schedule_accumulation_and_step(name):
    hvu = name.endswith("_hvu")
    model, batches = _setup(hvu)
    want = _restated(copy.deepcopy(model), batches, hvu)
    crit = Criterion(hvu)
    stats, opt, sync = _run(name, model, batches, crit)
    assert sync.events == ["acc True", "acc False", "finish"] * 2                       # the fifth batch is past num_training_steps_per_epoch
    assert len(crit.masks_seen) == 4 and all(m[0] is b[-1][0] for m, b in zip(crit.masks_seen, batches))
    assert [g["lr"] for g in opt.param_groups] == [LR[4] * 0.5, LR[4]]
    assert [g["weight_decay"] for g in opt.param_groups] == [WD[4], 0.0]                  # the zero-decay group is never poked
    assert set(stats) == {"loss", "lr", "min_lr", "grad_norm", "action_loss"}
    assert all(isinstance(v, float) for v in stats.values())
    assert (stats["lr"], stats["min_lr"]) == (LR[4], LR[4] * 0.5) and stats["action_loss"] == pytest.approx(stats["loss"])    # loss / 2 both ways
    assert model.training and all(p.grad is None for p in model.parameters())
    assert torch.equal(model.weight, want.weight) and torch.equal(model.bias, want.bias)


@pytest.mark.parametrize("name", RECIPES)
def test_train_one_epoch_hands_the_batch_to_the_mask_model(name):
    hvu = name.endswith("_hvu")
    model, batches = _setup(hvu)
    masks = (torch.full((2, 6), 0.25), torch.full((2, 8), 0.5))
    calls = []

    def mask_model(samples, *targets):                                                  # (samples, targets) or (samples, action_targets, scene_targets)
        calls.append(len(targets))
        return (samples.flip(0) * 2.0, *targets, masks)

    want = _restated(copy.deepcopy(model), batches, hvu, prep=lambda x, _: (x.flip(0) * 2.0, masks))
    crit = Criterion(hvu)
    _run(name, model, [b[:-1] for b in batches], crit, mask_model=mask_model)          # the loader's tuple needs no masks then
    assert calls == [2 if hvu else 1] * 4 and all(m is masks for m in crit.masks_seen)
    assert torch.equal(model.weight, want.weight) and torch.equal(model.bias, want.bias)


@pytest.mark.parametrize("name", RECIPES)
def test_train_one_epoch_stops_on_a_non_finite_loss(name, capsys):
    hvu = name.endswith("_hvu")
    model, batches = _setup(hvu)
    with pytest.raises(SystemExit):
        _run(name, model, batches, Criterion(hvu, bad=True))
    assert "stopping training" in capsys.readouterr().out
