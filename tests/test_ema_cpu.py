"""Model EMA without a GPU (devias_amd/ema.py): the arithmetic contract every path shares -- timm's ModelEma.update restated, three single-rounded fp32 operations with
the second factor (1. - decay) evaluated in double --, the ModelEma surface and its checkpoint round trip, the update's place in both recipes' train_one_epoch, and
the argument validation of the two C-ABI entry points, which precedes any launch."""
import copy
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import test_engine_cpu as te

DECAYS = (0.9999, 0.5, 0.0, 1.0)


@pytest.fixture(autouse=True)
def _global_rng_untouched():
    """module constructors draw from torch's global generator: leave it as found, tests that run later see the stream they always saw"""
    with torch.random.fork_rng(devices=[]):
        yield


def _model(seed=3):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(257, 389), nn.LayerNorm(389), nn.BatchNorm1d(389), nn.Linear(389, 3, bias=False))     # 100 k weights; one int64 buffer


def _perturb(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for v in model.state_dict().values():
            if v.dtype.is_floating_point:
                v.add_(torch.randn(v.shape, generator=g) * 0.1)
            else:
                v.add_(3)


@pytest.mark.parametrize("decay", DECAYS)
def test_update_is_the_torch_expression_and_within_the_float64_bound(decay):
    """3 updates on a CPU model: bit-equal to `ema_v * decay + (1. - decay) * model_v` entry by entry; each fp32 element of each update within
    3.1 * 2^-24 * (d|e| + (1-d)|w|) of the float64 evaluation on the same inputs: three roundings of the operations plus the roundings of the two factors, to first order
    (worst ratio seen: 0.71 of the bound)."""
    from devias_amd.ema import ModelEma
    model = _model()
    me = ModelEma(model, decay=decay)
    want = {k: v.clone() for k, v in model.state_dict().items()}
    worst = 0.0
    for step in range(3):
        _perturb(model, 10 + step)
        before = {k: v.clone() for k, v in me.state_dict().items()}
        me.update(model)
        msd, got = model.state_dict(), me.state_dict()
        for k in want:
            want[k] = (want[k] * decay + (1. - decay) * msd[k]).to(want[k].dtype)
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), (step, k)
            if got[k].dtype == torch.float32:
                e, w = before[k].double(), msd[k].double()
                bound = 3.1 * 2.0 ** -24 * (decay * e.abs() + (1.0 - decay) * w.abs())
                err = (got[k].double() - (decay * e + (1.0 - decay) * w)).abs()
                assert bool((err <= bound).all()), (step, k, float((err / bound.clamp_min(1e-300)).max()))
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print("worst error / bound at decay %g: %.3f" % (decay, worst))
    assert worst <= 1.0


def test_the_formula_test_tells_the_float32_complement_apart():
    """a mutant whose second factor is 1.0f - fl32(decay) instead of fl32(1. - decay) differs in bits at decay 0.9999"""
    d = 0.9999
    mutant_factor = float(np.float32(1.0) - np.float32(d))
    assert mutant_factor != float(np.float32(1.0 - d))
    g = torch.Generator().manual_seed(5)
    e, w = torch.randn(100003, generator=g), torch.randn(100003, generator=g)
    right, mutant = e * d + (1. - d) * w, e * d + mutant_factor * w
    assert not torch.equal(right, mutant)
    from devias_amd.ema import ModelEma
    lin = nn.Linear(100003, 1, bias=False)
    me = ModelEma(lin, decay=d)
    with torch.no_grad():
        me.ema.weight.copy_(e.view(1, -1)); lin.weight.copy_(w.view(1, -1))
    me.update(lin)
    assert torch.equal(me.ema.weight.view(-1), right) and not torch.equal(me.ema.weight.view(-1), mutant)


def test_model_ema_surface_and_checkpoint_round_trip(tmp_path):
    from devias_amd import ModelEma, checkpoint as ck
    model = _model()
    model.train()
    me = ModelEma(model, decay=0.99)
    assert me.decay == 0.99 and me.ema is not model and isinstance(me.ema, nn.Sequential)
    assert not me.ema.training and model.training
    assert all(not p.requires_grad for p in me.ema.parameters()) and all(p.requires_grad for p in model.parameters())
    assert list(me.state_dict()) == list(model.state_dict())
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(me.state_dict().values(), model.state_dict().values()))
    with pytest.raises(ValueError):
        ModelEma(model, decay=1.5)
    _perturb(model, 1)
    me.update(model)
    saved = {k: v.clone() for k, v in me.state_dict().items()}
    assert any(not torch.equal(saved[k], v) for k, v in model.state_dict().items())
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    ck.save_checkpoint(str(tmp_path), 4, model, optimizer=opt, model_ema=me)
    # resume into fresh objects: the shadow comes back bitwise, and is not the model's weights
    model2 = _model(seed=9)
    me2 = ModelEma(model2, decay=0.99)
    assert ck.auto_resume(str(tmp_path), model2, torch.optim.SGD(model2.parameters(), lr=0.1), model_ema=me2) == 5
    assert all(torch.equal(v, saved[k]) for k, v in me2.state_dict().items())
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in model2.state_dict().items())
    # ModelEma(resume=path) reads the same entry
    me3 = ModelEma(_model(seed=11), decay=0.99, resume=str(tmp_path / "checkpoint-4.pth"))
    assert all(torch.equal(v, saved[k]) for k, v in me3.state_dict().items()) and all(not p.requires_grad for p in me3.ema.parameters())
    # without model_ema: as before, the shadow entry of the file is ignored
    model4 = _model(seed=13)
    assert ck.auto_resume(str(tmp_path), model4, torch.optim.SGD(model4.parameters(), lr=0.1)) == 5
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in model4.state_dict().items())
    # a checkpoint without the entry leaves a given shadow alone
    ck.save_checkpoint(str(tmp_path), 6, model, optimizer=opt)
    me5 = ModelEma(_model(seed=15), decay=0.99)
    keep = {k: v.clone() for k, v in me5.state_dict().items()}
    assert ck.auto_resume(str(tmp_path), _model(seed=17), model_ema=me5) == 7
    assert all(torch.equal(v, keep[k]) for k, v in me5.state_dict().items())


def test_tied_tensor_is_updated_once_per_listing():
    """a module registered twice appears twice in state_dict(); timm's loop, restated, updates the shared shadow once per listing"""
    from devias_amd.ema import ModelEma
    shared = nn.Linear(4, 4)
    model = nn.Sequential(shared, nn.ReLU(), shared)
    me = ModelEma(model, decay=0.5)
    assert me.ema[0] is me.ema[2] and len(me.state_dict()) == 4
    e0 = me.ema[0].weight.clone()
    _perturb(model, 2)
    me.update(model)
    w = shared.weight.detach()
    once = e0 * 0.5 + (1. - 0.5) * w
    assert torch.equal(me.ema[0].weight, once * 0.5 + (1. - 0.5) * w)


@pytest.mark.parametrize("name", te.RECIPES)
def test_train_one_epoch_updates_the_shadow_after_each_optimizer_step(name):
    """update_freq = 2, five batches, two windows: the shadow is updated after each of the two optimizer steps and never after a micro-batch; the model's weights are
    those of the run without a shadow, bit for bit"""
    from devias_amd.ema import ModelEma
    hvu, decay = name.endswith("_hvu"), 0.75
    model, batches = te._setup(hvu)
    plain = copy.deepcopy(model)
    # the loop restated: test_engine_cpu._restated with the update after each step
    ref = copy.deepcopy(model)
    shadow = {k: v.clone() for k, v in ref.state_dict().items()}
    opt = te._optimizer(ref)
    for w in range(2):
        opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = te.LR[3 + w] * 0.5, te.LR[3 + w]
        opt.param_groups[0]["weight_decay"] = te.WD[3 + w]
        for batch in batches[2 * w:2 * w + 2]:
            (te._value(ref(batch[0])[1][0], batch[1], batch[2] if hvu else te.TEACHER, batch[-1]) / 2).backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)
        opt.step()
        opt.zero_grad(set_to_none=True)
        with torch.no_grad():
            for k, v in ref.state_dict().items():
                shadow[k] = shadow[k] * decay + (1. - decay) * v
    me = ModelEma(model, decay=decay)
    calls = []
    update = me.update
    me.update = lambda m: (calls.append(m), update(m))[1]
    te._run(name, model, batches, te.Criterion(hvu), model_ema=me)
    te._run(name, plain, batches, te.Criterion(hvu))
    assert len(calls) == 2 and all(m is model for m in calls)
    assert all(torch.equal(v, shadow[k]) for k, v in me.state_dict().items())
    assert not torch.equal(me.ema.weight, model.weight) and not me.ema.training
    assert torch.equal(model.weight, plain.weight) and torch.equal(model.bias, plain.bias)
    assert torch.equal(model.weight, ref.weight) and torch.equal(model.bias, ref.bias)


def test_c_abi_validates_before_any_launch():
    from devias_amd import _lib, optim
    lib = _lib.load()
    assert lib.devias_version() >= 172 and _lib.ABI_VERSION >= 172
    assert optim._REC.itemsize == 64 == _lib.OPT_TENSOR_BYTES and optim._REC.fields["ema"][1] == 56 and optim._REC.fields["ema"][0] == np.dtype("<u8")
    assert [optim._REC.fields[n][1] for n in ("param", "grad", "m", "v", "n", "lr", "wd", "bc1", "bc2s")] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    host = (ctypes.c_char * 64)()                                  # never dereferenced: every call below is refused by its validation
    t = ctypes.addressof(host)
    fused = lambda table, ct, ci, n, d, o: lib.devias_adamw_ema_multi(table, ct, ci, n, 0.9, 0.999, 1e-8, 1.0, None, d, o, None)      # noqa: E731
    alone = lambda table, ct, ci, n, d, o: lib.devias_ema_multi(table, ct, ci, n, d, o, None)                                         # noqa: E731
    for call, name in ((fused, b"devias_adamw_ema_multi"), (alone, b"devias_ema_multi")):
        bad = [(None, t, t, 1, 0.9, 0.1), (t, None, t, 1, 0.9, 0.1), (t, t, None, 1, 0.9, 0.1), (t, t, t, -1, 0.9, 0.1),
               (t, t, t, 1, -0.1, 0.1), (t, t, t, 1, 1.5, 0.1), (t, t, t, 1, math.nan, 0.1), (t, t, t, 1, 0.9, math.nan), (t, t, t, 1, 0.9, 1.5),
               (None, None, None, 0, 1.5, 0.1), (None, None, None, 0, math.nan, 0.1)]
        for args in bad:
            assert lib.devias_set_option(b"no_such_option", 1) == -1                   # puts another message into the error slot
            assert call(*args) == -1, (name, args)
            assert name in lib.devias_last_error(), (name, args, lib.devias_last_error())
        assert call(None, None, None, 0, 0.9, 0.1) == 0                               # nothing to do: no launch either
    # the Python wrappers refuse a bad decay and a CPU tensor before reaching the library
    from devias_amd import ops
    with pytest.raises(ValueError):
        ops.ema_factors(float("nan"))
    with pytest.raises(ValueError):
        ops.ema_factors(-0.1)
    d, o = ops.ema_factors(0.9999)
    assert np.float32(o) == np.float32(1.0 - 0.9999) and np.float32(o) != np.float32(1.0) - np.float32(d)
    z = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.ema_multi(z, torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0.9)
