"""Mixup / CutMix without a GPU: the host draw of devias_amd.mixup.Mixup against the table the real reference drew for every case of tests/golden/mixup_vectors.npz
(tests/golden/make_mixup_goldens.py), the three engines' mixup_fn argument, the C ABI's new entries and the hard-label criterion's refusal of a dense target."""
import ast
import ctypes

import numpy as np
import pytest
import torch

import golden_util as gu

FX = dict(np.load(gu.GOLDEN_DIR + "/mixup_vectors.npz", allow_pickle=False))
CASES = [str(c) for c in FX["cases"]]


def case(name):
    cfg = ast.literal_eval(str(FX[name + ".config"]))
    return cfg, {k: FX[f"{name}.{k}"] for k in ("seed", "x", "y", "out_x", "out_target", "kind", "use_cutmix", "lam_drawn", "lam_target", "boxes")}


def build(cfg, num_classes):
    from devias_amd.mixup import Mixup
    m = Mixup(prob=cfg["prob"], mode=cfg["mode"], label_smoothing=cfg["smoothing"], num_classes=num_classes, **cfg["kw"])
    m.mixup_enabled = cfg["enabled"]
    return m


def test_the_fixture_covers_what_it_must():
    modes, tags, dtypes, shapes, batches, smoothings, probs, enabled = (set() for _ in range(8))
    for name in CASES:
        cfg, _ = case(name)
        modes.add(cfg["mode"]); tags.add(cfg["tag"]); dtypes.add(cfg["dtype"]); shapes.add(tuple(cfg["shape"])); batches.add(cfg["B"])
        smoothings.add(cfg["smoothing"]); probs.add(cfg["prob"]); enabled.add(cfg["enabled"])
    assert modes == {"batch", "pair", "elem"} and tags == {"mixup", "cutmix", "both", "minmax"} and dtypes == {"fp32", "bf16"}
    assert shapes == {(3, 2, 8, 8), (3, 2, 10, 14), (1, 1, 5, 7)} and batches == {2, 4, 6}
    assert smoothings == {0.0, 0.1} and probs == {1.0, 0.5} and enabled == {True, False}


@pytest.mark.parametrize("name", CASES)
def test_host_draw_equals_the_reference_table(name):
    """after np.random.seed(s): kind, box and weight of every clip, and the lam that reaches the target, are the reference's"""
    from devias_amd import mixup as mx
    cfg, r = case(name)
    m = build(cfg, int(FX["num_classes"]))
    np.random.seed(int(r["seed"]))
    table = m.draw((cfg["B"],) + tuple(cfg["shape"]))
    assert len(table.rows) == cfg["B"]
    assert [row.kind for row in table.rows] == r["kind"].tolist()
    f32 = cfg["mode"] != "batch"
    for i, row in enumerate(table.rows):
        if row.kind == mx.CUTMIX:
            assert [row.yl, row.yh, row.xl, row.xh] == r["boxes"][i].tolist()
            assert bool(r["use_cutmix"][i])
        elif row.kind == mx.MIXUP:
            lam = r["lam_drawn"][i]
            assert row.w_self == float(np.float32(lam))
            assert row.w_other == (float(np.float32(1) - np.float32(lam)) if f32 else float(np.float32(1. - lam)))
    dtype = torch.bfloat16 if cfg["dtype"] == "bf16" else torch.float32
    if cfg["mode"] == "batch":
        assert isinstance(table.lam, float) and np.array_equal(np.full(cfg["B"], table.lam), r["lam_target"])
    else:
        assert table.lam.dtype == np.float32
        assert np.array_equal(torch.tensor(table.lam, dtype=dtype).float().numpy().astype(np.float64), r["lam_target"])
    # the draw consumed exactly the reference's random numbers: the next one agrees with a replay that skips nothing
    after = np.random.rand()
    np.random.seed(int(r["seed"]))
    m.draw((cfg["B"],) + tuple(cfg["shape"]))
    assert np.random.rand() == after


def test_mixup_attributes_and_the_even_batch_assertion():
    from devias_amd.mixup import Mixup
    m = Mixup()
    assert (m.mixup_alpha, m.cutmix_alpha, m.cutmix_minmax, m.mix_prob, m.switch_prob, m.mode, m.correct_lam, m.label_smoothing, m.num_classes, m.mixup_enabled) == \
        (1., 0., None, 1.0, 0.5, "batch", True, 0.1, 1000, True)
    assert Mixup(cutmix_minmax=(0.2, 0.8)).cutmix_alpha == 1.0
    with pytest.raises(AssertionError, match="even"):
        m.draw((3, 3, 2, 8, 8))
    with pytest.raises(AssertionError, match="even"):
        m(torch.zeros(3, 3, 2, 8, 8), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="device tensors"):
        m(torch.zeros(2, 3, 2, 8, 8), torch.zeros(2, dtype=torch.int64))
    import devias_amd
    assert devias_amd.Mixup is Mixup and devias_amd.SoftTargetCrossEntropy.__name__ == "SoftTargetCrossEntropy"


def test_engines_accept_a_mixup_and_refuse_any_other_callable():
    from devias_amd import engine_for_finetuning as plain, engine_for_finetuning_scene as scene, engine_for_multi_task as multi
    from devias_amd.mixup import Mixup
    net = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    mix = Mixup(0.8, 1.0, num_classes=5)
    assert plain.train_one_epoch(net, None, [], opt, "cpu", 0, mixup_fn=mix) == {}
    assert scene.train_one_epoch(net, net, None, [], opt, "cpu", 0, mixup_fn=mix) == {}
    assert multi.train_one_epoch(net, net, None, [], opt, "cpu", 0, mixup_fn=mix) == {}
    for call in (lambda f: plain.train_one_epoch(net, None, [], opt, "cpu", 0, mixup_fn=f), lambda f: scene.train_one_epoch(net, net, None, [], opt, "cpu", 0, mixup_fn=f),
                 lambda f: multi.train_one_epoch(net, net, None, [], opt, "cpu", 0, mixup_fn=f)):
        with pytest.raises(NotImplementedError, match="mixup"):
            call(lambda s, t: (s, t))


def test_abi_178_entries_resolve_and_validate_before_any_launch():
    from devias_amd import _lib
    assert _lib.ABI_VERSION >= 178
    lib = _lib.load()
    assert lib.devias_version() >= 178
    for name in ("devias_mixup_clips", "devias_mixup_target", "devias_soft_ce_fwd", "devias_soft_ce_bwd", "devias_soft_ce_workspace_bytes"):
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
    assert ctypes.sizeof(_lib.MixupRow) == 32
    assert lib.devias_soft_ce_workspace_bytes(8) == 32 and lib.devias_soft_ce_workspace_bytes(0) == 0
    rows = (_lib.MixupRow * 2)()
    assert lib.devias_mixup_clips(None, 2, 6, 8, 8, _lib.F32, rows, None) == -1 and b"devias_mixup_clips" in lib.devias_last_error()
    one = ctypes.c_void_p(16)          # never dereferenced: validation comes first
    assert lib.devias_mixup_clips(one, 3, 6, 8, 8, _lib.F32, rows, None) == -1 and b"even" in lib.devias_last_error()
    rows[1].kind = 7
    assert lib.devias_mixup_clips(one, 2, 6, 8, 8, _lib.F32, rows, None) == -1 and b"kind" in lib.devias_last_error()
    assert lib.devias_mixup_target(None, 2, 5, 1.0, 0.0, None, None, None, None) == -1 and b"devias_mixup_target" in lib.devias_last_error()
    assert lib.devias_soft_ce_fwd(one, one, 0, 5, _lib.F32, one, one, None) == -1 and b"devias_soft_ce_fwd" in lib.devias_last_error()
    assert lib.devias_soft_ce_bwd(one, one, 2, 1, _lib.F32, one, one, None) == -1 and b"devias_soft_ce_bwd" in lib.devias_last_error()


def test_label_smoothing_ce_still_refuses_a_dense_target():
    from devias_amd.losses import LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
    with pytest.raises(NotImplementedError, match="int64"):
        LabelSmoothingCrossEntropy(0.1)(torch.zeros(2, 5), torch.full((2, 5), 0.2))
    with pytest.raises(ValueError, match="soft target"):
        SoftTargetCrossEntropy()(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64))
