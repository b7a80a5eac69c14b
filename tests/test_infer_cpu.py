"""The forward-only encoder block (devias_encoder_block_infer, ABI 173) and the two evaluation entry points of the engine, without a GPU: the C-ABI surface,
the argument validation that precedes every launch, the workspace size query, and final_test_with_scene_label / merge against what the reference's own
engine/engine_for_slot.py returned (tests/golden/eval_engine.json, made by tests/golden/make_eval_goldens.py)."""
import ctypes
import json
import os
import re

import torch
import torch.nn as nn

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_infer_entry_points_are_declared_exported_and_bound():
    from devias_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "devias_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t|void|const char\*)\s+(devias_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in ("devias_encoder_block_infer", "devias_encoder_block_infer_workspace_bytes"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.devias_version() >= 173 and _lib.ABI_VERSION >= 173
    m = re.search(r"#define DEVIAS_CNT_BLOCK_INFER (\d+)", hdr)
    cnt_max = int(re.search(r"#define DEVIAS_CNT_MAX (\d+)", hdr).group(1))
    assert m and int(m.group(1)) == _lib.COUNTERS["block_infer"] == 24 < cnt_max == 25
    ids = [int(v) for v in re.findall(r"#define DEVIAS_CNT_(?!MAX)\w+ (\d+)", hdr)]
    assert len(ids) == len(set(ids))                                                   # the new counter took a free id
    assert sorted(_lib.COUNTERS.values()) == sorted(ids)
    lib.devias_counters_reset()
    assert lib.devias_counter(24) == 0 and lib.devias_counter(25) == -1


def _args(p, B=2, N=8, D=128, H=2, hidden=512, dtype=1, ws_bytes=None, rows=None, **kw):
    from devias_amd import _lib
    a = _lib.BlockArgs()
    a.B, a.N, a.D, a.H, a.hidden, a.dtype, a.eps = B, N, D, H, hidden, dtype, 1e-6
    for n in ("n1w", "n1b", "n2w", "n2b", "Wqkv", "Wp", "W1", "W2", "qkv_bias", "pb", "b1", "b2", "ws"):
        setattr(a, n, p)
    need = _lib.load().devias_encoder_block_infer_workspace_bytes(B, N, rows if rows is not None else B * N, D, H, hidden, dtype)
    a.ws_bytes = need if ws_bytes is None else ws_bytes
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_infer_validates_arguments_without_a_device():
    """each of these returns DEVIAS_EINVAL with a message before anything is launched (no device is needed to get there); the counter moves only on a launch"""
    from devias_amd import _lib
    lib = _lib.load()
    lib.devias_counters_reset()
    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 255) & ~255            # non-null, aligned host addresses: validation must refuse before any launch could read them
    x, x2 = p, p + 64
    fn = lib.devias_encoder_block_infer
    who = b"devias_encoder_block_infer"
    need = lib.devias_encoder_block_infer_workspace_bytes(2, 8, 16, 128, 2, 512, 1)
    assert need > 0
    cases = [
        ("null args", None, x, x2, 16),
        ("rows < B*N", _args(p), x, x2, 15),
        ("D != 64 H", _args(p, D=192, H=2), x, x2, 16),
        ("non-null ds1", _args(p, ds1=p), x, x2, 16),
        ("non-null ds2", _args(p, ds2=p), x, x2, 16),
        ("non-zero defer_wgrad", _args(p, defer_wgrad=1), x, x2, 16),
        ("non-null keep_dx1", _args(p, keep_dx1=p), x, x2, 16),
        ("x2 == x", _args(p), x, x, 16),
        ("null x", _args(p), None, x2, 16),
        ("a workspace one byte short", _args(p, ws_bytes=need - 1), x, x2, 16),
        ("a workspace sized for fewer rows", _args(p), x, x2, 32),
        ("null ws", _args(p, ws=None), x, x2, 16),
        ("bad dtype", _args(p, dtype=7), x, x2, 16),
        ("WqkvS without qkv_biasS", _args(p, WqkvS=p), x, x2, 16),
    ]
    for what, a, xi, xo, rows in cases:
        assert fn(ctypes.byref(a) if a is not None else None, xi, xo, rows, None) == EINVAL, what
        assert who in lib.devias_last_error(), what
    assert lib.devias_counter(_lib.COUNTERS["block_infer"]) == 0
    assert sum(lib.devias_counter(i) for i in _lib.COUNTERS.values()) == 0


def test_infer_workspace_size_query():
    from devias_amd import _lib
    lib = _lib.load()
    q = lib.devias_encoder_block_infer_workspace_bytes
    for dt, es in ((_lib.F32, 4), (_lib.BF16, 2)):
        for B, N, rows, D, H in ((2, 8, 16, 128, 2), (3, 197, 768, 128, 2), (32, 1568, 32 * 1568, 768, 12), (8, 1569, 12800, 768, 12)):
            hid = 4 * D
            pieces = rows * D * es * (1 + 3 + 1 + 1) + rows * hid * es + 2 * rows * 4 + B * H * N * 4      # u, qkv, o, x1; hact; LayerNorm statistics; lse
            assert q(B, N, rows, D, H, hid, dt) >= pieces, (B, N, rows, D, dt)
            assert q(B, N, rows + 256, D, H, hid, dt) > q(B, N, rows, D, H, hid, dt)                        # monotone in rows
            assert q(B, N, B * N - 1, D, H, hid, dt) == 0                                                    # fewer rows than tokens: no size
    # the region needs less memory than the training forward's arena alone: ViT-B at B = 32, the workspace plus x plus x2
    B, N, D, H, hid = 32, 1568, 768, 12, 3072
    for dt, es in ((_lib.F32, 4), (_lib.BF16, 2)):
        assert q(B, N, B * N, D, H, hid, dt) + 2 * B * N * D * es < lib.devias_encoder_block_save_bytes(B, N, D, H, hid, dt)
    # save == NULL is accepted: with it the call fails on something else (here: the short workspace), with a non-null one just the same
    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 255) & ~255
    for save in (None, p):
        a = _args(p, save=save, ws_bytes=16)
        assert lib.devias_encoder_block_infer(ctypes.byref(a), p, p + 64, 16, None) == EINVAL and b"workspace too small" in lib.devias_last_error()


# ---- the engine's two evaluation entry points against the reference's ------------------------------------------------------------------------------------------
class Replay(nn.Module):
    """returns the next of the given outputs at every call"""

    def __init__(self, outputs):
        super().__init__()
        self.outputs, self.calls = list(outputs), 0

    def forward(self, x, return_attn=False):
        self.calls += 1
        return self.outputs[self.calls - 1]


def _fixture():
    with open(os.path.join(gu.GOLDEN_DIR, "eval_engine.json")) as f:
        return json.load(f)


def test_final_test_with_scene_label_matches_reference_golden(tmp_path):
    from devias_amd.engine_for_slot import final_test_with_scene_label
    fx = _fixture()["scene"]
    student = [torch.tensor(z, dtype=torch.float32) for z in fx["student_scene_logits"]]
    teacher = [torch.tensor(t, dtype=torch.float32) for t in fx["teacher_logits"]]
    batches = [(torch.zeros(len(ids), 1), torch.zeros(len(ids), dtype=torch.long), ids, torch.tensor(c), torch.tensor(s))
               for ids, c, s in zip(fx["ids"], fx["chunk"], fx["split"])]
    model = Replay([(None, (None, z, None), None) for z in student])
    scene_model = Replay([(None, t) for t in teacher])
    model.train(); scene_model.train()
    path = str(tmp_path / "0.txt")
    stats = final_test_with_scene_label(batches, model, scene_model, "cpu", path, num_labels=fx["num_labels"])
    assert not model.training and not scene_model.training and model.calls == scene_model.calls == len(batches)
    assert open(path).read() == fx["file"]
    assert sorted(stats) == ["acc1", "acc5", "loss"]
    assert stats["acc1"] == fx["stats"]["acc1"] and stats["acc5"] == fx["stats"]["acc5"]
    # (the reference averages the batches' fp32 losses, this engine the samples' in float64: equal batches, so equal up to fp32 rounding)
    assert abs(stats["loss"] - fx["stats"]["loss"]) <= 1e-6 * abs(fx["stats"]["loss"])
    assert 0.0 < stats["acc1"] < stats["acc5"] < 100.0


def test_merge_matches_reference_golden(tmp_path):
    from devias_amd.engine_for_slot import merge
    fx = _fixture()["merge"]
    for rank, text in enumerate(fx["files"]):
        (tmp_path / f"{rank}.txt").write_text(text)
    top1, top5 = merge(str(tmp_path), len(fx["files"]))
    assert isinstance(top1, float) and isinstance(top5, float)
    assert top1 == fx["top1"] and top5 == fx["top5"]
    assert 0.0 < top1 < top5 < 100.0
    # the duplicated (chunk, split) is dropped: counted under a key of its own it changes the vote (the fixture's generator checked that on the reference)
    dup = [ln for ln in fx["files"][1].splitlines(True) if ln.startswith("vid3 ") and ln.endswith(" 4 2\n")]
    assert len(dup) == 1
    (tmp_path / "1.txt").write_text(fx["files"][1].replace(dup[0], dup[0][:-len(" 4 2\n")] + " 3 2\n"))
    assert merge(str(tmp_path), 2) != (top1, top5)


def test_merge_reads_what_final_test_with_scene_label_writes(tmp_path):
    """the writer's lines parse back: one video per sample here, so merge's accuracies are the per-sample ones the writer returned"""
    from devias_amd.engine_for_slot import final_test_with_scene_label, merge
    fx = _fixture()["scene"]
    student = [torch.tensor(z, dtype=torch.float32) for z in fx["student_scene_logits"]]
    teacher = [torch.tensor(t, dtype=torch.float32) for t in fx["teacher_logits"]]
    batches = [(torch.zeros(len(ids), 1), torch.zeros(len(ids), dtype=torch.long), ids, torch.tensor(c), torch.tensor(s))
               for ids, c, s in zip(fx["ids"], fx["chunk"], fx["split"])]
    stats = final_test_with_scene_label(batches, Replay([(None, (None, z, None), None) for z in student]), Replay([(None, t) for t in teacher]), "cpu",
                                        str(tmp_path / "0.txt"), num_labels=fx["num_labels"])
    assert merge(str(tmp_path), 1) == (stats["acc1"], stats["acc5"])
