"""The two-token multi-task baseline without a GPU: names, shapes, constructor defaults and optimizer groups against the fixtures the reference wrote
(tests/golden/make_multitask_goldens.py), the refusals that remain, the C ABI of the two-token head region and the distillation loss (surface, struct layouts,
validation before any launch), and the engine on stub models."""
import ctypes
import inspect
import json
import os
import re
import subprocess
from functools import partial

import pytest
import torch

from devias_amd import modeling_multi_task as mm
from devias_amd import optim_factory as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = json.load(open(os.path.join(GOLD, "multitask_state_dict_keys.json")))
OPTIM = json.load(open(os.path.join(GOLD, "multitask_optim.json")))
EINVAL, EUNSUPPORTED = -1, -3
TAGS = ("multitask", "multitask_unified")
_models = {}


def model(unified, frames=16):
    key = (unified, frames)
    if key not in _models:
        _models[key] = mm.disentangle_vit_base_patch16_224(num_classes=400, all_frames=frames, tubelet_size=2, unified_head=unified)
    return _models[key]


# ---- surface ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_names_and_shapes_are_the_references(tag):
    unified = tag == "multitask_unified"
    m = model(unified)
    want = KEYS[tag]
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want["state_dict"]) and got == want["state_dict"]
    names = [n for n, _ in m.named_parameters()]
    assert names == want["named_parameters"] and names[:2] == ["cls_token", "scene_token"]
    assert list(m.pos_embed.shape) == want["pos_embed"] == [1, 1568 + 2, 768] and "pos_embed" not in got
    assert sorted(m.no_weight_decay()) == want["no_weight_decay"] == ["cls_token", "pos_embed", "scene_token"]
    assert m.norm.eps == 1e-6
    if unified:
        assert not hasattr(m, "scene_head") and m.head.weight.shape == (400 + 365, 768)
    else:
        assert names[-4:] == ["head.weight", "head.bias", "scene_head.weight", "scene_head.bias"] and m.scene_head.weight.shape == (365, 768)


def test_constructor_defaults_are_the_references():
    sig = inspect.signature(mm.VisionTransformer.__init__).parameters
    names = [k for k in sig if k != "self"]
    assert names == list(KEYS["defaults"]) + ["compute_dtype"]
    for k, v in KEYS["defaults"].items():
        if k == "norm_layer":
            assert sig[k].default is torch.nn.LayerNorm
        else:
            assert sig[k].default == v and type(sig[k].default) is type(v), k
    m = mm.VisionTransformer(embed_dim=384, num_heads=6, depth=3, qkv_bias=True, num_classes=7, num_scene_classes=5, all_frames=2, fc_drop_rate=0.5, drop_rate=0.1,
                             attn_drop_rate=0.2, drop_path_rate=0.3, init_scale=0.5, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    assert isinstance(m.fc_dropout, torch.nn.Dropout) and m.fc_dropout.p == 0.5 and m.pos_drop.p == 0.1 and m.dropout_source is None
    assert [round(b.drop_path_rate, 6) for b in m.blocks] == [0.0, 0.15, 0.3]
    assert m.head.weight.shape == (7, 384) and m.scene_head.weight.shape == (5, 384) and m.get_classifier() is m.head
    # init_scale multiplies both heads: the same draws at init_scale 1 and 0.5
    pair = []
    for scale in (1.0, 0.5):
        torch.manual_seed(3)
        pair.append(mm.VisionTransformer(embed_dim=384, num_heads=6, depth=1, num_classes=7, num_scene_classes=5, all_frames=2, init_scale=scale))
    assert torch.equal(pair[1].head.weight.detach(), 0.5 * pair[0].head.weight.detach()) and float(pair[0].scene_head.weight.detach().abs().max()) > 0
    assert torch.equal(pair[1].scene_head.weight.detach(), 0.5 * pair[0].scene_head.weight.detach()) and torch.equal(pair[1].cls_token.detach(), pair[0].cls_token.detach())
    u = mm.VisionTransformer(embed_dim=384, num_heads=6, depth=1, num_classes=7, num_scene_classes=5, all_frames=2, unified_head=True, init_scale=0.0)
    assert u.head.weight.shape == (12, 384) and float(u.head.weight.detach().abs().max()) == 0.0
    import devias_amd
    assert isinstance(devias_amd.create_model("disentangle_vit_base_patch16_224", num_classes=7, all_frames=2), mm.VisionTransformer)
    assert devias_amd.disentangle_vit_base_patch16_224 is mm.disentangle_vit_base_patch16_224
    from devias_amd import engine_for_multi_task, multi_task_loss
    assert devias_amd.MultiTaskTrainLoss is multi_task_loss.TrainLoss and engine_for_multi_task.merge is __import__("devias_amd.engine_for_slot", fromlist=["merge"]).merge


def test_forms_that_are_not_built_raise_with_the_reason():
    with pytest.raises(NotImplementedError, match="learnable"):
        mm.disentangle_vit_base_patch16_224(use_learnable_pos_emb=True)
    with pytest.raises(NotImplementedError, match="checkpoint"):
        mm.disentangle_vit_base_patch16_224(use_checkpoint=True)
    with pytest.raises(ValueError, match="fc_drop_rate"):
        mm.disentangle_vit_base_patch16_224(fc_drop_rate=1.0)
    for unified in (False, True):
        with pytest.raises(RuntimeError, match="MI355X"):
            model(unified, 8).train()(torch.zeros(1, 3, 8, 224, 224))
        with pytest.raises(NotImplementedError, match="attention maps"):
            model(unified, 8)(torch.zeros(1, 3, 8, 224, 224), return_attn=True)
    from devias_amd import engine_for_multi_task as eng
    from devias_amd.multi_task_loss import TrainLoss
    with pytest.raises(NotImplementedError, match="mixup"):
        eng.train_one_epoch(model(False), model(True), None, [], None, "cpu", 0, mixup_fn=lambda s, t: (s, t))
    with pytest.raises(NotImplementedError, match="logit_criterion"):
        TrainLoss(None, "MSE")
    tl = TrainLoss(lambda z, y: z.sum(), "KL", unified_head=True, num_action_classes=4)
    with pytest.raises(ValueError, match="left-padded"):
        tl(((None, torch.zeros(2, 9)), (None, torch.zeros(2, 8))), (None, torch.zeros(2, 5)), torch.zeros(2, dtype=torch.int64))


@pytest.mark.parametrize("case", sorted(OPTIM["groups"]))
def test_parameter_groups_match_reference(case):
    g = OPTIM["groups"][case]
    m = model(g["unified_head"], 8)
    assert m.get_num_layers() == g["num_layers"]
    assigner = of.LayerDecayValueAssigner.from_decay(g["layer_decay"], g["num_layers"]) if g["layer_decay"] < 1.0 else None
    groups, names = of.get_parameter_groups(m, g["weight_decay"], m.no_weight_decay(), assigner.get_layer_id if assigner else None,
                                            assigner.get_scale if assigner else None, return_names=True)
    got = [[k, v["weight_decay"], v["lr_scale"], v["params"]] for k, v in names.items()]
    assert got == g["groups"]
    assert sum(len(x["params"]) for x in groups) == len(list(m.named_parameters()))
    if assigner:          # the reference sends scene_token to the LAST layer id (it is not in its stem list), cls_token to the stem
        where = {n: k for k, _, _, ps in got for n in ps}
        assert where["cls_token"] == "layer_0_no_decay" and where["scene_token"] == "layer_%d_no_decay" % (g["num_layers"] + 1)


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ("devias_two_token_head_workspace_bytes", "devias_two_token_head_save_bytes", "devias_two_token_head_fwd", "devias_two_token_head_bwd",
           "devias_two_token_head_launches", "devias_distill_workspace_bytes", "devias_distill_fwd", "devias_distill_bwd")


def test_abi_surface_and_struct_layouts(tmp_path):
    from devias_amd import _lib, build
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "devias_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t|void|const char\*)\s+(devias_\w+)\s*\(", hdr, flags=re.M))
    for name in SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.devias_version() >= 177 and _lib.ABI_VERSION >= 177
    assert "token_head.hip" in build.SOURCES and "distill.hip" in build.SOURCES
    # a counter of its own: neither bank grew
    assert lib.devias_counter(25) == -1 and lib.devias_region_counter(2) == -1
    consts = {n: int(v) for n, v in re.findall(r"#define DEVIAS_DISTILL_(\w+) (\d+)", hdr)}
    assert consts == {"KL": _lib.DISTILL_KL, "CE": _lib.DISTILL_CE}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "devias_amd.h"', 'int main(void) {']
    structs = {"devias_two_token_head_args": _lib.TwoTokenHeadArgs, "devias_two_token_head_grads": _lib.TwoTokenHeadGrads}
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname} {fl[0]} %zu\\n", offsetof({cname}, {fl[0]}));' for fl in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()}
    for cname, cls in structs.items():
        assert got[(cname, "size")] == ctypes.sizeof(cls)
        assert cls._fields_[0][0] == "struct_size" and cls.struct_size.offset == 0
        for fl in cls._fields_:
            assert got[(cname, fl[0])] == getattr(cls, fl[0]).offset, (cname, fl[0])


def _targs(p, B=3, Nt=70, D=384, Ca=101, Cs=365, dtype=1, unified=0, **kw):
    from devias_amd import _lib
    a = _lib.TwoTokenHeadArgs()
    a.struct_size = ctypes.sizeof(_lib.TwoTokenHeadArgs)
    a.B, a.Nt, a.D, a.Ca, a.Cs, a.dtype, a.unified, a.eps = B, Nt, D, Ca, Cs, dtype, unified, 1e-6
    for n in ("Wa", "Ws", "ba", "bs", "ln_w", "ln_b", "ws"):
        setattr(a, n, p)
    a.ws_bytes = max(_lib.load().devias_two_token_head_workspace_bytes(B, Nt, D, Ca, Cs, unified, dtype), 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _tgrads(p, **kw):
    from devias_amd import _lib
    g = _lib.TwoTokenHeadGrads()
    g.struct_size = ctypes.sizeof(_lib.TwoTokenHeadGrads)
    for n in ("dWa", "dba", "dWs", "dbs", "dln_w", "dln_b"):
        setattr(g, n, p)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_entry_points_validate_before_any_launch():
    """every case returns its code with a message naming the entry point; nothing is launched (no device is needed to get there) and no counter moves"""
    from devias_amd import _lib
    lib = _lib.load()
    lib.devias_counters_reset()
    buf = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(buf) + 255) & ~255
    ok = _targs(p)
    assert ok.ws_bytes > 0
    ref = lambda a: ctypes.byref(a) if a is not None else None      # noqa: E731
    fwd = lambda a, h=p, ta=p, ts=p, za=p, zs=p, save=p: lib.devias_two_token_head_fwd(ref(a), h, ta, ts, za, zs, save, None)      # noqa: E731
    bwd = lambda a, g, save=p, dza=p, dzs=p, dx=p: lib.devias_two_token_head_bwd(ref(a), save, dza, dzs, None, None, dx, ref(g), None)      # noqa: E731
    cases = [("null args", EINVAL, None), ("wrong struct_size", EINVAL, _targs(p, struct_size=ok.struct_size - 8)), ("bad dtype", EINVAL, _targs(p, dtype=7)),
             ("bad unified", EINVAL, _targs(p, unified=2)), ("unified with Ca != Cs", EINVAL, _targs(p, Ca=101, Cs=365, unified=1, ws_bytes=1 << 30)),
             ("D = 512", EUNSUPPORTED, _targs(p, D=512)), ("B = 0", EUNSUPPORTED, _targs(p, B=0)), ("Nt = 1", EUNSUPPORTED, _targs(p, Nt=1)),
             ("Ca = 1", EUNSUPPORTED, _targs(p, Ca=1)), ("Cs = 1", EUNSUPPORTED, _targs(p, Cs=1)), ("B Nt >= 2^31", EUNSUPPORTED, _targs(p, B=1 << 20, Nt=1 << 11)),
             ("null parameter", EINVAL, _targs(p, ln_w=None)), ("null scene head", EINVAL, _targs(p, Ws=None)), ("null ws", EINVAL, _targs(p, ws=None)),
             ("unaligned ws", EINVAL, _targs(p, ws=p + 4)), ("a workspace one byte short", EINVAL, _targs(p, ws_bytes=ok.ws_bytes - 1)), ("eps = 0", EINVAL, _targs(p, eps=0.0))]
    for what, code, a in cases:
        assert fwd(a) == code and b"devias_two_token_head_fwd" in lib.devias_last_error(), what
        assert bwd(a, _tgrads(p)) == code and b"devias_two_token_head_bwd" in lib.devias_last_error(), what
    assert fwd(ok, h=None) == EINVAL and fwd(ok, ta=None) == EINVAL and fwd(ok, ts=None) == EINVAL and fwd(ok, za=None) == EINVAL and fwd(ok, zs=None) == EINVAL
    assert fwd(ok, save=p + 8) == EINVAL and fwd(ok, h=p + 2) == EINVAL
    assert bwd(ok, None) == EINVAL and bwd(ok, _tgrads(p, struct_size=8)) == EINVAL and b"struct_size" in lib.devias_last_error()
    assert bwd(ok, _tgrads(p, dln_b=None)) == EINVAL and bwd(ok, _tgrads(p, dWs=None)) == EINVAL and bwd(ok, _tgrads(p), save=None) == EINVAL
    assert bwd(ok, _tgrads(p), dza=None) == EINVAL and bwd(ok, _tgrads(p), dzs=None) == EINVAL and bwd(ok, _tgrads(p), dzs=p + 8) == EINVAL
    assert bwd(ok, _tgrads(p), dx=None) == EINVAL and bwd(ok, _tgrads(p), dx=p + 8) == EINVAL
    q = lib.devias_two_token_head_workspace_bytes
    assert q(3, 70, 512, 101, 365, 0, 1) == 0 and q(0, 70, 384, 101, 365, 0, 1) == 0 and q(3, 1, 384, 101, 365, 0, 1) == 0 and q(3, 70, 384, 1, 365, 0, 1) == 0
    assert q(3, 70, 384, 101, 365, 0, 7) == 0 and q(3, 70, 384, 101, 365, 1, 1) == 0 and q(3, 70, 384, 466, 466, 1, 1) > 0
    assert q(32, 1570, 768, 400, 365, 0, 1) > q(3, 70, 384, 101, 365, 0, 1) > 0
    assert q(32, 1570, 768, 400, 365, 0, 1) == q(32, 2, 768, 400, 365, 0, 1)          # nothing in the workspace grows with Nt: the forward reads 2B rows
    s = lib.devias_two_token_head_save_bytes
    assert s(12, 768, 1) >= 2 * (12 * 768 * 4 + 12 * 4 + 12 * 768 * 2) and s(12, 768, 0) > s(12, 768, 1) and s(12, 512, 1) == 0 and s(0, 768, 1) == 0
    # the distillation loss
    dfwd = lambda z=p, t=p, B=3, C=365, Ct=365, dt=1, mode=0, w=1.0, tmin=p, loss=p, ws=p: lib.devias_distill_fwd(z, t, B, C, Ct, dt, mode, w, tmin, loss, ws, None)      # noqa: E731
    dbwd = lambda z=p, t=p, B=3, C=365, Ct=365, dt=1, mode=0, w=1.0, tmin=p, g=p, dz=p: lib.devias_distill_bwd(z, t, B, C, Ct, dt, mode, w, tmin, g, dz, None)      # noqa: E731
    for kw in (dict(z=None), dict(t=None), dict(B=0), dict(Ct=1, C=1), dict(C=364), dict(C=1 << 24), dict(dt=7), dict(mode=2), dict(w=float("nan")),
               dict(C=765, tmin=None)):
        assert dfwd(**kw) == EINVAL and b"devias_distill_fwd" in lib.devias_last_error(), kw
        assert dbwd(**kw) == EINVAL and b"devias_distill_bwd" in lib.devias_last_error(), kw
    assert dfwd(loss=None) == EINVAL and dfwd(ws=None) == EINVAL and dbwd(g=None) == EINVAL and dbwd(dz=None) == EINVAL
    assert lib.devias_distill_workspace_bytes(8) >= 32 and lib.devias_distill_workspace_bytes(0) == 0
    assert lib.devias_two_token_head_launches() == 0
    assert sum(lib.devias_counter(i) for i in _lib.COUNTERS.values()) == 0


# ---- the engine on stub models ----------------------------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """((token, action logits), (token, scene logits)) from the clip's mean -- or, as a teacher, (token, scene logits): linear models the CPU can train"""

    def __init__(self, Ca, Cs, teacher=False, unified=False):
        super().__init__()
        self.wa = torch.nn.Parameter(torch.arange(Ca, dtype=torch.float32) / Ca)
        self.ws = torch.nn.Parameter(torch.arange((Ca if unified else 0) + Cs, dtype=torch.float32).roll(2) / Cs)
        self.teacher, self.calls = teacher, 0

    def forward(self, x, return_attn=False):
        self.calls += 1
        m = x.float().mean(dim=(1, 2, 3, 4))
        tok = m[:, None]
        if self.teacher:
            return tok, m[:, None] * self.ws[None, :]
        return (tok, m[:, None] * self.wa[None, :]), (tok, m[:, None] * self.ws[None, :])


def _cpu_train_loss(student_output, teacher_outputs, target):
    """the reference's TrainLoss in plain torch (the package's own runs HIP kernels): what the engine hands its criterion, and what it does with the result"""
    import multitask_ref as mr
    (_, za), (_, zs) = student_output
    total, action, logit = mr.train_loss(za, zs, teacher_outputs[1], target, 0.1, "KL")
    return total, za, {"action_loss": float(action.detach()), "logit_loss": float(logit.detach())}


@pytest.mark.parametrize("unified", [False, True], ids=["separate", "unified"])
def test_engine_on_stub_models(tmp_path, unified):
    from devias_amd import engine_for_multi_task as eng
    Ca, Cs, B = 6, 5, 4
    student, teacher = _Stub(Ca, Cs, unified=unified), _Stub(Ca, Cs, teacher=True)
    clips = [torch.randn(B, 3, 2, 4, 4, generator=torch.Generator().manual_seed(i)) + (1.0 if i % 2 else -1.0) for i in range(4)]
    targets = [torch.randint(0, Ca, (B,), generator=torch.Generator().manual_seed(10 + i)) for i in range(4)]
    seen = []

    def crit(so, to, target):
        seen.append((target.clone(), to[1].requires_grad))
        if unified:          # the stub criterion distils the scene columns only
            so = (so[0], (so[1][0], so[1][1][:, Ca:]))
        return _cpu_train_loss(so, to, target)

    opt = torch.optim.SGD(student.parameters(), lr=0.1)
    w0 = (student.wa.detach().clone(), student.ws.detach().clone())
    stats = eng.train_one_epoch(student, teacher, crit, [(c, t, None, None) for c, t in zip(clips, targets)], opt, "cpu", 0, update_freq=2, check_finite_every=2)
    assert [s[0].tolist() for s in seen] == [t.tolist() for t in targets] and not any(s[1] for s in seen)          # the caller's targets; the teacher under no_grad
    assert teacher.calls == 4 and not teacher.training and student.training and teacher.ws.grad is None
    assert not torch.equal(student.wa.detach(), w0[0]) and not torch.equal(student.ws.detach(), w0[1])
    assert set(stats) >= {"loss", "action_loss", "logit_loss", "lr"} and abs(stats["action_loss"] + stats["logit_loss"] - 2 * stats["loss"]) < 1e-5      # loss / update_freq
    # validation and final_test score the ACTION logits; final_test_with_scene_label the SCENE logits against the teacher's argmax
    loader = [(c, t, ["vid%d_%d" % (i, j) for j in range(B)], torch.zeros(B, dtype=torch.int64), torch.arange(B)) for i, (c, t) in enumerate(zip(clips, targets))]
    val = eng.validation_one_epoch(loader, student, "cpu")
    with torch.no_grad():
        outs = [student(c) for c in clips]
        za, y = torch.cat([o[0][1] for o in outs]), torch.cat(targets)
        zs = torch.cat([o[1][1] for o in outs])[:, (Ca if unified else 0):]
        ys = torch.cat([teacher(c)[1].argmax(1) for c in clips])
    want = {"loss": float(torch.nn.functional.cross_entropy(za, y)), "acc1": 100.0 * float((za.argmax(1) == y).float().mean()), "acc5": 100.0 * float((za.topk(5, 1)[1] == y[:, None]).any(1).float().mean())}
    assert set(val) == {"loss", "acc1", "acc5"} and all(abs(val[k] - want[k]) < 1e-4 for k in want), (val, want)
    fin = eng.final_test(loader, student, "cpu", str(tmp_path / "0.txt"))
    assert all(abs(fin[k] - want[k]) < 1e-4 for k in want)
    rows = (tmp_path / "0.txt").read_text().splitlines()
    assert len(rows) == 1 + 4 * B and re.fullmatch(r"[\d.]+, [\d.]+", rows[0])
    assert rows[1] == "vid0_0 {} {} 0 0".format(str(za[0].numpy().tolist()), int(y[0]))
    top1, top5 = eng.merge(str(tmp_path), 1)[:2]
    assert abs(top1 - fin["acc1"]) < 1e-9 and abs(top5 - fin["acc5"]) < 1e-9
    sdir = tmp_path / "scene"
    sdir.mkdir()
    sc = eng.final_test_with_scene_label(loader, student, teacher, "cpu", str(sdir / "0.txt"), num_labels=Ca, unified_head=unified)
    swant = {"loss": float(torch.nn.functional.cross_entropy(zs, ys)), "acc1": 100.0 * float((zs.argmax(1) == ys).float().mean())}
    assert all(abs(sc[k] - swant[k]) < 1e-4 for k in swant), (sc, swant)
    srows = (sdir / "0.txt").read_text().splitlines()
    assert len(srows) == 1 + 4 * B and srows[1] == "vid0_0 {} {} 0 0".format(str(zs[0].numpy().tolist()), int(ys[0]))
    assert abs(eng.merge(str(sdir), 1)[0] - sc["acc1"]) < 1e-9
