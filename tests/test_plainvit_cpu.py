"""The plain video ViT without a GPU: names, shapes, constructor defaults and optimizer groups against the fixtures the reference wrote
(tests/golden/make_plainvit_goldens.py), the refusals that remain, the C ABI of the pooled-head region (surface, struct layouts, validation before any launch), and
the scene engine on stub models."""
import ctypes
import inspect
import json
import os
import re
import subprocess
from functools import partial

import pytest
import torch

from devias_amd import modeling_finetune as mf
from devias_amd import optim_factory as of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = json.load(open(os.path.join(GOLD, "plainvit_state_dict_keys.json")))
OPTIM = json.load(open(os.path.join(GOLD, "plainvit_optim.json")))
EINVAL, EUNSUPPORTED = -1, -3
_models = {}


def model(mean_pooling, frames=16):
    key = (mean_pooling, frames)
    if key not in _models:
        _models[key] = mf.vit_base_patch16_224(num_classes=365, all_frames=frames, tubelet_size=2, use_mean_pooling=mean_pooling)
    return _models[key]


# ---- surface ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["mean", "cls"])
def test_names_and_shapes_are_the_references(tag):
    m = model(tag == "mean")
    want = KEYS[tag]
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert list(got) == list(want["state_dict"]) and got == want["state_dict"]
    assert [n for n, _ in m.named_parameters()] == want["named_parameters"]
    assert list(m.pos_embed.shape) == want["pos_embed"] and "pos_embed" not in got
    if tag == "mean":
        assert not hasattr(m, "cls_token") and isinstance(m.norm, torch.nn.Identity) and m.fc_norm.eps == 1e-6
    else:
        assert m.fc_norm is None and m.norm.eps == 1e-6 and m.cls_token.shape == (1, 1, 768)


def test_constructor_defaults_are_the_references():
    sig = inspect.signature(mf.VisionTransformer.__init__).parameters
    names = [k for k in sig if k != "self"]
    assert names == list(KEYS["defaults"]) + ["compute_dtype"]
    for k, v in KEYS["defaults"].items():
        if k == "norm_layer":
            assert sig[k].default is torch.nn.LayerNorm
        else:
            assert sig[k].default == v and type(sig[k].default) is type(v), k
    assert sig["use_mean_pooling"].default is True
    # the rates reach the modules the slot model's blocks read them from
    m = mf.VisionTransformer(embed_dim=384, num_heads=6, depth=3, qkv_bias=True, num_classes=7, all_frames=2, fc_drop_rate=0.5, drop_rate=0.1, attn_drop_rate=0.2,
                             drop_path_rate=0.3, init_values=0.1, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    assert isinstance(m.fc_dropout, torch.nn.Dropout) and m.fc_dropout.p == 0.5 and m.pos_drop.p == 0.1 and m.dropout_source is None
    assert [round(b.drop_path_rate, 6) for b in m.blocks] == [0.0, 0.15, 0.3]
    assert m.blocks[1].attn.attn_drop.p == 0.2 and m.blocks[1].attn.proj_drop.p == 0.1 and m.blocks[1].mlp.drop.p == 0.1
    assert m.blocks[0].gamma_1 is not None          # init_values: the parameters exist and stay unapplied, as in Block
    assert m.get_classifier() is m.head
    import devias_amd
    assert isinstance(devias_amd.create_model("vit_base_patch16_224", num_classes=7, all_frames=2), mf.VisionTransformer)


def test_forms_that_are_not_built_raise_with_the_reason():
    with pytest.raises(NotImplementedError, match="learnable"):
        mf.vit_base_patch16_224(use_learnable_pos_emb=True)
    with pytest.raises(NotImplementedError, match="checkpoint"):
        mf.vit_base_patch16_224(use_checkpoint=True)
    with pytest.raises(ValueError, match="fc_drop_rate"):
        mf.vit_base_patch16_224(fc_drop_rate=1.0)
    for mp in (True, False):
        with pytest.raises(RuntimeError, match="MI355X"):
            model(mp, 8).train()(torch.zeros(1, 3, 8, 224, 224))
        with pytest.raises(NotImplementedError, match="attention maps"):
            model(mp, 8)(torch.zeros(1, 3, 8, 224, 224), return_attn=True)
    from devias_amd import engine_for_finetuning_scene as eng
    with pytest.raises(NotImplementedError, match="mixup"):
        eng.train_one_epoch(model(True), model(False), None, [], None, "cpu", 0, mixup_fn=lambda s, t: (s, t))


@pytest.mark.parametrize("case", sorted(OPTIM["groups"]))
def test_parameter_groups_match_reference(case):
    g = OPTIM["groups"][case]
    m = model(g["use_mean_pooling"], 8)
    assert m.get_num_layers() == g["num_layers"]
    assigner = of.LayerDecayValueAssigner.from_decay(g["layer_decay"], g["num_layers"]) if g["layer_decay"] < 1.0 else None
    groups, names = of.get_parameter_groups(m, g["weight_decay"], m.no_weight_decay(), assigner.get_layer_id if assigner else None,
                                            assigner.get_scale if assigner else None, return_names=True)
    got = [[k, v["weight_decay"], v["lr_scale"], v["params"]] for k, v in names.items()]
    assert got == g["groups"]
    assert sum(len(x["params"]) for x in groups) == len(list(m.named_parameters()))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------
POOL_SYMBOLS = ("devias_pool_head_workspace_bytes", "devias_pool_head_save_bytes", "devias_pool_head_fwd", "devias_pool_head_bwd", "devias_pool_head_launches")


def test_abi_surface_and_struct_layouts(tmp_path):
    import pool_head_bounds as pb
    from devias_amd import _lib, build
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "devias_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t|void|const char\*)\s+(devias_\w+)\s*\(", hdr, flags=re.M))
    for name in POOL_SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.devias_version() >= 176 and _lib.ABI_VERSION >= 176
    assert "token_head.hip" in build.SOURCES
    # a counter of its own: neither bank grew
    assert lib.devias_counter(25) == -1 and lib.devias_region_counter(2) == -1 and "pool_head" not in _lib.COUNTERS and "pool_head" not in _lib.REGION_COUNTERS
    consts = {n: int(v) for n, v in re.findall(r"#define DEVIAS_POOL_(\w+) (\d+)", hdr)}
    assert consts == {"MEAN": _lib.POOL_MEAN, "CLS": _lib.POOL_CLS, "HEAD_CHUNK": _lib.POOL_HEAD_CHUNK} and (pb.MEAN, pb.CLS, pb.CHUNK) == (0, 1, _lib.POOL_HEAD_CHUNK)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "devias_amd.h"', 'int main(void) {']
    structs = {"devias_pool_head_args": _lib.PoolHeadArgs, "devias_pool_head_grads": _lib.PoolHeadGrads}
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


def _pargs(p, B=3, Nt=70, D=384, C=101, dtype=1, pool=0, **kw):
    from devias_amd import _lib
    a = _lib.PoolHeadArgs()
    a.struct_size = ctypes.sizeof(_lib.PoolHeadArgs)
    a.B, a.Nt, a.D, a.C, a.dtype, a.pool, a.eps = B, Nt, D, C, dtype, pool, 1e-6
    for n in ("W", "bias", "ln_w", "ln_b", "ws"):
        setattr(a, n, p)
    a.ws_bytes = max(_lib.load().devias_pool_head_workspace_bytes(B, Nt, D, C, dtype), 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _pgrads(p, **kw):
    from devias_amd import _lib
    g = _lib.PoolHeadGrads()
    g.struct_size = ctypes.sizeof(_lib.PoolHeadGrads)
    for n in ("dW", "db", "dln_w", "dln_b"):
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
    ok = _pargs(p)
    assert ok.ws_bytes > 0
    ref = lambda a: ctypes.byref(a) if a is not None else None      # noqa: E731
    fwd = lambda a, h=p, tok=p, z=p, save=p: lib.devias_pool_head_fwd(ref(a), h, tok, z, save, None)      # noqa: E731
    bwd = lambda a, g, save=p, dz=p, dtok=None, dx=p: lib.devias_pool_head_bwd(ref(a), save, dz, dtok, dx, ref(g), None)      # noqa: E731
    cases = [("null args", EINVAL, None), ("wrong struct_size", EINVAL, _pargs(p, struct_size=ok.struct_size - 8)), ("bad dtype", EINVAL, _pargs(p, dtype=7)),
             ("bad pool", EINVAL, _pargs(p, pool=2)), ("D = 512", EUNSUPPORTED, _pargs(p, D=512)), ("B = 0", EUNSUPPORTED, _pargs(p, B=0)),
             ("Nt = 0", EUNSUPPORTED, _pargs(p, Nt=0)), ("C = 1", EUNSUPPORTED, _pargs(p, C=1)), ("B Nt >= 2^31", EUNSUPPORTED, _pargs(p, B=1 << 20, Nt=1 << 11)),
             ("null parameter", EINVAL, _pargs(p, ln_w=None)), ("null ws", EINVAL, _pargs(p, ws=None)), ("unaligned ws", EINVAL, _pargs(p, ws=p + 4)),
             ("a workspace one byte short", EINVAL, _pargs(p, ws_bytes=ok.ws_bytes - 1)), ("eps = 0", EINVAL, _pargs(p, eps=0.0))]
    for what, code, a in cases:
        assert fwd(a) == code and b"devias_pool_head_fwd" in lib.devias_last_error(), what
        assert bwd(a, _pgrads(p)) == code and b"devias_pool_head_bwd" in lib.devias_last_error(), what
    assert fwd(ok, h=None) == EINVAL and fwd(ok, tok=None) == EINVAL and fwd(ok, z=None) == EINVAL and fwd(ok, save=p + 8) == EINVAL and fwd(ok, h=p + 2) == EINVAL
    assert bwd(ok, None) == EINVAL and bwd(ok, _pgrads(p, struct_size=8)) == EINVAL and b"struct_size" in lib.devias_last_error()
    assert bwd(ok, _pgrads(p, dln_b=None)) == EINVAL and bwd(ok, _pgrads(p), save=None) == EINVAL and bwd(ok, _pgrads(p), dz=None) == EINVAL
    assert bwd(ok, _pgrads(p), dx=None) == EINVAL and bwd(ok, _pgrads(p), dx=p + 8) == EINVAL
    q = lib.devias_pool_head_workspace_bytes
    assert q(3, 70, 512, 101, 1) == 0 and q(0, 70, 384, 101, 1) == 0 and q(3, 0, 384, 101, 1) == 0 and q(3, 70, 384, 1, 1) == 0 and q(3, 70, 384, 101, 7) == 0
    assert q(32, 1568, 768, 365, 1) > q(3, 70, 384, 101, 1) > 0
    # the chunk sums: cdiv(Nt, chunk) fp32 rows per clip
    assert q(32, 1568, 768, 365, 1) - q(32, 64, 768, 365, 1) == 32 * (25 - 1) * 768 * 4
    s = lib.devias_pool_head_save_bytes
    assert s(12, 768, 1) >= 12 * 768 * 4 + 12 * 4 + 12 * 768 * 2 and s(12, 768, 0) > s(12, 768, 1) and s(12, 512, 1) == 0 and s(0, 768, 1) == 0
    assert lib.devias_pool_head_launches() == 0
    assert sum(lib.devias_counter(i) for i in _lib.COUNTERS.values()) == 0


# ---- the scene engine on stub models ----------------------------------------------------------------------------------------------------------
class _Stub(torch.nn.Module):
    """(token, logits) from the clip's mean: logits = mean * w, a linear model the CPU can train"""

    def __init__(self, C, shift=0):
        super().__init__()
        self.w = torch.nn.Parameter(torch.arange(C, dtype=torch.float32).roll(shift) / C)
        self.calls = 0

    def forward(self, x, return_attn=False):
        self.calls += 1
        m = x.float().mean(dim=(1, 2, 3, 4))
        z = m[:, None] * self.w[None, :]
        return m[:, None], z


def test_scene_engine_uses_the_teachers_argmax_and_ignores_the_callers_targets(tmp_path):
    from devias_amd import engine_for_finetuning_scene as eng
    C, B = 5, 4
    teacher, student = _Stub(C, shift=2), _Stub(C)
    clips = [torch.randn(B, 3, 2, 4, 4, generator=torch.Generator().manual_seed(i)) + (1.0 if i % 2 else -1.0) for i in range(4)]
    want = [teacher(c)[1].argmax(1) for c in clips]
    assert len({int(t[0]) for t in want}) == 2          # positive and negative clip means pick different classes
    seen = []

    def crit(out, target):
        seen.append(target.clone())
        return torch.nn.functional.cross_entropy(out, target)

    bogus = torch.full((B,), 10 ** 6, dtype=torch.int64)
    opt = torch.optim.SGD(student.parameters(), lr=0.1)
    w0 = student.w.detach().clone()
    t_calls = teacher.calls
    stats = eng.train_one_epoch(student, teacher, crit, [(c, bogus) for c in clips], opt, "cpu", 0, update_freq=2, check_finite_every=2)
    assert [s.tolist() for s in seen] == [w.tolist() for w in want] and all(s.dtype == torch.int64 for s in seen)
    assert teacher.calls == t_calls + 4 and not teacher.training and student.training
    assert teacher.w.grad is None and not torch.equal(student.w.detach(), w0) and torch.isfinite(torch.tensor(stats["loss"]))
    # validation and final_test: the targets are the teacher's, the file has the slot engine's line format
    loader = [(c, bogus, ["vid%d_%d" % (i, j) for j in range(B)], torch.zeros(B, dtype=torch.int64), torch.arange(B)) for i, c in enumerate(clips)]
    val = eng.validation_one_epoch(loader, student, teacher, "cpu")
    assert set(val) == {"loss", "acc1", "acc5"} and val["acc5"] == 100.0
    path = tmp_path / "0.txt"
    fin = eng.final_test(loader, student, teacher, "cpu", str(path))
    assert fin["acc1"] == val["acc1"]
    rows = path.read_text().splitlines()
    assert len(rows) == 1 + 4 * B and re.fullmatch(r"[\d.]+, [\d.]+", rows[0])
    with torch.no_grad():
        z = student(clips[0])[1]
    first = rows[1]
    assert first == "vid0_0 {} {} 0 0".format(str(z[0].numpy().tolist()), int(want[0][0])) and "output :" not in first
    top1, top5 = eng.merge(str(tmp_path), 1)[:2]
    assert abs(top1 - fin["acc1"]) < 1e-9 and top5 == 100.0
