"""The downstream recipe without a GPU: the model's surface against the reference's (tests/golden/downstream_state_dict_keys.json), the checkpoint report when a
slot-model checkpoint is loaded, the optimizer groups (downstream_optim.json), the C ABI of the fused head region and the cross-entropy (struct layouts, argument
validation before any launch, no scratch in the compiled kernels) and tests/downstream_ref.py against the step the real reference ran (downstream_t8.npz)."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import devias_amd
import downstream_ref as dr
from devias_amd import build, checkpoint, optim_factory as of, synth
from devias_amd import modeling_slot_fusion as msf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KEYS = json.load(open(os.path.join(GOLD, "downstream_state_dict_keys.json")))
OPTIM = json.load(open(os.path.join(GOLD, "downstream_optim.json")))
CFG = dict(num_classes=400, num_scene_classes=365, all_frames=8, num_latents=2, agg_weights_tie=True, agg_depth=8, head_type="mlp", slot_fusion_method="concat",
           downstream_nb_classes=48, use_input_ln=True)
# the reference constructor's keywords, in its order (model/modeling_slot_fusion.py:217-247)
REF_KEYWORDS = ["img_size", "patch_size", "in_chans", "num_classes", "embed_dim", "depth", "num_heads", "mlp_ratio", "qkv_bias", "qk_scale", "fc_drop_rate", "drop_rate",
                "attn_drop_rate", "drop_path_rate", "norm_layer", "init_values", "use_learnable_pos_emb", "init_scale", "all_frames", "tubelet_size", "use_checkpoint",
                "num_latents", "head_type", "agg_weights_tie", "agg_depth", "num_scene_classes", "slot_fusion_method", "downstream_nb_classes", "use_input_ln"]
EINVAL, EUNSUPPORTED = -1, -3
_model = []


def model():
    if not _model:
        _model.append(devias_amd.create_model("slot_fusion_vit_base_patch16_224", **CFG))
    return _model[0]


# ---- surface ---------------------------------------------------------------------------------------------------------------------------------
def test_names_and_shapes_are_the_references():
    want = KEYS["slot_fusion_vit_base_patch16_224.tied_s2_d8_cd48"]
    got = {k: list(v.shape) for k, v in model().state_dict().items()}
    assert list(got) == list(want) and got == want
    assert len(list(model().named_parameters())) == KEYS["named_parameters"] == 196


def test_constructor_keywords_and_factories():
    params = list(inspect.signature(msf.VisionTransformer.__init__).parameters)[1:]
    assert params == REF_KEYWORDS + ["compute_dtype"]
    ref_defaults = dict(num_latents=4, head_type="linear", agg_weights_tie=True, agg_depth=4, num_scene_classes=365, slot_fusion_method="concat", downstream_nb_classes=50,
                        use_input_ln=True, fc_drop_rate=0.0, all_frames=16)
    sig = inspect.signature(msf.VisionTransformer.__init__).parameters
    assert {k: sig[k].default for k in ref_defaults} == ref_defaults
    for name, D, depth in (("small", 384, 12), ("base", 768, 12), ("large", 1024, 24)):
        assert "slot_fusion_vit_%s_patch16_224" % name in devias_amd.modeling_slot._MODEL_REGISTRY
    m = model()
    assert m.action_norm.eps == m.scene_norm.eps == 1e-6 and m.fusion_head.fc_action_ln.eps == m.fusion_head.fc_input_ln.eps == 1e-5
    assert not hasattr(m, "mask_predictor")
    no_ln = devias_amd.create_model("slot_fusion_vit_small_patch16_224", **dict(CFG, use_input_ln=False, all_frames=4))
    assert not any("fc_input_ln" in n for n, _ in no_ln.named_parameters()) and no_ln.embed_dim == 384


def test_forms_the_reference_does_not_run_raise_with_the_reason():
    with pytest.raises(NotImplementedError, match="gap"):
        devias_amd.create_model("slot_fusion_vit_base_patch16_224", **dict(CFG, slot_fusion_method="gap"))
    with pytest.raises(NotImplementedError, match="Linear.forward"):
        devias_amd.create_model("slot_fusion_vit_base_patch16_224", **dict(CFG, head_type="linear"))
    with pytest.raises(RuntimeError, match="MI355X"):
        model()(torch.zeros(1, 3, 8, 224, 224))
    from devias_amd import engine_for_finetuning as eng
    with pytest.raises(NotImplementedError, match="mixup"):
        eng.train_one_epoch(model(), None, [], None, "cpu", 0, mixup_fn=lambda s, t: (s, t))
    from devias_amd.losses import LabelSmoothingCrossEntropy
    with pytest.raises(ValueError):
        LabelSmoothingCrossEntropy(1.0)


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["model", "module"])
def test_slot_checkpoint_loads_with_exactly_the_expected_report(key, capsys):
    slot = devias_amd.create_model("slot_vit_base_patch16_224", num_classes=400, all_frames=8, num_latents=2, slot_matching_method="matching", agg_weights_tie=True,
                                   agg_depth=8, num_scene_classes=365)
    synth.fill_module_(slot, seed=3)
    m = devias_amd.create_model("slot_fusion_vit_base_patch16_224", **CFG)
    sd = checkpoint.prepare_finetune_state_dict(m, {key: slot.state_dict(), "epoch": 7}, num_frames=8)
    missing, unexpected, errors = checkpoint.load_state_dict(m, sd)
    capsys.readouterr()
    own = list(m.state_dict())
    assert missing == [k for k in own if k.startswith(("action_norm.", "scene_norm.", "fusion_head."))]
    assert unexpected == [k for k in slot.state_dict() if k.startswith("mask_predictor.")] and len(unexpected) == 6 and not errors
    for k, v in slot.state_dict().items():
        if not k.startswith("mask_predictor."):
            assert torch.equal(m.state_dict()[k], v), k          # the pre-trained head included: it selects the slots


# ---- optimizer groups ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(OPTIM["groups"]))
def test_parameter_groups_match_reference(case):
    g = OPTIM["groups"][case]
    m = model()
    assert m.get_num_layers() == g["num_layers"]
    assigner = of.LayerDecayValueAssigner.from_decay(g["layer_decay"], g["num_layers"]) if g["layer_decay"] < 1.0 else None
    groups, names = of.get_parameter_groups(m, g["weight_decay"], m.no_weight_decay(), assigner.get_layer_id if assigner else None,
                                            assigner.get_scale if assigner else None, agg_block_scale=g["agg_block_scale"], return_names=True)
    got = [[k, v["weight_decay"], v["lr_scale"], v["params"]] for k, v in names.items()]
    assert got == g["groups"]
    assert sum(len(x["params"]) for x in groups) == 196


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------------
def test_abi_surface_and_struct_layouts(tmp_path):
    from devias_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "devias_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t|void|const char\*)\s+(devias_\w+)\s*\(", hdr, flags=re.M))
    for name in ("devias_fusion_head_workspace_bytes", "devias_fusion_head_save_bytes", "devias_fusion_head_fwd", "devias_fusion_head_bwd", "devias_softmax_ce_fwd",
                 "devias_softmax_ce_bwd", "devias_softmax_ce_workspace_bytes", "devias_region_counter"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.devias_version() >= 175 and _lib.ABI_VERSION >= 175
    ids = {n: int(v) for n, v in re.findall(r"#define DEVIAS_RCNT_(\w+) (\d+)", hdr)}
    assert ids == {"FUSION_HEAD": 0, "SOFTMAX_CE": 1, "MAX": 2} and _lib.REGION_COUNTERS == {"fusion_head": 0, "softmax_ce": 1}
    assert lib.devias_region_counter(2) == -1 and lib.devias_region_counter(-1) == -1
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "devias_amd.h"', 'int main(void) {']
    structs = {"devias_fusion_args": _lib.FusionArgs, "devias_fusion_grads": _lib.FusionGrads}
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
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in body.split(";") for n in re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.split(None, 1)[1] if decl.strip() else "") if n not in ("void", "float", "const")]
        assert [fl[0] for fl in cls._fields_] == fields, (cname, fields)
        for fl in cls._fields_:
            assert got[(cname, fl[0])] == getattr(cls, fl[0]).offset, (cname, fl[0])


def _fargs(p, B=3, S=2, D=384, nb=5, ns=3, Cd=48, dtype=1, use_input_ln=1, **kw):
    from devias_amd import _lib
    a = _lib.FusionArgs()
    a.struct_size = ctypes.sizeof(_lib.FusionArgs)
    a.B, a.S, a.D, a.nb, a.ns, a.Cd, a.dtype, a.use_input_ln = B, S, D, nb, ns, Cd, dtype, use_input_ln
    a.eps_norm, a.eps_ln = 1e-6, 1e-5
    for n in ("Wh", "Wd", "Wc", "bh", "an_w", "an_b", "sn_w", "sn_b", "bd", "ln_w", "ln_b", "in_w", "in_b", "bc", "ws"):
        setattr(a, n, p)
    a.ws_bytes = max(_lib.load().devias_fusion_head_workspace_bytes(B, S, D, nb + ns, Cd, dtype), 0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _fgrads(p, **kw):
    from devias_amd import _lib
    g = _lib.FusionGrads()
    g.struct_size = ctypes.sizeof(_lib.FusionGrads)
    for n, _ in _lib.FusionGrads._fields_[2:]:
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
    ok = _fargs(p)
    assert ok.ws_bytes > 0
    fwd = lambda a, x=p, i=p, o=p, idx=p, save=p: lib.devias_fusion_head_fwd(ctypes.byref(a) if a is not None else None, x, i, o, idx, save, None)      # noqa: E731
    bwd = lambda a, g, x=p, idx=p, i=p, save=p, do=p, ds=p: lib.devias_fusion_head_bwd(ctypes.byref(a) if a is not None else None, x, idx, i, save, do, None, ds,      # noqa: E731
                                                                                         ctypes.byref(g) if g is not None else None, None)
    cases = [("null args", EINVAL, None), ("wrong struct_size", EINVAL, _fargs(p, struct_size=ok.struct_size - 8)), ("bad dtype", EINVAL, _fargs(p, dtype=7)),
             ("S = 5", EUNSUPPORTED, _fargs(p, S=5)), ("Cd = 1", EUNSUPPORTED, _fargs(p, Cd=1)), ("D = 512", EUNSUPPORTED, _fargs(p, D=512)), ("B = 0", EUNSUPPORTED, _fargs(p, B=0)),
             ("null parameter", EINVAL, _fargs(p, Wd=None)), ("use_input_ln without its parameters", EINVAL, _fargs(p, in_w=None)), ("null ws", EINVAL, _fargs(p, ws=None)),
             ("a workspace one byte short", EINVAL, _fargs(p, ws_bytes=ok.ws_bytes - 1)), ("eps = 0", EINVAL, _fargs(p, eps_ln=0.0))]
    for what, code, a in cases:
        assert fwd(a) == code and b"devias_fusion_head_fwd" in lib.devias_last_error(), what
        assert bwd(a, _fgrads(p)) == code and b"devias_fusion_head_bwd" in lib.devias_last_error(), what
    assert fwd(ok, x=None) == EINVAL and fwd(ok, idx=None) == EINVAL and fwd(ok, save=p + 8) == EINVAL
    assert bwd(ok, None) == EINVAL and bwd(ok, _fgrads(p, struct_size=8)) == EINVAL and b"struct_size" in lib.devias_last_error()
    assert bwd(ok, _fgrads(p, dWd=None)) == EINVAL and bwd(ok, _fgrads(p), save=None) == EINVAL and bwd(ok, _fgrads(p), do=None) == EINVAL
    assert bwd(_fargs(p, use_input_ln=0, in_w=None, in_b=None), _fgrads(p, din_w=None, din_b=None), ds=None) == EINVAL          # without the input LN its destinations may be null
    q = lib.devias_fusion_head_workspace_bytes
    assert q(3, 5, 384, 8, 48, 1) == 0 and q(3, 2, 512, 8, 48, 1) == 0 and q(3, 2, 384, 8, 1, 1) == 0 and q(3, 2, 384, 8, 48, 7) == 0
    assert q(12, 4, 768, 765, 200, 1) > q(3, 2, 384, 8, 48, 1) > 0 and lib.devias_fusion_head_save_bytes(12, 768, 1) >= 2 * 12 * 768 * 2 + 12 * 10 * 4
    assert lib.devias_fusion_head_save_bytes(12, 512, 1) == 0
    # cross-entropy
    fw, bw = lib.devias_softmax_ce_fwd, lib.devias_softmax_ce_bwd
    for what, args in (("null logits", (None, p, 5, 48, 0, 0.1)), ("null target", (p, None, 5, 48, 0, 0.1)), ("bad dtype", (p, p, 5, 48, 3, 0.1)), ("C = 1", (p, p, 5, 1, 0, 0.1)),
                       ("B = 0", (p, p, 0, 48, 0, 0.1)), ("smoothing = 1", (p, p, 5, 48, 0, 1.0)), ("smoothing < 0", (p, p, 5, 48, 1, -0.1))):
        assert fw(*args, p, p, None) == EINVAL and b"devias_softmax_ce_fwd" in lib.devias_last_error(), what
        assert bw(*args, p, p, None) == EINVAL and b"devias_softmax_ce_bwd" in lib.devias_last_error(), what
    assert fw(p, p, 5, 48, 0, 0.1, None, p, None) == EINVAL and fw(p, p, 5, 48, 0, 0.1, p, None, None) == EINVAL
    assert bw(p, p, 5, 48, 0, 0.1, None, p, None) == EINVAL and bw(p, p, 5, 48, 0, 0.1, p, None, None) == EINVAL
    assert lib.devias_softmax_ce_workspace_bytes(5) == 20 and lib.devias_softmax_ce_workspace_bytes(0) == 0
    assert lib.devias_region_counter(0) == 0 and lib.devias_region_counter(1) == 0
    assert sum(lib.devias_counter(i) for i in _lib.COUNTERS.values()) == 0


@pytest.mark.timeout(600)
def test_fusion_head_kernels_use_no_scratch():
    """the ISA audit the project runs on its units: every kernel of csrc/fusion_head.hip under the production flags has a zero private segment and no scratch instruction"""
    src = os.path.join(ROOT, "devias_amd", "csrc", "fusion_head.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "fusion_head.s")
        r = subprocess.run([build.HIPCC] + list(build._flags("fusion_head.hip")) + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        isa = open(out).read()
    kernels = re.findall(r"^(_Z\w*(?:fusion_\w+|softmax_ce_\w+)_kernel\w*):", isa, flags=re.M)
    assert len(kernels) == 2 * 2 + 4 * 2 + 2 * 2 + 1, kernels          # gather fwd / bwd x 2 dtypes; middle fwd / bwd x 2 dtypes x input LN or not; CE fwd / bwd x 2; CE final
    segs = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", isa)
    assert len(segs) >= len(kernels) and all(int(s) == 0 for s in segs), segs
    assert not [ln for ln in isa.split("\n") if "scratch_" in ln.split(";")[0]]


# ---- the restatement against the reference's step ---------------------------------------------------------------------------------------------------
def test_downstream_ref_reproduces_the_reference_step():
    fx = dict(np.load(os.path.join(GOLD, "downstream_t8.npz"), allow_pickle=False))
    names = [str(n) for n in fx["param_names"]]
    assert names == [n for n, _ in model().named_parameters()]
    assert sorted(str(n) for n in fx["no_grad_names"]) == sorted(dr.NO_GRAD_NAMES)
    assert float(fx["gaps"].min()) >= 0.05 and fx["idx"].tolist() == [[1, 0], [1, 0]]
    shapes = {n: tuple(p.shape) for n, p in model().named_parameters() if not n.startswith(("blocks.", "patch_embed.", "agg_block.", "norm."))}
    P = {n: v.clone().requires_grad_(True) for n, v in synth.fill_params(shapes, seed=0).items()}
    slots = torch.from_numpy(fx["slots"]).clone().requires_grad_(True)
    y = synth.targets(2, 48, seed=1000)
    o = dr.fusion_forward(slots, P, 400, use_input_ln=True)
    loss = dr.label_smoothing_ce(o["out"], y, float(fx["smoothing"]))
    loss.backward()
    rel = lambda a, b: float((a.double() - torch.as_tensor(b).double()).abs().max() / torch.as_tensor(b).double().abs().max())      # noqa: E731
    assert o["idx"].tolist() == fx["idx"].tolist()
    assert rel(o["input"], fx["input"]) < 1e-5 and rel(o["out"], fx["out"]) < 1e-5 and abs(float(loss) - float(fx["loss"])) < 1e-5 * float(fx["loss"])
    assert rel(slots.grad, fx["dslots"]) < 1e-5
    nmax = float(fx["grad_norms"].max())
    for i, n in enumerate(names):
        if n not in P:
            continue
        if n in dr.NO_GRAD_NAMES:
            assert P[n].grad is None and fx["grad_norms"][i] == 0
            continue
        g = P[n].grad
        assert abs(float(g.double().norm()) - fx["grad_norms"][i]) <= 1e-4 * max(fx["grad_norms"][i], 1e-6 * nmax), n
        from golden_util import sample_idx
        s = g.reshape(-1)[torch.from_numpy(sample_idx(n, g.numel()))].double().numpy()
        assert np.abs(s - fx["grad_samples"][i]).max() <= 1e-4 * max(np.abs(fx["grad_samples"][i]).max(), 1e-6 * nmax), n
