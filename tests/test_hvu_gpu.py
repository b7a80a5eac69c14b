"""The HVU recipe on the device: devias_head_match_loss_labels_fwd/bwd (ground-truth scene labels, no scene teacher) through
devias_amd.hvu_train_loss.TrainLoss, devias_amd.fame.FAMEHVU and devias_amd.engine_for_slot_hvu, against the reference's own outputs
(tests/golden/hvu_loss.npz, vitb_t8_hvu.npz, fame_hvu_t8.npz) and tests/hvu_ref.py at shapes the fixtures do not cover."""
import types
from functools import partial

import numpy as np
import pytest
import torch

import golden_util as gu
import hvu_ref
from devias_amd import synth
from oracle import ref_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda"
NB, NS = 739, 248
LEAVES = ("slots_head", "slots", "maskp", "attn")


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def label_counter():
    from devias_amd import ops
    return ops.counters()["loss_labels"]


def random_case(B, S, nb, ns, dtype, seed=0, D=768, G=196, N=300, nh=4):
    g = torch.Generator().manual_seed(7000 + seed + 13 * B + 101 * S + nb)
    t = dict(slots_head=(torch.randn(B * S, nb + ns, generator=g) * 2).to(dtype), slots=torch.randn(B * S, D, generator=g).to(dtype),
             maskp=torch.sigmoid(torch.randn(B * S, G, generator=g)).to(dtype), attn=torch.softmax(torch.randn(B * nh, S, N, generator=g), dim=1),
             target=torch.randint(0, nb, (B,), generator=g), scene_target=torch.randint(0, ns, (B,), generator=g),
             fg=torch.randint(0, 257, (B, G), generator=g) / 256.0, fgN=torch.randint(0, 257, (B, N), generator=g) / 256.0)
    return {k: v.to(DEV) for k, v in t.items()}


def run_class(t, nb, ns, crit="KL", w_mp=1.0, w_md=1.0, sync=True):
    """forward + backward through the host class; returns (total, logits, loss_dict, grads of the four leaves, match)"""
    from devias_amd.hvu_train_loss import TrainLoss
    lv = {k: t[k].clone().requires_grad_(True) for k in LEAVES}
    c = TrainLoss(None, crit, mask_prediction_loss_weight=w_mp, mask_distill_loss_weight=w_md, num_action_classes=nb, num_scene_classes=ns, sync_loss_dict=sync)
    out = (None, (None, None, lv["attn"]), (lv["slots_head"], lv["slots"], lv["maskp"]))
    total, logits, ld = c(out, t["target"], t["scene_target"], fg_mask=(t["fg"], t["fgN"]))
    total.backward()
    return total.detach(), logits, ld, {k: lv[k].grad for k in LEAVES}, c.last_match


def run_ref(t, nb, crit="KL", w_mp=1.0, w_md=1.0):
    """tests/hvu_ref.py on the values the kernels saw (bf16 inputs widened exactly to fp32)"""
    lv = {k: t[k].float().cpu().clone().requires_grad_(True) for k in LEAVES}
    out = (None, (None, None, lv["attn"]), (lv["slots_head"], lv["slots"], lv["maskp"]))
    total, logits, ld, idx = hvu_ref.hvu_train_loss(out, t["target"].cpu(), t["scene_target"].cpu(), (t["fg"].cpu(), t["fgN"].cpu()), num_action_classes=nb,
                                                    scene_criterion=crit, mask_prediction_loss_weight=w_mp, mask_distill_loss_weight=w_md)
    total.backward()
    return total.detach(), logits.detach(), ld, {k: lv[k].grad for k in LEAVES}, torch.stack(idx, dim=1)


# ------------------------------------------------------------------------------------------------ the loss kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("crit", ["KL", "CE"])
def test_hvu_train_loss_against_reference_golden(dtype, S, crit):
    """the host class over devias_head_match_loss_labels_fwd/bwd against what the reference's hvu_train_loss.TrainLoss returned on the committed inputs
    (tests/golden/hvu_loss.npz).  Tolerances are those of test_train_loss_criteria_against_reference_golden; the fixture's assignment is decisive
    (relative cost gap >= 0.2, asserted by its generator also for bf16-rounded logits), so the match is asserted in BOTH dtypes."""
    fx = dict(np.load(gu.GOLDEN_DIR + "/hvu_loss.npz"))
    t = {k: torch.from_numpy(fx[f"s{S}.{k}"]).to(DEV) for k in LEAVES + ("target", "scene_target", "fg", "fgN")}
    for k in ("slots_head", "slots", "maskp"):
        t[k] = t[k].to(dtype)
    ys_before = t["scene_target"].clone()
    c0 = label_counter()
    total, logits, ld, grads, match = run_class(t, NB, NS, crit, w_mp=1.0, w_md=3.0)
    assert label_counter() - c0 == 2                                       # one forward + one backward, both served by the label kernels
    assert torch.equal(t["scene_target"], ys_before)                       # not offset in place (the reference does: hvu_train_loss.py:45-46)
    pre = f"s{S}.{crit}."
    tol_l, tol_g = (2e-5, 2e-5) if dtype == torch.float32 else (2e-2, 2e-2)
    assert match.cpu().tolist() == fx[pre + "match"].tolist()
    want = fx[pre + "losses"]
    got = [ld[k] for k in hvu_ref.LOSS_NAMES]
    print(f"hvu_loss S={S} {crit} {dtype}: losses {got} want {want.tolist()} total {float(total)} want {float(fx[pre + 'total'])}")
    for g_, w_ in zip(got, want):
        assert abs(g_ - w_) <= tol_l * max(1.0, abs(w_)), (got, want)
    assert abs(float(total) - float(fx[pre + "total"])) <= tol_l * abs(float(fx[pre + "total"]))
    assert rel(logits.float(), torch.from_numpy(fx[f"s{S}.logits"]).to(DEV)) < (1e-6 if dtype == torch.float32 else 1e-2)
    for k in LEAVES:
        e = rel(grads[k].float(), torch.from_numpy(fx[f"s{S}.d{k}"]).to(DEV))
        print(f"  d{k} rel {e:.2e}")
        assert e < tol_g, k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 5, 32])
@pytest.mark.parametrize("nb,ns", [(739, 248), (101, 365), (3, 2)])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_label_loss_against_hvu_ref_other_shapes(dtype, B, nb, ns, S):
    """tests/hvu_ref.py (pinned to the reference by the fixture's generator) on the same rounded values.  S = 1: one slot serves both labels and the
    cosine term is 0.  Bounds: the five terms and the total to 2e-5 (the fp32 bound of the golden test: fp32 statistics in both dtypes, sums of at most 987
    exponentials); the matched logits are copied, so equal; gradients to 1e-4 of their largest element in fp32 and to 1e-2 in bf16, whose
    stored gradients are rounded to 8 significant bits (2^-8 = 3.9e-3 of each element) -- the bounds test_head_match_loss uses for the teacher kernels."""
    t = random_case(B, S, nb, ns, dtype)
    total, logits, ld, grads, match = run_class(t, nb, ns, "CE" if B == 5 else "KL")
    rtotal, rlogits, rld, rgrads, ridx = run_ref(t, nb)
    assert match.cpu().tolist() == ridx.tolist()
    if S == 1:
        assert match.cpu().tolist() == [[0, 0]] * B and ld["cosine_loss"] == 0.0
    got = [ld[k] for k in hvu_ref.LOSS_NAMES] + [float(total)]
    want = [rld[k] for k in hvu_ref.LOSS_NAMES] + [float(rtotal)]
    for g_, w_ in zip(got, want):
        assert abs(g_ - w_) <= 2e-5 * max(1.0, abs(w_)), (got, want)
    assert torch.equal(logits.float().cpu(), rlogits)
    tol = 1e-4 if dtype == torch.float32 else 1e-2
    for k in LEAVES:
        if S == 1 and k == "slots":
            assert float(grads[k].float().abs().max()) == 0.0              # the cosine term is the only path into the slots
            continue
        assert rel(grads[k].float().cpu(), rgrads[k]) < (1e-4 if k == "attn" else tol), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_label_loss_is_bitwise_reproducible(dtype):
    """fixed-order reductions, no atomics: two runs give the same bits in the six losses and all four gradients"""
    t = random_case(5, 3, NB, NS, dtype, seed=1)
    a = run_class(t, NB, NS, sync=False)
    b = run_class(t, NB, NS, sync=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4], b[4])
    assert all(torch.is_tensor(v) and v.dim() == 0 for v in a[2].values())   # sync_loss_dict=False: 0-d device tensors, no host read
    for k in hvu_ref.LOSS_NAMES:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in LEAVES:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S", [2, 3])
def test_label_path_agrees_with_teacher_path_on_the_teachers_argmax(dtype, S):
    """scene_criterion 'CE' of the teacher loss is the cross-entropy against the teacher's argmax (train_loss.py:155-156): with teacher logits whose
    argmax is the label, the two entry points compute the same thing, which ties the label kernels to the kernels the reference goldens of
    test_kernels_gpu.py already pin.  Same match; losses and gradients within the 2e-5 fp32 bound (bf16: the stored gradients are the same fp32 values
    rounded once, so the same bound holds).  Beyond that bound: the LABELS mode of the two kernel templates runs the statements of the scene_ce branch with the
    file's helpers in the same order, so the six losses and all four gradients are bitwise equal as well."""
    from devias_amd import ops
    B, nb, ns = 6, 400, 365
    t = random_case(B, S, nb, ns, dtype, seed=2)
    teacher = torch.randn(B, ns, generator=torch.Generator().manual_seed(9)).to(DEV)
    teacher[torch.arange(B, device=DEV), t["scene_target"]] = 20.0
    args = [t[k] for k in LEAVES]
    losses_l, match_l, logits_l = ops.head_match_loss_labels_fwd(*args, t["target"], t["scene_target"], t["fg"], t["fgN"], nb, 1.0, 3.0, True)
    losses_t, match_t, logits_t = ops.head_match_loss_fwd(*args, teacher, t["target"], t["fg"], t["fgN"], nb, 2000.0, 1.0, 3.0, True)
    assert torch.equal(match_l, match_t) and torch.equal(logits_l, logits_t)
    g = torch.tensor([1.0], device=DEV)
    grads_l = ops.head_match_loss_labels_bwd(*args, t["target"], t["scene_target"], t["fg"], t["fgN"], match_l, g, nb, 1.0, 3.0, True)
    grads_t = ops.head_match_loss_bwd(*args, teacher, t["target"], t["fg"], t["fgN"], match_t, g, nb, 2000.0, 1.0, 3.0, True)
    bitwise = {"losses": torch.equal(losses_l, losses_t)}
    bitwise.update({"d" + k: torch.equal(a, b) for k, a, b in zip(LEAVES, grads_l, grads_t)})
    print(f"label vs teacher path ({dtype}, S={S}): bitwise equal {bitwise}")
    assert all(bitwise.values()), bitwise
    for a, b in zip(losses_l.tolist(), losses_t.tolist()):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (losses_l.tolist(), losses_t.tolist())
    for k, a, b in zip(LEAVES, grads_l, grads_t):
        assert rel(a.float(), b.float()) < 2e-5, k
    # scene_ce = 0 is the same number in the label entry point ('KL' against a one-hot target)
    losses_k, match_k, _ = ops.head_match_loss_labels_fwd(*args, t["target"], t["scene_target"], t["fg"], t["fgN"], nb, 1.0, 3.0, False)
    assert torch.equal(losses_k, losses_l) and torch.equal(match_k, match_l)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which,sample,value", [("target", 0, "nb"), ("scene_target", 0, "ns"), ("scene_target", 1, "neg"), ("target", 1, "neg")])
def test_out_of_range_label_gives_nan_total_and_zero_gradients_for_that_sample_only(dtype, which, sample, value):
    """labels are data: nothing is read through a label outside its range.  The overshooting labels (one past the last class) sit on sample 0 and the
    negative ones on sample 1 of 3, so that even a kernel without the guard would index inside the slots_head allocation."""
    from devias_amd import ops
    B, S, nb, ns = 3, 3, NB, NS
    t = random_case(B, S, nb, ns, dtype, seed=3)
    good = dict(t)
    args = [t[k] for k in LEAVES]
    g = torch.tensor([1.0], device=DEV)
    _, match_g, logits_g = ops.head_match_loss_labels_fwd(*args, good["target"], good["scene_target"], t["fg"], t["fgN"], nb, 1.0, 1.0)
    grads_g = ops.head_match_loss_labels_bwd(*args, good["target"], good["scene_target"], t["fg"], t["fgN"], match_g, g, nb, 1.0, 1.0)
    bad = {k: t[k].clone() for k in ("target", "scene_target")}
    bad[which][sample] = {"nb": nb, "ns": ns, "neg": -1}[value]
    losses, match, logits = ops.head_match_loss_labels_fwd(*args, bad["target"], bad["scene_target"], t["fg"], t["fgN"], nb, 1.0, 1.0)
    assert torch.isnan(losses).all()                                      # every batch mean holds the sample's NaN; so does the total
    assert match[sample].tolist() == [0, 1] and torch.equal(logits[sample], t["slots_head"][sample * S])
    others = [b for b in range(B) if b != sample]
    assert torch.equal(match[others], match_g[others]) and torch.equal(logits[others], logits_g[others])
    grads = ops.head_match_loss_labels_bwd(*args, bad["target"], bad["scene_target"], t["fg"], t["fgN"], match, g, nb, 1.0, 1.0)
    nh = t["attn"].shape[0] // B
    for k, got, want in zip(LEAVES, grads, grads_g):
        per = nh if k == "attn" else S                                     # leading rows per sample
        got, want = got.reshape(B, per, -1), want.reshape(B, per, -1)
        assert float(got[sample].float().abs().max()) == 0.0, k
        assert torch.equal(got[others], want[others]) and float(want[sample].float().abs().max()) > 0, k
    # through the host class: a NaN total for the engine's finite check
    from devias_amd.hvu_train_loss import TrainLoss
    tb = dict(t, **bad)
    total = TrainLoss(None, "KL")((None, (None, None, tb["attn"]), (tb["slots_head"], tb["slots"], tb["maskp"])), tb["target"], tb["scene_target"], fg_mask=(tb["fg"], tb["fgN"]))[0]
    assert torch.isnan(total).all()


# ------------------------------------------------------------------------------------------------ full step
def build(cfg, dtype, init_scale=1e-3):
    from devias_amd.modeling_slot import VisionTransformer
    m = VisionTransformer(patch_size=16, embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads, mlp_ratio=4,
                          qkv_bias=True, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), num_classes=cfg.num_classes,
                          all_frames=cfg.all_frames, tubelet_size=cfg.tubelet_size, init_scale=init_scale,
                          num_latents=cfg.num_latents, head_type=cfg.head_type, slot_matching_method="matching",
                          agg_weights_tie=cfg.agg_weights_tie, agg_depth=cfg.agg_depth,
                          num_scene_classes=cfg.num_scene_classes, compute_dtype=dtype)
    synth.fill_module_(m, seed=0)
    return m.cuda().train()


def hvu_inputs(cfg, B, seed=1000):
    x = synth.video(B, cfg.all_frames, cfg.img_size, seed=seed)
    y = synth.targets(B, cfg.num_classes, seed=seed)
    ys = synth.scene_targets(B, cfg.num_scene_classes, seed=seed)
    fg = synth.fg_masks(B, cfg.num_patches, cfg.grid * cfg.grid, seed=seed)
    return x, y, ys, fg


def run_step(model, cfg, B):
    from devias_amd.engine_for_slot_hvu import train_class_batch
    from devias_amd.hvu_train_loss import TrainLoss
    x, y, ys, fg = hvu_inputs(cfg, B)
    crit = TrainLoss(criterion=None, scene_criterion="KL", slot_matching_method="matching", mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0,
                     num_action_classes=cfg.num_classes, num_scene_classes=cfg.num_scene_classes)
    seen = {}
    h = model.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o))
    model.zero_grad()
    c0 = label_counter()
    total, logits, ld = train_class_batch(model, x.cuda(), y.cuda(), ys.cuda(), crit, fg_mask=(fg[0].cuda(), fg[1].cuda()))
    total.backward()
    h.remove()
    assert label_counter() - c0 == 2
    grads = {n: p.grad for n, p in model.named_parameters()}
    assert all(g is not None for g in grads.values())
    return seen["out"], total, logits, ld, grads, crit.last_match


def test_fp32_hvu_step_matches_reference_golden():
    """create_model-equivalent student with num_classes=739, num_scene_classes=248 (head width 987 through the same generic kernels as 765 and 466) under the
    HVU loss, against the reference's own step (tests/golden/vitb_t8_hvu.npz): TOL_FP32 = 1e-3 on outputs and loss, 5e-3 on every gradient, as
    test_fp32_step_matches_reference_golden"""
    fx, cfg, B = gu.load("vitb_t8_hvu")
    assert (cfg.num_classes, cfg.num_scene_classes) == (NB, NS)
    model = build(cfg, "fp32")
    assert tuple(model.head.weight.shape) == (NB + NS, 768)
    out, total, logits, ld, grads, match = run_step(model, cfg, B)
    idx = (match[:, 0].cpu().tolist(), match[:, 1].cpu().tolist())
    errs, gerrs = gu.check_against_golden(fx, out, float(total.detach()), logits, ld, grads, tol_out=1e-3, tol_grad=5e-3, idx=idx)
    print("vitb_t8_hvu fp32: max output err", max(errs.values()), "max grad err", max(gerrs.values()))


def test_bf16_hvu_step_close_to_reference():
    """the bounds of test_bf16_step_close_to_reference"""
    fx, cfg, B = gu.load("vitb_t8_hvu")
    model = build(cfg, "bf16")
    out, total, logits, ld, grads, match = run_step(model, cfg, B)
    e_logit = gu.rel(out[2][0].detach().float().cpu(), fx["slots_head"])
    e_total = abs(float(total) - float(fx["total_loss"])) / abs(float(fx["total_loss"]))
    names = [str(n) for n in fx["param_names"]]
    gn = np.array([float(grads[n].double().norm()) for n in names])
    e_gn = np.abs(gn - fx["grad_norms"]) / np.maximum(fx["grad_norms"], 1e-6 * fx["grad_norms"].max())
    print(f"vitb_t8_hvu bf16: logits rel {e_logit:.3e}, total loss rel {e_total:.3e}, grad-norm rel median {np.median(e_gn):.3e} max {e_gn.max():.3e}")
    assert e_logit < 5e-2 and e_total < 2e-2 and np.median(e_gn) < 5e-2
    assert torch.isfinite(total).all()


def test_create_model_with_hvu_class_counts():
    import devias_amd
    m = devias_amd.create_model("slot_vit_base_patch16_224", num_classes=NB, num_scene_classes=NS, all_frames=8, num_latents=2, slot_matching="matching",
                                agg_weights_tie=True, agg_depth=8)
    assert tuple(m.head.weight.shape) == (NB + NS, 768) and (m.num_classes, m.num_scene_classes) == (NB, NS)


# ------------------------------------------------------------------------------------------------ FAME
def test_fame_hvu_matches_reference_golden():
    """devias_amd.fame.FAMEHVU against the reference's fame_hvu.FAME (tests/golden/fame_hvu_t8.npz): labels exactly, masks to the tolerance of
    test_fame_matches_reference_golden (the fixture's masks are fame_t8.npz's bit for bit), clips and masks bitwise those of FAME.forward on the same draws"""
    from devias_amd.fame import FAME, FAMEHVU
    fx = dict(np.load(gu.GOLDEN_DIR + "/fame_hvu_t8.npz"))
    base = dict(np.load(gu.GOLDEN_DIR + "/fame_t8.npz"))
    assert np.array_equal(fx["mask"], base["mask"]) and np.array_equal(fx["masks_per_frame"], base["masks_per_frame"])
    B, T, size = int(fx["B"]), int(fx["T"]), int(fx["size"])
    x = synth.scene_video(B, T, size).cuda()
    f = FAMEHVU(beta=float(fx["beta"]), prob_aug=float(fx["prob_aug"]))
    assert "FAME" in str(f)
    a, s = torch.from_numpy(fx["action_label"]).cuda(), torch.from_numpy(fx["scene_label"]).cuda()
    a0, s0 = a.clone(), s.clone()
    perm, rand = torch.from_numpy(fx["perm"]), torch.from_numpy(fx["rand"])
    vids, a_out, s_out, (m, mpf) = f(x, a, s, index=perm, rand_batch=rand)
    assert a_out.is_cuda and s_out.is_cuda and torch.equal(a, a0) and torch.equal(s, s0)
    assert np.array_equal(a_out.cpu().numpy(), fx["out_action_label"]) and np.array_equal(s_out.cpu().numpy(), fx["out_scene_label"])
    assert m.shape == fx["mask"].shape and mpf.shape == fx["masks_per_frame"].shape
    for got, want in ((m.cpu().numpy(), fx["mask"]), (mpf.cpu().numpy(), fx["masks_per_frame"])):
        d = np.abs(got - want)
        assert float(d.max()) <= 6 / 256 + 1e-7 and float(d.mean()) < 2e-4, (float(d.max()), float(d.mean()))
    v2, lab2, (m2, mpf2) = FAME(beta=float(fx["beta"]), prob_aug=float(fx["prob_aug"]))(x, a, index=perm, rand_batch=rand)
    assert torch.equal(vids, v2) and torch.equal(a_out, lab2) and torch.equal(m, m2) and torch.equal(mpf, mpf2)


# ------------------------------------------------------------------------------------------------ engine
def small_model(dtype, nb=NB, ns=NS, frames=4):
    import devias_amd
    model = devias_amd.create_model("slot_vit_small_patch16_224", num_classes=nb, all_frames=frames, num_latents=2, slot_matching_method="matching",
                                    agg_weights_tie=True, agg_depth=2, num_scene_classes=ns, compute_dtype=dtype)
    synth.fill_module_(model, seed=0)
    return model.cuda().train()


def test_short_hvu_training_run_decreases_the_loss():
    """the model, optimizer, schedule and 12 steps of test_short_training_run_decreases_the_loss (layer-decay groups, cosine LR with warm-up, clipped fused
    AdamW, bf16, a fixed batch of 4 clips) driven through engine_for_slot_hvu.train_class_batch with 739 + 248 classes: the loss stays finite and the last step
    is below the first, and it falls at every step after the lr = 0 warm-up step within that test's 1e-3 slack.  (That test's 'falls by 0.3' margin belongs
    to the KL x 4000 teacher term and does not carry over.)"""
    from devias_amd import optim_factory as of
    from devias_amd.engine_for_slot_hvu import train_class_batch
    from devias_amd.hvu_train_loss import TrainLoss
    model = small_model("bf16")
    B = 4
    x = synth.scene_video(B, 4, 224).cuda()
    y, ys = synth.targets(B, NB).cuda(), synth.scene_targets(B, NS).cuda()
    y0, ys0 = y.clone(), ys.clone()
    fg = tuple(m.cuda() for m in synth.fg_masks(B, model.patch_embed.num_patches))
    crit = TrainLoss(None, "KL", slot_matching_method="matching", mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0)
    assigner = of.LayerDecayValueAssigner.from_decay(0.75, model.get_num_layers())
    args = types.SimpleNamespace(opt="adamw", lr=2e-3, weight_decay=0.05, opt_eps=1e-8, opt_betas=[0.9, 0.999])
    opt = of.create_optimizer(args, model, get_num_layer=assigner.get_layer_id, get_layer_scale=assigner.get_scale)
    sched = of.cosine_scheduler(2e-3, 1e-5, epochs=1, niter_per_ep=12, warmup_epochs=1, warmup_steps=2)
    losses = []
    c0 = label_counter()
    for it in range(12):
        for g in opt.param_groups:
            g["lr"] = sched[it] * g["lr_scale"]
        opt.zero_grad(set_to_none=True)
        loss, out, ld = train_class_batch(model, x, y, ys, crit, fg_mask=fg)
        loss.backward()
        opt.step(max_norm=5.0)
        losses.append(float(loss.detach().float().sum()))
        assert np.isfinite(losses[-1]) and float(opt.last_grad_norm) > 0
    print("hvu short run losses", losses, "falls at every step (1e-3 slack):", all(b <= a + 1e-3 for a, b in zip(losses[1:], losses[2:])))
    assert label_counter() - c0 == 24 and torch.equal(y, y0) and torch.equal(ys, ys0)
    assert losses[-1] < losses[0] and all(b <= a + 1e-3 for a, b in zip(losses[1:], losses[2:])), losses


class _RecordingSGD(torch.optim.SGD):
    """lr = 0: step() only records the accumulated gradients train_one_epoch hands it"""

    def step(self, closure=None):
        self.seen = [p.grad.detach().clone() for g in self.param_groups for p in g["params"]]
        self.steps = getattr(self, "steps", 0) + 1


def test_update_freq_two_accumulates_the_full_batch_gradient():
    """train_one_epoch with update_freq = 2 over two half batches against update_freq = 1 over the full batch (fp32 compute, masks given, no FAME).  The HVU
    loss has no cross-sample term (no batch minimum of teacher logits), so the two are equal up to summation order.  Bound: the 5e-3 gradient tolerance of the
    fp32 parity tests, each parameter's error scaled by max(its largest reference element, 1e-6 of the global largest) as golden_util.check_against_golden does."""
    from devias_amd.engine_for_slot_hvu import train_one_epoch
    from devias_amd.hvu_train_loss import TrainLoss
    cfg = ref_cpu.SlotViTConfig(embed_dim=384, num_heads=6, depth=2, all_frames=4, num_classes=NB, num_scene_classes=NS, num_latents=2, agg_depth=2)
    model = build(cfg, "fp32", init_scale=1.0)
    B = 4
    x, y, ys, fg = hvu_inputs(cfg, B)
    y0, ys0 = y.clone(), ys.clone()
    crit = TrainLoss(None, "KL", num_action_classes=NB, num_scene_classes=NS)
    params = [p for p in model.parameters()]

    def run(loader, update_freq):
        opt = _RecordingSGD(params, lr=0.0)
        train_one_epoch(model, crit, loader, opt, "cuda", 0, update_freq=update_freq, check_finite_every=1)
        assert opt.steps == 1
        return opt.seen, crit.last_match.clone()

    full, match_full = run([(x, y, ys, fg)], 1)
    h = B // 2
    halves = [(x[i:i + h], y[i:i + h], ys[i:i + h], (fg[0][i:i + h], fg[1][i:i + h])) for i in (0, h)]
    acc, match_last = run(halves, 2)
    assert torch.equal(match_last, match_full[h:])
    assert torch.equal(y, y0) and torch.equal(ys, ys0)                     # the caller's targets are not written
    gmax = max(float(g.abs().max()) for g in full)
    worst = max(float((a.double() - f.double()).abs().max() / max(float(f.abs().max()), 1e-6 * gmax)) for a, f in zip(acc, full))
    print("update_freq=2 vs full batch: worst scaled gradient error", worst)
    assert gmax > 0 and worst <= 5e-3, worst


def test_validation_loops_agree_with_plain_torch_topk():
    """validation_one_epoch / validation_action / validation_scene (engine_for_slot_hvu.py:156-280) against top-k and cross-entropy computed in plain torch on
    the model's own eval outputs: scene accuracy on the scene-selected slot's full [B, nb + ns] logits against scene_target + nb; the loss is the
    action cross-entropy in all three.  The loader's target tensors are not written."""
    from devias_amd.engine_for_slot_hvu import validation_action, validation_one_epoch, validation_scene
    nb, ns = 24, 16                                                        # few classes: top-5 hits and misses both occur
    model = small_model("fp32", nb, ns).eval()
    batches = []
    for i, B in enumerate((3, 2)):
        x = synth.video(B, 4, 224, seed=1000, first=3 * i)
        batches.append((x, synth.targets(B, nb, first=3 * i), synth.scene_targets(B, ns, first=3 * i)))
    keep = [(b[1].clone(), b[2].clone()) for b in batches]
    n = ce = 0.0
    hits = {"action_acc1": 0.0, "action_acc5": 0.0, "scene_acc1": 0.0, "scene_acc5": 0.0}
    with torch.no_grad():
        for x, y, ys in batches:
            _, (ao, so, _), _ = model(x.cuda())
            ao, so = ao.float().cpu(), so.float().cpu()
            assert ao.shape == so.shape == (x.shape[0], nb + ns)
            n += x.shape[0]
            ce += float(torch.nn.functional.cross_entropy(ao, y, reduction="sum"))
            for name, o, tgt in (("action", ao, y), ("scene", so, ys + nb)):
                top = o.topk(5, dim=1).indices
                hits[name + "_acc1"] += float((top[:, :1] == tgt[:, None]).any(1).sum())
                hits[name + "_acc5"] += float((top == tgt[:, None]).any(1).sum())
    want = {k: 100.0 * v / n for k, v in hits.items()}
    st = validation_one_epoch(batches, model, "cuda")
    assert set(st) == {"loss", "action_acc1", "action_acc5", "scene_acc1", "scene_acc5"}
    assert abs(st["loss"] - ce / n) < 1e-4 * abs(ce / n) and all(abs(st[k] - want[k]) < 1e-9 for k in want), (st, want)
    sa, ss = validation_action(batches, model, "cuda"), validation_scene(batches, model, "cuda")
    assert set(sa) == {"loss", "action_acc1", "action_acc5"} and set(ss) == {"loss", "scene_acc1", "scene_acc5"}
    assert all(sa[k] == st[k] for k in sa) and all(ss[k] == st[k] for k in ss)
    assert all(torch.equal(b[1], k[0]) and torch.equal(b[2], k[1]) for b, k in zip(batches, keep))


def test_engine_step_with_fame_hvu():
    """train_one_epoch with mask_model=FAMEHVU (engine_for_slot_hvu.py:64-65): steps run through the fused optimizer and yield a finite loss"""
    from devias_amd.engine_for_slot_hvu import train_one_epoch
    from devias_amd.fame import FAMEHVU
    from devias_amd.hvu_train_loss import TrainLoss
    from devias_amd.optim import FusedAdamW
    model = small_model("bf16")
    B = 4
    x = synth.scene_video(B, 4, 224)
    y, ys = synth.targets(B, NB), synth.scene_targets(B, NS)
    opt = FusedAdamW(model.parameters(), lr=1e-4)
    c0 = label_counter()
    st = train_one_epoch(model, TrainLoss(None, "CE"), [(x, y, ys, None, None)] * 2, opt, "cuda", 0, max_norm=5.0, mask_model=FAMEHVU(beta=0.5, prob_aug=0.5),
                         check_finite_every=1)
    assert label_counter() - c0 == 4
    assert np.isfinite(st["loss"]) and st["grad_norm"] > 0 and set(hvu_ref.LOSS_NAMES) <= set(st)
