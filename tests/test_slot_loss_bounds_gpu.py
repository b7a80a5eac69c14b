"""The accuracy anchor of the slot cross-attention kernels and the matching loss (GPU only): the three slot-attention kernel families, the two deferred
gradients and both loss entry-point pairs against float64 on graded inputs, each element held to the bound of tests/slot_loss_bounds.py
(worst |out - ref| / bound <= 1).  The float64 slot-attention references run in torch on the device and the loss reference is the CPU oracle: none of this
project's kernels.  Every call goes through served(), which asserts by launch counter which family ran (DEVIAS_CNT_SLOTM / _SLOTF_VALU / _SLOT, and
DEVIAS_CNT_LOSS_LABELS for the loss).  Backward references are taken on the saved attn / rsum / o the kernels themselves produced, so each entry point is bounded
on its own.  attn, rsum and ds destinations are prefilled with NaN: an element a kernel does not write is infinitely wrong.
Each case prints `[bound] <kernel> <shape> <variant> worst ratio ...`."""
import os

import pytest
import torch

import kernel_bounds as kb
import slot_loss_bounds as sb

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif("DEVIAS_SLOT_MFMA" in os.environ, reason="DEVIAS_SLOT_MFMA is set: it is read once per process and moves calls between the kernel families asserted here")]

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SCALE = sb.SLOT_SCALE


def ops():
    from devias_amd import ops as o
    return o


def say(kernel, shape, variant, ratios):
    print(f"[bound] {kernel} {shape} {variant} worst ratio " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def served(o, fn, **want):
    """run fn() with fresh counters; assert the slot-attention family counters (those not named must be 0), return the result"""
    o.counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    cnt = o.counters()
    for k in ("slotm", "slotf_valu", "slot", "loss_labels"):
        assert cnt[k] == want.get(k, 0), (k, want, {n: cnt[n] for n in ("slotm", "slotf_valu", "slot", "loss_labels")})
    return out


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def worst(into, ratios):
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)


def slot_layer(o, kind, B, S, N, h, D, dtype, folded, family, ext_on, seed):
    """one forward and one backward call of a family on one generator; returns the worst ratios"""
    mfma = family == "slotm"
    q, src, d_o, ext = sb.slot_inputs(kind, B, S, N, h, D, dtype, folded, seed=seed, device=DEV)
    ext = ext if ext_on else None
    tag = f"{family} {dtype} {kind} B={B} S={S} N={N} h={h} D={D} ext={int(ext_on)}"
    if folded:
        attn, rsum, out = served(o, lambda: o.slotf_fwd(q, src, B, S, N, h, D, SCALE, attn_out=nan(B * h, S, N), rsum_out=nan(B * h, S)), **{family: 1})
    else:
        attn, rsum, out = served(o, lambda: o.slot_attn_fwd(q, src, B, S, N, h, D, SCALE, attn_out=nan(B * h, S, N), rsum_out=nan(B * h, S)), **{family: 1})
    ref = sb.slot_fwd_ref(q, src, B, S, N, h, SCALE, dtype, folded, mfma)
    r = {k: kb.check(f"{tag} fwd {k}", t, *ref[k]) for k, t in (("attn", attn), ("rsum", rsum), ("out", out))}
    if folded:
        dq, ds = served(o, lambda: o.slotf_bwd(src, attn, rsum, out, d_o, ext, B, S, N, h, D, SCALE, ds_out=nan(B * h, S, N)), **{family: 1})
    else:
        dq, ds = served(o, lambda: o.slot_attn_bwd(q, src, attn, rsum, out, d_o, ext, B, S, N, h, D, SCALE, ds_out=nan(B * h, S, N)), **{family: 1})
    refb = sb.slot_bwd_ref(src, attn, rsum, out, d_o, ext, B, S, N, h, SCALE, dtype, folded, mfma)
    r.update({k: kb.check(f"{tag} bwd {k}", t, *refb[k]) for k, t in (("dq", dq), ("ds", ds))})
    return r


def slot_sweep(family, folded, dtype, B, S, h, D, Ns):
    o = ops()
    for kind in sb.SLOT_GENERATORS:
        ratios = {}
        for n_i, N in enumerate(Ns):
            for ext_on in (True, False):
                worst(ratios, slot_layer(o, kind, B, S, N, h, D, dtype, folded, family, ext_on, seed=20 + n_i))
        say(family, f"B={B} S={S} h={h} D={D} N={list(Ns)}", f"{dtype} {kind}", ratios)


# ------------------------------------------------------------------------------------------------ the matrix-core folded kernel: every bf16 call of the measured step
@pytest.mark.parametrize("D", [512, 768, 1024])
@pytest.mark.parametrize("S,h", [(1, 4), (2, 1), (2, 4), (4, 2), (4, 4)])
def test_slotm(S, h, D):
    """N: fewer tokens than a 32-token tile, one token into the second tile, exactly one workgroup of 128, one token into the second workgroup, three workgroups ragged"""
    slot_sweep("slotm", True, BF, 2, S, h, D, (7, 33, 128, 129, 300))


# ------------------------------------------------------------------------------------------------ the folded VALU kernels
@pytest.mark.parametrize("dtype,S,h,D", [(BF, 3, 2, 768), (F32, 3, 2, 768), (BF, 2, 2, 384), (F32, 2, 2, 384), (BF, 4, 4, 384), (F32, 4, 4, 384), (F32, 4, 4, 768),
                                         (BF, 3, 1, 1024), (F32, 1, 4, 512)])
def test_slotf_valu(dtype, S, h, D):
    """bf16 reaches these kernels only through S = 3 or D = 384; fp32 always (also at a shape the matrix-core kernel serves in bf16).  N: one ragged 64-token
    chunk, one token into the second, one into the third"""
    slot_sweep("slotf_valu", True, dtype, 2, S, h, D, (7, 65, 129))


# ------------------------------------------------------------------------------------------------ the unfolded kernels
@pytest.mark.parametrize("h", [1, 4])
@pytest.mark.parametrize("S", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_slot_unfolded(dtype, S, h):
    """S covers the three register forms (MAXS 2, 4, 8: slot_unfolded.hip:318-319).  N: a ragged chunk, exactly one 64-token chunk, one token into the second, two into the third"""
    slot_sweep("slot", False, dtype, 2, S, h, 512, (7, 64, 65, 130))


@pytest.mark.parametrize("L,S", [(4, 4), (17, 1), (4, 5)])                  # L S = 16: one group; 17: one pair into the second; 20: the 5-slot model at depth 4
@pytest.mark.parametrize("dtype", [F32, BF])
def test_slot_kv_grad_stacked(dtype, L, S):
    o = ops()
    B, N, h, D = 2, 70, 2, 512
    t = sb.stacked_inputs(L, B, S, N, h, D, dtype, seed=30, device=DEV)
    dkv = served(o, lambda: o.slot_attn_kv_grad(*t, L, B, S, N, h, D, SCALE), slot=1)
    ref, bound = sb.slot_kv_grad_ref(*t, L, B, S, N, h, SCALE, dtype)
    ratios = {"dkv": kb.check(f"kv_grad {dtype} L={L} S={S}", dkv, ref, bound, lambda i: kb.where2d(i, 2 * h * D))}
    if dtype == BF and L * S > sb.KVG_PAIRS:
        ratios["dkv_without_the_inter_group_term"] = kb.excess(dkv, ref, sb.slot_kv_grad_ref(*t, L, B, S, N, h, SCALE, dtype, inter_group=False)[1])[0]
    say("slot_kv_grad", f"L={L} B={B} S={S} N={N} h={h}", f"{dtype}", ratios)


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("dtype,S,h,D", [(BF, 4, 4, 768), (F32, 4, 4, 768), (BF, 3, 2, 384), (F32, 2, 1, 1024)])
def test_slotf_context_grad(dtype, S, h, D, L):
    """devias_slotf_pack + the batched GEMM; N % 8 != 0 (padded coefficient rows)"""
    o = ops()
    B, N = 2, 67
    qs, dzs, ds, A, r = sb.stacked_inputs(L, B, S, N, h, D, dtype, seed=31, device=DEV)
    dc = served(o, lambda: o.slotf_context_grad(A, r, ds, dzs, qs, L, B, S, N, h, D, SCALE))
    ref, bound = sb.slotf_context_grad_ref(A, r, ds, dzs, qs, L, B, S, N, h, D, SCALE, dtype)
    say("slotf_context_grad", f"L={L} B={B} S={S} N={N} h={h} D={D}", f"{dtype}", {"dc": kb.check(f"context_grad {dtype} L={L}", dc, ref, bound, lambda i: kb.where2d(i, D))})


# ------------------------------------------------------------------------------------------------ the matching loss
@pytest.mark.parametrize("crit", ["KL", "CE"])
@pytest.mark.parametrize("labels", [False, True])
@pytest.mark.parametrize("nb", [400, 101])
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_head_match_loss_bounds(dtype, B, S, nb, labels, crit):
    o = ops()
    t = sb.loss_inputs(B, S, nb, dtype, seed=40, device=DEV, labels=labels)
    margin = sb.match_margin(t, nb, labels)
    assert margin >= sb.MATCH_MARGIN, margin
    ref = sb.loss_ref(t, nb, dtype, crit, labels)
    ce = crit == "CE"
    if labels:
        args = (t["Z"], t["slots"], t["maskp"], t["attn"], t["target"], t["scene_target"], t["fg"], t["fgN"])
        losses, match, logits = served(o, lambda: o.head_match_loss_labels_fwd(*args, nb, 1.0, 1.0, scene_ce=ce), loss_labels=1)
        grads = served(o, lambda: o.head_match_loss_labels_bwd(*args, match, t["g_total"], nb, 1.0, 1.0, scene_ce=ce), loss_labels=1)
    else:
        args = (t["Z"], t["slots"], t["maskp"], t["attn"], t["teacher"], t["target"], t["fg"], t["fgN"])
        losses, match, logits = served(o, lambda: o.head_match_loss_fwd(*args, nb, 4000.0, 1.0, 1.0, scene_ce=ce))
        grads = served(o, lambda: o.head_match_loss_bwd(*args, match, t["g_total"], nb, 4000.0, 1.0, 1.0, scene_ce=ce))
    assert torch.equal(match.cpu(), ref["match"]), (match.cpu(), ref["match"])
    assert torch.equal(logits.cpu().double(), ref["logits"])
    got = dict(zip(("dZ", "d_slots", "d_maskp", "d_attn"), grads), losses=losses)
    tag = f"loss {dtype} B={B} S={S} nb={nb} {crit}{' labels' if labels else ''}"
    say("head_match_loss", f"B={B} S={S} nb={nb}", f"{dtype} {crit}{' labels' if labels else ''} margin {margin:.2f}",
        {k: kb.check(f"{tag} {k}", got[k].cpu(), *ref[k]) for k in sb.LOSS_OUTPUTS})
