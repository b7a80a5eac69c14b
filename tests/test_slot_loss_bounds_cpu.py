"""The bounds of tests/slot_loss_bounds.py proved without a GPU, as test_kernel_bounds_cpu.py proves kernel_bounds.py: for the three slot-attention kernel
families, the two deferred gradients and the matching loss, the CPU emulation of the documented algorithm (the float64 reference plus exactly the named
roundings, bf16 packs included; torch CPU fp32 arithmetic) stays inside the bound on every generator -- <= 0.5 under the slack-bearing bounds, <= 1 under the
factor-1 bounds of the deferred gradients -- and every seeded mutant exceeds 1 on the generators named for it.  A mutant that a generator cannot expose under
an honest bound is REPORTED there with its ratio (FWD_MUTANTS / BWD_MUTANTS say where each is asserted and why not elsewhere)."""
import pytest
import torch

import kernel_bounds as kb
import slot_loss_bounds as sb

BF, F32 = torch.bfloat16, torch.float32
SCALE = sb.SLOT_SCALE
FAMILIES = {"unfolded": (False, False), "valu": (True, False), "mfma": (True, True)}       # (folded, served by slotm_kernel)


def report(name, r):
    print(f"[bound-cpu] {name} worst ratio {r:.3f}")
    return r


# ------------------------------------------------------------------------------------------------ slot attention: the emulations
def slot_fwd_emul(q, src, B, S, N, h, scale, dtype, folded, mfma, mutant=None):
    """fp32 scores, slot softmax and sums; rsum of the fp32 A plus 1e-7; one rounding of o / z; slotm: A packed to bf16 for the Z product only"""
    q4, k4, v4 = (t.float() for t in sb.slot_views(q, src, B, S, N, h, folded))
    a = (scale * (q4 @ k4.transpose(-1, -2))).softmax(2)
    if mutant == "A_bf16":
        a = a.to(BF).float()
    az = a.to(BF).float() if mfma else a.clone()
    ar = a.clone()
    if mutant == "tail_token_not_in_z":
        az[..., N - 1] = 0
    if mutant == "tail_token_not_in_rsum":
        ar[..., N - 1] = 0
    rsum = ar.sum(-1) + (0.0 if mutant == "no_eps" else torch.tensor(1e-7))
    rz = rsum.roll(1, 1) if mutant == "neighbour_head_rsum" else rsum
    o = (az @ v4) / rz[..., None]
    return a.reshape(B * h, S, N), rsum.reshape(B * h, S), sb.slot_rows(o).to(dtype)


def slot_bwd_emul(src, attn, rsum, o, d_o, ext, B, S, N, h, scale, dtype, folded, mfma, mutant=None, o_unrounded=None):
    """delta from the STORED o, fp32 throughout, ds stored unrounded, one rounding of dq; slotm: scale dS packed to bf16 for the dQ' product"""
    dO, k4, v4 = (t.float() for t in sb.slot_views(d_o, src, B, S, N, h, folded))
    o4 = sb.slot_heads(o_unrounded if mutant == "delta_from_unrounded_o" else o, B, S, h).float()
    a, rinv = attn.reshape(B, h, S, N), 1.0 / rsum.reshape(B, h, S, 1)
    e = ext.reshape(B, h, S, N) if ext is not None else torch.zeros_like(a)
    if mutant == "rinv_of_wrong_slot":
        rinv = rinv.roll(1, 2)
    delta = (dO * o4).sum(-1, keepdim=True)
    dAbar = dO @ v4.transpose(-1, -2)
    dA = (dAbar - delta + e) * rinv if mutant == "ext_scaled_by_rinv" else (dAbar - delta) * rinv + e
    ds = a * (dA - (a * dA).sum(2, keepdim=True))
    if mutant == "ds_bf16":
        ds = ds.to(BF).float()
    w = ds * scale
    if mfma:
        w = w.to(BF).float()
    return sb.slot_rows(w @ k4).to(dtype), ds.reshape(B * h, S, N)


def kv_grad_emul(qs, dos, ds, A, r, L, B, S, N, h, scale, dtype, mutant=None):
    """fp32 sums in groups of 16 (layer, slot) pairs; the running value goes through the output dtype between groups"""
    cab = A / r[..., None]
    outs = []
    for coef, vec in ((scale * sb._pair_coefs(ds, L, B, S, N, h).float(), sb._pairs(qs, L, B, S, h).float()), (sb._pair_coefs(cab, L, B, S, N, h).float(), sb._pairs(dos, L, B, S, h).float())):
        acc = torch.zeros(B, h, N, vec.shape[-1])
        for g, p0 in enumerate(range(0, L * S, sb.KVG_PAIRS)):
            part = coef[:, :, p0:p0 + sb.KVG_PAIRS].transpose(-1, -2) @ vec[:, :, p0:p0 + sb.KVG_PAIRS]
            if g == 1 and mutant == "group2_dropped":
                part = torch.zeros_like(part)
            acc = part if (g == 1 and mutant == "group2_overwrites") else acc + part
            acc = acc.to(dtype).float()
        outs.append(acc)
    return torch.stack(outs, dim=2).permute(0, 3, 2, 1, 4).reshape(B * N, -1).to(dtype)


def context_grad_emul(A, r, ds, dzs, qps, L, B, S, N, h, D, scale, dtype, mutant=None):
    """devias_slotf_pack's rounding of the coefficients to the operand dtype, an fp32 GEMM, one rounding"""
    cab = A if mutant == "pack_without_rinv" else A / r[..., None]
    dc = torch.zeros(B, N, D)
    for coef, vec in ((cab, dzs), (scale * ds, qps)):
        dc = dc + torch.einsum("lbhsn,lbshd->bnd", coef.to(dtype).float().reshape(L, B, h, S, N), vec.float().reshape(L, B, S, h, D))
    return dc.reshape(B * N, D).to(dtype)


SB, SS, SH, SD = 2, 4, 2, 512


def slot_case(kind, family, dtype, N, seed=3):
    folded, mfma = FAMILIES[family]
    q, src, d_o, ext = sb.slot_inputs(kind, SB, SS, N, SH, SD, dtype, folded, seed=seed)
    return folded, mfma, q, src, d_o, ext


def fwd_ratios(kind, family, dtype, N, mutant=None):
    folded, mfma, q, src, d_o, ext = slot_case(kind, family, dtype, N)
    ref = sb.slot_fwd_ref(q, src, SB, SS, N, SH, SCALE, dtype, folded, mfma)
    out = dict(zip(("attn", "rsum", "out"), slot_fwd_emul(q, src, SB, SS, N, SH, SCALE, dtype, folded, mfma, mutant)))
    return {k: kb.excess(out[k], *ref[k])[0] for k in out}


def bwd_ratios(kind, family, dtype, N, mutant=None):
    folded, mfma, q, src, d_o, ext = slot_case(kind, family, dtype, N)
    fwd = sb.slot_fwd_ref(q, src, SB, SS, N, SH, SCALE, dtype, folded, mfma)
    attn, rsum, o = slot_fwd_emul(q, src, SB, SS, N, SH, SCALE, dtype, folded, mfma)          # the saved tensors a backward call is given
    ref = sb.slot_bwd_ref(src, attn, rsum, o, d_o, ext, SB, SS, N, SH, SCALE, dtype, folded, mfma)
    out = dict(zip(("dq", "ds"), slot_bwd_emul(src, attn, rsum, o, d_o, ext, SB, SS, N, SH, SCALE, dtype, folded, mfma, mutant, o_unrounded=fwd["out"][0])))
    return {k: kb.excess(out[k], *ref[k])[0] for k in out}


@pytest.mark.parametrize("kind", sb.SLOT_GENERATORS)
@pytest.mark.parametrize("family,dtype", [("unfolded", F32), ("unfolded", BF), ("valu", F32), ("valu", BF), ("mfma", BF)])
def test_slot_attention_emulation_inside_the_bounds(family, dtype, kind):
    for N in (33, 129):
        for name, rs in (("fwd", fwd_ratios(kind, family, dtype, N)), ("bwd", bwd_ratios(kind, family, dtype, N))):
            for k, r in rs.items():
                report(f"slot {family} {dtype} {kind} N={N} {name} {k}", r)
                assert r <= 0.5, (family, dtype, kind, N, name, k, r)


def test_starved_generator_starves_a_slot():
    """the generator's claim: the last slot's rsum is of the order of the 1e-7 guard, the others' of the order of N / (S - 1)"""
    for family, (folded, _) in FAMILIES.items():
        q, src, _, _ = sb.slot_inputs("starved", SB, SS, 129, SH, SD, BF, folded, seed=3)
        rsum = sb.slot_fwd_ref(q, src, SB, SS, 129, SH, SCALE, BF, folded)["rsum"][0].reshape(SB, SH, SS)
        assert float(rsum[..., -1].max()) < 2e-6 and float(rsum[..., -1].min()) > 1e-7, (family, rsum[..., -1])
        assert float(rsum[..., :-1].min()) > 10.0, (family, rsum)


# Where each mutant must exceed 1; on the other generators it is reported with its ratio.  Why a generator is left out:
#   no_eps                  1e-7 is 1e-9 of an rsum ~ N / S: below the fp32 resolution of every result except at the starved slot (there: ratio ~500)
#   A_bf16                  the bound's score term (Dk + 8) u_fp32 T is linear in T = scale sum |q||k|; at T ~ 15 (diffuse) it allows a relative 1e-3 on A, half a bf16
#                           rounding (ratio 2.2); at T ~ 90 (peaked), ~120 (offset) and ~35 (starved) it allows more than one (0.35, 0.21, 0.85).  An honest worst-case
#                           accumulation bound cannot tell a bf16 A from 520 unlucky fp32 roundings there.
#   ds_bf16                 with a bf16 dq on `offset`: every key carries the common vector w, so dq ~ w sum_j ds_ij does not cancel and its own output rounding
#                           u_bf16 |dq| exceeds the random sum of the ds roundings (0.42 / 0.50); with an fp32 dq it is asserted there too (4.8)
#   delta_from_unrounded_o  needs a bf16 o: an fp32 store rounds at 2^-24, inside the bound (0.003), so it is asserted in bf16 only; on `diffuse` in bf16 it reaches
#                           0.99 / 1.00 -- the error u_bf16 sum |dO o| is a random-sign sum while the bound holds the sum of absolute terms
ALL = sb.SLOT_GENERATORS
FWD_MUTANTS = {"no_eps": ("starved",), "tail_token_not_in_z": ALL, "tail_token_not_in_rsum": ALL, "A_bf16": ("diffuse",), "neighbour_head_rsum": ALL}
BWD_MUTANTS = {"ds_bf16": ("diffuse", "peaked", "starved"), "delta_from_unrounded_o": ("peaked", "offset", "starved"), "ext_scaled_by_rinv": ALL, "rinv_of_wrong_slot": ALL}


@pytest.mark.parametrize("kind", sb.SLOT_GENERATORS)
@pytest.mark.parametrize("mutant", list(FWD_MUTANTS))
@pytest.mark.parametrize("family,dtype", [("unfolded", F32), ("valu", F32), ("mfma", BF)])
def test_slot_forward_mutants(family, dtype, mutant, kind):
    rs = fwd_ratios(kind, family, dtype, 33, mutant)
    worst = report(f"slot {family} {dtype} {kind} fwd mutant {mutant}", max(rs.values()))
    if kind in FWD_MUTANTS[mutant]:
        assert worst > 1.0, (family, mutant, kind, rs)


@pytest.mark.parametrize("kind", sb.SLOT_GENERATORS)
@pytest.mark.parametrize("mutant", list(BWD_MUTANTS))
@pytest.mark.parametrize("family,dtype", [("unfolded", F32), ("valu", BF), ("mfma", BF)])
def test_slot_backward_mutants(family, dtype, mutant, kind):
    rs = bwd_ratios(kind, family, dtype, 33, mutant)
    worst = report(f"slot {family} {dtype} {kind} bwd mutant {mutant}", max(rs.values()))
    named = kind in BWD_MUTANTS[mutant] or (mutant == "ds_bf16" and dtype == F32)
    if named and not (mutant == "delta_from_unrounded_o" and dtype == F32):
        assert worst > 1.0, (family, mutant, kind, rs)


# ------------------------------------------------------------------------------------------------ deferred gradients
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("L,S", [(4, 4), (1, 5), (4, 5), (3, 8)])            # L S = 16 (one group), 5, 20 and 24 (two groups)
def test_kv_grad_emulation_and_mutants(dtype, L, S):
    B, N, h, D = 1, 70, 2, 512
    t = sb.stacked_inputs(L, B, S, N, h, D, dtype, seed=5)
    ref, bound = sb.slot_kv_grad_ref(*t, L, B, S, N, h, SCALE, dtype)
    r = report(f"kv_grad {dtype} L={L} S={S} emulation", kb.check("kv_grad emulation", kv_grad_emul(*t, L, B, S, N, h, SCALE, dtype), ref, bound))
    assert r <= 1.0
    if L * S > sb.KVG_PAIRS:
        for mutant in ("group2_overwrites", "group2_dropped"):
            rm = report(f"kv_grad {dtype} L={L} S={S} mutant {mutant}", kb.excess(kv_grad_emul(*t, L, B, S, N, h, SCALE, dtype, mutant), ref, bound)[0])
            assert rm > 1.0, (mutant, rm)
        if dtype == BF:
            # the inter-group rounding is a NAMED term: without it the same emulation is outside the bound
            plain = sb.slot_kv_grad_ref(*t, L, B, S, N, h, SCALE, dtype, inter_group=False)[1]
            rn = report(f"kv_grad {dtype} L={L} S={S} emulation against the bound WITHOUT the inter-group term", kb.excess(kv_grad_emul(*t, L, B, S, N, h, SCALE, dtype), ref, plain)[0])
            assert rn > 1.0, rn


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("L", [1, 4])
def test_context_grad_emulation_and_mutant(dtype, L):
    B, S, N, h, D = 2, 4, 37, 2, 512
    qs, dzs, ds, A, r = sb.stacked_inputs(L, B, S, N, h, D, dtype, seed=6)
    ref, bound = sb.slotf_context_grad_ref(A, r, ds, dzs, qs, L, B, S, N, h, D, SCALE, dtype)
    rr = report(f"context_grad {dtype} L={L} emulation", kb.check("context_grad emulation", context_grad_emul(A, r, ds, dzs, qs, L, B, S, N, h, D, SCALE, dtype), ref, bound))
    assert rr <= 1.0
    rm = report(f"context_grad {dtype} L={L} mutant pack_without_rinv", kb.excess(context_grad_emul(A, r, ds, dzs, qs, L, B, S, N, h, D, SCALE, dtype, "pack_without_rinv"), ref, bound)[0])
    assert rm > 1.0


# ------------------------------------------------------------------------------------------------ matching loss
def loss_emul(t, nb, dtype, crit, labels, w_scene=4000.0, w_mp=1.0, w_md=1.0, mutant=None):
    """loss.hip in torch fp32: fp32 statistics, the fp32 costs and their argmin, one rounding of each gradient to the operand dtype"""
    Z, sl, mp, at = t["Z"].float(), t["slots"].float(), t["maskp"].float(), t["attn"].float()
    target, fg, fgN = t["target"], t["fg"], t["fgN"]
    B = target.shape[0]
    C, D, G = Z.shape[1], sl.shape[1], mp.shape[1]
    S, nh, N = Z.shape[0] // B, at.shape[0] // B, at.shape[2]
    Z, sl, mp, at = Z.reshape(B, S, C), sl.reshape(B, S, D), mp.reshape(B, S, G), at.reshape(B, nh, S, N)
    g = t["g_total"][0] / B
    kl = not (labels or crit == "CE")
    if labels:
        st = t["scene_target"] + nb
    else:
        tch = t["teacher"]
        st = tch.argmax(1) + nb
        Tp = torch.cat([(tch.min() - 1.0).expand(B, nb), tch], 1)
        lt = Tp - torch.logsumexp(Tp, 1, keepdim=True)
    lse = torch.logsumexp(Z, -1)
    per = torch.zeros(B, 5)
    dZ, dS_, dM, dA = torch.zeros(B, S, C), torch.zeros(B, S, D), torch.zeros(B, S, G), torch.zeros(B, nh, S, N)
    match = []
    nrm = sl.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    n = sl / nrm
    dots = n @ n.transpose(1, 2)
    gc = g * 2.0 / (S * (S - 1))
    for b in range(B):
        y, s_ = int(target[b]), int(st[b])
        best, i, j = None, 0, 1
        for a_ in range(S):
            for b_ in range(S):
                c = -torch.exp(Z[b, a_, y] - lse[b, a_]) - torch.exp(Z[b, b_, s_] - lse[b, b_])
                if a_ != b_ and (best is None or c < best):
                    best, i, j = c, a_, b_
        match.append((i, j))
        per[b, 0] = lse[b, i] - Z[b, i, y]
        lse_i = lse[b, j] if mutant == "dZ_other_slots_lse" else lse[b, i]
        oh = torch.zeros(C); oh[y] = 1.0
        vi = g * (torch.exp(Z[b, i] - lse_i) - oh)
        if mutant == "dZ_no_softmax_off_target":
            vi = vi * oh
        dZ[b, i] += vi
        pj = torch.exp(Z[b, j] - lse[b, j])
        if kl:
            wk = w_scene / C
            per[b, 1] = (torch.exp(lt[b]) * (lt[b] - (Z[b, j] - lse[b, j]))).sum() * wk
            dZ[b, j] += g * wk * (pj - torch.exp(lt[b]))
        else:
            per[b, 1] = lse[b, j] - Z[b, j, s_]
            ohs = torch.zeros(C); ohs[s_] = 1.0
            dZ[b, j] += g * (pj - ohs)
        x = mp[b, i]
        per[b, 3] = (x.clamp_min(0) - x * fg[b] + torch.log1p(torch.exp(-x.abs()))).sum() * w_mp / G
        dM[b, i] = g * w_mp / G * (torch.sigmoid(x) - fg[b])
        a = at[b, :, i].sum(0) / nh - fgN[b]
        per[b, 4] = (a * a).sum() * w_md / N
        dA[b, :, i] = g * w_md * 2.0 / N * a / (1.0 if mutant == "d_attn_not_divided_by_nh" else nh)
        cs = 0.0
        for p_ in range(S):
            acc = torch.zeros(D)
            for q_ in range(S):
                if q_ != p_:
                    acc = acc + (n[b, q_] if mutant == "cosine_without_projection" else n[b, q_] - dots[b, p_, q_] * n[b, p_])
                    cs = cs + dots[b, p_, q_]
            dS_[b, p_] = gc * acc / nrm[b, p_]
        per[b, 2] = cs / (S * (S - 1))
    five = per.sum(0) / B
    return {"losses": torch.cat([five, five.sum()[None]]), "dZ": dZ.reshape(B * S, C).to(dtype), "d_slots": dS_.reshape(B * S, D).to(dtype),
            "d_maskp": dM.reshape(B * S, G).to(dtype), "d_attn": dA.reshape(B * nh, S, N), "match": torch.tensor(match, dtype=torch.int32)}


LOSS_MODES = [("KL", False), ("CE", False), ("KL", True), ("CE", True)]            # (scene criterion, ground-truth scene labels)
LOSS_MUTANTS = {"dZ_other_slots_lse": "dZ", "dZ_no_softmax_off_target": "dZ", "cosine_without_projection": "d_slots", "d_attn_not_divided_by_nh": "d_attn"}
_loss_cache = {}


def loss_case(dtype, B, S, nb, crit, labels):
    """inputs and reference, computed once per case and left unchanged"""
    key = (dtype, B, S, nb, crit, labels)
    if key not in _loss_cache:
        t = sb.loss_inputs(B, S, nb, dtype, seed=7, labels=labels)
        _loss_cache[key] = (t, sb.loss_ref(t, nb, dtype, crit, labels))
    return _loss_cache[key]


@pytest.mark.parametrize("crit,labels", LOSS_MODES)
@pytest.mark.parametrize("B,S,nb", [(5, 3, 101), (2, 2, 400), (5, 4, 400)])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_loss_emulation_inside_the_bounds(dtype, B, S, nb, crit, labels):
    t, ref = loss_case(dtype, B, S, nb, crit, labels)
    margin = sb.match_margin(t, nb, labels)
    assert margin >= sb.MATCH_MARGIN, margin
    out = loss_emul(t, nb, dtype, crit, labels)
    assert torch.equal(out["match"], ref["match"]), (out["match"], ref["match"])
    assert torch.equal(ref["logits"], t["Z"].double().reshape(B, S, -1)[torch.arange(B), ref["match"][:, 0].long()])
    for k in sb.LOSS_OUTPUTS:
        r = report(f"loss {dtype} B={B} S={S} nb={nb} {crit}{' labels' if labels else ''} margin {margin:.3f} {k}", kb.check(k, out[k], *ref[k]))
        assert r <= 0.5, (k, r)


@pytest.mark.parametrize("crit,labels", LOSS_MODES)
@pytest.mark.parametrize("mutant", list(LOSS_MUTANTS))
@pytest.mark.parametrize("dtype", [F32, BF])
def test_loss_mutants(dtype, mutant, crit, labels):
    B, S, nb = 5, 3, 101
    t, ref = loss_case(dtype, B, S, nb, crit, labels)
    out = loss_emul(t, nb, dtype, crit, labels, mutant=mutant)
    k = LOSS_MUTANTS[mutant]
    r = report(f"loss {dtype} {crit}{' labels' if labels else ''} mutant {mutant} {k}", kb.excess(out[k], *ref[k])[0])
    assert r > 1.0, (mutant, r)
    for other in sb.LOSS_OUTPUTS:
        if other != k:
            assert kb.excess(out[other], *ref[other])[0] <= 0.5, (mutant, other)
