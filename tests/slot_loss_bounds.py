"""Per-element error bounds against float64 for the slot cross-attention kernels and the matching loss, on graded inputs.

The sibling of kernel_bounds.py (same rules, same measure: excess(out, ref, bound) = max |out - ref| / bound, a test asserts <= 1): a plain helper module, no
fixtures, no plugin; torch arithmetic on whatever device the arguments live on (the loss reference is the project's CPU oracle and runs on the CPU).  Kernel
sources are cited by file name: slot_unfolded.hip, slot_valu.hip, slot_mfma.hip (below unfolded:, valu:, mfma:) and loss.hip live in devias_amd/csrc/.

Slot attention forward (three kernel families, one unit each: unfolded slot_fwd_kernel unfolded:38, folded VALU slotf_fwd_kernel valu:56, folded matrix-core slotm_kernel mfma:44)
    inputs are exact in both dtypes; scores, the slot softmax and all sums are fp32 in every kernel (unfolded:77-93, valu:88-104, mfma:113-154)
    sim   = scale q.k                        e_sim = (Dk + 8) u_fp32 T_ij,  T_ij = scale sum_d |q_id||k_jd|   (Dk = 512 unfolded, D folded)
    A     = softmax over the SLOT axis       e_A   = a_i (e_sim_ij + sum_i' a_i' e_sim_i'j + (8 + max_i' sim_i'j - sim_ij) u_fp32)   (expf of a rounded difference, divide)
    rsum  = sum_j A + 1e-7                   e_r   = (N + 8) u_fp32 sum_j a + sum_j e_A + 2 u_fp32 rsum   (unfolded:130, valu:156: the addition of 1e-7 and the constant's own rounding)
    o / z = sum_j (A / rsum) v_j             u_out |o| + (N + 8) u_fp32 sum_j abar |v_j| + sum_j e_abar |v_j|,  e_abar = (e_A + abar e_r) / rsum     (unfolded:135, valu:160: one rounding)
    slotm_kernel additionally                u_bf16 sum_j abar_ij |c_j|: A is packed to bf16 for the Z product (mfma:174) while rsum sums the fp32 A (mfma:154) -- no cancellation
Slot attention backward (on the SAVED attn, rsum and the stored o / z the kernel is given; slot_bwd_kernel unfolded:141, slotf_bwd_kernel valu:166, slotm_kernel<BWD>)
    delta_i = dO_i . o_i                     (Dv + 8) u_fp32 sum_d |dO o|                                   (unfolded:159-162, valu:182-185, mfma:75-84)
    dA    = (dAbar - delta) rinv + dA_ext    rinv ((Dv + 8) u_fp32 (|dO|.|v_j| + sum|dO o|) + 4 u_fp32 (|dAbar| + |delta|)) + 2 u_fp32 |dA_ext|   (unfolded:193, valu:211, mfma:156)
    ds    = a (dA - sum_i a dA)              a (e_dA + sum_i a e_dA + (S + 2) u_fp32 sum_i a |dA| + 3 u_fp32 (|dA| + sum_i a |dA|)); fp32, stored unrounded (unfolded:201, valu:219, mfma:167)
    dq    = scale sum_j ds k_j               u_out |dq| + scale sum_j e_ds |k_j| + (N + 8) u_fp32 scale sum_j |ds||k_j|     (one rounding: unfolded:235, valu:252)
    slotm_kernel additionally                u_bf16 scale sum_j |ds_ij||c_j|: scale dS is packed to bf16 for the dQ' product (mfma:172-174)
    All sums of ABSOLUTE terms: a result that cancels (dAbar against delta, dA against its slot mean) is held to the size of what was subtracted.
Deferred gradients (factor 1, rigorous)
    devias_slot_attn_kv_grad (unfolded:244)          u_out |r| + (L S + 8) u_fp32 sum |coef||vec|, and in bf16 ONE MORE u_out |running value| per completed group of 16
                                             (layer, slot) pairs: the kernel stores dk / dv (unfolded:311-312) and re-loads them (unfolded:293) between groups.  Named here, not
                                             removed: keeping the running sums in registers needs every pair's q / dO in LDS at once (128 KB at L S = 32), and an
                                             fp32 side buffer costs a second [B N, 2 h 512] stream; both cost more than the rounding is worth.
    slotf_context_grad (ops.py)              devias_slotf_pack rounds A / rsum and scale ds to the operand dtype (valu:273, valu:275): (u_dt + 3 u_fp32) sum |coef||vec|; the
                                             batched GEMM carries kernel_bounds' GEMM bound with K = 2 L h S: u_out |dc| + (K + 8) u_fp32 sum |coef||vec|
Matching loss (loss.hip; one workgroup per sample, fp32 statistics, block sums of 256 threads: a sum over n addends carries (n / 256 + 12) u_fp32)
    lse   = mx + logf(sum expf(z - mx))      e_lse = u_fp32 (sum_c p_c (|z_c - mx| + 3) + C / 256 + 12 + 2 |lse| + 2 |mx|)          (row_stats :48-55)
    p_c   = expf(z_c - lse)                  e_p   = p_c (e_lse + u_fp32 |z_c - lse| + 4 u_fp32)  -- ABSOLUTE, so p_y -> 1 (p_y - 1 cancels) is handled
    dZ    = g (p_c - 1[c = y]) on row i*;  g (p_c - 1[c = st]) (CE, labels) or g w_scene / C (p_c - t_c) (KL) on row j*:  the propagated e_p (and e_t of the teacher's
            softmax, with the pad = min - 1 rounding, :62-70) + 3 u_fp32 of the terms + one output rounding     (:258-275)
    d_maskp = g w_mp / G (sigmoid(x) - t)    |coef| (6 u_fp32 sigma + 2 u_fp32 (sigma + t)) + u_out |.|                               (:278-287)
    d_attn  = g w_md 2 / N a / nh,  a = mean_h attn - fgN:   |coef| / nh ((nh + 2) u_fp32 (mean_h |attn| + |fgN|) + 4 u_fp32 |a|) + 6 u_fp32 |.|   (:289-298)
    d_slots = gc / |x_i| sum_{j != i} (n_j - dots_ij n_i):  against sum_j (|n_j| + |dots_ij||n_i|), with e_n = (D / 256 + 14) u_fp32 for each of the two divisions by
              nrm and e_dots = 3 (D / 256 + 14) u_fp32 |n_i|.|n_j|;  one output rounding                                            (:301-331)
    the six scalars: the same terms summed (:155-207) and the mean over B (:211-219); out_logits is an exact copy; match is asserted EQUAL.

Constants.  The deferred-gradient bounds are rigorous (factor 1; a bf16 store alone reaches 0.99).  The others hold first-order arguments and device
transcendentals and carry ONE scalar slack each, set as kernel_bounds.py sets its own: twice what the CPU emulation (tests/test_slot_loss_bounds_cpu.py: the
float64 reference plus exactly the named roundings in torch CPU arithmetic) needs to stay at 1 over all generators.  Never fitted to a HIP kernel.

    bound                       slack    emulation's worst ratio at that slack (test_slot_loss_bounds_cpu.py prints them)
    slot attention forward      1.1352   out 0.50 (folded VALU, bf16, starved), 0.49 unfolded bf16, 0.40 slotm;  fp32 out 0.001;  attn 0.004;  rsum 0.001
    slot attention backward     1.6936   dq 0.50 (folded VALU, bf16, peaked), 0.48 unfolded bf16, 0.35 slotm;  fp32 dq 0.001;  ds 0.003
    kv_grad                     1        dkv 0.995 bf16 (the output rounding alone), 0.30 fp32
    context grad                1        dc 0.79 bf16, 0.11 fp32
    matching loss               1.99     dZ 0.50, d_slots 0.50, d_maskp 0.49 (bf16: the output rounding);  fp32 dZ 0.13, d_maskp 0.13, d_slots 0.04;  d_attn 0.11;  scalars 0.02
Each slack is twice what the emulation needs to stay at 1: 0.56760 -> 2 x 0.5676, 0.84674 -> 2 x 0.8468, 0.994 -> 2 x 0.995.  In fp32 the slot-attention bounds are two
to three orders of magnitude above the emulation: their (Dk + 8) u_fp32 T and (N + 8) u_fp32 terms are worst-case LINEAR accumulation bounds, as the issue states them
and as kernel_bounds.py states the GEMM's; what they still tell apart in fp32 is what the seeded mutants show (a token, a slot, a head, an rinv, the 1e-7).

Generators (SLOT_GENERATORS, slot_inputs; stacked_inputs; loss_inputs) say in their docstrings which failure each makes visible.
MATCH_MARGIN: loss_inputs builds every sample so that the best and the second-best assignment cost differ by at least that much on the float64 reference (checked
on the CPU by match_margin, asserted by both test files): the fp32 costs of the kernel (:145) carry ~1e-6, so `match` cannot legitimately flip and is asserted equal.
"""
import math

import torch

from kernel_bounds import U_BF16, U_FP32, _randn, graded, u_of

SLACK_SLOT_FWD = 2 * 0.5676    # the emulation needs 0.56760
SLACK_SLOT_BWD = 2 * 0.8468    # the emulation needs 0.84674
SLACK_LOSS = 2 * 0.995         # the emulation needs 0.994 (a bf16 store of dZ / d_slots)
EPS_RSUM = 1e-7
SLOT_SCALE = 512 ** -0.5
KVG_PAIRS = 16                  # slot_unfolded.hip:242
MATCH_MARGIN = 0.05
SLOT_GENERATORS = ("diffuse", "peaked", "offset", "starved")


# ------------------------------------------------------------------------------------------------ layouts
def slot_views(q, src, B, S, N, h, folded):
    """float64 (q [B, h, S, Dk], keys [B, h | 1, N, Dk], values [B, h | 1, N, Dv]) of q [B S, h Dk] and kv [B N, 2 h dh] (unfolded) or ctx [B N, D] (folded: keys = values = ctx)"""
    q4 = slot_heads(q, B, S, h)
    if folded:
        c = src.double().reshape(B, 1, N, -1)
        return q4, c, c
    kv = src.double().reshape(B, N, 2, h, -1)
    return q4, kv[:, :, 0].permute(0, 2, 1, 3), kv[:, :, 1].permute(0, 2, 1, 3)


def slot_heads(t, B, S, h):
    """[B S, h D] -> float64 [B, h, S, D]"""
    return t.double().reshape(B, S, h, -1).permute(0, 2, 1, 3)


def slot_rows(t):
    """[B, h, S, D] -> [B S, h D]"""
    B, h, S, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, h * D)


# ------------------------------------------------------------------------------------------------ generators
def slot_inputs(kind, B, S, N, h, D, dtype, folded, seed=0, device="cpu"):
    """q (or q') [B S, h D], src = kv [B N, 2 h D] (unfolded) or ctx [B N, D] (folded), d_o (or dz) [B S, h D], dA_ext fp32 [B h, S, N]; logit = SLOT_SCALE q.k.
      diffuse   logit std 1: every slot takes part at every token; an error of one slot, head or token shows at its own scale
      peaked    logit std 6 over the slots: A is nearly one-hot per token, so the softmax' propagated score error and a wrong slot's rinv are not averaged away
      offset    every key carries a common vector w (queries are projected off it, so the slot softmax does not see it): T = scale sum |q||k| is large, as for
                real keys with a common component -- the score-accumulation term is exercised, and a rounding of the scores (bf16 q or k) would show
      starved   the last slot's query carries a component against w: its logit is about 20 below the others at EVERY token, so its rsum is of the order of the
                1e-7 guard (N e^-20 ~ 1e-7): the + 1e-7, the division and the backward's rinv are exercised where they matter (S = 1 has no such slot)
    In all four V and d_o are graded per head (2^-6, 1, 2^5) and per slot (1, 2^-4, 2^3, 2^-2): an error confined to one head or slot is held to ITS scale.
    Unfolded V is graded per token too; the folded context is graded per COLUMN with q' graded inversely (logits unchanged, every z / dq' column scale present).
    dA_ext is graded per token with period 7 (coprime to 32, 64, 128): every 64-, 128- and 32-token tail holds every scale."""
    std = 6.0 if kind == "peaked" else 1.0
    a = math.sqrt(std / (SLOT_SCALE * math.sqrt(D)))
    q = _randn((B, S, h, D), seed + 1, device) * a
    k = _randn((B, N, 1 if folded else h, D), seed + 2, device) * a
    off = {"offset": 8.0, "starved": 2.0}.get(kind, 0.0)
    if off:
        w = off * (1.0 - 2.0 * (torch.arange(D, device=device) % 2)).float()
        q = q - (q @ w)[..., None] / float(w @ w) * w
        k = k + w
        if kind == "starved" and S > 1:
            q[:, S - 1] -= 20.0 / (SLOT_SCALE * float(w @ w)) * w
    head = torch.tensor([2.0 ** -6, 1.0, 2.0 ** 5], device=device)[torch.arange(h, device=device) % 3]
    slot = torch.tensor([1.0, 2.0 ** -4, 2.0 ** 3, 2.0 ** -2], device=device)[torch.arange(S, device=device) % 4]
    d_o = _randn((B, S, h, D), seed + 3, device) * head.flip(0)[None, None, :, None] * slot[None, :, None, None]
    if folded:
        col = graded(D, 3, device).float()
        src = (k[:, :, 0] * col).reshape(B * N, D)
        q = q / col
    else:
        rows = graded(N, 3, device).float()
        v = _randn((B, N, h, D), seed + 4, device) * head[None, None, :, None] * rows[None, :, None, None]
        src = torch.stack([k, v], dim=2).reshape(B * N, 2 * h * D)
    dA_ext = _randn((B * h, S, N), seed + 5, device) * 0.01 * graded(N, 3, device).float()
    return q.reshape(B * S, h * D).to(dtype), src.to(dtype), d_o.reshape(B * S, h * D).to(dtype), dA_ext.contiguous()


def stacked_inputs(L, B, S, N, h, D, dtype, seed=0, device="cpu"):
    """q_stack, do_stack [L, B S, h D]; ds_stack, attn_stack fp32 [L, B h, S, N]; rsum_stack fp32 [L, B h, S] for the deferred gradients of L weight-tied layers.
    ds and A are graded per (layer, token): 2^(-4 ((j - l) mod L)) -- at token j layer j mod L dominates the sum by 2^4 over the next one, so for every group of 16
    (layer, slot) pairs there are tokens where THAT group carries the result: a group that is dropped, overwritten or rounded once more shows at those tokens."""
    lj = (torch.arange(N, device=device)[None, :] - torch.arange(L, device=device)[:, None]) % L
    g = torch.pow(torch.tensor(2.0, device=device), -4.0 * lj.float())[:, None, None, :]
    qs = _randn((L, B * S, h * D), seed + 1, device).to(dtype)
    dos = _randn((L, B * S, h * D), seed + 2, device).to(dtype)
    ds = (_randn((L, B * h, S, N), seed + 3, device) * g).contiguous()
    A = (torch.softmax(_randn((L, B * h, S, N), seed + 4, device), dim=2) * g).contiguous()
    r = _randn((L, B * h, S), seed + 5, device).abs() + 0.5
    return qs, dos, ds, A, r


def loss_inputs(B, S, nb, dtype, ns=365, D=768, G=196, N=300, nh=4, seed=0, device="cpu", labels=False):
    """The tensors of one devias_head_match_loss[_labels] call as a dict.  Three sample kinds, b mod 3:
      0 diffuse    Z ~ 2 randn: the non-target p_c are ~1e-3 -- a softmax term that is missing or scaled (the other slot's lse) shows against ITS OWN size, not the
                   target class' g (p_y - 1)
      1 confident  Z[i*, y] = 22, p_y ~ 1 - 1e-6: p_y - 1 cancels, the bound there is absolute
      2 offset     the sample's Z rows carry + 80: lse ~ 85, so the fp32 rounding of lse (5e-6) is what limits every p_c
    In every sample slot i* = b mod S holds 10 at the action class and j* = (b + 1) mod S at the scene class (p ~ 0.9 there against ~1e-3 in the other slots),
    which keeps the assignment MATCH_MARGIN clear; the other 465 ... 764 classes of those rows stay diffuse.
    teacher: rows graded 2^-2 ... 2^2 (a wide range: the pad = min - 1 path); maskp holds exact 0 and 1; slots are graded 2^-6 ... 2^6 per row and slot 1 is nearly
    parallel to slot 0 (n_j - dots n_i cancels to 1e-2); g_total = 0.37."""
    C = nb + ns
    gi = torch.Generator(device="cpu").manual_seed(seed + 10)
    target = torch.randint(0, nb, (B,), generator=gi)
    scene = torch.randint(0, ns, (B,), generator=gi)
    teacher = _randn((B, ns), seed + 1, "cpu") * 3.0 * graded(B, 2).float()[:, None]
    st = scene if labels else teacher.argmax(1)
    Z = _randn((B, S, C), seed + 2, "cpu") * 2.0
    for b in range(B):
        i, j = b % S, (b + 1) % S
        Z[b, j, nb + int(st[b])] = 10.0
        Z[b, i, int(target[b])] = 22.0 if b % 3 == 1 else 10.0
        if b % 3 == 2:
            Z[b] += 80.0
    slots = _randn((B * S, D), seed + 3, "cpu").reshape(B, S, D)
    slots[:, 1] = 1.5 * slots[:, 0] + 0.01 * _randn((B, D), seed + 4, "cpu")
    slots = slots.reshape(B * S, D) * graded(B * S, 6).float()[:, None]
    maskp = torch.sigmoid(_randn((B * S, G), seed + 5, "cpu"))
    maskp[:, 0::7] = 0.0
    maskp[:, 3::7] = 1.0
    attn = torch.softmax(_randn((B * nh, S, N), seed + 6, "cpu"), dim=1)
    fg = torch.randint(0, 257, (B, G), generator=gi) / 256.0
    fgN = torch.randint(0, 257, (B, N), generator=gi) / 256.0
    t = {"Z": Z.reshape(B * S, C).to(dtype), "slots": slots.to(dtype), "maskp": maskp.to(dtype), "attn": attn.contiguous(), "teacher": teacher, "target": target,
         "scene_target": scene, "fg": fg, "fgN": fgN, "g_total": torch.tensor([0.37])}
    return {k: v.to(device) for k, v in t.items()}


def match_margin(t, nb, labels=False):
    """smallest gap, over the samples, between the best and the second-best assignment cost -p[i, y] - p[j, st] (i != j) on the float64 reference, on the CPU"""
    B = t["target"].shape[0]
    p = t["Z"].double().cpu().softmax(-1).reshape(B, -1, t["Z"].shape[1])
    st = (t["scene_target"].cpu() if labels else t["teacher"].cpu().argmax(1)) + nb
    S = p.shape[1]
    gaps = []
    for b in range(B):
        costs = sorted(float(-p[b, i, t["target"][b]] - p[b, j, st[b]]) for i in range(S) for j in range(S) if i != j)
        gaps.append(costs[1] - costs[0] if len(costs) > 1 else float("inf"))
    return min(gaps)


# ------------------------------------------------------------------------------------------------ slot attention
def slot_fwd_ref(q, src, B, S, N, h, scale, dtype, folded, mfma=False):
    """{"attn": [B h, S, N], "rsum": [B h, S], "out": [B S, h Dv]}: (ref, bound) each; mfma: the call is served by slotm_kernel"""
    q4, k4, v4 = slot_views(q, src, B, S, N, h, folded)
    Dk = q4.shape[-1]
    u, uo = U_FP32, u_of(dtype)
    sim = scale * (q4 @ k4.transpose(-1, -2))
    T = scale * (q4.abs() @ k4.abs().transpose(-1, -2))
    a = sim.softmax(2)
    e_sim = (Dk + 8) * u * T
    e_a = a * (e_sim + (a * e_sim).sum(2, keepdim=True) + (8 + sim.amax(2, keepdim=True) - sim) * u)
    sa = a.sum(-1)
    rsum = sa + EPS_RSUM
    e_r = (N + 8) * u * sa + e_a.sum(-1) + 2 * u * rsum
    abar = a / rsum[..., None]
    e_abar = (e_a + abar * e_r[..., None]) / rsum[..., None]
    o = abar @ v4
    av = abar @ v4.abs()
    f = (N + 8) * u * av + e_abar @ v4.abs()
    if mfma:
        f = f + U_BF16 * av
    s = SLACK_SLOT_FWD
    return {"attn": (a.reshape(B * h, S, N), s * e_a.reshape(B * h, S, N)), "rsum": (rsum.reshape(B * h, S), s * e_r.reshape(B * h, S)),
            "out": (slot_rows(o), slot_rows(s * (uo * o.abs() + f)))}


def slot_bwd_ref(src, attn, rsum, o, d_o, dA_ext, B, S, N, h, scale, dtype, folded, mfma=False):
    """{"dq": [B S, h Dk], "ds": [B h, S, N]}: (ref, bound) each, for the SAVED attn / rsum and the STORED o (or z) the kernel is given"""
    dO, k4, v4 = slot_views(d_o, src, B, S, N, h, folded)
    o4 = slot_heads(o, B, S, h)
    a, rinv = attn.double().reshape(B, h, S, N), 1.0 / rsum.double().reshape(B, h, S, 1)
    u, uo = U_FP32, u_of(dtype)
    kf = (dO.shape[-1] + 8) * u
    delta = (dO * o4).sum(-1, keepdim=True)
    a_delta = (dO * o4).abs().sum(-1, keepdim=True)
    dAbar = dO @ v4.transpose(-1, -2)
    a_dAbar = dO.abs() @ v4.abs().transpose(-1, -2)
    ext = dA_ext.double().reshape(B, h, S, N) if dA_ext is not None else torch.zeros_like(a)
    dA = (dAbar - delta) * rinv + ext
    e_dA = rinv * (kf * (a_dAbar + a_delta) + 4 * u * (dAbar.abs() + delta.abs())) + 2 * u * ext.abs()
    ts = (a * dA).sum(2, keepdim=True)
    a_ts = (a * dA.abs()).sum(2, keepdim=True)
    e_ts = (a * e_dA).sum(2, keepdim=True) + (S + 2) * u * a_ts
    ds = a * (dA - ts)
    e_ds = a * (e_dA + e_ts + 3 * u * (dA.abs() + a_ts))
    dq = scale * (ds @ k4)
    ak = scale * (ds.abs() @ k4.abs())
    f = scale * (e_ds @ k4.abs()) + (N + 8) * u * ak
    if mfma:
        f = f + U_BF16 * ak
    s = SLACK_SLOT_BWD
    return {"dq": (slot_rows(dq), slot_rows(s * (uo * dq.abs() + f))), "ds": (ds.reshape(B * h, S, N), s * e_ds.reshape(B * h, S, N))}


def _pairs(t, L, B, S, h):
    """[L, B S, h D] -> float64 [B, h, L S, D], pair p = l S + i (the kernel's order, slot_unfolded.hip:263)"""
    return t.double().reshape(L, B, S, h, -1).permute(1, 3, 0, 2, 4).reshape(B, h, L * S, -1)


def _pair_coefs(t, L, B, S, N, h):
    """[L, B h, S, N] -> float64 [B, h, L S, N]"""
    return t.double().reshape(L, B, h, S, N).permute(1, 2, 0, 3, 4).reshape(B, h, L * S, N)


def slot_kv_grad_ref(q_stack, do_stack, ds_stack, attn_stack, rsum_stack, L, B, S, N, h, scale, dtype, inter_group=True):
    """(ref, bound) of dkv [B N, 2 h dh]; factor 1.  inter_group = False leaves the bf16 store / re-load between groups out (what an ideal kernel would need)"""
    u, uo = U_FP32, u_of(dtype)
    P = L * S
    cab = attn_stack.double() / rsum_stack.double()[..., None]
    parts = []
    for coef, vec in ((scale * _pair_coefs(ds_stack, L, B, S, N, h), _pairs(q_stack, L, B, S, h)), (_pair_coefs(cab, L, B, S, N, h), _pairs(do_stack, L, B, S, h))):
        ref = coef.transpose(-1, -2) @ vec
        bound = uo * ref.abs() + (P + 8) * u * (coef.abs().transpose(-1, -2) @ vec.abs())
        if dtype == torch.bfloat16 and inter_group:
            for p1 in range(KVG_PAIRS, P, KVG_PAIRS):              # the value stored after each completed group but the last (slot_unfolded.hip:293, 311)
                bound = bound + uo * (coef[:, :, :p1].transpose(-1, -2) @ vec[:, :, :p1]).abs()
        parts.append((ref, bound))
    pack = lambda i: torch.stack([parts[0][i], parts[1][i]], dim=2).permute(0, 3, 2, 1, 4).reshape(B * N, -1)  # noqa: E731  [B, h, 2, N, dh] -> [B N, 2 h dh]
    return pack(0), pack(1)


def slotf_context_grad_ref(attn_stack, rsum_stack, ds_stack, dz_stack, qp_stack, L, B, S, N, h, D, scale, dtype):
    """(ref, bound) of dc [B N, D]; factor 1"""
    u, uo = U_FP32, u_of(dtype)
    K = 2 * L * h * S
    cab = attn_stack.double() / rsum_stack.double()[..., None]
    ref = torch.zeros(B, N, D, dtype=torch.float64, device=qp_stack.device)
    ab = torch.zeros_like(ref)
    for coef, vec in ((cab, dz_stack), (scale * ds_stack.double(), qp_stack)):
        c5, v5 = coef.reshape(L, B, h, S, N), vec.double().reshape(L, B, S, h, D)
        ref = ref + torch.einsum("lbhsn,lbshd->bnd", c5, v5)
        ab = ab + torch.einsum("lbhsn,lbshd->bnd", c5.abs(), v5.abs())
    bound = uo * ref.abs() + ((K + 8) * u + uo + 3 * u) * ab
    return ref.reshape(B * N, D), bound.reshape(B * N, D)


# ------------------------------------------------------------------------------------------------ matching loss
LOSS_OUTPUTS = ("losses", "dZ", "d_slots", "d_maskp", "d_attn")


def loss_ref(t, nb, dtype, crit="KL", labels=False, w_scene=4000.0, w_mp=1.0, w_md=1.0):
    """t: loss_inputs' dict (the values the kernel sees).  The reference is oracle/ref_cpu.train_loss (tests/hvu_ref.hvu_train_loss with labels) in float64 with
    autograd, on the CPU.  {"losses": [6], "dZ", "d_slots", "d_maskp", "d_attn": (ref, bound) on the CPU, "match": int [B, 2], "logits": [B, C] (exact copy)}"""
    import hvu_ref
    from oracle import ref_cpu
    Z, sl, mp, at = (t[k].detach().double().cpu().requires_grad_(True) for k in ("Z", "slots", "maskp", "attn"))
    target, fg, fgN = t["target"].cpu(), t["fg"].double().cpu(), t["fgN"].double().cpu()
    g = float(t["g_total"][0])
    out = (None, (None, None, at), (Z, sl, mp))
    if labels:
        total, logits, ld, idx = hvu_ref.hvu_train_loss(out, target, t["scene_target"].cpu(), (fg, fgN), nb, crit, w_mp, w_md)
    else:
        total, logits, ld, idx = ref_cpu.train_loss(ref_cpu.SlotViTConfig(num_classes=nb), out, t["teacher"].double().cpu(), target, (fg, fgN), w_scene, w_mp, w_md, crit)
    total.reshape(()).backward(torch.tensor(g, dtype=torch.float64))
    B = target.shape[0]
    C, D, G = Z.shape[1], sl.shape[1], mp.shape[1]
    S, nh, N = Z.shape[0] // B, at.shape[0] // B, at.shape[2]
    ns = C - nb
    u, uo = U_FP32, u_of(dtype)
    ar, ii, jj = torch.arange(B), idx[0], idx[1]
    gB = abs(g) / B
    kl = not (labels or crit == "CE")
    # ---- row statistics and probabilities
    Zd = Z.detach().reshape(B, S, C)
    mx, lse = Zd.amax(-1), torch.logsumexp(Zd, -1)
    p = torch.exp(Zd - lse[..., None])
    e_lse = u * ((p * ((Zd - mx[..., None]).abs() + 3)).sum(-1) + C / 256 + 12 + 2 * lse.abs() + 2 * mx.abs())
    e_p = p * (e_lse[..., None] + u * (Zd - lse[..., None]).abs() + 4 * u)
    y = target
    st = (t["scene_target"].cpu() if labels else t["teacher"].cpu().argmax(1)) + nb
    oh_y = torch.zeros(B, C, dtype=torch.float64).scatter_(1, y[:, None], 1.0)
    oh_s = torch.zeros(B, C, dtype=torch.float64).scatter_(1, st[:, None], 1.0)
    bZ = torch.zeros(B, S, C, dtype=torch.float64)
    bZ[ar, ii] += gB * (e_p[ar, ii] + 3 * u * (p[ar, ii] + oh_y))
    e_act = e_lse[ar, ii] + 2 * u * (lse[ar, ii].abs() + Zd[ar, ii, y].abs())
    if kl:
        tch = t["teacher"].double().cpu()
        pad = tch.min() - 1.0
        Tp = torch.cat([pad.expand(B, nb), tch], 1)
        tmx, tl = tch.amax(1), torch.logsumexp(Tp, 1)
        tc = torch.exp(Tp - tl[:, None])
        is_pad = (torch.arange(C) < nb).double()[None, :]
        e_tl = u * ((tc * ((Tp - tmx[:, None]).abs() + 3 + is_pad * pad.abs())).sum(1) + C / 256 + 12 + 2 * tl.abs() + 2 * tmx.abs())
        e_lt = e_tl[:, None] + u * (Tp.abs() + tl[:, None].abs() + is_pad * pad.abs())
        e_t = tc * (e_lt + 4 * u)
        wk = w_scene / C
        bZ[ar, jj] += gB * wk * (e_p[ar, jj] + e_t + 4 * u * (p[ar, jj] + tc))
        lz = Zd[ar, jj] - lse[ar, jj][:, None]
        lt = Tp - tl[:, None]
        e_lz = e_lse[ar, jj][:, None] + u * lz.abs()
        scn = (tc * (lt - lz)).abs().sum(1)
        e_scn = wk * ((e_t * (lt - lz).abs() + tc * (e_lt + e_lz + 2 * u * (lt - lz).abs())).sum(1) + (C / 256 + 12 + 3) * u * scn)
    else:
        bZ[ar, jj] += gB * (e_p[ar, jj] + 3 * u * (p[ar, jj] + oh_s))
        e_scn = e_lse[ar, jj] + 2 * u * (lse[ar, jj].abs() + Zd[ar, jj, st].abs())
    # ---- mask prediction (row i* only)
    x = mp.detach().reshape(B, S, G)[ar, ii]
    sg = torch.sigmoid(x)
    bM = torch.zeros(B, S, G, dtype=torch.float64)
    bM[ar, ii] = gB * w_mp / G * (6 * u * sg + 2 * u * (sg + fg))
    tau = x.clamp_min(0) + (x * fg).abs() + torch.log1p(torch.exp(-x.abs()))
    e_mp = w_mp / G * (G / 256 + 12 + 8) * u * tau.sum(1)
    # ---- mask distillation
    A5 = at.detach().reshape(B, nh, S, N)
    am = A5.mean(1)[ar, ii]
    adiff = am - fgN
    e_a = (nh + 2) * u * (am.abs() + fgN.abs())
    bA = torch.zeros(B, nh, S, N, dtype=torch.float64)
    bA[ar, :, ii] = (gB * w_md * 2.0 / N / nh * (e_a + 4 * u * adiff.abs()))[:, None, :].expand(B, nh, N)
    e_md = w_md / N * ((2 * adiff.abs() * e_a + 2 * u * adiff ** 2).sum(1) + (N / 256 + 12 + 3) * u * (adiff ** 2).sum(1))
    # ---- cosine term
    xs = sl.detach().reshape(B, S, D)
    nrm = xs.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    n = xs / nrm
    e_n = (D / 256 + 14) * u
    dots = n @ n.transpose(1, 2)
    adots = n.abs() @ n.abs().transpose(1, 2)
    e_dots = 3 * e_n * adots
    offd = 1.0 - torch.eye(S, dtype=torch.float64)
    terms = torch.einsum("ij,bjd->bid", offd, n.abs()) + (dots.abs() * offd).sum(2, keepdim=True) * n.abs()
    e_acc = e_n * terms + (e_dots * offd).sum(2, keepdim=True) * n.abs() + (S + 3) * u * terms
    gc = gB * 2.0 / (S * (S - 1)) if S > 1 else 0.0
    bS = (gc / nrm * (e_acc + (e_n + 3 * u) * terms)).reshape(B * S, D)
    e_cos = ((e_dots + 3 * u * dots.abs()) * offd).sum((1, 2)) / (S * (S - 1)) if S > 1 else torch.zeros(B, dtype=torch.float64)
    # ---- the six scalars: per-sample errors, then the mean over B and the total
    names = ("action_loss", "scene_loss", "cosine_loss", "mask_prediction_loss", "mask_distill_loss")
    ref6 = torch.tensor([ld[k] for k in names] + [float(total)], dtype=torch.float64)
    e5 = torch.stack([e_act.mean(), e_scn.mean(), e_cos.mean(), e_mp.mean(), e_md.mean()]) + (B + 2) * u * ref6[:5].abs()
    e6 = torch.cat([e5, (e5.sum() + 6 * u * ref6[:5].abs().sum())[None]])
    s = SLACK_LOSS
    grads = {"dZ": (Z.grad, bZ.reshape(B * S, C)), "d_slots": (sl.grad, bS), "d_maskp": (mp.grad, bM.reshape(B * S, G)), "d_attn": (at.grad, bA.reshape(B * nh, S, N))}
    out = {k: (r, s * ((U_FP32 if k == "d_attn" else uo) * r.abs() + b)) for k, (r, b) in grads.items()}
    out["losses"] = (ref6, s * (e6 + u * ref6.abs()))
    out["match"] = torch.stack([ii, jj], 1).to(torch.int32)
    out["logits"] = logits.detach()
    return out
