"""Per-element error bounds against float64 for the distillation kernels of the multi-task baseline's TrainLoss (devias_distill_fwd / _bwd, csrc/distill.hip).

The sibling of slot_loss_bounds.py's matching-loss part (same rules, same measure: excess(out, ref, bound) = max |out - ref| / bound, a test asserts <= 1).  u = U_FP32,
u_T the unit of the student logits' dtype.  Inputs are exact: the student logits z [B, C] (on T's grid), the fp32 teacher logits t [B, Ct], pad = C - Ct.  One
workgroup per row, fp32 statistics, block sums of 256 threads: a sum over n addends carries (n / 256 + 12) u.

    lse   = mx + logf(sum expf(z - mx))      e_lse = u (sum_c p_c (|z_c - mx| + 3) + C / 256 + 12 + 2 |lse| + 2 |mx|)            (row_stats of row_kernels.h)
    ls_c  = z_c - lse                        e_ls  = e_lse + u |ls_c|
    p_c   = expf(ls_c)                       e_p   = p_c (e_ls + 4 u)   -- ABSOLUTE, so p_y -> 1 (p_y - 1 cancels) is handled
    teacher row as the student sees it: tv_c = min(t) - 1 for c < pad (ONE fp32 rounding: e_tv = u |min(t) - 1|; the minimum itself is exact), t_{c - pad} after
    tlse  (as lse, over tv)                  e_tlse = the same formula + sum_c q_c e_tv_c
    lt_c  = tv_c - tlse                      e_lt  = e_tv + e_tlse + u |lt_c|
    q_c   = expf(lt_c)                       e_q   = q_c (e_lt + 4 u)
    KL row = sum_c q_c (lt_c - ls_c)         sum_c [e_q |lt - ls| + q (e_lt + e_ls + u |lt - ls|) + u |term|] + (C / 256 + 12) u sum_c |term|
    CE row = lse - z_y, y = pad + FIRST argmax_c t_c (exact: asserted through the gradient's one-hot)           e_lse + u |row|
    loss  = w / B sum_b row  (w = 1 for CE)  w / B (sum_b e_row + (B + 2) u sum_b |row|) + 3 u |loss|
    dz_c  = T(k (p_c - q_c)),  k = g w / B   (CE: k = g / B, q = onehot(y), e_q = 0)
                                             |k| (e_p + e_q + u |p - q|) + 3 u |dz| + u_T |dz| + 2 |k| 2^-126   (the last: p, q below the normal range are flushed)

SLACK = twice what the CPU emulation (emulate(): these formulas in torch CPU float32 with the kernels' roundings) needs over every case of both test files
(tests/test_multitask_loss_bounds_cpu.py prints the ratios and asserts the emulation stays under HALF the slack).  Never fitted to the HIP kernel.
Mutants (MUTANTS, emulate()): seeded faults the bounds must catch.
"""
import torch

from kernel_bounds import U_FP32, _randn, excess, u_of  # noqa: F401

U = U_FP32
SLACK = 2 * 0.992          # the emulation needs 0.9914 (bf16 dz: the output rounding alone); fp32 dz 0.372; loss 0.090
STD = 6.0                   # peaked logits
MODES = ("KL", "CE")
MUTANTS = ("tie_last_index", "pad_without_mass", "weight_on_ce", "weight_missing_on_kl", "pad_is_min", "mean_over_classes")
# (B, student width C, pad): C - pad teacher columns; pad 400 is the unified head's num_action_classes
CASES = [(B, C, pad) for B in (1, 3, 8) for C, pad in ((2, 0), (365, 0), (765, 0), (765, 400))]


def inputs(B, C, pad, dtype, seed=0):
    """-> dict(z [B, C] in dtype, t fp32 [B, C - pad], g fp32 scalar, w): peaked logits (std 6); the teacher's row 0 holds its maximum TWICE (columns 1 and
    min(3, Ct - 1)), so only the first-index rule picks column 1; where Ct = 2 the tie is columns 0 and 1"""
    Ct = C - pad
    z = (_randn((B, C), seed + 1, "cpu") * STD).to(dtype)
    t = _randn((B, Ct), seed + 2, "cpu") * STD
    top = float(t[0].max()) + 1.0
    first = 1 if Ct > 2 else 0
    t[0, first] = top
    t[0, min(3, Ct - 1)] = top
    return {"z": z, "t": t.contiguous(), "g": torch.tensor([0.75], dtype=torch.float32), "w": 2.0, "pad": pad, "first": first}


def _lse(v):
    """float64 rows v -> (lse [B, 1], p, e_lse [B, 1])"""
    C = v.shape[1]
    mx = v.max(1, keepdim=True).values
    lse = torch.logsumexp(v, 1, keepdim=True)
    p = torch.exp(v - lse)
    e = U * ((p * ((v - mx).abs() + 3)).sum(1, keepdim=True) + C / 256 + 12 + 2 * lse.abs() + 2 * mx.abs())
    return lse, p, e


def padded(I):
    """the float64 teacher rows as the student sees them, and the bound carried by each element"""
    t = I["t"].double()
    B = t.shape[0]
    if not I["pad"]:
        return t, torch.zeros_like(t)
    v = float(t.min()) - 1.0
    tv = torch.cat([torch.full((B, I["pad"]), v, dtype=torch.float64), t], 1)
    e = torch.cat([torch.full((B, I["pad"]), U * abs(v), dtype=torch.float64), torch.zeros_like(t)], 1)
    return tv, e


def bounds(I, mode, dtype):
    """-> (ref, bound) dicts over 'loss' [1] and 'dz' [B, C] at slack 1"""
    uT = u_of(dtype)
    z = I["z"].double()
    B, C = z.shape
    g, w = float(I["g"]), (I["w"] if mode == "KL" else 1.0)
    lse, p, e_lse = _lse(z)
    ls = z - lse
    e_ls = e_lse + U * ls.abs()
    e_p = p * (e_ls + 4 * U)
    if mode == "KL":
        tv, e_tv = padded(I)
        tlse, q, e_tlse = _lse(tv)
        e_tlse = e_tlse + (q * e_tv).sum(1, keepdim=True)
        lt = tv - tlse
        e_lt = e_tv + e_tlse + U * lt.abs()
        e_q = q * (e_lt + 4 * U)
        term = q * (lt - ls)
        e_term = e_q * (lt - ls).abs() + q * (e_lt + e_ls + U * (lt - ls).abs()) + U * term.abs()
        row = term.sum(1)
        e_row = e_term.sum(1) + (C / 256 + 12) * U * term.abs().sum(1)
    else:
        y = I["pad"] + torch.argmax(I["t"].double(), dim=1)
        q = torch.zeros_like(z)
        q[torch.arange(B), y] = 1.0
        e_q = torch.zeros_like(z)
        row = (lse - z.gather(1, y.view(-1, 1))).squeeze(1)
        e_row = e_lse.squeeze(1) + U * row.abs()
    loss = w / B * row.sum()
    e_loss = w / B * (e_row.sum() + (B + 2) * U * row.abs().sum()) + 3 * U * loss.abs()
    k = g * w / B
    dz = k * (p - q)
    e_dz = abs(k) * (e_p + e_q + U * (p - q).abs()) + (3 * U + uT) * dz.abs() + 2 * abs(k) * 2.0 ** -126
    return {"loss": loss.reshape(1), "dz": dz}, {"loss": e_loss.reshape(1), "dz": e_dz}


def ratios(out, ref, bnd):
    return {k: excess(out[k], ref[k], bnd[k] * SLACK)[0] for k in out}


def emulate(I, mode, dtype, mutant=None):
    """The kernels' arithmetic in torch CPU float32 with the output rounding of dz.  `mutant`: one of MUTANTS:
      tie_last_index        the argmax takes the LAST index of a duplicated maximum            (CE)
      pad_without_mass      the pad columns are left out of the teacher's softmax              (KL, pad > 0)
      pad_is_min            the pad value is min(t), not min(t) - 1                            (KL, pad > 0)
      weight_on_ce          the CE branch is multiplied by w
      weight_missing_on_kl  the KL branch is not
      mean_over_classes     the KL is divided by B * C ('mean' instead of 'batchmean')"""
    z, t = I["z"].float(), I["t"].float()
    B, C = z.shape
    pad = I["pad"]
    g = I["g"].float()[0]
    w = torch.tensor(I["w"] if mode == "KL" else 1.0, dtype=torch.float32)
    if mutant == "weight_on_ce" and mode == "CE":
        w = torch.tensor(I["w"], dtype=torch.float32)
    if mutant == "weight_missing_on_kl" and mode == "KL":
        w = torch.tensor(1.0, dtype=torch.float32)
    mx = z.max(1, keepdim=True).values
    lse = mx + torch.log(torch.exp(z - mx).sum(1, keepdim=True))
    p = torch.exp(z - lse)
    if mode == "CE":
        y = torch.argmax(t, dim=1)
        if mutant == "tie_last_index":
            y = t.shape[1] - 1 - torch.argmax(t.flip(1), dim=1)
        y = pad + y
        q = torch.zeros_like(z)
        q[torch.arange(B), y] = 1.0
        row = (lse - z.gather(1, y.view(-1, 1))).squeeze(1)
    else:
        tv = t
        if pad:
            fill = t.min() - (0.0 if mutant == "pad_is_min" else 1.0)
            tv = torch.cat([torch.full((B, pad), float(fill), dtype=torch.float32), t], 1)
        if pad and mutant == "pad_without_mass":
            tmx = t.max(1, keepdim=True).values
            tlse = tmx + torch.log(torch.exp(t - tmx).sum(1, keepdim=True))
            q = torch.cat([torch.zeros((B, pad)), torch.exp(t - tlse)], 1)
            lt = torch.cat([torch.zeros((B, pad)), t - tlse], 1)
        else:
            tmx = tv.max(1, keepdim=True).values
            tlse = tmx + torch.log(torch.exp(tv - tmx).sum(1, keepdim=True))
            lt = tv - tlse
            q = torch.exp(lt)
        row = (q * (lt - (z - lse))).sum(1)
    div = float(B * C) if (mutant == "mean_over_classes" and mode == "KL") else float(B)
    loss = row.sum() / div * w
    k = g * w / div
    return {"loss": loss.reshape(1), "dz": (k * (p - q)).to(dtype).float()}
