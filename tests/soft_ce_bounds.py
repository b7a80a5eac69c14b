"""Per-element error bounds against float64 for the soft-target chain of a mixed batch: devias_mixup_target (the dense target) and devias_soft_ce_fwd / _bwd (timm's
SoftTargetCrossEntropy), csrc/mixup.hip.

The sibling of multitask_loss_bounds.py (same rules, same measure: excess(out, ref, bound) = max |out - ref| / bound, a test asserts <= 1).  u = U_FP32, u_T the unit of
the logits' dtype.  Inputs are exact: logits z [B, C] (on T's grid), labels y [B], fp32 on / off values and per-row fp32 weights ws, wo.  One workgroup per row, fp32
statistics, block sums of 256 threads: a sum over n addends carries (n / 256 + 12) u.  No product is fused with a sum (the unit is compiled without contraction).

    t_c   = fl(v(y_b, c) ws) + fl(v(y_{B-1-b}, c) wo)     e_t  = u (|v1 ws| + |v2 wo| + |t_c|)          (v = on at the label, off elsewhere)
            rows the tests override exactly -- a one-hot row, a row times 0.5, a zero row -- carry e_t = 0, 0.5 e_t, 0
    v_c   = z_c - mx                                       e_v  = u |v_c|
    lser  = logf(sum_c expf(v_c))                          e_lser = u (sum_c p_c (|v_c| + 3) + C / 256 + 12 + 2 |lser|)
    St    = sum_c t_c                                      e_St = sum_c e_t + (C / 256 + 12) u sum_c |t_c|
    Stz   = sum_c fl(t_c v_c)                              e_Stz = sum_c (e_t |v_c| + 2 u |t_c v_c|) + (C / 256 + 12) u sum_c |t_c v_c|
    row   = fl(fl(lser St) - Stz)                          e_lser |St| + |lser| e_St + u |lser St| + e_Stz + u |row|     (no cancellation: t >= 0, v <= 0, lser >= 0)
    loss  = (sum_b row_b) / B                              1 / B (sum_b e_row + (B + 2) u sum_b |row|) + 3 u |loss|
    lse   = mx + lser                                      e_lse = e_lser + u (2 |lse| + 2 |mx|)                                          (row_stats of row_kernels.h)
    p_c   = expf(z_c - lse)                                e_p  = p_c (e_lse + u |z_c - lse| + 4 u)   -- ABSOLUTE, so p_y St - t_y -> 0 (a one-hot row) is handled
    dz_c  = T(k (p_c St - t_c)),  k = g / B                |k| (e_p |St| + p_c e_St + u |p_c St| + e_t + u |p_c St - t_c|) + 3 u |dz| + u_T |dz| + 2 |k| 2^-126

SLACK = twice what the CPU emulation (emulate(): these formulas in torch CPU float32 with the kernels' roundings) needs over every case
(tests/test_soft_ce_bounds_cpu.py prints the ratios and asserts the emulation stays under HALF the slack).  Never fitted to the HIP kernel.
Mutants (MUTANTS, emulate()): seeded faults the bounds must catch.
"""
import numpy as np
import torch

from kernel_bounds import U_FP32, _randn, excess, u_of  # noqa: F401

U = U_FP32
SLACK = 2 * 0.977        # the emulation needs 0.9760 (bf16 dz: the output rounding alone); fp32 dz 0.304; t 0.602; loss 0.106
STD = 6.0                # peaked logits
SMOOTHING = 0.1
MUTANTS = ("sum_t_assumed_one", "mean_over_classes", "partner_not_flipped", "smoothing_dropped", "grad_without_1_over_B")
CASES = [(B, C) for B in (1, 3, 8) for C in (2, 257, 400)]          # 257: one past the 256-thread stride
ROW_KINDS = ("mixed", "one_hot", "half", "zero")                     # row b is ROW_KINDS[b % 4]


def on_off(C, smoothing=SMOOTHING):
    """mixup_target's values: Python doubles, then fp32"""
    off = smoothing / C
    return float(np.float32(1. - smoothing + off)), float(np.float32(off))


def inputs(B, C, dtype, seed=0):
    """-> dict(z [B, C] in dtype, y int64 [B], ws / wo fp32 [B], on, off, g fp32 scalar).  Labels differ between a clip and its partner wherever the batch has two
    clips to tell apart; the weights are a mixup's (lam, 1 - lam in fp32)."""
    z = (_randn((B, C), seed + 1, "cpu") * STD).to(dtype)
    y = torch.tensor([(3 * b + 1) % C for b in range(B)], dtype=torch.int64)
    ws = torch.tensor([0.3 + 0.05 * b for b in range(B)], dtype=torch.float32)
    wo = torch.ones(B, dtype=torch.float32) - ws
    on, off = on_off(C)
    return {"z": z, "y": y, "ws": ws, "wo": wo, "on": on, "off": off, "g": torch.tensor([0.75], dtype=torch.float32)}


def override_rows(t, y):
    """the exact row edits both the reference and the device tensor get: row b % 4 == 1 an exact one-hot, == 2 times 0.5, == 3 zero"""
    for b in range(t.shape[0]):
        kind = ROW_KINDS[b % 4]
        if kind == "one_hot":
            t[b] = 0
            t[b, int(y[b])] = 1
        elif kind == "half":
            t[b] *= 0.5
        elif kind == "zero":
            t[b] = 0
    return t


def _dense(y, C, on, off, dt):
    t = torch.full((y.shape[0], C), off, dtype=dt)
    t[torch.arange(y.shape[0]), y] = on
    return t


def bounds(I, dtype):
    """-> (ref, bound) dicts over 't' [B, C], 'loss' [1] and 'dz' [B, C] at slack 1"""
    uT = u_of(dtype)
    z = I["z"].double()
    B, C = z.shape
    g = float(I["g"])
    a = _dense(I["y"], C, I["on"], I["off"], torch.float64) * I["ws"].double().view(-1, 1)
    b = _dense(I["y"].flip(0), C, I["on"], I["off"], torch.float64) * I["wo"].double().view(-1, 1)
    t = a + b
    e_t = U * (a.abs() + b.abs() + t.abs())
    scale = torch.tensor([{"mixed": 1.0, "half": 0.5}.get(ROW_KINDS[r % 4], 0.0) for r in range(B)], dtype=torch.float64).view(-1, 1)
    t, e_t = override_rows(t, I["y"]), e_t * scale
    blk = (C / 256 + 12) * U
    mx = z.max(1, keepdim=True).values
    v = z - mx
    lser = torch.logsumexp(v, 1, keepdim=True)
    p = torch.exp(v - lser)
    e_lser = U * ((p * (v.abs() + 3)).sum(1, keepdim=True) + C / 256 + 12 + 2 * lser.abs())
    St = t.sum(1, keepdim=True)
    e_St = e_t.sum(1, keepdim=True) + blk * t.abs().sum(1, keepdim=True)
    tv = t * v
    e_Stz = (e_t * v.abs() + 2 * U * tv.abs()).sum(1, keepdim=True) + blk * tv.abs().sum(1, keepdim=True)
    row = lser * St - tv.sum(1, keepdim=True)
    e_row = e_lser * St.abs() + lser.abs() * e_St + U * (lser * St).abs() + e_Stz + U * row.abs()
    loss = row.sum() / B
    e_loss = (e_row.sum() + (B + 2) * U * row.abs().sum()) / B + 3 * U * loss.abs()
    lse = mx + lser
    e_lse = e_lser + U * (2 * lse.abs() + 2 * mx.abs())
    e_p = p * (e_lse + U * (z - lse).abs() + 4 * U)
    k = g / B
    term = p * St - t
    dz = k * term
    e_dz = abs(k) * (e_p * St.abs() + p * e_St + U * (p * St).abs() + e_t + U * term.abs()) + (3 * U + uT) * dz.abs() + 2 * abs(k) * 2.0 ** -126
    return {"t": t, "loss": loss.reshape(1), "dz": dz}, {"t": e_t + 2.0 ** -149, "loss": e_loss.reshape(1), "dz": e_dz}


def ratios(out, ref, bnd):
    return {k: excess(out[k], ref[k], bnd[k] * SLACK)[0] for k in out}


def emulate(I, dtype, mutant=None):
    """The kernels' arithmetic in torch CPU float32 with the output rounding of dz.  `mutant`: one of MUTANTS:
      sum_t_assumed_one       the loss and the gradient take sum_c t = 1
      mean_over_classes       the loss is divided by B * C
      partner_not_flipped     the second one-hot reads y_b, not y_{B-1-b}
      smoothing_dropped       the target is built with on = 1, off = 0
      grad_without_1_over_B   dz is not divided by B"""
    z = I["z"].float()
    B, C = z.shape
    g = I["g"].float()[0]
    on, off = (1.0, 0.0) if mutant == "smoothing_dropped" else (I["on"], I["off"])
    y2 = I["y"] if mutant == "partner_not_flipped" else I["y"].flip(0)
    t = _dense(I["y"], C, on, off, torch.float32) * I["ws"].view(-1, 1) + _dense(y2, C, on, off, torch.float32) * I["wo"].view(-1, 1)
    t = override_rows(t, I["y"])
    mx = z.max(1, keepdim=True).values
    v = z - mx
    s = torch.exp(v).sum(1, keepdim=True)
    St = torch.ones((B, 1)) if mutant == "sum_t_assumed_one" else t.sum(1, keepdim=True)
    row = torch.log(s) * St - (t * v).sum(1, keepdim=True)
    div = float(B * C) if mutant == "mean_over_classes" else float(B)
    loss = row.sum() / div
    lse = mx + torch.log(s)
    k = g if mutant == "grad_without_1_over_B" else g / div
    return {"t": t, "loss": loss.reshape(1), "dz": (k * (torch.exp(z - lse) * St - t)).to(dtype).float()}
