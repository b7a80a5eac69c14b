"""Per-element error bounds against float64 for the fused head region of the downstream model (devias_fusion_head_fwd / _bwd) and the label-smoothing
cross-entropy (devias_softmax_ce_fwd / _bwd): csrc/fusion_head.hip.

A sibling of kernel_bounds.py / slot_loss_bounds.py (same rules, same measure: excess(out, ref, bound) = max |out - ref| / bound, a test asserts <= 1): a plain
helper module, torch arithmetic in float64 on the CPU.  u_T is the unit of the storage dtype (kernel_bounds.u_of), u = U_FP32; e_x is the bound carried by x.
Inputs are exact in both dtypes: the slots, the three weight matrices (generated on bf16's grid: the kernels' bf16 copies of the fp32 masters are then exact) and
the fp32 vectors.  A sum of n fp32 addends carries (n + 8) u in a GEMM (kernel_bounds' form) and (n / 256 + 12) u in a 256-thread block sum.

Forward (fusion_head.hip; one workgroup per row, statistics two-pass in fp32)
    gather + LN (fusion_gather_ln_fwd_kernel; n = D, eps 1e-6; also both LayerNorms of the middle chain, n = D / 2 and D, eps 1e-5)
        m    = sum x / n                              e_m    = (n / 256 + 12) u mean|x| + mean e_x
        d    = x - m                                  e_d    = e_x + e_m + u (|x| + |m|)            -- ABSOLUTE: a common offset of the row (m >> sigma) is held to u |m|
        rs   = rsqrt(sum d^2 / n + eps)               rho    = (n / 256 + 16) u + rs^2 mean(|d| e_d)  (relative; d rs / rs = -rs^2 mean(d delta))
        y    = d rs g + b                             e_y    = |g| (rs e_d + |xhat| rho) + 4 u (|g xhat| + |b|)
        input is stored in T                          e_in   = e_y + u_T |y|
    down projection, 2B rows (small-M GEMM)           e_u    = |Wd| e_in + (D + 8) u (|Wd| |in| + |bd|) + u_T |u|          (u is stored in T)
    middle chain (fusion_mid_fwd_kernel)              two half-row LNs on u (e_x = e_u), the input LN on their concatenation (e_x = e_h), nothing rounded to T between them
        r    = relu(h) mask                           e_r    = mask e_h + u_T |r| + 2 u |r|        (|relu(a) - relu(b)| <= |a - b|: a flipped sign costs no more than e_h)
    classifier                                        e_out  = |Wc| e_r + (D + 8) u (|Wc| |r| + |bc|) + u_T |out|
    idx is asserted EQUAL (the generators plant the selection with a gap >= MATCH_MARGIN on the float64 reference; the fp32 softmax statistics carry ~1e-6).
Backward (on the SAVED forward: the float64 reference takes the ReLU mask from the kernel's stored r and idx from the stored idx; every other quantity of the reference
is float64 from the slots, so the forward's e_* enter wherever the kernel re-reads a stored tensor)
    classifier        dWc = dout^T r                  |dout|^T e_r + (B + 8) u |dout|^T |r| ;   dbc: (B + 8) u sum|dout|
                      dr  = dout Wc                   e_dr   = (Cd + 8) u |dout| |Wc| + u_T |dr|                            (stored in T)
    middle chain (fusion_mid_bwd_kernel)   g = dr mask [r > 0]:  e_g = mask e_dr + 2 u |g|
        LN backward, gy = g gamma, c1 = mean gy, c2 = mean(gy xh), dx = rs (gy - c1 - xh c2), with the forward's xh carrying e_xh = rs e_d + |xh| rho:
                      e_dx = rs (|gamma| e_g + mean(|gamma| e_g) + |xh| mean(|xh gamma| e_g))         the incoming gradient's error through the (linear) map
                           + rs (e_xh mean|gy xh| + |xh| mean(|gy| e_xh))                             the map's own error: xh
                           + (rho + (n / 256 + 16) u) rs (|gy| + mean|gy| + |xh| mean|gy xh|)         rs and the two block sums -- sums of ABSOLUTE terms
        parameter gradients, per clip then over the clips in index order:
                      d gamma = sum_b g xh            sum_b (e_g |xh| + |g| e_xh) + (rows + 4) u sum_b |g xh| ;   d beta = sum_b g: sum_b e_g + (rows + 4) u sum_b |g|
        the input LN (when used) and then the two half-row LNs (rows = 2B for their shared parameter pair);  du is stored in T: + u_T |du|
    down projection   dWd = du^T in                   |du|^T e_in + e_du^T |in| + (2B + 8) u |du|^T |in| ;   dbd: sum e_du + (2B + 8) u sum|du|
                      dinp = du Wd (+ dinput)         e_dinp = e_du |Wd| + (D / 2 + 8) u |du| |Wd| + u_T |dinp|             (stored in T)
    gather backward (fusion_gather_ln_bwd_kernel)     the LN backward above with e_g = e_dinp and e_x = 0, summed over the (up to two) picks of a slot row in fp32,
                      one rounding: + u_T |dslots|;  rows no pick selects are asserted EXACTLY zero.
Cross-entropy (softmax_ce_*_kernel; row_stats of loss.hip)
    lse = mx + logf(sum expf(z - mx))                 e_lse  = u (sum_c p_c (|z_c - mx| + 3) + C / 256 + 12 + 2 |lse - mx|)      (relative to mx: the kernel never adds mx back)
    row = (1 - e)(lse - z_y) + e (lse - mean z)       e_row  = e_lse + u ((C / 256 + 14) mean|z - mx| + 4 (|z_y - mx| + |lse - mx|)) ;  loss = mean_b: + (B + 2) u mean|row|
    dz  = g / B (p_c - (1 - e)[c = y] - e / C)        |g| / B (p_c (e_lse' + u |z_c - lse| + 4 u) + 3 u (p_c + 1[c = y] + e / C)) + u_T |dz|,  e_lse' = e_lse + 2 u |lse|
                                                      -- ABSOLUTE in p_c, so p_y -> 1 (a peaked row: p_y - (1 - e) cancels) is handled

Slacks.  Each bound holds first-order arguments and device transcendentals and carries ONE scalar slack, set to twice what the CPU emulation (emulate() below: the
float64 reference's formulas with exactly the kernel's roundings, in torch CPU float32 arithmetic; tests/test_fusion_bounds_cpu.py prints the ratios) needs to stay
at 1 over all generators, both dtypes, use_input_ln on and off, mask absent and 50 %.  Never fitted to the HIP kernel.

    bound              slack       emulation's worst ratio at slack 1 (test_fusion_bounds_cpu.py prints them)
    forward            2 x 0.995   bf16 0.9950 (input: the store alone -- u_T = 2^-8 is the largest relative error of a bf16 rounding);  fp32 0.095 (input)
    backward           2 x 0.981   bf16 0.9804 (d fc_input_ln.bias at B = 1: the store of dr alone), dslots 0.006;  fp32 0.112 (d classifier.bias), dslots 1e-5
    cross-entropy      2 x 0.992   bf16 dz 0.9918 (the store), loss 0.052;  fp32 dz 0.537, loss 0.069
The activation bounds of the backward are one to two orders above the emulation in bf16 (more in fp32): every GEMM and LayerNorm behind a bf16 store carries that
store's error as a sum of ABSOLUTE terms (|W| e, mean(|gamma| e)), as kernel_bounds.py states the GEMM's.  What they still tell apart is what the mutants show:
eps_swap 808 (on 'faint'), scene_down 410, no_sum 2.8 (on 'collide'), no_drop_scale 4e4, ln_full 29, no_smooth_term > 1 at every C -- all in fp32.

Generators (GENERATORS, head_inputs) say in their docstrings which failure each makes visible.  Mutants (emulate(mutant=...), MUTANTS) must exceed 1.
"""
import math

import torch
import torch.nn.functional as F

import downstream_ref as dr
from kernel_bounds import U_FP32, _randn, excess, u_of  # noqa: F401

SLACK_FWD = 2 * 0.995       # the emulation needs 0.9950
SLACK_BWD = 2 * 0.981       # the emulation needs 0.9804
SLACK_CE = 2 * 0.992        # the emulation needs 0.9918
MATCH_MARGIN = 0.05
GENERATORS = ("diffuse", "offset", "collide", "last", "dead", "faint")
MUTANTS = ("eps_swap", "scene_down", "no_sum", "no_smooth_term", "no_drop_scale", "ln_full")
U = U_FP32
f = "fusion_head."
GRAD_NAMES = ("action_norm.weight", "action_norm.bias", "scene_norm.weight", "scene_norm.bias", f + "fc_action_down.weight", f + "fc_action_down.bias",
              f + "fc_action_ln.weight", f + "fc_action_ln.bias", f + "fc_input_ln.weight", f + "fc_input_ln.bias", f + "classifier.weight", f + "classifier.bias")


# ------------------------------------------------------------------------------------------------ generators
def _bf16_grid(t):
    return t.bfloat16().float()


def make_params(D, nb, ns, Cd, use_input_ln=True, seed=0):
    """fp32 parameters under the reference's names.  The three matrices lie on bf16's grid.  head.weight is small noise except two planted rows (class 0 of the
    action range, class nb of the scene range) along two orthogonal sign patterns: head_inputs moves a slot along one of them to plant a pick."""
    Dh = D // 2
    P = {}
    hw = _randn((nb + ns, D), seed + 1, "cpu") * 0.01
    hw = hw - hw.mean(1, keepdim=True)          # (rows without a constant component: a common offset of the slots moves no logit)
    va, vs = sign_patterns(D)
    hw[0] = va * (8.0 / D)
    hw[nb] = vs * (8.0 / D)
    P["head.weight"] = _bf16_grid(hw)
    P["head.bias"] = _randn((nb + ns,), seed + 2, "cpu") * 0.01
    for i, n in enumerate(("action_norm", "scene_norm")):
        P[n + ".weight"] = 1.0 + 0.25 * _randn((D,), seed + 3 + i, "cpu")
        P[n + ".bias"] = 0.1 * _randn((D,), seed + 5 + i, "cpu")
    for i, n in enumerate(("fc_action", "fc_scene")):
        P[f + n + "_down.weight"] = _bf16_grid(_randn((Dh, D), seed + 7 + i, "cpu") * (0.3 / math.sqrt(D)))
        P[f + n + "_down.bias"] = 0.05 * _randn((Dh,), seed + 9 + i, "cpu")
        P[f + n + "_ln.weight"] = 1.0 + 0.25 * _randn((Dh,), seed + 11 + i, "cpu")
        P[f + n + "_ln.bias"] = 0.1 * _randn((Dh,), seed + 13 + i, "cpu")
    if use_input_ln:
        P[f + "fc_input_ln.weight"] = 1.0 + 0.25 * _randn((D,), seed + 15, "cpu")
        P[f + "fc_input_ln.bias"] = 0.1 * _randn((D,), seed + 16, "cpu")
    P[f + "classifier.weight"] = _bf16_grid(_randn((Cd, D), seed + 17, "cpu") * 0.05)
    P[f + "classifier.bias"] = 0.05 * _randn((Cd,), seed + 18, "cpu")
    return P


def sign_patterns(D):
    k = torch.arange(D)
    return (1.0 - 2.0 * (k % 2)).float(), (1.0 - 2.0 * ((k // 2) % 2)).float()


def head_inputs(kind, B, S, D, dtype, P, seed=0):
    """slots [B, S, D] in `dtype`, a copy of P (its last LayerNorm bias shifted by + 1, except for 'dead'), dout [B, Cd] and dinput [B, 2D] in `dtype`, and the
    planted picks [B, 2].
      diffuse   slots ~ 0.5 randn, picks spread over the slots (clip b: slots b mod S and (b + 1) mod S): a wrong row, parameter set, half or scale shows at its own size
      offset    every slot row carries a common offset of 30: m >> sigma, the mean subtraction cancels -- a one-pass variance or a bf16 statistic shows
      collide   ia = is on odd clips: the backward must SUM the two gradients into one row (and round once)
      last      both picks are slot S - 1 / S - 2: an off-by-one in the gather or the scatter's row index shows
      dead      about half of h is negative (the other generators shift the last LayerNorm's bias by + 1: about 85 % positive): the ReLU mask carries the gradient
      faint     slots ~ 2^-6 randn, planted with 2^-5: the picked rows' variance is ~1e-3, where the LayerNorm's eps is 1e-3 of it -- 1e-5 in place of 1e-6 shows
                (the planted logit is 0.25: the relative gap to the runner-up is still ~0.19)
    The pick is planted by moving the chosen slot by +-2 along head.weight's planted rows (a logit 16 above the noise): the gap to the runner-up slot is >= MATCH_MARGIN
    on the float64 reference (asserted by both test files through selection_gap)."""
    x = _randn((B, S, D), seed + 21, "cpu") * (2.0 ** -6 if kind == "faint" else 0.5)
    amp = 2.0 ** -5 if kind == "faint" else 2.0
    if kind == "offset":
        x = x + 30.0
    va, vs = sign_patterns(D)
    picks = torch.zeros((B, 2), dtype=torch.int64)
    for b in range(B):
        if kind == "last":
            ia, is_ = S - 1, max(S - 2, 0)
        elif kind == "collide" and b % 2 == 1:
            ia = is_ = (b // 2) % S
        else:
            ia, is_ = b % S, (b + 1) % S
        picks[b, 0], picks[b, 1] = ia, is_
        x[b, ia] += amp * va
        x[b, is_] += amp * vs
    P = dict(P)
    if kind != "dead":          # the last LayerNorm's bias + 1: about 85 % of h is positive; 'dead' keeps the centred bias (about half)
        last = f + ("fc_input_ln.bias" if f + "fc_input_ln.bias" in P else "fc_action_ln.bias")
        P[last] = P[last] + 1.0
    Cd = P[f + "classifier.weight"].shape[0]
    dout = (_randn((B, Cd), seed + 22, "cpu") * 0.05).to(dtype)
    dinp = (_randn((B, 2 * D), seed + 23, "cpu") * 0.01).to(dtype)
    return x.to(dtype), P, dout, dinp, picks


def drop_mask(B, D, keep, seed=0):
    g = torch.Generator().manual_seed(seed + 31)
    return ((torch.rand((B, D), generator=g) < keep).float() / keep).contiguous()


def selection_gap(slots, P, nb):
    """(idx [B, 2], min relative gap) of the float64 reference's selection"""
    B, S, D = slots.shape
    Z = F.linear(slots.double().reshape(B * S, D), P["head.weight"].double(), P["head.bias"].double())
    idx, gaps = dr.select(Z, B, S, nb)
    return idx, float(gaps.min())


# ------------------------------------------------------------------------------------------------ float64 reference
def reference(slots, P, nb, use_input_ln, mask, dout, dinp, idx=None, relu_mask=None):
    """float64 forward and backward of the head region -> dict(input, out, idx, dslots, grads{name}, inter) with `inter` the intermediates the bounds need"""
    P64 = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    x = slots.double().clone().requires_grad_(True)
    o = dr.fusion_forward(x, P64, nb, use_input_ln, mask.double() if mask is not None else None, idx=idx, relu_mask=relu_mask)
    seed = (o["out"] * dout.double()).sum()
    if dinp is not None:
        seed = seed + (o["input"] * dinp.double()).sum()
    seed.backward()
    grads = {n: P64[n].grad for n in GRAD_NAMES if n in P64}
    none = [n for n in dr.NO_GRAD_NAMES if P64[n].grad is not None]
    assert not none, none
    return {"input": o["input"].detach(), "out": o["out"].detach(), "idx": o["idx"], "dslots": x.grad, "grads": grads, "u": o["u"].detach(), "r": o["r"].detach()}


# ------------------------------------------------------------------------------------------------ bounds
def _ln_fwd(x, e_x, g, b, eps, n):
    """float64 LayerNorm of the last axis with the docstring's error terms -> (y, e_y, aux) ; aux = (xh, e_xh, rs, rho) for the backward"""
    m = x.mean(-1, keepdim=True)
    e_m = (n / 256 + 12) * U * x.abs().mean(-1, keepdim=True) + e_x.mean(-1, keepdim=True)
    d = x - m
    e_d = e_x + e_m + U * (x.abs() + m.abs())
    rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    rho = (n / 256 + 16) * U + rs * rs * (d.abs() * e_d).mean(-1, keepdim=True)
    xh = d * rs
    e_xh = rs * e_d + xh.abs() * rho
    y = xh * g + b
    e_y = g.abs() * e_xh + 4 * U * ((g * xh).abs() + b.abs())
    return y, e_y, (xh, e_xh, rs, rho)


def _ln_bwd(gin, e_g, g, aux, n):
    """LayerNorm backward with the docstring's error terms -> (dx, e_dx, (dgamma_terms, e), (dbeta_terms, e)) ; the parameter terms are per row (the caller sums rows)"""
    xh, e_xh, rs, rho = aux
    gy = gin * g
    mean = lambda t: t.mean(-1, keepdim=True)      # noqa: E731
    c1, c2 = mean(gy), mean(gy * xh)
    dx = rs * (gy - c1 - xh * c2)
    ge = g.abs() * e_g
    e_dx = rs * (ge + mean(ge) + xh.abs() * mean(xh.abs() * ge)) \
        + rs * (e_xh * mean((gy * xh).abs()) + xh.abs() * mean(gy.abs() * e_xh)) \
        + (rho + (n / 256 + 16) * U) * rs * (gy.abs() + mean(gy.abs()) + xh.abs() * mean((gy * xh).abs()))
    return dx, e_dx, (gin * xh, e_g * xh.abs() + gin.abs() * e_xh), (gin, e_g)


def _rowsum(terms, e, rows):
    t = terms.reshape(rows, -1)
    return e.reshape(rows, -1).sum(0) + (rows + 4) * U * t.abs().sum(0)


def bounds(slots, P, nb, use_input_ln, mask, dout, dinp, idx, relu_mask, dtype):
    """-> (ref, bound) dicts over 'input', 'out', 'dslots' and the GRAD_NAMES present, at slack 1 (the tests multiply by SLACK_FWD / SLACK_BWD).  The float64 values are
    recomputed stage by stage here (and checked against reference()'s autograd in test_fusion_bounds_cpu.py)."""
    uT = u_of(dtype)
    B, S, D = slots.shape
    Dh = D // 2
    P = {k: v.double() for k, v in P.items()}
    x = slots.double()
    ar = torch.arange(B)
    mk = mask.double() if mask is not None else torch.ones((B, D), dtype=torch.float64)
    rows = torch.stack([x[ar, idx[:, 0].long()], x[ar, idx[:, 1].long()]], dim=1)                      # [B, 2, D]
    gN = torch.stack([P["action_norm.weight"], P["scene_norm.weight"]])[None]
    bN = torch.stack([P["action_norm.bias"], P["scene_norm.bias"]])[None]
    y, e_y, auxN = _ln_fwd(rows, torch.zeros_like(rows), gN, bN, dr.EPS_NORM, D)
    e_in = e_y + uT * y.abs()
    Wd, bd = P[f + "fc_action_down.weight"], P[f + "fc_action_down.bias"]
    u = y @ Wd.t() + bd                                                                                 # [B, 2, Dh]
    e_u = e_in @ Wd.abs().t() + (D + 8) * U * (y.abs() @ Wd.abs().t() + bd.abs()) + uT * u.abs()
    gl, bl = P[f + "fc_action_ln.weight"], P[f + "fc_action_ln.bias"]
    h, e_h, auxH = _ln_fwd(u, e_u, gl, bl, dr.EPS_LN, Dh)
    h, e_h = h.reshape(B, D), e_h.reshape(B, D)
    if use_input_ln:
        gi, bi = P[f + "fc_input_ln.weight"], P[f + "fc_input_ln.bias"]
        h2, e_h2, auxI = _ln_fwd(h, e_h, gi, bi, dr.EPS_LN, D)
    else:
        h2, e_h2 = h, e_h
    r = torch.relu(h2) * mk
    e_r = mk * e_h2 + (uT + 2 * U) * r.abs()
    Wc, bc = P[f + "classifier.weight"], P[f + "classifier.bias"]
    out = r @ Wc.t() + bc
    e_out = e_r @ Wc.abs().t() + (D + 8) * U * (r.abs() @ Wc.abs().t() + bc.abs()) + uT * out.abs()
    ref = {"input": y.reshape(B, 2 * D), "out": out}
    bnd = {"input": e_in.reshape(B, 2 * D), "out": e_out}
    # ---- backward on the saved forward's ReLU mask
    do = dout.double()
    rm = relu_mask.double() if relu_mask is not None else (h2 > 0).double()
    rb = h2 * rm * mk                                                                                    # the reference's r under that mask
    ref[f + "classifier.weight"] = do.t() @ rb
    bnd[f + "classifier.weight"] = do.abs().t() @ e_r + (B + 8) * U * (do.abs().t() @ rb.abs())
    ref[f + "classifier.bias"] = do.sum(0)
    bnd[f + "classifier.bias"] = (B + 8) * U * do.abs().sum(0)
    d_r = do @ Wc
    e_dr = (Wc.shape[0] + 8) * U * (do.abs() @ Wc.abs()) + uT * d_r.abs()
    g = d_r * mk * rm
    e_g = mk * rm * e_dr + 2 * U * g.abs()
    if use_input_ln:
        g2, e_g2, (tw, ew), (tb, eb) = _ln_bwd(g, e_g, gi, auxI, D)
        ref[f + "fc_input_ln.weight"], bnd[f + "fc_input_ln.weight"] = tw.sum(0), _rowsum(tw, ew, B)
        ref[f + "fc_input_ln.bias"], bnd[f + "fc_input_ln.bias"] = tb.sum(0), _rowsum(tb, eb, B)
    else:
        g2, e_g2 = g, e_g
    du, e_du, (tw, ew), (tb, eb) = _ln_bwd(g2.reshape(B, 2, Dh), e_g2.reshape(B, 2, Dh), gl, auxH, Dh)
    ref[f + "fc_action_ln.weight"], bnd[f + "fc_action_ln.weight"] = tw.reshape(2 * B, Dh).sum(0), _rowsum(tw, ew, 2 * B)
    ref[f + "fc_action_ln.bias"], bnd[f + "fc_action_ln.bias"] = tb.reshape(2 * B, Dh).sum(0), _rowsum(tb, eb, 2 * B)
    e_du = e_du + uT * du.abs()
    du2, e_du2, y2, e_in2 = du.reshape(2 * B, Dh), e_du.reshape(2 * B, Dh), y.reshape(2 * B, D), e_in.reshape(2 * B, D)
    ref[f + "fc_action_down.weight"] = du2.t() @ y2
    bnd[f + "fc_action_down.weight"] = du2.abs().t() @ e_in2 + e_du2.t() @ y2.abs() + (2 * B + 8) * U * (du2.abs().t() @ y2.abs())
    ref[f + "fc_action_down.bias"] = du2.sum(0)
    bnd[f + "fc_action_down.bias"] = e_du2.sum(0) + (2 * B + 8) * U * du2.abs().sum(0)
    dy = du @ Wd                                                                                        # [B, 2, D]
    e_dy = e_du @ Wd.abs() + (Dh + 8) * U * (du.abs() @ Wd.abs())
    if dinp is not None:
        di = dinp.double().reshape(B, 2, D)
        e_dy = e_dy + 2 * U * (dy.abs() + di.abs())
        dy = dy + di
    e_dy = e_dy + uT * dy.abs()
    dxr, e_dxr, (tw, ew), (tb, eb) = _ln_bwd(dy, e_dy, gN, auxN, D)
    for t, n in enumerate(("action_norm", "scene_norm")):
        ref[n + ".weight"], bnd[n + ".weight"] = tw[:, t].sum(0), _rowsum(tw[:, t], ew[:, t], B)
        ref[n + ".bias"], bnd[n + ".bias"] = tb[:, t].sum(0), _rowsum(tb[:, t], eb[:, t], B)
    dx, e_dx = torch.zeros_like(x), torch.zeros_like(x)
    for t in range(2):
        dx.index_put_((ar, idx[:, t].long()), dxr[:, t], accumulate=True)
        e_dx.index_put_((ar, idx[:, t].long()), e_dxr[:, t], accumulate=True)
    ref["dslots"] = dx
    bnd["dslots"] = e_dx + (uT + 2 * U) * dx.abs()
    return ref, bnd


def ce_inputs(C, B, kind, dtype, seed=0):
    """logits ~ 2 randn [B, C] and targets; kind 'last': every target is C - 1 (the row's last element); 'peaked': the target's logit is 30 (p_y -> 1, p_y - (1 - e) cancels)"""
    z = _randn((B, C), seed + 41, "cpu") * 2.0
    y = torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed + 42))
    if kind == "last":
        y[:] = C - 1
    if kind == "peaked":
        z[torch.arange(B), y] = 30.0
    return z.to(dtype), y


def ce_reference(z, y, eps, g=1.0):
    z64 = z.double().clone().requires_grad_(True)
    loss = dr.label_smoothing_ce(z64, y, eps)
    (loss * g).backward()
    return loss.detach(), z64.grad


def ce_bounds(z, y, eps, g, dtype):
    """-> (loss bound, dz bound) at slack 1"""
    uT = u_of(dtype)
    z = z.double()
    B, C = z.shape
    mx = z.max(-1, keepdim=True).values
    lse = torch.logsumexp(z, -1, keepdim=True)
    p = torch.exp(z - lse)
    e_lse = U * ((p * ((z - mx).abs() + 3)).sum(-1, keepdim=True) + C / 256 + 12 + 2 * (lse - mx).abs())
    zy = z.gather(1, y.view(-1, 1))
    e_row = e_lse + U * ((C / 256 + 14) * (z - mx).abs().mean(-1, keepdim=True) + 4 * ((zy - mx).abs() + (lse - mx).abs()))
    row = (1 - eps) * (lse - zy) + eps * (lse - z.mean(-1, keepdim=True))
    b_loss = e_row.mean() + (B + 2) * U * row.abs().mean()
    onehot = F.one_hot(y, C).double()
    dz = abs(g) / B * (p - (1 - eps) * onehot - eps / C)
    e_l2 = e_lse + 2 * U * lse.abs()
    b_dz = abs(g) / B * (p * (e_l2 + U * (z - lse).abs() + 4 * U) + 3 * U * (p + onehot + eps / C)) + uT * dz.abs()
    return b_loss, b_dz


# ------------------------------------------------------------------------------------------------ CPU emulation of the kernels
def _rt(t, dtype):
    return t.to(dtype).float()


def _e_ln(x, g, b, eps):
    m = x.mean(-1, keepdim=True)
    d = x - m
    rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rs * g + b, d * rs, rs


def _e_ln_bwd(gin, g, xh, rs):
    gy = gin * g
    c1, c2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    return rs * (gy - c1 - xh * c2)


def emulate(slots, P, nb, use_input_ln, mask, dout, dinp, dtype, mutant=None):
    """The kernels' arithmetic transcribed to torch CPU float32, with exactly their roundings to `dtype` (input, u, r, out; dr, du, dinp, dslots).  `mutant`: one of
    MUTANTS -- a seeded fault the bounds must catch."""
    B, S, D = slots.shape
    Dh = D // 2
    Pf = {k: v.float() for k, v in P.items()}
    x = slots.float()
    eps_n, eps_l = (dr.EPS_LN, dr.EPS_NORM) if mutant == "eps_swap" else (dr.EPS_NORM, dr.EPS_LN)
    Z = _rt(F.linear(x.reshape(B * S, D), Pf["head.weight"], Pf["head.bias"]), dtype)
    idx, _ = dr.select(Z, B, S, nb)
    ar = torch.arange(B)
    rows = torch.stack([x[ar, idx[:, 0]], x[ar, idx[:, 1]]], dim=1)
    gN = torch.stack([Pf["action_norm.weight"], Pf["scene_norm.weight"]])[None]
    bN = torch.stack([Pf["action_norm.bias"], Pf["scene_norm.bias"]])[None]
    y, xhN, rsN = _e_ln(rows, gN, bN, eps_n)
    y = _rt(y, dtype)                                                                                   # input
    Wd, bd = Pf[f + "fc_action_down.weight"], Pf[f + "fc_action_down.bias"]
    u = y @ Wd.t() + bd
    if mutant == "scene_down":
        u = torch.stack([u[:, 0], y[:, 1] @ Pf[f + "fc_scene_down.weight"].t() + Pf[f + "fc_scene_down.bias"]], dim=1)
    u = _rt(u, dtype)
    gl, bl = Pf[f + "fc_action_ln.weight"], Pf[f + "fc_action_ln.bias"]
    if mutant == "ln_full":
        h, xhH, rsH = _e_ln(u.reshape(B, 1, D), torch.cat([gl, gl]), torch.cat([bl, bl]), eps_l)
        h = h.reshape(B, D)
    else:
        h, xhH, rsH = _e_ln(u, gl, bl, eps_l)
        h = h.reshape(B, D)
    if use_input_ln:
        gi, bi = Pf[f + "fc_input_ln.weight"], Pf[f + "fc_input_ln.bias"]
        h2, xhI, rsI = _e_ln(h, gi, bi, eps_l)
    else:
        h2 = h
    mk = mask.float() if mask is not None else None
    if mk is not None and mutant == "no_drop_scale":
        mk = (mk > 0).float()
    r = torch.relu(h2)
    if mk is not None:
        r = r * mk
    r = _rt(r, dtype)
    Wc, bc = Pf[f + "classifier.weight"], Pf[f + "classifier.bias"]
    out = _rt(r @ Wc.t() + bc, dtype)
    # backward
    do = dout.float()
    G = {f + "classifier.weight": do.t() @ r, f + "classifier.bias": do.sum(0)}
    d_r = _rt(do @ Wc, dtype)
    g = torch.where(r > 0, d_r, torch.zeros_like(d_r))
    if mk is not None:
        g = g * mk
    if use_input_ln:
        G[f + "fc_input_ln.weight"], G[f + "fc_input_ln.bias"] = (g * xhI).sum(0), g.sum(0)
        g = _e_ln_bwd(g, gi, xhI, rsI)
    if mutant == "ln_full":
        gg = g.reshape(B, 1, D)
        G[f + "fc_action_ln.weight"] = (gg * xhH).reshape(2 * B, Dh).sum(0)
        G[f + "fc_action_ln.bias"] = g.reshape(2 * B, Dh).sum(0)
        du = _e_ln_bwd(gg, torch.cat([gl, gl]), xhH, rsH).reshape(B, 2, Dh)
    else:
        gg = g.reshape(B, 2, Dh)
        G[f + "fc_action_ln.weight"] = (gg * xhH).reshape(2 * B, Dh).sum(0)
        G[f + "fc_action_ln.bias"] = gg.reshape(2 * B, Dh).sum(0)
        du = _e_ln_bwd(gg, gl, xhH, rsH)
    du = _rt(du, dtype)
    G[f + "fc_action_down.weight"] = du.reshape(2 * B, Dh).t() @ y.reshape(2 * B, D)
    G[f + "fc_action_down.bias"] = du.reshape(2 * B, Dh).sum(0)
    dy = du @ Wd
    if dinp is not None:
        dy = dy + dinp.float().reshape(B, 2, D)
    dy = _rt(dy, dtype)
    for t, n in enumerate(("action_norm", "scene_norm")):
        G[n + ".weight"], G[n + ".bias"] = (dy[:, t] * xhN[:, t]).sum(0), dy[:, t].sum(0)
    dxr = _e_ln_bwd(dy, gN, xhN, rsN)
    dx = torch.zeros_like(x)
    for t in range(2):
        if mutant == "no_sum":
            dx[ar, idx[:, t]] = dxr[:, t]
        else:
            dx.index_put_((ar, idx[:, t]), dxr[:, t], accumulate=True)
    dx = _rt(dx, dtype)
    return {"input": y.reshape(B, 2 * D), "out": out, "idx": idx, "dslots": dx, "grads": G, "r": r}


def emulate_ce(z, y, eps, g, dtype, mutant=None):
    """the cross-entropy kernels in torch CPU float32 -> (loss, dz rounded to `dtype`)"""
    z = z.float()
    B, C = z.shape
    mx = z.max(-1, keepdim=True).values
    lse = torch.log(torch.exp(z - mx).sum(-1, keepdim=True))
    zm = (z - mx).mean(-1, keepdim=True)
    zy = z.gather(1, y.view(-1, 1)) - mx
    row = (1 - eps) * (lse - zy) + eps * (lse - zm)
    loss = row.sum() / B
    p = torch.exp(z - (mx + lse))
    off = 0.0 if mutant == "no_smooth_term" else eps / C
    dz = (g / B) * (p - (1 - eps) * F.one_hot(y, C).float() - off)
    return loss, _rt(dz, dtype)
