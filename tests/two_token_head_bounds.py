"""Per-element error bounds against float64 for the two-token head region of the multi-task baseline (devias_two_token_head_fwd / _bwd): csrc/two_token_head.hip.

A sibling of pool_head_bounds.py (same rules, same measure: excess(out, ref, bound) = max |out - ref| / bound, a test asserts <= 1; the LayerNorm forward / backward
terms of fusion_bounds.py are imported, not restated).  u_T is the unit of the storage dtype, u = U_FP32, e_x the bound carried by x.  Inputs are exact in both
dtypes: h, the head weights (on bf16's grid), the fp32 vectors, the fp32 masks.

The 2B token rows are STACKED as the kernels stack them: row j < B is row 0 of clip j (action), row B + j is row Nt - 1 of clip j (scene).
Forward
    t = the stacked rows of h                        e_t = 0
    y = LN(t; gamma, beta, eps 1e-6), n = D          e_y: fusion_bounds._ln_fwd          (the one `norm` serves both halves)
    token = T(y)                                     e_token = e_y + u_T |y|
    a = T(y mask)  (each half its own mask, which meets the UNROUNDED y)      e_a = mask e_y + (u_T + 2 u) |y mask|      -- held on its own (the save arena), at SLACK_A
    logits_x = T(a_x Wx^T + bx)                      e_logits = |W| e_a + (D + 8) u (|W| |a| + |b|) + u_T |logits|     (unified: Wx = W, bx = b for both halves)
Backward (on the saved forward: a, x^ and rstd are re-read, so their e_* enter)
    separate heads   dWx = dlogits_x^T a_x: |dl|^T e_a + (B + 8) u |dl|^T |a| ;   dbx = column sums: (B + 8) u sum|dl|
    unified head     ONE dW / db over the 2B stacked rows: the same terms with 2B for B
    da = dlogits W  (fp32)    e_da = (C + 8) u |dl| |W|
    g = da mask + dtoken      e_g = mask e_da + 3 u (|da mask| + |dtoken|)
    LayerNorm backward (fusion_bounds._ln_bwd) -> dt, e_dt;  d gamma = sum_j g x^, d beta = sum_j g over the 2B rows in a fixed order: fusion_bounds._rowsum
    rows 0 and Nt - 1 of each clip: dx = T(dt)   e_dx = e_dt + (u_T + 2 u) |dt| ;  every other row EXACTLY zero (bound 0)

Slacks.  SLACK_FWD / SLACK_BWD are twice what the CPU emulation (emulate(): the formulas above in torch CPU float32 with exactly the kernels' roundings) needs over
every generator, both dtypes, both head modes, masks absent and keep = 0.75, dtoken absent and present (tests/test_two_token_head_bounds_cpu.py prints the ratios
and asserts the emulation stays under HALF the slack).  SLACK_A = 1: the bound of `a` is one round-to-nearest of an fp32 value (|T(v) - v| <= u_T |v| holds without
slack) plus the LayerNorm's fp32 terms; only so can a second rounding (the mutant mask_after_round) show.  Never fitted to the HIP kernel.

Generators (GENERATORS) and mutants (MUTANTS): see inputs() and emulate().
"""
import torch

from fusion_bounds import _ln_bwd, _ln_fwd, _rowsum
from kernel_bounds import U_FP32, _randn, excess, graded, u_of  # noqa: F401

EPS = 1e-6
SLACK_FWD = 2 * 0.99        # the emulation needs 0.9896 (bf16 token: the store alone; logits 0.29; fp32: token 0.142, logits 0.010)
SLACK_BWD = 2 * 0.99        # the emulation needs 0.9890 (bf16 dWs at B = 1: the stored a alone; dx 0.974; fp32: dba 0.159, dWa 0.141, dbeta 0.101, dx 0.054)
SLACK_A = 1.0               # the emulation reaches 0.9951 in bf16 (0.166 in fp32)
KEEP = 0.75                 # 1 / keep is no power of two: T(T(y) / keep) differs from T(y / keep)
GENERATORS = ("graded", "tail", "offset")
MUTANTS = ("scene_row_nt2", "scene_row0", "dx_middle_nonzero", "unified_dw_missing_scene", "dgamma_missing_scene", "masks_swapped", "mask_after_round")
U = U_FP32


def _bf16_grid(t):
    return t.bfloat16().float()


def inputs(kind, B, Nt, D, Ca, Cs, dtype, unified, mask, dtok, seed=0):
    """-> dict(h [B, Nt, D] in dtype; Wa [Ca, D], Ws [Cs, D] fp32 on bf16's grid with their biases ba, bs -- unified: ONE head Wa [Ca + Cs, D], Ws = bs = None and both
    logits are Ca + Cs wide; gamma, beta fp32; mask_a, mask_s fp32 [B, D] or None; dlogits_a, dlogits_s and dtoken_a, dtoken_s (or None) in dtype)
      graded   token rows scaled by kernel_bounds.graded(Nt) (2^-6 ... 2^6, odd period 13): neighbouring rows differ in scale, so a wrong row shows in rstd and dx too
      tail     unit scale, the LAST token of every clip 64 times larger: rows Nt - 1 and Nt - 2 (and 0) are different vectors of different scale -- after the
               LayerNorm their tokens differ by O(1), far more than any bound, and their dx rows by a factor of 64
      offset   every row carries a common offset of 30 (m >> sigma in the LayerNorm): a one-pass variance or a statistic in T shows"""
    x = _randn((B, Nt, D), seed + 1, "cpu")
    if kind == "graded":
        x = x * graded(Nt).float()[None, :, None]
    elif kind == "tail":
        x[:, Nt - 1] *= 64.0
    elif kind == "offset":
        x = x + 30.0
    else:
        raise ValueError(kind)
    wa, ws = (Ca + Cs, Ca + Cs) if unified else (Ca, Cs)
    out = {"h": x.to(dtype), "unified": bool(unified),
           "Wa": _bf16_grid(_randn((wa, D), seed + 2, "cpu") * 0.05 * graded(wa, 3).float()[:, None]), "ba": 0.05 * _randn((wa,), seed + 3, "cpu"),
           "Ws": None, "bs": None,
           "gamma": torch.linspace(-1.0, 1.5, D) + 0.01 * _randn((D,), seed + 4, "cpu"), "beta": 0.1 * _randn((D,), seed + 5, "cpu"),
           "mask_a": None, "mask_s": None, "dtoken_a": None, "dtoken_s": None}
    if not unified:
        out["Ws"] = _bf16_grid(_randn((ws, D), seed + 12, "cpu") * 0.05 * graded(ws, 5).float()[:, None])
        out["bs"] = 0.05 * _randn((ws,), seed + 13, "cpu")
    if mask:
        g = torch.Generator().manual_seed(seed + 6)
        out["mask_a"] = ((torch.rand((B, D), generator=g) < KEEP).float() / KEEP).contiguous()
        out["mask_s"] = ((torch.rand((B, D), generator=g) < KEEP).float() / KEEP).contiguous()
    out["dlogits_a"] = (_randn((B, wa), seed + 7, "cpu") * 0.05 * graded(B, 2).float()[:, None]).to(dtype)
    out["dlogits_s"] = (_randn((B, ws), seed + 17, "cpu") * 0.05 * graded(B, 4).float()[:, None]).to(dtype)
    if dtok:
        out["dtoken_a"] = (_randn((B, D), seed + 8, "cpu") * 0.01).to(dtype)
        out["dtoken_s"] = (_randn((B, D), seed + 18, "cpu") * 0.01).to(dtype)
    return out


def _heads(I, cast):
    Wa, ba = cast(I["Wa"]), cast(I["ba"])
    return (Wa, ba, Wa, ba) if I["unified"] else (Wa, ba, cast(I["Ws"]), cast(I["bs"]))


# ------------------------------------------------------------------------------------------------ float64 reference (autograd)
def reference(I):
    """float64 autograd on the UNSTACKED form (norm over all rows, then rows 0 and -1) -> dict(token_a, token_s, a, logits_a, logits_s, dx, dWa, dba, [dWs, dbs,]
    dgamma, dbeta)"""
    names = ("h", "Wa", "ba", "gamma", "beta") + (() if I["unified"] else ("Ws", "bs"))
    P = {k: I[k].double().clone().requires_grad_(True) for k in names}
    D = P["h"].shape[-1]
    y = torch.nn.functional.layer_norm(P["h"], (D,), P["gamma"], P["beta"], EPS)
    ta, ts = y[:, 0], y[:, -1]
    aa = ta * I["mask_a"].double() if I["mask_a"] is not None else ta
    as_ = ts * I["mask_s"].double() if I["mask_s"] is not None else ts
    Ws, bs = (P["Wa"], P["ba"]) if I["unified"] else (P["Ws"], P["bs"])
    za, zs = aa @ P["Wa"].t() + P["ba"], as_ @ Ws.t() + bs
    seed = (za * I["dlogits_a"].double()).sum() + (zs * I["dlogits_s"].double()).sum()
    if I["dtoken_a"] is not None:
        seed = seed + (ta * I["dtoken_a"].double()).sum() + (ts * I["dtoken_s"].double()).sum()
    seed.backward()
    out = {"token_a": ta.detach(), "token_s": ts.detach(), "a": torch.cat([aa, as_]).detach(), "logits_a": za.detach(), "logits_s": zs.detach(), "dx": P["h"].grad,
           "dWa": P["Wa"].grad, "dba": P["ba"].grad, "dgamma": P["gamma"].grad, "dbeta": P["beta"].grad}
    if not I["unified"]:
        out.update(dWs=P["Ws"].grad, dbs=P["bs"].grad)
    return out


# ------------------------------------------------------------------------------------------------ bounds
def bounds(I, dtype):
    """-> (ref, bound) dicts over token_a, token_s, a, logits_a, logits_s, dx, dWa, dba, [dWs, dbs,] dgamma, dbeta at slack 1; the float64 values are recomputed
    stage by stage on the stacked rows (and checked against reference()'s autograd in test_two_token_head_bounds_cpu.py)"""
    uT = u_of(dtype)
    x = I["h"].double()
    B, Nt, D = x.shape
    dbl = lambda t: t.double()      # noqa: E731
    Wa, ba, Ws, bs = _heads(I, dbl)
    gm, bt = I["gamma"].double(), I["beta"].double()
    one = torch.ones((B, D), dtype=torch.float64)
    mk = torch.cat([I["mask_a"].double() if I["mask_a"] is not None else one, I["mask_s"].double() if I["mask_s"] is not None else one])
    t = torch.cat([x[:, 0], x[:, Nt - 1]])
    y, e_y, aux = _ln_fwd(t, torch.zeros_like(t), gm, bt, EPS, D)
    a = y * mk
    e_a = mk * e_y + (uT + 2 * U) * a.abs()
    e_tok = e_y + uT * y.abs()

    def head(a_, e_a_, W, b):
        z = a_ @ W.t() + b
        return z, e_a_ @ W.abs().t() + (D + 8) * U * (a_.abs() @ W.abs().t() + b.abs()) + uT * z.abs()

    za, e_za = head(a[:B], e_a[:B], Wa, ba)
    zs, e_zs = head(a[B:], e_a[B:], Ws, bs)
    ref = {"token_a": y[:B], "token_s": y[B:], "a": a, "logits_a": za, "logits_s": zs}
    bnd = {"token_a": e_tok[:B], "token_s": e_tok[B:], "a": e_a, "logits_a": e_za, "logits_s": e_zs}
    dla, dls = I["dlogits_a"].double(), I["dlogits_s"].double()

    def wgrad(dl, a_, e_a_, rows):
        return dl.t() @ a_, dl.abs().t() @ e_a_ + (rows + 8) * U * (dl.abs().t() @ a_.abs()), dl.sum(0), (rows + 8) * U * dl.abs().sum(0)

    if I["unified"]:
        ref["dWa"], bnd["dWa"], ref["dba"], bnd["dba"] = wgrad(torch.cat([dla, dls]), a, e_a, 2 * B)
    else:
        ref["dWa"], bnd["dWa"], ref["dba"], bnd["dba"] = wgrad(dla, a[:B], e_a[:B], B)
        ref["dWs"], bnd["dWs"], ref["dbs"], bnd["dbs"] = wgrad(dls, a[B:], e_a[B:], B)
    da = torch.cat([dla @ Wa, dls @ Ws])
    e_da = torch.cat([(Wa.shape[0] + 8) * U * (dla.abs() @ Wa.abs()), (Ws.shape[0] + 8) * U * (dls.abs() @ Ws.abs())])
    zero = torch.zeros((B, D), dtype=torch.float64)
    dtk = torch.cat([I["dtoken_a"].double() if I["dtoken_a"] is not None else zero, I["dtoken_s"].double() if I["dtoken_s"] is not None else zero])
    g = da * mk + dtk
    e_g = mk * e_da + 3 * U * ((da * mk).abs() + dtk.abs())
    dt, e_dt, (tw, ew), (tb, eb) = _ln_bwd(g, e_g, gm, aux, D)
    ref["dgamma"], bnd["dgamma"] = tw.sum(0), _rowsum(tw, ew, 2 * B)
    ref["dbeta"], bnd["dbeta"] = tb.sum(0), _rowsum(tb, eb, 2 * B)
    dx, e_dx = torch.zeros_like(x), torch.zeros_like(x)
    e_row = e_dt + (uT + 2 * U) * dt.abs()
    dx[:, 0], e_dx[:, 0] = dt[:B], e_row[:B]
    dx[:, Nt - 1], e_dx[:, Nt - 1] = dt[B:], e_row[B:]
    ref["dx"], bnd["dx"] = dx, e_dx
    return ref, bnd


SLACKS = {"token_a": SLACK_FWD, "token_s": SLACK_FWD, "logits_a": SLACK_FWD, "logits_s": SLACK_FWD, "a": SLACK_A, "dx": SLACK_BWD, "dWa": SLACK_BWD, "dba": SLACK_BWD,
          "dWs": SLACK_BWD, "dbs": SLACK_BWD, "dgamma": SLACK_BWD, "dbeta": SLACK_BWD}


def ratios(out, ref, bnd):
    """{name: excess against the bound at its slack} for the names present in `out`"""
    return {k: excess(out[k], ref[k], bnd[k] * SLACKS[k])[0] for k in out if k in ref}


# ------------------------------------------------------------------------------------------------ CPU emulation of the kernels
def _rt(t, dtype):
    return t.to(dtype).float()


def emulate(I, dtype, mutant=None):
    """The kernels' arithmetic in torch CPU float32 with exactly their roundings to `dtype` (token, a, logits, dx).  `mutant`: one of MUTANTS, a seeded fault:
      scene_row_nt2             the scene token is read from (and its dx row written to) row Nt - 2
      scene_row0                ... row 0: both tokens are the cls row, the scene dx row overwrites the action one
      dx_middle_nonzero         2^-20 of the action dx row is left in row 1 of a clip with Nt >= 3
      unified_dw_missing_scene  the unified head's dW / db sum the B action rows only
      dgamma_missing_scene      d gamma sums the stacked rows 0 .. B - 1
      masks_swapped             the action token meets the scene mask and the other way round (both directions)
      mask_after_round          a = T(T(y) mask)"""
    x = I["h"].float()
    B, Nt, D = x.shape
    flt = lambda t: t.float()      # noqa: E731
    Wa, ba, Ws, bs = _heads(I, flt)
    gm, bt = I["gamma"].float(), I["beta"].float()
    srow = Nt - 1
    if mutant == "scene_row_nt2":
        srow = max(Nt - 2, 0)
    elif mutant == "scene_row0":
        srow = 0
    ma, ms = I["mask_a"], I["mask_s"]
    if mutant == "masks_swapped":
        ma, ms = ms, ma
    mk = torch.cat([ma.float(), ms.float()]) if ma is not None else None
    t = torch.cat([x[:, 0], x[:, srow]])
    m = t.mean(-1, keepdim=True)
    d = t - m
    rs = torch.rsqrt((d * d).mean(-1, keepdim=True) + EPS)
    xh = d * rs
    y = xh * gm + bt
    token = _rt(y, dtype)
    if mk is None:
        a = token
    elif mutant == "mask_after_round":
        a = _rt(token * mk, dtype)
    else:
        a = _rt(y * mk, dtype)
    dla, dls = I["dlogits_a"].float(), I["dlogits_s"].float()
    out = {"token_a": token[:B], "token_s": token[B:], "a": a}
    if I["unified"]:
        z = _rt(a @ Wa.t() + ba, dtype)
        out["logits_a"], out["logits_s"] = z[:B], z[B:]
        dl2 = torch.cat([dla, dls])
        if mutant == "unified_dw_missing_scene":
            out["dWa"], out["dba"] = dla.t() @ a[:B], dla.sum(0)
        else:
            out["dWa"], out["dba"] = dl2.t() @ a, dl2.sum(0)
        g = dl2 @ Wa
    else:
        out["logits_a"], out["logits_s"] = _rt(a[:B] @ Wa.t() + ba, dtype), _rt(a[B:] @ Ws.t() + bs, dtype)
        out["dWa"], out["dba"], out["dWs"], out["dbs"] = dla.t() @ a[:B], dla.sum(0), dls.t() @ a[B:], dls.sum(0)
        g = torch.cat([dla @ Wa, dls @ Ws])
    if mk is not None:
        g = g * mk
    if I["dtoken_a"] is not None:
        g = g + torch.cat([I["dtoken_a"].float(), I["dtoken_s"].float()])
    out["dgamma"] = (g[:B] * xh[:B]).sum(0) if mutant == "dgamma_missing_scene" else (g * xh).sum(0)
    out["dbeta"] = g.sum(0)
    gy = g * gm
    c1, c2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    dt = _rt(rs * (gy - c1 - xh * c2), dtype)
    dx = torch.zeros_like(x)
    dx[:, 0] = dt[:B]
    dx[:, srow] = dt[B:]
    if mutant == "dx_middle_nonzero" and Nt >= 3:
        dx[:, 1] = _rt(dt[:B] * 2.0 ** -20, dtype)
    out["dx"] = dx
    return out
