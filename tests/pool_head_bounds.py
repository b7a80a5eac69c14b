"""Per-element error bounds against float64 for the pooled-head region of the plain video ViT (devias_pool_head_fwd / _bwd): csrc/pool_head.hip.

A sibling of fusion_bounds.py (same rules, same measure: excess(out, ref, bound) = max |out - ref| / bound, a test asserts <= 1; its LayerNorm forward / backward
terms are imported, not restated).  u_T is the unit of the storage dtype, u = U_FP32, e_x the bound carried by x.  Inputs are exact in both dtypes: h, the head
weight (on bf16's grid), the fp32 vectors, the fp32 mask.

Forward
    MEAN   s = sum of the Nt token rows in fp32, two stages (chunks of CHUNK tokens, then the chunks), ANY order    e_s = (Nt + 8) u sum|x|
           t = s * fl(1 / Nt)   -- a multiplication by the rounded reciprocal (two roundings), not a division           e_t = e_s / Nt + 3 u |t|
    CLS    t = row 0 of the clip                                                                                         e_t = 0
    y = LN(t; gamma, beta, eps 1e-6), n = D          e_y: fusion_bounds._ln_fwd
    token = T(y)                                     e_token = e_y + u_T |y|
    a = T(y mask)  (mask meets the UNROUNDED y)      e_a = mask e_y + (u_T + 2 u) |y mask|         -- held on its own (the save arena), at slack 1: see SLACK_A
    logits = T(a W^T + b)                            e_logits = |W| e_a + (D + 8) u (|W| |a| + |b|) + u_T |logits|
Backward (on the saved forward: a, x^ and rstd are re-read, so their e_* enter)
    dW = dlogits^T a          |dl|^T e_a + (B + 8) u |dl|^T |a| ;    db = column sums of dlogits: (B + 8) u sum|dl|
    da = dlogits W  (fp32)    e_da = (C + 8) u |dl| |W|
    g = da mask + dtoken      e_g = mask e_da + 3 u (|da mask| + |dtoken|)
    LayerNorm backward (fusion_bounds._ln_bwd) -> dt, e_dt;  d gamma = sum_b g x^, d beta = sum_b g over the clips in a fixed order: fusion_bounds._rowsum
    MEAN   every token row of clip b:  dx = T(dt * fl(1 / Nt))       e_dx = e_dt / Nt + (u_T + 3 u) |dt| / Nt
    CLS    row 0: dx = T(dt)   e_dx = e_dt + (u_T + 2 u) |dt| ;  every other row EXACTLY zero (bound 0)

Slacks.  SLACK_FWD / SLACK_BWD are twice what the CPU emulation (emulate(): the formulas above in torch CPU float32 with exactly the kernels' roundings) needs over
every generator, both dtypes, both pool modes, mask absent and keep = 0.75, dtoken absent and present (tests/test_pool_head_bounds_cpu.py prints the ratios and
asserts the emulation stays under HALF the slack).  SLACK_A = 1: the bound of `a` is one round-to-nearest of an fp32 value (|T(v) - v| <= u_T |v| holds without
slack) plus the LayerNorm's fp32 terms; only so can a second rounding (the mutant mask_after_round) show.  Never fitted to the HIP kernel.

Generators (GENERATORS) and mutants (MUTANTS): see inputs() and emulate().
"""
import torch

from fusion_bounds import _ln_bwd, _ln_fwd, _rowsum
from kernel_bounds import U_FP32, _randn, excess, graded, u_of  # noqa: F401

MEAN, CLS = 0, 1
CHUNK = 64                  # DEVIAS_POOL_HEAD_CHUNK (tests/test_plainvit_cpu.py holds the header, _lib and this to one value)
EPS = 1e-6
SLACK_FWD = 2 * 0.985       # the emulation needs 0.9847 (bf16 token: the store alone; logits 0.258; fp32: token 0.144, logits 0.010)
SLACK_BWD = 2 * 0.995       # the emulation needs 0.9947 (bf16 dW at B = 1: the stored a alone; dx 0.977; fp32: db 0.159, dW 0.121, dbeta 0.118, dx 0.036)
SLACK_A = 1.0               # the emulation reaches 0.9951 in bf16 (0.147 in fp32)
KEEP = 0.75                 # 1 / keep is no power of two: T(T(y) / keep) differs from T(y / keep)
GENERATORS = ("graded", "tail", "offset")
MUTANTS = ("drop_last", "partial_twice", "inv_nt_minus1", "mask_after_round", "dbeta_missing_clip", "cls_row1", "cls_nonzero_row")
U = U_FP32


def _bf16_grid(t):
    return t.bfloat16().float()


def inputs(kind, B, Nt, D, C, dtype, mask, dtok, seed=0):
    """-> dict(h [B, Nt, D] in dtype, W [C, D] fp32 on bf16's grid, bias, gamma, beta fp32, mask fp32 [B, D] or None, dlogits [B, C] and dtoken [B, D] or None in dtype)
      graded   token rows scaled by kernel_bounds.graded(Nt) (2^-6 ... 2^6, odd period 13): every chunk and ragged tail holds every scale; a wrong row set,
               a wrong 1 / Nt or a chunk counted twice moves the mean by far more than the bound
      tail     unit scale, the LAST token of every clip 64 times larger (and row 1 unlike row 0): a dropped last row of a ragged chunk, or CLS taking row 1, shows
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
    W = _bf16_grid(_randn((C, D), seed + 2, "cpu") * 0.05 * graded(C, 3).float()[:, None])
    out = {"h": x.to(dtype), "W": W, "bias": 0.05 * _randn((C,), seed + 3, "cpu"),
           "gamma": torch.linspace(-1.0, 1.5, D) + 0.01 * _randn((D,), seed + 4, "cpu"), "beta": 0.1 * _randn((D,), seed + 5, "cpu"),
           "mask": None, "dtoken": None}
    if mask:
        g = torch.Generator().manual_seed(seed + 6)
        out["mask"] = ((torch.rand((B, D), generator=g) < KEEP).float() / KEEP).contiguous()
    out["dlogits"] = (_randn((B, C), seed + 7, "cpu") * 0.05 * graded(B, 2).float()[:, None]).to(dtype)
    if dtok:
        out["dtoken"] = (_randn((B, D), seed + 8, "cpu") * 0.01).to(dtype)
    return out


# ------------------------------------------------------------------------------------------------ float64 reference (autograd) and the restatement a model test uses
def pool_head_forward(h, W, bias, gamma, beta, pool, mask=None, eps=EPS):
    """plain PyTorch in h's dtype: h [B, Nt, D] -> (token, a, logits)"""
    t = h.mean(1) if pool == MEAN else h[:, 0]
    y = torch.nn.functional.layer_norm(t, (h.shape[-1],), gamma, beta, eps)
    a = y * mask if mask is not None else y
    return y, a, a @ W.t() + bias


def reference(I, pool):
    """float64 autograd -> dict(token, a, logits, dx [B, Nt, D], dW, db, dgamma, dbeta)"""
    P = {k: I[k].double().clone().requires_grad_(True) for k in ("h", "W", "bias", "gamma", "beta")}
    mk = I["mask"].double() if I["mask"] is not None else None
    y, a, z = pool_head_forward(P["h"], P["W"], P["bias"], P["gamma"], P["beta"], pool, mk)
    seed = (z * I["dlogits"].double()).sum()
    if I["dtoken"] is not None:
        seed = seed + (y * I["dtoken"].double()).sum()
    seed.backward()
    return {"token": y.detach(), "a": a.detach(), "logits": z.detach(), "dx": P["h"].grad, "dW": P["W"].grad, "db": P["bias"].grad, "dgamma": P["gamma"].grad,
            "dbeta": P["beta"].grad}


# ------------------------------------------------------------------------------------------------ bounds
def bounds(I, pool, dtype):
    """-> (ref, bound) dicts over token, a, logits, dx, dW, db, dgamma, dbeta at slack 1; the float64 values are recomputed stage by stage (and checked against
    reference()'s autograd in test_pool_head_bounds_cpu.py)"""
    uT = u_of(dtype)
    x = I["h"].double()
    B, Nt, D = x.shape
    W, bias, gm, bt = (I[k].double() for k in ("W", "bias", "gamma", "beta"))
    C = W.shape[0]
    mk = I["mask"].double() if I["mask"] is not None else torch.ones((B, D), dtype=torch.float64)
    if pool == MEAN:
        t = x.sum(1) / Nt
        e_t = (Nt + 8) * U * x.abs().sum(1) / Nt + 3 * U * t.abs()
    else:
        t, e_t = x[:, 0], torch.zeros((B, D), dtype=torch.float64)
    y, e_y, aux = _ln_fwd(t, e_t, gm, bt, EPS, D)
    a = y * mk
    e_a = mk * e_y + (uT + 2 * U) * a.abs()
    z = a @ W.t() + bias
    e_z = e_a @ W.abs().t() + (D + 8) * U * (a.abs() @ W.abs().t() + bias.abs()) + uT * z.abs()
    ref = {"token": y, "a": a, "logits": z}
    bnd = {"token": e_y + uT * y.abs(), "a": e_a, "logits": e_z}
    dl = I["dlogits"].double()
    ref["dW"], bnd["dW"] = dl.t() @ a, dl.abs().t() @ e_a + (B + 8) * U * (dl.abs().t() @ a.abs())
    ref["db"], bnd["db"] = dl.sum(0), (B + 8) * U * dl.abs().sum(0)
    da = dl @ W
    e_da = (C + 8) * U * (dl.abs() @ W.abs())
    dtk = I["dtoken"].double() if I["dtoken"] is not None else torch.zeros((B, D), dtype=torch.float64)
    g = da * mk + dtk
    e_g = mk * e_da + 3 * U * ((da * mk).abs() + dtk.abs())
    dt, e_dt, (tw, ew), (tb, eb) = _ln_bwd(g, e_g, gm, aux, D)
    ref["dgamma"], bnd["dgamma"] = tw.sum(0), _rowsum(tw, ew, B)
    ref["dbeta"], bnd["dbeta"] = tb.sum(0), _rowsum(tb, eb, B)
    dx, e_dx = torch.zeros_like(x), torch.zeros_like(x)
    if pool == MEAN:
        dx[:] = (dt / Nt)[:, None]
        e_dx[:] = (e_dt / Nt + (uT + 3 * U) * dt.abs() / Nt)[:, None]
    else:
        dx[:, 0] = dt
        e_dx[:, 0] = e_dt + (uT + 2 * U) * dt.abs()
    ref["dx"], bnd["dx"] = dx, e_dx
    return ref, bnd


SLACKS = {"token": SLACK_FWD, "logits": SLACK_FWD, "a": SLACK_A, "dx": SLACK_BWD, "dW": SLACK_BWD, "db": SLACK_BWD, "dgamma": SLACK_BWD, "dbeta": SLACK_BWD}


def ratios(out, ref, bnd):
    """{name: excess against the bound at its slack} for the names present in `out`"""
    return {k: excess(out[k], ref[k], bnd[k] * SLACKS[k])[0] for k in out if k in ref}


# ------------------------------------------------------------------------------------------------ CPU emulation of the kernels
def _rt(t, dtype):
    return t.to(dtype).float()


def emulate(I, pool, dtype, mutant=None):
    """The kernels' arithmetic in torch CPU float32 with exactly their roundings to `dtype` (token, a, logits, dx).  `mutant`: one of MUTANTS, a seeded fault:
      drop_last           the last token of a ragged last chunk is not added            partial_twice       chunk 0's sum is added twice
      inv_nt_minus1       the forward multiplies by 1 / (Nt - 1)                        mask_after_round    a = T(T(y) mask)
                          (the LayerNorm forgets the forward's scale and its saved rstd carries the inverse into dx; the SAME wrong factor in both directions
                          would cancel but for eps, so the seeded fault is the forward's alone)
      dbeta_missing_clip  d beta sums the clips 0 .. B - 2                              cls_row1            CLS writes the dx row into token row 1
      cls_nonzero_row     CLS leaves 2^-20 of the dx row in the clip's last row"""
    x = I["h"].float()
    B, Nt, D = x.shape
    W, bias, gm, bt = (I[k].float() for k in ("W", "bias", "gamma", "beta"))
    mk = I["mask"].float() if I["mask"] is not None else None
    one = torch.tensor(1.0, dtype=torch.float32)
    inv_b = one / torch.tensor(float(Nt), dtype=torch.float32)
    inv = one / torch.tensor(float(Nt - 1), dtype=torch.float32) if (mutant == "inv_nt_minus1" and Nt > 1) else inv_b
    if pool == MEAN:
        s = torch.zeros((B, D), dtype=torch.float32)
        nch = (Nt + CHUNK - 1) // CHUNK
        for c in range(nch):
            t1 = min(Nt, (c + 1) * CHUNK)
            if mutant == "drop_last" and c == nch - 1 and Nt % CHUNK != 0:
                t1 -= 1
            part = x[:, c * CHUNK:t1].sum(1)
            s = s + part
            if mutant == "partial_twice" and c == 0:
                s = s + part
        t = s * inv
    else:
        t = x[:, 0]
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
    z = _rt(a @ W.t() + bias, dtype)
    dl = I["dlogits"].float()
    out = {"token": token, "a": a, "logits": z, "dW": dl.t() @ a, "db": dl.sum(0)}
    g = dl @ W
    if mk is not None:
        g = g * mk
    if I["dtoken"] is not None:
        g = g + I["dtoken"].float()
    out["dgamma"] = (g * xh).sum(0)
    out["dbeta"] = g[:B - 1].sum(0) if mutant == "dbeta_missing_clip" else g.sum(0)
    gy = g * gm
    c1, c2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    dt = rs * (gy - c1 - xh * c2)
    dx = torch.zeros_like(x)
    if pool == MEAN:
        dx[:] = _rt(dt * inv_b, dtype)[:, None]
    else:
        row = 1 if (mutant == "cls_row1" and Nt > 1) else 0
        dx[:, row] = _rt(dt, dtype)
        if mutant == "cls_nonzero_row" and Nt > 1:
            dx[:, Nt - 1] = _rt(dt * 2.0 ** -20, dtype)
    out["dx"] = dx
    return out
