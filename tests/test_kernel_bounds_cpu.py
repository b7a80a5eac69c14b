"""The bounds of tests/kernel_bounds.py proved without a GPU: for every operation, on every generator, the ideal result (float64 rounded once) and the
CPU emulation of the documented algorithm (the reference plus exactly the named roundings, torch CPU arithmetic) stay inside the bound, and every seeded
mutant -- the errors hand-written kernels make -- exceeds it.  The last tests record why the file exists: the maximum-norm `rel` metric of
tests/test_kernels_gpu.py at its tolerance passes those mutants on graded inputs (a flipped dropout-mask element among them).

Limits: the ideal <= 1 everywhere; the emulation <= 1 under the rigorous bounds (GEMM without activation, LayerNorm forward: their factor is 1 and a bf16
output rounding alone reaches ~1) and <= 0.5 under every bound that carries a slack (activations, LayerNorm backward, attention)."""
import math

import pytest
import torch

import kernel_bounds as kb

BF, F32 = torch.bfloat16, torch.float32
SPREADS = [0, 6]                      # the generators: single scale, graded 2^-6 ... 2^6
LOG2E = 1.4426950408889634


def rel(a, b):                        # the metric of tests/test_kernels_gpu.py
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def report(name, r):
    print(f"[bound-cpu] {name} worst ratio {r:.3f}")
    return r


# ------------------------------------------------------------------------------------------------ GEMM
GM, GN, GK = 256, 256, 512


def gemm_emul(A, B, bias, res, dtype, mutant=None, small_rows=None):
    """fp32 accumulation, one rounding of the output (the documented algorithm); mutants: the four wrong GEMMs of the issue's table"""
    a, b = A.float(), B.float()
    if mutant == "acc_bf16_every_64":
        acc = torch.zeros(A.shape[0], B.shape[0])
        for k0 in range(0, a.shape[1], 64):
            acc = (acc + a[:, k0:k0 + 64] @ b[:, k0:k0 + 64].t()).to(BF).float()
    else:
        acc = a @ b.t()
    if mutant == "kstep_dropped_small_rows":
        acc[small_rows] = a[small_rows, :-16] @ b[:, :-16].t()
    bb = bias.clone()
    if mutant == "bias_missing_last_8_cols":
        bb[-8:] = 0
    v = acc + bb
    if mutant == "double_rounding":
        v = v.to(dtype).float()
    return (v + res.float()).to(dtype)


def gemm_case(dtype, spread):
    A, B, bias, res = kb.gemm_inputs(GM, GN, GK, dtype, spread=spread, seed=10)
    r = kb.gemm_ref(A, B.t(), dtype, bias=bias, res=res)["out"]
    small = torch.argsort(kb.graded(GM, spread), stable=True)[:16]
    return A, B, bias, res, r, small


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("dtype", [BF, F32])
def test_gemm_ideal_and_emulation(dtype, spread):
    A, B, bias, res, (ref, bound), _ = gemm_case(dtype, spread)
    w = lambda i: kb.where2d(i, GN)  # noqa: E731
    report(f"gemm ideal {dtype} spread {spread}", kb.check("ideal", ref.to(dtype), ref, bound, w))
    report(f"gemm emulation {dtype} spread {spread}", kb.check("emulation", gemm_emul(A, B, bias, res, dtype), ref, bound, w))


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("mutant", ["double_rounding", "acc_bf16_every_64", "kstep_dropped_small_rows", "bias_missing_last_8_cols"])
def test_gemm_mutants_exceed_the_bound(mutant, spread):
    A, B, bias, res, (ref, bound), small = gemm_case(BF, spread)
    r, idx = kb.excess(gemm_emul(A, B, bias, res, BF, mutant, small), ref, bound)
    report(f"gemm mutant {mutant} spread {spread}", r)
    assert r > 1.0, (mutant, r)
    row, col = divmod(idx, GN)
    if mutant == "kstep_dropped_small_rows" and spread:
        assert row in small.tolist(), kb.where2d(idx, GN)         # the message names the rows at fault
    if mutant == "bias_missing_last_8_cols":
        assert col >= GN - 8, kb.where2d(idx, GN)


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("dtype", [BF, F32])
def test_gemm_layout_variants(dtype, spread):
    """res_mod (positional table), row scale, fp32 output with beta: ideal and emulation"""
    M, N, K = 130, 200, 72
    A, B, bias, pos = kb.gemm_inputs(M, N, K, dtype, spread=spread, seed=20, res_rows=10)
    ref, bound = kb.gemm_ref(A, B.t(), dtype, bias=bias, res=pos, res_mod=10)["out"]
    em = (A.float() @ B.float().t() + bias + pos.float().repeat(13, 1)).to(dtype)
    report(f"gemm res_mod {dtype} spread {spread}", kb.check("res_mod", em, ref, bound, lambda i: kb.where2d(i, N)))
    rs = (torch.arange(M) % 3).float() * 0.5
    _, _, _, res = kb.gemm_inputs(M, N, K, dtype, spread=spread, seed=20)
    ref, bound = kb.gemm_ref(A, B.t(), dtype, bias=bias, res=res, row_scale=rs, rows_per_scale=1)["out"]
    em = ((A.float() @ B.float().t() + bias) * rs[:, None] + res.float()).to(dtype)
    report(f"gemm row_scale {dtype} spread {spread}", kb.check("row_scale", em, ref, bound, lambda i: kb.where2d(i, N)))
    c_old = torch.randn(M, N, generator=torch.Generator().manual_seed(5)) * kb.graded(M, spread).float()[:, None]
    ref, bound = kb.gemm_ref(A, B.t(), dtype, out_f32=True, beta=1.0, c_old=c_old)["out"]
    em = A.float() @ B.float().t() + c_old
    report(f"gemm beta {dtype} spread {spread}", kb.check("out_f32 beta", em, ref, bound, lambda i: kb.where2d(i, N)))
    bad = A.float() @ B.float().t() + c_old.to(BF).float()          # C_old passing through bf16
    assert kb.excess(bad, ref, bound)[0] > 1.0


ACTS = [kb.ACT_GELU, kb.ACT_RELU, kb.ACT_SIGMOID, kb.ACT_DGELU, kb.ACT_DRELU]


def act_emul(v, aux, act, dtype, tanh_gelu=False):
    """fp32 epilogue arithmetic on the fp32 pre-activation v; bf16: the kernels' polynomial GELU (csrc/common.h)"""
    if act == kb.ACT_GELU:
        if tanh_gelu:
            return 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))
        return kb.gelu_poly_fp32(v) if dtype == BF else 0.5 * v * (1 + torch.erf(v * 0.70710678118654752440))
    if act == kb.ACT_RELU:
        return v.clamp_min(0)
    if act == kb.ACT_SIGMOID:
        return 1.0 / (1.0 + torch.exp(-v))
    if act == kb.ACT_DGELU:
        x = aux.float()
        return v * (kb.dgelu_poly_fp32(x) if dtype == BF else 0.5 * (1 + torch.erf(x * 0.70710678118654752440)) + x * 0.39894228040143267794 * torch.exp(-0.5 * x * x))
    return torch.where(aux.float() > 0, v, torch.zeros_like(v))


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("act", ACTS)
def test_activation_epilogues(act, dtype, spread):
    M, N, K = 130, 200, 72
    A, B, bias, _ = kb.gemm_inputs(M, N, K, dtype, spread=min(spread, 2), seed=30)        # (pre-activations across the activation's range, not far in its tails)
    aux = (torch.randn(M, N, generator=torch.Generator().manual_seed(31)) * 1.5).to(dtype)
    has_bias = act in (kb.ACT_GELU, kb.ACT_RELU, kb.ACT_SIGMOID)
    r = kb.gemm_ref(A, B.t(), dtype, bias=bias if has_bias else None, act=act, aux_in=aux)
    ref, bound = r["out"]
    w = lambda i: kb.where2d(i, N)  # noqa: E731
    v = A.float() @ B.float().t() + (bias if has_bias else 0)
    report(f"act {act} ideal {dtype} spread {spread}", kb.check("ideal", ref.to(dtype), ref, bound, w))
    y = act_emul(v, aux, act, dtype)
    report(f"act {act} emulation {dtype} spread {spread}", kb.check("emulation", y.to(dtype), ref, bound, w, limit=0.5))
    cs_ref, cs_bound = r["colsum"]
    report(f"act {act} colsum emulation {dtype} spread {spread}", kb.check("colsum", y.sum(0), cs_ref, cs_bound, limit=0.5))
    if act == kb.ACT_GELU:
        aref, abound = r["aux"]
        report(f"aux_out emulation {dtype} spread {spread}", kb.check("aux_out", v.to(dtype), aref, abound, w))
        # the activation is NOT bounded as if computed from the rounded copy: in bf16 that kernel would be wrong
        if dtype == BF:
            assert kb.excess(act_emul(v.to(BF).float(), aux, act, dtype).to(dtype), ref, bound)[0] > 1.0
        # mutant: the tanh form of GELU
        rt = kb.excess(act_emul(v, aux, act, F32, tanh_gelu=True).to(dtype), ref, bound)[0]
        report(f"act mutant tanh GELU {dtype} spread {spread}", rt)
        assert rt > 1.0, rt


@pytest.mark.parametrize("spread", SPREADS)
def test_colsum_from_the_rounded_output_exceeds_the_fused_bound(spread):
    """mutant: column sums taken from the bf16-rounded output where the fused path promises sums of the fp32 values (K = 64: the rigorous any-order term
    (K + 8) u_fp32 |A||B| of the accumulation grows with K and at K = 512 is as large as the M roundings of this mutant)"""
    A, B, bias, _ = kb.gemm_inputs(GM, GN, 64, BF, spread=spread, seed=10)
    v = A.float() @ B.float().t() + bias
    cs_ref, cs_bound = kb.gemm_ref(A, B.t(), BF, bias=bias)["colsum"]
    report(f"colsum emulation spread {spread}", kb.check("colsum", v.sum(0), cs_ref, cs_bound))
    rc = report(f"colsum mutant from the rounded output spread {spread}", kb.excess(v.to(BF).float().sum(0), cs_ref, cs_bound)[0])
    assert rc > 1.0, rc
    # ... which is what the fall-back over the stored C does (devias_colsum), and its bound allows
    cs2 = kb.gemm_ref(A, B.t(), BF, bias=bias, colsum_from_stored=True)["colsum"]
    kb.check("colsum over the stored C", v.to(BF).float().sum(0), *cs2)
    old = torch.randn(GN, generator=torch.Generator().manual_seed(3)) * 100
    cs3 = kb.gemm_ref(A, B.t(), BF, bias=bias, colsum_old=old, colsum_beta=1.0)["colsum"]
    kb.check("colsum with beta", v.sum(0) + old, *cs3)


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_emul(x, g, b, eps, dtype, one_pass=False):
    v = x.float()
    D = v.shape[1]
    mu = v.sum(1) / D
    if one_pass:
        var = (v * v).sum(1) / D - mu * mu
    else:
        d = v - mu[:, None]
        var = (d * d).sum(1) / D
    rs = torch.rsqrt(var + eps)
    return ((v - mu[:, None]) * rs[:, None] * g + b).to(dtype), mu, rs


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("M,D,eps", [(67, 1024, 1e-6), (130, 384, 1e-5)])
def test_layernorm_forward(M, D, eps, dtype, spread):
    x, g, b, _, _ = kb.layernorm_inputs(M, D, dtype, spread=spread, seed=40)
    r = kb.layernorm_fwd_ref(x, g, b, eps, dtype)
    w = lambda i: kb.where2d(i, D)  # noqa: E731
    report(f"ln fwd ideal {dtype} spread {spread}", kb.check("ideal y", r["y"][0].to(dtype), *r["y"], w))
    y, mu, rs = ln_fwd_emul(x, g, b, eps, dtype)
    report(f"ln fwd y emulation {dtype} spread {spread}", kb.check("y", y, *r["y"], w))
    report(f"ln fwd mean emulation {dtype} spread {spread}", kb.check("mean", mu, *r["mean"]))
    report(f"ln fwd rstd emulation {dtype} spread {spread}", kb.check("rstd", rs, *r["rstd"]))
    if dtype == F32:
        # mutant: one-pass E[x^2] - E[x]^2 variance in fp32; the rows offset by 100 standard deviations give it away
        _, _, rs1 = ln_fwd_emul(x, g, b, eps, dtype, one_pass=True)
        rr, idx = kb.excess(rs1, *r["rstd"])
        report(f"ln fwd mutant one-pass variance spread {spread}", rr)
        assert rr > 1.0 and idx % 3 == 2, (rr, idx)


def ln_bwd_emul(dy, x, g, mu, rs, dres, dtype, mutant=None):
    d, v = dy.float(), x.float()
    D = v.shape[1]
    xh = (v - mu[:, None]) * rs[:, None]
    a = d * g
    m1, m2 = a.sum(1, keepdim=True) / D, (a * xh).sum(1, keepdim=True) / D
    o = rs[:, None] * (a - m1 - xh * m2)
    if dres is not None:
        o = (o.to(dtype).float() + dres.float()) if mutant == "dres_after_rounding" else o + dres.float()
    dg = (d * (xh.to(BF).float() if mutant == "dgamma_from_bf16_xhat" else xh)).sum(0)
    return o.to(dtype), dg, d.sum(0), o.sum(0)


@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("M,D", [(67, 1024), (130, 384)])
def test_layernorm_backward(M, D, with_dres, dtype, spread):
    x, g, b, dy, dres = kb.layernorm_inputs(M, D, dtype, spread=spread, seed=50)
    dres = dres if with_dres else None
    _, mu, rs = ln_fwd_emul(x, g, b, 1e-6, dtype)
    r = kb.layernorm_bwd_ref(dy, x, g, mu, rs, dtype, dres=dres)
    w = lambda i: kb.where2d(i, D)  # noqa: E731
    report(f"ln bwd ideal {dtype} spread {spread}", kb.check("ideal dx", r["dx"][0].to(dtype), *r["dx"], w))
    dx, dg, db, cs = ln_bwd_emul(dy, x, g, mu, rs, dres, dtype)
    tag = f"{dtype} spread {spread} dres {with_dres}"
    report(f"ln bwd dx emulation {tag}", kb.check("dx", dx, *r["dx"], w, limit=0.5))
    report(f"ln bwd dgamma emulation {tag}", kb.check("dgamma", dg, *r["dgamma"], limit=0.5))
    report(f"ln bwd dbeta emulation {tag}", kb.check("dbeta", db, *r["dbeta"], limit=0.5))
    report(f"ln bwd dx_colsum emulation {tag}", kb.check("dx_colsum", cs, *r["dx_colsum"], limit=0.5))
    _, dg_m, _, _ = ln_bwd_emul(dy, x, g, mu, rs, dres, dtype, mutant="dgamma_from_bf16_xhat")
    rm = report(f"ln bwd mutant dgamma from bf16 xhat {tag}", kb.excess(dg_m, *r["dgamma"])[0])
    assert rm > 1.0, rm
    if with_dres and dtype == BF:
        dx_m = ln_bwd_emul(dy, x, g, mu, rs, dres, dtype, mutant="dres_after_rounding")[0]
        rm = report(f"ln bwd mutant dres after rounding {tag}", kb.excess(dx_m, *r["dx"])[0])
        assert rm > 1.0, rm


# ------------------------------------------------------------------------------------------------ attention
SCALE = 0.125
C = SCALE * LOG2E
AB, AN, AH = 2, 100, 3


def split(qkv, B, N, H):
    t = qkv.float().reshape(B, N, 3, H, 64)
    return tuple(t[:, :, i].permute(0, 2, 1, 3) for i in range(3))


def rows(t, B, N, H):
    return t.permute(0, 2, 1, 3).reshape(B * N, H * 64)


def f32(t):
    """one fp32 rounding of a float64 value.  The attention emulations compute every product, sum and exp2 in float64 and round it to fp32 where the kernels hold an
    fp32 value: the correctly rounded fp32 result, the same on every CPU whatever the order its BLAS and vector math library sum and approximate in."""
    return t.float().double()


def b16(t):
    return t.float().to(BF).double()


def attn_fwd_emul(qkv, B, N, H, dtype, prescaled=False, mutant=None, mask=None):
    """bf16: q' = bf16(q c) (or the caller's q'), S' = q' k in fp32, P = exp2(S' - m) rounded to bf16 for P V, l from the fp32 P, o rounded once.
    fp32: the same in fp32 with no intermediate rounding.  mask (attention dropout, float64 [B, H, N, N] of 0 or 1 / keep): P mask is one fp32 product, rounded
    once to bf16 for P V; l stays the sum of the un-dropped fp32 P.  Returns o [B N, H 64], lse [B, H, N]."""
    q, k, v = (t.double() for t in split(qkv, B, N, H))
    if dtype == BF:
        qs = q if prescaled else b16(f32(q * C))
    else:
        qs = f32(q * C)
    s = f32(qs @ k.transpose(-1, -2))
    if mutant == "last_key_dropped_small_head":
        s[:, 0, :, N - 1] = -float("inf")                     # head 0 is the head whose V is scaled 2^-6
    m = s.max(-1, keepdim=True).values
    p = f32(torch.exp2(s - m))
    l = f32(p.sum(-1, keepdim=True))
    if mutant == "l_from_other_values":                       # l taken from other values than the numerator: each 64-key tile's P relative to the running maximum
        l = torch.zeros_like(m)                               # at that tile, the earlier sum NOT rescaled when the maximum moves (the numerator is)
        for k0 in range(0, N, 64):
            mt = s[..., :k0 + 64].max(-1, keepdim=True).values
            l = f32(l + f32(torch.exp2(s[..., k0:k0 + 64] - mt)).sum(-1, keepdim=True))
        l = f32(l * torch.exp2(mt - m))
    pd = p if mask is None else f32(p * mask)
    if mutant == "l_from_the_dropped_p":                      # the normaliser (and lse) taken from the dropped probabilities
        l = f32(pd.sum(-1, keepdim=True))
    pb = b16(pd) if dtype == BF else pd
    o = f32(f32(pb @ v) / l)
    lse = f32((m + torch.log2(l)).squeeze(-1) / LOG2E)
    return rows(o, B, N, H).to(dtype), lse.float()


def prescale(qkv, B, N, H):
    return kb.attention_prescale(qkv, B, N, H, SCALE)


@pytest.mark.parametrize("std,koff", kb.ATTN_GENERATORS)
@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16_prescaled"])
def test_attention_forward(mode, std, koff):
    dtype = F32 if mode == "f32" else BF
    qkv, _ = kb.attention_inputs(AB, AN, AH, dtype, logit_std=std, seed=60, key_offset=koff)
    w = lambda i: kb.where_attn(i, AN, AH)  # noqa: E731
    if mode == "bf16_prescaled":
        qkv_k, seen = prescale(qkv, AB, AN, AH)
        r = kb.mhsa_fwd_ref(seen, AB, AN, AH, SCALE, dtype, q_rounded=False)
        o, lse = attn_fwd_emul(qkv_k, AB, AN, AH, dtype, prescaled=True)
    else:
        r = kb.mhsa_fwd_ref(qkv, AB, AN, AH, SCALE, dtype)
        o, lse = attn_fwd_emul(qkv, AB, AN, AH, dtype)
    report(f"mhsa fwd ideal {mode} std {std} koff {koff}", kb.check("ideal", r["out"][0].to(dtype), *r["out"], w))
    report(f"mhsa fwd out emulation {mode} std {std} koff {koff}", kb.check("out", o, *r["out"], w, limit=0.5))
    report(f"mhsa fwd lse emulation {mode} std {std} koff {koff}", kb.check("lse", lse, *r["lse"], limit=0.5))
    # mutants.  Pre-scaled path (no score-rounding term in its bound): asserted on every generator.  Plain path: on the offset-free generators -- with the key
    # offset its bound's u sum p T |v - o| term (T ~ 100) allows more than one key's weight, which is what that generator is for (kernel_bounds.ATTN_GENERATORS)
    if dtype == BF:
        for mutant in ("last_key_dropped_small_head", "l_from_other_values"):
            om, _ = attn_fwd_emul(qkv_k if mode == "bf16_prescaled" else qkv, AB, AN, AH, dtype, prescaled=mode == "bf16_prescaled", mutant=mutant)
            rm, idx = kb.excess(om, *r["out"])
            report(f"mhsa fwd mutant {mutant} {mode} std {std} koff {koff}", rm)
            if mode == "bf16_prescaled" or koff == 0.0:
                assert rm > 1.0, (mutant, rm, w(idx))
                if mutant == "last_key_dropped_small_head":
                    assert (idx % (AH * 64)) // 64 == 0, w(idx)                # the message names the head


def attn_bwd_emul(qkv, o, d_o, lse, B, N, H, dtype, prescaled=False, mutant=None, mask=None):
    """dQ kernel: scores from q' = bf16(q c); one-wave dK / dV kernel: scores from k' = bf16(k c) (plain path) -- with the flag both multiply the caller's q' and k.
    P = exp2(S' - lse log2 e); dP = dO V^T; delta = rowsum(dO o) from the stored o; P and dS rounded to bf16 for their products; outputs rounded once.
    mask (attention dropout): dP is masked (one fp32 product) before dS, dV comes from bf16(P mask); the scores are those of the plain emulation."""
    q, k, v = (t.double() for t in split(qkv, B, N, H))
    dO = d_o.double().reshape(B, N, H, 64).permute(0, 2, 1, 3)
    oo = o.double().reshape(B, N, H, 64).permute(0, 2, 1, 3)
    lse2 = f32(lse.double() * LOG2E)[..., None]
    r16 = b16 if dtype == BF else (lambda t: t)
    if prescaled:
        s_q = s_kv = f32(q @ k.transpose(-1, -2))
        q_un = q / C
        if mutant == "kc_rounded_on_the_flagged_path":
            s_kv = f32(q_un @ r16(f32(k * C)).transpose(-1, -2))
    else:
        s_q = f32(r16(f32(q * C)) @ k.transpose(-1, -2))
        s_kv = f32(q @ r16(f32(k * C)).transpose(-1, -2))
        q_un = q
    dP = f32(dO @ v.transpose(-1, -2))
    if mask is not None and mutant != "dp_left_unmasked":
        dP = f32(dP * mask)
    delta = f32((dO * oo).sum(-1, keepdim=True))
    p_q, p_kv = f32(torch.exp2(s_q - lse2)), f32(torch.exp2(s_kv - lse2))
    dq = f32(SCALE * (r16(f32(p_q * (dP - delta))) @ k))
    dk = f32(SCALE * (r16(f32(p_kv * (dP - delta))).transpose(-1, -2) @ q_un))
    dv = f32(r16(p_kv if mask is None else f32(p_kv * mask)).transpose(-1, -2) @ dO)
    # the bias gradients of the _bias entry point: fp32 column sums of the UNROUNDED dQ / dV accumulators (bf16: devias_amd.h:293-300; dbv = colsum(dO) on the one-wave path)
    dbq, dbv = f32(rows(dq, B, N, H).sum(0)), f32(rows(dv, B, N, H).sum(0))
    return tuple(rows(t, B, N, H).to(dtype) for t in (dq, dk, dv)) + (dbq.float(), dbv.float())


@pytest.mark.parametrize("std,koff", kb.ATTN_GENERATORS)
@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16_prescaled"])
def test_attention_backward(mode, std, koff):
    dtype = F32 if mode == "f32" else BF
    qkv, d_o = kb.attention_inputs(AB, AN, AH, dtype, logit_std=std, seed=70, key_offset=koff)
    w = lambda i: kb.where_attn(i, AN, AH)  # noqa: E731
    pre = mode == "bf16_prescaled"
    if pre:
        qkv_k, seen = prescale(qkv, AB, AN, AH)
    else:
        qkv_k, seen = qkv, qkv
    r = kb.mhsa_bwd_ref(seen, d_o, AB, AN, AH, SCALE, dtype, plain=not pre)
    o, lse = attn_fwd_emul(qkv_k, AB, AN, AH, dtype, prescaled=pre)
    got = attn_bwd_emul(qkv_k, o, d_o, lse, AB, AN, AH, dtype, prescaled=pre)
    for name, t in zip(("dq", "dk", "dv"), got[:3]):
        report(f"mhsa bwd {name} ideal {mode} std {std} koff {koff}", kb.check("ideal " + name, r[name][0].to(dtype), *r[name], w))
        report(f"mhsa bwd {name} emulation {mode} std {std} koff {koff}", kb.check(name, t, *r[name], w, limit=0.5))
    report(f"mhsa bwd dbq emulation {mode} std {std} koff {koff}", kb.check("dbq", got[3], *r["dbq"], limit=0.5))
    report(f"mhsa bwd dbv emulation {mode} std {std} koff {koff}", kb.check("dbv", got[4], *r["dbv"], limit=0.5))
    report(f"mhsa bwd dbv = colsum(dO) emulation {mode} std {std} koff {koff}", kb.check("dbv from dO", f32(d_o.double().sum(0)).float(), *r["dbv"], limit=0.5))
    if pre:
        # mutant: backward scores built from k c rounded while lse came from q c rounded, on the path that promises identical operands
        bad = attn_bwd_emul(qkv_k, o, d_o, lse, AB, AN, AH, dtype, prescaled=True, mutant="kc_rounded_on_the_flagged_path")
        worst = max(kb.excess(t, *r[name])[0] for name, t in zip(("dk", "dv"), bad[1:3]))
        report(f"mhsa bwd mutant k c rounded on the flagged path std {std} koff {koff}", worst)
        if koff > 0.0 or std > 1.0:           # (diffuse attention without the offset: one rounding of the scores moves P by less than P's own rounding -- 0.53, reported)
            assert worst > 1.0, worst
        # ... the plain path's bound allows exactly that
        rp = kb.mhsa_bwd_ref(seen, d_o, AB, AN, AH, SCALE, dtype, plain=True)
        for name, t in zip(("dk", "dv"), bad[1:3]):
            kb.check("plain bound, " + name, t, *rp[name], w)


# ------------------------------------------------------------------------------------------------ attention dropout
DROP_SEED = 0x5DEECE66D1234567


def drop_mask64(keep, B=AB, N=AN, H=AH, seed=DROP_SEED):
    from oracle import ref_cpu
    return ref_cpu.attn_drop_mask(keep, seed, B, H, N).double()


def flip_in_the_small_head(mask, qkv, B, N, H):
    """mutant (a): ONE mask element flipped (dropped <-> kept), in head 0 (V scaled 2^-6) of batch entry 0, at the last query and that row's most probable key"""
    q, k, _ = (t.double() for t in split(qkv, B, N, H))
    j = int(torch.argmax(q[0, 0, N - 1] @ k[0, 0].t()))
    bad = mask.clone()
    bad[0, 0, N - 1, j] = 0.0 if float(mask[0, 0, N - 1, j]) > 0 else float(mask.max())
    return bad


@pytest.mark.parametrize("std,koff", kb.ATTN_GENERATORS)
@pytest.mark.parametrize("keep", [0.9, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_attention_dropout(dtype, keep, std, koff):
    """forward and backward under the dropout mask of oracle.ref_cpu.attn_drop_mask: ideal <= 1, emulation <= 0.5, and the three mutants of a dropout kernel --
    (a) one flipped mask element in the small head, (b) the normaliser taken from the dropped probabilities, (c) dP left unmasked in the backward -- exceed 1 on
    the offset-free generators (reported on the key-offset one, whose bound's score term allows more: kernel_bounds.ATTN_GENERATORS)"""
    qkv, d_o = kb.attention_inputs(AB, AN, AH, dtype, logit_std=std, seed=80, key_offset=koff)
    mask = drop_mask64(keep)
    assert set(torch.unique(mask).tolist()) == {0.0, float(torch.tensor(1.0) / torch.tensor(keep))}
    w = lambda i: kb.where_attn(i, AN, AH)  # noqa: E731
    tag = f"{dtype} keep {keep} std {std} koff {koff}"
    rf = kb.mhsa_fwd_ref(qkv, AB, AN, AH, SCALE, dtype, mask=mask)
    o, lse = attn_fwd_emul(qkv, AB, AN, AH, dtype, mask=mask)
    report(f"mhsa dropout fwd ideal {tag}", kb.check("ideal", rf["out"][0].to(dtype), *rf["out"], w))
    report(f"mhsa dropout fwd out emulation {tag}", kb.check("out", o, *rf["out"], w, limit=0.5))
    report(f"mhsa dropout fwd lse emulation {tag}", kb.check("lse", lse, *rf["lse"], limit=0.5))
    plain = kb.mhsa_fwd_ref(qkv, AB, AN, AH, SCALE, dtype)
    assert torch.equal(rf["lse"][0], plain["lse"][0]) and torch.equal(rf["lse"][1], plain["lse"][1])          # lse: of the un-dropped p, reference and bound unchanged
    rb = kb.mhsa_bwd_ref(qkv, d_o, AB, AN, AH, SCALE, dtype, mask=mask)
    got = attn_bwd_emul(qkv, o, d_o, lse, AB, AN, AH, dtype, mask=mask)
    for name, t in zip(("dq", "dk", "dv"), got[:3]):
        report(f"mhsa dropout bwd {name} ideal {tag}", kb.check("ideal " + name, rb[name][0].to(dtype), *rb[name], w))
        report(f"mhsa dropout bwd {name} emulation {tag}", kb.check(name, t, *rb[name], w, limit=0.5))
    report(f"mhsa dropout bwd dbq emulation {tag}", kb.check("dbq", got[3], *rb["dbq"], limit=0.5))
    report(f"mhsa dropout bwd dbv emulation {tag}", kb.check("dbv", got[4], *rb["dbv"], limit=0.5))
    # attn_bias_fused = 0: the sums of the stored (rounded) thirds, and their bound
    rs = kb.mhsa_bwd_ref(qkv, d_o, AB, AN, AH, SCALE, dtype, mask=mask, bias_from_stored=True)
    for name, t in (("dbq", got[0]), ("dbv", got[2])):
        report(f"mhsa dropout bwd {name} from the stored tensor {tag}", kb.check(name + " stored", f32(t.double().sum(0)).float(), *rs[name], limit=0.5))
    # mutants
    offset_free = koff == 0.0
    om, _ = attn_fwd_emul(qkv, AB, AN, AH, dtype, mask=flip_in_the_small_head(mask, qkv, AB, AN, AH))
    ra, idx = kb.excess(om, *rf["out"])
    report(f"mhsa dropout mutant one flipped mask element {tag}", ra)
    om, _ = attn_fwd_emul(qkv, AB, AN, AH, dtype, mask=mask, mutant="l_from_the_dropped_p")
    rl = report(f"mhsa dropout mutant l from the dropped p {tag}", kb.excess(om, *rf["out"])[0])
    bad = attn_bwd_emul(qkv, o, d_o, lse, AB, AN, AH, dtype, mask=mask, mutant="dp_left_unmasked")
    rp = report(f"mhsa dropout mutant dP left unmasked {tag}", max(kb.excess(t, *rb[name])[0] for name, t in zip(("dq", "dk"), bad[:2])))
    if offset_free:
        assert ra > 1.0, (ra, w(idx))
        row, col = divmod(idx, AH * 64)
        assert (row, col // 64) == (AN - 1, 0), w(idx)                 # the message names the query and the head
        assert rl > 1.0, rl
        assert rp > 1.0, rp


def test_the_mask_free_attention_references_are_unchanged():
    """mask = None takes the code it always took; an all-ones mask (keep = 1) goes through the masked formulas and gives bitwise the same references and
    bounds -- but for dbv, whose bound drops the colsum(dO) alternative under a mask"""
    qkv, d_o = kb.attention_inputs(AB, AN, AH, BF, logit_std=6.0, seed=80)
    ones = torch.ones(AB, AH, AN, AN, dtype=torch.float64)
    a, b = kb.mhsa_fwd_ref(qkv, AB, AN, AH, SCALE, BF), kb.mhsa_fwd_ref(qkv, AB, AN, AH, SCALE, BF, mask=ones)
    for k in ("out", "lse"):
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]), k
    a, b = kb.mhsa_bwd_ref(qkv, d_o, AB, AN, AH, SCALE, BF), kb.mhsa_bwd_ref(qkv, d_o, AB, AN, AH, SCALE, BF, mask=ones)
    for k in ("dq", "dk", "dv", "dbq", "dbv"):
        assert torch.equal(a[k][0], b[k][0]), k
        assert torch.equal(a[k][1], b[k][1]) or k == "dbv", k
    assert bool((b["dbv"][1] < a["dbv"][1]).all())


# ------------------------------------------------------------------------------------------------ element-wise kernels
EW_N = 1027


@pytest.mark.parametrize("dtype", [BF, F32])
def test_elementwise_emulations(dtype):
    """every element-wise reference against torch CPU fp32 arithmetic with exactly the named roundings: <= 1 under the rigorous bounds, <= 0.5 under SLACK_ACT"""
    a, b = kb.elementwise_inputs(EW_N, dtype, seed=90), kb.elementwise_inputs(EW_N, dtype, seed=91)
    mask = kb.drop_mask(EW_N, 0.9, seed=92)
    af, bf_ = a.float(), b.float()
    report(f"mul_mask emulation {dtype}", kb.check("mul_mask", (af * mask).to(dtype), *kb.mul_mask_ref(a, mask, None, dtype)))
    report(f"mul_mask + b emulation {dtype}", kb.check("mul_mask + b", (af * mask + bf_).to(dtype), *kb.mul_mask_ref(a, mask, b, dtype)))
    if dtype == BF:                                              # mutant: b added after the product was stored
        assert kb.excess(((af * mask).to(BF).float() + bf_).to(BF), *kb.mul_mask_ref(a, mask, b, BF))[0] > 1.0
    report(f"add emulation {dtype}", kb.check("add", (af + bf_).to(dtype), *kb.add_ref(a, b, dtype)))
    x = kb.elementwise_inputs(300 * 764, dtype, seed=93).reshape(300, 764)
    sc = torch.linspace(-1.5, 2.0, 43)
    sc[3] = 0.0
    report(f"row_scale emulation {dtype}", kb.check("row_scale", (x.float() * sc.repeat_interleave(7)[:300, None]).to(dtype), *kb.row_scale_ref(x, sc, 7, dtype)))
    for sd, dd in ((F32, F32), (BF, F32), (F32, BF)):
        if dtype == BF and (sd, dd) == (F32, F32):
            continue
        src = kb.elementwise_inputs(EW_N, sd, seed=94)
        em = (src.float() * torch.tensor(1.0 / 3.0, dtype=F32)).to(dd)
        report(f"cast_scale emulation {sd} -> {dd}", kb.check("cast_scale", em, *kb.cast_scale_ref(src, 1.0 / 3.0, dd)))
    g = kb.elementwise_inputs(EW_N, dtype, seed=95)
    pre = (kb._randn((EW_N,), 96, "cpu") * 1.5).to(dtype)
    y = torch.sigmoid(pre.float()).to(dtype)
    gf, yf, pf = g.float(), y.float(), pre.float()
    report(f"act_bwd sigmoid emulation {dtype}", kb.check("sigmoid", (gf * yf * (1.0 - yf)).to(dtype), *kb.act_bwd_ref(g, y, kb.ACT_SIGMOID, dtype), limit=0.5))
    report(f"act_bwd relu emulation {dtype}", kb.check("relu", torch.where(pf > 0, gf, torch.zeros_like(gf)).to(dtype), *kb.act_bwd_ref(g, pre, kb.ACT_RELU, dtype), limit=0.5))
    report(f"act_bwd gelu emulation {dtype}", kb.check("gelu", act_emul(gf, pre, kb.ACT_DGELU, dtype).to(dtype), *kb.act_bwd_ref(g, pre, kb.ACT_GELU, dtype), limit=0.5))
    # mutant: the derivative of the tanh form
    t = math.sqrt(2 / math.pi) * (pf + 0.044715 * pf ** 3)
    dtanh = 0.5 * (1 + torch.tanh(t)) + 0.5 * pf * (1 - torch.tanh(t) ** 2) * math.sqrt(2 / math.pi) * (1 + 3 * 0.044715 * pf * pf)
    rt = report(f"act_bwd mutant tanh-form dGELU {dtype}", kb.excess((gf * dtanh).to(dtype), *kb.act_bwd_ref(g, pre, kb.ACT_GELU, dtype))[0])
    if dtype == F32:                                             # (bf16: the polynomial's own allowance, 5.5e-4, is of the size of the tanh form's error -- reported)
        assert rt > 1.0, rt
    r = kb.columns_inputs(260, 40, dtype, seed=97)
    report(f"rows_reduce_mod emulation {dtype}", kb.check("rows_reduce_mod", r.float().reshape(52, 5, 40).sum(0), *kb.rows_reduce_mod_ref(r, 5)))


def colsum_emul(x, beta=0.0, out_old=None, mutant=None):
    """the summation tree of devias_colsum in torch fp32: per 256-row block, lane ty sums rows ty, ty + 8, ... in order, the 8 lanes are added in order; the block
    partials i, i + 16, ... are summed per lane and the 16 lanes in order; out = t + beta out_old"""
    v = x.float()
    if mutant == "sums_after_a_bf16_store":
        v = v.to(BF).float()
    M, N = v.shape
    parts = []
    for r0 in range(0, M, 256):
        blk = v[r0:min(M, r0 + 256)]
        if mutant == "last_row_dropped" and r0 + 256 >= M:
            blk = blk[:-1]
        t = torch.zeros(N)
        for ty in range(8):
            s = torch.zeros(N)
            for row in blk[ty::8]:
                s = s + row
            t = t + s
        parts.append(t)
    if len(parts) == 1:
        t = parts[0]
    else:
        t = torch.zeros(N)
        for ly in range(16):
            s = torch.zeros(N)
            for part in parts[ly::16]:
                s = s + part
            t = t + s
    return t + beta * out_old if beta != 0.0 else t


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("M", [1, 256, 257, 4097])
def test_colsum_emulation_and_mutants(M, dtype):
    N = 40
    x = kb.columns_inputs(M, N, dtype, seed=98)
    old = kb._randn((N,), 99, "cpu") * kb.graded(N, 6).float() * 4.0
    for beta in (0.0, 1.0):
        ref, bound = kb.colsum_ref(x, beta, old)
        report(f"colsum emulation M {M} {dtype} beta {beta}", kb.check("colsum", colsum_emul(x, beta, old), ref, bound))
    ref, bound = kb.colsum_ref(x)
    rm = report(f"colsum mutant last row dropped M {M} {dtype}", kb.excess(colsum_emul(x, mutant="last_row_dropped"), ref, bound)[0])
    assert rm > 1.0, rm
    if dtype == F32:
        rm = report(f"colsum mutant sums after a bf16 store M {M}", kb.excess(colsum_emul(x, mutant="sums_after_a_bf16_store"), ref, bound)[0])
        assert rm > 1.0, rm


# ------------------------------------------------------------------------------------------------ what the old metric misses
OLD_TOL_GEMM = 2e-2 * 4            # test_kernels_gpu.py test_gemm_epilogues, bf16: TOL[bf16] * 4
OLD_TOL_ATTN = 2e-2                # test_kernels_gpu.py test_mhsa_fwd_bwd, bf16 out


@pytest.mark.parametrize("mutant", ["kstep_dropped_small_rows", "bias_missing_last_8_cols"])
def test_the_old_metric_passes_wrong_gemms_on_graded_inputs(mutant):
    A, B, bias, res, (ref, bound), small = gemm_case(BF, 6)
    bad = gemm_emul(A, B, bias, res, BF, mutant, small)
    assert rel(bad, ref) < OLD_TOL_GEMM                      # the recorded reason this file exists
    assert kb.excess(bad, ref, bound)[0] > 1.0


def test_the_old_metric_passes_a_dropped_key_in_the_small_head():
    qkv, _ = kb.attention_inputs(AB, AN, AH, BF, logit_std=1.0, seed=60)
    r = kb.mhsa_fwd_ref(qkv, AB, AN, AH, SCALE, BF)
    good, _ = attn_fwd_emul(qkv, AB, AN, AH, BF)
    bad, _ = attn_fwd_emul(qkv, AB, AN, AH, BF, mutant="last_key_dropped_small_head")
    assert rel(bad, r["out"][0]) < OLD_TOL_ATTN and abs(rel(bad, r["out"][0]) - rel(good, r["out"][0])) < 1e-6
    assert kb.excess(bad, *r["out"])[0] > 1.0


@pytest.mark.parametrize("keep", [0.9, 0.5])
def test_the_old_metric_passes_a_flipped_mask_element_in_the_small_head(keep):
    """test_mhsa_dropout_matches_the_reference_with_the_same_mask at its bf16 tolerance does not see one wrong mask element where V is small"""
    qkv, _ = kb.attention_inputs(AB, AN, AH, BF, logit_std=1.0, seed=80)
    mask = drop_mask64(keep)
    r = kb.mhsa_fwd_ref(qkv, AB, AN, AH, SCALE, BF, mask=mask)
    good, _ = attn_fwd_emul(qkv, AB, AN, AH, BF, mask=mask)
    bad, _ = attn_fwd_emul(qkv, AB, AN, AH, BF, mask=flip_in_the_small_head(mask, qkv, AB, AN, AH))
    assert rel(bad, r["out"][0]) < OLD_TOL_ATTN and abs(rel(bad, r["out"][0]) - rel(good, r["out"][0])) < 1e-6
    assert kb.excess(bad, *r["out"])[0] > 1.0
