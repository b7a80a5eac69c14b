"""The accuracy anchor of the kernels (GPU only): every GEMM kernel form, LayerNorm and the attention kernels (with and without dropout) against float64 on graded inputs, each element
held to the first-order bound of tests/kernel_bounds.py (worst |out - ref| / bound <= 1).  The float64 references run in torch on the device: none of this
project's kernels.  Every GEMM / attention call asserts through ops.counters() which kernel served it.  What no counter shows is not asserted: LayerNorm has none
(one kernel family serves it), and none tells whether a persistent launch on static lists cut its tail tiles in thirds (option gemm_tail_split = 3 is set; the
launch is asserted persistent and not on the queues).
Every option a case sets is restored by the `options` fixture of this file.  Each case prints `[bound] <kernel> <shape> <variant> worst ratio ...`."""
import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SCALE = 0.125


@pytest.fixture
def options():
    """the ops module; every process-wide option is put back to the value it had"""
    from devias_amd import ops as o
    with o.options():
        yield o


def cdiv(a, b):
    return -(-a // b)


def say(kernel, shape, variant, ratios):
    print(f"[bound] {kernel} {shape} {variant} worst ratio " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def served(o, fn, **want):
    """run fn() with fresh counters; assert the wanted counters, return (result, counters)"""
    o.counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    cnt = o.counters()
    for k, v in want.items():
        assert cnt[k] == v, (k, v, cnt)
    return out, cnt


# ------------------------------------------------------------------------------------------------ GEMM
def gemm_variant(o, A, B, bias, res, pre, dtype, ta, tb, epi, colsum_from_stored, want, split_k=1):
    """one devias_gemm call in layout (ta, tb) with epilogue `epi`, checked against float64; returns the worst ratios"""
    M, N = A.shape[0], B.shape[0]
    As = A.t().contiguous() if ta else A
    Bs = B.t().contiguous() if tb else B
    kw, rk = {}, {}
    if epi in ("bias", "bias_res", "res", "gelu_aux", "relu", "sigmoid", "res_mod", "res_rowscale", "rowscale_resmod"):
        kw["bias"] = rk["bias"] = bias
    if epi in ("bias_res", "res", "res_rowscale"):
        kw["res"] = rk["res"] = res
    if epi == "res_mod":
        rm = min(10, M)
        kw.update(res=res[:rm].contiguous(), res_mod=rm); rk.update(res=res[:rm], res_mod=rm)
    if epi == "rowscale_resmod":
        rs = (torch.arange(M, device=DEV) % 3).float() * 0.5
        kw.update(res=res[:2].contiguous(), res_mod=2, row_scale=rs, rows_per_scale=1); rk.update(res=res[:2], res_mod=2, row_scale=rs, rows_per_scale=1)
    if epi == "res_rowscale":
        rs = (torch.arange(M // 256, device=DEV) % 3).float() * 0.5
        kw.update(row_scale=rs, rows_per_scale=256); rk.update(row_scale=rs, rows_per_scale=256)
    if epi == "gelu_aux":
        kw.update(act=o.ACT_GELU, aux_out=torch.empty(M, N, dtype=dtype, device=DEV)); rk["act"] = kb.ACT_GELU
    if epi == "relu":
        kw["act"] = o.ACT_RELU; rk["act"] = kb.ACT_RELU
    if epi == "sigmoid":
        kw["act"] = o.ACT_SIGMOID; rk["act"] = kb.ACT_SIGMOID
    if epi in ("dgelu", "dgelu_colsum", "dgelu_colsum_beta1"):
        kw.update(act=o.ACT_DGELU, aux_in=pre); rk.update(act=kb.ACT_DGELU, aux_in=pre)
    cs_old = None
    if epi in ("colsum", "dgelu_colsum"):
        kw["colsum"] = torch.zeros(N, device=DEV)
    if epi == "dgelu_colsum_beta1":
        cs_old = kb.graded(N, 3, DEV).float() * 3.0
        kw.update(colsum=cs_old.clone(), colsum_beta=1.0); rk.update(colsum_old=cs_old, colsum_beta=1.0)
    if split_k != 1:
        kw["split_k"] = split_k
    c, _ = served(o, lambda: o.gemm(As, Bs, trans_a=ta, trans_b=tb, **kw), **want)
    assert c.dtype == dtype and c.shape == (M, N)
    r = kb.gemm_ref(A, B.t(), dtype, colsum_from_stored=colsum_from_stored, **rk)
    tag = f"ta={int(ta)} tb={int(tb)} {epi}"
    where = lambda i: kb.where2d(i, N)  # noqa: E731
    ratios = {"out": kb.check(f"{tag} out", c, *r["out"], where)}
    if "aux_out" in kw:
        ratios["aux"] = kb.check(f"{tag} aux_out", kw["aux_out"], *r["aux"], where)
    if "colsum" in kw:
        ratios["colsum"] = kb.check(f"{tag} colsum", kw["colsum"], *r["colsum"])
    return ratios


def gemm_data(M, N, K, dtype, seed):
    A, B, bias, res = kb.gemm_inputs(M, N, K, dtype, spread=6, seed=seed, device=DEV)
    pre = (kb._randn((M, N), seed + 9, DEV) * 1.5).to(dtype)
    return A, B, bias, res, pre


LAYOUTS = [(False, False), (False, True), (True, True), (True, False)]
EPIS = ["bias_res", "res_mod", "gelu_aux", "dgelu_colsum_beta1"]
EPIS_FUSED = EPIS + ["colsum"]          # the kernels that fuse the column sums: the plain sum too -- the bound that tells sums taken after the bf16 store apart


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,N,K", [(130, 200, 72), (70, 765, 100), (300, 128, 4), (4, 765, 768)])
def test_gemm128(M, N, K, dtype, options):
    """the 128x128 register-staged kernels (ragged / small / fp32 shapes), all four layouts; column sums come from devias_colsum over the stored C here"""
    o = options
    A, B, bias, res, pre = gemm_data(M, N, K, dtype, 100)
    name = "gemm128_f32" if dtype == F32 else "gemm128_bf16"
    for ta, tb in LAYOUTS:
        for epi in EPIS:
            auto_split = (not ta) and M <= 256 and K >= 512 and "colsum" not in epi          # ops.gemm splits K of small-M products itself
            want = {name: 1, "splitk_reduce": int(auto_split), "gemm256": 0, "gemm_ss": 0, "gemm_smallm": 0}
            say(name, (M, N, K), f"ta={int(ta)} tb={int(tb)} {epi}", gemm_variant(o, A, B, bias, res, pre, dtype, ta, tb, epi, True, want))


@pytest.mark.parametrize("epi_form", [1, 0])
@pytest.mark.parametrize("M,N,K", [(512, 512, 192), (256, 768, 64)])
def test_gemm256_one_tile_per_workgroup(M, N, K, epi_form, options):
    """the 256x256 LDS-DMA kernel, one tile per workgroup (at most one round of tiles), register-transposed (1) and LDS-staged (0) epilogue; fused fp32 column sums"""
    o = options
    o.set_option("gemm_epi", epi_form)
    A, B, bias, res, pre = gemm_data(M, N, K, BF, 200)
    for ta, tb in LAYOUTS:
        for epi in EPIS_FUSED:
            want = {"gemm256": 1, "gemm256p": 0, "gemm_ss": 0, "gemm128_bf16": 0, "splitk_reduce": 0}
            say("gemm256", (M, N, K), f"gemm_epi={epi_form} ta={int(ta)} tb={int(tb)} {epi}", gemm_variant(o, A, B, bias, res, pre, BF, ta, tb, epi, False, want))


@pytest.mark.parametrize("M,N,K", [(512, 384, 128), (256, 640, 320)])
def test_gemm_single_stage(M, N, K, options):
    """the 256x128 single-stage kernel (N a multiple of 128, not of 256), the three layouts it has"""
    o = options
    A, B, bias, res, pre = gemm_data(M, N, K, BF, 300)
    for ta, tb in [(False, False), (False, True), (True, True)]:
        for epi in EPIS_FUSED:
            want = {"gemm_ss": 1, "gemm256": 0, "gemm128_bf16": 0, "splitk_reduce": 0}
            say("gemm_ss", (M, N, K), f"ta={int(ta)} tb={int(tb)} {epi}", gemm_variant(o, A, B, bias, res, pre, BF, ta, tb, epi, False, want))


def _persistent_serves(tb, epi):
    """(as in test_kernels_gpu.py: the persistent kernels are compiled per kind of row the epilogue reads)"""
    return epi in (("bias", "plain", "colsum", "gelu_aux", "dgelu_colsum") if tb else ("bias", "plain", "colsum", "gelu_aux", "dgelu_colsum", "res", "res_rowscale"))


@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("epi", ["bias", "res", "gelu_aux", "dgelu_colsum", "plain", "colsum", "res_rowscale"])
@pytest.mark.parametrize("M,N,K", [(256 * 70, 1024, 128), (256 * 131, 512, 64), (256 * 99, 768, 768)])
def test_gemm_persistent(M, N, K, epi, tb, options):
    """the persistent 256x256 kernel: tiles pulled from the dynamic queues, and static tile lists with the tail tiles in thirds; on one shape the generic
    epilogue instantiation too (gemm_epi_spec 0).  Where the persistent kernels do not serve an epilogue the one-tile-per-workgroup kernel must."""
    o = options
    A, B, bias, res, pre = gemm_data(M, N, K, BF, 400)
    serves = _persistent_serves(tb, epi)
    modes = [("dynamic", 1, 2, 1), ("static thirds", 0, 3, 1)] + ([("dynamic generic", 1, 2, 0), ("static generic", 0, 3, 0)] if K == 128 else [])
    for mode, dyn, tail, spec in modes:
        o.set_option("gemm_persistent", 1); o.set_option("gemm_dynamic", dyn); o.set_option("gemm_tail_split", tail); o.set_option("gemm_epi_spec", spec)
        want = {"gemm256p": int(serves), "gemm256": int(not serves), "gemm256w": 0, "gemm256d": int(bool(dyn) and serves and K >= 128)}
        say("gemm256p" if serves else "gemm256", (M, N, K), f"{mode} tb={int(tb)} {epi}", gemm_variant(o, A, B, bias, res, pre, BF, False, tb, epi, False, want))


@pytest.mark.parametrize("epi", ["bias_res", "gelu_aux", "dgelu", "relu", "sigmoid", "plain", "rowscale_resmod"])
@pytest.mark.parametrize("M,N,K", [(64, 768, 3072), (96, 768, 768), (4, 384, 384), (70, 400, 768)])
def test_gemm_small_m(M, N, K, epi, options):
    """the small-M kernel (M <= 128, bf16: the four waves of a workgroup split K), B k-contiguous and its transposing variant"""
    o = options
    A, B, bias, res, pre = gemm_data(M, N, K, BF, 500)
    for tb in (False, True):
        want = {"gemm_smallm": 1, "splitk_reduce": 0, "gemm128_bf16": 0}
        say("gemm_smallm", (M, N, K), f"tb={int(tb)} {epi}", gemm_variant(o, A, B, bias, res, pre, BF, False, tb, epi, True, want))


@pytest.mark.parametrize("dtype", [F32, BF])
def test_gemm_small_m_split_k_reduce(dtype, options):
    """gemm_smallm = 0: the 64-row product split along K, the reduce kernel applying the epilogue"""
    o = options
    o.set_option("gemm_smallm", 0)
    M, N, K = 64, 768, 3072
    A, B, bias, res, pre = gemm_data(M, N, K, dtype, 600)
    for epi in ("bias_res", "gelu_aux", "dgelu", "plain"):
        want = {"splitk_reduce": 1, "gemm_smallm": 0}
        say("splitk_reduce", (M, N, K), f"{dtype} {epi}", gemm_variant(o, A, B, bias, res, pre, dtype, False, False, epi, True, want))


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("R,N,K", [(2048, 96, 160), (4096, 768, 512), (4, 768, 2048)])
def test_wgrad_split_k(R, N, K, dtype, options):
    """weight gradients dW [N, K] (fp32) = dY [R, N]^T X [R, K], the reduction over R split 1 / 3 / 8 ways, beta 0 and 1 (gradient accumulation), and ops.wgrad's own split"""
    o = options
    dY = (kb._randn((R, N), 701, DEV) * kb.graded(N, 6, DEV).float()[None, :] * kb.graded(R, 3, DEV).float()[:, None]).to(dtype)
    X = (kb._randn((R, K), 702, DEV) * kb.graded(K, 6, DEV).float()[None, :]).to(dtype)
    c_old = kb._randn((N, K), 703, DEV) * kb.graded(N, 6, DEV).float()[:, None] * kb.graded(K, 6, DEV).float()[None, :] * 8.0
    bk = 64 if dtype == BF else 16
    # the product's kernel: C [N, K] in full 256 x 256 tiles and the reduction in whole k-tiles -> the 256 x 256 kernel (one tile per workgroup: fp32 C is not
    # offered by the persistent form), otherwise the 128 x 128 one
    big = dtype == BF and N % 256 == 0 and K % 256 == 0 and R % 64 == 0
    kern = {"gemm256": int(big), "gemm256p": 0, "gemm_ss": 0, "gemm128_bf16": int(dtype == BF and not big), "gemm128_f32": int(dtype == F32)}
    where = lambda i: kb.where2d(i, K)  # noqa: E731
    for beta in (0.0, 1.0):
        ref, bound = kb.gemm_ref(dY.t(), X, dtype, out_f32=True, beta=beta, c_old=c_old)["out"]
        for sk in (1, 3, 8):
            eff = cdiv(R, cdiv(cdiv(R, sk), bk) * bk) if sk > 1 else 1                   # (devias_gemm rounds the slabs to whole k-tiles)
            out = c_old.clone()
            served(o, lambda: o.gemm(dY, X, trans_a=True, trans_b=True, out_f32=True, split_k=sk, out=out, beta=beta), splitk_reduce=int(eff > 1), **kern)
            say("wgrad", (R, N, K), f"{dtype} beta={beta} split_k={sk}", {"out": kb.check(f"wgrad beta {beta} split {sk}", out, ref, bound, where)})
        out = c_old.clone()
        sk = o.auto_split_k(N, K, R, bk=bk)
        eff = cdiv(R, cdiv(cdiv(R, sk), bk) * bk) if sk > 1 else 1
        served(o, lambda: o.wgrad(dY, X, out=out, beta=beta), splitk_reduce=int(eff > 1), **kern)
        say("wgrad", (R, N, K), f"{dtype} beta={beta} auto split {sk}", {"out": kb.check(f"ops.wgrad beta {beta}", out, ref, bound, where)})


@pytest.mark.parametrize("dtype", [F32, BF])
def test_gemm_batched(dtype, options):
    """batch > 1 launches (128x128 kernel): the strided shapes of test_gemm_batched_layouts"""
    o = options
    h, dh, D = 4, 512, 384
    name = "gemm128_f32" if dtype == F32 else "gemm128_bf16"
    mk = lambda r, c, s: (kb._randn((r, c), s, DEV) * 0.05 * kb.graded(r, 6, DEV).float()[:, None]).to(dtype)  # noqa: E731
    Wq, Wk, Wv, Wo, g = mk(h * dh, D, 801), mk(h * dh, D, 802), mk(h * dh, D, 803), mk(D, h * dh, 804), mk(h * D, D, 805)
    ratios = {}
    Wqk = torch.empty(h * D, D, dtype=dtype, device=DEV)
    served(o, lambda: o.gemm_batched(Wk, Wq, Wqk, D, D, dh, lda=D, ldb=D, ldc=D, stride_a=dh * D, stride_b=dh * D, stride_c=D * D, batch=h, trans_a=True, trans_b=True), **{name: 1})
    for i in range(h):
        ref, bound = kb.gemm_ref(Wk[i * dh:(i + 1) * dh].t(), Wq[i * dh:(i + 1) * dh], dtype)["out"]
        ratios[f"k^T q [{i}]"] = kb.check(f"Wk^T Wq batch {i}", Wqk[i * D:(i + 1) * D], ref, bound, lambda j: kb.where2d(j, D))
    Wov = torch.empty(D, h * D, dtype=dtype, device=DEV)
    served(o, lambda: o.gemm_batched(Wo, Wv, Wov, D, D, dh, lda=h * dh, ldb=D, ldc=h * D, stride_a=dh, stride_b=dh * D, stride_c=D, batch=h, trans_b=True), **{name: 1})
    for i in range(h):
        ref, bound = kb.gemm_ref(Wo[:, i * dh:(i + 1) * dh], Wv[i * dh:(i + 1) * dh], dtype)["out"]
        ratios[f"o v [{i}]"] = kb.check(f"Wo Wv batch {i}", Wov[:, i * D:(i + 1) * D].contiguous(), ref, bound, lambda j: kb.where2d(j, D))
    dWk = torch.empty(h * dh, D, dtype=torch.float32, device=DEV)
    served(o, lambda: o.gemm_batched(Wq, g, dWk, dh, D, D, lda=D, ldb=D, ldc=D, stride_a=dh * D, stride_b=D * D, stride_c=dh * D, batch=h), **{name: 1})
    for i in range(h):
        ref, bound = kb.gemm_ref(Wq[i * dh:(i + 1) * dh], g[i * D:(i + 1) * D].t(), dtype, out_f32=True)["out"]
        ratios[f"q g^T [{i}]"] = kb.check(f"Wq g^T batch {i}", dWk[i * dh:(i + 1) * dh], ref, bound, lambda j: kb.where2d(j, D))
    say(name, (D, D, dh), f"batched x{h}", ratios)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_CASES = [(M, D, eps, dtype) for (M, D) in [(4, 768), (67, 1024), (130, 384), (257, 512), (1571, 768), (3001, 2048)] for eps in (1e-6, 1e-5) for dtype in (F32, BF)] + \
           [(20011, 768, 1e-6, BF)]                # (once: the ragged rows-per-workgroup grid of the backward)


@pytest.mark.parametrize("M,D,eps,dtype", LN_CASES)
def test_layernorm(M, D, eps, dtype, options):
    """forward (y, mean, rstd) and backward (dx with and without dres, dgamma, dbeta with accumulation, dx_colsum) on graded rows with mean offsets of 0 / 0.5 / 100
    standard deviations and a gamma that crosses zero"""
    o = options
    x, g, b, dy, dres = kb.layernorm_inputs(M, D, dtype, spread=6, seed=900, device=DEV)
    where = lambda i: kb.where2d(i, D)  # noqa: E731
    y, mean, rstd = o.layernorm_fwd(x, g, b, eps)
    r = kb.layernorm_fwd_ref(x, g, b, eps, dtype)
    ratios = {k: kb.check(f"layernorm_fwd {k}", t, *r[k], where if k == "y" else None) for k, t in (("y", y), ("mean", mean), ("rstd", rstd))}
    say("layernorm_fwd", (M, D), f"{dtype} eps={eps}", ratios)
    dg_old, db_old = kb._randn((D,), 901, DEV) * 4.0, kb._randn((D,), 902, DEV) * 4.0
    for with_dres, beta_acc in ((True, 0.0), (False, 1.0)):
        cs = torch.empty(D, device=DEV)
        dx, dg, db = o.layernorm_bwd(dy, x, g, mean, rstd, dres=dres if with_dres else None, dgamma=dg_old.clone(), dbeta=db_old.clone(), beta_acc=beta_acc, dx_colsum=cs)
        r = kb.layernorm_bwd_ref(dy, x, g, mean, rstd, dtype, dres=dres if with_dres else None, dgamma_old=dg_old, dbeta_old=db_old, beta_acc=beta_acc)
        ratios = {k: kb.check(f"layernorm_bwd {k}", t, *r[k], where if k == "dx" else None) for k, t in (("dx", dx), ("dgamma", dg), ("dbeta", db), ("dx_colsum", cs))}
        say("layernorm_bwd", (M, D), f"{dtype} dres={int(with_dres)} beta_acc={beta_acc}", ratios)


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("std,koff", kb.ATTN_GENERATORS)
@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16_prescaled"])
@pytest.mark.parametrize("B,N,H", [(1, 64, 1), (2, 100, 3), (1, 333, 1), (2, 257, 2), (1, 288, 2), (1, 577, 2), (1, 1569, 1)])
def test_mhsa(B, N, H, mode, std, koff, options):
    """forward (out, lse) and backward (dQ, dK, dV per third; dbq / dbv of the _bias entry point) on V and dO graded per head and row, logit std 1, logit std 1 over keys with a common offset, and logit std 6 (kernel_bounds.ATTN_GENERATORS); bf16 also
    with DEVIAS_ATTN_Q_PRESCALED, and with both dK / dV kernels (attn_dkdv 1: one wave per SIMD, with its rest launch of 1 ... 255 keys; 0: two waves per SIMD)"""
    o = options
    dtype = F32 if mode == "f32" else BF
    pre = mode == "bf16_prescaled"
    qkv, d_o = kb.attention_inputs(B, N, H, dtype, logit_std=std, seed=1000, device=DEV, key_offset=koff)
    seen = qkv
    if pre:
        qkv, seen = kb.attention_prescale(qkv, B, N, H, SCALE)
    where = lambda i: kb.where_attn(i, N, H)  # noqa: E731
    fcnt = {"mhsa_fwd_f32": 1} if dtype == F32 else {"mhsa_fwd_bf16": 1, "mhsa_qpre": int(pre)}
    (out, lse), _ = served(o, lambda: o.mhsa_fwd(qkv, B, N, H, SCALE, q_prescaled=pre), **fcnt)
    rf = kb.mhsa_fwd_ref(seen, B, N, H, SCALE, dtype, q_rounded=not pre)
    say("mhsa_fwd", (B, N, H), f"{mode} std={std} koff={koff}", {"out": kb.check("mhsa_fwd out", out, *rf["out"], where), "lse": kb.check("mhsa_fwd lse", lse, *rf["lse"])})
    rb = kb.mhsa_bwd_ref(seen, d_o, B, N, H, SCALE, dtype, plain=not pre)
    D = H * 64
    for form in ((1, 0) if dtype == BF else (1,)):
        o.set_option("attn_dkdv", form)
        if dtype == F32:
            bcnt = {"mhsa_bwd_f32": 1}
        else:
            bcnt = {"mhsa_bwd_bf16": 1, "mhsa_qpre": int(pre), "dkdv1w": int(form == 1 and N >= 256), "dkdv1w_rest": int(form == 1 and N % 256 > 0), "dkdv2w": int(form == 0)}
        dqkv, _ = served(o, lambda: o.mhsa_bwd(qkv, out, d_o, lse, B, N, H, SCALE, q_prescaled=pre), **bcnt)
        g = dqkv.reshape(B * N, 3, D)
        ratios = {name: kb.check(f"mhsa_bwd {name} (attn_dkdv {form})", g[:, i].contiguous(), *rb[name], where) for i, name in enumerate(("dq", "dk", "dv"))}
        dbq, dbv = torch.full((D,), 7.0, device=DEV), torch.full((D,), -3.0, device=DEV)
        dqkv2, _ = served(o, lambda: o.mhsa_bwd(qkv, out, d_o, lse, B, N, H, SCALE, bias_out=(dbq, dbv), q_prescaled=pre), **bcnt)      # the same kernels serve the _bias entry point
        assert torch.equal(dqkv2, dqkv)
        ratios["dbq"] = kb.check("mhsa_bwd_bias dbq", dbq, *rb["dbq"])
        ratios["dbv"] = kb.check("mhsa_bwd_bias dbv", dbv, *rb["dbv"])
        say("mhsa_bwd", (B, N, H), f"{mode} std={std} koff={koff} attn_dkdv={form}", ratios)


# the last two shapes have B H % 8 == 0 (the XCD-aware linear grid); (3, 130, 8) tells a swapped hidx % H / hidx / H apart.  The seed varies with the shape: two
# are below 2^32 (s1 = 0), two have bit 63 set
DROP_SHAPES = {(1, 64, 1): 0x01234567, (2, 100, 3): 0x5DEECE66D1234567, (1, 333, 1): 0x9E3779B97F4A7C15, (2, 321, 4): 0xFFFFFFFF, (3, 130, 8): 0x8000000000000001}


def _drop_run(o, qkv, d_o, B, N, H, drop, fcnt, bcnt, bias=True):
    """forward, backward and (bias) the backward through the _bias entry point with pre-filled destinations (they are overwritten); counters asserted on each"""
    D = H * 64
    (out, lse), _ = served(o, lambda: o.mhsa_fwd(qkv, B, N, H, SCALE, drop=drop), **fcnt)
    dqkv, _ = served(o, lambda: o.mhsa_bwd(qkv, out, d_o, lse, B, N, H, SCALE, drop=drop), **bcnt)
    if not bias:
        return out, lse, dqkv
    dbq, dbv = torch.full((D,), 7.0, device=DEV), torch.full((D,), -3.0, device=DEV)
    dqkv2, _ = served(o, lambda: o.mhsa_bwd(qkv, out, d_o, lse, B, N, H, SCALE, drop=drop, bias_out=(dbq, dbv)), **bcnt)
    assert torch.equal(dqkv2, dqkv)
    return out, lse, dqkv, dbq, dbv


@pytest.mark.parametrize("std,koff", kb.ATTN_GENERATORS)
@pytest.mark.parametrize("keep", [0.9, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,N,H", list(DROP_SHAPES))
def test_mhsa_dropout(B, N, H, dtype, keep, std, koff, options):
    """attention dropout (the DROP instantiations of the four-wave forward, the <2, 4> dQ and the two-wave dK / dV kernel, and of the three fp32 kernels) under the
    mask of oracle.ref_cpu.attn_drop_mask: out, lse, dQ, dK, dV and the bias gradients (from the accumulators, and with attn_bias_fused = 0 from the stored tensor)
    within their float64 bounds; bitwise the same under the plain 3-D grid (attn_xcd = 0) where the XCD-aware one serves, under every attn_cfg, and run to run"""
    from oracle import ref_cpu
    o = options
    for name, v in (("attn_dkdv", 1), ("attn_xcd", 1), ("attn_cfg", 0), ("attn_bias_fused", 1)):
        o.set_option(name, v)
    seed = DROP_SHAPES[(B, N, H)]
    drop = (keep, seed)
    qkv, d_o = kb.attention_inputs(B, N, H, dtype, logit_std=std, seed=1100, device=DEV, key_offset=koff)
    mask = ref_cpu.attn_drop_mask(keep, seed, B, H, N).to(DEV).double()
    where = lambda i: kb.where_attn(i, N, H)  # noqa: E731
    D = H * 64
    if dtype == F32:
        fcnt, bcnt = {"mhsa_fwd_f32": 1, "mhsa_fwd_bf16": 0}, {"mhsa_bwd_f32": 1, "mhsa_bwd_bf16": 0}
    else:                    # dropout overrides attn_dkdv = 1: the two-wave dK / dV kernel
        fcnt, bcnt = {"mhsa_fwd_bf16": 1, "mhsa_qpre": 0}, {"mhsa_bwd_bf16": 1, "mhsa_qpre": 0, "dkdv2w": 1, "dkdv1w": 0, "dkdv1w_rest": 0}
    tag = f"{dtype} keep={keep} std={std} koff={koff}"
    out, lse, dqkv, dbq, dbv = _drop_run(o, qkv, d_o, B, N, H, drop, fcnt, bcnt)
    rf = kb.mhsa_fwd_ref(qkv, B, N, H, SCALE, dtype, mask=mask)
    say("mhsa_dropout fwd", (B, N, H), tag, {"out": kb.check("mhsa_fwd_dropout out", out, *rf["out"], where), "lse": kb.check("mhsa_fwd_dropout lse", lse, *rf["lse"])})
    rb = kb.mhsa_bwd_ref(qkv, d_o, B, N, H, SCALE, dtype, mask=mask)
    g = dqkv.reshape(B * N, 3, D)
    ratios = {name: kb.check(f"mhsa_bwd_dropout {name}", g[:, i].contiguous(), *rb[name], where) for i, name in enumerate(("dq", "dk", "dv"))}
    ratios["dbq"] = kb.check("mhsa_bwd_bias dbq (dropout)", dbq, *rb["dbq"])
    ratios["dbv"] = kb.check("mhsa_bwd_bias dbv (dropout)", dbv, *rb["dbv"])
    with o.options(attn_bias_fused=0):                    # the strided devias_colsum over the dQ and dV thirds of the stored dqkv
        _, _, dqkv_s, dbq_s, dbv_s = _drop_run(o, qkv, d_o, B, N, H, drop, fcnt, bcnt)
    assert torch.equal(dqkv_s, dqkv)
    rs = kb.mhsa_bwd_ref(qkv, d_o, B, N, H, SCALE, dtype, mask=mask, bias_from_stored=True)
    ratios["dbq_stored"] = kb.check("mhsa_bwd_bias dbq (dropout, attn_bias_fused 0)", dbq_s, *rs["dbq"])
    ratios["dbv_stored"] = kb.check("mhsa_bwd_bias dbv (dropout, attn_bias_fused 0)", dbv_s, *rs["dbv"])
    say("mhsa_dropout bwd", (B, N, H), tag, ratios)
    first = (out, lse, dqkv, dbq, dbv)
    if (B * H) % 8 == 0:                                  # "Same bits" on either grid (attn_common.h head_map)
        with o.options(attn_xcd=0):
            again = _drop_run(o, qkv, d_o, B, N, H, drop, fcnt, bcnt)
        for name, a, b in zip(("out", "lse", "dqkv", "dbq", "dbv"), first, again):
            assert torch.equal(a, b), f"attn_xcd 0 / 1 differ in {name}"
    if (B, N, H) == (2, 100, 3):                          # under p.drop only one kernel form exists
        for cfg in (1, 2, 3, 6, 7):
            with o.options(attn_cfg=cfg):
                again = _drop_run(o, qkv, d_o, B, N, H, drop, fcnt, bcnt, bias=False)
            for name, a, b in zip(("out", "lse", "dqkv"), first, again):
                assert torch.equal(a, b), f"attn_cfg {cfg} / 0 differ in {name}"
    # run to run: the mask is a function of the seed
    again = _drop_run(o, qkv, d_o, B, N, H, drop, fcnt, bcnt)
    for name, a, b in zip(("out", "lse", "dqkv", "dbq", "dbv"), first, again):
        assert torch.equal(a, b), f"two runs with the same seed differ in {name}"
    out_next, _ = o.mhsa_fwd(qkv, B, N, H, SCALE, drop=(keep, seed + 1))
    assert not torch.equal(out_next, out)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("B,N,H", [(2, 100, 3), (2, 321, 4)])
def test_mhsa_dropout_keep_one_is_no_dropout(B, N, H, dtype, options):
    """drop = (1.0, seed): the plain kernels serve (by counters: under attn_dkdv = 1 the one-wave dK / dV kernel, under 0 the two-wave one) and give bitwise the
    results of the entry points without dropout under the same option value"""
    o = options
    qkv, d_o = kb.attention_inputs(B, N, H, dtype, logit_std=6.0, seed=1200, device=DEV)
    drop = (1.0, DROP_SHAPES[(B, N, H)])
    for form in ((1, 0) if dtype == BF else (1,)):
        o.set_option("attn_dkdv", form)
        if dtype == F32:
            fcnt, bcnt = {"mhsa_fwd_f32": 1}, {"mhsa_bwd_f32": 1}
        else:
            fcnt = {"mhsa_fwd_bf16": 1}
            bcnt = {"mhsa_bwd_bf16": 1, "dkdv1w": int(form == 1 and N >= 256), "dkdv1w_rest": int(form == 1 and N % 256 > 0), "dkdv2w": int(form == 0)}
        out, lse, dqkv, dbq, dbv = _drop_run(o, qkv, d_o, B, N, H, drop, fcnt, bcnt)
        out_p, lse_p, dqkv_p, dbq_p, dbv_p = _drop_run(o, qkv, d_o, B, N, H, None, fcnt, bcnt)
        for name, a, b in zip(("out", "lse", "dqkv", "dbq", "dbv"), (out, lse, dqkv, dbq, dbv), (out_p, lse_p, dqkv_p, dbq_p, dbv_p)):
            assert torch.equal(a, b), f"keep = 1 differs from the plain entry point in {name} (attn_dkdv {form})"
