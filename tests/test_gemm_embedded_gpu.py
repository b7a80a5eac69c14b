"""The addressing half of the devias_gemm ABI (GPU only): every kernel family on operands EMBEDDED in larger allocations (tests/embedded_operands.py) -- leading
dimensions that differ from the widths (and from each other: ldc, ld_aux and ldr get three different paddings, lda != ldb, so one stride used in another's place
cannot cancel), bases that are only 8-byte or not at all aligned, NaN behind and between the rows of every input, a bitwise canary around every output.  ops.gemm
refuses non-contiguous tensors, so the calls go through embedded_operands.gemm_raw.  Per case:
  (a) every output (C, aux_out, column sums) within the float64 bound of tests/kernel_bounds.py on dense copies of the views (ratio <= 1; a NaN read from padding fails it);
  (b) the canary outside every output view bitwise intact, every input buffer bitwise unchanged;
  (c) `pad16` (the alignment class of the dense call): the same counters and bitwise the dense call's outputs -- the same kernel, the same arithmetic per element;
  (d) beta == 0: C (pre-filled with NaN inside the view) comes back finite (part of (a): a non-finite output is infinitely wrong).
Every call asserts its family through the counters; the expected family of a misaligned call comes from the launcher's predicates restated in
embedded_operands.gemm_predicates, not from a run.  Shapes are those of tests/test_kernel_bounds_gpu.py.  Each case prints `[bound] <kernel> <shape> <variant> worst ratio ...`."""
import pytest
import torch

import embedded_operands as eo
import kernel_bounds as kb
from test_kernel_bounds_gpu import BF, DEV, F32, LAYOUTS, EPIS, EPIS_FUSED, _persistent_serves, cdiv, gemm_data, options, say, served  # noqa: F401  (options: a fixture)

pytestmark = pytest.mark.gpu

DENSE = {k: ("dense", 1) for k in ("A", "B", "C", "aux", "res")}
ALL_PAD16 = {"A": ("pad16", 1), "B": ("pad16", 2), "C": ("pad16", 1), "aux": ("pad16", 2), "res": ("pad16", 3)}      # ldc + 8, ld_aux + 16, ldr + 24; lda != ldb
SINGLES = {who: {**DENSE, who: ("pad16", 1)} for who in ("C", "aux", "res")}                                           # one stride at a time


def every(name):
    return {k: (name, k2) for k, (_, k2) in ALL_PAD16.items()}


def vector_band(t=None, n=None):
    """an fp32 vector inside a canary band; t = None: pre-filled with NaN (an output the call must not read)"""
    src = t.reshape(1, -1) if t is not None else torch.full((1, n), eo.NAN, device=DEV)
    buf, view = eo.embed(src.float(), src.shape[1], 64, eo.TAIL_ROWS, eo.CANARY)
    return buf, view[0]


class Case:
    """one devias_gemm call in layout (ta, tb) with epilogue `epi` on operands embedded as `lay` says ({operand: (embedding, k)})"""

    def __init__(self, data, dtype, ta, tb, epi, lay, *, out_f32=False, beta=0.0, c_old=None, split_k=1):
        A, B, bias, res, pre = data
        self.M, self.N, self.K = M, N, K = A.shape[0], B.shape[0], A.shape[1]
        self.dtype, self.ta, self.tb, self.epi, self.lay = dtype, ta, tb, epi, lay
        self.inputs, self.outputs, self.kw, self.rk = {}, {}, {}, {}
        put = lambda name, t, who: self._input(name, t, lay[who])      # noqa: E731
        self.A = put("A", A.t().contiguous() if ta else A, "A")
        self.B = put("B", B.t().contiguous() if tb else B, "B")
        kw, rk = self.kw, self.rk
        kw.update(trans_a=ta, trans_b=tb, split_k=split_k, beta=beta)
        if epi in ("bias", "bias_res", "res", "gelu_aux", "res_mod", "res_rowscale", "rowscale_resmod"):
            kw["bias"] = rk["bias"] = bias
        if epi in ("bias_res", "res", "res_rowscale"):
            kw["res"] = put("res", res, "res"); rk["res"] = res
        if epi == "res_mod":
            rm = min(10, M)
            kw.update(res=put("res", res[:rm].contiguous(), "res"), res_mod=rm); rk.update(res=res[:rm], res_mod=rm)
        if epi == "rowscale_resmod":
            rs = (torch.arange(M, device=DEV) % 3).float() * 0.5
            kw.update(res=put("res", res[:2].contiguous(), "res"), res_mod=2, row_scale=rs, rows_per_scale=1); rk.update(res=res[:2], res_mod=2, row_scale=rs, rows_per_scale=1)
        if epi == "res_rowscale":
            rs = (torch.arange(M // 256, device=DEV) % 3).float() * 0.5
            kw.update(row_scale=rs, rows_per_scale=256); rk.update(row_scale=rs, rows_per_scale=256)
        if epi == "gelu_aux":
            kw.update(act=kb.ACT_GELU, aux_out=self._output("aux", (M, N), dtype, lay["aux"])); rk["act"] = kb.ACT_GELU
        if epi in ("dgelu", "dgelu_colsum", "dgelu_colsum_beta1"):
            kw.update(act=kb.ACT_DGELU, aux_in=put("aux_in", pre, "aux")); rk.update(act=kb.ACT_DGELU, aux_in=pre)
        if epi in ("colsum", "dgelu_colsum"):
            self.cs_buf, kw["colsum"] = vector_band(n=N)
        if epi == "dgelu_colsum_beta1":
            cs_old = kb.graded(N, 3, DEV).float() * 3.0
            self.cs_buf, kw["colsum"] = vector_band(t=cs_old)
            kw["colsum_beta"] = 1.0; rk.update(colsum_old=cs_old, colsum_beta=1.0)
        cdt = F32 if out_f32 else dtype
        self.C = self._output("C", (M, N), cdt, lay["C"], inside=c_old if beta != 0.0 else None)
        if out_f32:
            rk.update(out_f32=True, beta=beta, c_old=c_old)

    def _input(self, name, t, how):
        buf, view, ld, lead = eo.embed_as(t, how[0], k=how[1], fill=eo.NAN)
        self.inputs[name] = (buf, buf.clone())
        return view

    def _output(self, name, shape, dtype, how, inside=None):
        src = inside if inside is not None else torch.full(shape, eo.NAN, dtype=dtype, device=DEV)      # an output the call must not read holds NaN
        buf, view, ld, lead = eo.embed_as(src, how[0], k=how[1], fill=eo.CANARY)
        self.outputs[name] = (buf, shape, ld, lead)
        return view

    def args(self):
        return eo.fill_gemm_args(self.A, self.B, self.C, **self.kw)

    def run(self, o, want):
        _, self.cnt = served(o, lambda: eo.gemm_raw(o, self.A, self.B, self.C, **self.kw), **want)
        return self

    def results(self):
        out = {"out": self.C}
        if "aux_out" in self.kw:
            out["aux"] = self.kw["aux_out"]
        if "colsum" in self.kw:
            out["colsum"] = self.kw["colsum"]
        return out

    def check(self, ref, tag):
        """(a), (b), (d); returns the worst ratios"""
        where = lambda i: kb.where2d(i, self.N)  # noqa: E731
        ratios = {k: kb.check(f"{tag} {k}", t.contiguous(), *ref[k], where if k != "colsum" else None) for k, t in self.results().items()}
        for name, (buf, shape, ld, lead) in self.outputs.items():
            assert eo.intact(buf, shape, ld, lead, eo.CANARY), f"{tag}: a store outside the {name} view"
        if "colsum" in self.kw:
            assert eo.intact(self.cs_buf, (1, self.N), self.N, 64, eo.CANARY), f"{tag}: a store outside the column sums"
        for name, (buf, before) in self.inputs.items():
            assert eo.same_bits(buf, before), f"{tag}: input {name} (or what lies around it) was written"
        return ratios

    def same_as(self, dense, tag):
        """(c)"""
        assert self.cnt == dense.cnt, (tag, self.cnt, dense.cnt)
        for (k, a), b in zip(self.results().items(), dense.results().values()):
            assert eo.same_bits(a.contiguous(), b.contiguous()), f"{tag}: {k} differs from the dense call's"


def reference(case, data, colsum_from_stored):
    """the float64 reference of a Case's epilogue over the dense operands (the same for every layout and embedding)"""
    return kb.gemm_ref(data[0], data[1].t(), case.dtype, colsum_from_stored=colsum_from_stored, **case.rk)


def sweep(o, name, data, dtype, layouts, epis, embeddings, want, colsum_from_stored, variant=""):
    """dense + the given embeddings of every (layout, epilogue); pad16 embeddings are also held bitwise to the dense call"""
    M, N, K = data[0].shape[0], data[1].shape[0], data[0].shape[1]
    for epi in epis:
        ref = None
        for ta, tb in layouts:
            tag = f"{variant}ta={int(ta)} tb={int(tb)} {epi}"
            dense = Case(data, dtype, ta, tb, epi, DENSE).run(o, want(ta, tb, epi))
            ref = ref if ref is not None else reference(dense, data, colsum_from_stored)
            say(name, (M, N, K), f"{tag} dense", dense.check(ref, f"{tag} dense"))
            for label, lay in embeddings.items():
                if label in ("aux", "res") and not any(k in dense.kw for k in {"aux": ("aux_in", "aux_out"), "res": ("res",)}[label]):
                    continue                                          # (this epilogue has no such operand)
                c = Case(data, dtype, ta, tb, epi, lay)
                fam = eo.gemm_predicates(c.args(), {n: o.get_option(n) for n in ("gemm256", "gemm_ss", "gemm_smallm")})["family"]
                if all(v[0] in ("dense", "pad16") for v in lay.values()):
                    c.run(o, want(ta, tb, epi))
                    assert fam == eo.gemm_predicates(dense.args(), {n: o.get_option(n) for n in ("gemm256", "gemm_ss", "gemm_smallm")})["family"]
                    r = c.check(ref, f"{tag} {label}")
                    c.same_as(dense, f"{tag} {label}")
                else:                                                 # the family the predicates imply
                    c.run(o, {fam: 1, **{k: 0 for k in ("gemm256", "gemm_ss", "gemm_smallm", "gemm128_bf16", "gemm128_f32", "gemm256p") if k != fam}})
                    csf = colsum_from_stored or fam.startswith("gemm128")
                    r = c.check(ref if csf == colsum_from_stored else reference(c, data, csf), f"{tag} {label}")
                say(fam, (M, N, K), f"{tag} {label}", r)


PAD16_SET = {"pad16": ALL_PAD16, **SINGLES}


# ------------------------------------------------------------------------------------------------ 128 x 128
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,N,K", [(130, 200, 72), (300, 128, 4)])
def test_gemm128_embedded(M, N, K, dtype, options):
    """the 128 x 128 register-staged kernels under all five embeddings (vector, 4-wide and scalar staging / epilogue paths on a shape that is itself ragged)"""
    o = options
    name = "gemm128_f32" if dtype == F32 else "gemm128_bf16"
    data = gemm_data(M, N, K, dtype, 100)
    want = lambda ta, tb, epi: {name: 1, "splitk_reduce": 0, "gemm256": 0, "gemm_ss": 0, "gemm_smallm": 0}      # noqa: E731
    sweep(o, name, data, dtype, LAYOUTS, EPIS, {**PAD16_SET, **{n: every(n) for n in ("ld4", "base8", "odd")}}, want, True)


# ------------------------------------------------------------------------------------------------ 256 x 256, one tile per workgroup; 256 x 128 single stage
@pytest.mark.parametrize("epi_form", [1, 0])
def test_gemm256_one_tile_per_workgroup_embedded(epi_form, options):
    o = options
    o.set_option("gemm_epi", epi_form)
    data = gemm_data(512, 512, 192, BF, 200)
    want = lambda ta, tb, epi: {"gemm256": 1, "gemm256p": 0, "gemm_ss": 0, "gemm128_bf16": 0, "splitk_reduce": 0}      # noqa: E731
    sweep(o, "gemm256", data, BF, LAYOUTS, EPIS_FUSED, PAD16_SET, want, False, f"gemm_epi={epi_form} ")


def test_gemm_single_stage_embedded(options):
    o = options
    data = gemm_data(512, 384, 128, BF, 300)
    want = lambda ta, tb, epi: {"gemm_ss": 1, "gemm256": 0, "gemm128_bf16": 0, "splitk_reduce": 0}      # noqa: E731
    sweep(o, "gemm_ss", data, BF, [(False, False), (False, True), (True, True)], EPIS_FUSED, PAD16_SET, want, False)


@pytest.mark.parametrize("who", ["A", "B", "C", "side"])
@pytest.mark.parametrize("emb", ["ld4", "base8", "odd"])
def test_misaligned_operand_of_a_well_shaped_problem_falls_back(emb, who, options):
    """(512, 512, 192) bf16 tiles into the 256 x 256 kernel; with ONE operand at ld % 8 != 0, on an 8-byte base or at an odd stride and base the predicates of gemm_impl
    hand it to the 128 x 128 kernel (vector, 4-wide or scalar paths), which must hold the same bounds and guards.  `side`: the residual or the saved pre-activation."""
    o = options
    data = gemm_data(512, 512, 192, BF, 200)
    lays = {f"{emb} on {who}": {**DENSE, **({"aux": (emb, 1), "res": (emb, 1)} if who == "side" else {who: (emb, 1)})}}
    want = lambda ta, tb, epi: {"gemm256": 1, "gemm128_bf16": 0}      # noqa: E731   (the dense control)
    sweep(o, "gemm256", data, BF, [(False, False), (True, True)], EPIS, lays, want, False)


# ------------------------------------------------------------------------------------------------ persistent 256 x 256 (eight waves: static thirds, dynamic queues; four waves)
PERSISTENT_MODES = [("dynamic", 1, 2, 1, 0), ("static thirds", 0, 3, 1, 0), ("static generic", 0, 3, 0, 0), ("four-wave", 0, 2, 1, 15)]


@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize("M,N,K,epis", [(256 * 70, 1024, 128, ("bias", "plain", "colsum", "gelu_aux", "dgelu_colsum", "res", "res_rowscale")), (256 * 99, 768, 768, ("res", "dgelu_colsum"))])
def test_gemm_persistent_embedded(M, N, K, epis, tb, options):
    """the persistent kernels (their epilogue stores are issued from byte offsets built from ldc / ld_aux, the rows they read are fetched ahead at ldr / ld_aux): the
    dynamic queues, static lists with the tail in thirds, on the first shape also the generic epilogue instantiation and the four-wave kernel (gemm_w4 = 15, as
    tests/test_kernels_gpu.py reaches it)"""
    o = options
    data = gemm_data(M, N, K, BF, 400)
    for epi in epis:
        if not _persistent_serves(tb, epi):
            continue
        ref = None
        for mode, dyn, tail, spec, w4 in PERSISTENT_MODES[:(4 if K == 128 else 2)]:
            for n, v in (("gemm_persistent", 1), ("gemm_dynamic", dyn), ("gemm_tail_split", tail), ("gemm_epi_spec", spec), ("gemm_w4", w4)):
                o.set_option(n, v)
            w4_serves = bool(w4) and not (not tb and epi == "dgelu_colsum")
            want = {"gemm256p": 1, "gemm256": 0, "gemm256w": int(w4_serves), "gemm256d": int(bool(dyn) and K >= 128), "gemm128_bf16": 0}
            tag = f"{mode} tb={int(tb)} {epi}"
            dense = Case(data, BF, False, tb, epi, DENSE).run(o, want)
            ref = ref if ref is not None else reference(dense, data, False)
            say("gemm256p", (M, N, K), f"{tag} dense", dense.check(ref, f"{tag} dense"))
            for label, lay in PAD16_SET.items():
                if label in SINGLES and (mode != "static thirds" or (label != "C" and not any(k in dense.kw for k in {"aux": ("aux_in", "aux_out"), "res": ("res",)}[label]))):
                    continue                                          # (one stride at a time: on the static lists; the other modes share that epilogue code)
                c = Case(data, BF, False, tb, epi, lay).run(o, want)
                say("gemm256p", (M, N, K), f"{tag} {label}", c.check(ref, f"{tag} {label}"))
                c.same_as(dense, f"{tag} {label}")


# ------------------------------------------------------------------------------------------------ small M
@pytest.mark.parametrize("form,tb", [(1, False), (1, True), (2, False)])
@pytest.mark.parametrize("M,N,K", [(4, 384, 384), (70, 400, 768), (64, 768, 3072)])
def test_gemm_small_m_embedded(M, N, K, form, tb, options):
    """the small-M kernel in both launcher forms (gemm_smallm 1: a workgroup per row tile, and the transposing variant; 2: the default); it accepts ldc % 4 and 8-byte
    bases on C, res and aux, so `ld4` and `base8` on those stay with it (by the predicates)"""
    o = options
    o.set_option("gemm_smallm", form)
    data = gemm_data(M, N, K, BF, 500)
    want = lambda ta, tb_, epi: {"gemm_smallm": 1, "splitk_reduce": 0, "gemm128_bf16": 0}      # noqa: E731
    embeddings = dict(PAD16_SET)
    for emb in ("ld4", "base8"):
        embeddings[f"{emb} on C, res, aux"] = {**DENSE, "C": (emb, 1), "res": (emb, 1), "aux": (emb, 1)}
    sweep(o, "gemm_smallm", data, BF, [(False, tb)], ["bias_res", "gelu_aux", "dgelu", "rowscale_resmod"], embeddings, want, True, f"gemm_smallm={form} ")
    for emb in ("ld4", "base8"):          # (what the sweep asserted per call: the predicates keep these with the small-M kernel)
        c = Case(data, BF, False, tb, "bias_res", embeddings[f"{emb} on C, res, aux"])
        assert eo.gemm_predicates(c.args(), {"gemm_smallm": form})["family"] == "gemm_smallm"


# ------------------------------------------------------------------------------------------------ split-K into fp32 C
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("R,N,K", [(2048, 96, 160), (4096, 768, 512)])
def test_split_k_into_embedded_f32_c(R, N, K, dtype, options):
    """dW [N, K] (fp32) = dY^T X split 1 / 3 / 8 ways, beta 0 and 1: with C dense the plain reduce serves, with C embedded (ldc != N) the generic one; both within the
    bound, guards intact, and within each other's bound of one another"""
    o = options
    dY = (kb._randn((R, N), 701, DEV) * kb.graded(N, 6, DEV).float()[None, :] * kb.graded(R, 3, DEV).float()[:, None]).to(dtype)
    X = (kb._randn((R, K), 702, DEV) * kb.graded(K, 6, DEV).float()[None, :]).to(dtype)
    c_old = kb._randn((N, K), 703, DEV) * kb.graded(N, 6, DEV).float()[:, None] * kb.graded(K, 6, DEV).float()[None, :] * 8.0
    data = (dY.t().contiguous(), X.t().contiguous(), None, None, None)          # A [M = N, K = R] and B [N = K, K = R] as Case wants them; both stored transposed
    bk = 64 if dtype == BF else 16
    big = dtype == BF and N % 256 == 0 and K % 256 == 0 and R % 64 == 0
    kern = {"gemm256": int(big), "gemm256p": 0, "gemm_ss": 0, "gemm128_bf16": int(dtype == BF and not big), "gemm128_f32": int(dtype == F32)}
    for beta in (0.0, 1.0):
        ref = kb.gemm_ref(dY.t(), X, dtype, out_f32=True, beta=beta, c_old=c_old)
        for sk in (1, 3, 8):
            eff = cdiv(R, cdiv(cdiv(R, sk), bk) * bk) if sk > 1 else 1
            got = {}
            for label, lay in (("dense", DENSE), ("pad16", ALL_PAD16)):
                c = Case(data, dtype, True, True, "plain", {**DENSE, "C": lay["C"]}, out_f32=True, beta=beta, c_old=c_old, split_k=sk)
                q = eo.gemm_predicates(c.args())
                assert q["split"] == eff and q["plain_reduce"] == (eff > 1 and label == "dense"), (label, sk, q)
                c.run(o, {"splitk_reduce": int(eff > 1), **kern})
                tag = f"{dtype} beta={beta} split_k={sk} C {label}"
                say("wgrad", (R, N, K), tag, c.check(ref, tag))
                got[label] = c.C.contiguous()
            kb.check(f"beta={beta} split_k={sk}: embedded against dense C", got["pad16"], got["dense"].double(), 2.0 * ref["out"][1], lambda i: kb.where2d(i, K))


# ------------------------------------------------------------------------------------------------ batched launches
def _batched_intact(buf, views, fill):
    """views: [(shape, ld, lead)]; everything of buf outside all of them holds the fill"""
    out = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for shape, ld, lead in views:
        out &= eo.outside(buf, shape, ld, lead)
    want = torch.full((1,), fill, dtype=buf.dtype, device=buf.device)
    return bool((eo._bits(buf[out]) == eo._bits(want)).all())


def _problems(ts, ld, stride, fill, lead=64):
    """the 2-D tensors ts (one per problem, same shape) at row stride ld, problem i starting lead + i stride elements in: (buf, [views], [(shape, ld, lead_i)])"""
    R, W = ts[0].shape
    n = len(ts)
    buf = torch.full((lead + (n - 1) * stride + (R + eo.TAIL_ROWS) * ld,), fill, dtype=ts[0].dtype, device=DEV)
    views, where = [], []
    for i, t in enumerate(ts):
        v = buf.as_strided((R, W), (ld, 1), lead + i * stride)
        v.copy_(t)
        views.append(v); where.append(((R, W), ld, lead + i * stride))
    return buf, views, where


@pytest.mark.parametrize("dtype", [F32, BF])
def test_gemm_batched_embedded(dtype, options):
    """the three batch > 1 forms of test_gemm_batched at h = 4, dh = 128, D = 128 (the same kernel and vec / vc classes: tests/test_embedded_operands_cpu.py), every batch
    stride widened: problems that follow one another get a band of 256 rows between them, problems that sit side by side in one row get 8 padding columns -- NaN for A
    and B, the canary for C"""
    from devias_amd import _lib
    import ctypes
    o = options
    h, dh, D, PADC = 4, 128, 128, 8
    name = "gemm128_f32" if dtype == F32 else "gemm128_bf16"
    mk = lambda r, c, s: (kb._randn((r, c), s, DEV) * 0.05 * kb.graded(r, 6, DEV).float()[:, None]).to(dtype)  # noqa: E731
    Wq, Wk, Wv, Wo, g = mk(h * dh, D, 801), mk(h * dh, D, 802), mk(h * dh, D, 803), mk(D, h * dh, 804), mk(h * D, D, 805)
    rows = lambda t, n: [t[i * n:(i + 1) * n] for i in range(h)]      # noqa: E731
    cols = lambda t, n: [t[:, i * n:(i + 1) * n] for i in range(h)]      # noqa: E731
    band = eo.TAIL_ROWS * D

    def launch(A, B, C, M, N, K, ta, tb, c_f32, tag):
        (abuf, av, aw), (bbuf, bv, bw), (cbuf, cv, cw) = A, B, C
        a = _lib.GemmArgs()
        a.A, a.B, a.C = av[0].data_ptr(), bv[0].data_ptr(), cv[0].data_ptr()
        a.M, a.N, a.K, a.lda, a.ldb, a.ldc = M, N, K, aw[0][1], bw[0][1], cw[0][1]
        a.trans_a, a.trans_b, a.dtype, a.c_f32, a.split_k = int(ta), int(tb), o.dt_code(dtype), int(c_f32), 1
        a.batch, a.stride_a, a.stride_b, a.stride_c = h, aw[1][2] - aw[0][2], bw[1][2] - bw[0][2], cw[1][2] - cw[0][2]
        q = eo.gemm_predicates(a)
        assert q["family"] == name and q["vec"] and q["vc"], q
        before = (abuf.clone(), bbuf.clone())
        served(o, lambda: _lib.check(_lib.load().devias_gemm(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "devias_gemm(batched)"), **{name: 1})
        assert _batched_intact(cbuf, cw, eo.CANARY), f"{tag}: a store outside the C views"
        assert eo.same_bits(abuf, before[0]) and eo.same_bits(bbuf, before[1]), f"{tag}: an input was written"
        return cv

    nanC = lambda r, c, dt: [torch.full((r, c), eo.NAN, dtype=dt, device=DEV) for _ in range(h)]      # noqa: E731
    ratios = {}
    # Wqk_i [D, D] = Wk_i^T Wq_i: A_i, B_i stored [dh, D], problems one after another
    cv = launch(_problems(rows(Wk, dh), D, dh * D + band, eo.NAN), _problems(rows(Wq, dh), D, dh * D + band, eo.NAN), _problems(nanC(D, D, dtype), D, D * D + band, eo.CANARY),
                D, D, dh, True, True, False, "Wk^T Wq")
    for i in range(h):
        ref, bound = kb.gemm_ref(Wk[i * dh:(i + 1) * dh].t(), Wq[i * dh:(i + 1) * dh], dtype)["out"]
        ratios[f"k^T q [{i}]"] = kb.check(f"Wk^T Wq batch {i}", cv[i].contiguous(), ref, bound, lambda j: kb.where2d(j, D))
    # Wov_i [D, D] = Wo[:, i] Wv_i: A_i and C_i side by side in the rows of Wo / Wov
    cv = launch(_problems(cols(Wo, dh), h * (dh + PADC), dh + PADC, eo.NAN), _problems(rows(Wv, dh), D, dh * D + band, eo.NAN),
                _problems(nanC(D, D, dtype), h * (D + PADC), D + PADC, eo.CANARY), D, D, dh, False, True, False, "Wo Wv")
    for i in range(h):
        ref, bound = kb.gemm_ref(Wo[:, i * dh:(i + 1) * dh], Wv[i * dh:(i + 1) * dh], dtype)["out"]
        ratios[f"o v [{i}]"] = kb.check(f"Wo Wv batch {i}", cv[i].contiguous(), ref, bound, lambda j: kb.where2d(j, D))
    # dWk_i [dh, D] (fp32) = Wq_i g_i^T
    cv = launch(_problems(rows(Wq, dh), D, dh * D + band, eo.NAN), _problems(rows(g, D), D, D * D + band, eo.NAN), _problems(nanC(dh, D, F32), D, dh * D + band, eo.CANARY),
                dh, D, D, False, False, True, "Wq g^T")
    for i in range(h):
        ref, bound = kb.gemm_ref(Wq[i * dh:(i + 1) * dh], g[i * D:(i + 1) * D].t(), dtype, out_f32=True)["out"]
        ratios[f"q g^T [{i}]"] = kb.check(f"Wq g^T batch {i}", cv[i].contiguous(), ref, bound, lambda j: kb.where2d(j, D))
    say(name, (D, D, dh), f"batched x{h}, widened strides", ratios)
