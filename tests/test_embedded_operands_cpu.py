"""tests/embedded_operands.py checked on the CPU (the helper of tests/test_gemm_embedded_gpu.py): embed() yields the stride, offset and alignment class it is asked for,
intact() sees one changed element anywhere outside the view and ignores the view, a wrong "kernel" that ignores the leading dimension is caught under every embedding
but the dense one -- the condition under which the GPU checks can fail at all -- and the launcher's predicates restated in Python name the families the GPU tests
expect.  Also here, because validation precedes any launch and needs no GPU: devias_gemm and devias_wgrad_group refuse leading dimensions smaller than the rows they
stride over, with the field named and no counter moved."""
import ctypes

import pytest
import torch

import embedded_operands as eo

BF, F32 = torch.bfloat16, torch.float32


def _t(R, W, dtype):
    return (torch.arange(R * W, dtype=torch.float32).reshape(R, W) % 251 - 125).to(dtype)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("name", eo.LAYOUTS)
def test_embed_gives_the_requested_stride_offset_and_alignment(name, dtype):
    R, W, es = 5, 24, torch.empty(0, dtype=dtype).element_size()
    t = _t(R, W, dtype)
    buf, view, ld, lead = eo.embed_as(t, name, k=2, fill=eo.CANARY, tail_rows=3)
    assert view.stride() == (ld, 1) and view.storage_offset() == lead and tuple(view.shape) == (R, W)
    assert buf.numel() == lead + (R + 3) * ld and buf.data_ptr() % 16 == 0
    assert view.data_ptr() == buf.data_ptr() + lead * es
    assert torch.equal(view, t)
    assert eo.intact(buf, (R, W), ld, lead)
    want = {"dense": (W, 0, 0), "pad16": (W + 16, 0, 0), "ld4": (W + 4, 0, 0), "base8": (W + 8, 8, 0), "odd": (W + 1, es, es % 8)}[name]
    assert (ld, view.data_ptr() % 16, view.data_ptr() % 8) == want
    if name == "ld4":
        assert ld % 4 == 0 and ld % 8 != 0
    if name == "pad16":
        assert ld % 8 == 0 and eo.layout(name, W, es, 1)[0] == W + 8 and eo.layout(name, W, es, 3)[0] == W + 24


@pytest.mark.parametrize("fill", [eo.CANARY, eo.NAN])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_intact_sees_one_changed_element_outside_the_view_only(dtype, fill):
    R, W, ld, lead, tail = 6, 8, 13, 5, 4
    t = _t(R, W, dtype)
    spots = {"lead": 2, "padding of a middle row": lead + 3 * ld + W, "padding of the last row": lead + (R - 1) * ld + ld - 1,
             "first tail row": lead + R * ld + 1, "last tail row": lead + (R + tail) * ld - 1, "first element": 0}
    for where, idx in spots.items():
        for value in (0.0, -fill if fill == fill else 1.0, eo.CANARY if fill != fill else eo.NAN):
            buf, view = eo.embed(t, ld, lead, tail, fill)
            assert eo.intact(buf, (R, W), ld, lead)
            buf[idx] = value
            assert not eo.intact(buf, (R, W), ld, lead), (where, value)
    buf, view = eo.embed(t, ld, lead, tail, fill)
    view.fill_(float("nan")); view[2, 3] = eo.CANARY; view[:, 0] = 0.0
    assert eo.intact(buf, (R, W), ld, lead)
    # a NaN with another payload is not the fill
    if fill != fill:
        buf, view = eo.embed(t, ld, lead, tail, fill)
        bits = eo._bits(buf)
        bits[0] = bits[0] ^ 1
        assert bool(torch.isnan(buf[0].float())) and not eo.intact(buf, (R, W), ld, lead)


def test_same_bits():
    a = torch.tensor([1.0, float("nan"), -0.0])
    assert eo.same_bits(a, a.clone()) and not eo.same_bits(a, torch.tensor([1.0, float("nan"), 0.0]))


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("name", eo.LAYOUTS)
def test_a_kernel_that_ignores_the_leading_dimension_is_caught(name, dtype):
    """the wrong kernel: reads its input rows at stride W (so it reads NaN padding) and writes its result rows at stride W into a view whose stride is ld"""
    R, W = 7, 16
    x = _t(R, W, dtype)
    xbuf, xv, ldx, leadx = eo.embed_as(x, name, k=1, fill=eo.NAN, tail_rows=4)
    obuf, ov, ldo, leado = eo.embed_as(torch.zeros(R, W, dtype=dtype), name, k=2, fill=eo.CANARY, tail_rows=4)
    ov.fill_(eo.NAN)                                              # an output the call must not read

    def right():
        ov.copy_(xv.float().mul(2.0).to(dtype))

    def wrong_store():
        obuf[leado:leado + R * W] = xv.float().mul(2.0).to(dtype).reshape(-1)

    def wrong_load():
        ov.copy_(xbuf[leadx:leadx + R * W].reshape(R, W).float().mul(2.0).to(dtype))

    def ok():
        good = bool(torch.isfinite(ov.float()).all()) and not bool((ov.float() == eo.CANARY).any()) and torch.equal(ov, x.float().mul(2.0).to(dtype))
        return good and eo.intact(obuf, (R, W), ldo, leado) and eo.intact(xbuf, (R, W), ldx, leadx)

    right()
    assert ok()
    for bad in (wrong_store, wrong_load):
        obuf.fill_(eo.CANARY); ov.fill_(eo.NAN)
        bad()
        assert ok() == (name == "dense"), (name, bad.__name__)


# ------------------------------------------------------------------------------------------------ the launcher's predicates, restated
def _args(M, N, K, dtype, la="dense", lb="dense", lc="dense", lres=None, laux_out=None, ta=False, tb=False, **kw):
    mk = lambda r, c, name, k: eo.embed_as(torch.zeros(r, c, dtype=dtype), name, k=k, tail_rows=0)[1]      # noqa: E731
    A = mk(*((K, M) if ta else (M, K)), la, 1)
    B = mk(*((K, N) if tb else (N, K)), lb, 2)
    C = mk(M, N, lc, 1)
    if lres is not None:
        kw["res"] = mk(M, N, lres, 3)
    if laux_out is not None:
        kw.update(act=1, aux_out=mk(M, N, laux_out, 2))
    return eo.fill_gemm_args(A, B, C, trans_a=ta, trans_b=tb, **kw)


def test_predicates_name_the_family():
    p = lambda *a, **k: eo.gemm_predicates(_args(*a, **k))      # noqa: E731
    assert p(512, 512, 192, BF)["family"] == "gemm256" and p(512, 512, 192, BF, la="pad16", lb="pad16", lc="pad16", lres="pad16")["family"] == "gemm256"
    assert p(512, 384, 128, BF, lc="pad16")["family"] == "gemm_ss"
    assert p(512, 512, 192, F32)["family"] == "gemm128_f32" and p(130, 200, 72, BF)["family"] == "gemm128_bf16"
    for lay in ("ld4", "base8", "odd"):                          # the big-tile kernels need 16 bytes per lane everywhere
        for slot in ("la", "lb", "lc", "lres", "laux_out"):
            q = p(512, 512, 192, BF, **{slot: lay})
            assert q["family"] == "gemm128_bf16" and not q["big"] and not q["ss"], (lay, slot, q)
    q = p(512, 512, 192, BF, lc="ld4")
    assert q["vec"] and q["vc"] and not q["v16"]
    q = p(512, 512, 192, BF, lc="base8")
    assert q["vec"] and q["vc"] and not q["v16"]
    q = p(512, 512, 192, BF, lc="odd")
    assert q["vec"] and not q["vc"]
    q = p(512, 512, 192, BF, la="ld4")
    assert not q["vec"] and q["vc"] and q["v16"]
    # the small-M kernel takes ld % 4 and 8-byte bases on C, res and aux; its A and B need ld % 8
    for lay in ("pad16", "ld4", "base8"):
        assert p(70, 400, 768, BF, lc=lay, lres=lay)["family"] == "gemm_smallm" and p(4, 384, 384, BF, laux_out=lay)["family"] == "gemm_smallm"
    assert p(70, 400, 768, BF, lc="odd")["family"] == "gemm128_bf16" and p(70, 400, 768, BF, la="ld4")["family"] == "gemm128_bf16"
    assert p(70, 400, 768, BF, tb=True)["family"] == "gemm128_bf16" and eo.gemm_predicates(_args(70, 400, 768, BF, tb=True), {"gemm_smallm": 1})["family"] == "gemm_smallm"
    # split-K into fp32 C: the plain reduce only where ldc == N
    C = torch.zeros(96, 160)
    Cp = eo.embed_as(C, "pad16", tail_rows=0)[1]
    A, B = torch.zeros(2048, 96, dtype=BF), torch.zeros(2048, 160, dtype=BF)
    ws = torch.zeros(4)
    assert eo.gemm_predicates(eo.fill_gemm_args(A, B, C, trans_a=True, trans_b=True, split_k=3, ws=ws))["plain_reduce"]
    q = eo.gemm_predicates(eo.fill_gemm_args(A, B, Cp, trans_a=True, trans_b=True, split_k=3, ws=ws))
    assert not q["plain_reduce"] and q["split"] == 3


def test_batched_shapes_at_dh_128_select_what_dh_512_selects():
    """the three launches of test_gemm_batched at h = 4, dh = 128, D = 128 fall in the same kernel and vec / vc classes as its 512 / 384"""
    from devias_amd import _lib

    def forms(h, dh, D, dtype, pad=0):
        out = []
        for (M, N, K, lda, ldb, ldc, sa, sb, sc, ta, tb, cf) in ((D, D, dh, D, D, D, dh * D, dh * D, D * D, 1, 1, 0), (D, D, dh, h * dh, D, h * D, dh, dh * D, D, 0, 1, 0),
                                                                 (dh, D, D, D, D, D, dh * D, D * D, dh * D, 0, 0, 1)):
            a = _lib.GemmArgs()
            a.A = a.B = a.C = 4096
            a.M, a.N, a.K, a.lda, a.ldb, a.ldc, a.trans_a, a.trans_b, a.c_f32 = M, N, K, lda, ldb, ldc, ta, tb, cf
            a.dtype = _lib.BF16 if dtype == BF else _lib.F32
            a.batch, a.stride_a, a.stride_b, a.stride_c, a.split_k = h, sa + pad, sb + pad, sc + pad, 1
            q = eo.gemm_predicates(a)
            out.append((q["family"], q["vec"], q["vc"], q["v16"]))
        return out

    for dtype in (BF, F32):
        assert forms(4, 128, 128, dtype) == forms(4, 512, 384, dtype)
        assert forms(4, 128, 128, dtype, pad=256 * 128) == forms(4, 128, 128, dtype)          # widened batch strides keep the class
        assert all(f[0] == ("gemm128_bf16" if dtype == BF else "gemm128_f32") and f[1] and f[2] for f in forms(4, 128, 128, dtype))


# ------------------------------------------------------------------------------------------------ refusals (validation precedes any launch: no GPU needed)
def _counters(lib):
    from devias_amd import _lib
    return [lib.devias_counter(i) for i in _lib.COUNTERS.values()]


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, True), (True, False)])
def test_devias_gemm_refuses_short_leading_dimensions(ta, tb):
    from devias_amd import _lib
    lib = _lib.load()
    M, N, K = 24, 40, 16
    mk = lambda r, c: torch.zeros(r, c, dtype=BF)      # noqa: E731
    A, B, C, X = mk(*((K, M) if ta else (M, K))), mk(*((K, N) if tb else (N, K))), mk(M, N), mk(M, N)
    cases = [("lda", {}, "lda"), ("ldb", {}, "ldb"), ("ldc", {}, "ldc"), ("ld_aux", {"act": 1, "aux_out": X}, "ld_aux"), ("ld_aux", {"act": 4, "aux_in": X}, "ld_aux"),
             ("ldr", {"res": X}, "ldr")]
    for field, kw, word in cases:
        a = eo.fill_gemm_args(A, B, C, trans_a=ta, trans_b=tb, **kw)
        setattr(a, field, getattr(a, field) - 1)
        before = _counters(lib)
        assert lib.devias_gemm(ctypes.byref(a), None) == -1, field              # DEVIAS_EINVAL
        msg = lib.devias_last_error().decode()
        assert msg.startswith("devias_gemm: " + word + " "), (field, msg)
        assert _counters(lib) == before
    # ld_aux and ldr are only looked at where the operand is given (ops.gemm leaves ldr 0 without a residual)
    a = eo.fill_gemm_args(A, B, C, trans_a=ta, trans_b=tb)
    a.ld_aux = a.ldr = 0
    a.lda -= 1
    assert lib.devias_gemm(ctypes.byref(a), None) == -1 and lib.devias_last_error().decode().startswith("devias_gemm: lda ")


def test_devias_wgrad_group_refuses_bad_leading_dimensions():
    from devias_amd import _lib
    lib = _lib.load()
    dY, X, dW = torch.zeros(64, 256, dtype=BF), torch.zeros(64, 256, dtype=BF), torch.zeros(256, 256)
    ws = torch.zeros(64)
    for field, value in (("ldy", 256 + 4), ("ldy", 256 - 8), ("ldx", 256 - 8), ("ldx", 256 + 12)):
        job = eo.wgrad_job_raw(dY, X, dW)
        setattr(job, field, value)
        arr = (_lib.WgradJob * 1)(job)
        before = _counters(lib)
        assert lib.devias_wgrad_group_workspace_bytes(arr, 1, 8) == -1
        assert lib.devias_wgrad_group(arr, 1, 8, ws.data_ptr(), ws.numel() * 4, None) == -1, (field, value)
        assert f"{field}={value}" in lib.devias_last_error().decode()
        assert _counters(lib) == before
