"""Operands embedded in larger allocations, for the half of the devias_gemm / devias_wgrad_group ABI that ops.gemm never exercises: leading dimensions that differ from
the widths, bases that are not 16-byte aligned, and what lies around an operand.

A plain helper module (like kernel_bounds.py): no fixtures, no plugin; importing it needs no GPU (tests/test_embedded_operands_cpu.py checks it on the CPU).

    embed(t, ld, lead, tail_rows, fill) -> (buf, view)     view = t's values at row stride ld, `lead` elements into buf; everything else of buf holds `fill`
    intact(buf, view_shape, ld, lead)                      every element of buf OUTSIDE the view still holds the fill, bitwise (lead, padding columns, tail rows)
    LAYOUTS / layout(name, W, es, k)                       the named embeddings: (ld, lead) of a [R, W] operand of element size es
    gemm_raw / wgrad_job_raw                               _lib.GemmArgs / _lib.WgradJob filled directly from views (ld = stride(0)), none of ops.gemm's conveniences
    gemm_predicates                                        the launcher's eligibility predicates (csrc/gemm.hip gemm_impl) restated over a filled GemmArgs: the family a call
                                                           must be served by follows from them, not from a run

Fills: NaN behind and between the rows of every input (a read of padding poisons the result, which the float64 bound then refuses); the bf16-exact canary 12288.0
around every output, compared bitwise."""
import ctypes

import torch

CANARY = 12288.0                   # exact in bf16 (tests/test_elementwise_bounds_gpu.py GUARD)
NAN = float("nan")
TAIL_ROWS = 256                    # a whole 256-row tile past the last row still lands in the band
LAYOUTS = ("dense", "pad16", "ld4", "base8", "odd")
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.float16: torch.int16}


def layout(name, W, es, k=1):
    """(ld, lead in elements) of the named embedding of a [R, W] operand with element size es
    dense   ld = W,       lead 0                                  the control
    pad16   ld = W + 8 k, lead a multiple of 16 bytes             the alignment class of dense (where W % 8 == 0): the same family must serve
    ld4     ld = W + 4,   lead a multiple of 16 bytes             ld % 4 == 0, ld % 8 != 0 (where W % 8 == 0): 4-wide epilogue accesses without the 16-byte ones
    base8   ld = W + 8,   lead 8 bytes                            8-byte, not 16-byte aligned base
    odd     ld = W + 1,   lead 1                                  every vector predicate false"""
    if name == "dense":
        return W, 0
    if name == "pad16":
        return W + 8 * k, 64
    if name == "ld4":
        return W + 4, 64
    if name == "base8":
        return W + 8, 64 + 8 // es
    if name == "odd":
        return W + 1, 1
    raise ValueError(name)


def embed(t, ld, lead=0, tail_rows=TAIL_ROWS, fill=NAN):
    """(buf, view): buf one flat allocation filled with `fill`; view [R, W] with stride (ld, 1), `lead` elements in, holding t; tail_rows whole rows of fill follow"""
    R, W = t.shape
    assert ld >= W and lead >= 0 and tail_rows >= 0
    buf = torch.full((lead + (R + tail_rows) * ld,), fill, dtype=t.dtype, device=t.device)
    view = buf.as_strided((R, W), (ld, 1), lead)
    view.copy_(t)
    return buf, view


def embed_as(t, name, k=1, fill=NAN, tail_rows=TAIL_ROWS):
    """embed under a named layout; (buf, view, ld, lead)"""
    ld, lead = layout(name, t.shape[1], t.element_size(), k)
    buf, view = embed(t, ld, lead, tail_rows, fill)
    return buf, view, ld, lead


def _bits(t):
    return t.view(_BITS[t.dtype])


def outside(buf, view_shape, ld, lead):
    """bool mask over buf: True outside the [R, W] view at row stride ld that starts `lead` elements in"""
    R, W = view_shape
    idx = torch.arange(buf.numel(), device=buf.device) - lead
    return ~((idx >= 0) & (idx < R * ld) & (idx % ld < W))


def intact(buf, view_shape, ld, lead, fill=None):
    """every element outside the view holds the fill bitwise.  fill = None: the canary, or NaN where the first element outside the view is one (an embed() fill is
    one of the two; the pattern is torch.full's, so a NaN written by a kernel with another payload counts as damage)"""
    out = outside(buf, view_shape, ld, lead)
    if not bool(out.any()):
        return True
    got = buf[out]
    if fill is None:
        fill = NAN if bool(torch.isnan(got[0].float())) else CANARY
    want = torch.full((1,), fill, dtype=buf.dtype, device=buf.device)
    return bool((_bits(got) == _bits(want)).all())


def same_bits(a, b):
    """bitwise equality of two tensors of one dtype and shape (NaN equal to the same NaN)"""
    return a.shape == b.shape and a.dtype == b.dtype and bool((_bits(a.contiguous()) == _bits(b.contiguous())).all())


def _ld(t, name):
    assert t.dim() == 2 and t.stride(1) == 1, (name, tuple(t.shape), t.stride())
    return t.stride(0)


def fill_gemm_args(A, B, C, *, trans_a=False, trans_b=False, bias=None, act=0, aux_in=None, aux_out=None, res=None, res_mod=0, beta=0.0, split_k=1, ws=None,
                   colsum=None, colsum_beta=0.0, row_scale=None, rows_per_scale=0):
    """_lib.GemmArgs from 2-D views with unit column stride: every leading dimension is the view's stride(0).  Needs no GPU (pointers are only copied)."""
    from devias_amd import _lib
    dt = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}[A.dtype]
    assert B.dtype == A.dtype and C.dtype in (A.dtype, torch.float32)
    a = _lib.GemmArgs()
    a.lda, a.ldb, a.ldc = _ld(A, "A"), _ld(B, "B"), _ld(C, "C")
    M, K = (A.shape[1], A.shape[0]) if trans_a else A.shape
    N, Kb = (B.shape[1], B.shape[0]) if trans_b else B.shape
    assert K == Kb and tuple(C.shape) == (M, N)
    a.A, a.B, a.C = A.data_ptr(), B.data_ptr(), C.data_ptr()
    a.M, a.N, a.K = M, N, K
    a.trans_a, a.trans_b, a.dtype, a.c_f32 = int(trans_a), int(trans_b), dt, int(C.dtype == torch.float32)
    a.act, a.beta, a.split_k = act, beta, split_k
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N and bias.is_contiguous()
        a.bias = bias.data_ptr()
    for name, t in (("aux_in", aux_in), ("aux_out", aux_out)):
        if t is not None:
            assert t.dtype == A.dtype and tuple(t.shape) == (M, N)
            ld = _ld(t, name)
            assert a.ld_aux in (0, ld), "aux_in and aux_out share ld_aux"
            a.ld_aux = ld
            setattr(a, name, t.data_ptr())
    if res is not None:
        assert res.dtype == A.dtype and tuple(res.shape) == ((res_mod if res_mod > 0 else M), N)
        a.res, a.ldr, a.res_mod = res.data_ptr(), _ld(res, "res"), res_mod
    if row_scale is not None:
        assert row_scale.dtype == torch.float32 and rows_per_scale > 0 and row_scale.numel() * rows_per_scale >= M
        a.row_scale, a.rows_per_scale = row_scale.data_ptr(), rows_per_scale
    if colsum is not None:
        assert colsum.dtype == torch.float32 and colsum.numel() == N and split_k == 1
        a.colsum, a.colsum_beta = colsum.data_ptr(), colsum_beta
    if ws is not None:
        a.ws = ws.data_ptr()
    return a


def gemm_raw(o, A, B, C, **fields):
    """devias_gemm on the current stream with the arguments of fill_gemm_args; the workspace is sized as ops.gemm sizes it (split-K bytes from
    devias_gemm_workspace_bytes, column sums max(ceil(M / 128) N 4, devias_colsum_workspace_bytes)); split_k as given.  Returns the struct it passed."""
    from devias_amd import _lib
    lib = _lib.load()
    a = fill_gemm_args(A, B, C, **fields)
    nbytes = 0
    if a.colsum:
        nbytes = max(((a.M + 127) // 128) * a.N * 4, lib.devias_colsum_workspace_bytes(a.M, a.N))
    if a.split_k > 1:
        nbytes = max(nbytes, lib.devias_gemm_workspace_bytes(a.M, a.N, a.split_k))
    if nbytes and not a.ws:
        a.ws = o.workspace(nbytes, A.device).data_ptr()
    _lib.check(lib.devias_gemm(ctypes.byref(a), torch.cuda.current_stream().cuda_stream), "devias_gemm")
    return a


def wgrad_job_raw(dY, X, dW, beta=0.0):
    """_lib.WgradJob from views: ldy, ldx from stride(0); dW dense"""
    from devias_amd import _lib
    assert dY.dtype == X.dtype == torch.bfloat16 and dW.dtype == torch.float32 and dW.is_contiguous()
    assert dY.shape[0] == X.shape[0] and tuple(dW.shape) == (dY.shape[1], X.shape[1])
    return _lib.WgradJob(dY.data_ptr(), X.data_ptr(), dW.data_ptr(), dY.shape[0], dY.shape[1], X.shape[1], _ld(dY, "dY"), _ld(X, "X"), beta)


def gemm_predicates(a, opt=None):
    """csrc/gemm.hip gemm_impl's predicates over a filled GemmArgs `a`: {"vec", "vc", "v16", "big", "ss", "smallm", "family"}.  family is the counter that must count
    the product: gemm_smallm, gemm_ss, gemm256 (one of its forms: the caller knows which from the options it set), gemm128_bf16 or gemm128_f32.
    opt: option values where they differ from the defaults assumed here (gemm256 1, gemm_ss 1, gemm_smallm 2)."""
    opt = {"gemm256": 1, "gemm_ss": 1, "gemm_smallm": 2, **(opt or {})}
    bf = a.dtype == 1
    es = 2 if bf else 4
    ch = 16 // es
    al = lambda p, n: p is None or p % n == 0                  # noqa: E731   (an absent operand constrains nothing)
    batch = a.batch if a.batch > 1 else 1
    c_f32 = bool(a.c_f32) or not bf
    bk = 64 if bf else 16
    split = a.split_k if a.split_k > 1 else 1
    kps = a.K
    if split > 1:
        cdiv = lambda x, y: -(-x // y)                         # noqa: E731
        kps = cdiv(cdiv(a.K, split), bk) * bk
        split = cdiv(a.K, kps)
    vec = al(a.A, 16) and al(a.B, 16) and a.lda % ch == 0 and a.ldb % ch == 0
    vec = vec and (a.M if a.trans_a else a.K) % ch == 0 and (a.N if a.trans_b else a.K) % ch == 0
    if batch > 1:
        vec = vec and a.stride_a % ch == 0 and a.stride_b % ch == 0
    vc = a.N % 4 == 0 and a.ldc % 4 == 0 and al(a.C, 16 if c_f32 else 8) and al(a.bias, 16)
    if a.res:
        vc = vc and a.ldr % 4 == 0 and al(a.res, 8)
    if a.aux_in or a.aux_out:
        vc = vc and a.ld_aux % 4 == 0 and al(a.aux_in, 8) and al(a.aux_out, 8)
    if es == 4:
        vc = vc and al(a.res, 16) and al(a.aux_in, 16) and al(a.aux_out, 16) and al(a.C, 16)
    if batch > 1:
        vc = vc and a.stride_c % 4 == 0
    v16 = vc and a.N % 8 == 0 and a.ldc % 8 == 0 and al(a.C, 16) and al(a.bias, 16) and (not a.res or (a.ldr % 8 == 0 and al(a.res, 16))) and \
        (not (a.aux_in or a.aux_out) or (a.ld_aux % 8 == 0 and al(a.aux_in, 16) and al(a.aux_out, 16))) and (split == 1 or al(a.ws, 16))
    whole_k = a.K % 64 == 0 and kps % 64 == 0
    big = bool(opt["gemm256"]) and bf and vec and vc and a.M % 256 == 0 and a.N % 256 == 0 and whole_k and v16 and batch == 1
    ss = opt["gemm_ss"] != 0 and bf and vec and v16 and a.M % 256 == 0 and a.N % 128 == 0 and whole_k and batch == 1 and not (a.trans_a and not a.trans_b)
    if ss and big and (opt["gemm_ss"] < 0 or (not a.trans_a and not a.trans_b)):
        ss = False
    if ss:
        big = False
    smallm = bool(opt["gemm_smallm"]) and bf and not a.trans_a and (not a.trans_b or opt["gemm_smallm"] == 1) and a.M <= 128 and batch == 1 and not c_f32 and \
        not a.colsum and vec and vc and a.N % 16 == 0 and a.K % 128 == 0 and a.lda % 8 == 0 and a.ldb % 8 == 0 and a.ldc % 4 == 0 and al(a.C, 8) and al(a.bias, 16) and \
        (not a.res or (a.ldr % 4 == 0 and al(a.res, 8))) and (not (a.aux_in or a.aux_out) or (a.ld_aux % 4 == 0 and al(a.aux_in, 8) and al(a.aux_out, 8)))
    family = "gemm_smallm" if smallm else "gemm_ss" if ss else "gemm256" if big else "gemm128_bf16" if bf else "gemm128_f32"
    plain_reduce = split > 1 and c_f32 and a.ldc == a.N and (a.M * a.N) % 4 == 0 and not a.bias and a.act == 0 and not a.res and not a.row_scale and al(a.ws, 16) and al(a.C, 16)
    return {"vec": bool(vec), "vc": bool(vc), "v16": bool(v16), "big": bool(big), "ss": bool(ss), "smallm": bool(smallm), "family": family, "split": split,
            "plain_reduce": bool(plain_reduce)}
