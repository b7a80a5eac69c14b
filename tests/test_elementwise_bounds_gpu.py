"""The element-wise kernels of devias_amd/csrc/elementwise.hip (GPU only), which serve the regularised training step between the GEMMs: every element held to the
bound of tests/kernel_bounds.py against float64 on graded inputs (float64 references in torch on the device: none of this project's kernels), the exact kernels
(cast, rows_broadcast, patch_im2col) to torch.equal.  Sizes are the smallest that reach each path: one element, a tail shorter than a vector, one grid-stride wrap of
the 2048-workgroup grid plus a tail, a pointer that is not 16-byte aligned (a view offset by one element: a valid call, served by the scalar path), a ragged last
row group, one / two / seventeen row blocks of the column sums, part-filled and scalar column blocks.  Each case prints `[bound] <kernel> <shape> <variant> worst ratio ...`."""
import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
WRAP4 = 2 * 1024 * 1024 + 7        # four elements per thread: n / 4 > 2048 * 256, one wrap of the vector loop, and a 3-element tail
WRAP1 = 2048 * 256 + 3             # one element per thread
SIZES4 = [1, 3, 1027, WRAP4]
SIZES1 = [1, 3, 1027, WRAP1]
GUARD = 12288.0                    # (exact in bf16)


@pytest.fixture
def o():
    from devias_amd import ops
    return ops


def say(kernel, shape, variant, ratio):
    print(f"[bound] {kernel} {shape} {variant} worst ratio {ratio:.3f}")


def place(t, offset):
    """the same values in fresh memory; offset = 1: a view that starts one element into its buffer (contiguous, but not 16-byte aligned)"""
    if not offset:
        return t.clone()
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    assert buf[1:].data_ptr() % 16 != 0
    return buf[1:].reshape(t.shape)


def guarded(n, dtype, offset):
    """(buffer, view): an output view of n elements with one guard element on each side, (mis)aligned like place(); guards_intact(buffer) after the call"""
    lead = 1 if offset else 8
    buf = torch.full((lead + n + 1,), GUARD, dtype=dtype, device=DEV)
    view = buf[lead:lead + n]
    assert (view.data_ptr() % 16 != 0) == bool(offset)
    return buf, view


def guards_intact(buf, n):
    lead = buf.numel() - n - 1
    return bool((buf[:lead] == GUARD).all()) and float(buf[-1]) == GUARD


# ------------------------------------------------------------------------------------------------ cast, cast_scale
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("sd,dd", [(F32, BF), (BF, F32), (F32, F32), (BF, BF)])
def test_cast(sd, dd, offset, o):
    for n in SIZES4:
        src = place(kb.elementwise_inputs(n, sd, seed=2000, device=DEV), offset)
        assert torch.equal(o.cast(src, dd), src.to(dd)), (n, "aligned destination")
        buf, view = guarded(n, dd, offset)
        o.cast(src, dd, out=view)
        assert torch.equal(view, src.to(dd)) and guards_intact(buf, n), (n, "destination placed like the source")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("sd,dd", [(F32, F32), (BF, F32), (F32, BF)])
def test_cast_scale(sd, dd, offset, o):
    scale = 1.0 / 3.0
    for n in SIZES4:
        src = place(kb.elementwise_inputs(n, sd, seed=2010, device=DEV), offset)
        ref, bound = kb.cast_scale_ref(src, scale, dd)
        buf, view = guarded(n, dd, offset)
        o.cast(src, dd, out=view, scale=scale)
        r = kb.check(f"cast_scale {sd} -> {dd} n {n}", view, ref, bound)
        assert guards_intact(buf, n)
        if offset:                                          # one side aligned, the other not: still the scalar path
            r = max(r, kb.check(f"cast_scale {sd} -> {dd} n {n}, aligned destination", o.cast(src, dd, scale=scale), ref, bound))
        if sd == F32 and dd == F32:                         # in place (devias_cast_scale's contract: dst may be src)
            work = place(src, offset)
            o.cast(work, F32, out=work, scale=scale)
            assert torch.equal(work, view), (n, "in place")
        say("cast_scale", n, f"{sd} -> {dd} offset {offset}", r)


# ------------------------------------------------------------------------------------------------ add, mul_mask, act_bwd
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_add(dtype, offset, o):
    for n in SIZES4:
        a = place(kb.elementwise_inputs(n, dtype, seed=2020, device=DEV), offset)
        b = place(kb.elementwise_inputs(n, dtype, seed=2021, device=DEV).flip(0), offset)
        say("add", n, f"{dtype} offset {offset}", kb.check(f"add n {n}", o.add(a, b), *kb.add_ref(a, b, dtype)))
        if offset:
            b0 = b.clone()
            kb.check(f"add n {n}, only a unaligned", o.add(a, b0), *kb.add_ref(a, b0, dtype))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_mul_mask(dtype, with_b, offset, o):
    for n in SIZES1:
        a = place(kb.elementwise_inputs(n, dtype, seed=2030, device=DEV), offset)
        b = place(kb.elementwise_inputs(n, dtype, seed=2031, device=DEV).flip(0), offset) if with_b else None
        mask = place(kb.drop_mask(n, 0.9, seed=2032, device=DEV), offset)
        say("mul_mask", n, f"{dtype} b {int(with_b)} offset {offset}", kb.check(f"mul_mask n {n}", o.mul_mask(a, mask, b), *kb.mul_mask_ref(a, mask, b, dtype)))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("act", ["sigmoid", "relu", "gelu"])
@pytest.mark.parametrize("dtype", [F32, BF])
def test_act_bwd(dtype, act, offset, o):
    code, kcode = {"sigmoid": (o.ACT_SIGMOID, kb.ACT_SIGMOID), "relu": (o.ACT_RELU, kb.ACT_RELU), "gelu": (o.ACT_GELU, kb.ACT_GELU)}[act]
    for n in SIZES1:
        g = place(kb.elementwise_inputs(n, dtype, seed=2040, device=DEV), offset)
        pre = kb._randn((n,), 2041, DEV) * 1.5
        y = place((torch.sigmoid(pre) if act == "sigmoid" else pre).to(dtype), offset)        # sigmoid: the stored output; ReLU / GELU: the stored pre-activation
        say("act_bwd", n, f"{dtype} {act} offset {offset}", kb.check(f"act_bwd {act} n {n}", o.act_bwd(g, y, code), *kb.act_bwd_ref(g, y, kcode, dtype)))


# ------------------------------------------------------------------------------------------------ row_scale
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,N,rps", [(5, 4, 1), (300, 764, 7), (321, 768, 100)])
def test_row_scale(M, N, rps, dtype, o):
    """N a multiple of 4 but not always of 8; the last group of rows_per_scale rows ragged; a zero and negative factors"""
    x = kb.elementwise_inputs(M * N, dtype, seed=2050, device=DEV).reshape(M, N)
    groups = -(-M // rps)
    scale = torch.linspace(-1.5, 2.0, groups, device=DEV)
    scale[groups // 2] = 0.0
    assert float(scale.min()) < 0 and bool((scale == 0).any())
    say("row_scale", (M, N, rps), f"{dtype}", kb.check("row_scale", o.row_scale(x, scale, rps), *kb.row_scale_ref(x, scale, rps, dtype), lambda i: kb.where2d(i, N)))


# ------------------------------------------------------------------------------------------------ colsum
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M", [1, 256, 257, 4097])
def test_colsum(M, dtype, o):
    """one row block (the result written directly, beta applied there), two, and seventeen (more partials than the second stage has lanes); a full vector width, a
    ragged last lane group (200), a part-filled second column block (264), the scalar path (765: the row stride is no multiple of 8); a column range of a wider
    matrix starting at a multiple of 8 (vector path) and at an odd column (unaligned: scalar path)"""
    for N in (8, 200, 264, 765):
        x = kb.columns_inputs(M, N, dtype, seed=2060, device=DEV)
        old = kb._randn((N,), 2061, DEV) * kb.graded(N, 6, DEV).float() * 4.0
        for beta in (0.0, 1.0):
            out = o.colsum(x, out=old.clone(), beta=beta)
            say("colsum", (M, N), f"{dtype} beta {beta}", kb.check(f"colsum M {M} N {N} beta {beta}", out, *kb.colsum_ref(x, beta, old)))
        kb.check(f"colsum M {M} N {N} fresh output", o.colsum(x), *kb.colsum_ref(x))
    ld, count = 272, 200
    wide = kb.columns_inputs(M, ld, dtype, seed=2062, device=DEV)
    old = kb._randn((count,), 2063, DEV) * kb.graded(count, 6, DEV).float() * 4.0
    for c0 in (8, 3, 72):
        for beta in (0.0, 1.0):
            out = o.colsum(wide, out=old.clone(), beta=beta, cols=(c0, count))
            r = kb.check(f"colsum M {M} cols ({c0}, {count}) of {ld} beta {beta}", out, *kb.colsum_ref(wide[:, c0:c0 + count], beta, old))
            say("colsum", (M, ld), f"{dtype} cols=({c0}, {count}) beta {beta}", r)


# ------------------------------------------------------------------------------------------------ rows_reduce_mod, rows_broadcast
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,mod,N", [(12, 4, 40), (20, 1, 7), (260, 5, 768)])
def test_rows_reduce_mod_and_broadcast(M, mod, N, dtype, o):
    x = kb.columns_inputs(M, N, dtype, seed=2070, device=DEV)
    say("rows_reduce_mod", (M, mod, N), f"{dtype}", kb.check("rows_reduce_mod", o.rows_reduce_mod(x, mod), *kb.rows_reduce_mod_ref(x, mod), lambda i: kb.where2d(i, N)))
    src = kb.columns_inputs(mod, N, F32, seed=2071, device=DEV)
    for rows in (M, M + mod // 2 + 1):                      # (the second: M no multiple of mod)
        assert torch.equal(o.rows_broadcast(src, rows, dtype), src.repeat(-(-rows // mod), 1)[:rows].to(dtype)), rows


# ------------------------------------------------------------------------------------------------ patch_im2col
@pytest.mark.parametrize("sd,dd", [(F32, F32), (F32, BF), (BF, BF), (BF, F32)])
@pytest.mark.parametrize("shape,ts,ps", [((2, 3, 4, 32, 48), 2, 16), ((2, 2, 3, 16, 32), 1, 8), ((1, 3, 4, 16, 16), 2, 16)])
def test_patch_im2col(shape, ts, ps, sd, dd, o):
    """the geometry of test_cast_im2col_colsum_rows, tubelet = 1, and a single patch per frame"""
    B, C, T, H, W = shape
    v = kb.elementwise_inputs(B * C * T * H * W, sd, seed=2080, device=DEV).reshape(shape)
    ref = v.reshape(B, C, T // ts, ts, H // ps, ps, W // ps, ps).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B * (T // ts) * (H // ps) * (W // ps), C * ts * ps * ps)
    assert torch.equal(o.patch_im2col(v, ts, ps, dd), ref.to(dd))
