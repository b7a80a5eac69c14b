"""Output guards for the row kernels and attention (GPU only).  devias_layernorm_fwd / _bwd and devias_mhsa_fwd / _bwd take no leading dimension, so of
tests/embedded_operands.py only the bands apply: every output (and the workspace, at exactly its queried size) sits between a 64-element lead and 256 rows of the
bf16-exact canary, the row inputs sit before 256 rows of NaN.  The guarded call must give bitwise the unguarded call's outputs and leave every band intact.  Accuracy
is tests/test_kernel_bounds_gpu.py's business, and what lies behind the attention inputs test_mhsa_tail_tiles_read_zero_not_what_lies_behind_the_tensor's."""
import pytest
import torch

import embedded_operands as eo
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
SCALE = 0.125


def banded(shape, dtype, inside=None):
    """(buf, view) of an output: 2-D [R, W] (1-D: one row) at ld = W inside a canary band; pre-filled with NaN unless `inside` is given"""
    shape2 = tuple(shape) if len(shape) == 2 else (1, int(torch.Size(shape).numel()))
    src = inside.reshape(shape2) if inside is not None else torch.full(shape2, eo.NAN, dtype=dtype, device=DEV)
    buf, view = eo.embed(src, shape2[1], 64, eo.TAIL_ROWS, eo.CANARY)
    return buf, view.reshape(shape)


def before_nan(t):
    """the same rows followed by 256 rows of NaN"""
    return eo.embed(t, t.shape[1], 0, eo.TAIL_ROWS, eo.NAN)[1]


def bands_intact(bands):
    for name, (buf, view) in bands.items():
        shape2 = tuple(view.shape) if view.dim() == 2 else (1, view.numel())
        assert eo.intact(buf, shape2, shape2[1], 64, eo.CANARY), f"a store outside {name}"


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("M,D", [(67, 1024), (257, 512)])
def test_layernorm_outputs_inside_guard_bands(M, D, dtype):
    from devias_amd import _lib, ops
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    x, g, b, dy, dres = kb.layernorm_inputs(M, D, dtype, spread=6, seed=900, device=DEV)
    eps, dt = 1e-6, ops.dt_code(dtype)
    y0, mean0, rstd0 = ops.layernorm_fwd(x, g, b, eps)
    xg, dyg, dresg = before_nan(x), before_nan(dy), before_nan(dres)
    out = {"y": banded((M, D), dtype), "mean": banded((M,), F32), "rstd": banded((M,), F32)}
    _lib.check(lib.devias_layernorm_fwd(xg.data_ptr(), g.data_ptr(), b.data_ptr(), out["y"][1].data_ptr(), out["mean"][1].data_ptr(), out["rstd"][1].data_ptr(), M, D, eps, dt, st),
               "devias_layernorm_fwd")
    torch.cuda.synchronize()
    for name, want in (("y", y0), ("mean", mean0), ("rstd", rstd0)):
        assert eo.same_bits(out[name][1], want), f"layernorm_fwd {name} differs from the unguarded call's"
    bands_intact(out)
    dg_old, db_old = kb._randn((D,), 901, DEV) * 4.0, kb._randn((D,), 902, DEV) * 4.0
    nws = lib.devias_layernorm_bwd_workspace_bytes(M, D)
    for with_dres, beta_acc in ((True, 0.0), (False, 1.0)):
        cs0 = torch.empty(D, device=DEV)
        dx0, dg0, db0 = ops.layernorm_bwd(dy, x, g, mean0, rstd0, dres=dres if with_dres else None, dgamma=dg_old.clone(), dbeta=db_old.clone(), beta_acc=beta_acc, dx_colsum=cs0)
        keep = beta_acc != 0.0                                       # beta_acc = 0: destinations the call must not read
        out = {"dx": banded((M, D), dtype), "dgamma": banded((D,), F32, dg_old if keep else None), "dbeta": banded((D,), F32, db_old if keep else None),
               "dx_colsum": banded((D,), F32), "workspace": banded(((nws + 3) // 4,), F32)}
        _lib.check(lib.devias_layernorm_bwd(dyg.data_ptr(), xg.data_ptr(), g.data_ptr(), mean0.data_ptr(), rstd0.data_ptr(), dresg.data_ptr() if with_dres else None,
                                            out["dx"][1].data_ptr(), out["dgamma"][1].data_ptr(), out["dbeta"][1].data_ptr(), beta_acc, out["dx_colsum"][1].data_ptr(), M, D, dt,
                                            out["workspace"][1].data_ptr(), st), "devias_layernorm_bwd")
        torch.cuda.synchronize()
        for name, want in (("dx", dx0), ("dgamma", dg0), ("dbeta", db0), ("dx_colsum", cs0)):
            assert eo.same_bits(out[name][1], want), f"layernorm_bwd {name} differs from the unguarded call's (dres {with_dres}, beta_acc {beta_acc})"
        bands_intact(out)


@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("B,N,H", [(2, 100, 3), (1, 333, 1)])
def test_mhsa_outputs_inside_guard_bands(B, N, H, dtype):
    from devias_amd import _lib, ops
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    dt, D = ops.dt_code(dtype), H * 64
    qkv, d_o = kb.attention_inputs(B, N, H, dtype, logit_std=1.0, seed=1000, device=DEV)
    nws = (int(lib.devias_mhsa_bwd_workspace_bytes(B, N, H)) + 3) // 4

    def call(o, lse, delta, dqkv, ws):
        _lib.check(lib.devias_mhsa_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, H, SCALE, dt, st), "devias_mhsa_fwd")
        _lib.check(lib.devias_mhsa_bwd(qkv.data_ptr(), o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, N, H, SCALE, dt, ws.data_ptr(), st),
                   "devias_mhsa_bwd")
        torch.cuda.synchronize()

    plain = {"o": torch.empty(B * N, D, dtype=dtype, device=DEV), "lse": torch.empty(B, H, N, device=DEV), "delta": torch.empty(B, H, N, device=DEV),
             "dqkv": torch.empty_like(qkv), "workspace": torch.empty(max(nws, 1), device=DEV)}
    call(*plain.values())
    out = {"o": banded((B * N, D), dtype), "lse": banded((B * H * N,), F32), "delta": banded((B * H * N,), F32), "dqkv": banded(tuple(qkv.shape), dtype),
           "workspace": banded((max(nws, 1),), F32)}
    call(*(v for _, v in out.values()))
    for name in ("o", "lse", "delta", "dqkv"):
        assert eo.same_bits(out[name][1].reshape(-1), plain[name].reshape(-1)), f"mhsa {name} differs from the unguarded call's"
    bands_intact(out)
