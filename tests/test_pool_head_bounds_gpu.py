"""devias_pool_head_fwd / _bwd on the GPU against the float64 bounds of tests/pool_head_bounds.py: every element of every output, both pool modes, both dtypes, at
the shapes where the kernels take another path (one token, a few, one chunk less / exactly / plus one token, chunks plus a ragged tail, 1568 and 1569)."""
import pytest
import torch

import pool_head_bounds as pb

pytestmark = pytest.mark.gpu

T = pb.CHUNK
# (Nt, B, D, C, mask, dtoken, generator): every (D, dtype) thread layout of the streaming kernels meets a ragged chunk; C in {2, 101, 365, 400}; B in {1, 3}
CASES = [(1, 1, 384, 2, False, False, "graded"), (7, 3, 768, 101, True, True, "tail"), (T - 1, 3, 1024, 365, True, False, "graded"),
         (T, 1, 768, 400, False, True, "offset"), (T + 1, 3, 384, 365, True, True, "tail"), (2 * T + 3, 3, 1024, 101, False, False, "graded"),
         (2 * T + 3, 1, 768, 2, True, True, "offset"), (T + 1, 1, 1024, 400, True, True, "tail"), (2 * T + 3, 3, 384, 400, False, True, "graded"),
         (1568, 1, 768, 365, True, True, "graded"), (1569, 3, 768, 101, False, False, "tail")]
DTYPES = [torch.float32, torch.bfloat16]


def _al256(n):
    return (n + 255) // 256 * 256


def _run(I, pool, dtype, save=True, dx_buf=None, pad_rows=0):
    """-> dict of the region's outputs on the CPU (token, logits, and with save: a, dx, dW, db, dgamma, dbeta)"""
    from devias_amd import ops
    h = I["h"].cuda()
    B, Nt, D = h.shape
    C = I["W"].shape[0]
    keep = [I["W"].to(dtype).cuda(), I["bias"].cuda(), I["gamma"].cuda(), I["beta"].cuda()]
    mask = I["mask"].cuda() if I["mask"] is not None else None
    a = ops.pool_head_args(B, Nt, pool, pb.EPS, *keep, mask)
    token, logits, arena = ops.pool_head_fwd(a, h.view(B * Nt, D), save=save)
    out = {"token": token, "logits": logits}
    if save:
        off = _al256(B * D * 4) + _al256(B * 4)
        out["a"] = arena[off:off + B * D * h.element_size()].view(dtype).view(B, D).clone()
        dx = torch.empty((B * Nt, D), dtype=dtype, device="cuda") if dx_buf is None else dx_buf[pad_rows:pad_rows + B * Nt]
        grads = [torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for s in ((C, D), (C,), (D,), (D,))]
        dtok = I["dtoken"].cuda() if I["dtoken"] is not None else None
        ops.pool_head_bwd(a, arena, I["dlogits"].cuda(), dtok, dx, grads)
        out.update(dx=dx.view(B, Nt, D), dW=grads[0], db=grads[1], dgamma=grads[2], dbeta=grads[3])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("pool", [pb.MEAN, pb.CLS], ids=["mean", "cls"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "Nt%d_B%d_D%d_C%d_m%d_t%d_%s" % c)
def test_pool_head_region_within_bounds(case, pool, dtype):
    from devias_amd import ops
    Nt, B, D, C, mask, dtok, kind = case
    I = pb.inputs(kind, B, Nt, D, C, dtype, mask, dtok)
    ref, bnd = pb.bounds(I, pool, dtype)
    ops.counters(reset=True)
    n0 = ops.pool_head_launches()
    out = _run(I, pool, dtype)
    assert n0 == 0 and ops.pool_head_launches() == 2          # one per call: the forward, the backward
    r = pb.ratios(out, ref, bnd)
    print("pool_head", case, pool, dtype, {k: round(v, 4) for k, v in r.items()})
    assert set(r) == set(pb.SLACKS)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    # save = NULL: bitwise the saving forward; a second saving run: bitwise the first
    nosave = _run(I, pool, dtype, save=False)
    assert ops.pool_head_launches() == 3
    assert torch.equal(nosave["token"], out["token"]) and torch.equal(nosave["logits"], out["logits"])
    again = _run(I, pool, dtype)
    for k, v in out.items():
        assert torch.equal(again[k], v), k


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("pool", [pb.MEAN, pb.CLS], ids=["mean", "cls"])
def test_pool_head_backward_writes_its_rows_and_no_other(pool, dtype):
    """dx inside a larger canary-filled buffer: every row of the B clips is written (no canary left), the rows just before and after are untouched"""
    Nt, B, D, C = 2 * T + 3, 3, 768, 101
    I = pb.inputs("graded", B, Nt, D, C, dtype, True, True)
    pad = 5
    canary = 12288.0          # exact in bf16
    buf = torch.full((B * Nt + 2 * pad, D), canary, dtype=dtype, device="cuda")
    out = _run(I, pool, dtype, dx_buf=buf, pad_rows=pad)
    host = buf.cpu().float()
    assert bool((host[:pad] == canary).all()) and bool((host[pad + B * Nt:] == canary).all())
    assert not bool((out["dx"].float() == canary).any())
    if pool == pb.CLS:
        assert bool((out["dx"][:, 1:] == 0).all())
