"""devias_two_token_head_fwd / _bwd on the GPU against the float64 bounds of tests/two_token_head_bounds.py: every element of every output, both head modes, both
dtypes, at the smallest shapes where the kernels can go wrong (no patch rows between the two tokens, a few rows, one chunk of the dx kernel less / exactly / plus one
row, two chunks and a ragged tail), the canary around dx and bitwise repeatability."""
import pytest
import torch

import two_token_head_bounds as tb

pytestmark = pytest.mark.gpu

# (Nt, B, D, Ca, Cs, unified, masks, dtoken, generator): every (D, dtype) thread layout of the dx kernel meets a ragged chunk; every Nt, B, D, (Ca, Cs) and both head
# modes, masks and dtoken absent and present
CASES = [(2, 1, 384, 2, 2, False, False, False, "graded"), (2, 3, 768, 101, 365, True, True, True, "tail"), (3, 3, 1024, 400, 365, False, True, True, "tail"),
         (7, 1, 768, 2, 2, True, True, False, "offset"), (63, 3, 384, 101, 365, False, True, False, "graded"), (64, 1, 1024, 400, 365, True, False, True, "offset"),
         (65, 3, 768, 400, 365, False, True, True, "tail"), (65, 1, 384, 101, 365, True, True, True, "graded"), (131, 3, 1024, 101, 365, True, True, True, "tail"),
         (131, 3, 768, 2, 2, False, False, True, "graded"), (131, 1, 384, 400, 365, False, True, True, "offset")]
DTYPES = [torch.float32, torch.bfloat16]


def _al256(n):
    return (n + 255) // 256 * 256


def _run(I, dtype, save=True, dx_buf=None, pad_rows=0):
    """-> dict of the region's outputs on the CPU (tokens, logits, and with save: a, dx and the parameter gradients)"""
    from devias_amd import ops
    h = I["h"].cuda()
    B, Nt, D = h.shape
    cu = lambda t: t.cuda() if t is not None else None      # noqa: E731
    Wa, Ws = I["Wa"].to(dtype).cuda(), (I["Ws"].to(dtype).cuda() if I["Ws"] is not None else None)
    keep = [Wa, cu(I["ba"]), Ws, cu(I["bs"]), cu(I["gamma"]), cu(I["beta"]), cu(I["mask_a"]), cu(I["mask_s"])]
    a = ops.two_token_head_args(B, Nt, tb.EPS, *keep)
    token_a, token_s, logits_a, logits_s, arena = ops.two_token_head_fwd(a, h.view(B * Nt, D), save=save)
    out = {"token_a": token_a, "token_s": token_s, "logits_a": logits_a, "logits_s": logits_s}
    if save:
        off = _al256(2 * B * D * 4) + _al256(2 * B * 4)
        out["a"] = arena[off:off + 2 * B * D * h.element_size()].view(dtype).view(2 * B, D).clone()
        dx = torch.empty((B * Nt, D), dtype=dtype, device="cuda") if dx_buf is None else dx_buf[pad_rows:pad_rows + B * Nt]
        shapes = [(a.Ca, D), (a.Ca,), (a.Cs, D), (a.Cs,), (D,), (D,)]
        grads = [torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for s in shapes]
        if I["unified"]:
            grads[2] = grads[3] = None
        ops.two_token_head_bwd(a, arena, I["dlogits_a"].cuda(), I["dlogits_s"].cuda(), cu(I["dtoken_a"]), cu(I["dtoken_s"]), dx, grads)
        out.update(dx=dx.view(B, Nt, D), dWa=grads[0], dba=grads[1], dgamma=grads[4], dbeta=grads[5])
        if not I["unified"]:
            out.update(dWs=grads[2], dbs=grads[3])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "Nt%d_B%d_D%d_Ca%d_Cs%d_u%d_m%d_t%d_%s" % c)
def test_two_token_head_region_within_bounds(case, dtype):
    from devias_amd import ops
    Nt, B, D, Ca, Cs, uni, mask, dtok, kind = case
    I = tb.inputs(kind, B, Nt, D, Ca, Cs, dtype, uni, mask, dtok)
    ref, bnd = tb.bounds(I, dtype)
    ops.counters(reset=True)
    n0 = ops.two_token_head_launches()
    out = _run(I, dtype)
    assert n0 == 0 and ops.two_token_head_launches() == 2          # one per call: the forward, the backward
    r = tb.ratios(out, ref, bnd)
    print("two_token_head", case, dtype, {k: round(v, 4) for k, v in r.items()})
    assert set(r) == set(ref) == set(tb.SLACKS) - ({"dWs", "dbs"} if uni else set())
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    # every row of dx between the two tokens is exactly zero (the bound there is 0; said once more in plain words)
    assert bool((out["dx"][:, 1:Nt - 1] == 0).all())
    # save = NULL: bitwise the saving forward; a second saving run: bitwise the first (no atomics, fixed reduction orders)
    nosave = _run(I, dtype, save=False)
    assert ops.two_token_head_launches() == 3
    for k in ("token_a", "token_s", "logits_a", "logits_s"):
        assert torch.equal(nosave[k], out[k]), k
    again = _run(I, dtype)
    for k, v in out.items():
        assert torch.equal(again[k], v), k


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("unified", [False, True], ids=["separate", "unified"])
def test_two_token_head_backward_writes_its_rows_and_no_other(unified, dtype):
    """dx inside a larger canary-filled buffer: every row of the B clips is written (no canary left), the rows just before and after are untouched"""
    Nt, B, D, Ca, Cs = 131, 3, 768, 101, 365
    I = tb.inputs("graded", B, Nt, D, Ca, Cs, dtype, unified, True, True)
    pad = 5
    canary = 12288.0          # exact in bf16
    buf = torch.full((B * Nt + 2 * pad, D), canary, dtype=dtype, device="cuda")
    out = _run(I, dtype, dx_buf=buf, pad_rows=pad)
    host = buf.cpu().float()
    assert bool((host[:pad] == canary).all()) and bool((host[pad + B * Nt:] == canary).all())
    assert not bool((out["dx"].float() == canary).any())
    assert bool((out["dx"][:, 1:Nt - 1] == 0).all()) and bool((out["dx"][:, 0] != 0).any()) and bool((out["dx"][:, Nt - 1] != 0).any())


def test_two_token_head_is_bitwise_repeatable_at_the_training_shape():
    """two calls on the same inputs at Nt = 1570 (the model's token count at 16 frames), bf16, both head modes: bitwise-equal outputs"""
    for unified in (False, True):
        I = tb.inputs("graded", 2, 1570, 768, 400, 365, torch.bfloat16, unified, True, True)
        first, second = _run(I, torch.bfloat16), _run(I, torch.bfloat16)
        for k, v in first.items():
            assert torch.equal(second[k], v), (unified, k)
