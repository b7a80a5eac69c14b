#!/usr/bin/env python3
"""Every output of every slot cross-attention entry point (devias_slot_attn_fwd / _bwd / _kv_grad, devias_slotf_fwd / _bwd / _pack through slotf_context_grad), as raw
bytes in ONE file: to hold a change of csrc/slot_*.hip to the bits of the library before it.

    DEVIAS_LIB_PATH=/path/to/the/other/libdevias_amd.so python tools/slot_bits_dump.py before.bin
    python tools/slot_bits_dump.py after.bin && cmp before.bin after.bin

The inputs are those of tests/slot_loss_bounds.py (generators diffuse and starved), at the smallest shapes that reach every instantiation and both sides of every chunk edge:
  folded, matrix cores   bf16, B = 2, (S, h) in (1, 4), (2, 4), (4, 4), D in {512, 768, 1024}, N in {7, 129}, with and without d_attn_ext
  folded, VALU           fp32, and bf16 under ops.options(slot_mfma=0); B = 2, S in {2, 3}, h = 4, D in {384, 1024}, N in {7, 65}
  unfolded               both dtypes, B = 2, S in {2, 3, 5} (the three MAXS forms), h = 2, N in {7, 65}
  kv_grad                both dtypes, B = 2, S = 3, h = 2, N = 65, L = 6 (18 pairs: crosses one group of 16)
  context grad           both dtypes, B = 2, S = 2, h = 4, D = 512, N = 13 (N % 8 != 0), L = 2
Each call is checked by launch counter to have been served by the family it names (as tests/test_slot_loss_bounds_gpu.py does).  Per tensor a text line
`case name dtype shape`, then its bytes.  The file's sha256 is printed."""
import contextlib
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda"
FAMILIES = ("slotm", "slotf_valu", "slot")


def served(fn, **want):
    """run fn() with fresh counters; the slot-attention family counters must be exactly `want` (those not named: 0)"""
    from devias_amd import ops
    ops.counters(reset=True)
    out = fn()
    torch.cuda.synchronize()
    cnt = ops.counters()
    got = {k: cnt[k] for k in FAMILIES}
    assert got == {k: want.get(k, 0) for k in FAMILIES}, (want, got)
    return out


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def layer_case(kind, family, folded, dtype, B, S, N, h, D, ext_on):
    """one forward and one backward call of a family: attn, rsum, out, dq, ds"""
    import slot_loss_bounds as sb
    from devias_amd import ops
    q, src, d_o, ext = sb.slot_inputs(kind, B, S, N, h, D, dtype, folded, seed=20, device=DEV)
    ext = ext if ext_on else None
    scale = sb.SLOT_SCALE
    no_mfma = ops.options(slot_mfma=0) if family == "slotf_valu" and dtype == torch.bfloat16 else contextlib.nullcontext()
    with no_mfma:
        if folded:
            attn, rsum, out = served(lambda: ops.slotf_fwd(q, src, B, S, N, h, D, scale, attn_out=nan(B * h, S, N), rsum_out=nan(B * h, S)), **{family: 1})
            dq, ds = served(lambda: ops.slotf_bwd(src, attn, rsum, out, d_o, ext, B, S, N, h, D, scale, ds_out=nan(B * h, S, N)), **{family: 1})
        else:
            attn, rsum, out = served(lambda: ops.slot_attn_fwd(q, src, B, S, N, h, D, scale, attn_out=nan(B * h, S, N), rsum_out=nan(B * h, S)), **{family: 1})
            dq, ds = served(lambda: ops.slot_attn_bwd(q, src, attn, rsum, out, d_o, ext, B, S, N, h, D, scale, ds_out=nan(B * h, S, N)), **{family: 1})
    return {"attn": attn, "rsum": rsum, "out": out, "dq": dq, "ds": ds}


def kv_grad_case(dtype, L=6, B=2, S=3, N=65, h=2, D=512):
    import slot_loss_bounds as sb
    from devias_amd import ops
    t = sb.stacked_inputs(L, B, S, N, h, D, dtype, seed=30, device=DEV)
    return {"dkv": served(lambda: ops.slot_attn_kv_grad(*t, L, B, S, N, h, D, sb.SLOT_SCALE), slot=1)}


def context_grad_case(dtype, L=2, B=2, S=2, N=13, h=4, D=512):
    import slot_loss_bounds as sb
    from devias_amd import ops
    qs, dzs, ds, A, r = sb.stacked_inputs(L, B, S, N, h, D, dtype, seed=31, device=DEV)
    return {"dc": served(lambda: ops.slotf_context_grad(A, r, ds, dzs, qs, L, B, S, N, h, D, sb.SLOT_SCALE))}      # devias_slotf_pack counts nothing


def cases():
    """(case name, function that runs it)"""
    BF, F32 = torch.bfloat16, torch.float32
    name = {BF: "bf16", F32: "fp32"}
    for kind in ("diffuse", "starved"):
        for S, h in ((1, 4), (2, 4), (4, 4)):
            for D in (512, 768, 1024):
                for N in (7, 129):
                    for ext_on in (True, False):
                        yield ("slotm_%s_S%d_h%d_D%d_N%d_ext%d" % (kind, S, h, D, N, ext_on),
                               lambda k=kind, s=S, hh=h, d=D, n=N, e=ext_on: layer_case(k, "slotm", True, BF, 2, s, n, hh, d, e))
        for dtype in (F32, BF):
            for S in (2, 3):
                for D in (384, 1024):
                    for N in (7, 65):
                        yield ("slotf_valu_%s_%s_S%d_D%d_N%d" % (kind, name[dtype], S, D, N),
                               lambda k=kind, t=dtype, s=S, d=D, n=N: layer_case(k, "slotf_valu", True, t, 2, s, n, 4, d, True))
            for S in (2, 3, 5):
                for N in (7, 65):
                    yield ("slot_%s_%s_S%d_N%d" % (kind, name[dtype], S, N), lambda k=kind, t=dtype, s=S, n=N: layer_case(k, "slot", False, t, 2, s, n, 2, 512, True))
    for dtype in (F32, BF):
        yield "kv_grad_%s" % name[dtype], lambda t=dtype: kv_grad_case(t)
        yield "context_grad_%s" % name[dtype], lambda t=dtype: context_grad_case(t)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    if not torch.cuda.is_available():
        sys.exit("slot_bits_dump.py runs the kernels on a GPU: none here")
    if "DEVIAS_SLOT_MFMA" in os.environ:
        sys.exit("slot_bits_dump.py: DEVIAS_SLOT_MFMA is set; it moves calls between the kernel families checked here")
    from devias_amd import _lib
    digest, n = hashlib.sha256(), 0
    with open(sys.argv[1], "wb") as f:
        for name, run in cases():
            out = run()
            torch.cuda.synchronize()
            for k, t in out.items():
                raw = t.contiguous().cpu().view(torch.uint8).numpy().tobytes()
                head = ("%s %s %s %s\n" % (name, k, str(t.dtype), tuple(t.shape))).encode()
                f.write(head); f.write(raw)
                digest.update(head); digest.update(raw)
                n += 1
    print("%s: %d tensors of %s, sha256 %s" % (sys.argv[1], n, _lib.LIB_PATH, digest.hexdigest()))


if __name__ == "__main__":
    main()
