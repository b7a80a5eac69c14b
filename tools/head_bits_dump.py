#!/usr/bin/env python3
"""Every output, every gradient and the stored `a` of the two token-head regions (devias_pool_head_*, devias_two_token_head_*), as raw bytes in ONE file: to hold a
change of csrc/token_head.hip to the bits of the library before it.

    DEVIAS_LIB_PATH=/path/to/the/other/libdevias_amd.so python tools/head_bits_dump.py before.bin
    python tools/head_bits_dump.py after.bin && cmp before.bin after.bin

The inputs are those of tests/pool_head_bounds.py and tests/two_token_head_bounds.py, at the smallest shapes that reach every branch: the pooled head at Nt in {1, 65},
D in {384, 1024}, MEAN and CLS; the two-token head at Nt in {2, 65, 131}, D in {384, 768, 1024}, separate and unified heads, generators graded and tail; masks and
dtoken present; fp32 and bf16; each case with a save arena (forward + backward) and without one (forward alone).  Per tensor a text line `case name dtype shape`, then
its bytes.  The file's sha256 is printed."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _al256(n):
    return (n + 255) // 256 * 256


def _cu(t):
    return t.cuda() if t is not None else None


def pool_case(pool, Nt, D, dtype, save, B=2, C=3):
    import pool_head_bounds as pb
    from devias_amd import ops
    I = pb.inputs("graded", B, Nt, D, C, dtype, True, True)
    keep = [I["W"].to(dtype).cuda(), I["bias"].cuda(), I["gamma"].cuda(), I["beta"].cuda(), I["mask"].cuda()]
    a = ops.pool_head_args(B, Nt, pool, pb.EPS, *keep)
    token, logits, arena = ops.pool_head_fwd(a, I["h"].cuda().view(B * Nt, D), save=save)
    out = {"token": token, "logits": logits}
    if save:
        off = _al256(B * D * 4) + _al256(B * 4)
        out["a"] = arena[off:off + B * D * token.element_size()].clone()
        dx = torch.empty((B * Nt, D), dtype=dtype, device="cuda")
        grads = [torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for s in ((C, D), (C,), (D,), (D,))]
        ops.pool_head_bwd(a, arena, I["dlogits"].cuda(), I["dtoken"].cuda(), dx, grads)
        out.update(dx=dx, dW=grads[0], db=grads[1], dgamma=grads[2], dbeta=grads[3])
    return out


def two_token_case(kind, unified, Nt, D, dtype, save, B=3, Ca=101, Cs=365):
    import two_token_head_bounds as tb
    from devias_amd import ops
    I = tb.inputs(kind, B, Nt, D, Ca, Cs, dtype, unified, True, True)
    keep = [I["Wa"].to(dtype).cuda(), _cu(I["ba"]), _cu(I["Ws"].to(dtype) if I["Ws"] is not None else None), _cu(I["bs"]), I["gamma"].cuda(), I["beta"].cuda(),
            I["mask_a"].cuda(), I["mask_s"].cuda()]
    a = ops.two_token_head_args(B, Nt, tb.EPS, *keep)
    token_a, token_s, logits_a, logits_s, arena = ops.two_token_head_fwd(a, I["h"].cuda().view(B * Nt, D), save=save)
    out = {"token_a": token_a, "token_s": token_s, "logits_a": logits_a, "logits_s": logits_s}
    if save:
        off = _al256(2 * B * D * 4) + _al256(2 * B * 4)
        out["a"] = arena[off:off + 2 * B * D * token_a.element_size()].clone()
        dx = torch.empty((B * Nt, D), dtype=dtype, device="cuda")
        grads = [torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for s in ((a.Ca, D), (a.Ca,), (a.Cs, D), (a.Cs,), (D,), (D,))]
        if unified:
            grads[2] = grads[3] = None
        ops.two_token_head_bwd(a, arena, I["dlogits_a"].cuda(), I["dlogits_s"].cuda(), I["dtoken_a"].cuda(), I["dtoken_s"].cuda(), dx, grads)
        out.update(dx=dx, **{n: g for n, g in zip(("dWa", "dba", "dWs", "dbs", "dgamma", "dbeta"), grads) if g is not None})
    return out


def cases():
    """(case name, function that runs it)"""
    for dtype in (torch.float32, torch.bfloat16):
        for save in (True, False):
            tail = "%s_save%d" % ("fp32" if dtype == torch.float32 else "bf16", save)
            for pool in (0, 1):          # DEVIAS_POOL_MEAN, DEVIAS_POOL_CLS
                for Nt in (1, 65):
                    for D in (384, 1024):
                        yield "pool%d_Nt%d_D%d_%s" % (pool, Nt, D, tail), lambda p=pool, n=Nt, d=D, t=dtype, s=save: pool_case(p, n, d, t, s)
            for unified in (False, True):
                for kind in ("graded", "tail"):
                    for Nt in (2, 65, 131):
                        for D in (384, 768, 1024):
                            yield ("tt_u%d_%s_Nt%d_D%d_%s" % (unified, kind, Nt, D, tail),
                                   lambda k=kind, u=unified, n=Nt, d=D, t=dtype, s=save: two_token_case(k, u, n, d, t, s))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    if not torch.cuda.is_available():
        sys.exit("head_bits_dump.py runs the regions on a GPU: none here")
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
