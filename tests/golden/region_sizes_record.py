#!/usr/bin/env python3
"""Record what every arena / scratch / workspace size query of the fused-region units (csrc/regions.hip, fusion_head.hip, token_head.hip) returns, as
tests/golden/region_sizes.json: the table tests/test_region_sizes_cpu.py holds the library to, exactly.

    python tests/golden/region_sizes_record.py [path/to/libdevias_amd.so]          # default: the library of this tree

Run it on the library of the commit BEFORE a change that must leave the arena layouts alone, and commit the table with that change.  No device is needed: the
split policies behind the workspace sizes count on the device's compute units and fall back to 256 (MI355X) without one, which is what the table holds.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
F32, BF16 = 0, 1
AGG_FIELDS = ("B", "N", "S", "D", "depth", "tied", "heads", "dh", "ff")


def cases():
    """[(function, positional int arguments or a dict of devias_agg_args fields)]: per region the smallest accepted case and the recipe's, fp32 and bf16"""
    out = []
    for dt in (F32, BF16):
        for B, N, D, H, hid in ((1, 8, 64, 1, 256), (12, 1568, 768, 12, 3072)):
            for q in ("save", "scratch", "workspace"):
                out.append((f"devias_encoder_block_{q}_bytes", [B, N, D, H, hid, dt]))
            for rows in (B * N, (B * N + 255) // 256 * 256):          # the forward-only block: exactly B N rows, and padded to whole 256-row tiles
                out.append(("devias_encoder_block_infer_workspace_bytes", [B, N, rows, D, H, hid, dt]))
        for R, D, C, h1, h2, G in ((1, 1, 1, 1, 1, 1), (24, 768, 765, 512, 256, 196)):
            out.append(("devias_head_workspace_bytes", [R, D, C, h1, h2, G, dt]))
            out.append(("devias_head_save_bytes", [R, D, h1, h2, dt]))
        for agg in ((1, 8, 1, 384, 1, 0, 1, 64, 4), (1, 8, 1, 384, 1, 1, 1, 64, 4), (2, 9, 2, 512, 2, 0, 2, 64, 8), (12, 1568, 2, 768, 8, 1, 4, 512, 3072)):
            for q in ("save", "scratch", "workspace"):
                out.append((f"devias_agg_block_{q}_bytes", dict(zip(AGG_FIELDS, agg), dtype=dt)))
        for B, S, D, C, Cd in ((1, 1, 384, 2, 2), (2, 3, 1024, 5, 5), (12, 4, 768, 765, 174), (1, 1, 512, 2, 2)):          # (the last: an unsupported D, 0)
            out.append(("devias_fusion_head_workspace_bytes", [B, S, D, C, Cd, dt]))
            out.append(("devias_fusion_head_save_bytes", [B, D, dt]))
        for B, Nt, D, C in ((1, 1, 384, 2), (2, 65, 1024, 3), (32, 1568, 768, 400), (2, 65, 512, 3)):                      # (the last: an unsupported D, 0)
            out.append(("devias_pool_head_workspace_bytes", [B, Nt, D, C, dt]))
            out.append(("devias_pool_head_save_bytes", [B, D, dt]))
        for B, Nt, D, Ca, Cs, uni in ((1, 2, 384, 2, 2, 0), (3, 65, 1024, 101, 365, 0), (3, 65, 1024, 101, 101, 1), (32, 1570, 768, 400, 365, 0), (32, 1570, 768, 765, 765, 1),
                                      (3, 65, 512, 101, 365, 0)):                                                          # (the last: an unsupported D, 0)
            out.append(("devias_two_token_head_workspace_bytes", [B, Nt, D, Ca, Cs, uni, dt]))
            out.append(("devias_two_token_head_save_bytes", [B, D, dt]))
    for B in (1, 12):
        out.append(("devias_softmax_ce_workspace_bytes", [B]))
    for B in (1, 32):
        out.append(("devias_distill_workspace_bytes", [B]))
    return out


def query(lib, _lib, fn, args):
    """one size query through ctypes (`_lib`: devias_amd._lib, for the argument types and the devias_agg_args mirror)"""
    f = getattr(lib, fn)
    f.restype, f.argtypes = _lib.PROTOTYPES[fn]
    if isinstance(args, dict):
        a = _lib.AggArgs()
        for k, v in args.items():
            setattr(a, k, v)
        return int(f(ctypes.byref(a)))
    return int(f(*args))


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from devias_amd import _lib
    lib = ctypes.CDLL(sys.argv[1]) if len(sys.argv) > 1 else _lib.load()
    table = [{"fn": fn, "args": args, "bytes": query(lib, _lib, fn, args)} for fn, args in cases()]
    with open(os.path.join(HERE, "region_sizes.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in table) + "\n]\n")
    print(f"{len(table)} size queries recorded")


if __name__ == "__main__":
    main()
