#!/usr/bin/env python3
"""Device time of the matching loss, forward + backward, teacher entry points against label entry points, in one process on one GPU:

    python tools/loss_labels_time.py [--batch 32] [--slots 2] [--nb 400] [--ns 365] [--dtype bf16]

Both paths see the same student outputs; the teacher logits carry their argmax on the label, so with scene_ce = 1 both compute the same numbers
(checked before timing).  The two are timed in alternating windows of `--iters` launches between device events, `--rounds` windows each; the line
printed is the median window of each path in microseconds per forward + backward, and the spread (min..max) of the windows.  A pair is three launches
of 4-25 us, so a window measures the host's enqueue where that is the longer; for the kernels' own durations run the script under the profiler,
`rocprofv3 --kernel-trace --stats -d OUT -o loss -- python tools/loss_labels_time.py --iters 100 --rounds 3`, and read the loss_fwd_kernel / loss_bwd_kernel
dispatches (template argument LABELS = true / false) from its output."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devias_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--slots", type=int, default=2)
    ap.add_argument("--nb", type=int, default=400)
    ap.add_argument("--ns", type=int, default=365)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    B, S, nb, ns, D, G, N, nh = a.batch, a.slots, a.nb, a.ns, 768, 196, 1568, 4
    g = torch.Generator().manual_seed(1)
    Z = (torch.randn(B * S, nb + ns, generator=g) * 2).to(dt).cuda()
    slots = torch.randn(B * S, D, generator=g).to(dt).cuda()
    maskp = torch.rand(B * S, G, generator=g).to(dt).cuda()
    attn = torch.softmax(torch.randn(B * nh, S, N, generator=g), dim=1).cuda()
    y, ys = torch.randint(0, nb, (B,), generator=g).cuda(), torch.randint(0, ns, (B,), generator=g).cuda()
    fg, fgN = (torch.randint(0, 257, (B, G), generator=g) / 256.0).cuda(), (torch.randint(0, 257, (B, N), generator=g) / 256.0).cuda()
    teacher = torch.randn(B, ns, generator=g).cuda()
    teacher[torch.arange(B, device="cuda"), ys] = 20.0
    one = torch.ones(1, device="cuda")

    def run_teacher(scene_ce):
        losses, match, _ = ops.head_match_loss_fwd(Z, slots, maskp, attn, teacher, y, fg, fgN, nb, 4000.0, 1.0, 1.0, scene_ce)
        return losses, ops.head_match_loss_bwd(Z, slots, maskp, attn, teacher, y, fg, fgN, match, one, nb, 4000.0, 1.0, 1.0, scene_ce)

    def run_labels():
        losses, match, _ = ops.head_match_loss_labels_fwd(Z, slots, maskp, attn, y, ys, fg, fgN, nb, 1.0, 1.0)
        return losses, ops.head_match_loss_labels_bwd(Z, slots, maskp, attn, y, ys, fg, fgN, match, one, nb, 1.0, 1.0)

    lt, gt = run_teacher(True)
    ll, gl = run_labels()
    assert torch.equal(lt, ll) and all(torch.equal(p, q) for p, q in zip(gt, gl)), "the two paths disagree"
    paths = {"teacher_kl": lambda: run_teacher(False), "teacher_ce": lambda: run_teacher(True), "labels": run_labels}
    times = {k: [] for k in paths}
    for f in paths.values():                       # warm-up: code objects, workspace
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.iters)
    out = {"what": "matching loss forward + backward, microseconds per pair between device events (host enqueue included where it is the longer)",
           "shape": dict(B=B, S=S, nb=nb, ns=ns, D=D, G=G, N=N, nh=nh, dtype=a.dtype), "iters": a.iters, "rounds": a.rounds}
    for k, v in times.items():
        out[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
