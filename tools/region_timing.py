"""What the region timing tools (plainvit_time.py, multitask_time.py, downstream_time.py) measure with: alternating blocks of calls timed by device events, the
kernels of one profiled call, and a comparison that carries its own A/A spread."""
from __future__ import annotations

import statistics
import time

import torch


def block(fn, iters):
    """(device-event ms per call, host ms to issue one call)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    t1 = time.perf_counter()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, (t1 - t0) * 1e3 / iters


def med(v, unit="ms"):
    return "%.3f %s (min %.3f, max %.3f, n = %d)" % (statistics.median(v), unit, min(v), max(v), len(v))


def kernels(fn):
    """[(name, device ms)] of one profiled call -- copies and memsets left out --, or None where the profiler gives none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [(str(e.name), e.time_range.elapsed_us() / 1000.0) for e in prof.events()
              if str(getattr(e, "device_type", "")).endswith("CUDA") and not str(e.name).lower().startswith(("memcpy", "memset"))]
        return ev or None
    except Exception as e:          # noqa: BLE001
        print("profiler unavailable:", e)
        return None


def kernel_summary(k):
    return "%d kernels, %.3f ms of kernel time in one profiled call" % (len(k), sum(t for _, t in k)) if k else "kernels: not measured"


def compare(name, new, old, rounds, iters, warm=5, old_name="eager ATen", profiled=True):
    """new / new again / old in alternating blocks -> report lines; the A/A spread is |median(new) - median(new again)|"""
    for fn in (new, old):
        for _ in range(warm):
            fn()
    a, a2, o = [], [], []
    for _ in range(rounds):
        a.append(block(new, iters)); o.append(block(old, iters)); a2.append(block(new, iters))
    ka, ko = (kernels(new), kernels(old)) if profiled else (None, None)
    ma, ma2, mo = (statistics.median(v[0] for v in s) for s in (a, a2, o))
    lines = ["%s: fused       per call %s; host issue %s; %s" % (name, med([v[0] for v in a]), med([v[1] for v in a]), kernel_summary(ka)),
             "    fused again (A/A) per call %s; host issue %s" % (med([v[0] for v in a2]), med([v[1] for v in a2])),
             "    %-17s per call %s; host issue %s; %s" % (old_name, med([v[0] for v in o]), med([v[1] for v in o]), kernel_summary(ko)),
             "    device-event time: %s / fused = %.2fx; A/A spread %.3f ms (%.1f %% of fused)%s" % (
                 old_name, mo / ma, abs(ma - ma2), 100.0 * abs(ma - ma2) / ma,
                 "; kernel time %.2fx" % (sum(t for _, t in ko) / sum(t for _, t in ka)) if ka and ko else "")]
    if ka:
        lines.append("    the fused kernels: " + ", ".join("%s %.1f us" % (n.split("(")[0][-36:], t * 1e3) for n, t in ka))
    return lines
