#!/usr/bin/env python3
"""What the forward-only encoder region (devias_encoder_block_infer) buys, measured in ONE process on the device's own clock.

    python tools/infer_time.py [--batch 32] [--windows 9] [--out profiles/infer.txt]

ViT-B/16, 16 x 224^2, bf16.  Every comparison alternates its arms window by window (arm 1, arm 2, arm 1 again ... in each of >= 9 windows), times a window with a
HIP event pair, and reports median and min..max per arm.  The baseline arm runs TWICE per window under two labels (an A/A pair): the difference of those two medians
is the spread that a real difference has to exceed.
  1. the student's forward under no_grad (model.eval()), modeling_slot._INFER off against on
  2. the frozen teacher's forward (1569 tokens per clip), off against on
  3. torch.cuda.max_memory_allocated around one student forward under no_grad, off and on, beside what the size functions say"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def ab(title, arms, windows, iters, log):
    """arms: [(label, fn)]; the first arm is the baseline and runs again at the end of every window as `label (A/A)`"""
    arms = arms + [(arms[0][0] + " (A/A)", arms[0][1])]
    for _, fn in arms:                     # warm-up: workspaces, weight copies, clocks
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {label: [] for label, _ in arms}
    for _ in range(windows):
        for label, fn in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[label].append(e0.elapsed_time(e1) / iters)
    med = {k: statistics.median(v) for k, v in ms.items()}
    base = arms[0][0]
    spread = abs(med[base] - med[base + " (A/A)"])
    log(f"== {title}: {windows} windows x {iters} calls per arm, ms per call")
    for label, _ in arms:
        v = ms[label]
        log(f"   {label:34s} median {med[label]:9.4f}   min..max {min(v):9.4f} .. {max(v):9.4f}")
    for label, _ in arms[1:-1]:
        d = med[label] - med[base]
        log(f"   {label} - {base}: {d:+.4f} ms ({100.0 * d / med[base]:+.2f} %); A/A spread {spread:.4f} ms -> "
            + ("faster by more than the spread" if d < -spread else "slower by more than the spread" if d > spread else "within the spread"))
    return med, spread


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.windows >= 9
    import devias_amd.modeling_slot as ms
    from devias_amd import _lib, create_model, synth
    from devias_amd.modeling_finetune import vit_base_patch16_224
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    B, N, D, H, hid = args.batch, 1568, 768, 12, 3072
    dev = torch.device("cuda:0")
    log(f"tools/infer_time.py: {torch.cuda.get_device_name(dev)}, ViT-B/16 16x224^2 bf16, B = {B}, library ABI {_lib.load().devias_version()}")
    student = create_model("slot_vit_base_patch16_224", img_size=224, num_classes=400, all_frames=16, tubelet_size=2, init_scale=0.001, num_latents=2, head_type="linear",
                           slot_matching="matching", agg_weights_tie=True, agg_depth=8, num_scene_classes=365, compute_dtype="bf16")
    teacher = vit_base_patch16_224(num_classes=365, all_frames=16, tubelet_size=2, use_mean_pooling=False, init_scale=0.001, compute_dtype="bf16")
    with torch.no_grad():
        synth.fill_module_(student, seed=0)
        synth.fill_module_(teacher, seed=1)
    student, teacher = student.to(dev).eval(), teacher.to(dev).eval()
    x = synth.video(B, 16, 224).to(dev).bfloat16()

    def fwd(model, on):
        def run():
            ms._INFER = on
            with torch.no_grad():
                return model(x)
        return run

    keep = ms._INFER
    try:
        # 3. memory first, while nothing but the weights and the clips is allocated: one forward each, absolute peaks (the forward-only workspace is grow-only and stays)
        mem = {}
        for on in (False, True):
            torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev) / 2 ** 20
            out = fwd(student, on)()
            torch.cuda.synchronize()
            mem[on] = (before, torch.cuda.max_memory_allocated(dev) / 2 ** 20)
            del out
        ab("1. student forward, no_grad", [("_INFER off (training forward)", fwd(student, False)), ("_INFER on (forward-only region)", fwd(student, True))], args.windows, 3, log)
        ab("2. teacher forward", [("_INFER off (per-kernel loop)", fwd(teacher, False)), ("_INFER on (forward-only region)", fwd(teacher, True))], args.windows, 3, log)
    finally:
        ms._INFER = keep
    M = B * N
    lib = _lib.load()
    save = lib.devias_encoder_block_save_bytes(B, N, D, H, hid, _lib.BF16) / 2 ** 20
    ws = lib.devias_encoder_block_infer_workspace_bytes(B, N, M, D, H, hid, _lib.BF16) / 2 ** 20
    log(f"== 3. memory, student forward under no_grad (MiB): size functions: save arena {save:.1f} per block x {len(student.blocks)} blocks (each a fresh allocation), "
        f"forward-only workspace {ws:.1f} ONCE; saved pre-activation no longer written: {M * hid * 2 / 2 ** 20:.1f} per block")
    log(f"   torch.cuda.max_memory_allocated over one forward (allocated before it -> peak): _INFER off {mem[False][0]:.1f} -> {mem[False][1]:.1f}, "
        f"on {mem[True][0]:.1f} -> {mem[True][1]:.1f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
