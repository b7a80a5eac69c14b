"""Clip ingest on the GPU: devias_clip_ingest through devias_amd.ingest.ClipIngest against the float64 statement and bound of tests/ingest_bounds.py, against what the real
reference computed for every case of tests/golden/ingest_vectors.npz, bitwise on identity boxes; ragged batches, embedded operands, the staging ring, and one training
step of the tiny plain ViT fed through IngestLoader."""
import random
from functools import partial

import numpy as np
import pytest
import torch

import embedded_operands as eo
import ingest_bounds as ib
from devias_amd import synth
from test_ingest_bounds_cpu import FX, SWEEP, TAB
from test_ingest_cpu import make

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def _bits(t):
    return t.detach().float().cpu().contiguous().numpy().view(np.uint32)


def _ingest(crop, dtype=torch.float32):
    from devias_amd.ingest import ClipIngest
    return ClipIngest(crop, out_dtype=dtype, device=DEV)


def _check(name, got, frames, box, S_h, S_w, bf16):
    ref, M = ib.statement(frames, box, S_h, S_w, TAB)
    r, k = ib.worst(got, ref, ib.bound(ref, M, bf16))
    assert r <= 1.0, (name, box, r, k)
    return r


@DTYPES
def test_every_recorded_case_and_a_sweep_of_boxes_within_the_bound(dtype):
    bf16 = dtype == torch.bfloat16
    worst = 0.0
    for name, c in FX.items():
        out = make(c, out_dtype=dtype, device=DEV)(torch.from_numpy(c["frames"])[None].to(DEV), [c["box"]])
        assert out.dtype == dtype and tuple(out.shape) == (1, 3, 2, c["S"], c["S"]) and out.is_cuda
        worst = max(worst, _check(name, out[0].float().cpu().numpy(), c["frames"], c["box"], c["S"], c["S"], bf16))
    m = _ingest((16, 20), dtype)                                   # the sweep: every box of one frame set in ONE call, resized to 16 x 20
    for name in sorted({n for n, _ in SWEEP}):
        boxes = [b for n, b in SWEEP if n == name]
        f = torch.from_numpy(FX[name]["frames"]).to(DEV)
        out = m([f] * len(boxes), boxes).float().cpu().numpy()
        for k, b in enumerate(boxes):
            worst = max(worst, _check(name, out[k], FX[name]["frames"], b, 16, 20, bf16))
    print(f"[ingest kernel, {'bf16' if bf16 else 'fp32'}] at most {worst:.3f} of the bound")


def test_against_the_reference_output_with_no_added_margin():
    """|kernel - reference| <= bound(element) + the case's recorded reference distance: the triangle inequality through the float64 statement"""
    for name, c in FX.items():
        got = make(c, device=DEV)(torch.from_numpy(c["frames"])[None].to(DEV), [c["box"]])[0].cpu().numpy().astype(np.float64)
        ref, M = ib.statement(c["frames"], c["box"], c["S"], c["S"], TAB)
        over = np.abs(got - c["out"]) - (ib.bound(ref, M) + c["ref_dist"])
        assert bool((over <= 0).all()), (name, float(over.max()))


def test_identity_boxes_are_the_reference_bitwise():
    n = 0
    for name, c in FX.items():
        i, j, h, w, fl = c["box"]
        if c["kind"] == "train":
            continue
        assert h == c["S"] and w == c["S"] and not fl
        m = make(c, device=DEV)
        f = torch.from_numpy(c["frames"])[None].to(DEV)
        box = m.center_box(*c["frames"].shape[1:3]) if c["kind"] == "center" else m.test_box(*c["frames"].shape[1:3], int(c["split"][0]), int(c["split"][1]))
        assert np.array_equal(_bits(m(f, [box])[0]), c["out"].view(np.uint32)), name
        n += 1
    assert n >= 12


@DTYPES
def test_ragged_batch_equals_its_clips_one_at_a_time(dtype):
    names = ("t00", "t03", "t06")                                  # 20 x 27, 37 x 23, 8 x 200
    m = _ingest(16, dtype)
    clips = [torch.from_numpy(FX[n]["frames"]) for n in names]
    boxes = [ib.sweep_boxes(*c.shape[1:3], 1, seed=70 + k)[0] for k, c in enumerate(clips)]
    singles = torch.cat([m(c[None].to(DEV), [b]) for c, b in zip(clips, boxes)])
    assert np.array_equal(_bits(m([c.to(DEV) for c in clips], boxes)), _bits(singles))          # a list of device tensors
    assert np.array_equal(_bits(m(clips, boxes)), _bits(singles))                                # a list of host tensors: the staging buffer
    gaps, layout, parts = (5, 33, 2), [], []                                                     # a packed buffer with gaps between the clips
    off = 0
    for c, g in zip(clips, gaps):
        parts.append(torch.full((g,), 255, dtype=torch.uint8))
        off += g
        layout.append((off, c.shape[1], c.shape[2]))
        parts.append(c.reshape(-1))
        off += c.numel()
    buf = torch.cat(parts + [torch.full((7,), 255, dtype=torch.uint8)]).to(DEV)
    assert np.array_equal(_bits(m.ingest_buffer(buf, 2, layout, boxes)), _bits(singles))
    for k, (n, b) in enumerate(zip(names, boxes)):
        _check(n, singles[k].float().cpu().numpy(), FX[n]["frames"], b, 16, 16, dtype == torch.bfloat16)


@DTYPES
def test_more_clips_than_one_launch_carries_rows_for(dtype):
    from devias_amd import _lib
    B = _lib.INGEST_ROWS_PER_LAUNCH + 2
    frames = FX["t00"]["frames"]
    boxes = ib.sweep_boxes(*frames.shape[1:3], B, seed=5)
    out = _ingest(16, dtype)([torch.from_numpy(frames).to(DEV)] * B, boxes).float().cpu().numpy()
    for k, b in enumerate(boxes):
        _check(k, out[k], frames, b, 16, 16, dtype == torch.bfloat16)


def test_a_buffer_smaller_than_one_wide_load():
    """six bytes of frames: the kernel's 8-byte tap loads do not fit, the byte-load form serves"""
    frames = np.array([[[[3, 250, 17], [99, 0, 255]]]], dtype=np.uint8)          # [T = 1, 1, 2, 3]
    for box in ((0, 0, 1, 2, 0), (0, 0, 1, 2, 1), (0, 1, 1, 1, 0)):
        out = _ingest((3, 5))(torch.from_numpy(frames)[None].to(DEV), [box])
        _check("tiny", out[0].cpu().numpy(), frames, box, 3, 5, False)


@DTYPES
@pytest.mark.parametrize("S,lead", [(16, 64), (20, 65), (18, 64)], ids=["S16_aligned", "S20_off_by_one_element", "S18"])
def test_embedded_operands_leave_the_canary_intact(S, lead, dtype):
    """the source inside a larger allocation at an odd byte offset; the output inside a bitwise canary: the 16-byte path (S = 16, aligned base) and the scalar path"""
    names = ("t00", "t03", "t06")
    m = _ingest(S, dtype)
    clips = [torch.from_numpy(FX[n]["frames"]) for n in names]
    boxes = [ib.sweep_boxes(*c.shape[1:3], 1, seed=90 + k)[0] for k, c in enumerate(clips)]
    want = m([c.to(DEV) for c in clips], boxes)
    big = torch.full((3 + sum(c.numel() for c in clips) + 64,), 255, dtype=torch.uint8, device=DEV)
    src = big[3:3 + sum(c.numel() for c in clips)]
    assert src.data_ptr() % 2 == 1
    layout, off = [], 0
    for c in clips:
        src[off:off + c.numel()].copy_(c.reshape(-1))
        layout.append((off, c.shape[1], c.shape[2]))
        off += c.numel()
    R = 3 * 3 * 2 * S
    buf, view = eo.embed(torch.zeros((R, S), dtype=dtype, device=DEV), S, lead, fill=eo.CANARY)
    out = view.view(3, 3, 2, S, S)
    assert out.is_contiguous() and (out.data_ptr() % 16 == 0) == (lead == 64)
    m.ingest_buffer(src, 2, layout, boxes, out=out)
    torch.cuda.synchronize()
    assert eo.intact(buf, (R, S), S, lead, fill=eo.CANARY)
    assert np.array_equal(_bits(out), _bits(want))
    assert bool((big[:3] == 255).all()) and bool((big[3 + off:] == 255).all())


def test_successive_calls_from_host_tensors_reuse_the_staging_ring():
    m = _ingest(16)
    g = torch.Generator().manual_seed(11)
    batches = [torch.randint(0, 256, (2, 2, 20 + k, 27, 3), dtype=torch.uint8, generator=g) for k in range(m.RING + 2)]          # growing: every slot is reallocated once
    boxes = [ib.sweep_boxes(b.shape[2], b.shape[3], 2, seed=k) for k, b in enumerate(batches)]
    outs = [m(b, bx) for b, bx in zip(batches, boxes)]              # no synchronisation between the calls
    torch.cuda.synchronize()
    assert m._slot == (m.RING + 2) % m.RING and all(e is not None for e in m._events)
    for b, bx, o in zip(batches, boxes, outs):
        assert np.array_equal(_bits(o), _bits(m(b.to(DEV), bx)))


def test_one_training_step_through_the_loader_is_the_step_on_the_ingested_clip():
    from devias_amd import engine_for_finetuning as eng
    from devias_amd.ingest import IngestLoader
    from devias_amd.losses import LabelSmoothingCrossEntropy
    from devias_amd.modeling_finetune import VisionTransformer
    model = VisionTransformer(num_classes=17, compute_dtype="fp32", embed_dim=384, depth=2, num_heads=6, qkv_bias=True, all_frames=2, init_scale=1.0,
                              norm_layer=partial(torch.nn.LayerNorm, eps=1e-6))
    synth.fill_module_(model, seed=0)
    model = model.to(DEV).train()
    g = torch.Generator().manual_seed(3)
    frames = torch.randint(0, 256, (2, 2, 240, 250, 3), dtype=torch.uint8, generator=g)
    y = synth.targets(2, 17, seed=40)
    m, crit = _ingest(224), LabelSmoothingCrossEntropy(0.1)
    random.seed(21)
    np.random.seed(22)
    clip = m(frames)
    assert tuple(clip.shape) == (2, 3, 2, 224, 224) and clip.is_cuda
    want, _ = eng.train_class_batch(model, clip, y.to(DEV), crit)
    random.seed(21)
    np.random.seed(22)
    stats = eng.train_one_epoch(model, crit, IngestLoader([(frames, y, None, None)], m, mode="train"), torch.optim.SGD(model.parameters(), lr=0.0), DEV, 0,
                                check_finite_every=1)
    assert np.isfinite(stats["loss"]) and stats["loss"] == float(want.detach())
