"""RandAugment on the GPU: devias_randaug_stats / devias_randaug_apply through devias_amd.randaug.RandAugment, bitwise against what Pillow returned for every per-op and
chain case of tests/golden/randaug_vectors.npz, and bitwise against randaug_cpu on drawn plans over ragged, unaligned, mixed batches; what a skipped layer leaves alone,
the bytes around the clips, the launch counts, and the loader end to end."""
import random

import numpy as np
import pytest
import torch

from test_randaug_cpu import FX, SETS, chains, op_cases

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = 0xA5


def _ra(config="rand-m7-n4-mstd0.5-inc1", interp="bicubic"):
    from devias_amd.randaug import RandAugment
    return RandAugment(config, interp, device=DEV)


def _launches(plans, sizes, resample):
    """kernel launches the plans take: per layer one apply launch per 32 clips with an op, one stats launch per 32 clips whose op needs statistics"""
    from devias_amd import _lib
    from devias_amd import randaug as R
    n = 0
    for k in range(max(len(p) for p in plans)):
        ops = [R.lower(p[k][0], p[k][2], H, W, resample)[0] if k < len(p) and p[k][1] else R.OP_NONE for p, (H, W) in zip(plans, sizes)]
        n += -(-sum(o != R.OP_NONE for o in ops) // _lib.RANDAUG_ROWS_PER_LAUNCH) + -(-sum(o in R.NEEDS_STATS for o in ops) // _lib.RANDAUG_ROWS_PER_LAUNCH)
    return n


@pytest.mark.parametrize("fset", SETS)
def test_every_per_op_case_is_bitwise_pillow(fset):
    """all cases of a frame set as ONE batch per resampling: a clip per case, one layer, mixed ops"""
    from devias_amd import ops
    from devias_amd import randaug as R
    frames = torch.from_numpy(FX["frames." + fset]).to(DEV)
    for code, interp in ((R.BICUBIC, "bicubic"), (R.BILINEAR, "bilinear")):
        cases = [c for c in op_cases(fset) if c[3] == code and (code == R.BICUBIC or c[0] in ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"))]
        if not cases:
            continue
        plans = [[(c[0], True, c[4])] for c in cases]
        ops.counters(reset=True)
        out = _ra(interp=interp)([frames] * len(cases), plans)
        torch.cuda.synchronize()
        assert ops.randaug_launches() == _launches(plans, [frames.shape[1:3]] * len(cases), code)
        for c, o in zip(cases, out):
            assert o.dtype == torch.uint8 and o.is_cuda and np.array_equal(o.cpu().numpy(), c[5]), (fset, c[:4])
    assert np.array_equal(frames.cpu().numpy(), FX["frames." + fset])          # the input is not written


def test_every_chain_is_bitwise_pillow():
    for k, config, interp, frames, seeds, layers, out, nxt in chains():
        ra = _ra(config, interp)
        random.seed(seeds[0])
        np.random.seed(seeds[1])
        got = ra(torch.from_numpy(frames)[None])             # host frames, plans drawn inside
        assert (random.random(), np.random.uniform()) == nxt
        assert tuple(got.shape) == (1,) + frames.shape and got.is_cuda and np.array_equal(got[0].cpu().numpy(), out), k


def _drawn(ra, n, seed):
    random.seed(seed)
    np.random.seed(seed + 1)
    return [ra.draw() for _ in range(n)]


def _embedded(clips, gaps, lead=16, trail=48):
    """the clips packed with `gaps` bytes in front of each into the lower half of a double-sized buffer that sits inside a larger allocation, everything else CANARY"""
    from devias_amd.randaug import RandAugment
    layout, off = [], 0
    for c, g in zip(clips, gaps):
        off += g
        layout.append((off, c.shape[1], c.shape[2]))
        off += c.numel()
    half = RandAugment.half_of(off + 3)
    big = torch.full((lead + 2 * half + trail,), CANARY, dtype=torch.uint8, device=DEV)
    buf = big[lead:lead + 2 * half]
    for c, (o, _, _) in zip(clips, layout):
        buf[o:o + c.numel()].copy_(c.reshape(-1))
    return big, buf, layout, half


def _ragged_clips(T=2):
    g = torch.Generator().manual_seed(9)
    return [torch.randint(0, 256, (T, H, W, 3), dtype=torch.uint8, generator=g) for H, W in ((20, 27), (37, 23), (1, 9), (16, 16), (9, 1), (33, 40), (2, 2), (24, 50))]


@pytest.mark.parametrize("gaps", [(0, 8, 0, 8, 0, 10, 0, 8), (1, 5, 2, 3, 7, 1, 9, 4)], ids=["some_clips_16_byte_aligned", "odd_offsets"])
def test_drawn_plans_on_a_ragged_batch_are_bitwise_the_host_statement_and_touch_nothing_else(gaps):
    from devias_amd import ops
    from devias_amd.randaug import randaug_cpu
    ra, clips = _ra(), _ragged_clips()
    plans = _drawn(ra, len(clips), 200 + sum(gaps))
    plans[3] = [(n, False, ()) for n, _, _ in plans[3]]       # a clip with no layer applied at all
    big, buf, layout, half = _embedded(clips, gaps)
    aligned = sum(o % 16 == 0 for o, _, _ in layout)          # a clip that starts on 16 bytes takes the 16-byte path, any other the byte path
    assert buf.data_ptr() % 16 == 0 and (aligned >= 5 if gaps[0] == 0 else layout[0][0] % 2 == 1 and aligned <= 2)
    ops.counters(reset=True)
    got, where = ra.augment_buffer(buf, 2, layout, plans)
    torch.cuda.synchronize()
    assert got.data_ptr() == buf.data_ptr()                   # a double-sized buffer is used as it is: no copy
    assert ops.randaug_launches() == _launches(plans, [c.shape[1:3] for c in clips], ra.resample)
    host = big.cpu().numpy()
    homes = np.zeros(host.shape, dtype=bool)
    for c, p, (o0, _, _), (o1, H, W) in zip(clips, plans, layout, where):
        assert (H, W) == tuple(c.shape[1:3]) and o1 in (o0, o0 + half)
        assert np.array_equal(host[16 + o1:16 + o1 + c.numel()].reshape(c.shape), randaug_cpu(c, p).numpy())
        homes[16 + o0:16 + o0 + c.numel()] = homes[16 + half + o0:16 + half + o0 + c.numel()] = True
    assert where[3] == layout[3]                              # a clip none of whose layers was applied keeps its bits (checked above) and its offset
    assert bool((host[~homes] == CANARY).all())               # the bands around both halves and every gap between the clips' homes
    assert any(o1 != o0 for (o0, _, _), (o1, _, _) in zip(layout, where)) and any(o1 == o0 for (o0, _, _), (o1, _, _) in zip(layout, where))


def test_a_layer_nobody_applies_launches_nothing_and_identities_are_skipped():
    from devias_amd import ops
    clips = _ragged_clips()[:3]
    plans = [[("Invert", True, ()), ("Rotate", False, ()), ("Rotate", True, (0.0,)), ("Equalize", True, ())],
             [("ShearX", True, (0.2,)), ("Equalize", False, ()), ("ColorIncreasing", True, (1.0,)), ("ContrastIncreasing", True, (1.5,))],
             [("Invert", False, ()), ("Invert", False, ()), ("PosterizeIncreasing", True, (8,)), ("SharpnessIncreasing", False, ())]]
    ra = _ra()
    big, buf, layout, half = _embedded(clips, (0, 0, 0))
    ops.counters(reset=True)
    _, where = ra.augment_buffer(buf, 2, layout, plans)
    torch.cuda.synchronize()
    assert ops.randaug_launches() == 3                        # layer 0: one apply; layers 1 and 2: nothing; layer 3: one stats, one apply
    assert where[0] == layout[0] and where[1][0] == layout[1][0] + half and where[2] == layout[2]
    host = buf.cpu().numpy()
    from devias_amd.randaug import randaug_cpu
    for c, p, (o, _, _) in zip(clips, plans, where):
        assert np.array_equal(host[o:o + c.numel()].reshape(c.shape), randaug_cpu(c, p).numpy())
    assert np.array_equal(host[where[2][0]:where[2][0] + clips[2].numel()], clips[2].reshape(-1).numpy())


def test_a_buffer_that_is_not_double_sized_is_copied_into_one_only_when_a_layer_needs_the_other_half():
    from devias_amd.randaug import randaug_cpu
    ra, c = _ra(), _ragged_clips()[0]
    flat = c.reshape(-1).to(DEV)
    same, where = ra.augment_buffer(flat.clone(), 2, [(0, 20, 27)], [[("Invert", True, ()), ("SolarizeAdd", True, (60,))]])
    assert same.numel() == flat.numel() and where == [(0, 20, 27)]
    assert np.array_equal(same.cpu().numpy().reshape(c.shape), randaug_cpu(c, [("Invert", True, ()), ("SolarizeAdd", True, (60,))]).numpy())
    plan = [("TranslateYRel", True, (-0.3,)), ("SharpnessIncreasing", True, (1.8,)), ("Rotate", True, (17.5,))]
    grown, where = ra.augment_buffer(flat, 2, [(0, 20, 27)], [plan])
    assert grown.numel() == 2 * ra.half_of(flat.numel()) and where[0][0] == ra.half_of(flat.numel())          # three flips: the upper half
    assert np.array_equal(grown[where[0][0]:where[0][0] + flat.numel()].cpu().numpy().reshape(c.shape), randaug_cpu(c, plan).numpy())


def test_more_clips_than_one_launch_carries_rows_for():
    from devias_amd import _lib, ops
    from devias_amd.randaug import randaug_cpu
    B = _lib.RANDAUG_ROWS_PER_LAUNCH + 3
    ra, c = _ra(), _ragged_clips()[0]
    plans = [[("AutoContrast", True, ()), ("ShearY", True, (0.01 * k - 0.17,))] for k in range(B)]
    ops.counters(reset=True)
    out = ra(torch.stack([c] * B).to(DEV), plans)
    torch.cuda.synchronize()
    assert ops.randaug_launches() == 6 and tuple(out.shape) == (B,) + tuple(c.shape)
    for k in (0, 1, B - 4, B - 1):
        assert np.array_equal(out[k].cpu().numpy(), randaug_cpu(c, plans[k]).numpy()), k


def test_the_loader_end_to_end_is_the_ingest_of_the_host_statement_with_the_same_boxes():
    from devias_amd.ingest import ClipIngest, IngestLoader
    from devias_amd.randaug import randaug_cpu
    ra, m = _ra(), ClipIngest(16, device=DEV)
    clips, labels = _ragged_clips()[:4], torch.arange(4)
    for src in (clips, [c.to(DEV) for c in clips]):           # host frames: staged once into the double-sized buffer; device frames: copied, not written
        random.seed(61)
        np.random.seed(62)
        batch, = list(IngestLoader([(src, labels)], m, mode="train", randaug=ra))
        after = (random.random(), np.random.uniform())
        random.seed(61)
        np.random.seed(62)
        plans, boxes = [], []
        for c in clips:
            plans.append(ra.draw())
            boxes.append(m.draw(c.shape[1], c.shape[2]))
        assert (random.random(), np.random.uniform()) == after
        want = m([randaug_cpu(c, p).to(DEV) for c, p in zip(clips, plans)], boxes)
        assert batch[1] is labels and batch[0].is_cuda and np.array_equal(batch[0].cpu().numpy().view(np.uint32), want.cpu().numpy().view(np.uint32))
        assert all(torch.equal(s.cpu(), c) for s, c in zip(src, clips))
