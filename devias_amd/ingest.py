"""Clip ingest on the device: what the reference's workers do to a decoded clip after RandAugment -- ToTensor (/255), tensor_normalize, random_resized_crop, horizontal_flip
(dataset/kinetics.py:_aug_frame; the same lines in ssv2.py, hvu.py, activitynet.py, hat_decode.py) -- and, for validation / test, after the short-side Resize: CenterCrop
or the view's window, ClipToTensor, Normalize.  The frames cross the bus as uint8 (a quarter of the fp32 clip) and ONE kernel launch (devias_clip_ingest) writes the clip.

The draws are the reference's, on the host, from Python's `random` and numpy's global state in the reference's order and amount (ClipIngest.draw); the boxes reach the
device as kernel arguments.  RandAugment, which the reference runs on the uint8 frames before all of this, is devias_amd.randaug's: IngestLoader(..., randaug=...) draws
its plan before each clip's box and runs it on the staged buffer that the ingest then reads.  Out of scope: decoding, the short-side Resize of validation / test (the
worker's antialiased uint8 resize), motion_shift, random erasing, FastCollateMixup."""
from __future__ import annotations

import math
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
Box = Tuple[int, int, int, int, int]          # i, j, h, w, flip


def tap_table(mean=MEAN, std=STD) -> torch.Tensor:
    """fp32 [3, 256]: every value a normalised tap can take, fl(fl(fl(u / 255) - m_c) / s_c), by the reference's three fp32 operations"""
    u = torch.arange(256, dtype=torch.float32) / 255.0
    return ((u[None, :] - torch.tensor(list(mean), dtype=torch.float32)[:, None]) / torch.tensor(list(std), dtype=torch.float32)[:, None]).contiguous()


def resize_taps(n_in: int, n_out: int, flip: bool = False):
    """first tap, second tap (int64 [n_out]) and the second's weight (fp32 [n_out]) of the half-pixel rule src = max((d + 0.5) n_in / n_out - 0.5, 0), from integers as
    the kernel computes them: ((2d + 1) n_in - n_out) / (2 n_out) has the first tap as quotient and lambda as remainder / (2 n_out), rounded once.  flip: for output
    index x the source side index is n_out - 1 - x."""
    d = torch.arange(n_out, dtype=torch.int64)
    if flip:
        d = n_out - 1 - d
    num, den = (2 * d + 1) * n_in - n_out, 2 * n_out
    pos = num > 0
    i0 = torch.where(pos, torch.div(num.clamp(min=0), den, rounding_mode="floor"), torch.zeros_like(num))
    rem = torch.where(pos, num.clamp(min=0) % den, torch.zeros_like(num))
    lam = rem.to(torch.float32) / torch.tensor(float(den), dtype=torch.float32)
    return i0, torch.clamp(i0 + 1, max=n_in - 1), lam


def ingest_cpu(frames: torch.Tensor, box: Box, table: torch.Tensor, S_h: int, S_w: int, out_dtype=torch.float32) -> torch.Tensor:
    """the kernel's arithmetic restated with torch on the host for ONE clip: uint8 [T, H0, W0, 3] -> [3, T, S_h, S_w]; every product and sum is one fp32 torch operation,
    rounded on its own as in the kernel"""
    i, j, h, w, flip = (int(v) for v in box)
    f = frames[:, i:i + h, j:j + w, :].to(torch.int64)
    x = torch.stack([table[c][f[..., c]] for c in range(3)])                # [3, T, h, w] taps
    r0, r1, ly = resize_taps(h, S_h)
    c0, c1, lx = resize_taps(w, S_w, bool(flip))
    ly = ly[:, None]
    wy0, wx0 = 1.0 - ly, 1.0 - lx
    top, bot = x[:, :, r0], x[:, :, r1]
    p = wx0 * top[..., c0] + lx * top[..., c1]
    q = wx0 * bot[..., c0] + lx * bot[..., c1]
    return (wy0 * p + ly * q).to(out_dtype)


def check_clips(frames, who: str = "ClipIngest"):
    """the clips of a batch given as uint8 [B, T, H0, W0, 3] or as a list of B tensors [T, H0_b, W0_b, 3] -> (list of clips, T)"""
    clips: List[torch.Tensor] = list(frames) if isinstance(frames, (list, tuple)) else None
    if clips is None:
        if not (isinstance(frames, torch.Tensor) and frames.dim() == 5):
            raise ValueError(f"{who}: uint8 frames [B, T, H0, W0, 3] or a list of B tensors [T, H0, W0, 3] expected")
        clips = list(frames.unbind(0))
    if not clips or any(not isinstance(c, torch.Tensor) or c.dtype != torch.uint8 or c.dim() != 4 or c.shape[3] != 3 or c.numel() == 0 for c in clips):
        raise ValueError(f"{who}: every clip is a non-empty uint8 tensor [T, H0, W0, 3]")
    T = clips[0].shape[0]
    if any(c.shape[0] != T for c in clips) or len({c.device for c in clips}) != 1:
        raise ValueError(f"{who}: the clips of a batch share T and the device")
    return clips, T


class ClipIngest:
    """uint8 frames -> the normalised, cropped, resized, flipped clip [B, 3, T, S, S] on the device, one launch.

    draw(H0, W0)                         the reference's random_resized_crop box and flip for one clip, from `random` and `numpy.random` in the reference's order
    center_box / test_box                the validation CenterCrop and the test view's window (kinetics.py:202-229): identity boxes, no draws
    __call__(frames, boxes=None)         frames: uint8 [B, T, H0, W0, 3] or a list of B tensors [T, H0_b, W0_b, 3], on the host or on the device; boxes: one
                                         (i, j, h, w, flip) per clip, drawn here where None.  Host frames are packed into a pinned staging buffer of a small ring and
                                         copied with one non_blocking transfer; the launch goes to the current stream.
    On a CPU device the clip is computed by ingest_cpu, a torch restatement of the kernel's arithmetic (the class and IngestLoader can be exercised without a GPU)."""
    RING = 3

    def __init__(self, crop_size=224, mean=MEAN, std=STD, scale=(0.08, 1.0), ratio=(0.75, 1.3333), flip=True, out_dtype=torch.float32, device=None):
        self.S_h, self.S_w = (int(crop_size), int(crop_size)) if isinstance(crop_size, (int, np.integer)) else (int(crop_size[0]), int(crop_size[1]))
        if self.S_h < 1 or self.S_w < 1:
            raise ValueError(f"ClipIngest: crop_size {crop_size}")
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"ClipIngest: out_dtype float32 or bfloat16, got {out_dtype}")
        self.crop_size, self.mean, self.std, self.scale, self.ratio, self.flip, self.out_dtype = crop_size, tuple(mean), tuple(std), tuple(scale), tuple(ratio), bool(flip), out_dtype
        self.device = torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.table = tap_table(self.mean, self.std)        # host copy; the device copy is made once per device (_table_on)
        self._tables = {}
        self._host = [None] * self.RING                     # pinned staging buffers, grown on demand
        self._events = [None] * self.RING
        self._slot = 0

    # ---- the boxes (host only) -----------------------------------------------------------------------------------------------------------------------
    def draw(self, H0: int, W0: int) -> Box:
        """video_transforms._get_param_spatial_crop (:498-537) and horizontal_flip's draw (:175) for one clip of H0 x W0 frames.  Per attempt: random.uniform (area),
        random.uniform (log ratio), one np.random.uniform() (the reference evaluates it although switch_hw is False), and on success two random.randint; after ten
        failed attempts the central fallback box.  Then, unless flip=False (SSV2), one np.random.uniform() for the flip."""
        height, width = int(H0), int(W0)
        box = None
        for _ in range(10):
            area = height * width
            target_area = random.uniform(*self.scale) * area
            log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
            aspect_ratio = math.exp(random.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            np.random.uniform()
            if 0 < w <= width and 0 < h <= height:
                i = random.randint(0, height - h)
                j = random.randint(0, width - w)
                box = (i, j, h, w)
                break
        if box is None:
            in_ratio = float(width) / float(height)
            if in_ratio < min(self.ratio):
                w = width
                h = int(round(w / min(self.ratio)))
            elif in_ratio > max(self.ratio):
                h = height
                w = int(round(h * max(self.ratio)))
            else:
                w, h = width, height
            box = ((height - h) // 2, (width - w) // 2, h, w)
        flipped = int(np.random.uniform() < 0.5) if self.flip else 0
        return box + (flipped,)

    def center_box(self, H0: int, W0: int) -> Box:
        """video_transforms.CenterCrop (:1164-1166)"""
        if self.S_w > W0 or self.S_h > H0:
            raise ValueError(f"center_box: a {H0} x {W0} frame is smaller than the {self.S_h} x {self.S_w} crop")
        return int(round((H0 - self.S_h) / 2.)), int(round((W0 - self.S_w) / 2.)), self.S_h, self.S_w, 0

    def test_box(self, H0: int, W0: int, split_nb: int, num_crop: int = 3) -> Box:
        """kinetics.py:202-229: the window of view `split_nb` of `num_crop` along the longer side of a frame whose shorter side is the crop size"""
        S = self.S_h
        if self.S_h != self.S_w or min(H0, W0) != S:
            raise ValueError(f"test_box: the frame's short side must be the (square) crop size {self.S_h} x {self.S_w}, got {H0} x {W0}")
        if num_crop > 1:
            spatial_step = 1.0 * (max(H0, W0) - S) / (num_crop - 1)
            start = int(int(split_nb) * spatial_step)
        else:
            start = (max(H0, W0) - S) // 2
        return (start, 0, S, S, 0) if H0 >= W0 else (0, start, S, S, 0)

    # ---- the device side -----------------------------------------------------------------------------------------------------------------------------
    def _table_on(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._tables:
            self._tables[key] = self.table.to(device)
        return self._tables[key]

    def _stage(self, clips: Sequence[torch.Tensor], nbytes: int, device, alloc: Optional[int] = None) -> torch.Tensor:
        """the host clips packed back to back into the next pinned buffer of the ring and copied to a fresh device buffer with one non_blocking transfer; alloc: the
        device buffer's size where it is to be larger than the clips (RandAugment's double-sized buffer: the clips fill its lower part)"""
        s = self._slot
        self._slot = (s + 1) % self.RING
        if self._events[s] is not None:
            self._events[s].synchronize()                   # the copy that last read this pinned buffer has finished
        if self._host[s] is None or self._host[s].numel() < nbytes:
            self._host[s] = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        host, off = self._host[s], 0
        for c in clips:
            n = c.numel()
            host[off:off + n].view(c.shape).copy_(c)
            off += n
        dev = torch.empty(max(nbytes, int(alloc or 0)), dtype=torch.uint8, device=device)
        dev[:nbytes].copy_(host[:nbytes], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._events[s] = ev
        return dev

    def ingest_buffer(self, buf: torch.Tensor, T: int, layout: Sequence[Tuple[int, int, int]], boxes: Sequence[Box], out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """one launch over a flat uint8 device buffer: layout[b] = (byte offset, H0, W0) of clip b's [T, H0, W0, 3] frames; out: a contiguous [B, 3, T, S_h, S_w] tensor of
        out_dtype to write into (allocated where None)"""
        from . import ops
        B = len(layout)
        if len(boxes) != B:
            raise ValueError(f"ClipIngest: {len(boxes)} boxes for {B} clips")
        rows = (_lib.IngestRow * B)(*[_lib.IngestRow(int(off), int(H0), int(W0), int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(b[4]), 0) for (off, H0, W0), b in zip(layout, boxes)])
        if out is None:
            out = torch.empty((B, 3, int(T), self.S_h, self.S_w), dtype=self.out_dtype, device=buf.device)
        return ops.clip_ingest(buf, self._table_on(buf.device), rows, int(T), out)

    def __call__(self, frames, boxes: Optional[Sequence[Box]] = None) -> torch.Tensor:
        clips, T = check_clips(frames)
        if boxes is None:
            boxes = [self.draw(c.shape[1], c.shape[2]) for c in clips]
        if len(boxes) != len(clips):
            raise ValueError(f"ClipIngest: {len(boxes)} boxes for {len(clips)} clips")
        src_dev = clips[0].device
        device = src_dev if src_dev.type != "cpu" else self.device
        if device.type == "cpu":
            for c, b in zip(clips, boxes):
                i, j, h, w, fl = (int(v) for v in b)
                if h < 1 or w < 1 or i < 0 or j < 0 or i + h > c.shape[1] or j + w > c.shape[2] or fl not in (0, 1):
                    raise ValueError(f"ClipIngest: box {tuple(b)} is empty or leaves its {c.shape[1]} x {c.shape[2]} frame")
            return torch.stack([ingest_cpu(c, b, self.table, self.S_h, self.S_w, self.out_dtype) for c, b in zip(clips, boxes)])
        sizes = [c.numel() for c in clips]
        offsets = [0] + list(np.cumsum(sizes)[:-1])
        if src_dev.type == "cpu":
            buf = self._stage(clips, int(sum(sizes)), device)
        elif isinstance(frames, torch.Tensor) and frames.is_contiguous():
            buf = frames.view(-1)                            # the batch is already one buffer
        else:
            buf = torch.cat([c.reshape(-1) for c in clips])
        return self.ingest_buffer(buf, T, [(int(o), c.shape[1], c.shape[2]) for o, c in zip(offsets, clips)], boxes)


class IngestLoader:
    """Wraps any loader whose field 0 is uint8 frames ([B, T, H0, W0, 3] or a list of [T, H0_b, W0_b, 3]) and yields the same batches with field 0 replaced by the
    device clip; every other field passes through untouched.  The engines are not edited: their `.to(device)` on a tensor that is already there is a no-op.
    mode "train": boxes and flips drawn per clip, in batch order (ClipIngest.draw); "center": the validation CenterCrop; "test": the view's window, with split_nb read
    from field 4 of the batch, where the reference's test dataset puts it (buffer, label, name, chunk_nb, split_nb), and num_crop views per video.
    randaug (mode "train" only): a devias_amd.randaug.RandAugment.  The draws are then made clip by clip in the reference's order (_aug_frame): the clip's RandAugment
    plan, then its box and flip.  The frames are staged once, into the lower half of a double-sized buffer; the layers run in that buffer and the ingest reads the
    clips where the last layer left them.  Without it the draws and the path are what they were."""

    def __init__(self, data_loader, ingest: ClipIngest, mode: str = "train", num_crop: int = 3, randaug=None):
        if mode not in ("train", "center", "test"):
            raise ValueError(f"IngestLoader: mode {mode!r}")
        if randaug is not None and mode != "train":
            raise ValueError(f"IngestLoader: RandAugment belongs to training; mode {mode!r} takes no randaug")
        self.data_loader, self.ingest, self.mode, self.num_crop, self.randaug = data_loader, ingest, mode, int(num_crop), randaug

    def __len__(self):
        return len(self.data_loader)

    def __getattr__(self, name):              # dataset, sampler, batch_size, ...: the wrapped loader's
        return getattr(self.__dict__["data_loader"], name)

    def _boxes(self, batch, frames):
        sizes = [(c.shape[1], c.shape[2]) for c in frames] if isinstance(frames, (list, tuple)) else [(frames.shape[2], frames.shape[3])] * frames.shape[0]
        if self.mode == "train":
            return [self.ingest.draw(H0, W0) for H0, W0 in sizes]
        if self.mode == "center":
            return [self.ingest.center_box(H0, W0) for H0, W0 in sizes]
        split = batch[4]
        split = split.tolist() if isinstance(split, torch.Tensor) else list(split)
        return [self.ingest.test_box(H0, W0, int(s), self.num_crop) for (H0, W0), s in zip(sizes, split)]

    def _augmented(self, frames) -> torch.Tensor:
        """RandAugment, then the ingest: plan and box drawn per clip, in that order"""
        ra, m = self.randaug, self.ingest
        clips, T = check_clips(frames, "IngestLoader")
        plans, boxes = [], []
        for c in clips:
            plans.append(ra.draw())
            boxes.append(m.draw(c.shape[1], c.shape[2]))
        src_dev = clips[0].device
        device = src_dev if src_dev.type != "cpu" else m.device
        if device.type == "cpu":
            from .randaug import randaug_cpu
            return m([randaug_cpu(c, p, ra.resample) for c, p in zip(clips, plans)], boxes)
        sizes = [c.numel() for c in clips]
        offsets = [0] + [int(v) for v in np.cumsum(sizes)[:-1]]
        nbytes, half = int(sum(sizes)), ra.half_of(sum(sizes))
        if src_dev.type == "cpu":
            buf = m._stage(clips, nbytes, device, alloc=2 * half)
        else:                                                # device frames are the caller's: the layers run on a copy
            buf = torch.empty(2 * half, dtype=torch.uint8, device=device)
            for c, o, n in zip(clips, offsets, sizes):
                buf[o:o + n].view(c.shape).copy_(c)
        buf, layout = ra.augment_buffer(buf, T, [(o, c.shape[1], c.shape[2]) for o, c in zip(offsets, clips)], plans)
        return m.ingest_buffer(buf, T, layout, boxes)

    def __iter__(self):
        for batch in self.data_loader:
            if not isinstance(batch, (list, tuple)):
                raise TypeError(f"IngestLoader: a batch is a list or tuple whose field 0 holds the uint8 frames, got {type(batch).__name__}")
            clip = self._augmented(batch[0]) if self.randaug is not None else self.ingest(batch[0], self._boxes(batch, batch[0]))
            yield type(batch)([clip] + list(batch[1:]))
