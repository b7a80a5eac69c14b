"""utils/transform/mixup.py's Mixup on the device: the reference's draws from numpy's global random state, in its order, on the host; the clip batch mixed in place by
ONE kernel launch (devias_mixup_clips) and the dense soft target written by one more (devias_mixup_target).

Every mode of the reference pairs clip i with clip B-1-i at the same pixel, so the draw ends in one table of B rows (kind, weights, box); the rows reach the device as
kernel arguments: no copy, no host sync, nothing for the next step's table to race with.  FastCollateMixup (collate-time, uint8, CPU) is not built."""
from __future__ import annotations

from typing import List, NamedTuple

import numpy as np
import torch

from . import _lib, ops

NONE, MIXUP, CUTMIX = _lib.MIX_NONE, _lib.MIX_MIXUP, _lib.MIX_CUTMIX


def _box_around_centre(H, W, lam):
    """the CutMix box of mixup.py's rand_bbox at margin 0: sides int(H sqrt(1 - lam)), int(W sqrt(1 - lam)) around a centre drawn uniformly over the plane (row first,
    then column), clipped to the plane"""
    side = np.sqrt(1 - lam)
    bh, bw = int(H * side), int(W * side)
    cy = np.random.randint(0, H)
    cx = np.random.randint(0, W)
    return np.clip(cy - bh // 2, 0, H), np.clip(cy + bh // 2, 0, H), np.clip(cx - bw // 2, 0, W), np.clip(cx + bw // 2, 0, W)


def _box_from_ratios(H, W, lo, hi):
    """the box of mixup.py's rand_bbox_minmax: height, then width, drawn between the two ratios of the plane's sides; then the top row, then the left column"""
    bh = np.random.randint(int(H * lo), int(H * hi))
    bw = np.random.randint(int(W * lo), int(W * hi))
    top = np.random.randint(0, H - bh)
    left = np.random.randint(0, W - bw)
    return top, top + bh, left, left + bw


def cutmix_bbox_and_lam(img_shape, lam, ratio_minmax=None, correct_lam=True):
    """mixup.py:77-87: the box (yl, yh, xl, xh) for a plane img_shape[-2:] and the lambda, corrected to the area the clipped box kept"""
    H, W = int(img_shape[-2]), int(img_shape[-1])
    if ratio_minmax is not None:
        assert len(ratio_minmax) == 2
        box = _box_from_ratios(H, W, ratio_minmax[0], ratio_minmax[1])
    else:
        box = _box_around_centre(H, W, lam)
    if correct_lam or ratio_minmax is not None:
        lam = 1. - (box[1] - box[0]) * (box[3] - box[2]) / float(H * W)
    return box, lam


class MixRow(NamedTuple):
    """one clip's row of the table: MIXUP reads w_self / w_other, CUTMIX reads the box"""
    kind: int = NONE
    w_self: float = 1.0
    w_other: float = 0.0
    yl: int = 0
    yh: int = 0
    xl: int = 0
    xh: int = 0


class MixTable(NamedTuple):
    """What one draw decided.  rows: per clip, what devias_mixup_clips does.  lam: what the reference's `lam` is when it reaches mixup_target -- a Python float in
    'batch' mode, a float32 array [B] in 'elem' / 'pair' mode (the corrected cutmix value where a box was drawn, 1 for an unmixed clip)."""
    rows: List[MixRow]
    lam: object


def mixup_target(target, num_classes, lam=1., smoothing=0.0, device=None):
    """mixup.py:22-27: y1 * lam + y2 * (1. - lam) over smoothed one-hot rows of `target` and of its flip -> fp32 [B, C], one launch.  `lam`: a Python / numpy scalar
    (rounded to fp32 as ATen rounds a scalar operand, 1. - lam taken in double first), or a tensor / array of B values whose dtype is kept: 1. - lam is taken in that
    dtype, as the reference's `1. - lam` on its lam tensor is."""
    target = target.to(device=device if device is not None else target.device, dtype=torch.int64).contiguous().view(-1)
    B = target.shape[0]
    off_value = smoothing / num_classes
    on_value = 1. - smoothing + off_value
    if isinstance(lam, np.ndarray):
        lam = torch.from_numpy(np.ascontiguousarray(lam))
    if isinstance(lam, torch.Tensor):
        lam = lam.detach().to("cpu").reshape(-1)
        if lam.numel() != B:
            raise ValueError(f"mixup_target: {lam.numel()} lam values for {B} targets")
        w_self, w_other = lam.float().tolist(), (1. - lam).float().tolist()
    else:
        w_self, w_other = [float(np.float32(lam))] * B, [float(np.float32(1. - lam))] * B
    return ops.mixup_target(target, num_classes, np.float32(on_value), np.float32(off_value), w_self, w_other)


class Mixup:
    """utils/transform/mixup.py:90-218 with its arguments and attributes.  `__call__(x, target)` mixes the device tensor x [B, ..., H, W] (fp32 or bf16, B even) in place
    and returns (x, fp32 soft target [B, num_classes]).  The random draws are the reference's, from numpy's global state in the reference's order: after
    np.random.seed(s) both produce the same parameters in every mode."""

    def __init__(self, mixup_alpha=1., cutmix_alpha=0., cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode='batch', correct_lam=True, label_smoothing=0.1,
                 num_classes=1000):
        self.mixup_alpha = mixup_alpha
        self.cutmix_alpha = cutmix_alpha
        self.cutmix_minmax = cutmix_minmax
        if self.cutmix_minmax is not None:
            assert len(self.cutmix_minmax) == 2
            self.cutmix_alpha = 1.0          # (:112) forced when minmax is active
        self.mix_prob = prob
        self.switch_prob = switch_prob
        self.label_smoothing = label_smoothing
        self.num_classes = num_classes
        self.mode = mode
        self.correct_lam = correct_lam
        self.mixup_enabled = True            # the training loop may switch mixing off

    # ---- the draws (host only) ---------------------------------------------------------------------------------------------------------------------
    def _params_per_elem(self, batch_size):
        """:121-139 -> (float32 lam [n], bool use_cutmix [n]).  Draw order: the switch, the cutmix betas, the mixup betas, then who is mixed at all."""
        lam = np.ones(batch_size, dtype=np.float32)
        use_cutmix = np.zeros(batch_size, dtype=bool)
        if not self.mixup_enabled:
            return lam, use_cutmix
        a_mix, a_cut = self.mixup_alpha, self.cutmix_alpha
        if a_mix > 0. and a_cut > 0.:
            use_cutmix = np.random.rand(batch_size) < self.switch_prob
            from_cut = np.random.beta(a_cut, a_cut, size=batch_size)
            from_mix = np.random.beta(a_mix, a_mix, size=batch_size)
            drawn = np.where(use_cutmix, from_cut, from_mix)
        elif a_mix > 0.:
            drawn = np.random.beta(a_mix, a_mix, size=batch_size)
        elif a_cut > 0.:
            use_cutmix = np.ones(batch_size, dtype=bool)
            drawn = np.random.beta(a_cut, a_cut, size=batch_size)
        else:
            raise AssertionError("one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax not None must hold")
        mixed = np.random.rand(batch_size) < self.mix_prob
        return np.where(mixed, drawn.astype(np.float32), lam), use_cutmix

    def _params_per_batch(self):
        """:141-157 -> (Python float lam, use_cutmix).  Draw order: whether to mix, the switch, one beta."""
        if not (self.mixup_enabled and np.random.rand() < self.mix_prob):
            return 1., False
        a_mix, a_cut = self.mixup_alpha, self.cutmix_alpha
        if a_mix > 0. and a_cut > 0.:
            use_cutmix = bool(np.random.rand() < self.switch_prob)
        elif a_mix > 0. or a_cut > 0.:
            use_cutmix = not a_mix > 0.
        else:
            raise AssertionError("one of mixup_alpha > 0, cutmix_alpha > 0, cutmix_minmax not None must hold")
        alpha = a_cut if use_cutmix else a_mix
        return float(np.random.beta(alpha, alpha)), use_cutmix

    def _row(self, shape, lam, use_cutmix, f32):
        """the row and the lam that the reference's loop body (:166-173) leaves for one clip whose drawn lam is not 1; `f32`: the 'elem' / 'pair' weights, float32
        arithmetic on numpy scalars, where 'batch' mode hands ATen Python doubles"""
        if use_cutmix:
            (yl, yh, xl, xh), lam = cutmix_bbox_and_lam(shape, lam, ratio_minmax=self.cutmix_minmax, correct_lam=self.correct_lam)
            return MixRow(CUTMIX, 1.0, 0.0, int(yl), int(yh), int(xl), int(xh)), lam
        if f32:
            return MixRow(MIXUP, float(np.float32(lam)), float(np.float32(1) - np.float32(lam))), lam
        return MixRow(MIXUP, float(np.float32(lam)), float(np.float32(1. - lam))), lam

    def draw(self, shape) -> MixTable:
        """Everything random about one call for a batch of `shape` [B, ..., H, W], drawn from numpy's global state as the reference's _mix_elem / _mix_pair /
        _mix_batch draw it.  Host only: needs no GPU."""
        B = int(shape[0])
        assert B % 2 == 0, 'Batch size should be even when using this'
        if self.mode in ('elem', 'pair'):
            n = B if self.mode == 'elem' else B // 2
            lam_batch, use_cutmix = self._params_per_elem(n)
            rows = [MixRow()] * B
            for i in range(n):
                if lam_batch[i] != 1.:
                    row, lam = self._row(tuple(shape[1:]), lam_batch[i], use_cutmix[i], True)
                    rows[i] = row
                    if row.kind == CUTMIX:
                        lam_batch[i] = lam
                    if self.mode == 'pair':
                        rows[B - 1 - i] = row
            if self.mode == 'pair':
                lam_batch = np.concatenate((lam_batch, lam_batch[::-1]))
            return MixTable(rows, lam_batch)
        lam, use_cutmix = self._params_per_batch()
        if lam == 1.:
            return MixTable([MixRow()] * B, 1.)
        row, lam = self._row(tuple(shape), lam, use_cutmix, False)
        return MixTable([row] * B, lam)

    # ---- the device side ---------------------------------------------------------------------------------------------------------------------------
    def apply(self, x: torch.Tensor, target: torch.Tensor, table: MixTable):
        """mix x in place by `table` and build the soft target (two launches; a table of NONE rows launches only the target)"""
        B = x.shape[0]
        if any(r.kind != NONE for r in table.rows):
            ctable = (_lib.MixupRow * B)(*[_lib.MixupRow(r.kind, r.w_self, r.w_other, r.yl, r.yh, r.xl, r.xh, 0) for r in table.rows])
            ops.mixup_clips(x, ctable)
        lam = table.lam
        if isinstance(lam, np.ndarray):
            lam = torch.tensor(lam, dtype=x.dtype)          # (:174) the clip's dtype: bf16 clips round lam, and 1. - lam, to bf16
        return x, mixup_target(target, self.num_classes, lam, self.label_smoothing, x.device)

    def __call__(self, x: torch.Tensor, target: torch.Tensor):
        assert len(x) % 2 == 0, 'Batch size should be even when using this'
        if not (isinstance(x, torch.Tensor) and x.is_cuda and isinstance(target, torch.Tensor) and target.is_cuda):
            raise RuntimeError("devias_amd.mixup.Mixup mixes device tensors (HIP kernels only; no CPU fallback)")
        return self.apply(x, target, self.draw(x.shape))
