"""Classification losses of the downstream recipe (run_slot_downstream.py: timm's LabelSmoothingCrossEntropy, or nn.CrossEntropyLoss with smoothing 0) over the
label-smoothing cross-entropy kernels (devias_softmax_ce_fwd / _bwd, csrc/fusion_head.hip).  Hard int64 targets only: the recipe runs with mixup and cutmix at 0."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd import Function

from . import ops


class SoftmaxCEFn(Function):
    """logits [B, C] (fp32 or bf16), int64 target [B] -> fp32 loss [1]; the upstream gradient stays on the device (loss / update_freq costs no sync)"""

    @staticmethod
    def forward(ctx, logits, target, smoothing):
        logits = logits.contiguous()
        ctx.saved = (logits, target)
        ctx.smoothing = smoothing
        return ops.softmax_ce_fwd(logits, target, smoothing)

    @staticmethod
    def backward(ctx, g):
        logits, target = ctx.saved
        return ops.softmax_ce_bwd(logits, target, g.reshape(1).float().contiguous(), ctx.smoothing), None, None


class LabelSmoothingCrossEntropy(nn.Module):
    """timm.loss.LabelSmoothingCrossEntropy(smoothing): mean_b[(1 - e)(lse_b - z[b, y_b]) + e (lse_b - mean_c z[b, c])].  A target outside [0, C) makes the loss NaN
    (the engine stops on a non-finite loss); it is never used as an index."""

    def __init__(self, smoothing: float = 0.1):
        super().__init__()
        if not 0.0 <= float(smoothing) < 1.0:
            raise ValueError(f"smoothing must be in [0, 1), got {smoothing}")
        self.smoothing = float(smoothing)
        self.confidence = 1.0 - self.smoothing

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if target.dtype != torch.int64 or target.dim() != 1:
            raise NotImplementedError("soft targets (mixup / cutmix) are not part of the downstream recipe: int64 class indices [B] expected")
        target = target.to(device=x.device).contiguous()
        return SoftmaxCEFn.apply(x, target, self.smoothing)[0]


class CrossEntropyLoss(LabelSmoothingCrossEntropy):
    """torch.nn.CrossEntropyLoss() with its defaults (mean reduction, hard targets): smoothing 0"""

    def __init__(self):
        super().__init__(0.0)
