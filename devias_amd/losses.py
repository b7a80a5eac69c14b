"""Classification losses of the downstream recipe (run_slot_downstream.py: timm's LabelSmoothingCrossEntropy, or nn.CrossEntropyLoss with smoothing 0) over the
label-smoothing cross-entropy kernels (devias_softmax_ce_fwd / _bwd, csrc/fusion_head.hip), which take hard int64 targets only, and timm's SoftTargetCrossEntropy, the
criterion the drivers switch to under mixup / cutmix (devias_amd.mixup.Mixup), over devias_soft_ce_fwd / _bwd (csrc/mixup.hip)."""
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


class SoftCEFn(Function):
    """logits [B, C] (fp32 or bf16), fp32 soft target [B, C] -> fp32 loss [1]; the upstream gradient stays on the device"""

    @staticmethod
    def forward(ctx, logits, target):
        logits = logits.contiguous()
        ctx.saved = (logits, target)
        return ops.soft_ce_fwd(logits, target)

    @staticmethod
    def backward(ctx, g):
        logits, target = ctx.saved
        return ops.soft_ce_bwd(logits, target, g.reshape(1).float().contiguous()), None


class SoftTargetCrossEntropy(nn.Module):
    """timm.loss.SoftTargetCrossEntropy(): mean_b sum_c -target[b, c] log_softmax(x)[b, c] against a dense fp32 target [B, C], as devias_amd.mixup.Mixup returns it.
    The rows need not sum to 1."""

    def forward(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if not target.is_floating_point() or target.shape != x.shape:
            raise ValueError(f"a dense soft target of the logits' shape {tuple(x.shape)} expected, got {target.dtype} {tuple(target.shape)}")
        target = target.to(device=x.device, dtype=torch.float32).contiguous()
        return SoftCEFn.apply(x, target).reshape(())          # (a view: its backward launches nothing, where indexing [0] scatters into zeros)


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
            raise NotImplementedError("int64 class indices [B] expected: a dense soft target (mixup / cutmix) goes to SoftTargetCrossEntropy")
        target = target.to(device=x.device).contiguous()
        return SoftmaxCEFn.apply(x, target, self.smoothing)[0]


class CrossEntropyLoss(LabelSmoothingCrossEntropy):
    """torch.nn.CrossEntropyLoss() with its defaults (mean reduction, hard targets): smoothing 0"""

    def __init__(self):
        super().__init__(0.0)
