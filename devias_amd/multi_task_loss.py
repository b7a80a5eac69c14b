"""TrainLoss of the two-token multi-task baseline with the reference's interface (run_multi_task_finetuning.py:31-78): the action term is the given criterion
(devias_amd.losses.LabelSmoothingCrossEntropy / CrossEntropyLoss, unchanged), the scene term distils the frozen teacher's logits into the scene head through
devias_distill_fwd / _bwd (csrc/distill.hip).  With the unified head the teacher row is read as num_action_classes columns of (the whole teacher tensor's
minimum - 1) followed by its logits (:48-52) -- those pad columns carry softmax mass in the KL, as in the reference -- without the padded tensor ever existing."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib, ops

LOSS_NAMES = ("action_loss", "logit_loss")


class DistillFn(Function):
    """student logits [B, C] (fp32 or bf16), fp32 teacher logits [B, Ct <= C] -> fp32 loss [1]; the upstream gradient stays on the device"""

    @staticmethod
    def forward(ctx, student, teacher, mode, weight):
        student = student.contiguous()
        loss, tmin = ops.distill_fwd(student, teacher, mode, weight)
        ctx.saved = (student, teacher, tmin)
        ctx.mode, ctx.weight = mode, weight
        return loss

    @staticmethod
    def backward(ctx, g):
        student, teacher, tmin = ctx.saved
        return ops.distill_bwd(student, teacher, tmin, g.reshape(1).float().contiguous(), ctx.mode, ctx.weight), None, None, None


class TrainLoss(nn.Module):
    """Drop-in for the driver's TrainLoss.

    forward(student_output, teacher_outputs, target) -> (total_loss[1], action_logit[B, C], loss_dict)
    `loss_dict` holds Python floats like the reference ('action_loss', 'logit_loss'), which costs ONE device->host copy of 2 floats; pass sync_loss_dict=False to
    get 0-d device tensors instead (no host sync at all).  'KL' is multiplied by logit_criterion_weight; 'CE' (cross-entropy against the teacher's argmax, first
    index on ties) is not -- the reference applies the weight in the KL branch only (:58-68)."""

    def __init__(self, criterion, logit_criterion, unified_head=False, num_action_classes=400, logit_criterion_weight=1.0, sync_loss_dict=True):
        super().__init__()
        if logit_criterion not in ("KL", "CE"):                 # the reference raises NotImplementedError inside forward (:70-71)
            raise NotImplementedError(f"logit_criterion must be 'KL' or 'CE' (run_multi_task_finetuning.py:93), got {logit_criterion!r}")
        self.criterion = criterion
        self.logit_criterion = logit_criterion
        self.logit_criterion_weight = float(logit_criterion_weight)
        self.unified_head = bool(unified_head)
        self.num_action_classes = int(num_action_classes)
        self.sync_loss_dict = sync_loss_dict

    def forward(self, student_output, teacher_outputs, target):
        (_, action_logit), (_, scene_logit) = student_output
        _, teacher_scene_logit = teacher_outputs
        teacher = teacher_scene_logit.detach().to(device=scene_logit.device, dtype=torch.float32).contiguous()
        pad = self.num_action_classes if self.unified_head else 0
        if scene_logit.dim() != 2 or teacher.dim() != 2 or scene_logit.shape != (teacher.shape[0], pad + teacher.shape[1]):
            raise ValueError(f"scene logits {tuple(scene_logit.shape)} do not match teacher logits {tuple(teacher.shape)} left-padded by {pad} columns")
        action_loss = self.criterion(action_logit, target).reshape(1)
        mode = _lib.DISTILL_CE if self.logit_criterion == "CE" else _lib.DISTILL_KL
        logit_loss = DistillFn.apply(scene_logit, teacher, mode, self.logit_criterion_weight)
        total = action_loss.float() + logit_loss
        parts = torch.cat([action_loss.detach().float(), logit_loss.detach()])
        vals = parts.tolist() if self.sync_loss_dict else parts
        return total, action_logit, {k: vals[i] for i, k in enumerate(LOSS_NAMES)}
