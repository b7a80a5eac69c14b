"""TrainLoss of the HVU recipe with the reference's interface (utils/loss/hvu_train_loss.py:8-130): every clip carries a ground-truth
scene label, so there is no scene teacher.  Computed by ONE fused HIP launch (devias_head_match_loss_labels_fwd) instead of B host-side
SciPy assignments and five .item() syncs (:60, :124-128).  A Kinetics host that cached the teacher's argmax offline can use it the same way."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd import Function

from . import ops
from .train_loss import LOSS_NAMES

HVU_NUM_ACTION_CLASSES = 739          # run_slot_finetuning_hvu.py:35-36
HVU_NUM_SCENE_CLASSES = 248


class HeadMatchLossLabelsFn(Function):
    @staticmethod
    def forward(ctx, slots_head, slots, maskp, attn, target, scene_target, fg, fgN, nb, w_mp, w_md, scene_ce=False):
        slots_head, slots, maskp, attn = (t.contiguous() for t in (slots_head, slots, maskp, attn))
        losses, match, logits = ops.head_match_loss_labels_fwd(slots_head, slots, maskp, attn, target, scene_target, fg, fgN, nb, w_mp, w_md, scene_ce)
        ctx.saved = (slots_head, slots, maskp, attn, target, scene_target, fg, fgN, match)
        ctx.w = (nb, w_mp, w_md, scene_ce)
        ctx.mark_non_differentiable(losses, match, logits)
        total = losses[5:6].clone()
        return total, losses, match, logits

    @staticmethod
    def backward(ctx, g_total, *_):
        slots_head, slots, maskp, attn, target, scene_target, fg, fgN, match = ctx.saved
        nb, w_mp, w_md, scene_ce = ctx.w
        g = g_total.reshape(1).float().contiguous()
        dZ, dslots, dmask, dattn = ops.head_match_loss_labels_bwd(slots_head, slots, maskp, attn, target, scene_target, fg, fgN, match, g,
                                                                  nb, w_mp, w_md, scene_ce)
        return dZ, dslots, dmask, dattn, None, None, None, None, None, None, None, None


class TrainLoss(nn.Module):
    """Drop-in for utils.loss.hvu_train_loss.TrainLoss ('matching'; scene_criterion 'KL' or 'CE', which are the same number against a
    one-hot target: hvu_train_loss.py:94 and :96-101).  There is no scene_loss_weight in this class (as in the reference).

    forward(student_output, action_targets, scene_targets, fg_mask) -> (total_loss[1], action_logit[B,C], loss_dict)
    `scene_targets` are class indices in [0, num_scene_classes).  The one deliberate difference from the reference: they are NOT mutated.
    The reference adds num_action_classes to the caller's tensor in place (`scene_target += self.num_action_classes`, hvu_train_loss.py:45-46),
    so calling it twice on one tensor shifts the labels twice; here the offset is applied inside the kernel.
    The reference imports the two class counts from its driver (:6, :17-18); here they are constructor arguments with those values as defaults.
    A label outside its range gives a NaN total (and zero gradients for that sample): the engine's finite check stops the run.
    `loss_dict` holds Python floats like the reference, which costs ONE device->host copy of 6 floats; pass sync_loss_dict=False to get 0-d
    device tensors instead (no host sync at all).  `last_match` is the int32 [B, 2] (action slot, scene slot) assignment of the last call."""

    def __init__(self, criterion=None, scene_criterion="KL", slot_matching_method="matching", mask_prediction_loss_weight=1.0,
                 mask_distill_loss_weight=1.0, num_action_classes: int = HVU_NUM_ACTION_CLASSES, num_scene_classes: int = HVU_NUM_SCENE_CLASSES,
                 sync_loss_dict=True):
        super().__init__()
        if slot_matching_method != "matching":
            raise NotImplementedError("only the 'matching' branch exists (hvu_train_loss.py:28-29, 129-130)")
        if scene_criterion not in ("KL", "CE"):                 # the reference silently adds no scene term for anything else (:93-101)
            raise ValueError(f"scene_criterion must be 'KL' or 'CE', got {scene_criterion!r}")
        self.criterion = criterion            # accepted, never used in the matching branch (as in the reference)
        self.scene_criterion = scene_criterion
        self.num_action_classes = int(num_action_classes)
        self.num_scene_classes = int(num_scene_classes)
        self.slot_matching_method = slot_matching_method
        self.mask_prediction_loss_weight = float(mask_prediction_loss_weight)
        self.mask_distill_loss_weight = float(mask_distill_loss_weight)
        self.sync_loss_dict = sync_loss_dict
        self.last_match = None

    def forward(self, student_output, action_targets, scene_targets, fg_mask=None):
        _, (_, _, attn), (slots_head, slots, mask_predictions) = student_output
        if slots_head.shape[1] != self.num_action_classes + self.num_scene_classes:
            raise ValueError(f"head width {slots_head.shape[1]} != num_action_classes {self.num_action_classes} + num_scene_classes {self.num_scene_classes}")
        fg, fgN = fg_mask
        dev = slots_head.device
        fg = fg.to(device=dev, dtype=torch.float32).contiguous()       # k/256 masks: the reference's .half() is value-preserving
        fgN = fgN.to(device=dev, dtype=torch.float32).contiguous()
        target = action_targets.to(device=dev, dtype=torch.int64).contiguous()
        scene_target = scene_targets.to(device=dev, dtype=torch.int64).contiguous()       # read only: never offset in place
        total, losses, match, logits = HeadMatchLossLabelsFn.apply(
            slots_head, slots, mask_predictions, attn, target, scene_target, fg, fgN, self.num_action_classes,
            self.mask_prediction_loss_weight, self.mask_distill_loss_weight, self.scene_criterion == "CE")
        self.last_match = match
        if self.sync_loss_dict:
            vals = losses.tolist()
            loss_dict = {k: vals[i] for i, k in enumerate(LOSS_NAMES)}
        else:
            loss_dict = {k: losses[i] for i, k in enumerate(LOSS_NAMES)}
        return total, logits, loss_dict
