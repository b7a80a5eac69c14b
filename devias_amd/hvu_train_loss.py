"""TrainLoss of the HVU recipe with the reference's interface (utils/loss/hvu_train_loss.py:8-130): every clip carries a ground-truth
scene label, so there is no scene teacher.  Computed by ONE fused HIP launch (devias_head_match_loss_labels_fwd) instead of B host-side
SciPy assignments and five .item() syncs (:60, :124-128).  A Kinetics host that cached the teacher's argmax offline can use it the same way."""
from __future__ import annotations

import torch
import torch.nn as nn

from .train_loss import LOSS_NAMES, _matching_loss  # noqa: F401   (LOSS_NAMES: part of this module's surface)

HVU_NUM_ACTION_CLASSES = 739          # run_slot_finetuning_hvu.py:35-36
HVU_NUM_SCENE_CLASSES = 248


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
        slots_head = student_output[2][0]
        if slots_head.shape[1] != self.num_action_classes + self.num_scene_classes:
            raise ValueError(f"head width {slots_head.shape[1]} != num_action_classes {self.num_action_classes} + num_scene_classes {self.num_scene_classes}")
        scene_target = scene_targets.to(device=slots_head.device, dtype=torch.int64).contiguous()       # read only: never offset in place
        return _matching_loss(self, student_output, scene_target, action_targets, fg_mask, 0.0)       # no scene weight in this recipe
