"""Step semantics of engine/engine_for_slot_hvu.py for the MI355X path: every batch carries action AND scene labels, so there is no scene
teacher.  train_class_batch (:12-15), a lean train_one_epoch (:23-153) without per-step host syncs, and the three validation loops
(:156-280) with their sums kept on the device.  Unlike the reference's loops (`scene_targets += HVU_NUM_ACTION_CLASSES`, :176, :220, :261)
nothing here writes into the caller's target tensors."""
from __future__ import annotations

from typing import Iterable, Optional

import torch

from .engine_for_slot import _batch_metrics, _evaluate, _run_steps


def train_class_batch(model, samples, action_targets, scene_targets, train_criterion, fg_mask=None):
    """engine/engine_for_slot_hvu.py:12-15"""
    student_output = model(samples)
    total_loss, output, loss_dict = train_criterion(student_output, action_targets, scene_targets, fg_mask=fg_mask)
    return total_loss, output, loss_dict


def train_one_epoch(model, train_criterion, data_loader: Iterable, optimizer, device, epoch: int,
                    max_norm: float = 0, start_steps: int = 0, lr_schedule_values=None, wd_schedule_values=None,
                    num_training_steps_per_epoch: Optional[int] = None, update_freq: int = 1, mask_model=None,
                    grad_sync=None, check_finite_every: int = 50, log_every: int = 100, model_ema=None):
    """engine/engine_for_slot_hvu.py:23-153 restated for this stack, with the keyword surface of engine_for_slot.train_one_epoch: batches are
    (samples, action_targets, scene_targets, ...) (:43); LR/WD schedule poke (:49-54), H2D (:56-58), mask model (:64-65; without one the
    masks are batch[3]), train_class_batch; backward, optional gradient all-reduce and optimizer step are engine_for_slot._run_steps.
    The per-step `loss.item()` finite check (:79-83) and `torch.cuda.synchronize()` (:110) are replaced by one host check every
    `check_finite_every` steps."""
    model.train(True)

    def step(batch):
        samples, action_targets, scene_targets = (t.to(device, non_blocking=True) for t in batch[:3])
        if mask_model is not None:
            samples, action_targets, scene_targets, masks = mask_model(samples, action_targets, scene_targets)
        else:
            masks = tuple(m.to(device, non_blocking=True) for m in batch[3])
        loss, _output, loss_dict = train_class_batch(model, samples, action_targets, scene_targets, train_criterion, fg_mask=masks)
        return loss, loss_dict

    return _run_steps(step, data_loader, model, optimizer, max_norm, start_steps, lr_schedule_values, wd_schedule_values, num_training_steps_per_epoch,
                      update_freq, grad_sync, check_finite_every, model_ema)


def _validate(data_loader, model, device, action: bool, scene: bool, topk=(1, 5)):
    """One pass over the loader.  The loss is the cross-entropy of the action-selected slot's [B, nb + ns] logits against the action target in
    all three loops (:181, :225, :266); scene accuracy is taken on the scene-selected slot's full logits against scene_target + nb
    (:176, :184).  [n, sum of CE, action hits@k..., scene hits@k...] stay on the device; one host read at the end of the loader (_evaluate)."""
    nb = int(model.num_classes)
    names = ["%s_acc%d" % (what, k) for what, on in (("action", action), ("scene", scene)) if on for k in topk]

    def per_batch(out, fields, _batch):
        _, (action_output, scene_output, _attn), _ = out
        m = _batch_metrics(action_output.float(), fields[1], topk)
        parts = [m if action else m[:2]]
        if scene:
            parts.append(_batch_metrics(scene_output.float(), fields[2] + nb, topk)[2:])            # + nb: a new tensor, the loader's labels stay as they are
        return torch.cat(parts)

    return _evaluate(data_loader, model, device, 3, names, per_batch)


@torch.no_grad()
def validation_one_epoch(data_loader, model, device):
    """engine/engine_for_slot_hvu.py:156-200 -> {'loss', 'action_acc1', 'action_acc5', 'scene_acc1', 'scene_acc5'} (sample-weighted means, acc in percent)"""
    return _validate(data_loader, model, device, action=True, scene=True)


@torch.no_grad()
def validation_action(data_loader, model, device, header="Val:"):
    """engine/engine_for_slot_hvu.py:203-239 -> {'loss', 'action_acc1', 'action_acc5'}"""
    return _validate(data_loader, model, device, action=True, scene=False)


@torch.no_grad()
def validation_scene(data_loader, model, device, header="Val:"):
    """engine/engine_for_slot_hvu.py:243-280 -> {'loss', 'scene_acc1', 'scene_acc5'}"""
    return _validate(data_loader, model, device, action=False, scene=True)
