"""Step semantics of engine/engine_for_slot_hvu.py for the MI355X path: every batch carries action AND scene labels, so there is no scene
teacher.  train_class_batch (:12-15), a lean train_one_epoch (:23-153) without per-step host syncs, and the three validation loops
(:156-280) with their sums kept on the device.  Unlike the reference's loops (`scene_targets += HVU_NUM_ACTION_CLASSES`, :176, :220, :261)
nothing here writes into the caller's target tensors."""
from __future__ import annotations

import math
import sys
from typing import Iterable, Optional

import torch

from .engine_for_slot import _batch_metrics
from .optim import FusedAdamW


def train_class_batch(model, samples, action_targets, scene_targets, train_criterion, fg_mask=None):
    """engine/engine_for_slot_hvu.py:12-15"""
    student_output = model(samples)
    total_loss, output, loss_dict = train_criterion(student_output, action_targets, scene_targets, fg_mask=fg_mask)
    return total_loss, output, loss_dict


def train_one_epoch(model, train_criterion, data_loader: Iterable, optimizer, device, epoch: int,
                    max_norm: float = 0, start_steps: int = 0, lr_schedule_values=None, wd_schedule_values=None,
                    num_training_steps_per_epoch: Optional[int] = None, update_freq: int = 1, mask_model=None,
                    grad_sync=None, check_finite_every: int = 50, log_every: int = 100):
    """engine/engine_for_slot_hvu.py:23-153 restated for this stack, with the keyword surface of engine_for_slot.train_one_epoch: batches are
    (samples, action_targets, scene_targets, ...) (:43); LR/WD schedule poke (:49-54), H2D (:56-58), mask model (:64-65; without one the
    masks are batch[3]), train_class_batch, backward, optional gradient all-reduce (`grad_sync`, devias_amd.parallel), optimizer step.
    The per-step `loss.item()` finite check (:79-83) and `torch.cuda.synchronize()` (:110) are replaced by one host check every
    `check_finite_every` steps."""
    model.train(True)
    optimizer.zero_grad(set_to_none=True)
    stats = {}
    n_steps = 0
    grad_norm = None
    for data_iter_step, batch in enumerate(data_loader):
        samples, action_targets, scene_targets = batch[0], batch[1], batch[2]
        step = data_iter_step // update_freq
        if num_training_steps_per_epoch is not None and step >= num_training_steps_per_epoch:
            continue
        it = start_steps + step
        if (lr_schedule_values is not None or wd_schedule_values is not None) and data_iter_step % update_freq == 0:
            for group in optimizer.param_groups:
                if lr_schedule_values is not None:
                    group["lr"] = lr_schedule_values[it] * group.get("lr_scale", 1.0)
                if wd_schedule_values is not None and group["weight_decay"] > 0:
                    group["weight_decay"] = wd_schedule_values[it]
        samples = samples.to(device, non_blocking=True)
        action_targets = action_targets.to(device, non_blocking=True)
        scene_targets = scene_targets.to(device, non_blocking=True)
        if mask_model is not None:
            samples, action_targets, scene_targets, masks = mask_model(samples, action_targets, scene_targets)
        else:
            masks = tuple(m.to(device, non_blocking=True) for m in batch[3])
        loss, output, loss_dict = train_class_batch(model, samples, action_targets, scene_targets, train_criterion, fg_mask=masks)
        if update_freq > 1:
            loss = loss / update_freq
        if grad_sync is not None:
            # gradient accumulation: only the LAST micro-batch of a window starts the bucket all-reduces (earlier ones just accumulate)
            grad_sync.set_accumulate((data_iter_step + 1) % update_freq != 0)
        loss.backward()
        if (data_iter_step + 1) % update_freq == 0:
            if grad_sync is not None:
                grad_sync.finish()
            if isinstance(optimizer, FusedAdamW) and optimizer.multi_tensor:
                # gradient norm + clip_grad_norm_ (utils/utils.py:388-394) fused into the update; the norm stays on the device
                optimizer.step(max_norm=float(max_norm or 0.0))
                grad_norm = optimizer.last_grad_norm
            else:
                if max_norm and max_norm > 0:
                    grad_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
                optimizer.step()
            optimizer.zero_grad(set_to_none=True)
        n_steps += 1
        if check_finite_every and n_steps % check_finite_every == 0:
            loss_value = float(loss.detach().float().sum())
            if not math.isfinite(loss_value):
                print("Loss is {}, stopping training".format(loss_value))
                sys.exit(1)
            stats["loss"] = loss_value
            if grad_norm is not None:
                stats["grad_norm"] = float(grad_norm)
            stats["lr"] = max(g["lr"] for g in optimizer.param_groups)
            stats["min_lr"] = min(g["lr"] for g in optimizer.param_groups)
            stats.update({k: float(v) for k, v in loss_dict.items()})
    return stats


def _validate(data_loader, model, device, action: bool, scene: bool, topk=(1, 5)):
    """One pass over the loader.  The loss is the cross-entropy of the action-selected slot's [B, nb + ns] logits against the action target in
    all three loops (:181, :225, :266); scene accuracy is taken on the scene-selected slot's full logits against scene_target + nb
    (:176, :184).  [n, sum of CE, action hits@k..., scene hits@k...] stay on the device; one host read at the end of the loader."""
    model.eval()
    nb = int(model.num_classes)
    K = len(topk)
    acc = torch.zeros(2 + 2 * K, dtype=torch.float64, device=device)
    for batch in data_loader:
        videos = batch[0].to(device, non_blocking=True)
        action_targets = batch[1].to(device, non_blocking=True)
        scene_targets = batch[2].to(device, non_blocking=True) + nb            # a new tensor: the loader's labels stay as they are
        _, (action_output, scene_output, _attn), _ = model(videos)
        m = _batch_metrics(action_output.float(), action_targets, topk)
        acc[:2 + K] += m
        if scene:
            acc[2 + K:] += _batch_metrics(scene_output.float(), scene_targets, topk)[2:]
    vals = acc.tolist()
    n = max(vals[0], 1.0)
    out = {"loss": vals[1] / n}
    if action:
        out.update({"action_acc%d" % k: 100.0 * vals[2 + i] / n for i, k in enumerate(topk)})
    if scene:
        out.update({"scene_acc%d" % k: 100.0 * vals[2 + K + i] / n for i, k in enumerate(topk)})
    return out


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
