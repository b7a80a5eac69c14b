"""Step semantics of engine/engine_for_finetuning_scene.py, the engine that trains the scene teacher behind --scene_model_path (run_class_finetuning.py): the plain
(model, criterion) engine with every step's target replaced by the argmax of a frozen scene model's logits, on the shared step loop and evaluation pass of
engine_for_slot: train_class_batch (:13-16), train_one_epoch (:24-146), validation_one_epoch (:150-188), final_test (:192-243), merge (:246-286).

The target never leaves the device: `scene_model(samples)[1].argmax(1)` under torch.no_grad() feeds the criterion directly (the reference moves it `.to(device)`,
a no-op there too), so a step has no host sync beyond the shared loop's check of the loss every `check_finite_every` micro-batches."""
from __future__ import annotations

from typing import Iterable, Optional

import torch

from . import engine_for_slot as _es
from .engine_for_finetuning import train_class_batch  # noqa: F401  (:13-16, the same function in both reference engines)


@torch.no_grad()
def scene_targets(scene_model, samples):
    """engine/engine_for_finetuning_scene.py:59-63: int64 [B], the frozen scene model's top class per clip"""
    _, teacher_scene_logit = scene_model(samples, return_attn=False)
    return torch.argmax(teacher_scene_logit.float(), dim=1)


def train_one_epoch(model, scene_model, criterion, data_loader: Iterable, optimizer, device, epoch: int, loss_scaler=None, max_norm: float = 0, model_ema=None,
                    mixup_fn=None, log_writer=None, start_steps: int = 0, lr_schedule_values=None, wd_schedule_values=None,
                    num_training_steps_per_epoch: Optional[int] = None, update_freq: int = 1, grad_sync=None, check_finite_every: int = 50):
    """engine/engine_for_finetuning_scene.py:24-146 on engine_for_slot._run_steps.  The batch's own targets are ignored (:59-63 overwrite them).  `loss_scaler` and
    `log_writer` are accepted and unused (bf16 / fp32 need no loss scale).  `mixup_fn`: None or a devias_amd.mixup.Mixup."""
    mixup_fn = _es._device_mixup(mixup_fn)
    model.train(True)
    scene_model.eval()

    def step(batch):
        samples = batch[0].to(device, non_blocking=True)
        targets = scene_targets(scene_model, samples)
        if mixup_fn is not None:                                  # (:65-66) AFTER the teacher's argmax on the unmixed clip
            samples, targets = mixup_fn(samples, targets)
        loss, _output = train_class_batch(model, samples, targets, criterion)
        return loss, {}

    return _es._run_steps(step, data_loader, model, optimizer, max_norm, start_steps or 0, lr_schedule_values, wd_schedule_values, num_training_steps_per_epoch,
                          update_freq or 1, grad_sync, check_finite_every, model_ema)


@torch.no_grad()
def validation_one_epoch(data_loader, model, scene_model, device, topk=(1, 5)):
    """engine/engine_for_finetuning_scene.py:150-188 -> {'loss', 'acc1', 'acc5'} against the scene model's argmax, sample-weighted means (acc in percent)"""
    scene_model.eval()
    return _es._evaluate(data_loader, model, device, 1, ["acc%d" % k for k in topk],
                         lambda out, f, _: _es._batch_metrics(out[1].float(), scene_targets(scene_model, f[0]), topk))


@torch.no_grad()
def final_test(data_loader, model, scene_model, device, file):
    """engine/engine_for_finetuning_scene.py:192-243: one line `id [logits] target chunk split` per sample (the target is the scene model's argmax) after a first
    line with the LAST batch's `acc1, acc5`: the slot engine's line format, not the plain engine's `output : ` markers"""
    scene_model.eval()
    lines = ["0.0, 0.0\n"]

    def per_batch(out, fields, batch):
        output, target = out[1].float(), scene_targets(scene_model, fields[0])
        m = _es._batch_metrics(output, target, (1, 5))
        rows, tgt, mh = output.cpu().numpy(), target.cpu().numpy(), m.cpu().numpy()
        lines[0] = "{}, {}\n".format(100.0 * mh[2] / mh[0], 100.0 * mh[3] / mh[0])
        for i, (sample_id, chunk_nb, split_nb) in enumerate(zip(*batch[2:5])):
            lines.append("{} {} {} {} {}\n".format(sample_id, str(rows[i].tolist()), str(int(tgt[i])), str(int(chunk_nb)), str(int(split_nb))))
        return m

    stats = _es._evaluate(data_loader, model, device, 1, ["acc1", "acc5"], per_batch)
    with open(file, "w") as f:
        f.writelines(lines)
    return stats


merge = _es.merge          # engine/engine_for_finetuning_scene.py:246-286 reads the slot engine's line format: the same vote
