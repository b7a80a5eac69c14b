"""Step semantics of engine/engine_for_multi_task.py, the engine of the two-token multi-task baseline (run_multi_task_finetuning.py), on the shared step loop and
evaluation pass of engine_for_slot: train_class_batch (:13-19), train_one_epoch (:27-149), validation_one_epoch (:152-185), final_test (:188-240),
final_test_with_scene_label (:243-304), merge (:307-347).

The model returns ((action_token, action_logits), (scene_token, scene_logits)); the evaluation loops score the action logits `model(x)[0][1]`, the scene test
scores the scene logits against the frozen teacher's argmax."""
from __future__ import annotations

from typing import Iterable, Optional

import torch

from . import engine_for_slot as _es


def train_class_batch(model, scene_model, samples, target, train_criterion):
    """engine/engine_for_multi_task.py:13-19: the teacher runs under no_grad; the criterion is devias_amd.multi_task_loss.TrainLoss"""
    student_output = model(samples, return_attn=False)
    with torch.no_grad():
        teacher_output = scene_model(samples, return_attn=False)
    total_loss, output, loss_dict = train_criterion(student_output, teacher_output, target)
    return total_loss, output, loss_dict


def train_one_epoch(model, scene_model, train_criterion, data_loader: Iterable, optimizer, device, epoch: int, loss_scaler=None, max_norm: float = 0, model_ema=None,
                    mixup_fn=None, log_writer=None, start_steps: int = 0, lr_schedule_values=None, wd_schedule_values=None,
                    num_training_steps_per_epoch: Optional[int] = None, update_freq: int = 1, grad_sync=None, check_finite_every: int = 50):
    """engine/engine_for_multi_task.py:27-149 on engine_for_slot._run_steps: batches are (samples, targets, _, _); one host check of the loss every
    `check_finite_every` micro-batches instead of `loss.item()` and `torch.cuda.synchronize()` at every step.  `loss_scaler` and `log_writer` are accepted and unused
    (bf16 / fp32 need no loss scale).  `mixup_fn`: None or a devias_amd.mixup.Mixup."""
    mixup_fn = _es._device_mixup(mixup_fn)
    model.train(True)
    scene_model.eval()

    def step(batch):
        samples, targets = (t.to(device, non_blocking=True) for t in batch[:2])
        if mixup_fn is not None:                                  # (:64-65) student and teacher both see the mixed clip; TrainLoss is given a SoftTargetCrossEntropy
            samples, targets = mixup_fn(samples, targets)
        loss, _output, loss_dict = train_class_batch(model, scene_model, samples, targets, train_criterion)
        return loss, loss_dict

    return _es._run_steps(step, data_loader, model, optimizer, max_norm, start_steps or 0, lr_schedule_values, wd_schedule_values, num_training_steps_per_epoch,
                          update_freq or 1, grad_sync, check_finite_every, model_ema)


@torch.no_grad()
def validation_one_epoch(data_loader, model, device, topk=(1, 5)):
    """engine/engine_for_multi_task.py:152-185 -> {'loss', 'acc1', 'acc5'} of the action logits as sample-weighted means (acc in percent)"""
    return _es._evaluate(data_loader, model, device, 2, ["acc%d" % k for k in topk], lambda out, f, _: _es._batch_metrics(out[0][1].float(), f[1], topk))


def _write_lines(first, lines, output, target, m, batch):
    """the slot engine's file lines: a first line with the LAST batch's `acc1, acc5`, then `id [logits] target chunk split` per sample"""
    rows, tgt, mh = output.cpu().numpy(), target.cpu().numpy(), m.cpu().numpy()
    first[0] = "{}, {}\n".format(100.0 * mh[2] / mh[0], 100.0 * mh[3] / mh[0])
    for i, (sample_id, chunk_nb, split_nb) in enumerate(zip(*batch[2:5])):
        lines.append("{} {} {} {} {}\n".format(sample_id, str(rows[i].tolist()), str(int(tgt[i])), str(int(chunk_nb)), str(int(split_nb))))


@torch.no_grad()
def final_test(data_loader, model, device, file):
    """engine/engine_for_multi_task.py:188-240: as validation, and the per-sample lines written to `file`"""
    first, lines = ["0.0, 0.0\n"], []

    def per_batch(out, fields, batch):
        output, target = out[0][1].float(), fields[1]
        m = _es._batch_metrics(output, target, (1, 5))
        _write_lines(first, lines, output, target, m, batch)
        return m

    stats = _es._evaluate(data_loader, model, device, 2, ["acc1", "acc5"], per_batch)
    with open(file, "w") as f:
        f.writelines(first + lines)
    return stats


@torch.no_grad()
def final_test_with_scene_label(data_loader, model, scene_model, device, file, num_labels=400, unified_head=False):
    """engine/engine_for_multi_task.py:243-304: the scene logits -- cut to the scene classes `[:, num_labels:]` under the unified head -- against the frozen
    teacher's argmax as the target"""
    scene_model.eval()
    first, lines = ["0.0, 0.0\n"], []

    def per_batch(out, fields, batch):
        output = out[1][1].float()
        if unified_head:
            output = output[:, num_labels:]
        target = torch.argmax(scene_model(fields[0], return_attn=False)[1].float(), dim=1)
        m = _es._batch_metrics(output, target, (1, 5))
        _write_lines(first, lines, output, target, m, batch)
        return m

    stats = _es._evaluate(data_loader, model, device, 1, ["acc1", "acc5"], per_batch)
    with open(file, "w") as f:
        f.writelines(first + lines)
    return stats


merge = _es.merge          # engine/engine_for_multi_task.py:307-347 reads the slot engine's line format: the same vote
