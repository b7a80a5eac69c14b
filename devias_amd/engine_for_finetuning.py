"""Step semantics of engine/engine_for_finetuning.py, the plain (model, criterion) engine of the downstream recipe (run_slot_downstream.py), on the shared step loop
and evaluation pass of engine_for_slot: train_class_batch (:13-16), train_one_epoch (:24-143), validation_one_epoch (:146-179), final_test (:183-235), merge (:238-278)."""
from __future__ import annotations

import os
import tempfile
from typing import Iterable, Optional

import torch

from . import engine_for_slot as _es


def train_class_batch(model, samples, target, criterion):
    """engine/engine_for_finetuning.py:13-16: the model returns (token, logits); the criterion sees the logits"""
    _, outputs = model(samples)
    loss = criterion(outputs, target)
    return loss, outputs


def train_one_epoch(model, criterion, data_loader: Iterable, optimizer, device, epoch: int, loss_scaler=None, max_norm: float = 0, model_ema=None, mixup_fn=None,
                    log_writer=None, start_steps: int = 0, lr_schedule_values=None, wd_schedule_values=None, num_training_steps_per_epoch: Optional[int] = None,
                    update_freq: int = 1, grad_sync=None, check_finite_every: int = 50):
    """engine/engine_for_finetuning.py:24-143 on engine_for_slot._run_steps: one host check of the loss every `check_finite_every` micro-batches instead of
    `loss.item()` and `torch.cuda.synchronize()` at every step.  `loss_scaler` and `log_writer` are accepted and unused (bf16 / fp32 need no loss scale).  `mixup_fn`:
    None or a devias_amd.mixup.Mixup (the batch is mixed in place on the device)."""
    mixup_fn = _es._device_mixup(mixup_fn)
    model.train(True)

    def step(batch):
        samples, targets = (t.to(device, non_blocking=True) for t in batch[:2])
        if mixup_fn is not None:                                  # (:62-63) after the copy to the device; the criterion is then a SoftTargetCrossEntropy
            samples, targets = mixup_fn(samples, targets)
        loss, _output = train_class_batch(model, samples, targets, criterion)
        return loss, {}

    return _es._run_steps(step, data_loader, model, optimizer, max_norm, start_steps or 0, lr_schedule_values, wd_schedule_values, num_training_steps_per_epoch,
                          update_freq or 1, grad_sync, check_finite_every, model_ema)


@torch.no_grad()
def validation_one_epoch(data_loader, model, device, topk=(1, 5)):
    """engine/engine_for_finetuning.py:146-179 -> {'loss', 'acc1', 'acc5'} as sample-weighted means (acc in percent)"""
    return _es._evaluate(data_loader, model, device, 2, ["acc%d" % k for k in topk], lambda out, f, _: _es._batch_metrics(out[1].float(), f[1], topk))


@torch.no_grad()
def final_test(data_loader, model, device, file):
    """engine/engine_for_finetuning.py:183-235: one line `id output : [logits] : output target chunk split` per sample after a first line with the LAST batch's
    `acc1, acc5`"""
    lines = ["0.0, 0.0\n"]

    def per_batch(out, fields, batch):
        output, target = out[1].float(), fields[1]
        m = _es._batch_metrics(output, target, (1, 5))
        rows, tgt, mh = output.cpu().numpy(), target.cpu().numpy(), m.cpu().numpy()
        lines[0] = "{}, {}\n".format(100.0 * mh[2] / mh[0], 100.0 * mh[3] / mh[0])
        for i, (sample_id, chunk_nb, split_nb) in enumerate(zip(*batch[2:5])):
            lines.append("{} {} {} {} {}\n".format(sample_id, "output : " + str(rows[i].tolist()) + " : output", str(int(tgt[i])), str(int(chunk_nb)), str(int(split_nb))))
        return m

    stats = _es._evaluate(data_loader, model, device, 2, ["acc1", "acc5"], per_batch)
    with open(file, "w") as f:
        f.writelines(lines)
    return stats


def merge(eval_path, num_tasks):
    """engine/engine_for_finetuning.py:238-278: the multi-view vote over `0.txt` ... `(num_tasks - 1).txt`.  This engine's files mark the logits with
    `output : [` ... `] : output` (for sample ids that contain brackets, :209); with the markers taken out and the id replaced by a number a line is the slot engine's, whose merge does the vote."""
    names = {}
    with tempfile.TemporaryDirectory() as td:
        for x in range(num_tasks):
            with open(os.path.join(eval_path, str(x) + ".txt"), "r") as f:
                rows = f.readlines()
            out = rows[:1]
            for r in rows[1:]:
                name, tail = r.split("output : [", 1)
                data, rest = tail.split("] : output", 1)
                out.append("v{} [{}]{}".format(names.setdefault(name, len(names)), data, rest))
            with open(os.path.join(td, str(x) + ".txt"), "w") as f:
                f.writelines(out)
        return _es.merge(td, num_tasks)
