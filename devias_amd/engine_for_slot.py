"""Step semantics of engine/engine_for_slot.py for the MI355X path: train_class_batch (:50-56) and a lean
train_one_epoch (:64-214) without per-step host syncs.  The teacher may be a module (forward under no_grad, as in the
reference) or precomputed scene logits (the primary benchmark metric treats them as an input)."""
from __future__ import annotations

import math
import os
import sys
from typing import Iterable, Optional

import numpy as np
import torch

from .optim import FusedAdamW


def train_class_batch(model, scene_model, samples, target, train_criterion, fg_mask=None):
    """engine/engine_for_slot.py:50-56.  `scene_model` is a module returning (token, logits) or a [B, 365] logits tensor."""
    student_output = model(samples)
    if torch.is_tensor(scene_model):
        teacher_output = (None, scene_model)
    else:
        with torch.no_grad():
            teacher_output = scene_model(samples, return_attn=False)
    total_loss, output, loss_dict = train_criterion(model, student_output, teacher_output, target, fg_mask=fg_mask)
    return total_loss, output, loss_dict


def _device_mixup(mixup_fn):
    """the `mixup_fn` of the plain, scene and multi-task engines: None, or a devias_amd.mixup.Mixup (batch mixed in place by one kernel launch, dense soft target).  Any
    other callable -- the reference's host-side Mixup among them -- is refused: its nine tensor passes per batch are not built."""
    if mixup_fn is None:
        return None
    from .mixup import Mixup
    if not isinstance(mixup_fn, Mixup):
        raise NotImplementedError(f"mixup_fn must be a devias_amd.mixup.Mixup (mixup / cutmix on the device), got {type(mixup_fn).__name__}: no other mixup callable is built")
    return mixup_fn


def _run_steps(step, data_loader, model, optimizer, max_norm, start_steps, lr_schedule_values, wd_schedule_values, num_training_steps_per_epoch, update_freq, grad_sync, check_finite_every, model_ema=None):
    """The part of train_one_epoch that does not depend on the recipe (shared with engine_for_slot_hvu): LR/WD schedule poke, gradient accumulation over
    `update_freq` micro-batches, optional gradient all-reduce (`grad_sync`, devias_amd.parallel), clip + optimizer step, and one host check of the loss
    every `check_finite_every` micro-batches.  `step(batch) -> (loss, loss_dict)` is the recipe: H2D copies, mask model, train_class_batch.
    `model_ema` (devias_amd.ema.ModelEma) is updated after each optimizer step and only then (engine/engine_for_slot.py:154-155, 165-168): inside the fused
    optimizer's launch where that is what steps, by `model_ema.update(model)` after any other optimizer."""
    optimizer.zero_grad(set_to_none=True)
    stats, grad_norm = {}, None
    for data_iter_step, batch in enumerate(data_loader):
        it = data_iter_step // update_freq
        if num_training_steps_per_epoch is not None and it >= num_training_steps_per_epoch:
            continue
        it += start_steps
        if (lr_schedule_values is not None or wd_schedule_values is not None) and data_iter_step % update_freq == 0:
            for group in optimizer.param_groups:
                if lr_schedule_values is not None:
                    group["lr"] = lr_schedule_values[it] * group.get("lr_scale", 1.0)
                if wd_schedule_values is not None and group["weight_decay"] > 0:
                    group["weight_decay"] = wd_schedule_values[it]
        loss, loss_dict = step(batch)
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
                if model_ema is not None and model_ema.source is model and model_ema.on_device_of(model):
                    optimizer.step(max_norm=float(max_norm or 0.0), ema=model_ema)
                else:
                    optimizer.step(max_norm=float(max_norm or 0.0))
                    if model_ema is not None:                      # a shadow kept on the host (--model_ema_force_cpu), or of a wrapped model
                        model_ema.update(model)
                grad_norm = optimizer.last_grad_norm
            else:
                if max_norm and max_norm > 0:
                    grad_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
                optimizer.step()
                if model_ema is not None:
                    model_ema.update(model)
            optimizer.zero_grad(set_to_none=True)
        if check_finite_every and (data_iter_step + 1) % check_finite_every == 0:          # skipped batches only follow, so this counts the ones run
            loss_value = float(loss.detach().float().sum())
            if not math.isfinite(loss_value):
                print("Loss is {}, stopping training".format(loss_value))
                sys.exit(1)
            if grad_norm is not None:
                stats["grad_norm"] = float(grad_norm)
            stats.update(loss=loss_value, lr=max(g["lr"] for g in optimizer.param_groups), min_lr=min(g["lr"] for g in optimizer.param_groups), **{k: float(v) for k, v in loss_dict.items()})
    return stats


def train_one_epoch(model, scene_model, train_criterion, data_loader: Iterable, optimizer, device, epoch: int,
                    max_norm: float = 0, start_steps: int = 0, lr_schedule_values=None, wd_schedule_values=None,
                    num_training_steps_per_epoch: Optional[int] = None, update_freq: int = 1, mask_model=None,
                    grad_sync=None, check_finite_every: int = 50, log_every: int = 100, model_ema=None):
    """engine/engine_for_slot.py:64-214 restated for this stack: LR/WD schedule poke (:91-96), H2D (:98-99), mask model (:106-108), train_class_batch,
    backward, optional gradient all-reduce, optimizer step (_run_steps).  The per-step `loss.item()` finite check (:140-144) and
    `torch.cuda.synchronize()` (:171) are replaced by one host check every `check_finite_every` steps."""
    model.train(True)
    if not torch.is_tensor(scene_model):
        scene_model.eval()

    def step(batch):
        samples, targets = (t.to(device, non_blocking=True) for t in batch[:2])
        if mask_model is not None:
            samples, targets, masks = mask_model(samples, targets)
        else:
            masks = tuple(m.to(device, non_blocking=True) for m in batch[2])
        loss, _output, loss_dict = train_class_batch(model, scene_model, samples, targets, train_criterion, fg_mask=masks)
        return loss, loss_dict

    return _run_steps(step, data_loader, model, optimizer, max_norm, start_steps, lr_schedule_values, wd_schedule_values, num_training_steps_per_epoch,
                      update_freq, grad_sync, check_finite_every, model_ema)


def _evaluate(data_loader, model, device, n_fields, names, per_batch):
    """One eval-mode pass, shared by every validation loop of both recipes: the first `n_fields` fields of a batch go to the device, the model runs on field 0,
    and `per_batch(model output, device fields, batch)` returns float64 [n, sum of CE, one hit count per name].  The sums stay on the device; one host read at
    the end of the loader (the reference reads three scalars per batch).  -> {'loss', *names} as sample-weighted means (the hit counts in percent)"""
    model.eval()
    acc = torch.zeros(2 + len(names), dtype=torch.float64, device=device)
    for batch in data_loader:
        fields = [f.to(device, non_blocking=True) for f in batch[:n_fields]]
        acc += per_batch(model(fields[0]), fields, batch)
    vals = acc.tolist()
    n = max(vals[0], 1.0)
    return {"loss": vals[1] / n, **{k: 100.0 * h / n for k, h in zip(names, vals[2:])}}


@torch.no_grad()
def validation_one_epoch(data_loader, model, device, topk=(1, 5)):
    """engine/engine_for_slot.py:215-250: eval-mode forward, cross-entropy of the selected action logits [B, nb + ns] against
    the action target, top-1 / top-5 accuracy.  Returns {'loss', 'acc1', 'acc5'} as sample-weighted means (acc in percent)."""
    return _evaluate(data_loader, model, device, 2, ["acc%d" % k for k in topk], lambda out, f, _: _batch_metrics(out[1][0].float(), f[1], topk))


def _batch_metrics(output, target, topk):
    """[B, sum of per-sample CE, top-k hit counts] of one batch (timm.utils.accuracy semantics: a hit if the target is among the
    k largest logits).  [B, 765] metric arithmetic, not part of the hot path."""
    logp = torch.log_softmax(output, dim=-1)
    ce = -logp.gather(1, target.view(-1, 1)).sum()
    _, pred = output.topk(max(topk), dim=1)
    hit = pred.eq(target.view(-1, 1))
    vals = [torch.tensor(float(output.shape[0]), device=output.device, dtype=torch.float64), ce.double()]
    vals += [hit[:, :k].any(dim=1).sum().double() for k in topk]
    return torch.stack(vals)


@torch.no_grad()
def final_test(data_loader, model, device, file):
    """engine/engine_for_slot.py:253-303: as validation, and one line `id [logits] target chunk split` per sample written to
    `file` after a first line with the LAST batch's `acc1, acc5` (the reference writes exactly that)."""
    lines = ["0.0, 0.0\n"]

    def per_batch(out, fields, batch):
        output, target = out[1][0].float(), fields[1]
        m = _batch_metrics(output, target, (1, 5))
        rows, tgt, mh = output.cpu().numpy(), target.cpu().numpy(), m.cpu().numpy()
        lines[0] = "{}, {}\n".format(100.0 * mh[2] / mh[0], 100.0 * mh[3] / mh[0])
        for i, (sample_id, chunk_nb, split_nb) in enumerate(zip(*batch[2:5])):
            lines.append("{} {} {} {} {}\n".format(sample_id, str(rows[i].tolist()), str(int(tgt[i])), str(int(chunk_nb)), str(int(split_nb))))
        return m

    stats = _evaluate(data_loader, model, device, 2, ["acc1", "acc5"], per_batch)
    with open(file, "w") as f:
        f.writelines(lines)
    return stats


@torch.no_grad()
def final_test_with_scene_label(data_loader, model, scene_model, device, file, num_labels=400):
    """engine/engine_for_slot.py:310-367, the `--eval --eval_scene` mode: the logits of the selected SCENE slot, cut to the scene classes `[:, num_labels:]` of the
    unified head, against the frozen teacher's argmax as the target.  Writes the reference's file -- a first line with the LAST batch's `acc1, acc5` (the reference
    formats the two 0-d tensors timm's `accuracy` returns; so does this), then one line `id [logits] target chunk split` per sample -- and returns
    {'loss', 'acc1', 'acc5'} as sample-weighted means (acc in percent)."""
    scene_model.eval()
    first, lines = ["0.0, 0.0\n"], []

    def per_batch(out, fields, batch):
        output = out[1][1].float()[:, num_labels:]
        target = torch.argmax(scene_model(fields[0], return_attn=False)[1], dim=1)
        m = _batch_metrics(output, target, (1, 5))
        n = output.shape[0]
        first[0] = "{}, {}\n".format(m[2].float() * 100. / n, m[3].float() * 100. / n)
        rows, tgt = output.cpu().numpy(), target.cpu().numpy()
        for i, (sample_id, chunk_nb, split_nb) in enumerate(zip(*batch[2:5])):
            lines.append("{} {} {} {} {}\n".format(sample_id, str(rows[i].tolist()), str(int(tgt[i])), str(int(chunk_nb)), str(int(split_nb))))
        return m

    stats = _evaluate(data_loader, model, device, 1, ["acc1", "acc5"], per_batch)
    with open(file, "w") as f:
        f.writelines(first + lines)
    return stats


def merge(eval_path, num_tasks):
    """engine/engine_for_slot.py:370-419, the multi-view vote every reported test accuracy goes through: reads `0.txt` ... `(num_tasks - 1).txt` as written by
    final_test / final_test_with_scene_label, takes the softmax of every view, drops a repeated (chunk, split) of a video (the first one stays; the key is the
    reference's, the two numbers' digits joined), averages the views of a video and returns (top-1, top-5) in percent.  A video's label is that of its last kept
    view.  Vectorised numpy in the calling process: one softmax over all views, one segmented sum over the views sorted by video (the reference maps a pool of 64
    processes over the videos)."""
    index, seen, vid, label, feats = {}, set(), [], [], []
    for x in range(num_tasks):
        with open(os.path.join(eval_path, str(x) + ".txt"), "r") as f:
            rows = f.readlines()[1:]
        for line in rows:
            line = line.strip()
            name, rest = line.split("[")[0], line.split("]")[1].split(" ")
            v = index.setdefault(name, len(index))
            if len(label) <= v:
                label.append(0)
            if (v, rest[2] + rest[3]) in seen:
                continue
            seen.add((v, rest[2] + rest[3]))
            label[v] = int(rest[1])
            vid.append(v)
            feats.append(np.array(line.split("[")[1].split("]")[0].split(","), dtype=np.float64))
    if not vid:
        return float("nan"), float("nan")
    z = np.stack(feats)
    z = np.exp(z - z.max(axis=1, keepdims=True))
    p = z / z.sum(axis=1, keepdims=True)
    vid, label = np.asarray(vid), np.asarray(label)
    order = np.argsort(vid, kind="stable")
    counts = np.bincount(vid, minlength=len(index))
    mean = np.add.reduceat(p[order], np.concatenate(([0], np.cumsum(counts)[:-1])), axis=0) / counts[:, None]
    top5 = np.argsort(-mean, axis=1)[:, :5]
    top1 = (np.argmax(mean, axis=1) == label) * 1.0
    return float(np.mean(top1) * 100), float(np.mean((top5 == label[:, None]).any(axis=1) * 1.0) * 100)
