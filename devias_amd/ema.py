"""Model EMA: the shadow weights the reference's drivers keep under --model_ema (run_slot_finetuning.py:506-510 builds timm's ModelEma, the engines call
`model_ema.update(model)` after each optimizer step, engine/engine_for_slot.py:154-155, 165-168, and utils/utils.py:456-457 saves them under 'model_ema').

timm's update, restated (timm is not a dependency): per state_dict entry, in the entry's dtype,

    ema_v.copy_(ema_v * decay + (1. - decay) * model_v)

which for fp32 is three single-rounded operations, fl(fl(e * fl32(decay)) + fl(w * fl32(1. - decay))), the second factor evaluated in double first.  Every path here
computes exactly that: fp32 contiguous entries on the GPU in one devias_ema_multi launch over a cached descriptor table (or inside the optimizer's own launch,
FusedAdamW.step(ema=...), which then hands this class only the entries it did not cover), anything else by the torch expression itself.

A state_dict lists a tensor shared by several modules (the tied aggregator layers) once per module, and timm's loop updates the shared shadow once per listing.  One launch
cannot apply two updates to one tensor in order, so the k-th listing of a tensor goes into the k-th launch.

The launches write the shadows through raw pointers, which Tensor._version does not see: each calls invalidate_weight_cache(), or a later forward of `.ema` would run on
the stale compute-dtype copies of its weights (weight_cache.py)."""
from __future__ import annotations

import copy

import numpy as np
import torch

from . import ops
from .optim import _REC, chunk_lists
from .weight_cache import invalidate_weight_cache


def _on_kernel_path(ema_v: torch.Tensor, model_v: torch.Tensor) -> bool:
    return (ema_v.is_cuda and model_v.device == ema_v.device and ema_v.dtype == torch.float32 and model_v.dtype == torch.float32
            and ema_v.is_contiguous() and model_v.is_contiguous() and ema_v.numel() == model_v.numel() and ema_v.numel() > 0
            and not overlaps(ema_v, model_v))


def overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    """do the two contiguous tensors share bytes"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


class _Launch:
    """one devias_ema_multi launch: the device table of (param, ema, n) records and its chunk lists"""

    def __init__(self, pairs, device):
        rec = np.zeros(len(pairs), _REC)
        for i, (ema_v, model_v) in enumerate(pairs):
            rec[i]["param"], rec[i]["ema"], rec[i]["n"] = model_v.data_ptr(), ema_v.data_ptr(), ema_v.numel()
        self.table = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(device)
        self.chunk_tensor, self.chunk_index = chunk_lists([e.numel() for e, _ in pairs], device)


class ModelEma:
    """timm.utils.ModelEma's surface: `.ema` (a deep copy of `model` in eval mode, no gradients), `.decay`, `.update(model)`; `device='cpu'` keeps the shadow on the
    host (the reference's --model_ema_force_cpu).  `resume` names a checkpoint file whose shadow is loaded: the 'model_ema' entry of a checkpoint of
    devias_amd.checkpoint.save_checkpoint, or timm's 'state_dict_ema'."""

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, device="", resume: str = ""):
        ops.ema_factors(decay)                                   # refuses a decay outside [0, 1]
        self.ema = copy.deepcopy(model)
        self.ema.eval()
        self.decay = decay
        self.device = device
        if device:
            self.ema.to(device=device)
        self.ema_has_module = hasattr(self.ema, "module")
        self.source = model                                      # FusedAdamW.step(ema=...) finds its parameters' names here
        self._plans = {}
        if resume:
            ck = torch.load(resume, map_location="cpu", weights_only=False)
            for key in ("model_ema", "state_dict_ema"):
                if isinstance(ck, dict) and key in ck:
                    ck = ck[key]
                    break
            self.load_state_dict(ck)
        for p in self.ema.parameters():
            p.requires_grad_(False)

    def state_dict(self):
        return self.ema.state_dict()

    def load_state_dict(self, state_dict, strict: bool = True):
        out = self.ema.load_state_dict(state_dict, strict=strict)
        invalidate_weight_cache()                                # belt and braces, as checkpoint.load_state_dict: copy_ moves Tensor._version
        return out

    def on_device_of(self, model: torch.nn.Module) -> bool:
        """every shadow parameter lives on the GPU of its model parameter: what the fused optimizer launch needs"""
        dev = {p.device for p in model.parameters()}
        return len(dev) == 1 and next(iter(dev)).type == "cuda" and all(p.device in dev for p in self.ema.parameters())

    @torch.no_grad()
    def update(self, model: torch.nn.Module) -> None:
        needs_module = hasattr(model, "module") and not self.ema_has_module
        msd = model.state_dict()
        self.apply([(ema_v, msd["module." + k if needs_module else k].detach()) for k, ema_v in self.ema.state_dict().items()])

    @torch.no_grad()
    def apply(self, pairs) -> None:
        """the update for the given (shadow, model value) pairs, in order"""
        kernel, seen, rounds = [], {}, []
        for ema_v, model_v in pairs:
            if self.device:
                model_v = model_v.to(device=self.device)
            if _on_kernel_path(ema_v, model_v):
                k = seen[ema_v.data_ptr()] = seen.get(ema_v.data_ptr(), 0) + 1
                if k > len(rounds):
                    rounds.append([])
                rounds[k - 1].append((ema_v, model_v))
                kernel.append((ema_v.data_ptr(), model_v.data_ptr(), ema_v.numel()))
            else:
                ema_v.copy_(ema_v * self.decay + (1. - self.decay) * model_v)
        if not rounds:
            return
        key = tuple(kernel)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= 8:                            # storage moved (module.to(), new tensors): drop the tables of the old addresses
                self._plans.clear()
            plan = self._plans[key] = [_Launch(r, r[0][0].device) for r in rounds]
        invalidate_weight_cache()
        for launch in plan:
            ops.ema_multi(launch.table, launch.chunk_tensor, launch.chunk_index, self.decay)
