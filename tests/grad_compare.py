"""Element-wise comparison of two gradient sets {name: grad} (a plain helper module like golden_util.py).

A norm comparison hides almost every error that is not parallel to the gradient: ||g + e||^2 = ||g||^2 + 2 g.e + ||e||^2, so a 20 % error
orthogonal to g moves the norm by 2 %.  This module measures, per parameter,
  rel  -- ||g - r|| / max(||r||, 1e-6 * max_p ||r_p||)   (the floor convention of golden_util.check_against_golden: a handful of
          gradients are mathematically zero and hold only round-off in the reference too),
  cos  -- the cosine between g and r,
  blk  -- the worst relative error over blocks of 64 output features (rows of a weight viewed as [out, -1], entries of a bias); for
          the qkv weight one block is one head's q, k or v.  A block is measured against max(||r_b||, a tenth of the tensor's RMS block
          norm, the global floor), so that a nearly-empty block does not turn round-off into a large ratio,
and groups parameters into families that carry one bound each."""
import math
import re
from dataclasses import dataclass

import torch

BLOCK = 64

# first match wins
FAMILIES = (
    ("latents", re.compile(r"^agg_block\.latents$")),
    ("patch_embed", re.compile(r"^patch_embed\.")),
    ("qkv_weight", re.compile(r"^blocks\.\d+\.attn\.qkv\.weight$")),
    ("qv_bias", re.compile(r"^blocks\.\d+\.attn\.[qv]_bias$")),
    ("proj", re.compile(r"^blocks\.\d+\.attn\.proj\.")),
    ("fc1", re.compile(r"^blocks\.\d+\.mlp\.fc1\.")),
    ("fc2", re.compile(r"^blocks\.\d+\.mlp\.fc2\.")),
    ("norm", re.compile(r"^(blocks\.\d+\.norm[12]|norm)\.")),
    ("agg_block", re.compile(r"^agg_block\.")),
    ("head", re.compile(r"^(head|mask_predictor)\.")),
)
FAMILY_NAMES = tuple(f for f, _ in FAMILIES)


def family(name: str) -> str:
    for fam, rx in FAMILIES:
        if rx.search(name):
            return fam
    raise KeyError(f"parameter {name!r} belongs to no gradient family")


@dataclass
class ParamErr:
    rel: float
    cos: float
    blk: float

    @property
    def worst(self) -> float:
        return max(self.rel, self.blk)


def compare(grads: dict, ref: dict, block: int = BLOCK) -> dict:
    """{name: ParamErr} for every name of `ref`; `grads` must hold the same names and shapes"""
    assert set(grads) == set(ref), sorted(set(grads) ^ set(ref))[:8]
    floor = 1e-6 * max(float(r.detach().double().norm()) for r in ref.values())
    out = {}
    for n in ref:
        g = grads[n].detach().double()                # float64 on the gradients' own device
        r = ref[n].detach().to(device=g.device, dtype=torch.float64)
        assert g.shape == r.shape, (n, tuple(g.shape), tuple(r.shape))
        e = g - r
        rn, gn = float(r.norm()), float(g.norm())
        rel = float(e.norm()) / max(rn, floor)
        cos = float((g * r).sum()) / (gn * rn) if gn > 0 and rn > 0 else (1.0 if gn == rn else 0.0)
        rows = r.shape[0] if r.dim() > 0 else 1
        nb = max(1, math.ceil(rows / block))
        # per-block squared norms over the leading (output-feature) dimension
        pad = nb * block - rows
        e2 = (e.reshape(rows, -1) ** 2).sum(1)
        r2 = (r.reshape(rows, -1) ** 2).sum(1)
        if pad:
            e2 = torch.cat((e2, e2.new_zeros(pad)))
            r2 = torch.cat((r2, r2.new_zeros(pad)))
        eb = e2.reshape(nb, -1).sum(1).sqrt()
        rb = r2.reshape(nb, -1).sum(1).sqrt()
        bfloor = max(0.1 * rn / math.sqrt(nb), floor)
        blk = float((eb / rb.clamp_min(bfloor)).max())
        out[n] = ParamErr(rel, cos, blk)
    return out


def summarize(errs: dict) -> dict:
    """{family: (worst rel, smallest cos, worst blk, name of the worst parameter)}"""
    fam = {}
    for n, e in errs.items():
        f = family(n)
        w = fam.get(f)
        if w is None:
            fam[f] = (e.rel, e.cos, e.blk, n)
        else:
            fam[f] = (max(w[0], e.rel), min(w[1], e.cos), max(w[2], e.blk), n if e.worst > max(w[0], w[2]) else w[3])
    return fam


def report(errs: dict, label: str) -> dict:
    """prints one line per family (worst rel, smallest cosine, worst 64-row block, the parameter that holds the worst) and returns summarize()"""
    fam = summarize(errs)
    for f in FAMILY_NAMES:
        if f in fam:
            rel, cos, blk, n = fam[f]
            print(f"[grad] {label} {f:<11} rel {rel:.2e}  cos {cos:.8f}  blk64 {blk:.2e}  ({n})")
    return fam


def violations(errs: dict, bounds: dict, scale: float = 1.0) -> dict:
    """{name: (family, worst of rel / blk, bound)} of every parameter whose rel or blk error exceeds scale * its family's bound"""
    bad = {}
    for n, e in errs.items():
        f = family(n)
        tol = scale * bounds[f]
        if not (e.rel <= tol and e.blk <= tol):
            bad[n] = (f, e.worst, tol)
    return bad


def check(grads: dict, ref: dict, bounds: dict, label: str, scale: float = 1.0) -> dict:
    """compare + report + assert every parameter within its family's bound (times `scale`); returns the per-parameter errors"""
    errs = compare(grads, ref)
    report(errs, label)
    bad = violations(errs, bounds, scale)
    worst = sorted(bad.items(), key=lambda kv: -kv[1][1] / kv[1][2])
    assert not bad, f"{label}: {len(bad)} gradients off their family bound: " + ", ".join(
        f"{n} [{f}] {v:.3e} > {t:.1e}" for n, (f, v, t) in worst[:8])
    return errs
