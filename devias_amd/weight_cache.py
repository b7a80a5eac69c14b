"""Compute-dtype weight copies (bf16 mode): one cast per parameter per WEIGHT UPDATE.

A copy is valid while (weights epoch, Tensor._version, storage address, device) are unchanged.  `_version` catches every in-place
update made through autograd-visible tensors (torch optimizers, load_state_dict, EMA copy_); updates made behind autograd's back --
the fused optimizer writes parameters through raw pointers in the C ABI, and `.data` writes such as broadcast_parameters -- do not
bump it, so those call invalidate_weight_cache(), which advances the global epoch.  Entries are keyed on the Parameter OBJECT
through a WeakKeyDictionary: they die with their model, and an id()/address reused by a later model cannot hit them.
"""
from __future__ import annotations

import weakref

import torch

from . import ops

_WEIGHTS_EPOCH = [0]


def invalidate_weight_cache() -> None:
    """Call after changing parameter VALUES in a way `Tensor._version` cannot see (raw-pointer kernels, `.data` writes)."""
    _WEIGHTS_EPOCH[0] += 1


class _WeakIdDict:
    """object -> value, keyed on IDENTITY and holding the key weakly (WeakKeyDictionary compares keys with ==, which is elementwise for
    tensors).  An entry disappears when its key object dies, so a recycled id() can never alias it."""

    def __init__(self):
        self._d = {}

    def get(self, obj, default=None):
        e = self._d.get(id(obj))
        return e[1] if e is not None and e[0]() is obj else default

    def __setitem__(self, obj, value):
        k = id(obj)
        self._d[k] = (weakref.ref(obj, lambda _r, k=k, d=self._d: d.pop(k, None) if (d.get(k) is not None and d[k][0] is _r) else None), value)

    def __len__(self):
        return len(self._d)


def _f32(p: torch.Tensor) -> torch.Tensor:
    d = p.detach()
    return d if d.dtype == torch.float32 and d.is_contiguous() else d.float().contiguous()


class _WeightCache:
    def __init__(self):
        self._c = _WeakIdDict()                      # Parameter -> (stamp, compute-dtype copy)
        self._cat = _WeakIdDict()                    # first Parameter of a concatenation -> {ids of the others: (stamps, weakrefs, copy)}
        self._qkvb = _WeakIdDict()                   # q_bias Parameter -> (stamps, weakref to v_bias, fp32 q_bias | 0 | v_bias)
        self._t = _WeakIdDict()                      # Parameter -> (stamp, transposed compute-dtype copy)
        self._qs = _WeakIdDict()                     # qkv weight Parameter / fp32 qkv bias tensor -> (stamp, copy with the q third scaled)
        self.casts = 0                               # number of casts performed (tests)
        self.transposes = 0
        self.qscaled = 0                             # q-scaled copies made (tests)

    @staticmethod
    def _stamp(p: torch.Tensor):
        return (_WEIGHTS_EPOCH[0], p._version, p.data_ptr(), p.device)

    def get(self, p: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        d = p.detach()
        if d.dim() > 2:
            d = d.reshape(d.shape[0], -1)
        if dtype == torch.float32:
            return d if d.is_contiguous() else d.contiguous()
        stamp = self._stamp(p)
        hit = self._c.get(p)
        if hit is not None and hit[0] == stamp and hit[1].dtype == dtype:
            return hit[1]
        w = ops.cast(d.contiguous(), dtype)
        self.casts += 1
        self._c[p] = (stamp, w)
        return w

    def get_t(self, p: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """the TRANSPOSE of a 2-D weight in the compute dtype ([in, out] for an nn.Linear weight [out, in]), cached like get(): what the encoder block's dgrad GEMMs
        read (devias_block_args.W*T) -- dY W with W transposed is a product of two k-contiguous operands, the fast layout of the GEMM kernels (round 6: 9-17 % less
        K-loop time than reading W through transposing LDS loads; same bits).  One extra copy per weight and weight update; bf16 mode only (callers)."""
        stamp = self._stamp(p)
        hit = self._t.get(p)
        if hit is not None and hit[0] == stamp and hit[1].dtype == dtype:
            return hit[1]
        w = self.get(p, dtype).t().contiguous()
        self.transposes += 1
        self._t[p] = (stamp, w)
        return w

    def get_qscaled(self, p: torch.Tensor, rows: int, factor: float, dtype: torch.dtype) -> torch.Tensor:
        """the compute-dtype copy of a [3D, D] qkv weight (or a [3D] fp32 qkv bias: dtype = torch.float32) whose first `rows` rows / entries -- the q third -- are multiplied
        by `factor` = scale * log2(e) IN FP32, before the rounding: the qkv GEMM then leaves q' = q * scale * log2(e) rounded ONCE, and forward, dQ and dK / dV kernels
        multiply the same bf16 operands (DEVIAS_ATTN_Q_PRESCALED, devias_block_args.WqkvS).  Cached like get(); backward reads the unscaled copies."""
        stamp = self._stamp(p) + (rows, factor)
        hit = self._qs.get(p)
        if hit is not None and hit[0] == stamp and hit[1].dtype == dtype:
            return hit[1]
        d = p.detach().float()
        d = d.reshape(d.shape[0], -1).clone() if d.dim() > 1 else d.clone()
        d[:rows] *= factor
        w = d if dtype == torch.float32 else ops.cast(d.contiguous(), dtype)
        self.qscaled += 1
        self._qs[p] = (stamp, w)
        return w

    def get_cat(self, ps, dtype: torch.dtype) -> torch.Tensor:
        """row-concatenation of several weights (to_k | to_v) in the compute dtype, cached like get()."""
        stamps = tuple(self._stamp(p) for p in ps)
        slot = self._cat.get(ps[0])
        key = tuple(id(p) for p in ps[1:])
        if slot is not None:
            hit = slot.get(key)
            if hit is not None and hit[0] == stamps and hit[2].dtype == dtype and all(r() is q for r, q in zip(hit[1], ps[1:])):
                return hit[2]
        w = torch.cat([self.get(p, dtype) for p in ps], dim=0).contiguous()
        if slot is None:
            slot = self._cat[ps[0]] = {}
        slot[key] = (stamps, tuple(weakref.ref(q) for q in ps[1:]), w)
        return w

    def qkv_bias(self, qb: torch.Tensor, vb: torch.Tensor) -> torch.Tensor:
        """fp32 [3D] = q_bias | zeros | v_bias (modeling_slot.py:97-99), rebuilt only when one of the two changed"""
        stamp = (self._stamp(qb), self._stamp(vb))
        hit = self._qkvb.get(qb)
        if hit is not None and hit[0] == stamp and hit[1]() is vb:
            return hit[2]
        t = torch.cat((_f32(qb), torch.zeros_like(_f32(vb)), _f32(vb))).contiguous()
        self._qkvb[qb] = (stamp, weakref.ref(vb), t)
        return t


_WCACHE = _WeightCache()

# scale * log2(e) for head dim 64: the factor the q third of the qkv projection carries where the attention kernels run with DEVIAS_ATTN_Q_PRESCALED
_Q_PRESCALE = (64 ** -0.5) * 1.4426950408889634


def _use_q_prescale(cdt, drop=None) -> bool:
    """bf16 encoder blocks without attention dropout: the qkv GEMM runs on a copy of its weight / bias whose q third carries scale * log2(e), so that forward, dQ and
    dK / dV kernels multiply the same bf16 operands (library option attn_qpre, default 1; 0 = every kernel scales on its own: A/B aid)."""
    return cdt == torch.bfloat16 and drop is None and ops.get_option("attn_qpre") != 0
