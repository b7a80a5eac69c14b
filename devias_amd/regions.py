"""The fused regions: ONE library call per region and direction (devias_encoder_block_* / devias_agg_block_* / devias_head_*).

The kernel sequence of a region is issued by the library (csrc/regions.hip) -- the same launches in the same order as the per-kernel
Functions of devias_amd.functions, bitwise the same results (tests/test_regions_gpu.py) -- so a step costs ~40 Python -> library hops instead of ~750.
What backward needs lives in ONE arena tensor per region call, backward temporaries in a grow-only scratch buffer per stream, the
parameter gradients of a region in one flat fp32 tensor (or straight in the data-parallel gradient bucket views).
"""
from __future__ import annotations

import ctypes as _ct
import math

import torch
from torch.autograd import Function

from . import _lib as _L
from . import ops
from .functions import _LAYER_KEYS, _gout, _peek_colsum, _publish_colsum, _weight_sets
from .weight_cache import _Q_PRESCALE, _WCACHE, _f32, _use_q_prescale

_scratch_bufs = {}


def _scratch(nbytes: int, device) -> torch.Tensor:
    """grow-only backward scratch per (device, stream): the temporaries of a region's backward are dead when its kernels have run, and the
    kernels of one stream are ordered"""
    key = (torch.device(device).index or 0, torch.cuda.current_stream(device).cuda_stream)
    buf = _scratch_bufs.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = None
        _scratch_bufs.pop(key, None)
        buf = _scratch_bufs[key] = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    return buf


class _GradDest:
    """fp32 gradient destinations of one region: a parameter whose gradient bucket view is free gets that view (a fresh alias, see _gout);
    the others are carved out of ONE flat tensor"""

    def __init__(self, items, device):
        self.out = []
        views = [(_gout(p, shape) if p is not None else None) for p, shape in items]
        total = 0
        for (p, shape), v in zip(items, views):
            if v is None:
                total += (math.prod(shape) + 63) // 64 * 64           # 256-byte aligned pieces
        flat = torch.empty((total,), dtype=torch.float32, device=device) if total else None
        off = 0
        for (p, shape), v in zip(items, views):
            if v is None:
                n = math.prod(shape)
                v = flat[off:off + n].view(shape)
                off += (n + 63) // 64 * 64
            self.out.append(v)

    def ptrs(self):
        return [t.data_ptr() for t in self.out]


def _region_state(ctx, who: str, index: int):
    """The fused-region Functions keep their arena, weight copies and argument struct on `ctx` as raw pointers (not save_for_backward: the arena is
    written by the library, not by autograd) and drop them after ONE backward.  A second backward (retain_graph=True) or an input modified in place
    between forward and backward must fail with a message, not with a TypeError on None or silently wrong gradients.  `index`: where the
    region's input stands in ctx.keep."""
    if ctx.keep is None:
        raise RuntimeError(f"{who}: backward already consumed this region's saved arena; the fused regions support ONE backward per forward "
                           "(run forward again instead of retain_graph=True)")
    x = ctx.keep[index]
    if x._version != ctx.x_version:
        raise RuntimeError(f"{who}: the region's input was modified in place between forward and backward (version {ctx.x_version} -> {x._version}); "
                           "its saved activations no longer match it")


def _will_backward(ctx, grad_enabled) -> bool:
    """Whether a forward has to save for a backward: the caller had autograd on (read BEFORE apply: inside forward it is always off) and an input requires a
    gradient.  Where not, nothing is kept on `ctx` and the caller hands the library no arena (save = NULL: it keeps the intermediates in its workspace; same bits)."""
    ctx.keep = ctx.args = None
    return bool(grad_enabled) and any(ctx.needs_input_grad)


class EncoderBlockRegionFn(Function):
    """EncoderBlockFn as one devias_encoder_block_fwd / _bwd call (Block.forward, modeling_slot.py:142-152)"""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkvw, qb, vb, pw, pb, n2w, n2b, f1w, f1b, f2w, f2b, meta, ds1=None, ds2=None):
        B, N, H, eps, cdt = meta
        lib = _L.load()
        dev = x.device
        D = x.shape[1]
        hid = f1w.shape[0]
        dt = ops.dt_code(cdt)
        x = x.contiguous()
        keep = [_f32(n1w), _f32(n1b), _f32(n2w), _f32(n2b)] + [_WCACHE.get(w, cdt) for w in (qkvw, pw, f1w, f2w)] + \
               [_WCACHE.qkv_bias(qb, vb), _f32(pb), _f32(f1b), _f32(f2b)]
        save = torch.empty((lib.devias_encoder_block_save_bytes(B, N, D, H, hid, dt),), dtype=torch.uint8, device=dev)
        a = _L.BlockArgs()
        a.B, a.N, a.D, a.H, a.hidden, a.dtype, a.eps = B, N, D, H, hid, dt, eps
        (a.n1w, a.n1b, a.n2w, a.n2b, a.Wqkv, a.Wp, a.W1, a.W2, a.qkv_bias, a.pb, a.b1, a.b2) = [t.data_ptr() for t in keep]
        if _use_q_prescale(cdt):
            qs = [_WCACHE.get_qscaled(qkvw, D, _Q_PRESCALE, cdt), _WCACHE.get_qscaled(keep[8], D, _Q_PRESCALE, torch.float32)]
            keep = keep + qs
            a.WqkvS, a.qkv_biasS = qs[0].data_ptr(), qs[1].data_ptr()
        if cdt != torch.float32 and any(ctx.needs_input_grad):
            # transposed weight copies for the four dgrad GEMMs of the backward (bf16 mode: the fp32 parity kernels stage through registers and do not care)
            wt = [_WCACHE.get_t(w, cdt) for w in (qkvw, pw, f1w, f2w)]
            keep = keep + wt
            (a.WqkvT, a.WpT, a.W1T, a.W2T) = [t.data_ptr() for t in wt]
        a.ds1 = ds1.data_ptr() if ds1 is not None else None
        a.ds2 = ds2.data_ptr() if ds2 is not None else None
        a.save = save.data_ptr()
        ops.attach_workspace(a, lib.devias_encoder_block_workspace_bytes(B, N, D, H, hid, dt), dev)
        x2 = torch.empty_like(x)
        _L.check(lib.devias_encoder_block_fwd(_ct.byref(a), x.data_ptr(), x2.data_ptr(), ops._stream()), "devias_encoder_block_fwd")
        ctx.args = a
        ctx.meta = meta
        ctx.keep = (keep, save, ds1, ds2, x)
        ctx.x_version = x._version
        ctx.params = (n1w, n1b, qkvw, pw, pb, n2w, n2b, f1w, f1b, f2w, f2b, qb, vb)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        B, N, H, eps, cdt = ctx.meta
        lib = _L.load()
        _region_state(ctx, "EncoderBlockRegionFn", 4)
        a = ctx.args
        keep, save, ds1, ds2, x = ctx.keep
        (p_n1w, p_n1b, p_qkvw, p_pw, p_pb, p_n2w, p_n2b, p_f1w, p_f1b, p_f2w, p_f2b, p_qb, p_vb) = ctx.params
        dev = x.device
        D, hid = a.D, a.hidden
        dx2 = dx2.contiguous()
        ready = _peek_colsum(dx2) if ds2 is None else None          # colsum(dx2) = fc2 bias gradient, published by the next block's LayerNorm backward
        b2_dst = _gout(p_f2b) if ready is not None else None
        # (q_bias and v_bias are two parameters: their gradients go to two destinations -- bucket views under GradSync, else pieces of the flat tensor --
        # instead of one [3D] vector that autograd would have to slice and GradSync to copy: 24 device-to-device copies per step, +1.0 ms)
        gd = _GradDest([(p_n1w, (D,)), (p_n1b, (D,)), (p_qkvw, (3 * D, D)), (p_qb, (D,)), (p_pw, (D, D)), (p_pb, (D,)), (p_n2w, (D,)), (p_n2b, (D,)),
                        (p_f1w, (hid, D)), (p_f1b, (hid,)), (p_f2w, (D, hid)), (None if ready is not None else p_f2b, (1,) if ready is not None else (D,)),
                        (None, (D,)), (p_vb, (D,))], dev)
        g = _L.BlockGrads()
        (g.dn1w, g.dn1b, g.dWqkv, g.dbq, g.dWp, g.dbp, g.dn2w, g.dn2b, g.dW1, g.db1, g.dW2, g.db2, g.dx_colsum, g.dbv) = gd.ptrs()
        g.db2_done = 1 if ready is not None else 0
        ops.attach_workspace(a, a.ws_bytes, dev)
        nscr = lib.devias_encoder_block_scratch_bytes(B, N, D, H, hid, a.dtype)
        scr = _scratch(nscr, dev)
        dx = torch.empty_like(x)
        # the weight gradients the queue takes (ops.wgrad_defer_mask): the block skips them and writes dhpre | dqkv | dx1 to a retention buffer instead of its scratch
        M = B * N
        defer = ops.wgrad_defer_mask((p_f2w, p_f1w, p_pw, p_qkvw), cdt, M, D, hid, True)
        kept = None
        if defer:
            es, al = x.element_size(), lambda n: (n + 255) // 256 * 256          # noqa: E731
            nds = int(ds1 is not None) + int(ds2 is not None)          # stochastic depth: the rescaled branch gradients are operands too
            kept = ops.keep_buffer(al(M * hid * es) + al(M * 3 * D * es) + (1 + nds) * al(M * D * es), dev)
            a.defer_wgrad = defer
            a.keep_dhpre = kept.data_ptr()
            a.keep_dqkv = a.keep_dhpre + al(M * hid * es)
            a.keep_dx1 = a.keep_dqkv + al(M * 3 * D * es)
            nxt = a.keep_dx1 + al(M * D * es)
            if ds2 is not None:
                a.keep_g2, nxt = nxt, nxt + al(M * D * es)
            if ds1 is not None:
                a.keep_g1 = nxt
        _L.check(lib.devias_encoder_block_bwd(_ct.byref(a), x.data_ptr(), dx2.data_ptr(), dx.data_ptr(), _ct.byref(g), scr.data_ptr(), scr.numel(), ops._stream()),
                 "devias_encoder_block_bwd")
        if defer:
            jobs = (_L.WgradJob * 4)()
            _L.check(lib.devias_encoder_block_wgrad_operands(_ct.byref(a), dx2.data_ptr(), _ct.byref(g), jobs), "devias_encoder_block_wgrad_operands")
            ops.wgrad_enqueue([_L.WgradJob.from_buffer_copy(jobs[i]) for i in range(4) if defer >> i & 1], (dx2, save, [gd.out[i].untyped_storage() for i in (10, 8, 4, 2)]), dev, lent=kept)      # (storages, not tensors: the OBJECTS handed to autograd must stay unshared, see _gout)
        ctx.keep = ctx.args = None
        (dn1w, dn1b, dWqkv, dbq, dWp, dbp, dn2w, dn2b, dW1, db1, dW2, db2, dxs, dbv) = gd.out
        if ready is not None:
            db2 = ready if b2_dst is None else b2_dst.copy_(ready)
        _publish_colsum(dx, dxs)
        return (dx, dn1w, dn1b, dWqkv, dbq, dbv, dWp, dbp, dn2w, dn2b, dW1, db1, dW2, db2, None, None, None)


class HeadRegionFn(Function):
    """HeadFn as one devias_head_fwd / _bwd call"""

    @staticmethod
    def forward(ctx, slots, hw, hb, w0, b0, w2, b2, w4, b4, cdt, drop_mask=None):
        lib = _L.load()
        dev = slots.device
        slots = slots.contiguous()
        R, D = slots.shape
        C, h1, h2, G = hw.shape[0], w0.shape[0], w2.shape[0], w4.shape[0]
        dt = ops.dt_code(cdt)
        keep = [_WCACHE.get(w, cdt) for w in (hw, w0, w2, w4)] + [_f32(hb), _f32(b0), _f32(b2), _f32(b4)]
        a = _L.HeadArgs()
        a.R, a.D, a.C, a.h1, a.h2, a.G, a.dtype = R, D, C, h1, h2, G, dt
        (a.Wh, a.W0, a.W2, a.W4, a.bh, a.b0, a.b2, a.b4) = [t.data_ptr() for t in keep]
        ops.attach_workspace(a, lib.devias_head_workspace_bytes(R, D, C, h1, h2, G, dt), dev)
        if drop_mask is not None:            # fc_dropout (modeling_slot.py:291,393): 0 / (1/keep) per element of the head's input
            drop_mask = ops._chk(drop_mask, "head.drop_mask", torch.float32)
            assert drop_mask.shape == (R, D)
            a.drop_mask = drop_mask.data_ptr()
        save = torch.empty((lib.devias_head_save_bytes(R, D, h1, h2, dt),), dtype=torch.uint8, device=dev)
        Z = torch.empty((R, C), dtype=cdt, device=dev)
        Mk = torch.empty((R, G), dtype=cdt, device=dev)
        _L.check(lib.devias_head_fwd(_ct.byref(a), slots.data_ptr(), Z.data_ptr(), Mk.data_ptr(), save.data_ptr(), ops._stream()), "devias_head_fwd")
        ctx.args = a
        ctx.keep = (keep, save, slots, Mk, drop_mask)
        ctx.x_version = slots._version
        ctx.params = (hw, hb, w0, b0, w2, b2, w4, b4)
        return Z, Mk

    @staticmethod
    def backward(ctx, dZ, dM):
        lib = _L.load()
        _region_state(ctx, "HeadRegionFn", 2)
        a = ctx.args
        keep, save, slots, Mk, drop_mask = ctx.keep
        hw, hb, w0, b0, w2, b2, w4, b4 = ctx.params
        dev = slots.device
        dZ = dZ.contiguous() if dZ is not None else torch.zeros((a.R, a.C), dtype=slots.dtype, device=dev)
        dM = dM.contiguous() if dM is not None else torch.zeros_like(Mk)
        gd = _GradDest([(hw, tuple(hw.shape)), (hb, tuple(hb.shape)), (w0, tuple(w0.shape)), (b0, tuple(b0.shape)), (w2, tuple(w2.shape)), (b2, tuple(b2.shape)),
                        (w4, tuple(w4.shape)), (b4, tuple(b4.shape))], dev)
        g = _L.HeadGrads()
        (g.dWh, g.dbh, g.dW0, g.db0, g.dW2, g.db2, g.dW4, g.db4) = gd.ptrs()
        ops.attach_workspace(a, a.ws_bytes, dev)
        dslots = torch.empty_like(slots)
        _L.check(lib.devias_head_bwd(_ct.byref(a), slots.data_ptr(), Mk.data_ptr(), save.data_ptr(), dZ.data_ptr(), dM.data_ptr(), dslots.data_ptr(),
                                     _ct.byref(g), ops._stream()), "devias_head_bwd")
        ctx.keep = ctx.args = None
        return (dslots, *gd.out, None, None)


class FusionHeadFn(Function):
    """Everything after the slots of the slot-fusion classifier (model/modeling_slot_fusion.py:379-400, MLPHead :42-53) as one devias_fusion_head_fwd / _bwd call:
    slots [B*S, D] -> (input [B, 2D], out [B, Cd], idx int32 [B, 2]).  The pre-trained head (hw, hb) only selects and gets no gradient; drop_mask: optional fp32
    [B, D] of 0 / (1 / keep), fc_dropout on relu(h).  meta's last entry is the caller's torch.is_grad_enabled(), read BEFORE apply (inside forward autograd is
    always off, and needs_input_grad reports requires_grad whatever the mode): where it is False, or no input requires a gradient, nothing is saved -- no arena, and
    the library keeps u, r and the statistics in its workspace (devias_fusion_head_fwd with save = NULL; same bits)."""

    @staticmethod
    def forward(ctx, slots, hw, hb, an_w, an_b, sn_w, sn_b, dw, db, lw, lb, iw, ib, cw, cb, meta, drop_mask=None):
        B, S, nb, eps_norm, eps_ln, cdt, grad_enabled = meta
        lib = _L.load()
        dev = slots.device
        slots = slots.contiguous()
        R, D = slots.shape
        Cd, C = cw.shape[0], hw.shape[0]
        assert R == B * S and dw.shape == (D // 2, D) and cw.shape[1] == D and hw.shape[1] == D
        dt = ops.dt_code(cdt)
        mats = [_WCACHE.get(w, cdt) for w in (hw, dw, cw)]
        vecs = [_f32(t) for t in (hb, an_w, an_b, sn_w, sn_b, db, lw, lb)] + [(_f32(t) if t is not None else None) for t in (iw, ib)] + [_f32(cb)]
        a = _L.FusionArgs()
        a.struct_size = _ct.sizeof(_L.FusionArgs)
        a.B, a.S, a.D, a.nb, a.ns, a.Cd, a.dtype, a.use_input_ln = B, S, D, nb, C - nb, Cd, dt, int(iw is not None)
        a.eps_norm, a.eps_ln = eps_norm, eps_ln
        (a.Wh, a.Wd, a.Wc) = [t.data_ptr() for t in mats]
        (a.bh, a.an_w, a.an_b, a.sn_w, a.sn_b, a.bd, a.ln_w, a.ln_b, a.in_w, a.in_b, a.bc) = [(t.data_ptr() if t is not None else None) for t in vecs]
        if drop_mask is not None:
            drop_mask = ops._chk(drop_mask, "fusion_head.drop_mask", torch.float32)
            assert drop_mask.shape == (B, D)
            a.drop_mask = drop_mask.data_ptr()
        nws = lib.devias_fusion_head_workspace_bytes(B, S, D, C, Cd, dt)
        if nws <= 0:
            raise NotImplementedError(f"devias_fusion_head: unsupported dims B={B} S={S} D={D} C={C} Cd={Cd} (D in 384 / 768 / 1024, S <= 4, Cd >= 2)")
        ops.attach_workspace(a, nws, dev)
        need_bwd = _will_backward(ctx, grad_enabled)
        save = torch.empty((lib.devias_fusion_head_save_bytes(B, D, dt),), dtype=torch.uint8, device=dev) if need_bwd else None
        inp = torch.empty((B, 2 * D), dtype=cdt, device=dev)
        out = torch.empty((B, Cd), dtype=cdt, device=dev)
        idx = torch.empty((B, 2), dtype=torch.int32, device=dev)
        _L.check(lib.devias_fusion_head_fwd(_ct.byref(a), slots.data_ptr(), inp.data_ptr(), out.data_ptr(), idx.data_ptr(), save.data_ptr() if save is not None else None,
                                            ops._stream()), "devias_fusion_head_fwd")
        ctx.mark_non_differentiable(idx)
        if need_bwd:
            ctx.args = a
            ctx.keep = (mats + vecs, save, slots, inp, idx, drop_mask)
            ctx.x_version = slots._version
            ctx.params = (an_w, an_b, sn_w, sn_b, dw, db, lw, lb, iw, ib, cw, cb)
        return inp, out, idx

    @staticmethod
    def backward(ctx, dinp, dout, _didx):
        lib = _L.load()
        _region_state(ctx, "FusionHeadFn", 2)
        a = ctx.args
        keep, save, slots, inp, idx, drop_mask = ctx.keep
        an_w, an_b, sn_w, sn_b, dw, db, lw, lb, iw, ib, cw, cb = ctx.params
        dev = slots.device
        dout = dout.contiguous() if dout is not None else torch.zeros((a.B, a.Cd), dtype=slots.dtype, device=dev)
        dinp = dinp.contiguous() if dinp is not None else None
        live = [p for p in (an_w, an_b, sn_w, sn_b, dw, db, lw, lb, iw, ib, cw, cb)]
        gd = _GradDest([(p, tuple(p.shape)) for p in live if p is not None], dev)
        it = iter(gd.out)
        outs = [(next(it) if p is not None else None) for p in live]
        g = _L.FusionGrads()
        g.struct_size = _ct.sizeof(_L.FusionGrads)
        (g.dan_w, g.dan_b, g.dsn_w, g.dsn_b, g.dWd, g.dbd, g.dln_w, g.dln_b, g.din_w, g.din_b, g.dWc, g.dbc) = [(t.data_ptr() if t is not None else None) for t in outs]
        ops.attach_workspace(a, a.ws_bytes, dev)
        dslots = torch.empty_like(slots)
        _L.check(lib.devias_fusion_head_bwd(_ct.byref(a), slots.data_ptr(), idx.data_ptr(), inp.data_ptr(), save.data_ptr(), dout.data_ptr(),
                                            dinp.data_ptr() if dinp is not None else None, dslots.data_ptr(), _ct.byref(g), ops._stream()), "devias_fusion_head_bwd")
        ctx.keep = ctx.args = None
        return (dslots, None, None, *outs, None, None)


class PoolHeadRegionFn(Function):
    """The plain video ViT's part after the encoder (model/modeling_finetune.py:314-325) as one devias_pool_head_fwd / _bwd call: h [B*Nt, D] ->
    (token [B, D], logits [B, C]).  meta = (B, Nt, pool, eps, cdt, grad_enabled): pool is _lib.POOL_MEAN (fc_norm(x.mean(1)); ln_w / ln_b are fc_norm's) or
    _lib.POOL_CLS (norm(x)[:, 0]; ln_w / ln_b are norm's); grad_enabled is the caller's torch.is_grad_enabled(), read BEFORE apply (see FusionHeadFn): where it is
    False, or no input requires a gradient, nothing is saved (devias_pool_head_fwd with save = NULL; same bits).  drop_mask: optional fp32 [B, D] of 0 / (1 / keep),
    fc_dropout on the token."""

    @staticmethod
    def forward(ctx, h, ln_w, ln_b, hw, hb, meta, drop_mask=None):
        B, Nt, pool, eps, cdt, grad_enabled = meta
        h = h.contiguous()
        keep = [_WCACHE.get(hw, cdt), _f32(hb), _f32(ln_w), _f32(ln_b)]
        a = ops.pool_head_args(B, Nt, pool, eps, *keep, drop_mask)
        need_bwd = _will_backward(ctx, grad_enabled)
        token, logits, save = ops.pool_head_fwd(a, h, save=need_bwd)
        if need_bwd:
            ctx.args = a
            ctx.keep = (keep, save, h, drop_mask)
            ctx.x_version = h._version
            ctx.params = (ln_w, ln_b, hw, hb)
        return token, logits

    @staticmethod
    def backward(ctx, dtoken, dlogits):
        _region_state(ctx, "PoolHeadRegionFn", 2)
        a = ctx.args
        keep, save, h, drop_mask = ctx.keep
        ln_w, ln_b, hw, hb = ctx.params
        dev = h.device
        dlogits = dlogits.contiguous() if dlogits is not None else torch.zeros((a.B, a.C), dtype=h.dtype, device=dev)
        dtoken = dtoken.contiguous() if dtoken is not None else None
        gd = _GradDest([(p, tuple(p.shape)) for p in (hw, hb, ln_w, ln_b)], dev)
        dx = torch.empty_like(h)
        ops.pool_head_bwd(a, save, dlogits, dtoken, dx, gd.out)
        ctx.keep = ctx.args = None
        dW, db, dlw, dlb = gd.out
        return (dx, dlw, dlb, dW, db, None, None)


class TwoTokenHeadRegionFn(Function):
    """The two-token multi-task baseline's part after the encoder (model/modeling_multi_task.py:318-334) as one devias_two_token_head_fwd / _bwd call: h [B*Nt, D] ->
    (token_a [B, D], logits_a [B, Ca], token_s [B, D], logits_s [B, Cs]) from rows 0 and Nt - 1 of each clip.  sw = sb = None is the unified head: both tokens go
    through (hw, hb) in one GEMM and the two logits are the halves of one [2B, Ca] tensor.  meta = (B, Nt, eps, cdt, grad_enabled): grad_enabled is the caller's
    torch.is_grad_enabled(), read BEFORE apply (see FusionHeadFn): where it is False, or no input requires a gradient, nothing is saved (save = NULL; same bits).
    mask_a / mask_s: optional fp32 [B, D] of 0 / (1 / keep), fc_dropout's two draws."""

    @staticmethod
    def forward(ctx, h, ln_w, ln_b, hw, hb, sw, sb, meta, mask_a=None, mask_s=None):
        B, Nt, eps, cdt, grad_enabled = meta
        h = h.contiguous()
        unified = sw is None
        keep = [_WCACHE.get(hw, cdt), _f32(hb), None if unified else _WCACHE.get(sw, cdt), None if unified else _f32(sb), _f32(ln_w), _f32(ln_b)]
        a = ops.two_token_head_args(B, Nt, eps, *keep, mask_a, mask_s)
        need_bwd = _will_backward(ctx, grad_enabled)
        token_a, token_s, logits_a, logits_s, save = ops.two_token_head_fwd(a, h, save=need_bwd)
        if need_bwd:
            ctx.args = a
            ctx.keep = (keep, save, h, mask_a, mask_s)
            ctx.x_version = h._version
            ctx.params = (ln_w, ln_b, hw, hb, sw, sb)
        return token_a, logits_a, token_s, logits_s

    @staticmethod
    def backward(ctx, dtoken_a, dlogits_a, dtoken_s, dlogits_s):
        _region_state(ctx, "TwoTokenHeadRegionFn", 2)
        a = ctx.args
        keep, save, h, mask_a, mask_s = ctx.keep
        ln_w, ln_b, hw, hb, sw, sb = ctx.params
        dev = h.device

        def ready(t, shape):          # a contiguous, 16-byte aligned tensor (a GEMM operand); zeros where autograd sent nothing
            if t is None:
                return torch.zeros(shape, dtype=h.dtype, device=dev)
            t = t.contiguous()
            return t.clone() if t.data_ptr() % 16 else t

        dlogits_a, dlogits_s = ready(dlogits_a, (a.B, a.Ca)), ready(dlogits_s, (a.B, a.Cs))
        dtoken_a = dtoken_a.contiguous() if dtoken_a is not None else None
        dtoken_s = dtoken_s.contiguous() if dtoken_s is not None else None
        live = (hw, hb, sw, sb, ln_w, ln_b)
        gd = _GradDest([(p, tuple(p.shape)) for p in live if p is not None], dev)
        it = iter(gd.out)
        dW, db, dWs, dbs, dlw, dlb = [(next(it) if p is not None else None) for p in live]
        dx = torch.empty_like(h)
        ops.two_token_head_bwd(a, save, dlogits_a, dlogits_s, dtoken_a, dtoken_s, dx, (dW, db, dWs, dbs, dlw, dlb))
        ctx.keep = ctx.args = None
        return (dx, dlw, dlb, dW, db, dWs, dbs, None, None, None)


_AGG_MATS = ("to_q", "to_k", "to_v", "to_out_w", "ff0_w", "ff3_w")                      # -> devias_agg_layer_params.Wq Wk Wv Wo W1 W2
_AGG_VECS = ("to_out_b", "norm_w", "norm_b", "ctx_w", "ctx_b", "ff0_b", "ff3_b", "ffn_w", "ffn_b")   # -> bo norm_w norm_b ctx_w ctx_b b1 b2 ffn_w ffn_b
# (devias_agg_layer_grads -- dWq dWk dWv dWo dbo dnorm_w dnorm_b dctx_w dctx_b dW1 db1 dW2 db2 dffn_w dffn_b -- is in _LAYER_KEYS order)


class AggBlockRegionFn(Function):
    """AggBlockFoldFn as one devias_agg_block_fwd / _bwd call"""

    @staticmethod
    def forward(ctx, x, norm_w, norm_b, latents, last_w, last_b, meta, *layer_params):
        B, N, S, depth, tied, heads, dh, eps_enc, eps_agg, cdt = meta
        lib = _L.load()
        dev = x.device
        x = x.contiguous()
        D = x.shape[1]
        nset = 1 if tied else depth
        assert depth <= _L.AGG_MAX_DEPTH
        LP = _weight_sets(layer_params, nset)
        dt = ops.dt_code(cdt)
        a = _L.AggArgs()
        a.B, a.N, a.S, a.D, a.depth, a.tied, a.heads, a.dh, a.ff, a.dtype = B, N, S, D, depth, int(bool(tied)), heads, dh, LP[0]["ff0_w"].shape[0], dt
        a.eps_enc, a.eps_agg = eps_enc, eps_agg
        keep = [_f32(norm_w), _f32(norm_b), _f32(latents), _f32(last_w), _f32(last_b)]
        (a.norm_w, a.norm_b, a.latents, a.last_w, a.last_b) = [t.data_ptr() for t in keep]
        for i, P in enumerate(LP):
            mats = [_WCACHE.get(P[k], cdt) for k in _AGG_MATS]
            vecs = [_f32(P[k]) for k in _AGG_VECS]
            keep += mats + vecs
            for f, t in zip(_L.AGG_PARAM_FIELDS, mats + vecs):
                setattr(a.sets[i], f, t.data_ptr())
        save = torch.empty((lib.devias_agg_block_save_bytes(_ct.byref(a)),), dtype=torch.uint8, device=dev)
        a.save = save.data_ptr()
        ops.attach_workspace(a, lib.devias_agg_block_workspace_bytes(_ct.byref(a)), dev)
        slots = torch.empty((B * S, D), dtype=cdt, device=dev)
        attn_ptr = _ct.c_void_p()
        _L.check(lib.devias_agg_block_fwd(_ct.byref(a), x.data_ptr(), slots.data_ptr(), _ct.byref(attn_ptr), ops._stream()), "devias_agg_block_fwd")
        off = attn_ptr.value - save.data_ptr()
        # the last layer's slot softmax is a VIEW of the arena (no copy of 2.4 MB per step): whoever keeps `attn` alive keeps the whole arena alive,
        # and it is overwritten by nothing (an arena belongs to one forward); clone it to hold it beyond the step
        attn = save[off:off + B * heads * S * N * 4].view(torch.float32).view(B * heads, S, N)
        ctx.args = a
        ctx.meta = meta
        ctx.keep = (keep, save, x)
        ctx.x_version = x._version
        ctx.params = (norm_w, norm_b, latents, last_w, last_b, LP)
        return slots, attn

    @staticmethod
    def backward(ctx, dslots, dattn):
        B, N, S, depth, tied, heads, dh, eps_enc, eps_agg, cdt = ctx.meta
        lib = _L.load()
        _region_state(ctx, "AggBlockRegionFn", 2)
        a = ctx.args
        keep, save, x = ctx.keep
        norm_w, norm_b, latents, last_w, last_b, LP = ctx.params
        dev = x.device
        D = a.D
        nset = 1 if tied else depth
        items = [(norm_w, (D,)), (norm_b, (D,)), (latents, tuple(latents.shape)), (last_w, (D,)), (last_b, (D,)), (None, (D,))]
        for P in LP:
            items += [(P[k], tuple(P[k].shape)) for k in _LAYER_KEYS]
        gd = _GradDest(items, dev)
        ptrs = gd.ptrs()
        g = _L.AggGrads()
        (g.dnorm_w, g.dnorm_b, g.dlatents, g.dlast_w, g.dlast_b, g.dx_colsum) = ptrs[:6]
        nk = len(_LAYER_KEYS)
        for i in range(nset):
            for f, ptr in zip(_L.AGG_GRAD_FIELDS, ptrs[6 + nk * i:6 + nk * (i + 1)]):
                setattr(g.sets[i], f, ptr)
        ops.attach_workspace(a, a.ws_bytes, dev)
        scr = _scratch(lib.devias_agg_block_scratch_bytes(_ct.byref(a)), dev)
        dslots = dslots.contiguous()
        dattn = dattn.contiguous() if dattn is not None else None
        dx = torch.empty_like(x)
        _L.check(lib.devias_agg_block_bwd(_ct.byref(a), x.data_ptr(), dslots.data_ptr(), dattn.data_ptr() if dattn is not None else None, dx.data_ptr(),
                                          _ct.byref(g), scr.data_ptr(), scr.numel(), ops._stream()), "devias_agg_block_bwd")
        ctx.keep = ctx.args = None
        out = gd.out
        _publish_colsum(dx, out[5])
        return (dx, out[0], out[1], out[2], out[3], out[4], None, *out[6:])
