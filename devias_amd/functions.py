"""The per-kernel autograd Functions of the slot-DEVIAS student: forward and hand-written backward of each part of the model as a sequence of
library calls (devias_amd.ops), one kernel per call.

    PatchEmbedFn   tubelet im2col -> GEMM(+bias +sinusoid pos)                       (modeling_slot.py:171-177, :354-355)
    EncoderBlockFn LN -> QKV GEMM -> flash MHSA -> proj GEMM(+res) -> LN -> fc1 GEMM(+GELU) -> fc2 GEMM(+res)   (:142-152)
    AggBlockFn     final LN -> [context LN -> K|V GEMM once per distinct weight set] -> depth x slot layer -> LN
    AggBlockFoldFn (the same with the folded slot attention)   (agg_block/agg_block.py:120-139, agg_block/attention.py:32-40,120-141)
    HeadFn         shared head GEMM + MaskPredictor MLP (ReLU/ReLU/Sigmoid epilogues)     (modeling_slot.py:392-393, :209-216)
    HeadMlpFn      the same behind the reference's MLPHead

devias_amd.regions runs the encoder block, the folded aggregation block and the head as ONE library call per direction; this module also holds the
gradient plumbing both share: the column-sum tags that travel on gradient tensors, the gradient-bucket destinations, the weight sets of the
aggregation block.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch.autograd import Function

from . import ops
from .ops import ACT_DGELU, ACT_DRELU, ACT_GELU, ACT_RELU, ACT_SIGMOID
from .weight_cache import _Q_PRESCALE, _WCACHE, _f32, _use_q_prescale

# column sums of a residual-stream gradient, produced for free by the LayerNorm-backward kernel that wrote it and consumed by the
# next backward region as the bias gradient of its last Linear.  The sum travels ON the gradient tensor object (autograd hands the
# same object to the next node when there is a single consumer) together with the tensor's storage address and VERSION COUNTER at the
# time of publication.  Two ways the sum could go stale are both caught: autograd builds a new tensor (hooks, out-of-place
# accumulation): the attribute is absent; autograd accumulates a second consumer's gradient IN PLACE into the tagged tensor
# (InputBuffer does that when the residual stream feeds two consumers): `_version` has moved.  In both cases the sum is recomputed.
_COLSUM_STATS = {"hit": 0, "miss": 0}


def _publish_colsum(dx: torch.Tensor, cs: torch.Tensor) -> None:
    dx._devias_colsum = (cs, dx.data_ptr(), dx._version)


def _peek_colsum(dy: torch.Tensor) -> Optional[torch.Tensor]:
    """the published column sums of `dy` if they are still those of its current contents, else None (the tag is consumed either way)"""
    tag = getattr(dy, "_devias_colsum", None)
    if tag is None:
        _COLSUM_STATS["miss"] += 1
        return None
    del dy._devias_colsum
    cs, ptr, ver = tag
    if ptr == dy.data_ptr() and ver == dy._version and cs.numel() == dy.shape[1] and cs.device == dy.device:
        _COLSUM_STATS["hit"] += 1
        return cs
    _COLSUM_STATS["miss"] += 1
    return None


def _take_colsum(dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    cs = _peek_colsum(dy)
    if cs is not None:
        if out is not None:
            out.copy_(cs)
            return out
        return cs
    return ops.colsum(dy, out=out)


# ---- gradient destinations ---------------------------------------------------------------------------------------------------------
# A data-parallel gradient bucket (devias_amd.parallel.GradSync) registers, on every parameter, the fp32 view of its flat bucket
# (`_devias_grad_out`).  When the parameter has no gradient yet, the weight-gradient kernels write straight into that view and a FRESH
# alias of it is returned to autograd: AccumulateGrad adopts a gradient tensor without copying only when nobody else holds a reference to
# that tensor object (the registered view is held by GradSync and by the parameter attribute, so returning it would be cloned -- ADVICE r2).
# A bucket is then complete the moment its last kernel finishes (no pack pass, no copy).
def _gout(p: Optional[torch.Tensor], shape=None) -> Optional[torch.Tensor]:
    if p is None or p.grad is not None:
        return None                                   # accumulation (update_freq > 1, tied uses): autograd adds a fresh tensor in place
    v = getattr(p, "_devias_grad_out", None)
    if v is None:
        return None
    if v.device != p.device:
        raise RuntimeError("gradient bucket and parameter live on different devices: build GradSync AFTER model.to(device)")
    return v.view(v.shape if shape is None else shape)


# =====================================================================================================
# autograd Functions (forward and hand-written backward over the C ABI)
# =====================================================================================================
class PatchEmbedFn(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, pos, meta):
        ts, ps, cdt = meta
        A = ops.patch_im2col(x, ts, ps, cdt)                          # [B*N, C*ts*ps*ps]
        w = _WCACHE.get(weight, cdt)
        y = ops.gemm(A, w, bias=_f32(bias), res=pos, res_mod=pos.shape[0])
        ctx.A = A
        ctx.params = (weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        weight, bias = ctx.params
        dW = ops.wgrad(dy, ctx.A, out=_gout(weight, (weight.shape[0], -1))).view(weight.shape)
        db = _take_colsum(dy, out=_gout(bias))
        ctx.A = None
        return None, dW, db, None, None


class EncoderBlockFn(Function):
    """x -> x + proj(MHSA(LN1 x)) -> + fc2(GELU(fc1(LN2 .)))   (Block.forward, modeling_slot.py:142-152; no LayerScale, drop_path 0)"""

    @staticmethod
    def forward(ctx, x, n1w, n1b, qkvw, qb, vb, pw, pb, n2w, n2b, f1w, f1b, f2w, f2b, meta, ds1=None, ds2=None, drop=None):
        """drop = (E1, E2, attn): training with drop_rate / attn_drop_rate > 0 (modeling_slot.py:110,114,66).  E1 / E2: fp32 [M, D] element masks of
        proj_drop / Mlp.drop, each 0 or 1 / keep and already carrying the branch's per-sample drop_path factor (then ds1 / ds2 are None); attn =
        (keep, seed) of the softmax-matrix dropout (ops.mhsa_fwd) or None."""
        B, N, H, eps, cdt = meta
        scale = 64 ** -0.5
        E1, E2, adrop = drop if drop is not None else (None, None, None)
        assert (E1 is None) == (E2 is None) and (E1 is None or (ds1 is None and ds2 is None))
        n1w_, n1b_, n2w_, n2b_ = _f32(n1w), _f32(n1b), _f32(n2w), _f32(n2b)
        Wqkv, Wp, W1, W2 = (_WCACHE.get(w, cdt) for w in (qkvw, pw, f1w, f2w))
        u, mean1, rstd1 = ops.layernorm_fwd(x, n1w_, n1b_, eps)
        qkv_bias = _WCACHE.qkv_bias(qb, vb)                                             # q_bias | 0 | v_bias (modeling_slot.py:97-99)
        qpre = _use_q_prescale(cdt, adrop)               # q' = q * scale * log2(e) straight from the GEMM (a weight / bias copy whose q third carries the factor): see _use_q_prescale
        if qpre:
            D = x.shape[1]
            qkv = ops.gemm(u, _WCACHE.get_qscaled(qkvw, D, _Q_PRESCALE, cdt), bias=_WCACHE.get_qscaled(qkv_bias, D, _Q_PRESCALE, torch.float32))
        else:
            qkv = ops.gemm(u, Wqkv, bias=qkv_bias)                                      # [M, 3D] == [B,N,3,H,64]
        o, lse = ops.mhsa_fwd(qkv, B, N, H, scale, drop=adrop, q_prescaled=qpre)
        if E1 is None:
            x1 = ops.gemm(o, Wp, bias=_f32(pb), res=x, row_scale=ds1, rows_per_scale=N)   # x + drop_path(proj(.))
        else:
            x1 = ops.mul_mask(ops.gemm(o, Wp, bias=_f32(pb)), E1, x)                      # x + drop_path(proj_drop(proj(.)))
        u2, mean2, rstd2 = ops.layernorm_fwd(x1, n2w_, n2b_, eps)
        hpre = torch.empty((x.shape[0], W1.shape[0]), dtype=cdt, device=x.device)
        hact = ops.gemm(u2, W1, bias=_f32(f1b), act=ACT_GELU, aux_out=hpre)
        if E2 is None:
            x2 = ops.gemm(hact, W2, bias=_f32(f2b), res=x1, row_scale=ds2, rows_per_scale=N)   # x1 + drop_path(mlp(.))
        else:
            x2 = ops.mul_mask(ops.gemm(hact, W2, bias=_f32(f2b)), E2, x1)                 # x1 + drop_path(drop(fc2(.)))
        ctx.meta = meta
        ctx.drop = (E1, E2, adrop)
        ctx.qpre = qpre
        ctx.ds = (ds1, ds2)
        ctx.params = (n1w, n1b, qkvw, pw, pb, n2w, n2b, f1w, f1b, f2w, f2b, qb, vb)
        ctx.saved = (x, u, mean1, rstd1, qkv, o, lse, x1, u2, mean2, rstd2, hpre, hact, n1w_, n2w_, Wqkv, Wp, W1, W2)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        B, N, H, eps, cdt = ctx.meta
        scale = 64 ** -0.5
        (x, u, mean1, rstd1, qkv, o, lse, x1, u2, mean2, rstd2, hpre, hact, n1w_, n2w_, Wqkv, Wp, W1, W2) = ctx.saved
        ctx.saved = None
        dx2 = dx2.contiguous()
        D = x.shape[1]
        dev = x.device
        ds1, ds2 = ctx.ds
        E1, E2, adrop = ctx.drop
        (p_n1w, p_n1b, p_qkvw, p_pw, p_pb, p_n2w, p_n2b, p_f1w, p_f1b, p_f2w, p_f2b, p_qb, p_vb) = ctx.params
        f32 = lambda n: torch.empty((n,), dtype=torch.float32, device=dev)          # noqa: E731
        dst = lambda p_, n: _gout(p_) if _gout(p_) is not None else f32(n)          # noqa: E731  (gradient bucket view, or a fresh buffer)
        # ---- MLP branch (g2 = gradient of the branch output: dx2 scaled by the per-sample stochastic-depth factor, if any)
        if E2 is not None:
            g2 = ops.mul_mask(dx2, E2)
            db2 = ops.colsum(g2, out=_gout(p_f2b))
        elif ds2 is None:
            g2, db2 = dx2, _take_colsum(dx2, out=_gout(p_f2b))                          # fc2 bias gradient
        else:
            g2 = ops.row_scale(dx2, ds2, N)
            db2 = ops.colsum(g2, out=_gout(p_f2b))
        # the weight gradients the queue takes (ops.wgrad_defer_mask; the same jobs in the same order as the fused region's): destination now, product at the flush
        defer = ops.wgrad_defer_mask((p_f2w, p_f1w, p_pw, p_qkvw), cdt, x.shape[0], D, W1.shape[0], E1 is None and E2 is None)
        jobs = []

        def wgrad(i, dY, X, p_):
            if not defer >> i & 1:
                return ops.wgrad(dY, X, out=_gout(p_))
            dW = _gout(p_)
            if dW is None:
                dW = torch.empty((dY.shape[1], X.shape[1]), dtype=torch.float32, device=dev)
            jobs.append((ops.wgrad_job(dY, X, dW), dY, (X, dW.untyped_storage())))      # (the queue keeps dW's STORAGE: the object handed to autograd must stay unshared -- even a view of it would hold it --, see _gout)
            return dW
        dW2 = wgrad(0, g2, hact, p_f2w)
        db1 = dst(p_f1b, W1.shape[0])
        dhpre = ops.gemm(g2, W2, trans_b=True, act=ACT_DGELU, aux_in=hpre, colsum=db1)   # (g2 W2) * gelu'(pre); db1 = colsum
        dW1 = wgrad(1, dhpre, u2, p_f1w)
        du2 = ops.gemm(dhpre, W1, trans_b=True)
        dbp = dst(p_pb, D)
        dx1, dn2w, dn2b = ops.layernorm_bwd(du2, x1, n2w_, mean2, rstd2, dres=dx2, dx_colsum=dbp,
                                            dgamma=_gout(p_n2w), dbeta=_gout(p_n2b))      # + residual gradient; dbp = colsum(dx1)
        # ---- attention branch
        if E1 is not None:
            g1 = ops.mul_mask(dx1, E1)
            dbp = ops.colsum(g1, out=dbp)
        elif ds1 is None:
            g1 = dx1
        else:
            g1 = ops.row_scale(dx1, ds1, N)
            dbp = ops.colsum(g1, out=dbp)
        dWp = wgrad(2, g1, o, p_pw)
        dbq, dbv = dst(p_qb, D), dst(p_vb, D)                                  # q_bias | (k: no bias) | v_bias, each to its own destination
        if ops.mhsa_bwd_dv_from_do(g1.dtype, adrop):
            # softmax rows sum to one: sum_keys dV = sum_queries dO -- the v_bias gradient is the column sum of d_o, taken from the GEMM that produces it
            d_o = ops.gemm(g1, Wp, trans_b=True, colsum=dbv)
            dqkv = ops.mhsa_bwd(qkv, o, d_o, lse, B, N, H, scale, drop=adrop, bias_out=(dbq, None), q_prescaled=ctx.qpre)
        else:
            d_o = ops.gemm(g1, Wp, trans_b=True)
            dqkv = ops.mhsa_bwd(qkv, o, d_o, lse, B, N, H, scale, drop=adrop, bias_out=(dbq, dbv), q_prescaled=ctx.qpre)
        dWqkv = wgrad(3, dqkv, u, p_qkvw)
        du = ops.gemm(dqkv, Wqkv, trans_b=True)
        dxs = f32(D)
        dx, dn1w, dn1b = ops.layernorm_bwd(du, x, n1w_, mean1, rstd1, dres=dx1, dx_colsum=dxs, dgamma=_gout(p_n1w), dbeta=_gout(p_n1b))
        _publish_colsum(dx, dxs)
        if jobs:
            ops.wgrad_enqueue([j for j, _, _ in jobs], [(dY, X) for _, dY, X in jobs], dev)
        return (dx, dn1w, dn1b, dWqkv, dbq, dbv, dWp, dbp, dn2w, dn2b, dW1, db1, dW2, db2, None, None, None, None)


class DropMaskFn(Function):
    """y = x * mask with a caller-drawn fp32 mask of 0 / (1 / keep): nn.Dropout with its mask made explicit (pos_drop, modeling_slot.py:280,356)"""

    @staticmethod
    def forward(ctx, x, mask):
        ctx.mask = mask
        return ops.mul_mask(x, mask)

    @staticmethod
    def backward(ctx, dy):
        return ops.mul_mask(dy.contiguous(), ctx.mask), None


# =====================================================================================================
# aggregation block: one forward and one backward, two forms of the slot attention
# =====================================================================================================
_LAYER_KEYS = ("to_q", "to_k", "to_v", "to_out_w", "to_out_b", "norm_w", "norm_b", "ctx_w", "ctx_b",
               "ff0_w", "ff0_b", "ff3_w", "ff3_b", "ffn_w", "ffn_b")


def _weight_sets(layer_params, nset: int):
    """AggregationBlock.layer_params() as one {key: parameter} per distinct weight set (1 when the layers are tied, else one per layer)"""
    n = len(_LAYER_KEYS)
    assert len(layer_params) == nset * n
    return [dict(zip(_LAYER_KEYS, layer_params[i * n:(i + 1) * n])) for i in range(nset)]


# ---- folded aggregation block -------------------------------------------------------------------------------------------------------------
# sim = scale (Wk_h^T q) . c_j and o = Wv_h sum_j Abar c_j: the to_k / to_v projections move to the slot side (composite D x D weights per head,
# built once per forward), the per-layer stream is the context c [M, D] instead of K|V [M, 2*h*512], and the K|V GEMM + its dgrad + wgrad vanish
# (csrc/slot_valu.hip "folded form", csrc/slot_mfma.hip).  Same parameters, same outputs, same gradients; summation order differs (fp32 round-off).
def _composites(P, heads, dh, D, cdt):
    """Wqk [h*D, D] (Wqk_h = Wk_h^T Wq_h) and Wov [D, h*D] (Wov_h = Wo_h Wv_h) in the compute dtype, + the operands for their backward"""
    Wq, Wk, Wv, Wo = (_WCACHE.get(P[k], cdt) for k in ("to_q", "to_k", "to_v", "to_out_w"))
    inner = heads * dh
    Wqk = torch.empty((heads * D, D), dtype=cdt, device=Wq.device)
    ops.gemm_batched(Wk, Wq, Wqk, D, D, dh, lda=D, ldb=D, ldc=D, stride_a=dh * D, stride_b=dh * D, stride_c=D * D, batch=heads,
                     trans_a=True, trans_b=True)
    Wov = torch.empty((D, heads * D), dtype=cdt, device=Wq.device)
    ops.gemm_batched(Wo, Wv, Wov, D, D, dh, lda=inner, ldb=D, ldc=heads * D, stride_a=dh, stride_b=dh * D, stride_c=D, batch=heads,
                     trans_b=True)
    return Wqk, Wov, (Wq, Wk, Wv, Wo)


def _composite_grads(dWqk, dWov, W4, heads, dh, D, cdt):
    """gradients of to_q / to_k / to_v / to_out.weight (fp32) from those of the composites (fp32 accumulators over the layers)"""
    Wq, Wk, Wv, Wo = W4
    inner = heads * dh
    dev = Wq.device
    gqk = dWqk if cdt == torch.float32 else ops.cast(dWqk, cdt)
    gov = dWov if cdt == torch.float32 else ops.cast(dWov, cdt)
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
    dWq, dWk, dWv, dWo = f(inner, D), f(inner, D), f(inner, D), f(D, inner)
    ops.gemm_batched(Wk, gqk, dWq, dh, D, D, lda=D, ldb=D, ldc=D, stride_a=dh * D, stride_b=D * D, stride_c=dh * D, batch=heads, trans_b=True)
    ops.gemm_batched(Wq, gqk, dWk, dh, D, D, lda=D, ldb=D, ldc=D, stride_a=dh * D, stride_b=D * D, stride_c=dh * D, batch=heads)
    ops.gemm_batched(gov, Wv, dWo, D, dh, D, lda=heads * D, ldb=D, ldc=inner, stride_a=D, stride_b=dh * D, stride_c=dh, batch=heads)
    ops.gemm_batched(Wo, gov, dWv, dh, D, D, lda=inner, ldb=heads * D, ldc=D, stride_a=dh, stride_b=D, stride_c=dh * D, batch=heads,
                     trans_a=True, trans_b=True)
    return dWq, dWk, dWv, dWo


class _AggGeometry(NamedTuple):
    B: int
    S: int
    N: int
    heads: int
    dh: int
    D: int
    scale: float
    cdt: torch.dtype


# A form supplies the three places where the two formulations of the slot attention differ (`g`: _AggGeometry).
#   prepare(P, c, g)        once per weight set, after its context LayerNorm c: what the layers of that set share
#   weights(P, prep, cdt)   per layer: the weights of the query projection and of the output projection; KEY_Q / KEY_O name their gradient accumulators
#   attend / attend_bwd     per layer: the slot attention between the two projections; q_l / dq have WIDTH(g) columns
#   finish(G, ...)          once per weight set, over the layers [sl] that used it: the deferred gradient of the context c, and G's to_q / to_k / to_v / to_out_w
class _Unfolded:
    """the reference's formulation: K|V = c [Wk | Wv]^T once per weight set, attention over K and V (slot_attn_*)"""
    KEY_Q, KEY_O = "to_q", "to_out_w"

    @staticmethod
    def width(g):
        return g.heads * g.dh

    @staticmethod
    def prepare(P, c, g):
        Wkv = _WCACHE.get_cat((P["to_k"], P["to_v"]), g.cdt)
        return Wkv, ops.gemm(c, Wkv)                                                      # [M, 2*inner] == [B,N,2,h,dh]

    @staticmethod
    def weights(P, prep, cdt):
        return _WCACHE.get(P["to_q"], cdt), _WCACHE.get(P["to_out_w"], cdt)

    @staticmethod
    def attend(q_l, c, prep, g, attn_l, rsum_l):
        B, S, N, heads, dh, D, scale, cdt = g
        return ops.slot_attn_fwd(q_l, prep[1], B, S, N, heads, dh, scale, attn_out=attn_l, rsum_out=rsum_l)[2]

    @staticmethod
    def attend_bwd(q_l, c, prep, g, attn_l, rsum_l, o, d_o, dattn, ds_l):
        B, S, N, heads, dh, D, scale, cdt = g
        return ops.slot_attn_bwd(q_l, prep[1], attn_l, rsum_l, o, d_o, dattn, B, S, N, heads, dh, scale, ds_out=ds_l)[0]

    @staticmethod
    def finish(G, c, prep, g, q_stack, do_stack, ds_stack, attn_stack, rsum_stack, sl, nl):
        B, S, N, heads, dh, D, scale, cdt = g
        dkv = ops.slot_attn_kv_grad(q_stack[sl], do_stack[sl], ds_stack[sl], attn_stack[sl], rsum_stack[sl], nl, B, S, N, heads, dh, scale)
        dc = ops.gemm(dkv, prep[0], trans_b=True)
        dWkv = ops.wgrad(dkv, c)
        G["to_k"], G["to_v"] = dWkv[:heads * dh], dWkv[heads * dh:]
        return dc


class _Folded:
    """the folded formulation: composite weights once per weight set, attention over the context itself (slotf_*)"""
    KEY_Q, KEY_O = "Wqk", "Wov"

    @staticmethod
    def width(g):
        return g.heads * g.D

    @staticmethod
    def prepare(P, c, g):
        return _composites(P, g.heads, g.dh, g.D, g.cdt)

    @staticmethod
    def weights(P, prep, cdt):
        return prep[0], prep[1]

    @staticmethod
    def attend(q_l, c, prep, g, attn_l, rsum_l):
        B, S, N, heads, dh, D, scale, cdt = g
        return ops.slotf_fwd(q_l, c, B, S, N, heads, D, scale, attn_out=attn_l, rsum_out=rsum_l)[2]

    @staticmethod
    def attend_bwd(q_l, c, prep, g, attn_l, rsum_l, o, d_o, dattn, ds_l):
        B, S, N, heads, dh, D, scale, cdt = g
        return ops.slotf_bwd(c, attn_l, rsum_l, o, d_o, dattn, B, S, N, heads, D, scale, ds_out=ds_l)[0]

    @staticmethod
    def finish(G, c, prep, g, q_stack, do_stack, ds_stack, attn_stack, rsum_stack, sl, nl):
        B, S, N, heads, dh, D, scale, cdt = g
        dc = ops.slotf_context_grad(attn_stack[sl], rsum_stack[sl], ds_stack[sl], do_stack[sl], q_stack[sl], nl, B, S, N, heads, D, scale)
        G["to_q"], G["to_k"], G["to_v"], G["to_out_w"] = _composite_grads(G.pop("Wqk"), G.pop("Wov"), prep[2], heads, dh, D, cdt)
        return dc


def _agg_forward(form, ctx, x, norm_w, norm_b, latents, last_w, last_b, meta, *layer_params):
    B, N, S, depth, tied, heads, dh, eps_enc, eps_agg, cdt = meta
    LP = _weight_sets(layer_params, 1 if tied else depth)
    dev = x.device
    g = _AggGeometry(B, S, N, heads, dh, x.shape[1], dh ** -0.5, cdt)
    feats, m0, r0 = ops.layernorm_fwd(x, _f32(norm_w), _f32(norm_b), eps_enc)        # modeling_slot.py:373
    # context LayerNorm + what the form shares among the layers (fused K|V projection / composite weights), once per distinct weight set (the reference
    # redoes it every layer)
    sets = []
    for P in LP:
        c, mc, rc = ops.layernorm_fwd(feats, _f32(P["ctx_w"]), _f32(P["ctx_b"]), eps_agg)
        sets.append((c, mc, rc, form.prepare(P, c, g)))
    xs = ops.rows_broadcast(_f32(latents), B * S, cdt)                                # agg_block.py:112-114
    q_stack = torch.empty((depth, B * S, form.width(g)), dtype=cdt, device=dev)
    attn_stack = torch.empty((depth, B * heads, S, N), dtype=torch.float32, device=dev)
    rsum_stack = torch.empty((depth, B * heads, S), dtype=torch.float32, device=dev)
    layers = []
    for l in range(depth):
        si = 0 if tied else l
        P = LP[si]
        c, _, _, prep = sets[si]
        Wq, Wo = form.weights(P, prep, cdt)
        W1, W2 = (_WCACHE.get(P[k], cdt) for k in ("ff0_w", "ff3_w"))
        qn, mq, rq = ops.layernorm_fwd(xs, _f32(P["norm_w"]), _f32(P["norm_b"]), eps_agg)
        q = ops.gemm(qn, Wq, out=q_stack[l])
        o = form.attend(q, c, prep, g, attn_stack[l], rsum_stack[l])
        xs1 = ops.gemm(o, Wo, bias=_f32(P["to_out_b"]), res=xs)
        f, mf, rf = ops.layernorm_fwd(xs1, _f32(P["ffn_w"]), _f32(P["ffn_b"]), eps_agg)
        fpre = torch.empty((B * S, W1.shape[0]), dtype=cdt, device=dev)
        fact = ops.gemm(f, W1, bias=_f32(P["ff0_b"]), act=ACT_GELU, aux_out=fpre)
        xs2 = ops.gemm(fact, W2, bias=_f32(P["ff3_b"]), res=xs1)
        layers.append((xs, mq, rq, qn, o, xs1, mf, rf, f, fpre, fact, Wq, Wo, W1, W2))
        xs = xs2
    slots, ml, rl = ops.layernorm_fwd(xs, _f32(last_w), _f32(last_b), eps_agg)
    ctx.meta = meta
    ctx.saved = (x, m0, r0, feats, sets, layers, q_stack, attn_stack, rsum_stack, xs, ml, rl,
                 _f32(norm_w), _f32(last_w), [{k: _f32(P[k]) for k in ("norm_w", "ctx_w", "ffn_w")} for P in LP])
    return slots, attn_stack[depth - 1]


def _agg_backward(form, ctx, dslots, dattn):
    B, N, S, depth, tied, heads, dh, eps_enc, eps_agg, cdt = ctx.meta
    (x, m0, r0, feats, sets, layers, q_stack, attn_stack, rsum_stack, xs_last, ml, rl, norm_w, last_w, LNW) = ctx.saved
    ctx.saved = None
    nset = 1 if tied else depth
    dev = x.device
    g = _AggGeometry(B, S, N, heads, dh, x.shape[1], dh ** -0.5, cdt)
    G = [dict() for _ in range(nset)]        # gradient accumulators per distinct weight set

    def acc_w(si, key, dY, X):
        if key in G[si]:
            ops.wgrad(dY, X, out=G[si][key], beta=1.0)
        else:
            G[si][key] = ops.wgrad(dY, X)

    def acc_b(si, key, dY):
        if key in G[si]:
            ops.colsum(dY, out=G[si][key], beta=1.0)
        else:
            G[si][key] = ops.colsum(dY)

    def ln_bwd(si, kw, kb, dy, xin, gamma, mean, rstd, dres):
        if kw in G[si]:
            dxo, _, _ = ops.layernorm_bwd(dy, xin, gamma, mean, rstd, dres=dres, dgamma=G[si][kw], dbeta=G[si][kb], beta_acc=1.0)
        else:
            dxo, G[si][kw], G[si][kb] = ops.layernorm_bwd(dy, xin, gamma, mean, rstd, dres=dres)
        return dxo

    dxs, dlast_w, dlast_b = ops.layernorm_bwd(dslots.contiguous(), xs_last, last_w, ml, rl)
    do_stack = torch.empty((depth, B * S, form.width(g)), dtype=cdt, device=dev)
    ds_stack = torch.empty((depth, B * heads, S, N), dtype=torch.float32, device=dev)
    dattn_ext = dattn.contiguous() if dattn is not None else None
    for l in reversed(range(depth)):
        si = 0 if tied else l
        (xs_in, mq, rq, qn, o, xs1, mf, rf, f, fpre, fact, Wq, Wo, W1, W2) = layers[l]
        c, _, _, prep = sets[si]
        # feed-forward: xs2 = xs1 + W2 gelu(W1 LN(xs1) + b1) + b2
        dfpre = ops.gemm(dxs, W2, trans_b=True, act=ACT_DGELU, aux_in=fpre)
        acc_w(si, "ff3_w", dxs, fact); acc_b(si, "ff3_b", dxs)
        df = ops.gemm(dfpre, W1, trans_b=True)
        acc_w(si, "ff0_w", dfpre, f); acc_b(si, "ff0_b", dfpre)
        dxs1 = ln_bwd(si, "ffn_w", "ffn_b", df, xs1, LNW[si]["ffn_w"], mf, rf, dxs)
        # cross attention: xs1 = xs + Wo o + bo
        d_o = ops.gemm(dxs1, Wo, trans_b=True, out=do_stack[l])
        acc_w(si, form.KEY_O, dxs1, o); acc_b(si, "to_out_b", dxs1)
        dq = form.attend_bwd(q_stack[l], c, prep, g, attn_stack[l], rsum_stack[l], o, d_o, dattn_ext if l == depth - 1 else None, ds_stack[l])
        dqn = ops.gemm(dq, Wq, trans_b=True)
        acc_w(si, form.KEY_Q, dq, qn)
        dxs = ln_bwd(si, "norm_w", "norm_b", dqn, xs_in, LNW[si]["norm_w"], mq, rq, dxs1)
    dlatents = ops.rows_reduce_mod(dxs, S)
    # deferred K/V (or context) gradients: one pass per distinct weight set over all the layers that used it
    dfeats = None
    for si in range(nset):
        c, mc, rc, prep = sets[si]
        sl, nl = (slice(0, depth), depth) if tied else (slice(si, si + 1), 1)
        dc = form.finish(G[si], c, prep, g, q_stack, do_stack, ds_stack, attn_stack, rsum_stack, sl, nl)
        dfeats, G[si]["ctx_w"], G[si]["ctx_b"] = ops.layernorm_bwd(dc, feats, LNW[si]["ctx_w"], mc, rc, dres=dfeats)
    dxs = torch.empty((x.shape[1],), dtype=torch.float32, device=dev)
    dx, dnorm_w, dnorm_b = ops.layernorm_bwd(dfeats, x, norm_w, m0, r0, dx_colsum=dxs)
    _publish_colsum(dx, dxs)
    flat = []
    for si in range(nset):
        flat += [G[si][k] for k in _LAYER_KEYS]
    return (dx, dnorm_w, dnorm_b, dlatents, dlast_w, dlast_b, None, *flat)


class AggBlockFn(Function):
    """encoder output -> final LN -> AggregationBlock -> (slots [B*S, D], attn [B*h, S, N] fp32)."""

    @staticmethod
    def forward(ctx, *args):
        return _agg_forward(_Unfolded, ctx, *args)

    @staticmethod
    def backward(ctx, dslots, dattn):
        return _agg_backward(_Unfolded, ctx, dslots, dattn)


class AggBlockFoldFn(Function):
    """encoder output -> final LN -> AggregationBlock (folded slot attention) -> (slots [B*S, D], attn [B*h, S, N] fp32)."""

    @staticmethod
    def forward(ctx, *args):
        return _agg_forward(_Folded, ctx, *args)

    @staticmethod
    def backward(ctx, dslots, dattn):
        return _agg_backward(_Folded, ctx, dslots, dattn)


# =====================================================================================================
# heads
# =====================================================================================================
def _mask_predictor_fwd(slots, W0, b0, W2, b2, W4, b4):
    """MaskPredictor (modeling_slot.py:209-216): Linear -> ReLU -> Linear -> ReLU -> Linear -> Sigmoid, the activations in the GEMM epilogues"""
    m1 = ops.gemm(slots, W0, bias=_f32(b0), act=ACT_RELU)
    m2 = ops.gemm(m1, W2, bias=_f32(b2), act=ACT_RELU)
    Mk = ops.gemm(m2, W4, bias=_f32(b4), act=ACT_SIGMOID)
    return m1, m2, Mk


def _mask_predictor_bwd(dM, slots, m1, m2, Mk, W0, W2, W4):
    """-> (gradient of `slots` through the MaskPredictor, dW0, db0, dW2, db2, dW4, db4)"""
    dp3 = ops.act_bwd(dM, Mk, ACT_SIGMOID)
    dW4, db4 = ops.wgrad(dp3, m2), ops.colsum(dp3)
    dp2 = ops.gemm(dp3, W4, trans_b=True, act=ACT_DRELU, aux_in=m2)
    dW2, db2 = ops.wgrad(dp2, m1), ops.colsum(dp2)
    dp1 = ops.gemm(dp2, W2, trans_b=True, act=ACT_DRELU, aux_in=m1)
    dW0, db0 = ops.wgrad(dp1, slots), ops.colsum(dp1)
    ds_m = ops.gemm(dp1, W0, trans_b=True)
    return ds_m, dW0, db0, dW2, db2, dW4, db4


class HeadFn(Function):
    """slots -> (slots_head = head(slots), mask_predictions = MaskPredictor(slots))  (modeling_slot.py:392-393, 209-216)"""

    @staticmethod
    def forward(ctx, slots, hw, hb, w0, b0, w2, b2, w4, b4, cdt):
        Wh, W0, W2, W4 = (_WCACHE.get(w, cdt) for w in (hw, w0, w2, w4))
        Z = ops.gemm(slots, Wh, bias=_f32(hb))
        m1, m2, Mk = _mask_predictor_fwd(slots, W0, b0, W2, b2, W4, b4)
        ctx.saved = (slots, m1, m2, Mk, Wh, W0, W2, W4)
        return Z, Mk

    @staticmethod
    def backward(ctx, dZ, dM):
        slots, m1, m2, Mk, Wh, W0, W2, W4 = ctx.saved
        ctx.saved = None
        dZ = dZ.contiguous() if dZ is not None else torch.zeros((slots.shape[0], Wh.shape[0]), dtype=slots.dtype, device=slots.device)
        dM = dM.contiguous() if dM is not None else torch.zeros_like(Mk)
        ds_m, dW0, db0, dW2, db2, dW4, db4 = _mask_predictor_bwd(dM, slots, m1, m2, Mk, W0, W2, W4)
        dslots = ops.gemm(dZ, Wh, trans_b=True, res=ds_m)
        dWh, dbh = ops.wgrad(dZ, slots), ops.colsum(dZ)
        return dslots, dWh, dbh, dW0, db0, dW2, db2, dW4, db4, None


class HeadMlpFn(Function):
    """head_type='mlp' (MLPHead, modeling_slot.py:23-34, 307-313): slots -> (slots_head = fc2(relu(fc1(dropout(slots)))), mask_predictions = MaskPredictor(slots)).
    Not on any DEVIAS recipe's path (docs/TRAIN.md uses 'linear'), so it is composed from the per-kernel calls (GEMM with the ReLU / dReLU / Sigmoid
    epilogues, weight gradients, column sums) instead of having a fused region of its own."""

    @staticmethod
    def forward(ctx, slots, f1w, f1b, f2w, f2b, w0, b0, w2, b2, w4, b4, cdt, drop_mask=None):
        F1, F2, W0, W2, W4 = (_WCACHE.get(w, cdt) for w in (f1w, f2w, w0, w2, w4))
        slots = slots.contiguous()
        xin = ops.mul_mask(slots, drop_mask) if drop_mask is not None else slots          # fc_dropout applies to the head's input only (:393)
        t = ops.gemm(xin, F1, bias=_f32(f1b), act=ACT_RELU)
        Z = ops.gemm(t, F2, bias=_f32(f2b))
        m1, m2, Mk = _mask_predictor_fwd(slots, W0, b0, W2, b2, W4, b4)
        ctx.saved = (slots, xin, t, m1, m2, Mk, F1, F2, W0, W2, W4, drop_mask)
        return Z, Mk

    @staticmethod
    def backward(ctx, dZ, dM):
        if ctx.saved is None:
            raise RuntimeError("HeadMlpFn: backward already consumed the saved activations (one backward per forward)")
        slots, xin, t, m1, m2, Mk, F1, F2, W0, W2, W4, drop_mask = ctx.saved
        ctx.saved = None
        dZ = dZ.contiguous() if dZ is not None else torch.zeros((slots.shape[0], F2.shape[0]), dtype=slots.dtype, device=slots.device)
        dM = dM.contiguous() if dM is not None else torch.zeros_like(Mk)
        ds_m, dW0, db0, dW2, db2, dW4, db4 = _mask_predictor_bwd(dM, slots, m1, m2, Mk, W0, W2, W4)
        dF2, dbf2 = ops.wgrad(dZ, t), ops.colsum(dZ)
        dt = ops.gemm(dZ, F2, trans_b=True, act=ACT_DRELU, aux_in=t)
        dF1, dbf1 = ops.wgrad(dt, xin), ops.colsum(dt)
        if drop_mask is not None:
            dslots = ops.mul_mask(ops.gemm(dt, F1, trans_b=True), drop_mask, ds_m)
        else:
            dslots = ops.gemm(dt, F1, trans_b=True, res=ds_m)
        return dslots, dF1, dbf1, dF2, dbf2, dW0, db0, dW2, db2, dW4, db4, None, None
