"""The plain video ViT (model/modeling_finetune.py:178-334 of the reference, `vit_base_patch16_224`): the scene teacher behind --scene_model_path
(use_mean_pooling=False: cls token + N patch tokens) and the action baseline (use_mean_pooling=True, the reference's default: fc_norm of the mean token).

`forward(x, return_attn=False)` returns `(token[B, D], logits[B, num_classes])` like the reference (:314-325).

Frozen (eval(), or under torch.no_grad(): what `engine/engine_for_slot.train_class_batch` calls, :52-53): forward only, nothing saved.  In cls-token mode
N + 1 = 1569 tokens per clip is odd, so the token matrix is padded (once, with zero rows at the END of the batch) to a multiple of 256 rows to stay on the
full-tile GEMM kernels; the attention kernels handle the ragged sequence length themselves.  Mean-pooling mode runs the blocks' forward-only region on the
unpadded tokens and the pooled-head region without a save arena.

Trainable (`self.training and torch.is_grad_enabled()`): PatchEmbedFn, the cls row prepended in cls-token mode, Block.run per block (the slot model's training
path, unpadded: B * 1569 rows run the 128 x 128 GEMM kernels) and regions.PoolHeadRegionFn (csrc/token_head.hip) for everything after the encoder."""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn

from . import _lib, modeling_slot, ops
from .functions import DropMaskFn, PatchEmbedFn
from .modeling_slot import Block, DropoutSource, PatchEmbed, _cfg, get_sinusoid_encoding_table, register_model
from .ops import ACT_GELU
from .regions import PoolHeadRegionFn
from .weight_cache import _WCACHE, _f32


class VisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=False, qk_scale=None, fc_drop_rate=0., drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., norm_layer=nn.LayerNorm, init_values=0., use_learnable_pos_emb=False, init_scale=0.,
                 all_frames=16, tubelet_size=2, use_checkpoint=False, use_mean_pooling=True, compute_dtype='bf16'):
        super().__init__()
        if use_learnable_pos_emb:
            raise NotImplementedError("learnable pos-emb is not used by DEVIAS (sinusoid table only)")
        if use_checkpoint:
            raise NotImplementedError("use_checkpoint=True: activation checkpointing re-runs a block's forward inside backward, which the fused regions "
                                      "(one saved arena, ONE backward per forward) do not support; 288 GB hold the activations")
        for nm, v in (("fc_drop_rate", fc_drop_rate), ("drop_rate", drop_rate), ("attn_drop_rate", attn_drop_rate), ("drop_path_rate", drop_path_rate)):
            if not 0.0 <= float(v) < 1.0:
                raise ValueError(f"{nm} must be in [0, 1), got {v}")
        self.dropout_source = None             # None: DropoutSource() (torch's generators); tests install one with given masks
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.tubelet_size = tubelet_size
        self.use_mean_pooling = bool(use_mean_pooling)
        self.use_checkpoint = False
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      num_frames=all_frames, tubelet_size=tubelet_size)
        num_patches = self.patch_embed.num_patches
        if not use_mean_pooling:
            self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
            nn.init.trunc_normal_(self.cls_token, std=.02)
            num_patches += 1
        self.pos_embed = get_sinusoid_encoding_table(num_patches, embed_dim)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                  attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, init_values=init_values) for i in range(depth)])
        self.norm = nn.Identity() if use_mean_pooling else norm_layer(embed_dim)
        self.fc_norm = norm_layer(embed_dim) if use_mean_pooling else None
        self.fc_drop_rate = float(fc_drop_rate)
        self.fc_dropout = nn.Dropout(p=fc_drop_rate) if fc_drop_rate > 0 else nn.Identity()      # parameter-free container as in the reference (:238); applied in PoolHeadRegionFn
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
        nn.init.trunc_normal_(self.head.weight, std=.02)
        self.apply(self._init_weights)
        self.head.weight.data.mul_(init_scale)
        self.head.bias.data.mul_(init_scale)
        self.compute_dtype = {'bf16': torch.bfloat16, 'fp32': torch.float32}[compute_dtype]
        self._pos_cache = {}

    def _init_weights(self, m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def get_num_layers(self):
        return len(self.blocks)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {'pos_embed', 'cls_token'}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=''):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def set_compute_dtype(self, compute_dtype):
        self.compute_dtype = {'bf16': torch.bfloat16, 'fp32': torch.float32}[compute_dtype]
        return self

    def _pos(self, device, dtype):
        key = (str(device), dtype)
        if key not in self._pos_cache:
            self._pos_cache[key] = self.pos_embed[0].to(device=device, dtype=dtype).contiguous()
        return self._pos_cache[key]

    def forward_features(self, x, return_attn=False):
        """the reference's token (:273-311)"""
        if self._builds_graph() or self.use_mean_pooling:
            return self.forward(x, return_attn)[0]
        return self._frozen_features(x, return_attn)

    @torch.no_grad()
    def _frozen_features(self, x, return_attn=False):
        if return_attn:
            raise NotImplementedError("per-block attention maps are never materialised by the fused MHSA kernel")
        if not x.is_cuda:
            raise RuntimeError("devias_amd teacher runs on an MI355X only (HIP kernels; no CPU fallback)")
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        x = x.contiguous()
        B = x.shape[0]
        pe = self.patch_embed
        N, D, cdt = pe.num_patches, self.embed_dim, self.compute_dtype
        Nt = N + 1
        pos = self._pos(x.device, cdt)                                   # [N+1, D]
        A = ops.patch_im2col(x, pe.tubelet_size, pe.patch_size[0], cdt)
        tok = ops.gemm(A, _WCACHE.get(pe.proj.weight, cdt), bias=_f32(pe.proj.bias), res=pos[1:].contiguous(), res_mod=N)
        cls = (self.cls_token.detach().reshape(1, D).float() + pos[:1].float()).to(cdt)        # cls FIRST, then + pos (:277-283)
        M = B * Nt
        Mp = ((M + 255) // 256) * 256
        h = torch.zeros((Mp, D), dtype=cdt, device=x.device)
        hv = h[:M].view(B, Nt, D)
        hv[:, 0] = cls
        hv[:, 1:] = tok.view(B, N, D)
        if modeling_slot._INFER:
            # one library call per block over the padded ping-pong pair (devias_encoder_block_infer: the kernels of the loop below in its order, every intermediate in the
            # stream's workspace); the call zeroes the pad rows of its attention output itself.  Bitwise the loop's (token, logits).
            h2 = torch.empty_like(h)
            for blk in self.blocks:
                blk.run_infer(h, h2, B, Nt, cdt, False)
                h, h2 = h2, h
            return self._cls_norm(h, M, B, Nt, D)
        scale = 64 ** -0.5
        # attention output buffer, padded like h: allocated ONCE, mhsa_fwd writes its first M rows in place every block and the pad rows
        # stay zero (no per-block zeros() + slice copy)
        o = torch.zeros((Mp, D), dtype=cdt, device=x.device) if Mp != M else torch.empty((M, D), dtype=cdt, device=x.device)
        for blk in self.blocks:
            a = blk.attn
            Wqkv, Wp, W1, W2 = (_WCACHE.get(w, cdt) for w in (a.qkv.weight, a.proj.weight, blk.mlp.fc1.weight, blk.mlp.fc2.weight))
            u, _, _ = ops.layernorm_fwd(h, _f32(blk.norm1.weight), _f32(blk.norm1.bias), blk.norm1.eps)
            qkv = ops.gemm(u, Wqkv, bias=_WCACHE.qkv_bias(a.q_bias, a.v_bias))          # q_bias | 0 | v_bias, rebuilt only when a bias changed
            ops.mhsa_fwd(qkv[:M], B, Nt, a.num_heads, scale, out=o[:M])
            h1 = ops.gemm(o, Wp, bias=_f32(a.proj.bias), res=h)
            u2, _, _ = ops.layernorm_fwd(h1, _f32(blk.norm2.weight), _f32(blk.norm2.bias), blk.norm2.eps)
            act = ops.gemm(u2, W1, bias=_f32(blk.mlp.fc1.bias), act=ACT_GELU)
            h = ops.gemm(act, W2, bias=_f32(blk.mlp.fc2.bias), res=h1)
        return self._cls_norm(h, M, B, Nt, D)

    def _cls_norm(self, h, M, B, Nt, D):
        tokens0 = h[:M].view(B, Nt, D)[:, 0].contiguous()                # only the cls rows need the final LayerNorm
        y, _, _ = ops.layernorm_fwd(tokens0, _f32(self.norm.weight), _f32(self.norm.bias), self.norm.eps)
        return y

    @torch.no_grad()
    def _frozen_forward(self, x, return_attn=False):
        token = self._frozen_features(x, return_attn)
        logits = ops.gemm(token, _WCACHE.get(self.head.weight, self.compute_dtype), bias=_f32(self.head.bias))
        return token, logits

    def _builds_graph(self):
        return self.training and torch.is_grad_enabled()

    def _pooled_forward(self, x):
        """PatchEmbedFn -> (cls row) -> Block.run per block -> PoolHeadRegionFn, on the unpadded [B * Nt, D] token matrix.  With autograd on this is the training
        step's forward; under torch.no_grad() Block.run takes the forward-only region and the head region saves nothing (bitwise the same outputs at zero drop rates)."""
        if not x.is_cuda:
            raise RuntimeError("devias_amd.VisionTransformer runs on an MI355X only (HIP kernels; no CPU fallback): move the model and the input to cuda")
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        x = x.contiguous()
        if not isinstance(self.head, nn.Linear) or self.num_classes < 2 or self.embed_dim not in (384, 768, 1024):
            raise NotImplementedError(f"the pooled-head region is built for at least 2 classes and widths 384 / 768 / 1024, got {self.num_classes} classes, D={self.embed_dim}")
        B = x.shape[0]
        pe = self.patch_embed
        N, D, cdt = pe.num_patches, self.embed_dim, self.compute_dtype
        pos = self._pos(x.device, cdt)
        pmeta = (pe.tubelet_size, pe.patch_size[0], cdt)
        if self.use_mean_pooling:
            Nt = N
            h = PatchEmbedFn.apply(x, pe.proj.weight, pe.proj.bias, pos, pmeta)
        else:
            Nt = N + 1
            key = (str(x.device), cdt, "patches")
            if key not in self._pos_cache:
                self._pos_cache[key] = pos[1:].contiguous()
            tok = PatchEmbedFn.apply(x, pe.proj.weight, pe.proj.bias, self._pos_cache[key], pmeta)
            cls = (self.cls_token.reshape(1, D).float() + pos[:1].float()).to(cdt)                 # cls FIRST, then + pos (:277-283)
            h = torch.cat([cls.expand(B, 1, D), tok.view(B, N, D)], dim=1).reshape(B * Nt, D)
        src = self.dropout_source or DropoutSource()
        if self.training and self.pos_drop.p > 0:
            h = DropMaskFn.apply(h, src.element_mask("pos", -1, tuple(h.shape), 1.0 - float(self.pos_drop.p), h.device))
        for i, blk in enumerate(self.blocks):
            h = blk.run(h, B, Nt, cdt, i, src)
        drop_mask = None
        if self.training and self.fc_drop_rate > 0:
            keep = 1.0 - self.fc_drop_rate                  # nn.Dropout(fc_drop_rate) on the token (:320): Bernoulli(keep) / keep, drawn like drop_path's masks
            drop_mask = self.dropout_source.element_mask("head", -2, (B, D), keep, x.device) if self.dropout_source is not None else \
                ((keep + torch.rand((B, D), device=x.device, dtype=torch.float32)).floor() / keep).contiguous()
        ln = self.fc_norm if self.use_mean_pooling else self.norm
        meta = (B, Nt, _lib.POOL_MEAN if self.use_mean_pooling else _lib.POOL_CLS, ln.eps, cdt, torch.is_grad_enabled())      # (read here: inside a Function's forward autograd is always off)
        args = (h, ln.weight, ln.bias, self.head.weight, self.head.bias, meta)
        return PoolHeadRegionFn.apply(*args, drop_mask) if drop_mask is not None else PoolHeadRegionFn.apply(*args)

    def forward(self, x, return_attn=False):
        if return_attn:
            raise NotImplementedError("per-block attention maps are never materialised by the fused MHSA kernel")
        if self._builds_graph():
            return self._pooled_forward(x)
        if self.use_mean_pooling:
            with torch.no_grad():
                return self._pooled_forward(x)
        return self._frozen_forward(x, return_attn)          # eval() or no_grad in cls-token mode: the frozen teacher's path, tensors without a graph


@register_model
def vit_base_patch16_224(pretrained=False, **kwargs):
    model = VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                              norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
    model.default_cfg = _cfg()
    return model
