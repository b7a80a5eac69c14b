"""The two-token multi-task baseline (model/modeling_multi_task.py:178-343 of the reference, `disentangle_vit_base_patch16_224`): ONE encoder over
`cls | patches | scene` tokens with a head per token -- the action head trained on labels, the scene head distilled from the frozen scene teacher
(devias_amd.multi_task_loss.TrainLoss, devias_amd.engine_for_multi_task).  It is the baseline the slot model is compared against.

`forward(x, return_attn=False)` returns `((action_token, action_logits), (scene_token, scene_logits))` like the reference (:324-334): the tokens are
norm(x)[:, 0] and norm(x)[:, -1] before fc_dropout.  With `unified_head` one head of num_classes + num_scene_classes rows serves both tokens.

Trainable (`self.training and torch.is_grad_enabled()`): PatchEmbedFn, the cls row prepended and the scene row appended (each parameter + its position row in
fp32, then cast, as the plain ViT builds its cls row), Block.run per block on the unpadded [B * (N + 2), D] token matrix and regions.TwoTokenHeadRegionFn
(csrc/token_head.hip) for everything after the encoder.  Otherwise (eval(), or under torch.no_grad()) the same path runs without a graph: the blocks take the
forward-only region and the head region saves nothing; at zero drop rates the outputs are bitwise the training forward's."""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn

from .functions import DropMaskFn, PatchEmbedFn
from .modeling_slot import Block, DropoutSource, PatchEmbed, _cfg, get_sinusoid_encoding_table, register_model
from .regions import TwoTokenHeadRegionFn


class VisionTransformer(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=False, qk_scale=None, fc_drop_rate=0., drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., norm_layer=nn.LayerNorm, init_values=0., use_learnable_pos_emb=False, init_scale=0.,
                 all_frames=16, tubelet_size=2, use_checkpoint=False, unified_head=False, num_scene_classes=365, compute_dtype='bf16'):
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
        self.num_scene_classes = num_scene_classes
        self.num_features = self.embed_dim = embed_dim
        self.tubelet_size = tubelet_size
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      num_frames=all_frames, tubelet_size=tubelet_size)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        nn.init.trunc_normal_(self.cls_token, std=.02)
        self.scene_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        nn.init.trunc_normal_(self.scene_token, std=.02)
        self.use_checkpoint = False
        self.unified_head = bool(unified_head)
        self.pos_embed = get_sinusoid_encoding_table(num_patches + 2, embed_dim)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                  attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, init_values=init_values) for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.fc_drop_rate = float(fc_drop_rate)
        self.fc_dropout = nn.Dropout(p=fc_drop_rate) if fc_drop_rate > 0 else nn.Identity()      # parameter-free container as in the reference (:246); applied in TwoTokenHeadRegionFn
        if self.unified_head:
            self.head = nn.Linear(embed_dim, num_classes + num_scene_classes) if num_classes > 0 else nn.Identity()
        else:
            self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()
            self.scene_head = nn.Linear(embed_dim, num_scene_classes) if num_scene_classes > 0 else nn.Identity()
        heads = [self.head] + ([] if self.unified_head else [self.scene_head])
        for h in heads:
            nn.init.trunc_normal_(h.weight, std=.02)
        self.apply(self._init_weights)
        for h in heads:
            h.weight.data.mul_(init_scale)
            h.bias.data.mul_(init_scale)
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
        return {'pos_embed', 'cls_token', 'scene_token'}

    def get_classifier(self):
        return self.head

    def reset_classifier(self, num_classes, global_pool=''):
        self.num_classes = num_classes
        self.head = nn.Linear(self.embed_dim, num_classes) if num_classes > 0 else nn.Identity()

    def set_compute_dtype(self, compute_dtype):
        self.compute_dtype = {'bf16': torch.bfloat16, 'fp32': torch.float32}[compute_dtype]
        return self

    def _pos(self, device, dtype):
        """(the whole N + 2 row table, its rows 1 .. N for the patches) on the device in the compute dtype"""
        key = (str(device), dtype)
        if key not in self._pos_cache:
            pos = self.pos_embed[0].to(device=device, dtype=dtype).contiguous()
            self._pos_cache[key] = (pos, pos[1:-1].contiguous())
        return self._pos_cache[key]

    def forward_features(self, x, return_attn=False):
        """the reference's (action token, scene token, attn_list) (:293-321); attn_list is always empty"""
        (ta, _), (ts, _) = self.forward(x, return_attn)
        return ta, ts, []

    def _builds_graph(self):
        return self.training and torch.is_grad_enabled()

    def _run(self, x):
        """PatchEmbedFn -> cat(cls, patches, scene) -> Block.run per block -> TwoTokenHeadRegionFn, on the unpadded [B * Nt, D] token matrix.  With autograd on this is the
        training step's forward; under torch.no_grad() Block.run takes the forward-only region and the head region saves nothing."""
        if not x.is_cuda:
            raise RuntimeError("devias_amd multi-task VisionTransformer runs on an MI355X only (HIP kernels; no CPU fallback): move the model and the input to cuda")
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        x = x.contiguous()
        heads = [self.head] + ([] if self.unified_head else [self.scene_head])
        if not all(isinstance(h, nn.Linear) and h.out_features >= 2 for h in heads) or self.embed_dim not in (384, 768, 1024):
            raise NotImplementedError(f"the two-token head region is built for heads of at least 2 classes and widths 384 / 768 / 1024, got "
                                      f"{self.num_classes} + {self.num_scene_classes} classes, D={self.embed_dim}")
        B = x.shape[0]
        pe = self.patch_embed
        N, D, cdt = pe.num_patches, self.embed_dim, self.compute_dtype
        Nt = N + 2
        pos, pos_patches = self._pos(x.device, cdt)
        tok = PatchEmbedFn.apply(x, pe.proj.weight, pe.proj.bias, pos_patches, (pe.tubelet_size, pe.patch_size[0], cdt))
        cls = (self.cls_token.reshape(1, D).float() + pos[:1].float()).to(cdt)                     # cat(cls, patches, scene), THEN + pos (:296-301)
        scene = (self.scene_token.reshape(1, D).float() + pos[N + 1:].float()).to(cdt)
        h = torch.cat([cls.expand(B, 1, D), tok.view(B, N, D), scene.expand(B, 1, D)], dim=1).reshape(B * Nt, D)
        src = self.dropout_source or DropoutSource()
        if self.training and self.pos_drop.p > 0:
            h = DropMaskFn.apply(h, src.element_mask("pos", -1, tuple(h.shape), 1.0 - float(self.pos_drop.p), h.device))
        for i, blk in enumerate(self.blocks):
            h = blk.run(h, B, Nt, cdt, i, src)
        masks = ()
        if self.training and self.fc_drop_rate > 0:
            keep = 1.0 - self.fc_drop_rate                  # nn.Dropout(fc_drop_rate) on each token (:326-330): two independent Bernoulli(keep) / keep draws
            masks = (src.element_mask("head", -2, (B, D), keep, x.device).contiguous(), src.element_mask("scene_head", -3, (B, D), keep, x.device).contiguous())
        meta = (B, Nt, self.norm.eps, cdt, torch.is_grad_enabled())      # (read here: inside a Function's forward autograd is always off)
        sw, sb = (None, None) if self.unified_head else (self.scene_head.weight, self.scene_head.bias)
        ta, za, ts, zs = TwoTokenHeadRegionFn.apply(h, self.norm.weight, self.norm.bias, self.head.weight, self.head.bias, sw, sb, meta, *masks)
        return (ta, za), (ts, zs)

    def forward(self, x, return_attn=False):
        if return_attn:
            raise NotImplementedError("per-block attention maps are never materialised by the fused MHSA kernel")
        if self._builds_graph():
            return self._run(x)
        with torch.no_grad():
            return self._run(x)


@register_model
def disentangle_vit_base_patch16_224(pretrained=False, **kwargs):
    model = VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                              norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
    model.default_cfg = _cfg()
    return model
