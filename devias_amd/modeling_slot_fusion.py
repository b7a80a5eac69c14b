"""The downstream model of docs/DOWNSTREAM.md: the slot-DEVIAS encoder and aggregation block, the frozen pre-trained head as slot selector, and the MLPHead fusion
classifier on the (action, scene) slot pair (model/modeling_slot_fusion.py).  Same constructor keywords and parameter names as the reference (a reference
state_dict loads, and one saved here loads there); forward() returns the reference's (input [B, 2D], output [B, downstream_nb_classes]).

The encoder, the aggregation block and their forward-only paths are the slot model's (devias_amd.modeling_slot: this class derives from its VisionTransformer and
runs its forward_features and aggregation call); everything after the slots is one fused region per direction (regions.FusionHeadFn, csrc/fusion_head.hip).
Only head_type='mlp' with slot_fusion_method='concat' is built: it is the form the reference's documentation runs ('linear' + 'concat' raises a TypeError there:
nn.Linear.forward is called with two tokens), and 'gap' is the reference's baseline without slots."""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn

from . import modeling_slot as _ms
from .modeling_slot import _cfg, register_model
from .regions import FusionHeadFn


class MLPHead(nn.Module):
    """parameter container of model/modeling_slot_fusion.py:23-40.  fc_scene_down / fc_scene_ln exist, load, save and count as parameters and are never used: the
    reference's forward sends both tokens through fc_action_down / fc_action_ln (:43-44), so they never receive a gradient."""

    def __init__(self, in_dim, out_dim, fc_drop_rate=0., use_input_ln=True):
        super().__init__()
        self.fc_action_down = nn.Linear(in_dim, in_dim // 2)
        self.fc_scene_down = nn.Linear(in_dim, in_dim // 2)
        self.fc_action_ln = nn.LayerNorm(in_dim // 2)
        self.fc_scene_ln = nn.LayerNorm(in_dim // 2)
        self.use_input_ln = use_input_ln
        if use_input_ln:
            self.fc_input_ln = nn.LayerNorm(in_dim)
        self.classifier = nn.Linear(in_dim, out_dim)
        self.fc_dropout = nn.Dropout(p=fc_drop_rate) if fc_drop_rate > 0 else nn.Identity()
        self.relu = nn.ReLU()


class VisionTransformer(_ms.VisionTransformer):
    """model/modeling_slot_fusion.py:214-403.  Extra kwarg: compute_dtype in {'bf16', 'fp32'}."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4., qkv_bias=False,
                 qk_scale=None, fc_drop_rate=0., drop_rate=0., attn_drop_rate=0., drop_path_rate=0., norm_layer=nn.LayerNorm, init_values=0.,
                 use_learnable_pos_emb=False, init_scale=0., all_frames=16, tubelet_size=2, use_checkpoint=False, num_latents=4, head_type='linear',
                 agg_weights_tie=True, agg_depth=4, num_scene_classes=365, slot_fusion_method='concat', downstream_nb_classes=50, use_input_ln=True,
                 compute_dtype='bf16'):
        if slot_fusion_method == 'gap':
            raise NotImplementedError("slot_fusion_method='gap' is the reference's baseline without slots (mean token -> action_norm -> linear head); "
                                      "the downstream recipe runs 'concat'")
        if slot_fusion_method != 'concat':
            raise NotImplementedError(f"slot_fusion_method must be 'concat', got {slot_fusion_method!r} (modeling_slot_fusion.py:305-306)")
        if head_type == 'linear':
            raise NotImplementedError("head_type='linear' with 'concat' does not run in the reference (Linear.forward() takes 2 positional arguments but 3 were "
                                      "given, modeling_slot_fusion.py:399); the downstream recipe runs head_type='mlp'")
        if head_type != 'mlp':
            raise ValueError(f"head_type must be 'mlp', got {head_type!r}")
        if not downstream_nb_classes or downstream_nb_classes < 2:
            raise NotImplementedError("downstream_nb_classes must be at least 2 (the fused classifier region)")
        # the slot model's tree (patch embed, blocks, norm, aggregation block, the linear pre-trained head); its mask predictor is not part of this model
        super().__init__(img_size=img_size, patch_size=patch_size, in_chans=in_chans, num_classes=num_classes, embed_dim=embed_dim, depth=depth, num_heads=num_heads,
                         mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, fc_drop_rate=fc_drop_rate, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate,
                         drop_path_rate=drop_path_rate, norm_layer=norm_layer, init_values=init_values, use_learnable_pos_emb=use_learnable_pos_emb,
                         init_scale=1.0, all_frames=all_frames, tubelet_size=tubelet_size, use_checkpoint=use_checkpoint, num_latents=num_latents, head_type='linear',
                         slot_matching_method='matching', num_scene_classes=num_scene_classes, agg_weights_tie=agg_weights_tie, agg_depth=agg_depth,
                         compute_dtype=compute_dtype)
        del self.mask_predictor
        del self.slot_matching_method, self.select_slots_info
        self.slot_fusion_method = slot_fusion_method
        self.use_input_ln = use_input_ln
        self.head_type = head_type
        head = self.head
        del self.head                                                   # registration order of the reference: action_norm, scene_norm, head, fusion_head
        self.action_norm = norm_layer(embed_dim)
        self.scene_norm = norm_layer(embed_dim)
        self.head = head
        self.fusion_head = MLPHead(embed_dim, downstream_nb_classes, fc_drop_rate=fc_drop_rate, use_input_ln=use_input_ln)
        nn.init.trunc_normal_(self.fusion_head.classifier.weight, std=.02)
        self.apply(self._init_weights)
        self.last_idx = None          # int32 [B, 2] of the last forward: (action slot, scene slot)

    def get_select_slot_info(self):
        raise NotImplementedError("the fusion model keeps no selection statistics (modeling_slot_fusion.py has none)")

    reset_select_slot_info = get_select_slot_info

    def forward(self, x, return_attn=False):
        B = x.shape[0]
        D = self.embed_dim
        cdt = self.compute_dtype
        h = self.forward_features(x, return_attn)
        S = self.agg_block.num_latents
        if S > 4 or D not in (384, 768, 1024):
            raise NotImplementedError(f"the fused classifier region is built for at most 4 slots and widths 384 / 768 / 1024, got S={S} D={D}")
        slots, _attn = self._aggregate(h, B)
        fh = self.fusion_head
        drop_mask = None
        if self.training and self.fc_drop_rate > 0:
            keep = 1.0 - self.fc_drop_rate                  # nn.Dropout(fc_drop_rate) on relu(.) (MLPHead.forward :49): Bernoulli(keep) / keep, drawn like drop_path's masks
            src = self.dropout_source
            drop_mask = src.element_mask("fusion", -2, (B, D), keep, x.device) if src is not None else \
                ((keep + torch.rand((B, D), device=x.device, dtype=torch.float32)).floor() / keep).contiguous()
        iln = (fh.fc_input_ln.weight, fh.fc_input_ln.bias) if fh.use_input_ln else (None, None)
        fmeta = (B, S, self.num_classes, self.action_norm.eps, fh.fc_action_ln.eps, cdt, torch.is_grad_enabled())      # (read here: inside a Function's forward autograd is always off)
        args = (slots, self.head.weight, self.head.bias, self.action_norm.weight, self.action_norm.bias, self.scene_norm.weight, self.scene_norm.bias,
                fh.fc_action_down.weight, fh.fc_action_down.bias, fh.fc_action_ln.weight, fh.fc_action_ln.bias, iln[0], iln[1], fh.classifier.weight, fh.classifier.bias, fmeta)
        inp, out, idx = FusionHeadFn.apply(*args, drop_mask) if drop_mask is not None else FusionHeadFn.apply(*args)
        self.last_idx = idx
        return inp, out


def _make(embed_dim, depth, num_heads, kwargs):
    model = VisionTransformer(patch_size=16, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4, qkv_bias=True,
                              norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
    model.default_cfg = _cfg()
    return model


@register_model
def slot_fusion_vit_base_patch16_224(pretrained=False, **kwargs):
    return _make(768, 12, 12, kwargs)


@register_model
def slot_fusion_vit_small_patch16_224(pretrained=False, **kwargs):
    """not in the reference (its forward hard-wires 768, :380)"""
    return _make(384, 12, 6, kwargs)


@register_model
def slot_fusion_vit_large_patch16_224(pretrained=False, **kwargs):
    """not in the reference"""
    return _make(1024, 24, 16, kwargs)
