"""MI355X-native slot-DEVIAS student model behind the reference's timm-style surface.

Mirrors model/modeling_slot.py + agg_block/{agg_block,attention}.py of the reference: same constructor kwargs,
same module tree / parameter names (state_dict compatible), same `forward()` 3-tuple.  The nn.Module
objects below (nn.Linear, nn.LayerNorm, nn.Conv3d ...) are PARAMETER CONTAINERS only: their own forward() is never
called.  All arithmetic runs in libdevias_amd.so (hand-written gfx950 HIP kernels) through autograd Functions that live
in two other modules; this one holds the reference surface and chooses among them (Block.run, VisionTransformer.forward):

    devias_amd.regions     EncoderBlockRegionFn, AggBlockRegionFn, HeadRegionFn: one library call per region and direction (the default)
    devias_amd.functions   PatchEmbedFn, DropMaskFn, and the same regions kernel by kernel: EncoderBlockFn (also what runs with nn.Dropout inside
                           the block), AggBlockFoldFn, AggBlockFn (unfolded slot attention: more than 4 slots, other widths), HeadFn, HeadMlpFn
    devias_amd.weight_cache  the compute-dtype copies of the weights that all of them read

`compute_dtype` selects the activation/weight storage type of the kernels: 'fp32' (parity mode: exact fp32 MFMA / VALU
kernels) or 'bf16' (measured mode: bf16 storage, fp32 accumulation and statistics).  Master parameters are always fp32.
There is no PyTorch fallback: without a GPU + the built HIP library forward() raises.
"""
from __future__ import annotations

import os
from functools import partial
from typing import Dict, List

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .functions import AggBlockFn, AggBlockFoldFn, DropMaskFn, EncoderBlockFn, HeadFn, HeadMlpFn, PatchEmbedFn
from .regions import AggBlockRegionFn, EncoderBlockRegionFn, HeadRegionFn
from .weight_cache import _Q_PRESCALE, _WCACHE, _f32, _use_q_prescale

_REGIONS = os.environ.get("DEVIAS_REGIONS", "1") != "0"      # the fused regions (devias_amd.regions); 0 = the per-kernel Functions
_INFER = os.environ.get("DEVIAS_INFER_REGION", "1") != "0"   # under no_grad the encoder blocks run devias_encoder_block_infer (no save arena, fc1 with one output); 0 = the training forward
_AGG_FOLD = os.environ.get("DEVIAS_AGG_FOLD", "1") != "0"    # the folded slot attention where it applies (VisionTransformer.forward); 0 = always the unfolded form

_MODEL_REGISTRY: Dict[str, callable] = {}


def register_model(fn):
    """timm.models.registry.register_model stand-in (timm is used when importable, see create_model)."""
    _MODEL_REGISTRY[fn.__name__] = fn
    try:  # register with timm too so `timm.create_model('slot_vit_base_patch16_224', ...)` works as in the reference
        from timm.models.registry import register_model as _timm_register  # type: ignore
        _timm_register(fn)
    except Exception:
        pass
    return fn


def create_model(name: str, pretrained: bool = False, **kwargs):
    """timm.create_model look-alike: drops None kwargs like timm does (run_slot_finetuning.py:371-390)."""
    kwargs = {k: v for k, v in kwargs.items() if v is not None}
    return _MODEL_REGISTRY[name](pretrained=pretrained, **kwargs)


def _cfg(url="", **kwargs):
    return {"url": url, "num_classes": 400, "input_size": (3, 224, 224), "pool_size": None, "crop_pct": .9,
            "interpolation": "bicubic", "mean": (0.5, 0.5, 0.5), "std": (0.5, 0.5, 0.5), **kwargs}


def get_sinusoid_encoding_table(n_position: int, d_hid: int) -> torch.Tensor:
    """float64 table cast to fp32, [1, N, D] (modeling_slot.py:181-191)."""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    j = np.arange(d_hid)
    angle = pos / np.power(10000.0, 2.0 * (j // 2) / d_hid)[None, :]
    table = angle.copy()
    table[:, 0::2] = np.sin(angle[:, 0::2])
    table[:, 1::2] = np.cos(angle[:, 1::2])
    return torch.tensor(table, dtype=torch.float32).unsqueeze(0)


class DropoutSource:
    """Where the training-time dropout masks of the encoder come from.  The default draws them from torch's generators, as nn.Dropout does
    (element masks: the device generator, like the drop_path masks; the seed of the attention-matrix mask: the CPU generator, no device sync).
    Tests and tests/golden/make_goldens.py replace it (VisionTransformer.dropout_source) to give the reference, the oracle and the kernels the SAME masks."""

    def element_mask(self, kind: str, block: int, shape, keep: float, device) -> torch.Tensor:
        """fp32 mask of 0 / (1 / keep); kind in {'pos', 'proj', 'mlp'}"""
        return ((keep + torch.rand(shape, device=device, dtype=torch.float32)).floor() / keep).contiguous()

    def path_scale(self, block: int, B: int, keep: float, device) -> torch.Tensor:
        """fp32 [2, B]: timm 0.4.12 drop_path (modeling_slot.py:36-47) masks of the attention and the MLP branch, 0 / (1 / keep) per sample"""
        return ((keep + torch.rand((2, B), device=device, dtype=torch.float32)).floor() / keep).contiguous()

    def attn_seed(self, block: int) -> int:
        return int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())


# =====================================================================================================
# module tree (parameter containers with the reference's names)
# =====================================================================================================
class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0., attn_head_dim=None):
        super().__init__()
        self.num_heads = num_heads
        head_dim = dim // num_heads if attn_head_dim is None else attn_head_dim
        all_head_dim = head_dim * num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, all_head_dim * 3, bias=False)
        if qkv_bias:
            self.q_bias = nn.Parameter(torch.zeros(all_head_dim))
            self.v_bias = nn.Parameter(torch.zeros(all_head_dim))
        else:
            self.q_bias = None
            self.v_bias = None
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(all_head_dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        if head_dim != 64:
            raise ValueError(f"devias_amd MHSA kernels are built for head_dim 64 (ViT-S/B/L), got {head_dim}")


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0., drop_path=0.,
                 init_values=None, act_layer=nn.GELU, norm_layer=nn.LayerNorm, attn_head_dim=None):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                              proj_drop=drop, attn_head_dim=attn_head_dim)
        self.drop_path_rate = float(drop_path)
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        if init_values and init_values > 0:   # gamma_1/2 exist in the reference but are never applied (:136-152)
            self.gamma_1 = nn.Parameter(init_values * torch.ones(dim), requires_grad=True)
            self.gamma_2 = nn.Parameter(init_values * torch.ones(dim), requires_grad=True)
        else:
            self.gamma_1, self.gamma_2 = None, None

    def run(self, x, B, N, cdt, index=0, source=None):
        a = self.attn
        if a.q_bias is None:
            raise NotImplementedError("qkv_bias=False is not used by any DEVIAS entrypoint")
        ds1 = ds2 = None
        if self.training and self.drop_path_rate > 0:
            # timm 0.4.12 drop_path (modeling_slot.py:36-47): per-sample Bernoulli(keep) mask scaled by 1/keep, drawn independently
            # for the attention and the MLP branch; applied inside the residual GEMM epilogues (row_scale)
            source = source or DropoutSource()
            ds = source.path_scale(index, B, 1.0 - self.drop_path_rate, x.device)
            ds1, ds2 = ds[0], ds[1]
        meta = (B, N, a.num_heads, self.norm1.eps, cdt)
        args = (x, self.norm1.weight, self.norm1.bias, a.qkv.weight, a.q_bias, a.v_bias, a.proj.weight, a.proj.bias, self.norm2.weight, self.norm2.bias,
                self.mlp.fc1.weight, self.mlp.fc1.bias, self.mlp.fc2.weight, self.mlp.fc2.bias, meta)
        p_drop, p_attn = float(a.proj_drop.p), float(a.attn_drop.p)          # Mlp.drop.p == proj_drop.p (Block.__init__: both `drop`)
        if self.training and (p_drop > 0 or p_attn > 0):
            # nn.Dropout inside the block (modeling_slot.py:110 attn_drop, :114 proj_drop, :66 Mlp.drop): the per-kernel sequence, not the fused region
            # (no DEVIAS recipe sets these rates; the region's GEMM epilogues carry no element mask)
            source = source or DropoutSource()
            E1 = E2 = None
            if p_drop > 0:
                M, D = x.shape
                E1 = source.element_mask("proj", index, (M, D), 1.0 - p_drop, x.device)
                E2 = source.element_mask("mlp", index, (M, D), 1.0 - p_drop, x.device)
                if ds1 is not None:                                           # drop_path(dropout(.)): one mask carries both factors
                    E1 = (E1.view(B, N, D) * ds1.view(B, 1, 1)).view(M, D).contiguous()
                    E2 = (E2.view(B, N, D) * ds2.view(B, 1, 1)).view(M, D).contiguous()
                    ds1 = ds2 = None
            adrop = (1.0 - p_attn, source.attn_seed(index)) if p_attn > 0 else None
            return EncoderBlockFn.apply(*args, ds1, ds2, (E1, E2, adrop))
        if _REGIONS and _INFER and ds1 is None and not torch.is_grad_enabled():
            # nobody will ask for a backward (validation_one_epoch, final_test*, feature extraction): no arena, nothing saved; bitwise the region's output
            x = x.contiguous()
            return self.run_infer(x, torch.empty_like(x), B, N, cdt, _use_q_prescale(cdt))
        return (EncoderBlockRegionFn if _REGIONS else EncoderBlockFn).apply(*args, ds1, ds2)


    def run_infer(self, x, x2, B, N, cdt, q_prescale):
        """x [rows, D] -> x2 [rows, D], rows >= B * N, by one devias_encoder_block_infer call (ops.encoder_block_infer); q_prescale: the qkv GEMM runs on the q-scaled
        copies of its weight and bias, as the training forward's does (the teacher keeps none)"""
        a = self.attn
        D = x.shape[1]
        qkv_bias = _WCACHE.qkv_bias(a.q_bias, a.v_bias)
        qs = (_WCACHE.get_qscaled(a.qkv.weight, D, _Q_PRESCALE, cdt), _WCACHE.get_qscaled(qkv_bias, D, _Q_PRESCALE, torch.float32)) if q_prescale else None
        return ops.encoder_block_infer(x, x2, B, N, a.num_heads, self.norm1.eps,
                                       (_f32(self.norm1.weight), _f32(self.norm1.bias), _f32(self.norm2.weight), _f32(self.norm2.bias)),
                                       tuple(_WCACHE.get(w, cdt) for w in (a.qkv.weight, a.proj.weight, self.mlp.fc1.weight, self.mlp.fc2.weight)),
                                       (qkv_bias, _f32(a.proj.bias), _f32(self.mlp.fc1.bias), _f32(self.mlp.fc2.bias)), qs)


class PatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, num_frames=16, tubelet_size=2):
        super().__init__()
        img_size = (img_size, img_size) if not isinstance(img_size, (tuple, list)) else tuple(img_size)
        patch_size = (patch_size, patch_size) if not isinstance(patch_size, (tuple, list)) else tuple(patch_size)
        self.tubelet_size = int(tubelet_size)
        self.num_patches = (img_size[1] // patch_size[1]) * (img_size[0] // patch_size[0]) * (num_frames // self.tubelet_size)
        self.img_size = img_size
        self.patch_size = patch_size
        self.proj = nn.Conv3d(in_channels=in_chans, out_channels=embed_dim,
                              kernel_size=(self.tubelet_size, patch_size[0], patch_size[1]),
                              stride=(self.tubelet_size, patch_size[0], patch_size[1]))


class MLPHead(nn.Module):
    """parameter container of the reference's MLPHead (model/modeling_slot.py:23-34): fc1 -> ReLU -> fc2; the arithmetic runs in HeadMlpFn"""

    def __init__(self, in_dim, out_dim, hidden_dim):
        super().__init__()
        self.fc1 = nn.Linear(in_dim, hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, out_dim)
        self.act = nn.ReLU()


class MaskPredictor(nn.Module):
    def __init__(self, dim=768, out=196):
        super().__init__()
        self.decoder = nn.Sequential(nn.Linear(dim, 512), nn.ReLU(), nn.Linear(512, 256), nn.ReLU(), nn.Linear(256, out),
                                     nn.Sigmoid())
        self.act = nn.ReLU()


class PreNorm(nn.Module):
    def __init__(self, dim, fn, context_dim=None):
        super().__init__()
        self.fn = fn
        self.norm = nn.LayerNorm(dim)
        self.norm_context = nn.LayerNorm(context_dim) if context_dim is not None else None


class FeedForward(nn.Module):
    def __init__(self, dim, mult=4, dropout=0.):
        super().__init__()
        self.activation = nn.GELU()
        self.net = nn.Sequential(nn.Linear(dim, int(dim * mult)), self.activation, nn.Dropout(dropout),
                                 nn.Linear(int(dim * mult), dim), nn.Identity())


class SlotAttention(nn.Module):
    """agg_block/attention.py:85-141 (class `Attention` there)."""

    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        inner_dim = dim_head * heads
        context_dim = context_dim if context_dim is not None else query_dim
        self.heads, self.dim_head = heads, dim_head
        self.to_q = nn.Linear(query_dim, inner_dim, bias=False)
        self.to_k = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_v = nn.Linear(context_dim, inner_dim, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner_dim, query_dim), nn.Dropout(dropout))


class AggregationBlock(nn.Module):
    """agg_block/agg_block.py:8-139 with the DEVIAS settings (learned queries, pre-norm, GELU FF x4, no pos-enc, last LN)."""

    def __init__(self, *, depth=4, input_channels=768, num_latents=4, latent_dim=768, weight_tie_layers=True, ff_mult=4):
        super().__init__()
        self.num_latents, self.latent_dim, self.input_dim = num_latents, latent_dim, input_channels
        self.depth, self.weight_tie_layers = depth, weight_tie_layers
        self.heads, self.dim_head = 4, 512                                        # agg_block.py:83
        self.latents = nn.Parameter(torch.randn(num_latents, latent_dim))         # agg_block.py:62
        mk_attn = lambda: PreNorm(latent_dim, SlotAttention(latent_dim, input_channels, heads=self.heads, dim_head=self.dim_head),
                                  context_dim=input_channels)
        mk_ff = lambda: PreNorm(latent_dim, FeedForward(latent_dim, mult=ff_mult))
        self.layers = nn.ModuleList([])
        cached = None
        for _ in range(depth):
            if weight_tie_layers:
                cached = cached or (mk_attn(), mk_ff())            # cache_fn: the SAME module objects every layer
                a, f = cached
            else:
                a, f = mk_attn(), mk_ff()
            self.layers.append(nn.ModuleList([a, nn.Identity(), f, nn.Identity()]))
        self.last_layer = nn.Sequential(nn.LayerNorm(latent_dim))

    def layer_params(self) -> List[torch.Tensor]:
        out = []
        for l in range(1 if self.weight_tie_layers else self.depth):
            a, _, f, _ = self.layers[l]
            out += [a.fn.to_q.weight, a.fn.to_k.weight, a.fn.to_v.weight, a.fn.to_out[0].weight, a.fn.to_out[0].bias,
                    a.norm.weight, a.norm.bias, a.norm_context.weight, a.norm_context.bias,
                    f.fn.net[0].weight, f.fn.net[0].bias, f.fn.net[3].weight, f.fn.net[3].bias, f.norm.weight, f.norm.bias]
        return out


class VisionTransformer(nn.Module):
    """Slot-DEVIAS student (model/modeling_slot.py:219-413).  Extra kwarg: compute_dtype in {'bf16', 'fp32'}."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4., qkv_bias=False, qk_scale=None, fc_drop_rate=0., drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., norm_layer=nn.LayerNorm, init_values=0., use_learnable_pos_emb=False, init_scale=0.,
                 all_frames=16, tubelet_size=2, use_checkpoint=False, num_latents=4, head_type='linear',
                 slot_matching_method='hard_select', num_scene_classes=365, agg_weights_tie=False, agg_depth=4,
                 slot_matching=None, compute_dtype='bf16'):
        super().__init__()
        if slot_matching is not None:          # the reference's driver passes this misspelt kwarg (run_slot_finetuning.py:386)
            slot_matching_method = slot_matching
        if slot_matching_method not in ('hard_select', 'matching'):
            raise ValueError("incorrent slot_matching_method")
        if head_type not in ('linear', 'mlp'):
            raise ValueError(f"head_type must be 'linear' or 'mlp' (modeling_slot.py:300-313), got {head_type!r}")
        for nm, v in (("fc_drop_rate", fc_drop_rate), ("drop_rate", drop_rate), ("attn_drop_rate", attn_drop_rate)):
            if not 0.0 <= float(v) < 1.0:
                raise ValueError(f"{nm} must be in [0, 1), got {v}")
        self.dropout_source = None             # None: DropoutSource() (torch's generators); tests install one with given masks
        if use_learnable_pos_emb:
            raise NotImplementedError("learnable pos-emb is not used by DEVIAS (sinusoid table only)")
        self.num_slots = num_latents
        self.num_classes = num_classes
        self.num_scene_classes = num_scene_classes
        self.num_features = self.embed_dim = embed_dim
        self.tubelet_size = tubelet_size
        self.patch_embed = PatchEmbed(img_size=img_size, patch_size=patch_size, in_chans=in_chans, embed_dim=embed_dim,
                                      num_frames=all_frames, tubelet_size=tubelet_size)
        num_patches = self.patch_embed.num_patches
        self.use_checkpoint = use_checkpoint   # accepted and ignored: no activation checkpointing is needed in 288 GB
        self.slot_matching_method = slot_matching_method
        self.head_type = head_type
        self.select_slots_info = [[0, 0] for _ in range(self.num_slots)]
        self.pos_embed = get_sinusoid_encoding_table(num_patches, embed_dim)     # plain attribute, not in state_dict
        self._pos_cache = {}
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, depth)]
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate,
                  attn_drop=attn_drop_rate, drop_path=dpr[i], norm_layer=norm_layer, init_values=init_values)
            for i in range(depth)])
        self.norm = norm_layer(embed_dim)
        self.fc_drop_rate = float(fc_drop_rate)
        self.fc_dropout = nn.Dropout(p=fc_drop_rate) if fc_drop_rate > 0 else nn.Identity()     # parameter container as in the reference (:291); applied in HeadRegionFn
        self.agg_block = AggregationBlock(num_latents=num_latents, weight_tie_layers=agg_weights_tie, depth=agg_depth,
                                          input_channels=embed_dim, latent_dim=embed_dim)
        grid = (img_size // patch_size) if not isinstance(img_size, (tuple, list)) else (img_size[0] // patch_size)
        self.mask_predictor = MaskPredictor(embed_dim, grid * grid)
        if head_type == 'linear':                                                # modeling_slot.py:300-305
            self.head = nn.Linear(embed_dim, num_classes + num_scene_classes) if num_classes > 0 else nn.Identity()
            nn.init.trunc_normal_(self.head.weight, std=.02)
            self.apply(self._init_weights)
            self.head.weight.data.mul_(init_scale)
            self.head.bias.data.mul_(init_scale)
        else:                                                                     # 'mlp': modeling_slot.py:306-313
            self.head = MLPHead(embed_dim, num_classes + num_scene_classes, hidden_dim=512) if num_classes > 0 else nn.Identity()
            nn.init.trunc_normal_(self.head.fc1.weight, std=.02)
            nn.init.trunc_normal_(self.head.fc2.weight, std=.02)
            self.apply(self._init_weights)
            self.head.fc2.weight.data.mul_(init_scale)
            self.head.fc2.bias.data.mul_(init_scale)
        self.set_compute_dtype(compute_dtype)

    # ---- reference surface -------------------------------------------------------------------------------
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

    def get_select_slot_info(self):
        print("action slot : " + " | ".join(str(s[0]) for s in self.select_slots_info))
        print("scene slot : " + " | ".join(str(s[1]) for s in self.select_slots_info))

    def reset_select_slot_info(self):
        self.select_slots_info = [[0, 0] for _ in range(self.num_slots)]

    def set_compute_dtype(self, compute_dtype):
        table = {'bf16': torch.bfloat16, 'bfloat16': torch.bfloat16, torch.bfloat16: torch.bfloat16,
                 'fp32': torch.float32, 'float32': torch.float32, torch.float32: torch.float32}
        if compute_dtype not in table:
            raise ValueError(f"compute_dtype must be 'bf16' or 'fp32', got {compute_dtype!r}")
        self.compute_dtype = table[compute_dtype]
        return self

    # ---- forward -----------------------------------------------------------------------------------------
    def _pos(self, device, dtype):
        key = (str(device), dtype)
        if key not in self._pos_cache:
            self._pos_cache[key] = self.pos_embed[0].to(device=device, dtype=dtype).contiguous()
        return self._pos_cache[key]

    def _prep_input(self, x):
        if not x.is_cuda:
            raise RuntimeError("devias_amd.VisionTransformer runs on an MI355X only (HIP kernels; no CPU fallback): "
                               "move the model and the input to cuda")
        B, C, T, H, W = x.shape
        assert H == self.patch_embed.img_size[0] and W == self.patch_embed.img_size[1], \
            f"Input image size ({H}*{W}) doesn't match model ({self.patch_embed.img_size[0]}*{self.patch_embed.img_size[1]})."
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()          # fp16 clips (samples.half(), engine_for_slot.py:108) are widened losslessly
        return x.contiguous()

    def forward_features(self, x, return_attn=False):
        if return_attn:
            raise NotImplementedError("per-block attention maps are never materialised by the fused MHSA kernel")
        x = self._prep_input(x)
        B = x.shape[0]
        N = self.patch_embed.num_patches
        cdt = self.compute_dtype
        pe = self.patch_embed
        h = PatchEmbedFn.apply(x, pe.proj.weight, pe.proj.bias, self._pos(x.device, cdt), (pe.tubelet_size, pe.patch_size[0], cdt))
        src = self.dropout_source or DropoutSource()
        if self.training and self.pos_drop.p > 0:                                 # pos_drop (modeling_slot.py:280,356)
            h = DropMaskFn.apply(h, src.element_mask("pos", -1, tuple(h.shape), 1.0 - float(self.pos_drop.p), h.device))
        for i, blk in enumerate(self.blocks):
            h = blk.run(h, B, N, cdt, i, src)
        return h          # [B*N, D], BEFORE the final LayerNorm (it is fused into AggBlockFn)

    def _aggregate(self, h, B):
        """final LayerNorm + aggregation block on the encoder's output h [B*N, D] -> (slots [B*S, D], the last layer's slot softmax); shared with the downstream model"""
        N, D, cdt = self.patch_embed.num_patches, self.embed_dim, self.compute_dtype
        ab = self.agg_block
        S = ab.num_latents
        meta = (B, N, S, ab.depth, ab.weight_tie_layers, ab.heads, ab.dim_head, self.norm.eps, ab.last_layer[0].eps, cdt)
        fold = _AGG_FOLD and S <= 4 and D in (384, 512, 768, 1024)
        return ((AggBlockRegionFn if _REGIONS else AggBlockFoldFn) if fold else AggBlockFn).apply(h, self.norm.weight, self.norm.bias, ab.latents, ab.last_layer[0].weight,
                                                                                                ab.last_layer[0].bias, meta, *ab.layer_params())

    def forward(self, x, return_attn=False):
        B = x.shape[0]
        N = self.patch_embed.num_patches
        D = self.embed_dim
        cdt = self.compute_dtype
        h = self.forward_features(x, return_attn)
        S = self.agg_block.num_latents
        slots, attn = self._aggregate(h, B)
        if self.slot_matching_method == 'hard_select':
            raise NotImplementedError("only slot_matching_method='matching' is on the DEVIAS training path "
                                      "(the reference's hard_select branch returns empty lists, modeling_slot.py:388)")
        mp = self.mask_predictor.decoder
        drop_mask = None
        if self.training and self.fc_drop_rate > 0:
            # nn.Dropout(fc_drop_rate) on the head's input only (modeling_slot.py:393): element-wise Bernoulli(keep) / keep, drawn like drop_path's masks
            keep = 1.0 - self.fc_drop_rate
            drop_mask = ((keep + torch.rand((B * S, D), device=x.device, dtype=torch.float32)).floor() / keep).contiguous()
        if self.head_type == 'mlp':
            slots_head, mask_predictions = HeadMlpFn.apply(slots, self.head.fc1.weight, self.head.fc1.bias, self.head.fc2.weight, self.head.fc2.bias,
                                                           mp[0].weight, mp[0].bias, mp[2].weight, mp[2].bias, mp[4].weight, mp[4].bias, cdt, drop_mask)
        else:
            head_fn = HeadRegionFn if (_REGIONS or drop_mask is not None) else HeadFn
            head_args = (slots, self.head.weight, self.head.bias, mp[0].weight, mp[0].bias, mp[2].weight, mp[2].bias, mp[4].weight, mp[4].bias, cdt)
            slots_head, mask_predictions = head_fn.apply(*head_args, drop_mask) if drop_mask is not None else head_fn.apply(*head_args)
        idx = ops.slot_select(slots_head.detach(), B, S, self.num_classes).long()      # modeling_slot.py:395-401
        ar = torch.arange(B, device=x.device)
        sv, hv = slots.view(B, S, D), slots_head.view(B, S, -1)
        action_feat, scene_feat = sv[ar, idx[:, 0]], sv[ar, idx[:, 1]]
        action_logit, scene_logit = hv[ar, idx[:, 0]], hv[ar, idx[:, 1]]
        return (action_feat, scene_feat), (action_logit, scene_logit, attn), (slots_head, slots, mask_predictions)


@register_model
def slot_vit_base_patch16_224(pretrained=False, **kwargs):
    model = VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True,
                              norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
    model.default_cfg = _cfg()
    return model


@register_model
def slot_vit_small_patch16_224(pretrained=False, **kwargs):
    """not in the reference (its wrapper hard-wires 768); needed by BASELINE config 1"""
    model = VisionTransformer(patch_size=16, embed_dim=384, depth=12, num_heads=6, mlp_ratio=4, qkv_bias=True,
                              norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
    model.default_cfg = _cfg()
    return model


@register_model
def slot_vit_large_patch16_224(pretrained=False, **kwargs):
    """not in the reference; BASELINE config 4 (D=1024, 24 blocks, 16 heads)"""
    model = VisionTransformer(patch_size=16, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, qkv_bias=True,
                              norm_layer=partial(nn.LayerNorm, eps=1e-6), **kwargs)
    model.default_cfg = _cfg()
    return model
