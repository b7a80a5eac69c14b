"""Plain-PyTorch restatement of the reference's plain video ViT (model/modeling_finetune.py:273-325) in both pool modes, on oracle/ref_cpu.py's patch embedding and
encoder block, and of the part after the encoder alone (pool_head: what csrc/token_head.hip fuses; tools/plainvit_time.py runs it eagerly on the GPU as the ATen
yardstick).  tests/golden/make_plainvit_goldens.py checks forward() against the real reference while it writes the fixtures; a mismatch aborts.

P maps the reference's parameter names to tensors; dtype and device follow the inputs."""
import torch
import torch.nn.functional as F

from oracle import ref_cpu

EPS = 1e-6          # the model's norm_layer: partial(nn.LayerNorm, eps=1e-6)


def pool_head(h, P, mean_pooling, drop_mask=None, eps=EPS):
    """h [B, Nt, D] (the encoder's output) -> (token [B, D], logits [B, C]): fc_norm(h.mean(1)) or norm(h)[:, 0], the fc_dropout mask (0 or 1 / keep), head"""
    D = h.shape[-1]
    if mean_pooling:
        token = F.layer_norm(h.mean(1), (D,), P["fc_norm.weight"], P["fc_norm.bias"], eps)
    else:
        token = F.layer_norm(h, (D,), P["norm.weight"], P["norm.bias"], eps)[:, 0]
    a = token * drop_mask.to(token.dtype) if drop_mask is not None else token
    return token, F.linear(a, P["head.weight"], P["head.bias"])


def encode(P, cfg, x, mean_pooling):
    """patch embedding, the cls row in cls-token mode (cls FIRST, then + pos: :277-283), the blocks -> h [B, Nt, D]"""
    h = ref_cpu.patch_embed(P, cfg, x)
    B = h.shape[0]
    if not mean_pooling:
        h = torch.cat([P["cls_token"].expand(B, -1, -1).to(h.dtype), h], dim=1)
    h = h + ref_cpu.sinusoid_table(h.shape[1], cfg.embed_dim).to(h.dtype)
    for i in range(cfg.depth):
        h = ref_cpu.encoder_block(P, cfg, i, h)
    return h


def forward(P, cfg, x, mean_pooling, drop_mask=None):
    return pool_head(encode(P, cfg, x, mean_pooling), P, mean_pooling, drop_mask, cfg.eps_encoder)


def label_smoothing_ce(z, y, eps):
    """timm.loss.LabelSmoothingCrossEntropy(eps)"""
    lp = F.log_softmax(z, dim=-1)
    return ((1.0 - eps) * -lp.gather(1, y.view(-1, 1)).squeeze(1) + eps * -lp.mean(-1)).mean()
