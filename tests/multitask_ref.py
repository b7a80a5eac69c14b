"""Plain-PyTorch restatement of the reference's two-token multi-task baseline (model/modeling_multi_task.py:293-334) on oracle/ref_cpu.py's patch embedding and
encoder block, of the part after the encoder alone (two_token_head: what csrc/token_head.hip fuses; tools/multitask_time.py runs it eagerly on the GPU as the
ATen yardstick) and of the driver's TrainLoss (run_multi_task_finetuning.py:31-78).  tests/golden/make_multitask_goldens.py checks forward() and train_loss()
against the real reference while it writes the fixtures; a mismatch aborts.

P maps the reference's parameter names to tensors; dtype and device follow the inputs.  The unified head is the absence of "scene_head.weight" in P."""
import torch
import torch.nn.functional as F

from oracle import ref_cpu
from plainvit_ref import label_smoothing_ce  # noqa: F401  (timm's LabelSmoothingCrossEntropy, the driver's action criterion)

EPS = 1e-6          # the model's norm_layer: partial(nn.LayerNorm, eps=1e-6)


def two_token_head(h, P, mask_a=None, mask_s=None, eps=EPS):
    """h [B, Nt, D] (the encoder's output) -> ((action_token, action_logits), (scene_token, scene_logits)): norm(h)[:, 0] and norm(h)[:, -1], the two fc_dropout
    masks (0 or 1 / keep), head and scene_head (or head for both)"""
    D = h.shape[-1]
    y = F.layer_norm(h, (D,), P["norm.weight"], P["norm.bias"], eps)
    ta, ts = y[:, 0], y[:, -1]
    aa = ta * mask_a.to(ta.dtype) if mask_a is not None else ta
    as_ = ts * mask_s.to(ts.dtype) if mask_s is not None else ts
    sw, sb = (P["scene_head.weight"], P["scene_head.bias"]) if "scene_head.weight" in P else (P["head.weight"], P["head.bias"])
    return (ta, F.linear(aa, P["head.weight"], P["head.bias"])), (ts, F.linear(as_, sw, sb))


def encode(P, cfg, x):
    """patch embedding, cat(cls, patches, scene), then + pos (:294-301), the blocks -> h [B, N + 2, D]"""
    h = ref_cpu.patch_embed(P, cfg, x)
    B = h.shape[0]
    h = torch.cat([P["cls_token"].expand(B, -1, -1).to(h.dtype), h, P["scene_token"].expand(B, -1, -1).to(h.dtype)], dim=1)
    h = h + ref_cpu.sinusoid_table(h.shape[1], cfg.embed_dim).to(h.dtype)
    for i in range(cfg.depth):
        h = ref_cpu.encoder_block(P, cfg, i, h)
    return h


def forward(P, cfg, x, mask_a=None, mask_s=None):
    return two_token_head(encode(P, cfg, x), P, mask_a, mask_s, cfg.eps_encoder)


def distill(scene_logit, teacher, logit_criterion, pad=0, weight=1.0):
    """the scene term (:48-68): teacher [B, Ct] left-padded with `pad` columns of (its global minimum - 1); 'KL' (batchmean, log_target) times `weight`, or 'CE'
    against the padded teacher's argmax, without the weight"""
    if pad:
        fill = torch.full((teacher.shape[0], pad), float(teacher.min()) - 1.0, dtype=teacher.dtype, device=teacher.device)
        teacher = torch.cat([fill, teacher], dim=1)
    if logit_criterion == "CE":
        return F.cross_entropy(scene_logit, torch.argmax(teacher, dim=1))
    if logit_criterion == "KL":
        return F.kl_div(F.log_softmax(scene_logit, dim=-1), F.log_softmax(teacher, dim=-1), reduction="batchmean", log_target=True) * weight
    raise NotImplementedError(logit_criterion)


def train_loss(action_logit, scene_logit, teacher, target, smoothing, logit_criterion, unified_head=False, num_action_classes=400, weight=1.0):
    """-> (total, action_loss, logit_loss)"""
    action = label_smoothing_ce(action_logit, target, smoothing)
    logit = distill(scene_logit, teacher, logit_criterion, num_action_classes if unified_head else 0, weight)
    return action + logit, action, logit
