"""Plain-PyTorch restatement of everything after the slots of the reference's downstream model (model/modeling_slot_fusion.py:23-53, 379-400) and of timm's
LabelSmoothingCrossEntropy, in whatever dtype the inputs have (the bound tests run it in float64; tools/downstream_time.py runs it eagerly on the GPU as the ATen
yardstick).  tests/golden/make_downstream_goldens.py checks it against the real reference while it writes downstream_t8.npz; a mismatch aborts.

P maps the reference's parameter names (`head.weight`, `action_norm.weight`, `fusion_head.fc_action_down.weight`, ...) to tensors."""
import torch
import torch.nn.functional as F

EPS_NORM, EPS_LN = 1e-6, 1e-5          # the model's norm_layer (partial(nn.LayerNorm, eps=1e-6)); plain nn.LayerNorm inside MLPHead
NO_GRAD_NAMES = ("head.weight", "head.bias", "fusion_head.fc_scene_down.weight", "fusion_head.fc_scene_down.bias", "fusion_head.fc_scene_ln.weight",
                 "fusion_head.fc_scene_ln.bias")


def select_idx(Z, B, S, nb):
    """idx [B, 2] alone: what the model computes (modeling_slot_fusion.py:383-389)"""
    p = torch.softmax(Z, dim=-1).view(B, S, -1)
    return torch.stack([torch.argmax(p[:, :, :nb].max(dim=-1).values, dim=1), torch.argmax(p[:, :, nb:].max(dim=-1).values, dim=1)], dim=1)


def select(Z, B, S, nb):
    """-> idx [B, 2] (action slot, scene slot; torch.argmax: first slot wins ties) and the relative gaps [B, 2] between the best and the runner-up slot
    (inf for S = 1) of `Z` [B*S, nb+ns]"""
    p = torch.softmax(Z, dim=-1).view(B, S, -1)
    ma, ms = p[:, :, :nb].max(dim=-1).values, p[:, :, nb:].max(dim=-1).values          # [B, S]
    idx = torch.stack([torch.argmax(ma, dim=1), torch.argmax(ms, dim=1)], dim=1)
    gaps = []
    for m in (ma, ms):
        if S == 1:
            gaps.append(torch.full((B,), float("inf"), dtype=m.dtype))
        else:
            top = m.topk(2, dim=1).values
            gaps.append((top[:, 0] - top[:, 1]) / top[:, 0])
    return idx, torch.stack(gaps, dim=1)


def fusion_forward(slots, P, nb, use_input_ln=True, drop_mask=None, idx=None, relu_mask=None, scene_down=False, eps_norm=EPS_NORM, eps_ln=EPS_LN, half_ln=True):
    """slots [B, S, D] -> dict(input [B, 2D], out [B, Cd], idx [B, 2], u [B, D], h, r [B, D]).
    idx: use this selection instead of the head's (the bound tests judge a backward on the SAVED forward); relu_mask: bool [B, D] to use instead of h > 0.
    scene_down / half_ln: the mutants of tests/fusion_bounds.py (fc_scene_* for the scene token; one LayerNorm over D instead of two over D/2)."""
    B, S, D = slots.shape
    if idx is None:
        Z = F.linear(slots.reshape(B * S, D).detach(), P["head.weight"].detach(), P["head.bias"].detach())
        idx = select_idx(Z, B, S, nb)
    ar = torch.arange(B, device=slots.device)
    a = F.layer_norm(slots[ar, idx[:, 0].long()], (D,), P["action_norm.weight"], P["action_norm.bias"], eps_norm)
    s = F.layer_norm(slots[ar, idx[:, 1].long()], (D,), P["scene_norm.weight"], P["scene_norm.bias"], eps_norm)
    inp = torch.cat([a, s], dim=1)
    f = "fusion_head."
    ua = F.linear(a, P[f + "fc_action_down.weight"], P[f + "fc_action_down.bias"])
    sd = "fc_scene" if scene_down else "fc_action"          # the reference sends BOTH tokens through fc_action_down / fc_action_ln (:43-44)
    us = F.linear(s, P[f + sd + "_down.weight"], P[f + sd + "_down.bias"])
    u = torch.cat([ua, us], dim=1)
    if half_ln:
        h = torch.cat([F.layer_norm(ua, (D // 2,), P[f + "fc_action_ln.weight"], P[f + "fc_action_ln.bias"], eps_ln),
                       F.layer_norm(us, (D // 2,), P[f + sd + "_ln.weight"], P[f + sd + "_ln.bias"], eps_ln)], dim=1)
    else:
        h = F.layer_norm(u, (D,), torch.cat([P[f + "fc_action_ln.weight"]] * 2), torch.cat([P[f + "fc_action_ln.bias"]] * 2), eps_ln)
    if use_input_ln:
        h = F.layer_norm(h, (D,), P[f + "fc_input_ln.weight"], P[f + "fc_input_ln.bias"], eps_ln)
    r = torch.relu(h) if relu_mask is None else h * relu_mask.to(h.dtype)
    if drop_mask is not None:
        r = r * drop_mask.to(r.dtype)
    out = F.linear(r, P[f + "classifier.weight"], P[f + "classifier.bias"])
    return {"input": inp, "out": out, "idx": idx, "u": u, "h": h, "r": r}


def label_smoothing_ce(z, y, smoothing=0.1):
    """timm.loss.LabelSmoothingCrossEntropy.forward"""
    logp = F.log_softmax(z, dim=-1)
    nll = -logp.gather(dim=-1, index=y.unsqueeze(1)).squeeze(1)
    smooth = -logp.mean(dim=-1)
    return ((1.0 - smoothing) * nll + smoothing * smooth).mean()
