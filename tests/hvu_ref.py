"""Plain-PyTorch CPU restatement of the HVU recipe's loss and FAME label routing (test infrastructure, beside oracle/ref_cpu.py, which it
reuses for the assignment).  tests/golden/make_hvu_goldens.py checks both against the real reference classes; the tests then use them at
shapes the fixtures do not cover.  References are `file:line` of the reference repository."""
import torch
import torch.nn.functional as F

from oracle.ref_cpu import match_slots

LOSS_NAMES = ("action_loss", "scene_loss", "cosine_loss", "mask_prediction_loss", "mask_distill_loss")


def hvu_train_loss(student_output, action_targets, scene_targets, fg_mask, num_action_classes=739, scene_criterion="KL",
                   mask_prediction_loss_weight=1.0, mask_distill_loss_weight=1.0):
    """TrainLoss.forward of utils/loss/hvu_train_loss.py:27-128 ('matching').  `scene_targets` are class indices in [0, ns) and are NOT
    mutated (the reference offsets the caller's tensor in place, :45-46).
    Returns (total_loss[1], matched action logits [B,C], dict of 5 floats, (i*, j*) index tensors)."""
    _, (_, _, attn), (slots_head, slots, mask_predictions) = student_output
    bs = action_targets.shape[0]
    S = slots_head.shape[0] // bs                                         # :38
    nh = attn.shape[0] // bs                                              # :39
    C = slots_head.shape[1]
    nb = num_action_classes
    Ahat = attn.reshape(bs, nh, S, -1).mean(dim=1)                        # :42
    M = mask_predictions.reshape(bs, S, -1)                               # :43
    scene_target = scene_targets + nb                                     # :45-46, out of place
    p = slots_head.softmax(-1).detach().reshape(bs, S, C)                 # :48
    Z = slots_head.view(bs, S, C)                                         # :70
    fg196, fgN = fg_mask
    act = slots_head.new_zeros(1); scn = slots_head.new_zeros(1)
    mp = slots_head.new_zeros(1); md = slots_head.new_zeros(1)
    rows, ii, jj = [], [], []
    for b in range(bs):
        cost = torch.stack([-p[b, :, action_targets[b]], -p[b, :, scene_target[b]]], dim=1)       # :53-57
        if S == 1:                                                        # a 1 x 2 cost matrix assigns the one slot to its cheaper column (:60)
            i = j = 0
        else:
            i, j = match_slots(cost)                                      # :60
        ii.append(i); jj.append(j)
        md = md + F.mse_loss(Ahat[b, i], fgN[b]) * mask_distill_loss_weight                          # :84
        mp = mp + F.binary_cross_entropy_with_logits(M[b, i], fg196[b]) * mask_prediction_loss_weight  # :85-88
        act = act + F.cross_entropy(Z[b, i], action_targets[b])                                      # :89
        rows.append(Z[b, i])
        if scene_criterion == "CE":
            scn = scn + F.cross_entropy(Z[b, j], scene_target[b])                                     # :94
        elif scene_criterion == "KL":
            log_prob = F.log_softmax(Z[b, j].unsqueeze(0), dim=1)                                     # :97-101: [1, C] input, 'batchmean' divides by 1
            onehot = torch.zeros_like(log_prob).scatter_(1, scene_target[b].view(1, 1), 1)
            scn = scn + F.kl_div(log_prob, onehot, reduction="batchmean")
        else:
            raise ValueError(scene_criterion)
    act, scn, mp, md = act / bs, scn / bs, mp / bs, md / bs                                          # :105-108
    if S > 1:
        sl = F.normalize(slots.reshape(bs, S, -1), p=2, dim=2)                                       # :110-119
        cs = torch.bmm(sl, sl.transpose(1, 2)) * (1 - torch.eye(S, dtype=sl.dtype))
        cos = (cs.sum(dim=(1, 2)) / (S * (S - 1))).mean()
    else:
        cos = slots.new_zeros(())                                         # one slot has no pair (the reference would divide by S - 1 = 0)
    total = act + scn + cos + mp + md                                                                # :121
    ld = {"action_loss": act.item(), "scene_loss": scn.item(), "cosine_loss": cos.item(), "mask_prediction_loss": mp.item(),
          "mask_distill_loss": md.item()}
    return total, torch.stack(rows), ld, (torch.tensor(ii), torch.tensor(jj))


def fame_hvu_labels(action_label, scene_label, perm, rand, prob_aug):
    """labels out of utils/transform/fame_hvu.py:126-141 given its two random draws (`perm` = torch.randperm, :123; `rand` = torch.rand, :130):
    an augmented clip keeps its action label and takes the scene label of the clip whose background it received"""
    fused_scene = scene_label[perm]                                       # :127
    if prob_aug < 1:
        aug, ori = torch.where(rand < prob_aug)[0], torch.where(rand >= prob_aug)[0]                 # :131-132
        return torch.cat([action_label[aug], action_label[ori]]), torch.cat([fused_scene[aug], scene_label[ori]])   # :134-135
    return action_label, scene_label                                      # :140-141


def fame_route_table(perm, rand, prob_aug):
    """(src, partner, aug) per output row -- what devias_amd.fame.FAME._mix hands the mixing kernel -- from the same two draws"""
    B = perm.shape[0]
    if prob_aug < 1:
        aug_ind, ori_ind = torch.where(rand < prob_aug)[0], torch.where(rand >= prob_aug)[0]
        src = torch.cat([aug_ind, ori_ind])
        aug = torch.cat([torch.ones_like(aug_ind), torch.zeros_like(ori_ind)])
    else:
        src, aug = torch.arange(B), torch.ones(B, dtype=torch.int64)
    return src, perm[src], aug
