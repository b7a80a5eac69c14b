"""The HVU recipe (ground-truth scene labels, no scene teacher) without a GPU: tests/hvu_ref.py against what the reference's own
utils/loss/hvu_train_loss.py and utils/transform/fame_hvu.py returned (tests/golden/hvu_loss.npz, fame_hvu_t8.npz, made by
tests/golden/make_hvu_goldens.py), the C-ABI surface of the two label entry points and their argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import golden_util as gu
import hvu_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB, NS = 739, 248
LEAVES = ("slots_head", "slots", "maskp", "attn")


def _loss_fixture(S):
    fx = dict(np.load(gu.GOLDEN_DIR + "/hvu_loss.npz"))
    t = {k: torch.from_numpy(fx[f"s{S}.{k}"]) for k in LEAVES + ("target", "scene_target", "fg", "fgN")}
    return fx, t


@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("crit", ["KL", "CE"])
def test_hvu_ref_matches_reference_golden(S, crit):
    """values, match and gradients, to the tolerances of test_oracle_loss_criteria_match_reference_golden; the caller's scene labels stay as they are"""
    fx, t = _loss_fixture(S)
    lv = {k: t[k].clone().requires_grad_(True) for k in LEAVES}
    out = (None, (None, None, lv["attn"]), (lv["slots_head"], lv["slots"], lv["maskp"]))
    ys = t["scene_target"].clone()
    total, logits, ld, idx = hvu_ref.hvu_train_loss(out, t["target"], ys, (t["fg"], t["fgN"]), num_action_classes=NB, scene_criterion=crit,
                                                    mask_prediction_loss_weight=1.0, mask_distill_loss_weight=3.0)
    assert torch.equal(ys, t["scene_target"]) and int(ys.max()) < NS                 # not offset in place (the reference does: hvu_train_loss.py:45-46)
    total.backward()
    pre = f"s{S}.{crit}."
    assert abs(float(total.detach()) - float(fx[pre + "total"])) < 1e-5 * abs(float(fx[pre + "total"]))
    assert np.allclose([ld[k] for k in hvu_ref.LOSS_NAMES], fx[pre + "losses"], rtol=1e-5, atol=1e-7)
    assert torch.stack(idx, dim=1).tolist() == fx[pre + "match"].tolist()
    assert gu.rel(logits.detach(), fx[f"s{S}.logits"]) < 1e-6
    for k in lv:
        assert gu.rel(lv[k].grad, fx[f"s{S}.d{k}"]) < 1e-5, k


@pytest.mark.parametrize("S", [2, 3, 4])
def test_kl_equals_ce_in_the_reference_fixture(S):
    """against a one-hot target kl_div(..., 'batchmean') on a [1, C] input is the cross-entropy (hvu_train_loss.py:94, :96-101)"""
    fx, _ = _loss_fixture(S)
    assert abs(float(fx[f"s{S}.KL.total"]) - float(fx[f"s{S}.CE.total"])) <= 1e-6 * abs(float(fx[f"s{S}.CE.total"]))
    assert np.allclose(fx[f"s{S}.KL.losses"], fx[f"s{S}.CE.losses"], rtol=1e-6, atol=0)
    assert fx[f"s{S}.KL.match"].tolist() == fx[f"s{S}.CE.match"].tolist()
    m = fx[f"s{S}.KL.match"]
    assert (m[:, 0] != m[:, 1]).all() and len({tuple(r) for r in m.tolist()}) > 1       # the fixture exercises more than one assignment


def test_fame_hvu_label_routing_matches_reference_golden():
    """an augmented clip keeps its action label and takes the scene label of the clip whose background it received (fame_hvu.py:126-135); the masks are
    fame.py's, bit for bit.  devias_amd.fame.route_hvu_labels is index arithmetic and runs here on the CPU."""
    from devias_amd.fame import FAMEHVU, route_hvu_labels
    fx = dict(np.load(gu.GOLDEN_DIR + "/fame_hvu_t8.npz"))
    base = dict(np.load(gu.GOLDEN_DIR + "/fame_t8.npz"))
    assert np.array_equal(fx["mask"], base["mask"]) and np.array_equal(fx["masks_per_frame"], base["masks_per_frame"])
    assert np.array_equal(fx["rand"], base["rand"]) and np.array_equal(fx["perm"], base["perm"]) and np.array_equal(fx["action_label"], base["label"])
    assert np.array_equal(fx["out_action_label"], base["out_label"])
    a, s = torch.from_numpy(fx["action_label"]), torch.from_numpy(fx["scene_label"])
    perm, rand, prob = torch.from_numpy(fx["perm"]), torch.from_numpy(fx["rand"]), float(fx["prob_aug"])
    oa, os_ = hvu_ref.fame_hvu_labels(a, s, perm, rand, prob)
    assert oa.tolist() == fx["out_action_label"].tolist() and os_.tolist() == fx["out_scene_label"].tolist()
    src, partner, aug = hvu_ref.fame_route_table(perm, rand, prob)
    ra, rs = route_hvu_labels(a, s, src.int(), partner.int(), aug.int(), prob)
    assert ra.tolist() == fx["out_action_label"].tolist() and rs.tolist() == fx["out_scene_label"].tolist()
    assert fx["out_scene_label"].tolist() != fx["scene_label"][src.numpy()].tolist()     # the fixture does route a partner's scene label
    assert a.tolist() == fx["action_label"].tolist() and s.tolist() == fx["scene_label"].tolist()
    # prob_aug >= 1: the reference returns the scene labels as they came in (fame_hvu.py:138-141)
    src, partner, aug = hvu_ref.fame_route_table(perm, rand, 1.0)
    assert route_hvu_labels(a, s, src, partner, aug, 1.0)[1].tolist() == hvu_ref.fame_hvu_labels(a, s, perm, rand, 1.0)[1].tolist() == s.tolist()
    assert "FAME" in str(FAMEHVU(beta=0.5, prob_aug=0.5))


def test_label_entry_points_are_declared_exported_and_bound():
    from devias_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "devias_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int32_t|int64_t|void|const char\*)\s+(devias_\w+)\s*\(", hdr, flags=re.M))
    lib = _lib.load()
    for name in ("devias_head_match_loss_labels_fwd", "devias_head_match_loss_labels_bwd"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.devias_version() >= 168 and _lib.ABI_VERSION >= 168
    m = re.search(r"#define DEVIAS_CNT_LOSS_LABELS (\d+)", hdr)
    cnt_max = int(re.search(r"#define DEVIAS_CNT_MAX (\d+)", hdr).group(1))
    assert m and int(m.group(1)) == _lib.COUNTERS["loss_labels"] < cnt_max
    ids = [int(v) for v in re.findall(r"#define DEVIAS_CNT_(?!MAX)\w+ (\d+)", hdr)]
    assert len(ids) == len(set(ids))                                                   # the new counter took a free id
    # the teacher entry points and their struct are as they were
    assert _lib.PROTOTYPES["devias_head_match_loss_fwd"] == _lib.PROTOTYPES["devias_head_match_loss_labels_fwd"]
    assert ctypes.sizeof(_lib.LossDims) == 14 * 4


def _dims(**kw):
    from devias_amd import _lib
    d = _lib.LossDims()
    base = dict(B=2, S=2, C=NB + NS, nb=NB, ns=NS, D=8, G=4, N=6, nh=1, w_scene=0.0, w_mask_pred=1.0, w_mask_distill=1.0, dtype=_lib.F32, scene_ce=0)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_label_entry_points_validate_arguments_without_a_device():
    """null pointers, bad dims and a bad dtype return DEVIAS_EINVAL with a message before anything is launched; the counter moves only on a launch"""
    from devias_amd import _lib
    lib = _lib.load()
    lib.devias_counters_reset()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                       # a non-null host address: validation must refuse before any launch could read it
    fwd, bwd = lib.devias_head_match_loss_labels_fwd, lib.devias_head_match_loss_labels_bwd
    n_fwd, n_bwd = 12, 14                           # pointer arguments after `d` and before `stream`
    cases = [(None, "null dims")]
    cases += [(_dims(**kw), "bad dims") for kw in (dict(B=0), dict(S=0), dict(S=9), dict(C=NB + NS + 1), dict(nb=0, ns=NB + NS), dict(nb=NB + NS, ns=0),
                                                   dict(nb=-1, ns=NB + NS + 1), dict(D=0), dict(G=0), dict(N=0), dict(nh=0))]
    cases += [(_dims(dtype=7), "bad dtype")]
    for d, what in cases:
        ref = ctypes.byref(d) if d is not None else None
        assert fwd(ref, *([p] * n_fwd), None) == -1, what
        assert b"devias_head_match_loss_labels_fwd" in lib.devias_last_error() and what.encode() in lib.devias_last_error()
        assert bwd(ref, *([p] * n_bwd), None) == -1, what
        assert b"devias_head_match_loss_labels_bwd" in lib.devias_last_error() and what.encode() in lib.devias_last_error()
    d = _dims()
    for scene_ce in (0, 1):                         # both values are accepted; a null pointer in any position is not
        d.scene_ce = scene_ce
        for i in range(n_fwd):
            args = [p] * n_fwd
            args[i] = None
            assert fwd(ctypes.byref(d), *args, None) == -1 and b"labels_fwd: null pointer" in lib.devias_last_error(), i
        for i in range(n_bwd):
            args = [p] * n_bwd
            args[i] = None
            assert bwd(ctypes.byref(d), *args, None) == -1 and b"labels_bwd: null pointer" in lib.devias_last_error(), i
    assert lib.devias_counter(_lib.COUNTERS["loss_labels"]) == 0


def test_host_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from devias_amd import ops
    from devias_amd.hvu_train_loss import TrainLoss
    B, S = 2, 2
    Z, sl, mp, at = torch.zeros(B * S, NB + NS), torch.zeros(B * S, 8), torch.zeros(B * S, 4), torch.zeros(B, S, 6)
    y, ys, fg, fgN = torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), torch.zeros(B, 4), torch.zeros(B, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.head_match_loss_labels_fwd(Z, sl, mp, at, y, ys, fg, fgN, NB, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TrainLoss(None, "KL")((None, (None, None, at), (Z, sl, mp)), y, ys, fg_mask=(fg, fgN))
    with pytest.raises(ValueError, match="head width"):
        TrainLoss(None, "KL", num_action_classes=400)((None, (None, None, at), (Z, sl, mp)), y, ys, fg_mask=(fg, fgN))
    with pytest.raises(NotImplementedError):
        TrainLoss(None, "KL", slot_matching_method="hard_select")
    with pytest.raises(ValueError):
        TrainLoss(None, "MSE")
    c = TrainLoss(None, "CE", "matching", 2.0, 3.0)                                   # the reference's positional order (hvu_train_loss.py:12-13)
    assert (c.scene_criterion, c.mask_prediction_loss_weight, c.mask_distill_loss_weight, c.num_action_classes, c.num_scene_classes) == ("CE", 2.0, 3.0, NB, NS)
    assert not hasattr(c, "scene_loss_weight") and c.last_match is None and c.sync_loss_dict is True


def test_synth_scene_targets():
    from devias_amd import synth
    s = synth.scene_targets(64)
    assert s.dtype == torch.int64 and int(s.min()) >= 0 and int(s.max()) < NS and len(set(s.tolist())) > 16
    assert torch.equal(s, synth.scene_targets(64)) and torch.equal(synth.scene_targets(8, first=5), s[5:13])
    assert not torch.equal(s % 101, synth.targets(64, 101))                          # hashed on their own key
    assert int(synth.scene_targets(64, num_scene=2).max()) == 1
