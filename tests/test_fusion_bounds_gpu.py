"""devias_fusion_head_fwd / _bwd and devias_softmax_ce_fwd / _bwd on the GPU against float64, element by element, under the bounds of tests/fusion_bounds.py
(head level, no encoder).  The backward's reference takes the ReLU mask from the kernel's stored r and idx from the stored idx; no element is excluded anywhere."""
import ctypes

import pytest
import torch

import fusion_bounds as fb

pytestmark = pytest.mark.gpu
f = fb.f
DEV = "cuda"

PARAM_ORDER = ("head.weight", "head.bias", "action_norm.weight", "action_norm.bias", "scene_norm.weight", "scene_norm.bias", f + "fc_action_down.weight",
               f + "fc_action_down.bias", f + "fc_action_ln.weight", f + "fc_action_ln.bias", f + "fc_input_ln.weight", f + "fc_input_ln.bias",
               f + "classifier.weight", f + "classifier.bias")


def _al(n):
    return (n + 255) // 256 * 256


def run_direct(slots, P, nb, use_in, mask, dout, dinp, dtype, no_save=False):
    """one devias_fusion_head_fwd and one _bwd call through ctypes on buffers of exactly the queried sizes -> outputs, gradients and the stored r;
    no_save: the forward alone with save = NULL (u, r and the statistics in the workspace) -> input, out, idx"""
    from devias_amd import _lib, ops
    lib = _lib.load()
    B, S, D = slots.shape
    C, Cd = P["head.weight"].shape[0], P[f + "classifier.weight"].shape[0]
    dt = ops.dt_code(dtype)
    es = 2 if dtype == torch.bfloat16 else 4
    dev = {k: (v.to(DEV, dtype) if v.dim() == 2 else v.to(DEV)).contiguous() for k, v in P.items()}
    a = _lib.FusionArgs()
    a.struct_size = ctypes.sizeof(_lib.FusionArgs)
    a.B, a.S, a.D, a.nb, a.ns, a.Cd, a.dtype, a.use_input_ln = B, S, D, nb, C - nb, Cd, dt, int(use_in)
    a.eps_norm, a.eps_ln = 1e-6, 1e-5
    a.Wh, a.Wd, a.Wc = (dev[k].data_ptr() for k in ("head.weight", f + "fc_action_down.weight", f + "classifier.weight"))
    a.bh, a.an_w, a.an_b, a.sn_w, a.sn_b, a.bd, a.ln_w, a.ln_b, a.bc = (dev[k].data_ptr() for k in (
        "head.bias", "action_norm.weight", "action_norm.bias", "scene_norm.weight", "scene_norm.bias", f + "fc_action_down.bias", f + "fc_action_ln.weight",
        f + "fc_action_ln.bias", f + "classifier.bias"))
    if use_in:
        a.in_w, a.in_b = dev[f + "fc_input_ln.weight"].data_ptr(), dev[f + "fc_input_ln.bias"].data_ptr()
    mk = mask.to(DEV).contiguous() if mask is not None else None
    a.drop_mask = mk.data_ptr() if mk is not None else None
    nws = lib.devias_fusion_head_workspace_bytes(B, S, D, C, Cd, dt)
    assert nws > 0
    ws = torch.full((nws,), 0x7f, dtype=torch.uint8, device=DEV)
    a.ws, a.ws_bytes = ws.data_ptr(), nws
    save = torch.full((lib.devias_fusion_head_save_bytes(B, D, dt),), 0x7f, dtype=torch.uint8, device=DEV)
    x = slots.to(DEV).reshape(B * S, D).contiguous()
    inp = torch.empty((B, 2 * D), dtype=dtype, device=DEV)
    out = torch.empty((B, Cd), dtype=dtype, device=DEV)
    idx = torch.full((B, 2), -7, dtype=torch.int32, device=DEV)
    st = ops._stream()
    ops.counters(reset=True)
    _lib.check(lib.devias_fusion_head_fwd(ctypes.byref(a), x.data_ptr(), inp.data_ptr(), out.data_ptr(), idx.data_ptr(), None if no_save else save.data_ptr(), st),
               "devias_fusion_head_fwd")
    assert ops.region_counters()["fusion_head"] == 1
    if no_save:
        torch.cuda.synchronize()
        assert bool((save == 0x7f).all())
        return {"input": inp.cpu(), "out": out.cpu(), "idx": idx.cpu().long()}
    r = save[_al(B * D * es):_al(B * D * es) + B * D * es].view(dtype).view(B, D).clone()
    names = [n for n in fb.GRAD_NAMES if n in P]
    G = {n: torch.full(tuple(P[n].shape), float("nan"), dtype=torch.float32, device=DEV) for n in names}
    g = _lib.FusionGrads()
    g.struct_size = ctypes.sizeof(_lib.FusionGrads)
    for fld, n in zip(("dan_w", "dan_b", "dsn_w", "dsn_b", "dWd", "dbd", "dln_w", "dln_b", "din_w", "din_b", "dWc", "dbc"), fb.GRAD_NAMES):
        if n in G:
            setattr(g, fld, G[n].data_ptr())
    do, di = dout.to(DEV).contiguous(), (dinp.to(DEV).contiguous() if dinp is not None else None)
    dslots = torch.full_like(x, float("nan"))
    ops.counters(reset=True)
    _lib.check(lib.devias_fusion_head_bwd(ctypes.byref(a), x.data_ptr(), idx.data_ptr(), inp.data_ptr(), save.data_ptr(), do.data_ptr(), di.data_ptr() if di is not None else None,
                                          dslots.data_ptr(), ctypes.byref(g), st), "devias_fusion_head_bwd")
    assert ops.region_counters()["fusion_head"] == 1
    torch.cuda.synchronize()
    return {"input": inp.cpu(), "out": out.cpu(), "idx": idx.cpu().long(), "dslots": dslots.cpu().view(B, S, D), "grads": {n: v.cpu() for n, v in G.items()}, "r": r.cpu()}


#        B  S  D    nb   ns   Cd   use_in masked
SHAPES = [(1, 1, 384, 5, 3, 2, True, False),
          (3, 2, 384, 5, 3, 48, False, True),
          (3, 3, 768, 400, 365, 101, True, True),
          (12, 4, 768, 400, 365, 200, True, False),
          (12, 2, 768, 400, 365, 48, True, True),
          (3, 4, 384, 400, 365, 101, False, False),
          (1, 3, 768, 5, 3, 200, False, True),
          (12, 1, 384, 5, 3, 2, True, True),
          (3, 3, 1024, 400, 365, 48, True, True),          # the widest supported row: all four elements per lane live
          (2, 2, 1024, 5, 3, 101, False, False)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dS%dD%d_%d+%d_Cd%d_ln%d_m%d" % s)
def test_fusion_head_region_within_bounds(shape, dtype):
    B, S, D, nb, ns, Cd, use_in, masked = shape
    worst = {}
    for kind in fb.GENERATORS:
        P = fb.make_params(D, nb, ns, Cd, use_in, seed=1)
        slots, P, dout, dinp, picks = fb.head_inputs(kind, B, S, D, dtype, P, seed=1)
        mask = fb.drop_mask(B, D, 0.5, seed=1) if masked else None
        idx64, gap = fb.selection_gap(slots, P, nb)
        assert gap >= fb.MATCH_MARGIN and torch.equal(idx64, picks), (kind, gap)
        got = run_direct(slots, P, nb, use_in, mask, dout, dinp, dtype)
        assert torch.equal(got["idx"], picks), (kind, got["idx"], picks)
        ref, bnd = fb.bounds(slots, P, nb, use_in, mask, dout, dinp, got["idx"], got["r"] > 0, dtype)
        res = {"input": fb.excess(got["input"], ref["input"], bnd["input"] * fb.SLACK_FWD)[0], "out": fb.excess(got["out"], ref["out"], bnd["out"] * fb.SLACK_FWD)[0],
               "dslots": fb.excess(got["dslots"], ref["dslots"], bnd["dslots"] * fb.SLACK_BWD)[0]}
        for n, g in got["grads"].items():
            res[n] = fb.excess(g, ref[n], bnd[n] * fb.SLACK_BWD)[0]
        for n, v in res.items():
            worst[n] = max(worst.get(n, 0.0), v)
        print(f"fusion_head {kind} {shape} {dtype}: " + ", ".join(f"{n.replace(f, '')}={v:.3f}" for n, v in res.items()))
        bad = {n: v for n, v in res.items() if not v <= 1.0}
        assert not bad, (kind, bad)
        # every row of dslots that no pick selects is exactly zero
        sel = torch.zeros(B, S, dtype=torch.bool)
        sel[torch.arange(B), picks[:, 0]] = True
        sel[torch.arange(B), picks[:, 1]] = True
        assert bool((got["dslots"][~sel] == 0).all()) and bool(torch.isfinite(got["dslots"]).all())
        if kind in ("collide", "offset"):          # the forward without a save arena (save = NULL: u, r, statistics in the workspace) gives the saved forward's bits
            bare = run_direct(slots, P, nb, use_in, mask, dout, dinp, dtype, no_save=True)
            for n in ("input", "out", "idx"):
                assert torch.equal(got[n], bare[n]), (kind, n)
        if kind == "collide":          # two runs give the same bits, in every output (the dirty workspace and arena of run_direct included)
            again = run_direct(slots, P, nb, use_in, mask, dout, dinp, dtype)
            for n in ("input", "out", "idx", "dslots", "r"):
                assert torch.equal(got[n], again[n]), n
            for n in got["grads"]:
                assert torch.equal(got["grads"][n], again["grads"][n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_fusion_head_function_is_the_region_and_leaves_six_parameters_without_gradient(dtype):
    """regions.FusionHeadFn: the direct calls' bits through autograd; head.* and fc_scene_* keep grad None; under no_grad the same out, nothing saved"""
    from devias_amd import ops
    from devias_amd.regions import FusionHeadFn
    B, S, D, nb, ns, Cd = 3, 3, 384, 5, 3, 48
    P = fb.make_params(D, nb, ns, Cd, True, seed=2)
    slots, P, dout, dinp, picks = fb.head_inputs("collide", B, S, D, dtype, P, seed=2)
    mask = fb.drop_mask(B, D, 0.5, seed=2)
    want = run_direct(slots, P, nb, True, mask, dout, dinp, dtype)
    prm = {k: torch.nn.Parameter(v.to(DEV)) for k, v in P.items()}
    x = slots.to(DEV).reshape(B * S, D).requires_grad_(True)
    meta = (B, S, nb, 1e-6, 1e-5, dtype, True)
    args = [prm[n] for n in PARAM_ORDER]
    ops.counters(reset=True)
    inp, out, idx = FusionHeadFn.apply(x, *args, meta, mask.to(DEV))
    assert ops.region_counters() == {"fusion_head": 1, "softmax_ce": 0}
    torch.autograd.backward([inp, out], [dinp.to(DEV), dout.to(DEV)])
    assert ops.region_counters() == {"fusion_head": 2, "softmax_ce": 0}
    assert torch.equal(inp.cpu(), want["input"]) and torch.equal(out.cpu(), want["out"]) and torch.equal(idx.cpu().long(), want["idx"])
    assert torch.equal(x.grad.cpu().view(B, S, D), want["dslots"])
    for n, g in want["grads"].items():
        assert torch.equal(prm[n].grad.cpu(), g), n
    for n in ("head.weight", "head.bias", f + "fc_scene_down.weight", f + "fc_scene_down.bias", f + "fc_scene_ln.weight", f + "fc_scene_ln.bias"):
        assert prm[n].grad is None, n
    # gradients disabled (the caller reads torch.is_grad_enabled() before apply, as the model does): the same bits, and nothing is kept -- although x and the
    # parameters require grad, the call allocates its three outputs and no arena
    from devias_amd import _lib
    nsave = _lib.load().devias_fusion_head_save_bytes(B, D, ops.dt_code(dtype))
    assert nsave >= 2 * B * D * x.element_size()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        inp2, out2, idx2 = FusionHeadFn.apply(x, *args, (B, S, nb, 1e-6, 1e-5, dtype, torch.is_grad_enabled()), mask.to(DEV))
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    outs = sum((t.numel() * t.element_size() + 511) // 512 * 512 for t in (inp2, out2, idx2))
    assert held <= outs < outs + nsave, (held, outs, nsave)
    assert out2.grad_fn is None and torch.equal(out2, out) and torch.equal(inp2, inp) and torch.equal(idx2, idx)
    assert ops.region_counters()["fusion_head"] == 3


CE_CASES = [(C, B, eps, kind) for C in (2, 48, 101, 1000) for B in (1, 5) for eps in (0.0, 0.1) for kind in ("plain", "last", "peaked")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_softmax_ce_within_bounds(dtype):
    from devias_amd import ops
    worst = {"loss": 0.0, "dz": 0.0}
    for C, B, eps, kind in CE_CASES:
        z, y = fb.ce_inputs(C, B, kind, dtype)
        g = torch.tensor([0.5], dtype=torch.float32, device=DEV)
        zd, yd = z.to(DEV), y.to(DEV)
        ops.counters(reset=True)
        loss = ops.softmax_ce_fwd(zd, yd, eps)
        assert ops.region_counters() == {"fusion_head": 0, "softmax_ce": 1}
        dz = ops.softmax_ce_bwd(zd, yd, g, eps)
        assert ops.region_counters() == {"fusion_head": 0, "softmax_ce": 2}
        rl, rdz = fb.ce_reference(z, y, eps, 0.5)
        bl, bdz = fb.ce_bounds(z, y, eps, 0.5, dtype)
        el, ed = fb.excess(loss.cpu()[0], rl, bl * fb.SLACK_CE)[0], fb.excess(dz.cpu(), rdz, bdz * fb.SLACK_CE)[0]
        worst["loss"], worst["dz"] = max(worst["loss"], el), max(worst["dz"], ed)
        assert el <= 1.0 and ed <= 1.0, (C, B, eps, kind, el, ed)
    print("softmax_ce", dtype, worst)


def test_softmax_ce_out_of_range_target_and_module():
    """a target outside [0, C) is never an index: that row's loss is NaN (so the mean is), its gradient row zero; the nn.Module over the kernels equals F.cross_entropy"""
    from devias_amd import ops
    from devias_amd.losses import CrossEntropyLoss, LabelSmoothingCrossEntropy
    z, y = fb.ce_inputs(48, 5, "plain", torch.float32)
    for bad in (48, -1, 2 ** 40):
        yb = y.clone()
        yb[2] = bad
        loss = ops.softmax_ce_fwd(z.to(DEV), yb.to(DEV), 0.1)
        dz = ops.softmax_ce_bwd(z.to(DEV), yb.to(DEV), torch.ones(1, device=DEV), 0.1)
        assert bool(torch.isnan(loss).all()) and bool((dz[2] == 0).all()) and bool(torch.isfinite(dz).all())
    zd = z.to(DEV).requires_grad_(True)
    loss = LabelSmoothingCrossEntropy(0.1)(zd, y.to(DEV))
    (loss / 4).backward()
    zr = z.clone().double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(zr, y, label_smoothing=0.1)
    (ref / 4).backward()
    assert abs(float(loss) - float(ref)) < 1e-5 * abs(float(ref)) and torch.allclose(zd.grad.cpu().double(), zr.grad, atol=1e-7)
    assert abs(float(CrossEntropyLoss()(z.to(DEV), y.to(DEV))) - float(torch.nn.functional.cross_entropy(z.double(), y))) < 1e-5
    with pytest.raises(NotImplementedError):
        LabelSmoothingCrossEntropy(0.1)(zd, torch.rand(5, 48, device=DEV))
