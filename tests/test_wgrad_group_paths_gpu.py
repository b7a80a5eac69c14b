"""The encoder blocks' weight gradients through the queue of devias_amd.ops (WGRAD_GROUP blocks per grouped launch) on `vitb_t16`, B = 8: against the immediate
per-product path every encoder weight gradient stays within twice the weight-gradient bound of tests/kernel_bounds.py (both are within that bound of float64) and
EVERYTHING else -- outputs, every other gradient -- is bitwise the same; a parameter with a hook or with .grad already set gets exactly the immediate path's bits;
after backward() nothing is pending and the retention buffers are back in their pool."""
import pytest
import torch

import golden_util as gu
import kernel_bounds as kb
from devias_amd import ops
from test_regions_gpu import _build, _crit, _data

pytestmark = pytest.mark.gpu
_WEIGHTS = ("mlp.fc2.weight", "mlp.fc1.weight", "attn.proj.weight", "attn.qkv.weight")      # the order a block's backward produces them in


def _run(model, crit, data, G, regions=True, prep=None, seed=None):
    import devias_amd.modeling_slot as ms
    x, y, tl, fg = data
    old, old_g = ms._REGIONS, ops.WGRAD_GROUP
    ms._REGIONS, ops.WGRAD_GROUP = regions, G
    try:
        for p in model.parameters():
            p.grad = None
        if prep is not None:
            prep(model)
        if seed is not None:
            torch.manual_seed(seed)                # (the stochastic-depth masks are drawn in forward)
        out = model(x)
        total, logits, ld = crit(model, out, (None, tl), y, fg_mask=fg)
        total.backward()
        assert ops.wgrad_pending() == 0, "jobs left pending after backward()"
        torch.cuda.synchronize()
    finally:
        ms._REGIONS, ops.WGRAD_GROUP = old, old_g
    (af, sf), (al, sl, attn), (sh, slots, mk) = out
    outs = {"total": total.detach().clone(), "slots": slots.detach().clone(), "mask": mk.detach().clone(), "action_logit": al.detach().clone()}
    return outs, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _setup(seed=None, **kw):
    """the model, its inputs, the immediate path's results and the float64 bound of every encoder weight gradient (operands recorded on the per-kernel path)"""
    fx, cfg, _ = gu.load("vitb_t16")
    model, crit, data = _build(cfg, "bf16", **kw), _crit(), _data(cfg, 8)
    M, D = 8 * cfg.num_patches, cfg.embed_dim
    shapes = [(D, 4 * D), (4 * D, D), (D, D), (3 * D, D)]
    bounds, real = [], ops.wgrad

    def spy(dY, X, out=None, beta=0.0):
        if dY.shape[0] == M and (dY.shape[1], X.shape[1]) in shapes and dY.dtype == torch.bfloat16:
            bounds.append(kb.gemm_ref(dY.t(), X, torch.bfloat16, out_f32=True)["out"][1].float())
        return real(dY, X, out=out, beta=beta)
    ops.wgrad = spy
    try:
        o_pk, g_pk = _run(model, crit, data, 0, regions=False, seed=seed)
    finally:
        ops.wgrad = real
    assert len(bounds) == 4 * cfg.depth, len(bounds)
    names = [f"blocks.{b}.{w}" for b in reversed(range(cfg.depth)) for w in _WEIGHTS]
    bound = dict(zip(names, bounds))
    o0, g0 = _run(model, crit, data, 0, seed=seed)
    for k in g0:                     # (the aggregation block's tied weight sets are reduced in another order by the region: tests/test_regions_gpu.py)
        assert "agg_block" in k or torch.equal(g0[k], g_pk[k]), k
    return model, crit, data, o0, g0, bound


@pytest.fixture(scope="module")
def setup():
    return _setup()


def _against_immediate(setup, G, seed=None):
    model, crit, data, o0, g0, bound = setup
    ops.counters(reset=True)
    _run(model, crit, data, 0, seed=seed)
    cnt0 = ops.counters(reset=True)
    o1, g1 = _run(model, crit, data, G, seed=seed)
    cnt = ops.counters()
    # every encoder weight gradient went through the grouped launches: one combine per ceil(12 / G) launches in place of 48 split-K reduces
    assert cnt["gemm256"] == cnt0["gemm256"] >= 12 * 4 and cnt["splitk_reduce"] == cnt0["splitk_reduce"] - 48 + -(-12 // G), (cnt0, cnt)
    for k in o0:
        assert torch.equal(o0[k], o1[k]), f"G = {G}: output {k} differs"
    worst = 0.0
    for k in g0:
        if k in bound:
            assert g1[k].shape == bound[k].shape
            r, idx = kb.excess(g1[k], g0[k].double(), 2.0 * bound[k].double())
            worst = max(worst, r)
            assert r <= 1.0, f"G = {G}: {k}: |grouped - immediate| / (2 bound) = {r:.3g} at {kb.where2d(idx, g0[k].shape[1])}"
        else:
            assert torch.equal(g0[k], g1[k]), f"G = {G}: gradient {k} differs"
    changed = sum(not torch.equal(g0[k], g1[k]) for k in bound)
    print(f"G = {G}: worst |grouped - immediate| / (2 bound) = {worst:.3g}; {changed} of {len(bound)} encoder weight gradients differ in some bit")
    # the per-kernel Functions enqueue the same jobs in the same order: the same bits
    o2, g2 = _run(model, crit, data, G, regions=False, seed=seed)
    for k in g1:
        assert "agg_block" in k or torch.equal(g1[k], g2[k]), f"G = {G}: {k}: fused region and per-kernel path differ"


@pytest.mark.parametrize("G", [1, 4])
def test_grouped_against_immediate(setup, G):
    _against_immediate(setup, G)


def test_grouped_against_immediate_with_stochastic_depth():
    """drop_path 0.3 (every block but the first rescales its branch gradients per sample): the rescaled copies are operands of the deferred products, kept in the
    retention buffer (region) or as the tensors they are (per-kernel path); same masks by the same seed"""
    _against_immediate(_setup(seed=7, drop_path_rate=0.3), 4, seed=7)


def test_guards_keep_the_immediate_path(setup):
    """anomaly mode scans every returned gradient: nothing may be deferred under it (exactly the immediate path's bits)"""
    model, crit, data, o0, g0, bound = setup
    with torch.autograd.set_detect_anomaly(True):
        _, g1 = _run(model, crit, data, 4)
    for k in bound:
        assert torch.equal(g1[k], g0[k]), k


def test_hooked_or_accumulating_parameters_take_the_immediate_path(setup):
    model, crit, data, o0, g0, bound = setup
    hooked, preset = "blocks.3.mlp.fc1.weight", "blocks.5.attn.proj.weight"
    params = dict(model.named_parameters())
    handle = []

    def prep(m):
        handle.append(params[hooked].register_hook(lambda g: g))
        params[preset].grad = torch.zeros_like(params[preset])
    try:
        for regions in (True, False):
            _, g1 = _run(model, crit, data, 4, regions=regions, prep=prep)
            for k in (hooked, preset):
                assert torch.equal(g1[k], g0[k]), f"{k} (regions {regions}): not the immediate path's bits"
            handle.pop().remove()
    finally:
        for h in handle:
            h.remove()


def test_two_backward_passes_leave_nothing_behind(setup):
    model, crit, data, o0, g0, bound = setup
    for G in (4, 5):                      # 12 blocks: G = 4 flushes on the count alone, G = 5 leaves two blocks to the engine's callback
        before = ops.wgrad_keep_stats()[0]       # (process-wide: earlier tests made buffers of their own sizes)
        _, g1 = _run(model, crit, data, G)
        made, free = ops.wgrad_keep_stats()
        _, g2 = _run(model, crit, data, G)
        assert ops.wgrad_pending() == 0 and all(not q.keep and not q.jobs for q in ops._wgrad_queues.values())
        assert ops.wgrad_keep_stats() == (made, made), (ops.wgrad_keep_stats(), made, free)      # every retention buffer reused and given back
        assert made - before <= G, (before, made)          # at most G blocks are ever pending
        for k in g1:
            assert torch.equal(g1[k], g2[k]), f"G = {G}: {k}: two passes differ"
