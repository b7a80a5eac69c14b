"""The optimizer kernels of devias_amd/csrc/elementwise.hip on the GPU, each output element held to the bounds of tests/optim_bounds.py against float64 (float64
references in torch on the device: none of this project's kernels): devias_adamw_multi and devias_adamw_ema_multi over a hand-built table, devias_adamw_step,
devias_grad_sumsq_multi, devias_clip_coef, and FusedAdamW.step end to end, one step at a time.  Sizes are the smallest that reach each path: one element, a tail
shorter than a float4, a chunk boundary on either side (DEVIAS_OPT_CHUNK = 16384), three chunks with a tail, one wrap of the 2048-workgroup grid, more than 256
partials; pointers that are not 16-byte aligned, all four or one alone.  Each case prints `[bound] <kernel> <shape> <variant> worst ratio ...`."""
import math

import numpy as np
import pytest
import torch

import kernel_bounds as kb
import optim_bounds as ob
from test_elementwise_bounds_gpu import guarded, guards_intact, place, say

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
EPS = 1e-8
LR_MIN = 1e-3 * 0.75 ** 13
LENS = [1, 3, 4, 1027, ob.CHUNK - 1, ob.CHUNK, ob.CHUNK + 1, 2 * ob.CHUNK + 7]
# every table row has hyper-parameters of its own: a descriptor read from the wrong row shows
ROW_LR = [1e-3, LR_MIN, 3e-4, 1e-3 * 0.75 ** 5, 1e-3, LR_MIN, 7e-4, 1e-3 * 0.75 ** 9]
ROW_WD = [0.05, 0.05, 0.0, 0.01, 0.0, 0.05, 0.05, 0.01]
ROW_STEP = [1, 2, 100000, 3, 1, 100000, 2, 1]
VARIANTS = {"aligned": (0, 0, 0, 0), "all offset": (1, 1, 1, 1), "only grad offset": (0, 1, 0, 0), "only exp_avg_sq offset": (0, 0, 0, 1)}     # p, g, m, v


@pytest.fixture
def o():
    from devias_amd import ops
    return ops


def hyper(i, betas, grad_scale, coef):
    return dict(lr=ROW_LR[i], wd=ROW_WD[i], beta1=betas[0], beta2=betas[1], eps=EPS, step=ROW_STEP[i], grad_scale=grad_scale, coef=coef)


class Table:
    """the inputs of LENS (kept unchanged), guarded working copies placed per `offsets`, and the device table over them"""

    def __init__(self, offsets, state, scale, betas, shadows=()):
        from devias_amd.optim import _REC, chunk_lists
        self.inputs, self.work, self.shadow = [], [], {}
        rec = np.zeros(len(LENS), _REC)
        for i, n in enumerate(LENS):
            p, g = ob.adamw_inputs(n, seed=100 + 10 * i, device=DEV)
            m, v = ob.adamw_state(g, state, scale, seed=100 + 10 * i)
            self.inputs.append((p, g, m, v))
            bufs = []
            for t, off in ((p, offsets[0]), (m, offsets[2]), (v, offsets[3])):
                buf, view = guarded(n, F32, off)
                view.copy_(t)
                bufs.append((buf, view))
            gw = place(g, offsets[1])
            self.work.append((bufs, gw))
            e = 0
            if i in shadows:
                self.shadow[i] = place(kb._randn((n,), 900 + i, DEV), shadows[i])
                e = self.shadow[i].data_ptr()
            t = ROW_STEP[i]
            rec[i] = (bufs[0][1].data_ptr(), gw.data_ptr(), bufs[1][1].data_ptr(), bufs[2][1].data_ptr(), n, ROW_LR[i], ROW_WD[i],
                      1.0 - betas[0] ** t, math.sqrt(1.0 - betas[1] ** t), e)
        self.table = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV)
        self.ct, self.ci = chunk_lists(LENS, DEV)

    def outputs(self, i):
        bufs, _ = self.work[i]
        return {"p": bufs[0][1], "m": bufs[1][1], "v": bufs[2][1]}

    def intact(self, i):
        bufs, gw = self.work[i]
        return all(guards_intact(buf, LENS[i]) for buf, _ in bufs) and torch.equal(gw, self.inputs[i][1])


# ------------------------------------------------------------------------------------------------ devias_adamw_multi
@pytest.mark.parametrize("state,grad_scale,coef", [("fresh", 1.0, None), ("warm", 0.37, 0.83)])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("betas", ob.BETAS)
def test_adamw_multi(betas, variant, state, grad_scale, coef, o):
    coef_dev = None if coef is None else torch.tensor([coef], dtype=F32, device=DEV)
    coef64 = 1.0 if coef is None else float(coef_dev)
    T = Table(VARIANTS[variant], state, grad_scale * coef64, betas)
    o.adamw_multi(T.table, T.ct, T.ci, betas[0], betas[1], EPS, grad_scale, coef_dev)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for i, n in enumerate(LENS):
        ref = ob.adamw_ref(*T.inputs[i], **hyper(i, betas, grad_scale, coef64))
        for k, out in T.outputs(i).items():
            print(f"[bound] adamw_multi n {n} {variant} {state} betas {betas} {k}' ratio {kb.excess(out, *ref[k])[0]:.3f}")
        for k, out in T.outputs(i).items():
            worst[k] = max(worst[k], kb.check(f"adamw_multi {k}' row {i} n {n} {variant} {state} betas {betas}", out, *ref[k]))
        assert T.intact(i), (i, n, "a guard element or the gradient was written")
    say("adamw_multi", "table", f"{variant} {state} betas {betas}", max(worst.values()))


# ------------------------------------------------------------------------------------------------ devias_adamw_ema_multi
@pytest.mark.parametrize("betas", ob.BETAS)
def test_adamw_ema_multi_equals_adamw_multi_and_holds_the_shadow(betas, o):
    """shadows on rows 1, 3, 6, 7 (row 3's not 16-byte aligned), none on the others: p, m, v bit-equal to devias_adamw_multi on the same inputs; the shadow is
    torch's three-rounding expression of the updated p (tests/test_ema_gpu.py)"""
    decay = 0.9999
    plain = Table(VARIANTS["aligned"], "warm", 1.0, betas)
    fused = Table(VARIANTS["aligned"], "warm", 1.0, betas, shadows={1: 0, 3: 1, 6: 0, 7: 0})
    before = {i: e.clone() for i, e in fused.shadow.items()}
    o.adamw_multi(plain.table, plain.ct, plain.ci, betas[0], betas[1], EPS)
    o.adamw_ema_multi(fused.table, fused.ct, fused.ci, betas[0], betas[1], EPS, decay)
    for i, n in enumerate(LENS):
        for k, out in fused.outputs(i).items():
            assert torch.equal(out, plain.outputs(i)[k]), (i, n, k)
        assert fused.intact(i)
        ref = ob.adamw_ref(*fused.inputs[i], **hyper(i, betas, 1.0, 1.0))
        kb.check(f"adamw_ema_multi p' row {i}", fused.outputs(i)["p"], *ref["p"])
    for i, e in fused.shadow.items():
        want = before[i] * decay + (1. - decay) * fused.outputs(i)["p"]
        assert not torch.equal(e, before[i]) and torch.equal(e, want), (i, float((e - want).abs().max()))


# ------------------------------------------------------------------------------------------------ devias_adamw_step
@pytest.mark.parametrize("step", [1, 2, 100000])
@pytest.mark.parametrize("betas", ob.BETAS)
def test_adamw_step(betas, step, o):
    """one element per thread over at most 2048 workgroups: 2048 * 256 + 3 wraps the grid once and leaves a tail"""
    for j, n in enumerate([1, 3, 1027, 2048 * 256 + 3]):
        state, gs = (("fresh", 1.0), ("warm", 0.37))[(j + step) % 2]
        h = dict(lr=(1e-3, LR_MIN)[j % 2], wd=(0.05, 0.0)[(j // 2) % 2], beta1=betas[0], beta2=betas[1], eps=EPS, step=step, grad_scale=gs)
        p, g = ob.adamw_inputs(n, seed=300 + j, device=DEV)
        m, v = ob.adamw_state(g, state, gs, seed=300 + j)
        ref = ob.adamw_ref(p, g, m, v, **h)
        pw, mw, vw, gw = p.clone(), m.clone(), v.clone(), g.clone()
        o.adamw_step(pw, gw, mw, vw, h["lr"], betas[0], betas[1], EPS, h["wd"], step, gs)
        r = {}
        for k, out in (("p", pw), ("m", mw), ("v", vw)):
            r[k] = kb.excess(out, *ref[k])[0]
        print(f"[bound] adamw_step n {n} {state} step {step} betas {betas} m' {r['m']:.3f} v' {r['v']:.3f} p' {r['p']:.3f}")
        for k, out in (("p", pw), ("m", mw), ("v", vw)):
            kb.check(f"adamw_step {k}' n {n} {state} step {step} betas {betas}", out, *ref[k])
        assert torch.equal(gw, g)
        say("adamw_step", n, f"{state} step {step} betas {betas}", max(r.values()))


# ------------------------------------------------------------------------------------------------ devias_grad_sumsq_multi, devias_clip_coef
N_BIG = 256 * ob.CHUNK + 1027                                # 257 chunks: the second pass of clip_coef_kernel's thread loop; the last chunk partial, with a 3-element tail
HOT = {"none": (), "tail": ob.hot_tail(N_BIG), "last partial chunk": (256 * ob.CHUNK + 5,), "end of a full chunk": (ob.CHUNK - 1, 255 * ob.CHUNK + ob.CHUNK - 2)}


def grad_table(grads):
    from devias_amd.optim import _REC, chunk_lists
    rec = np.zeros(len(grads), _REC)
    for i, g in enumerate(grads):
        rec[i]["grad"], rec[i]["n"] = g.data_ptr(), g.numel()
    return (torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(DEV),) + chunk_lists([g.numel() for g in grads], DEV)


def clip_out():
    buf = torch.full((4,), 12288.0, dtype=F32, device=DEV)
    return buf, buf[1:3]


def run_clip(o, partials, k, max_norm):
    buf, out = clip_out()
    o.clip_coef(partials, k, max_norm, out)
    assert float(buf[0]) == 12288.0 and float(buf[3]) == 12288.0
    ref = ob.clip_ref(partials[:k], max_norm)
    rn, rc = ob.scalar_ratio(out[0], *ref["norm"]), ob.scalar_ratio(out[1], *ref["coef"])
    assert rn <= 1.0 and rc <= 1.0, (k, max_norm, out.tolist(), ref)
    return out.tolist(), ref, max(rn, rc)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("hot", list(HOT))
def test_grad_sumsq_and_clip_coef_over_257_chunks(hot, offset, o):
    g = place(ob.sumsq_inputs(N_BIG, HOT[hot], seed=400, device=DEV), offset)
    table, ct, ci = grad_table([g])
    ref, bound = ob.sumsq_ref(g, aligned=not offset)
    for k in (0, 1, 256, 257):
        partials = torch.full((258,), 12288.0, dtype=F32, device=DEV)
        if k:
            o.grad_sumsq_multi(table, ct[:k], ci[:k], partials)
        else:                                                    # n_chunks = 0 with valid lists (an empty torch view has no address to pass): nothing is launched
            from devias_amd import _lib
            _lib.check(_lib.load().devias_grad_sumsq_multi(table.data_ptr(), ct.data_ptr(), ci.data_ptr(), 0, partials.data_ptr(), None), "devias_grad_sumsq_multi")
        assert bool((partials[k:] == 12288.0).all()), k
        r = kb.check(f"sumsq partials, {k} chunks, hot {hot}, offset {offset}", partials[:k], ref[:k], bound[:k]) if k else 0.0
        say("grad_sumsq_multi", N_BIG, f"{k} chunks hot {hot} offset {offset}", r)
        norm = math.sqrt(float(ref[:k].sum()))
        for max_norm in (0.0, 1e9, 0.5 * norm if k else 0.5):
            out, cref, rc = run_clip(o, partials, k, max_norm)
            if max_norm == 0.0 or max_norm == 1e9 or k == 0:
                assert out[1] == 1.0, (k, max_norm, out)             # exactly 1: max_norm = 0, max_norm far above the norm, a zero norm
            else:
                assert out[1] < 0.51
            assert ob.scalar_ratio(out[0], norm, cref["norm"][1] + float(bound[:k].sum()) / (2 * norm) if k else 0.0) <= 1.0     # and against the float64 gradients
            say("clip_coef", k, f"max_norm {max_norm:.3g} hot {hot} offset {offset}", rc)


@pytest.mark.parametrize("offset", [0, 1])
def test_grad_sumsq_over_the_table_of_lengths(offset, o):
    """every length of the AdamW table, the largest scale in each tensor's len & 3 tail"""
    grads = [place(ob.sumsq_inputs(n, ob.hot_tail(n), seed=420 + i, device=DEV), offset) for i, n in enumerate(LENS)]
    table, ct, ci = grad_table(grads)
    partials = torch.full((ct.numel() + 1,), 12288.0, dtype=F32, device=DEV)
    o.grad_sumsq_multi(table, ct, ci, partials)
    refs = [ob.sumsq_ref(g, aligned=not offset) for g in grads]
    ref, bound = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])
    say("grad_sumsq_multi", "table", f"offset {offset}", kb.check(f"sumsq partials over the table, offset {offset}", partials[:-1], ref, bound))
    assert float(partials[-1]) == 12288.0


def test_clip_coef_at_a_tiny_norm_and_at_zero(o):
    g = ob.sumsq_inputs(1027, (), seed=430, device=DEV)
    g = (g.double() * (2e-6 / float(g.double().norm()))).float()          # norm 2e-6: the + 1e-6 of clip_grad_norm_ decides between 1/3 and 1/2
    table, ct, ci = grad_table([g])
    partials = torch.empty(1, dtype=F32, device=DEV)
    o.grad_sumsq_multi(table, ct, ci, partials)
    kb.check("sumsq at norm 2e-6", partials, *ob.sumsq_ref(g))
    out, ref, r = run_clip(o, partials, 1, 1e-6)
    assert abs(out[1] - 1.0 / 3.0) < 1e-3 and abs(out[0] - 2e-6) < 1e-9
    say("clip_coef", 1, "norm 2e-6 max_norm 1e-6", r)
    zero = torch.zeros(ob.CHUNK + 3, dtype=F32, device=DEV)
    table, ct, ci = grad_table([zero])
    partials = torch.full((2,), 12288.0, dtype=F32, device=DEV)
    o.grad_sumsq_multi(table, ct, ci, partials)
    assert partials.tolist() == [0.0, 0.0]
    out, _, _ = run_clip(o, partials, 2, 1.0)
    assert out == [0.0, 1.0]


# ------------------------------------------------------------------------------------------------ FusedAdamW.step, end to end
E2E_LENS = [3, 1027, ob.CHUNK + 1, 4, ob.CHUNK, 1]


@pytest.mark.parametrize("multi_tensor", [True, False])
def test_fused_adamw_every_step_inside_the_one_step_bound(multi_tensor):
    """three steps, three groups (lr, lr_scale, weight decay), betas (0.9, 0.999), the clip active (multi-tensor path), parameter 2 without a gradient in step 2 (its
    step count falls behind): after each step every p, exp_avg, exp_avg_sq is held to the ONE-step bound from copies taken before it"""
    from devias_amd.optim import FusedAdamW
    betas = (0.9, 0.999)
    params = [ob.adamw_inputs(n, seed=500 + i, device=DEV)[0].requires_grad_(True) for i, n in enumerate(E2E_LENS)]
    groups = [{"params": params[0:2], "weight_decay": 0.05, "lr_scale": 0.75 ** 13}, {"params": params[2:4], "weight_decay": 0.0, "lr_scale": 1.0},
              {"params": params[4:], "weight_decay": 0.01, "lr_scale": 0.5}]
    opt = FusedAdamW(groups, lr=1e-3, betas=betas, eps=EPS, multi_tensor=multi_tensor)
    group_of = {id(p): g for g in opt.param_groups for p in g["params"]}
    for step in (1, 2, 3):
        lr = 1e-3 * (1.0 - 0.1 * step)
        for g in opt.param_groups:
            g["lr"] = lr * g["lr_scale"]
        grads = [None if (step == 2 and i == 2) else ob.adamw_inputs(n, seed=600 + 10 * step + i, device=DEV)[1] for i, n in enumerate(E2E_LENS)]
        before = []
        for p, g in zip(params, grads):
            p.grad = g
            st = opt.state.get(p, {})
            zeros = torch.zeros_like(p.detach())
            before.append((p.detach().clone(), st["exp_avg"].clone() if st else zeros, st["exp_avg_sq"].clone() if st else zeros.clone(), st.get("step", 0)))
        coef, coef_err = 1.0, 0.0
        if multi_tensor:
            parts = [ob.sumsq_ref(g, aligned=g.data_ptr() % 16 == 0) for g in grads if g is not None]
            pref, perr = torch.cat([x[0] for x in parts]), torch.cat([x[1] for x in parts])
            max_norm = 0.25 * math.sqrt(float(pref.sum()))                # below the norm: the clip is active
            clip = ob.clip_ref(pref, max_norm, perr)
            coef, coef_err = clip["coef"]
            assert coef < 0.26
            opt.step(max_norm=max_norm)
            rn = ob.scalar_ratio(opt.last_grad_norm, *clip["norm"])
            say("FusedAdamW", "last_grad_norm", f"step {step}", rn)
            assert rn <= 1.0, (float(opt.last_grad_norm), clip["norm"])
        else:
            opt.step()
        for i, (p, g) in enumerate(zip(params, grads)):
            p0, m0, v0, t0 = before[i]
            if g is None:
                assert torch.equal(p.detach(), p0) and opt.state[p].get("step", 0) == t0, i
                continue
            st, grp = opt.state[p], group_of[id(p)]
            assert st["step"] == t0 + 1
            ref = ob.adamw_ref(p0, g, m0, v0, lr=grp["lr"], wd=grp["weight_decay"], beta1=betas[0], beta2=betas[1], eps=EPS, step=st["step"],
                               coef=coef, coef_err=coef_err)
            r = max(kb.check(f"FusedAdamW(multi_tensor={multi_tensor}) step {step} tensor {i} {k}'", out, *ref[k])
                    for k, out in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])))
            say("FusedAdamW", E2E_LENS[i], f"multi_tensor {multi_tensor} step {step} own step {st['step']}", r)
