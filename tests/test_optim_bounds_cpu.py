"""The bounds of tests/optim_bounds.py, without a GPU: a numpy fp32 emulation of the optimizer kernels' arithmetic -- the float64 reference plus exactly the named
roundings, with FMA contraction on and off (the unit is built with -ffp-contract=fast; a fused multiply-add is the exact product and sum in double, rounded once) --
stays at <= 1 on every generator; an algebraically equal form of exp_avg stays at <= 1; each seeded mutant exceeds 1 on a named generator.  For the AdamW mutants the
older metric rel = max|a - b| / max|b| on the PARAMETERS is printed beside the ratio: `old rel passes` means it is below that metric's 2e-6.

Worst ratios of the emulation over betas (0.9, 0.999) / (0.9, 0.95), step 1 / 2 / 100000, fresh / warm state, wd 0 / 0.05, lr 1e-3 / 1e-3 0.75^13, scale 1 / 0.37 x 0.83,
contraction on / off, 32 775 elements (printed by test_emulation_stays_inside_the_bounds):
    adamw_multi_kernel   m' 0.345   v' 0.716   p' 0.999  (p': the rounding of a result just above a power of two, alone)
    adamw_kernel         m' 0.345   v' 0.716   p' 0.999
    control (b1 m + (1 - b1) g')   m' 0.743
    sumsq partials 0.058 (aligned), 0.058 (scalar path);  norm 0.065, coefficient 0.209
Mutants, all at betas (0.9, 0.999), lr 1e-3, wd 0.05, step 1 (worst ratio of m', v', p';  the old rel on p' and whether it is below that metric's 2e-6):
    mutant                                   state   m'        v'        p'        old rel on p'
    parent's 1.0f - fl32(beta) complements   fresh   1.24      54.5      6.78      7.1e-08  passes
    parent's fp32 powf bias corrections      fresh   0.30      0.67      6.72      7.1e-08  passes
    eps before the division by sqrt(bc2)     fresh   0.30      0.67      1.4e+06   3.2e-06  fails
    eps under the square root                fresh   0.30      0.67      1.4e+06   4.5e-06  fails
    bc1 used for bc2                         fresh   0.30      0.67      8.9e+06   4.1e-05  fails
    decay applied to the updated value       warm    0.35      0.40      76.5      6.9e-08  passes
    coupled L2 decay                         fresh   5.6e+37   3.7e+36   1.6e+08   4.5e-05  fails
    coef in m' but not in v'                 fresh   0.28      7.6e+05   1.2e+05   8.4e-07  passes
    1 - 3 element tail left unwritten        fresh   4.2e+06   4.2e+06   3.2e+05   4.3e-06  fails
    second chunk at the first chunk's offset warm    5.6e+35   3.9e+33   6.9e+39   1.1      fails
    clip coefficient without the + 1e-6 at norm 2e-6: 1.2e+06;  partial 256 dropped: norm 7.2e+03, coefficient 4.8e+03;  sum of squares without its tail: 1.1e+06
"""
import math

import numpy as np
import pytest
import torch

import kernel_bounds as kb
import optim_bounds as ob

F = np.float32
N = 2 * ob.CHUNK + 7
LR_MIN = 1e-3 * 0.75 ** 13
EPS = 1e-8


def fma(a, b, c, fused):
    if fused:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)
    return (F(1) * (a * b) + c).astype(F)


def emulate(p, g, m, v, *, lr, wd, beta1, beta2, eps, step, grad_scale=1.0, coef=1.0, fused=True, kernel="multi", mutant=None):
    """adamw_multi_kernel (elementwise.hip:277-283) or adamw_kernel (:198-203) in numpy fp32; `mutant` names one deliberate deviation"""
    p, g, m, v = (t.numpy().astype(F) for t in (p, g, m, v))
    b2, c1, c2 = F(beta2), F(1.0 - beta1), F(1.0 - beta2)
    if mutant == "parent complements":
        c1, c2 = F(1) - F(beta1), F(1) - F(beta2)
    lrf, wdf, epsf = F(lr), F(wd), F(eps)
    bc1, bc2s = F(1.0 - beta1 ** step), F(math.sqrt(1.0 - beta2 ** step))
    if mutant == "fp32 powf bias corrections":
        bc1 = F(1) - np.power(F(beta1), F(step), dtype=F)
        bc2s = np.sqrt(F(1) - np.power(F(beta2), F(step), dtype=F), dtype=F)
    if mutant == "bc1 for bc2":
        bc2s = np.sqrt(bc1, dtype=F)
    gs = F(grad_scale) * F(coef)
    decay = fma(-lrf, wdf, F(1), fused)
    gi = g * gs
    gv = g * F(grad_scale) if mutant == "coef in m' but not in v'" else gi
    if mutant == "coupled L2 decay":
        gi = gv = fma(wdf, p, gi, fused)
        decay = F(1)
    pi = p * decay
    mi = fma(c1, gi - m, m, fused)
    vi = fma(b2, v, (c2 * gv) * gv, fused)
    s = np.sqrt(vi, dtype=F)
    if mutant == "eps before the division by sqrt(bc2)":
        D = (s + epsf) / bc2s
    elif mutant == "eps under the square root":
        D = np.sqrt(vi / (bc2s * bc2s) + epsf, dtype=F)
    elif kernel == "multi":
        D = fma(s, F(1) / bc2s, epsf, fused)
    else:
        D = s / bc2s + epsf
    stepsz = lrf / bc1
    if mutant == "decay applied to the updated value":
        pn = fma(-stepsz, mi / D, p, fused) * decay
    else:
        pn = fma(-stepsz, mi / D, pi, fused)
    out = {"p": pn, "m": mi, "v": vi}
    if mutant == "tail left unwritten":
        k = len(p) - (len(p) & 3)
        for name, old in (("p", p), ("m", m), ("v", v)):
            out[name][k:] = old[k:]
    return {k: torch.from_numpy(np.ascontiguousarray(t)) for k, t in out.items()}


def ratios(out, ref):
    return {k: kb.excess(out[k], *ref[k])[0] for k in ("p", "m", "v")}


def old_rel(out, ref):
    a, b = out["p"].double(), ref["p"][0]
    return float((a - b).abs().max() / b.abs().max())


def cases():
    for betas in ob.BETAS:
        for step in (1, 2, 100000):
            for state in ("fresh", "warm"):
                for wd in (0.0, 0.05):
                    for lr in (1e-3, LR_MIN):
                        for gs, coef in ((1.0, 1.0), (0.37, 0.83)):
                            yield dict(lr=lr, wd=wd, beta1=betas[0], beta2=betas[1], eps=EPS, step=step, grad_scale=gs, coef=float(F(coef))), state


@pytest.fixture(scope="module")
def data():
    p, g = ob.adamw_inputs(N, seed=10)
    assert float(g.abs()[g != 0].min()) >= 2.0 ** -40 and bool((g == 0).any()) and bool((p == 0).any())
    return p, g


def test_generators_reach_what_they_claim(data):
    p, g = data
    for lo in (0, ob.CHUNK, 2 * ob.CHUNK):                      # every chunk and the 7-element tail: gradients on both sides of eps, zeros of both
        a = g[lo:lo + ob.CHUNK].abs()
        assert bool((a[a > 0] < EPS).any()) and bool((a > 4 * EPS).any())
    assert bool((g[:ob.CHUNK] == 0).any()) and bool((p[:ob.CHUNK] == 0).any())
    m, v = ob.adamw_state(g, "warm", seed=10)
    nz = g != 0
    assert float(((g - m).abs()[nz] / g.abs()[nz]).max()) < 0.1 and bool((v >= 0).all())


def test_emulation_stays_inside_the_bounds(data):
    p, g = data
    worst = {}
    for hyper, state in cases():
        m, v = ob.adamw_state(g, state, hyper["grad_scale"] * hyper["coef"], seed=10)
        ref = ob.adamw_ref(p, g, m, v, **hyper)
        for kernel in ("multi", "step"):
            for fused in (True, False):
                r = ratios(emulate(p, g, m, v, fused=fused, kernel=kernel, **hyper), ref)
                for k, x in r.items():
                    assert x <= 1.0, (kernel, fused, state, hyper, k, x)
                    worst[(kernel, k)] = max(worst.get((kernel, k), 0.0), x)
    for (kernel, k), x in sorted(worst.items()):
        print(f"[bound] emulation adamw {kernel} {k}' worst ratio {x:.3f}")


def test_control_the_other_expression_order_stays_inside(data):
    """m' = b1 m + (1 - b1) g' with fl32(b1): algebraically equal, other roundings; the m' bound must hold it (and p', which carries m')"""
    p, g = data
    worst = 0.0
    for hyper, state in cases():
        scale = hyper["grad_scale"] * hyper["coef"]
        m, v = ob.adamw_state(g, state, scale, seed=10)
        ref = ob.adamw_ref(p, g, m, v, **hyper)
        gi = g.numpy() * (F(hyper["grad_scale"]) * F(hyper["coef"]))
        for fused in (True, False):
            mi = fma(F(hyper["beta1"]), m.numpy(), F(1.0 - hyper["beta1"]) * gi, fused)
            r = kb.excess(torch.from_numpy(mi), *ref["m"])[0]
            assert r <= 1.0, (state, hyper, fused, r)
            worst = max(worst, r)
    print(f"[bound] control b1 m + (1 - b1) g' m' worst ratio {worst:.3f}")


H999 = dict(lr=1e-3, wd=0.05, beta1=0.9, beta2=0.999, eps=EPS, step=1)
MUTANTS = [   # (mutant, hyper-parameters, state, the output that must exceed its bound)
    ("parent complements", H999, "fresh", "v"),
    ("fp32 powf bias corrections", H999, "fresh", "p"),
    ("eps before the division by sqrt(bc2)", H999, "fresh", "p"),
    ("eps under the square root", H999, "fresh", "p"),
    ("bc1 for bc2", H999, "fresh", "p"),
    ("decay applied to the updated value", H999, "warm", "p"),
    ("coupled L2 decay", H999, "fresh", "m"),
    ("coef in m' but not in v'", dict(H999, grad_scale=1.0, coef=float(F(0.83))), "fresh", "v"),
    ("tail left unwritten", H999, "fresh", "m"),
]


def test_mutants_exceed_the_bounds(data):
    p, g = data
    for mutant, hyper, state, key in MUTANTS:
        m, v = ob.adamw_state(g, state, hyper.get("coef", 1.0), seed=10)
        ref = ob.adamw_ref(p, g, m, v, **hyper)
        for kernel in (("step",) if mutant == "fp32 powf bias corrections" else ("multi",)):
            out = emulate(p, g, m, v, kernel=kernel, mutant=mutant, **hyper)
            r, rel = ratios(out, ref), old_rel(out, ref)
            print(f"[mutant] {mutant:40s} {state:5s} betas ({hyper['beta1']}, {hyper['beta2']})  m' {r['m']:9.3g}  v' {r['v']:9.3g}  p' {r['p']:9.3g}   "
                  f"old rel on p' {rel:.2e} ({'passes' if rel < 2e-6 else 'fails'})")
            assert r[key] > 1.0, (mutant, key, r)


def test_mutant_second_chunk_reads_the_first_chunks_offset(data):
    p, g = data
    m, v = ob.adamw_state(g, "warm", seed=10)
    ref = ob.adamw_ref(p, g, m, v, **H999)
    out = emulate(p, g, m, v, **H999)
    first = emulate(p[:ob.CHUNK], g[:ob.CHUNK], m[:ob.CHUNK], v[:ob.CHUNK], **H999)
    for k in out:
        out[k][ob.CHUNK:2 * ob.CHUNK] = first[k]
    r = ratios(out, ref)
    print(f"[mutant] second chunk at the first chunk's offset  m' {r['m']:.3g} v' {r['v']:.3g} p' {r['p']:.3g}   old rel on p' {old_rel(out, ref):.2e}")
    assert min(r.values()) > 1.0, r


# ------------------------------------------------------------------------------------------------ gradient norm
def emulate_sumsq(chunk, aligned=True, fused=True, drop_tail=False):
    """sumsq_multi_kernel (:217-231) on one chunk: thread t owns float4 t, t + 256, ...; six wave levels; (r0 + r1) + (r2 + r3)"""
    g = chunk.numpy().astype(F)
    n = len(g)
    s = np.zeros(256, F)
    done = 0
    if aligned:
        n4 = n >> 2
        it = -(-n4 // 256)
        q = np.zeros((it * 256, 4), F)
        q[:n4] = g[:4 * n4].reshape(n4, 4)
        q = q.reshape(it, 256, 4)
        for i in range(it):
            x = q[i]
            t = x[:, 0] * x[:, 0]
            for c in (1, 2, 3):
                t = fma(x[:, c], x[:, c], t, fused)
            s = (s + t).astype(F)
        done = 4 * n4
    if not drop_tail:
        rest = g[done:]
        it = -(-len(rest) // 256)
        r = np.zeros(it * 256, F)
        r[:len(rest)] = rest
        for row in r.reshape(it, 256):
            s = fma(row, row, s, fused)
    w = s.reshape(4, 64)
    for off in (1, 2, 4, 8, 32, 16):
        w = (w + w[:, np.arange(64) ^ off]).astype(F)
    red = w[:, 0]
    return F(F(red[0] + red[1]) + F(red[2] + red[3]))


def emulate_clip(partials, max_norm, eps_const=F(1e-6), drop=None):
    """clip_coef_kernel (:236-248): thread t owns partials t, t + 256, ...; an eight-level tree over 256 threads"""
    x = partials.numpy().astype(F)
    if drop is not None:
        x = np.delete(x, drop)
    it = max(-(-len(x) // 256), 1)
    r = np.zeros(it * 256, F)
    r[:len(x)] = x
    s = np.zeros(256, F)
    for row in r.reshape(it, 256):
        s = (s + row).astype(F)
    w = 128
    while w:
        s[:w] = s[:w] + s[w:2 * w]
        w >>= 1
    norm = np.sqrt(s[0], dtype=F)
    c = F(max_norm) / F(norm + eps_const) if max_norm > 0 else F(1)
    return float(norm), float(min(c, F(1)))


def test_sumsq_emulation_and_dropped_tail():
    worst = {True: 0.0, False: 0.0}
    for n in (1, 3, 1027, ob.CHUNK - 1, ob.CHUNK):
        g = ob.sumsq_inputs(n, ob.hot_tail(n), seed=20)
        for aligned in (True, False):
            ref, bound = ob.sumsq_ref(g, aligned)
            for fused in (True, False):
                r = ob.scalar_ratio(emulate_sumsq(g, aligned, fused), float(ref[0]), float(bound[0]))
                assert r <= 1.0, (n, aligned, fused, r)
                worst[aligned] = max(worst[aligned], r)
        if n & 3 and n > 4:                                  # mutant: the len & 3 tail, which holds the largest scale, is not summed
            ref, bound = ob.sumsq_ref(g, True)
            r = ob.scalar_ratio(emulate_sumsq(g, True, True, drop_tail=True), float(ref[0]), float(bound[0]))
            print(f"[mutant] sum of squares without its tail, n {n}: ratio {r:.3g}")
            assert r > 1.0
    print(f"[bound] emulation sumsq worst ratio aligned {worst[True]:.3f} scalar path {worst[False]:.3f}")


def test_clip_emulation_cases_and_mutants():
    worst = {"norm": 0.0, "coef": 0.0}
    g = torch.Generator().manual_seed(30)
    for n in (0, 1, 256, 257, 600):
        part = (torch.rand(n, generator=g) + 0.5).float()
        norm = math.sqrt(float(part.double().sum()))
        for max_norm in (0.0, 1e9, 0.5 * norm if n else 0.5, 1e-6):
            ref = ob.clip_ref(part, max_norm)
            out = dict(zip(("norm", "coef"), emulate_clip(part, max_norm)))
            for k in out:
                r = ob.scalar_ratio(out[k], *ref[k])
                assert r <= 1.0, (n, max_norm, k, out[k], ref[k])
                worst[k] = max(worst[k], r)
            if max_norm in (0.0, 1e9) or (n == 0 and max_norm > 1e-6):
                assert out["coef"] == 1.0 and ref["coef"] == (1.0, 0.0), (n, max_norm)
    print(f"[bound] emulation clip worst ratio norm {worst['norm']:.3f} coef {worst['coef']:.3f}")
    # a norm near 2e-6 under max_norm 1e-6: the + 1e-6 decides between 1/3 and 1/2
    tiny = torch.full((3,), (2e-6) ** 2 / 3, dtype=torch.float32)
    ref = ob.clip_ref(tiny, 1e-6)
    assert abs(ref["coef"][0] - 1.0 / 3.0) < 1e-3
    assert ob.scalar_ratio(emulate_clip(tiny, 1e-6)[1], *ref["coef"]) <= 1.0
    r = ob.scalar_ratio(emulate_clip(tiny, 1e-6, eps_const=F(0))[1], *ref["coef"])
    print(f"[mutant] clip coefficient without the + 1e-6 at norm 2e-6: ratio {r:.3g}")
    assert r > 1.0
    # the partial at index 256 (the second pass of the thread loop) dropped
    part = (torch.rand(257, generator=g) + 0.5).float()
    ref = ob.clip_ref(part, 1.0)
    rn, rc = (ob.scalar_ratio(x, *ref[k]) for x, k in zip(emulate_clip(part, 1.0, drop=256), ("norm", "coef")))
    print(f"[mutant] partial 256 dropped: norm ratio {rn:.3g}, coefficient ratio {rc:.3g}")
    assert rn > 1.0 and rc > 1.0
    # an all-zero gradient: norm 0, coefficient exactly 1
    zero = torch.zeros(5)
    assert emulate_clip(zero, 1.0) == (0.0, 1.0) and ob.clip_ref(zero, 1.0) == {"norm": (0.0, 0.0), "coef": (1.0, 0.0)}
