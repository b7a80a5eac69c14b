"""Per-element error bounds against float64 for the optimizer kernels of devias_amd/csrc/elementwise.hip: the AdamW step (adamw_kernel, adamw_multi_kernel), the
gradient sum of squares (sumsq_multi_kernel) and the clip coefficient (clip_coef_kernel), on graded inputs.

The sibling of kernel_bounds.py and slot_loss_bounds.py (same rules, same measure: excess(out, ref, bound) = max |out - ref| / bound, a test asserts <= 1): a plain
helper module, no fixtures, no plugin; torch arithmetic on whatever device the arguments live on.  u = u_fp32 = 2^-24.  Line numbers are those of elementwise.hip.

Why: the older optimizer tests compare PARAMETERS with rel = max|a - b| / max|b| < 2e-6.  The update is lr ~ 1e-4 ... 1e-3 next to parameters of size 1 ... 4, so
that metric passes an error of several per cent of the update, never sees exp_avg, and on randn gradients never has sqrt(v) near eps.  Here m', v' and p' are each
held element by element, the parameters include exact zeros (no u |p| term hides the update there) and the gradients cross eps inside every chunk and tail.

AdamW (adamw_ref).  The reference is exact AdamW in float64 from the fp32 tensors and the DOUBLE hyper-parameters, as torch.optim.AdamW states it:
    g' = g grad_scale coef,   m' = m + (1 - b1)(g' - m),   v' = b2 v + (1 - b2) g'^2,   A = sqrt(v') / sqrt(bc2),   D = A + eps,
    U = (lr / bc1) m' / D,    p' = p (1 - lr wd) - U,      bc1 = 1 - b1^step,  bc2 = 1 - b2^step
One bound covers adamw_multi_kernel (:277-283) and adamw_kernel (:198-203, which divides by bc2_sqrt where the other multiplies by its reciprocal).  The kernels are
handed fl32(b2), fl32(1 - b1), fl32(1 - b2) with the complements formed in double by the host (include/devias_amd.h), and fl32 of lr, wd, bc1, sqrt(bc2), eps.
    r_g   relative error of the scaled gradient: 0 when grad_scale = coef = 1 (the product by 1.0f is exact), else 3 u: fl32(grad_scale), its product with the
          device coefficient (:275), the product with g (:198, :279);  + coef_err / coef where the caller's coefficient itself carries an error (clip_ref)
    m'    u |m'|                              the rounding of the result (:200, :281; the same whether or not the compiler contracts the product into an FMA)
          + 3 u (1 - b1)(|g'| + |m|)          the subtraction g' - m, fl32(1 - b1), the product -- against the size of WHAT WAS SUBTRACTED, not of the difference, so
                                              that the bound does not pin the expression order: b1 m + (1 - b1) g' rounds (1 - b1) g' twice and stays inside it
          + (|fl32(b1) - b1| + u b1) |m|      the constant b1 itself where a kernel multiplies by it (that second form; the exact figure for the given b1: 0.44 u
                                              b1 at 0.9), and the product b1 m where it is not contracted into the sum
          + (1 - b1) |g'| r_g
    v'    u v' + 2 u b2 v + 3 u (1 - b2) g'^2 + 2 (1 - b2) g'^2 r_g          over its two non-negative addends (:201, :282): the result; fl32(b2) and the product;
                                              fl32(1 - b2) and the two products of (1 - b2) g' g'; g' enters squared
    D     A (e_v / (2 v') + u) + 3 u A + u eps + u D          sqrtf of the rounded v' (correctly rounded, below); fl32(sqrt(bc2)), the reciprocal `ib2` (:277) or
                                              the division (:202), the product; fl32(eps); the sum (:202, :283)
    U     (lr / bc1) (e_m / D + |m'| / D  e_D / D) + 5 u |U|       the m' bound carried through lr / (bc1 D) and the D bound through the division: its v' part is
                                              |U| (A / D) e_v / (2 v'), and A / D = sqrt(v') / (sqrt(v') + eps sqrt(bc2)) keeps it from exploding where eps dominates;
                                              5 u: the division m' / D, `step` = fl32(lr) / fl32(bc1) (three roundings, :277, :203), the final product
    p'    u |p'| + (2 + 3 lr wd) u |p (1 - lr wd)| + e_U      the result; the decay product and the fp32 1 - lr wd (:199, :277, :280; 3 lr wd u: fl32(lr), fl32(wd), their
                                              product, all next to 1) -- no decay term at wd = 0, where the factor is exactly 1.  An element with p = 0 carries no u |p|
                                              term at all: there the bound is the bound of the update.
The bounds are first order with factor 1 and no slack.  They rely on `sqrtf` and `/` being correctly rounded: the unit is built with -ffp-contract=fast and WITHOUT
fast-math (devias_amd/build.py: FLAGS), and hipcc's default keeps fp32 division and square root correctly rounded.  Contraction only removes roundings that are counted.

Gradient norm.
    sumsq_ref   partials[c] = sum of the squares of chunk c (DEVIAS_OPT_CHUNK = 16384 elements):  depth u sum, as kernel_bounds.colsum_depth counts it -- the longest chain
                of roundings one addend goes through in sumsq_multi_kernel's tree (:217-231): its product (1), the three additions inside its float4 (3), the thread's
                chain over ceil(len / 1024) float4 iterations, one more for the len & 3 tail (:224), six wave levels (:228), three adds of the four wave sums (:231).
                The scalar path of a gradient that is not 16-byte aligned (:226): 1 + ceil(len / 256) + 6 + 3.
    clip_ref    norm = sqrt(sum_c partials[c]),  coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1, from the partials the kernel is given (fp32, exact) or from
                float64 partials with their own bounds.  clip_coef_kernel's tree (:236-248): the thread's chain of ceil(n / 256) partials, eight levels;  norm:
                e_sum / (2 norm) + u norm (one sqrtf);  coef: c (e_norm + u 1e-6 + u (norm + 1e-6)) / (norm + 1e-6) + 2 u c  (the constant 1e-6f, the sum, fl32(max_norm),
                the division), and exactly 1 -- bound 0 -- where max_norm = 0 or c exceeds 1 by more than its bound.

Generators.  adamw_inputs: g = randn (|.| >= 2^-6) x powers of two cycling over 2^-34 ... 2^-8 with period 27, exact zeros every 31st element; p = randn x powers of
two 2^-6 ... 2^6 with period 13 (coprime to 27: every pair of scales meets), exact zeros every 37th.  27, 13, 31 and 37 are coprime to 4, 256 and 16384, so every
chunk, float4 and tail holds every scale; |g| >= 2^-40, nothing is denormal.  sqrt(v') / sqrt(bc2) crosses eps = 1e-8 ~ 2^-26.6 inside every chunk: the three
possible placements of eps differ there by factors.  States: `fresh` (m = v = 0) and `warm` (m = g' (1 + 2^-6 randn), so that g' - m cancels; v = g'^2 (1 + randn / 8)).
sumsq_inputs: one scale (2^-10 randn, graded 2^-3 ... 2^3) and `hot` indices that hold +-(1 ... 2): in the len & 3 tail, in the last partial chunk, in chunk number 256.

What the emulation measures (tests/test_optim_bounds_cpu.py: the float64 reference plus exactly the named roundings in numpy fp32, FMA contraction on and off; its
docstring holds the full table) and what the kernels measured on an MI355X (tests/test_optim_bounds_gpu.py prints them):

    kernel, variant                                          emulation (m', v', p')     measured on the device (m', v', p')
    devias_adamw_multi   aligned                             0.35  0.72  0.999          0.32  0.72  0.99
                         all four pointers offset                                       0.32  0.72  0.99
                         only the gradient offset                                       0.32  0.72  0.99
                         only exp_avg_sq offset                                         0.32  0.72  0.99
                         fresh / warm, betas (0.9, 0.999)                               0.30  0.67  0.99 / 0.32  0.72  0.99
                         fresh / warm, betas (0.9, 0.95)                                0.30  0.49  0.99 / 0.32  0.61  0.99
    devias_adamw_ema_multi   p, m, v bit-equal to devias_adamw_multi; the shadow bit-equal to torch's three-rounding expression
    devias_adamw_step    betas (0.9, 0.999), step 1 / 2 / 100000   0.35  0.72  0.999    0.30  0.69  0.998 / 0.32  0.73  0.998 / 0.32  0.73  0.9995
                         betas (0.9, 0.95)                                              0.30  0.58  0.998 / 0.32  0.65  0.998 / 0.32  0.65  0.999
    control b1 m + (1 - b1) g'                               m' 0.74
    devias_grad_sumsq_multi   aligned / offset gradient      0.06 / 0.06                0.10 / 0.02
    devias_clip_coef     norm, coefficient                   0.07, 0.21                 0.23 (the worse of the two)
    FusedAdamW.step      multi-tensor with clip / per tensor                            0.99 / 0.99;  last_grad_norm 0.015
p' reaches 0.9995 by the rounding of the result alone: a parameter just above a power of two (1.0003) takes half an ulp = u; every other term is orders below it there.
Before the kernels took (float)(1.0 - beta) from the host, the same tests measured exp_avg_sq at 54 (devias_adamw_multi and devias_adamw_step, fresh state, betas
(0.9, 0.999); the emulation of 1.0f - fl32(beta) gives 54.5) and exp_avg at 1.08 ... 1.14; with (0.9, 0.95) exp_avg_sq at 1.05 ... 1.17.
"""
import math

import torch

from kernel_bounds import U_FP32, _randn, graded

CHUNK = 16384                      # DEVIAS_OPT_CHUNK, include/devias_amd.h
N_SCALE = 3                        # roundings of the gradient's scaling (r_g)
CLIP_EPS = 1e-6                    # clip_grad_norm_'s constant, :247
G_EXP = (-34, -8)                  # powers of two of the graded gradient
BETAS = ((0.9, 0.999), (0.9, 0.95))


def fl32(x):
    """the fp32 value nearest to the double x, as a double"""
    return float(torch.tensor(x, dtype=torch.float64).float())


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_ref(p, g, m, v, *, lr, wd, beta1, beta2, eps, step, grad_scale=1.0, coef=1.0, coef_err=0.0):
    """{"p": (ref, bound), "m": (ref, bound), "v": (ref, bound)} of one AdamW step on the fp32 tensors p, g, m, v (module docstring).  coef: the clip coefficient as
    a float (the float64 reference value); coef_err: its bound, carried through d / d coef into all three."""
    u = U_FP32
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    c1, c2 = 1.0 - beta1, 1.0 - beta2
    bc1, bc2s = 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)
    rg = (0.0 if (grad_scale == 1.0 and coef == 1.0) else N_SCALE * u) + (coef_err / abs(coef) if coef_err else 0.0)
    gp = g * (float(grad_scale) * float(coef))
    mn = m + c1 * (gp - m)
    e_m = u * mn.abs() + 3 * u * c1 * (gp.abs() + m.abs()) + (abs(fl32(beta1) - beta1) + u * beta1) * m.abs() + c1 * gp.abs() * rg
    t1, t2 = beta2 * v, c2 * gp * gp
    vn = t1 + t2
    e_v = u * vn + 2 * u * t1 + 3 * u * t2 + 2 * t2 * rg
    A = vn.sqrt() / bc2s
    D = A + eps
    e_sqrt = torch.where(vn > 0, e_v / (2 * vn).clamp_min(2.0 ** -300), torch.zeros_like(vn)) + u
    e_D = A * e_sqrt + 3 * u * A + u * eps + u * D
    Q = mn / D
    U = (lr / bc1) * Q
    e_U = (lr / bc1) * (e_m / D + Q.abs() * e_D / D) + 5 * u * U.abs()
    pd = p * (1.0 - lr * wd)
    pn = pd - U
    e_p = u * pn.abs() + (0.0 if wd == 0.0 else (2 + 3 * lr * wd) * u) * pd.abs() + e_U
    return {"p": (pn, e_p), "m": (mn, e_m), "v": (vn, e_v)}


def adamw_inputs(n, seed=0, device="cpu"):
    """(p, g) fp32 [n], graded independently (module docstring)"""
    i = torch.arange(n, dtype=torch.int64, device=device)
    lo, hi = G_EXP
    period = hi - lo + 1                                      # 27
    r = _randn((n,), seed + 1, device)
    r = torch.where(r.abs() < 2.0 ** -6, torch.full_like(r, 2.0 ** -6), r)
    g = r * torch.pow(torch.tensor(2.0, dtype=torch.float64, device=device), ((14 * i) % period + lo).double()).float()
    g[i % 31 == 5] = 0.0
    p = _randn((n,), seed + 2, device) * graded(n, 6, device).float()
    p[i % 37 == 3] = 0.0
    return p, g


def adamw_state(g, kind, scale=1.0, seed=0):
    """(m, v) fp32: `fresh` zeros; `warm` m = g' (1 + 2^-6 randn), v = g'^2 (1 + randn / 8) with g' = g scale"""
    if kind == "fresh":
        return torch.zeros_like(g), torch.zeros_like(g)
    gp = g.double() * scale
    n, dev = g.numel(), g.device
    m = (gp * (1.0 + 2.0 ** -6 * _randn((n,), seed + 3, dev).double())).float()
    v = (gp * gp * (1.0 + 0.125 * _randn((n,), seed + 4, dev).double().clamp(-4, 4))).float()
    return m, v


# ------------------------------------------------------------------------------------------------ gradient norm
def sumsq_depth(length, aligned=True):
    """the longest chain of fp32 roundings one addend of sumsq_multi_kernel goes through, for a chunk of `length` elements"""
    if aligned:
        return 1 + 3 + -(-(length >> 2) // 256) + 1 + 6 + 3
    return 1 + -(-length // 256) + 6 + 3


def sumsq_ref(g, aligned=True):
    """(partials, bounds) float64 [ceil(n / CHUNK)] of the fp32 gradient g (one chunk, or a whole tensor: one partial per chunk)"""
    g = g.double().reshape(-1)
    n = g.numel()
    k = -(-n // CHUNK)
    sq = torch.zeros(k * CHUNK, dtype=torch.float64, device=g.device)
    sq[:n] = g * g
    s = sq.reshape(k, CHUNK).sum(1)
    lens = [min(CHUNK, n - c * CHUNK) for c in range(k)]
    depth = torch.tensor([sumsq_depth(ln, aligned) for ln in lens], dtype=torch.float64, device=g.device)
    return s, depth * U_FP32 * s


def clip_depth(n):
    return -(-n // 256) + 8


def clip_ref(partials, max_norm, partials_err=None):
    """{"norm": (ref, bound), "coef": (ref, bound)} as Python floats, from the partials (the fp32 tensor the kernel reads, or float64 references with `partials_err`)"""
    u = U_FP32
    n = partials.numel()
    total = float(partials.double().sum()) if n else 0.0
    e_tot = clip_depth(n) * u * total + (float(partials_err.double().sum()) if partials_err is not None and n else 0.0)
    norm = math.sqrt(total)
    e_norm = (e_tot / (2 * norm) if norm > 0 else math.sqrt(e_tot)) + u * norm
    if not max_norm > 0:
        return {"norm": (norm, e_norm), "coef": (1.0, 0.0)}
    den = norm + CLIP_EPS
    c = max_norm / den
    e_c = c * (e_norm + u * CLIP_EPS + u * den) / den + 2 * u * c
    if c - e_c > 1.0:
        return {"norm": (norm, e_norm), "coef": (1.0, 0.0)}
    return {"norm": (norm, e_norm), "coef": (min(1.0, c), e_c)}


def sumsq_inputs(n, hot=(), seed=0, device="cpu", scale=2.0 ** -10):
    """fp32 [n]: randn at `scale`, mildly graded; the `hot` indices hold +-(1 ... 2), far above everything else"""
    g = _randn((n,), seed, device) * graded(n, 3, device).float() * scale
    for j, i in enumerate(hot):
        g[i] = (1.0 + 0.25 * (j % 4)) * (-1.0 if j % 2 else 1.0)
    return g


def hot_tail(n):
    """the indices of the len & 3 tail of the tensor's last chunk (empty when n is a multiple of 4)"""
    return tuple(range(n - (n & 3), n))


def scalar_ratio(out, ref, bound):
    return abs(float(out) - ref) / (bound + 2.0 ** -126)
