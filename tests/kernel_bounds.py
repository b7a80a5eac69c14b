"""Per-element error bounds against float64 for the GEMM, LayerNorm, attention (with and without dropout) and element-wise kernels, on graded inputs.

A plain helper module (like grad_compare.py and golden_util.py): no fixtures, no plugin.  Everything here is torch arithmetic on whatever
device the arguments live on -- float64 on the GPU in tests/test_kernel_bounds_gpu.py (none of this project's kernels), the CPU in
tests/test_kernel_bounds_cpu.py.

Why: `rel(a, b) = max|a - b| / max|b|` on single-scale randn data cannot see an error confined to rows or columns that are small next to
the tensor's largest element (a sub-tile that misses a k-step, a tail whose bias is not added, a dropped ragged key), nor one extra bf16
rounding.  Here every element is held to the first-order error bound of an IDEAL implementation of the documented algorithm, and the
inputs are graded so that every tile, third, wave slice and ragged tail holds every scale.

Unit roundoffs: u_bf16 = 2^-8, u_fp32 = 2^-24.   excess(out, ref, bound) = max |out - ref| / bound;   a test asserts excess <= 1.

Each *_ref function returns (ref, bound) tensors of the output's shape (or a dict of such pairs).  One named term per rounding the
kernel's design makes, nothing else:  (Kernel sources are cited by file name: gemm.hip, gemm_common.h, common.h, layernorm.hip, attn_fwd.hip, attn_mfma16.hip, attn_f32.hip,
attn_bwd1w.hip, attn_common.h, attention.hip, elementwise.hip live in devias_amd/csrc/, devias_amd.h is include/devias_amd.h.)

GEMM (devias_gemm, every layout and kernel form; include/devias_amd.h "epilogue order")
    pre   = A B + bias                      fp32 accumulation, any order:     e_pre = (K + 8) u_fp32 (|A||B| + |bias|)
    out   = f(pre) * row_scale + res        stored once:                      u_out |ref| + (K + 8) u_fp32 S,
            S = |A||B| + |bias| + |res| (res also stands for the positional table of res_mod), + |beta C_old| for fp32 C (out_f32 / wgrad)
    activations propagate e_pre through |f'| and add the term of the device function:
        GELU   fp32 erff: 8 u_fp32 |x|;   bf16: the degree-17 polynomial of devias_amd/csrc/common.h:124-139, |erf error| <= 6e-5 scaled by 1 + 6e-5
               -> 0.5 |x| 1.3e-4 (a rounding the design makes on purpose: the fit is an order of magnitude below bf16 resolution)
        dGELU  (aux_in exact) fp32 erff + expf: 16 u_fp32 |A B|;   bf16: devias_amd/csrc/common.h:127,141-144, |error| <= 5.3e-4 -> 5.5e-4 |A B| with its fp32 evaluation
        sigmoid expf: 8 u_fp32 |y|;   ReLU / dReLU: exact (a sign that e_pre can flip counts |f'| = 1)
    aux_out  its own rounding of the fp32 pre-activation (gemm_common.h:145-149: stored BEFORE the activation, which continues in fp32):
             u_out |pre| + e_pre
    colsum   sums of the fp32 values BEFORE rounding (gemm_common.h:183-186): (M/128 + 128 + 8) u_fp32 sum|.| for the summation, PLUS the sum over the rows of
             each addend's own fp32 bound part ((K + 8) u_fp32 S and the activation term): the addends are fp32 values that carry that error against
             float64 before they are summed.  This second term is not in the issue's statement of the bound and makes it several times looser at
             large K and under dGELU (its polynomial term, 5.5e-4 |A B| per addend, dominates): sums taken after the bf16 store are told apart by the
             plain `colsum` epilogue (no activation, small K), not by the dGELU one -- the GPU tests run both on every kernel that fuses the sums.
             Where devias_gemm falls back to devias_colsum over the stored C (gemm.hip:338) u_out sum|C| on top.

LayerNorm (devias_amd/csrc/layernorm.hip: one wave per row, fp32 statistics, two-pass variance, one rounding of the output)
    forward   mean: (D + 2) u sum|x| / D;   rstd: rstd ((D + 8) u / 2 + 4 u + e_mean^2 / (2 (var + eps)))  (two-pass: first order in e_mean vanishes);
              y: u_out |y| + |gamma| (rstd (2 u |x - mean| + e_mean) + |x - mean| e_rstd) + 3 u (|xhat gamma| + |beta|)      (rigorous, factor 1)
    backward  a = dy gamma, m1 = mean(a), m2 = mean(a xhat), dx = rstd (a - m1 - xhat m2) (+ dres), against the SUM OF ABSOLUTE TERMS
              |a| + |m1| + |xhat m2| (cancellation-aware); dgamma / dbeta / dx_colsum as fp32 column sums over M rows, any order;
              dres is added in fp32 BEFORE the one rounding of dx (layernorm.hip:205-211); dx_colsum sums the fp32 values before rounding (:207).
              The reference takes the same saved mean / rstd tensors the kernel is given.

MHSA forward (devias_amd/csrc/attn_fwd.hip; bf16: q' = bf16(q c), c = scale log2 e, attn_fwd.hip:49-59; P rounded to bf16 for the P V product; o rounded once)
    o:   u (|o| + sum_j p_j |v_j| + sum_j p_j T_j |v_j - o|) + 64 u_fp32 (sum_j p_j |v_j| + sum_j p_j T_j |v_j - o|),   T_j = scale sum_d |q_d| |k_jd|
         The last term is the fp32 accumulation of a score's 64 products (fp32 kernel: the sequential FMA chain of attn_f32.hip:45-47; bf16: the MFMAs' fp32
         accumulators).  It is invisible next to u_bf16, but with u = u_fp32 the q-rounding term alone counts ONE rounding per score where the kernel makes 64:
         without it, at this slack, the fp32 forward kernel measured 1.18 at B, N, H = 1, 1569, 1, logit std 6 (0.44 with it).
    lse: u sum_j p_j T_j  (+ the fp32 floor 64 u_fp32 (sum_j p_j T_j + 1) + 4 u_fp32 |lse|)
    Under DEVIAS_ATTN_Q_PRESCALED the reference is taken on the q the kernels see (q' / c): the q' rounding is the caller's and its term is dropped.
    fp32 inputs: u = u_fp32 throughout.

MHSA backward (include/devias_amd.h:256-277; dS = P o (dP - delta), delta = rowsum(dO o O) from the STORED o)
    kernel probabilities  p^ = p (1 + eps),  |eps_ij| <= E_ij:
        plain path      E_ij = u (T_ij + sum_j p_j T_j): the backward rounds q c (dQ kernel, attn_mfma16.hip:204-208) or k c (one-wave dK / dV kernel,
                        attn_bwd1w.hip:251-256) or nothing (two-wave kernel, attn_mfma16.hip:471) while the saved lse came from the forward's q c
                        (devias_amd.h:273-274: "differ ... by two bf16 roundings")
        pre-scaled path E_ij = 0: all kernels multiply the SAME bf16 operands (devias_amd.h:274-275)
        both            + 64 u_fp32 (T_ij + sum_j p_j T_j + 1)
    delta:  sum_d |dO_d| bound_o_d + 64 u_fp32 sum_d |dO_d o_d|             (o is an input that carries the forward's bound)
    dS:     p ((E + u) |dP - delta| + 64 u_fp32 |dO||v| + e_delta)          (P and dS are rounded to bf16 for their MFMAs: attn_mfma16.hip:323, 484-489)
    dQ = scale dS k,  dK = scale dS^T q,  dV = P^T dO:  the propagated term + u_out |result| + 64 u_fp32 of the absolute products
    dbq / dbv (the _bias entry point): fp32 column sums over all B N rows (from the accumulators in bf16; dbv = colsum(dO) where
    devias_mhsa_bwd_bias_dv_from_do says so -- the same value, softmax rows sum to one).

MHSA with dropout (attn_common.h:40-50: element (b, h, query, key) of the softmax matrix is kept when a hash of (seed, b H + h, i, j) is below keep 2^32, and kept
elements are scaled by 1 / keep; oracle.ref_cpu.attn_drop_mask restates the hash, and its fp32 values widened are the `mask` of the references, 0 or 1 / keep.
Never with the pre-scaled path: attention.hip:112 refuses it.)  With pm = p o mask:
    forward   o = pm v; the probability that is rounded to bf16 for the P V product is the fp32 product p mask (attn_fwd.hip:146; fp32: attn_f32.hip:50), so
              pv = pm |v|.  Row sums and lse are of the UN-dropped p: the lse reference and bound are unchanged.  A perturbation eps_j of score j moves o by
              sum_j p_j eps_j (mask_j v_j - o): the score-rounding term is sum_j p_j T_j |mask_j v_jd - o_d|.  Otherwise the formula above.
    backward  dP = mask o (dO v^T) (attn_mfma16.hip:315, 473-478; fp32: attn_f32.hip:111, 172), |dP| <= mask o (|dO| |v|^T); delta = rowsum(dO o o) from the stored
              DROPPED o, with its masked forward bound; dS = p o (dP - delta); dV = pm^T dO with its propagated term built from pm; dQ, dK from that dS as before.
              E keeps the plain path's term: the dropout dQ kernel and the two-wave dK / dV kernel round no operand, but the saved lse came from the forward's q c.
              dbq / dbv: column sums as before, without the colsum(dO) alternative (under a mask it is no longer dbv); with option attn_bias_fused = 0 the sums are
              taken from the stored dqkv (devias_colsum over its thirds): + u_out sum_rows |.|.
    The slacks are those of attention without dropout; the dropout emulation needs less than they allow (table below).

Element-wise kernels (devias_amd/csrc/elementwise.hip; all rigorous with factor 1 but act_bwd, which carries SLACK_ACT for its device transcendental)
    mul_mask     y = a mask (+ b):  u_out |y| + 2 u_fp32 (|a mask| + |b|)         (the fp32 product and sum, :169-171)
    row_scale, cast_scale   y = x s:  u_out |y| + u_fp32 |y|                       (one fp32 product, :36-39, :189)
    add          u_out |y| + u_fp32 (|a| + |b|)                                     (:158-161)
    act_bwd      sigmoid g y (1 - y) from the stored output: 3 u_fp32 |.|;  ReLU: exact;  GELU g gelu'(x) from the stored pre-activation: the dGELU term of the
                 GEMM epilogue above (16 u_fp32 |g|, + DGELU_POLY_ERR |g| in bf16)    (:178-180)
    colsum       out = beta out_old + sum_m x:  depth u_fp32 (sum|x| + |beta out_old|), depth = the longest chain of fp32 additions an addend goes through in
                 the summation tree (:66-69, 76-132):  stage 1, per 256-row block: each of 8 row lanes adds its 32 rows in order (32), the 8 lane sums are added in
                 order (8);  stage 2 (more than one block): each of 16 lanes adds every 16th block partial, ceil(ceil(M / 256) / 16) of them, and the 16 lane
                 sums are added in order (16);  + 8 for beta out_old and its sum.  depth = 32 + 8 + ceil(ceil(M / 256) / 16) + 16 + 8.
    rows_reduce_mod   one sequential chain per output (:139-141):  (M / mod + 1) u_fp32 sum|x|
    cast, rows_broadcast, patch_im2col   exact: torch.equal against .to(dtype)
    Inputs: graded over the flat index; for colsum and rows_reduce_mod the COLUMNS are graded and the rows are at one scale (columns_inputs).

Constants.  The GEMM and LayerNorm-forward bounds are rigorous; their factor is 1.  The activation, LayerNorm-backward and attention bounds
hold first-order arguments and a device transcendental: each carries ONE scalar slack on the whole bound, set so that the CPU emulation
(the float64 reference plus exactly the named roundings, torch CPU arithmetic: tests/test_kernel_bounds_cpu.py) stays at <= 0.5 over all
generators; the margin of 2 covers summation order and exp2 / erf differences between torch CPU and the device.  Never fitted to the HIP
kernels.  A bf16 output alone reaches ratio ~1 at slack 1 (u_bf16 is attained next to powers of two), so these slacks are about 2.

    bound               slack   emulation's worst ratio at that slack (test_kernel_bounds_cpu.py prints them)
    GEMM, no activation   1     0.99 bf16 (the output rounding alone), 0.05 fp32;  aux_out 0.99 / 0.05;  fused colsum 0.01
    LayerNorm forward     1     y 0.99 bf16, 0.13 fp32;  mean 0.01;  rstd 0.01
    activations           2     0.49 bf16 (GELU 0.487, ReLU 0.492, sigmoid 0.494, dGELU 0.485, dReLU 0.489), 0.22 fp32 (sigmoid);  colsum 0.17
    LayerNorm backward    2     dx 0.50 bf16, 0.15 fp32;  dgamma 0.02;  dbeta 0.02;  dx_colsum 0.002
    attention forward     1.4486  out 0.50 (bf16, pre-scaled q, logit std 6), 0.34 pre-scaled diffuse, 0.29 bf16 plain, 0.02 fp32;  lse 0.16
    attention backward    1.6086  dV 0.50 (bf16, pre-scaled q, logit std 6), dQ 0.24, dK 0.22;  plain path 0.10;  fp32 0.01;  dbq 0.01, dbv 0.08
    attention dropout, fwd  1.4486  out 0.45 (bf16, keep 0.9, logit std 6), 0.29 keep 0.5, 0.03 fp32;  lse 0.16 (bf16), 0.01 fp32      (the slacks of attention: unchanged)
    attention dropout, bwd  1.6086  dQ 0.07, dK 0.07, dV 0.12 (bf16, keep 0.5, logit std 6);  fp32 <= 0.01;  dbq 0.001, dbv 0.014;  from the stored tensor 0.002 / 0.015
    element-wise            1     bf16 stores reach 0.88 - 1.00; fp32: mul_mask 0.45, add 0.49, row_scale 0.50, cast_scale 0.42;  colsum <= 0.015;  rows_reduce_mod 0.02
    act_bwd                 2     sigmoid 0.49 bf16 / 0.31 fp32, GELU 0.48 / 0.07, ReLU 0 (exact)
Each slack is twice what the emulation needs to stay at 1: 0.99 and 0.99 (a bf16 store: 2), 0.72422 -> 2 x 0.7243, 0.80425 -> 2 x 0.8043.

Where this departs from the issue's "done when": it asks the emulation at <= 0.5 for EVERY operation.  Under the factor-1 bounds (GEMM without activation, aux_out,
LayerNorm forward) the one bf16 store of the ideal result already reaches 0.99, so there the emulation is held to <= 1 and to <= 0.5 only under the slack-bearing bounds.
The attention generators (ATTN_GENERATORS): logit std 1 (diffuse), logit std 6 (peaked), and logit std 1 over keys that carry a common offset.  The offset makes
T large (~100): under the plain path's bound, whose score-rounding term grows with T, that generator holds the plain kernels to little and the forward mutants are
asserted on the two offset-free generators there (and on all three under the pre-scaled path's bound, which has no such term).  It exists for the roundings OF THE
SCORES: without it one bf16 rounding of k c moves P by less than P's own rounding at diffuse attention (the seeded mutant of the pre-scaled backward: 0.53 at logit
std 1 without the offset, 3.9 with it, 2.9 at logit std 6), so that mutant is asserted on the offset and the peaked generator and reported on the plain diffuse one.
"""
import math

import torch

U_BF16 = 2.0 ** -8
U_FP32 = 2.0 ** -24
SLACK_ACT = 2.0
SLACK_LN_BWD = 2.0
SLACK_ATTN_FWD = 2 * 0.7243      # the emulation needs 0.72422
SLACK_ATTN_BWD = 2 * 0.8043      # the emulation needs 0.80425
ERF_POLY_ERR = 1.3e-4          # devias_amd/csrc/common.h:126,138
DGELU_POLY_ERR = 5.5e-4        # devias_amd/csrc/common.h:127 (fit error 5.3e-4) + its fp32 Horner evaluation
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SIGMOID, ACT_DGELU, ACT_DRELU = 0, 1, 2, 3, 4, 5


def u_of(dtype):
    return U_BF16 if dtype == torch.bfloat16 else U_FP32


# ------------------------------------------------------------------------------------------------ graded inputs
def graded(n, spread=6, device="cpu"):
    """power-of-two scales 2^e_i, e_i cycling through [-spread, +spread] with an odd period 2 spread + 1 (coprime to 16 ... 256; spread 6:
    e_i = (7 i mod 13) - 6): every tile, third, wave slice and ragged tail holds every scale, and bf16 values stay exact under the scaling"""
    if spread == 0:
        return torch.ones(n, dtype=torch.float64, device=device)
    period = 2 * spread + 1
    mult = next(m for m in range(period // 2 + 1, 2 * period) if math.gcd(m, period) == 1)
    e = (mult * torch.arange(n, dtype=torch.int64, device=device)) % period - spread
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=device), e.double())


def _randn(shape, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32).to(device)


def gemm_inputs(M, N, K, dtype, spread=6, seed=0, device="cpu", res_rows=None):
    """A [M, K] with graded rows, B [N, K] with graded output columns, bias fp32 [N] graded, res [M (or res_rows), N] graded by the outer product"""
    rm, cn = graded(M, spread, device).float(), graded(N, spread, device).float()
    A = (_randn((M, K), seed + 1, device) * rm[:, None]).to(dtype)
    B = (_randn((N, K), seed + 2, device) * 0.25 * cn[:, None]).to(dtype)
    bias = _randn((N,), seed + 3, device) * cn
    R = M if res_rows is None else res_rows
    res = (_randn((R, N), seed + 4, device) * rm[:R, None] * cn[None, :]).to(dtype)
    return A, B, bias, res


def layernorm_inputs(M, D, dtype, spread=6, seed=0, device="cpu"):
    """rows graded, a per-row mean offset of 0 / 0.5 / 100 row standard deviations, gamma crossing zero"""
    rm = graded(M, spread, device).float()
    off = torch.tensor([0.0, 0.5, 100.0], device=device)[torch.arange(M, device=device) % 3]
    x = ((_randn((M, D), seed + 1, device) + off[:, None]) * rm[:, None]).to(dtype)
    gamma = torch.linspace(-1.0, 1.5, D, device=device) + 0.01 * _randn((D,), seed + 2, device)
    beta = 0.1 * _randn((D,), seed + 3, device)
    dy = (_randn((M, D), seed + 4, device) * graded(M, spread, device).flip(0).float()[:, None]).to(dtype)
    dres = (_randn((M, D), seed + 5, device) * rm[:, None] * 0.5).to(dtype)
    return x, gamma, beta, dy, dres


# (logit std, key offset): diffuse attention; diffuse attention over keys with a common offset (large T: score roundings matter); peaked attention
ATTN_GENERATORS = ((1.0, 0.0), (1.0, 16.0), (6.0, 0.0))


def attention_inputs(B, N, H, dtype, logit_std=1.0, spread=6, seed=0, device="cpu", key_offset=0.0):
    """qkv [B N, 3 H 64] and dO [B N, H 64]: V and dO graded per head (2^-6, 1, 2^5, ...) and per key / query row; q, k at the given logit std
    (logit = scale q.k, scale = 1/8: std = a^2 for q, k ~ a randn).  key_offset adds the same vector (+-offset, alternating over the head dim) to every
    key: it shifts each row of logits by a constant, which the softmax does not see, but the products |q||k| (the T of the bounds) grow with it -- a
    rounding of the scores then matters at diffuse attention too, as it does for real keys with a common component."""
    a = math.sqrt(logit_std)
    head = torch.tensor([2.0 ** -6, 1.0, 2.0 ** 5], device=device)[torch.arange(H, device=device) % 3]
    rows = graded(N, min(spread, 3), device).float()
    x = _randn((B, N, 3, H, 64), seed + 1, device)
    x[:, :, 0] *= a
    x[:, :, 1] *= a
    x[:, :, 1] += key_offset * (1.0 - 2.0 * (torch.arange(64, device=device) % 2))
    x[:, :, 2] *= head[None, None, :, None] * rows[None, :, None, None]
    d_o = _randn((B, N, H, 64), seed + 2, device) * head.flip(0)[None, None, :, None] * rows.flip(0)[None, :, None, None]
    return x.reshape(B * N, 3 * H * 64).to(dtype), d_o.reshape(B * N, H * 64).to(dtype)


def attention_prescale(qkv, B, N, H, scale):
    """DEVIAS_ATTN_Q_PRESCALED: (the tensor a caller passes, its q third q' = bf16(q scale log2 e);  the float64 values the kernels then see with the UNSCALED q, q' / c)"""
    c = scale * 1.4426950408889634
    t = qkv.float().reshape(B * N, 3, H * 64).clone()
    t[:, 0] *= c
    pre = t.to(torch.bfloat16)
    seen = pre.double()
    seen[:, 0] /= c
    return pre.reshape(B * N, -1), seen.reshape(B * N, -1)


# ------------------------------------------------------------------------------------------------ the measure
def excess(out, ref, bound):
    """(max |out - ref| / bound, flat index of the worst element); a non-finite output is infinitely wrong.  The smallest normal fp32 number is added to
    every bound: below it the formats (and the kernels, which flush denormals) hold no relative precision."""
    out = out.double().reshape(-1)
    ref, bound = ref.reshape(-1), bound.reshape(-1)
    ratio = (out - ref).abs() / (bound + 2.0 ** -126)
    ratio = torch.where(torch.isfinite(out), ratio, torch.full_like(ratio, float("inf")))
    worst = int(torch.argmax(ratio))
    return float(ratio[worst]), worst


def where2d(idx, ncols):
    r, c = divmod(int(idx), int(ncols))
    return f"(row {r}, col {c}; 256-tile ({r // 256}, {c // 256}), row {r % 256} / col {c % 256} within it)"


def where_attn(idx, N, H):
    """index into a [B N, H 64] tensor"""
    row, col = divmod(int(idx), H * 64)
    return f"(b {row // N}, h {col // 64}, row {row % N}, d {col % 64})"


def check(name, out, ref, bound, where=None, limit=1.0):
    """assert excess <= limit with a message that names the element, and return the ratio"""
    r, idx = excess(out, ref, bound)
    loc = where(idx) if where is not None else f"(flat index {idx})"
    assert r <= limit, (f"{name}: worst |out - ref| / bound = {r:.3g} > {limit:g} at {loc}: out {float(out.reshape(-1)[idx]):.9g} "
                        f"ref {float(ref.reshape(-1)[idx]):.9g} bound {float(bound.reshape(-1)[idx]):.3g}")
    return r


# ------------------------------------------------------------------------------------------------ GEMM
def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gemm_ref(A, Bt, dtype, *, bias=None, res=None, res_mod=0, act=ACT_NONE, aux_in=None, row_scale=None, rows_per_scale=0,
             out_f32=False, beta=0.0, c_old=None, colsum_old=None, colsum_beta=0.0, colsum_from_stored=False):
    """A [M, K], Bt [K, N] (the caller applies trans_a / trans_b), any dtype; `dtype` is the operand dtype of the kernel call.
    Returns {"out": (ref, bound), "aux": (ref, bound) for GELU, "colsum": (ref, bound)}."""
    A, Bt = A.double(), Bt.double()
    M, K = A.shape
    N = Bt.shape[1]
    u_out = U_FP32 if (out_f32 or dtype == torch.float32) else U_BF16
    kf = (K + 8) * U_FP32
    prod = A @ Bt
    s_pre = A.abs() @ Bt.abs()
    pre = prod
    if bias is not None:
        pre = pre + bias.double()
        s_pre = s_pre + bias.double().abs()
    e_pre = kf * s_pre
    slack = 1.0
    e_f = torch.zeros_like(pre)
    if act == ACT_NONE:
        y, e_y = pre, e_pre
    else:
        slack = SLACK_ACT
        if act == ACT_GELU:
            y = gelu64(pre)
            e_f = (8 * U_FP32 if dtype == torch.float32 else 0.5 * ERF_POLY_ERR + 8 * U_FP32) * pre.abs()
            e_y = dgelu64(pre).abs() * e_pre + e_f
        elif act == ACT_RELU:
            y = pre.clamp_min(0.0)
            e_y = ((pre > 0) | (pre.abs() <= e_pre)).double() * e_pre
        elif act == ACT_SIGMOID:
            y = torch.sigmoid(pre)
            e_y = y * (1 - y) * e_pre + 8 * U_FP32 * y
        elif act == ACT_DGELU:
            d = dgelu64(aux_in.double())
            y = pre * d
            e_y = d.abs() * e_pre + (16 * U_FP32 if dtype == torch.float32 else DGELU_POLY_ERR + 16 * U_FP32) * pre.abs()
        elif act == ACT_DRELU:
            d = (aux_in.double() > 0).double()
            y, e_y = pre * d, d * e_pre
        else:
            raise ValueError(act)
    if row_scale is not None:
        rs = row_scale.double().repeat_interleave(rows_per_scale)[:M, None]
        y, e_y = y * rs, e_y * rs.abs() + U_FP32 * (y * rs).abs()
    ref = y
    extra = torch.zeros_like(ref)
    if res is not None:
        r = res.double()
        r = r.repeat((M + res_mod - 1) // res_mod, 1)[:M] if res_mod > 0 else r
        ref = ref + r
        extra = extra + r.abs()
    if beta != 0.0:
        ref = ref + beta * c_old.double()
        extra = extra + (beta * c_old.double()).abs()
    f32_part = e_y + kf * extra                 # everything but the rounding of the stored value
    out = {"out": (ref, slack * (u_out * ref.abs() + f32_part))}
    if act == ACT_GELU:
        out["aux"] = (pre, u_out * pre.abs() + e_pre)
    cs_ref = ref.sum(0)
    cs_abs = ref.abs().sum(0)
    if colsum_old is not None and colsum_beta != 0.0:
        cs_ref = cs_ref + colsum_beta * colsum_old.double()
        cs_abs = cs_abs + (colsum_beta * colsum_old.double()).abs()
    cs_bound = f32_part.sum(0) + (M / 128 + 128 + 8) * U_FP32 * cs_abs
    if colsum_from_stored:
        cs_bound = cs_bound + u_out * ref.abs().sum(0)
    out["colsum"] = (cs_ref, slack * cs_bound)
    return out


def gelu_poly_fp32(x):
    """the bf16 kernels' GELU (devias_amd/csrc/common.h gelu_fast) in torch fp32: the documented algorithm, for the CPU emulation"""
    x = x.float()
    t = x.clamp(-4.0, 4.0) * 0.25
    u = t * t
    c = (2.681678368e+00, -1.466233920e+01, 3.579562272e+01, -5.219407220e+01, 5.153296562e+01, -3.705950413e+01, 2.021369346e+01, -8.499460359e+00, 3.191358921e+00)
    p = torch.full_like(u, c[0])
    for k in c[1:]:
        p = p * u + k
    e = (p * t * 1.00006).clamp(-1.0, 1.0)
    return x * (0.5 + 0.5 * e)


def dgelu_poly_fp32(x):
    """devias_amd/csrc/common.h dgelu_fast in torch fp32"""
    x = x.float()
    t = x.clamp(-4.0, 4.0) * 0.25
    u = t * t
    c = (1.612753209e+01, -8.526842075e+01, 1.980196598e+02, -2.676213605e+02, 2.352999263e+02, -1.420446591e+02, 5.973788243e+01, -1.694027150e+01, 3.190259248e+00)
    p = torch.full_like(u, c[0])
    for k in c[1:]:
        p = p * u + k
    return 0.5 + p * t


# ------------------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd_ref(x, gamma, beta, eps, dtype):
    """{"y", "mean", "rstd"}: (ref, bound) each; rigorous, factor 1"""
    x, g, b = x.double(), gamma.double(), beta.double()
    D = x.shape[1]
    u, u_out = U_FP32, u_of(dtype)
    mean = x.mean(1)
    xc = x - mean[:, None]
    var = (xc * xc).mean(1)
    rstd = (var + eps).rsqrt()
    e_mean = (D + 2) * u * x.abs().sum(1) / D
    e_rstd = rstd * ((D + 8) * u / 2 + 4 * u + e_mean * e_mean / (2 * (var + eps)))
    xh = xc * rstd[:, None]
    y = xh * g + b
    e_y = u_out * y.abs() + g.abs() * (rstd[:, None] * (2 * u * xc.abs() + e_mean[:, None]) + xc.abs() * e_rstd[:, None]) + 3 * u * ((xh * g).abs() + b.abs())
    return {"y": (y, e_y), "mean": (mean, e_mean), "rstd": (rstd, e_rstd)}


def layernorm_bwd_ref(dy, x, gamma, mean, rstd, dtype, dres=None, dgamma_old=None, dbeta_old=None, beta_acc=0.0):
    """{"dx", "dgamma", "dbeta", "dx_colsum"}: (ref, bound) each, for the SAME saved mean / rstd tensors the kernel is given"""
    dy, x, g, mu, rs = dy.double(), x.double(), gamma.double(), mean.double()[:, None], rstd.double()[:, None]
    M, D = x.shape
    u, u_out = U_FP32, u_of(dtype)
    xh = (x - mu) * rs
    a = dy * g
    m1 = a.mean(1, keepdim=True)
    m2 = (a * xh).mean(1, keepdim=True)
    e_xh = 3 * u * xh.abs()
    e_m1 = (D + 4) * u * a.abs().mean(1, keepdim=True)
    e_m2 = (D + 6) * u * (a * xh).abs().mean(1, keepdim=True) + (a.abs() * e_xh).mean(1, keepdim=True)
    dx = rs * (a - m1 - xh * m2)
    terms = a.abs() + m1.abs() + (xh * m2).abs()
    f32_part = rs * (6 * u * terms + e_m1 + xh.abs() * e_m2 + e_xh * m2.abs())
    if dres is not None:
        dx = dx + dres.double()
        f32_part = f32_part + u * (dres.double().abs() + dx.abs())
    s = SLACK_LN_BWD
    out = {"dx": (dx, s * (u_out * dx.abs() + f32_part))}
    col = (M + 8) * u
    dg, dg_abs = (dy * xh).sum(0), (dy * xh).abs().sum(0)
    db, db_abs = dy.sum(0), dy.abs().sum(0)
    e_dg = (dy.abs() * e_xh).sum(0)
    if beta_acc != 0.0:
        dg, dg_abs = dg + beta_acc * dgamma_old.double(), dg_abs + (beta_acc * dgamma_old.double()).abs()
        db, db_abs = db + beta_acc * dbeta_old.double(), db_abs + (beta_acc * dbeta_old.double()).abs()
    out["dgamma"] = (dg, s * (col * dg_abs + e_dg))
    out["dbeta"] = (db, s * col * db_abs)
    out["dx_colsum"] = (dx.sum(0), s * (f32_part.sum(0) + col * dx.abs().sum(0)))
    return out


# ------------------------------------------------------------------------------------------------ attention
def _heads(t, B, N, H, third=None):
    """[B N, (3) H 64] -> [B, H, N, 64] float64"""
    if third is None:
        return t.double().reshape(B, N, H, 64).permute(0, 2, 1, 3)
    return t.double().reshape(B, N, 3, H, 64)[:, :, third].permute(0, 2, 1, 3)


def _rows(t, B, N, H):
    """[B, H, N, 64] -> [B N, H 64]"""
    return t.permute(0, 2, 1, 3).reshape(B * N, H * 64)


def _attn_core(qkv, B, N, H, scale):
    q, k, v = (_heads(qkv, B, N, H, i) for i in range(3))
    s = scale * (q @ k.transpose(-1, -2))
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    T = scale * (q.abs() @ k.abs().transpose(-1, -2))
    return q, k, v, p, lse, T


def mhsa_fwd_ref(qkv, B, N, H, scale, dtype, q_rounded=True, mask=None):
    """qkv: the values the kernels see, with the UNSCALED q (q' / c under DEVIAS_ATTN_Q_PRESCALED, then q_rounded = False: the rounding was the caller's).
    mask: attention dropout, float64 [B, H, N, N] of 0 or 1 / keep (never with the pre-scaled path).
    {"out": (ref, bound) [B N, H 64], "lse": (ref, bound) [B, H, N]}"""
    assert mask is None or q_rounded, "attention dropout is not offered with DEVIAS_ATTN_Q_PRESCALED"
    q, k, v, p, lse, T = _attn_core(qkv, B, N, H, scale)
    u = u_of(dtype)
    sr = 1.0 if (q_rounded or dtype == torch.float32) else 0.0
    pm = p if mask is None else p * mask
    o = pm @ v
    pv = pm @ v.abs()
    pT = (p * T).sum(-1)
    w = p * T
    wv = torch.empty_like(o)
    for d in range(64):
        vd = v[..., None, :, d] if mask is None else mask * v[..., None, :, d]
        wv[..., d] = (w * (vd - o[..., :, None, d]).abs()).sum(-1)
    s = SLACK_ATTN_FWD
    b_o = s * (u * (o.abs() + pv + sr * wv) + 64 * U_FP32 * (pv + wv))
    b_l = s * (u * sr * pT + 64 * U_FP32 * (pT + 1.0) + 4 * U_FP32 * lse.abs())
    return {"out": (_rows(o, B, N, H), _rows(b_o, B, N, H)), "lse": (lse, b_l)}


def mhsa_bwd_ref(qkv, d_o, B, N, H, scale, dtype, plain=True, mask=None, bias_from_stored=False):
    """plain = False: the DEVIAS_ATTN_Q_PRESCALED path (qkv holds q' / c: the backward's scores ARE the forward's, no score term).
    mask: attention dropout, float64 [B, H, N, N] of 0 or 1 / keep (plain path only).  bias_from_stored: dbq / dbv are column sums of the STORED dqkv
    (option attn_bias_fused = 0 in bf16; the fp32 kernels always).
    {"dq", "dk", "dv"}: (ref, bound) [B N, H 64] each; {"dbq", "dbv"}: (ref, bound) [H 64]"""
    assert mask is None or plain, "attention dropout is not offered with DEVIAS_ATTN_Q_PRESCALED"
    q, k, v, p, lse, T = _attn_core(qkv, B, N, H, scale)
    dO = _heads(d_o, B, N, H)
    u, f = u_of(dtype), 64 * U_FP32
    sr = 1.0 if (plain or dtype == torch.float32) else 0.0
    fwd = mhsa_fwd_ref(qkv, B, N, H, scale, dtype, q_rounded=bool(sr), mask=mask)
    o, b_o = _heads(fwd["out"][0], B, N, H), _heads(fwd["out"][1], B, N, H)
    pT = (p * T).sum(-1, keepdim=True)
    E = u * sr * (T + pT) + f * (T + pT + 1.0)
    dP = dO @ v.transpose(-1, -2)
    aP = dO.abs() @ v.abs().transpose(-1, -2)
    if mask is not None:
        dP, aP, p_v = mask * dP, mask * aP, p * mask        # dP_ij = mask_ij (dO_i . v_j);  dV takes P o mask
    else:
        p_v = p
    delta = (dO * o).sum(-1, keepdim=True)
    e_delta = (dO.abs() * b_o).sum(-1, keepdim=True) + f * (dO * o).abs().sum(-1, keepdim=True)
    dS = p * (dP - delta)
    e_dS = p * ((E + u) * (dP - delta).abs() + f * aP + e_delta)
    s = SLACK_ATTN_BWD
    dq, dk, dv = scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), p_v.transpose(-1, -2) @ dO
    f_dq = scale * (e_dS @ k.abs()) + f * scale * (dS.abs() @ k.abs())
    f_dk = scale * (e_dS.transpose(-1, -2) @ q.abs()) + f * scale * (dS.abs().transpose(-1, -2) @ q.abs())
    f_dv = ((E + u) * p_v).transpose(-1, -2) @ dO.abs() + f * (p_v.transpose(-1, -2) @ dO.abs())
    out = {}
    for name, r, fp in (("dq", dq, f_dq), ("dk", dk, f_dk), ("dv", dv, f_dv)):
        out[name] = (_rows(r, B, N, H), _rows(s * (u * r.abs() + fp), B, N, H))
    col = (B * N / 128 + 128 + 8) * U_FP32
    stored = u if (bias_from_stored and dtype != torch.float32) else (U_FP32 if dtype == torch.float32 else 0.0)      # the sums are taken from the stored tensor
    for name, r, fp, also in (("dbq", dq, f_dq, None), ("dbv", dv, f_dv, dO if mask is None else None)):      # (under a mask colsum(dO) is no longer dbv)
        rr, ff = _rows(r, B, N, H), _rows(fp, B, N, H)
        bound = ff.sum(0) + (col + stored) * rr.abs().sum(0)
        if also is not None:
            bound = bound + col * _rows(also, B, N, H).abs().sum(0)
        out[name] = (rr.sum(0), s * bound)
    return out


# ------------------------------------------------------------------------------------------------ element-wise kernels (devias_amd/csrc/elementwise.hip)
def elementwise_inputs(n, dtype, seed=0, device="cpu", spread=6):
    """[n] values graded over the flat index"""
    return (_randn((n,), seed, device) * graded(n, spread, device).float()).to(dtype)


def columns_inputs(M, N, dtype, seed=0, device="cpu", spread=6):
    """[M, N] for the column / row-class sums: the COLUMNS graded, the rows at one scale -- a summed-away row then stands out at 1 / M of its column's sum against a
    bound of ~depth 2^-24; with graded rows the fp32 summation's own allowance would hide it"""
    return (_randn((M, N), seed, device) * graded(N, spread, device).float()[None, :]).to(dtype)


def drop_mask(n, keep, seed=0, device="cpu"):
    """an element-wise dropout mask as the model draws it: fp32 [n] of 0 or 1 / keep"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(n, generator=g) < keep).float() / torch.tensor(keep, dtype=torch.float32)).to(device)


def mul_mask_ref(a, mask, b, dtype):
    """y = a mask (+ b): the fp32 product and the fp32 sum round once each, against the sum of absolute terms (rigorous whether or not the compiler contracts
    them into one FMA); one rounding of the output"""
    am = a.double() * mask.double()
    y, s_abs = (am, am.abs()) if b is None else (am + b.double(), am.abs() + b.double().abs())
    e_mul, e_add = U_FP32 * s_abs, U_FP32 * s_abs
    return y, u_of(dtype) * y.abs() + e_mul + e_add


def row_scale_ref(x, scale, rows_per_scale, dtype):
    """y = x scale[row / rows_per_scale]: one fp32 product, one rounding of the output"""
    M = x.shape[0]
    y = x.double() * scale.double().repeat_interleave(rows_per_scale)[:M, None]
    return y, u_of(dtype) * y.abs() + U_FP32 * y.abs()


def cast_scale_ref(src, scale, out_dtype):
    """y = (out dtype)(src scale) with the fp32 value of `scale` the kernel is handed: one fp32 product, one rounding of the output"""
    y = src.double() * float(torch.tensor(scale, dtype=torch.float32))
    return y, u_of(out_dtype) * y.abs() + U_FP32 * y.abs()


def add_ref(a, b, dtype):
    y = a.double() + b.double()
    return y, u_of(dtype) * y.abs() + U_FP32 * (a.double().abs() + b.double().abs())


def act_bwd_ref(dy, y, act, dtype):
    """devias_act_bwd: sigmoid dx = g y (1 - y) from the stored OUTPUT y (three fp32 roundings: 1 - y, and two products); ReLU dx = g [y > 0] (exact);
    GELU dx = g gelu'(x) from the stored PRE-activation x (the dGELU term of gemm_ref).  Slack SLACK_ACT."""
    g, v = dy.double(), y.double()
    if act == ACT_SIGMOID:
        r = g * v * (1.0 - v)
        e = 3 * U_FP32 * r.abs()
    elif act == ACT_RELU:
        r = g * (v > 0).double()
        e = torch.zeros_like(r)
    elif act == ACT_GELU:
        r = g * dgelu64(v)
        e = (16 * U_FP32 if dtype == torch.float32 else DGELU_POLY_ERR + 16 * U_FP32) * g.abs()
    else:
        raise ValueError(act)
    return r, SLACK_ACT * (u_of(dtype) * r.abs() + e)


def colsum_depth(M):
    """the longest chain of fp32 additions one addend of devias_colsum goes through (the tree is in the module docstring)"""
    nparts = -(-M // 256)
    return 32 + 8 + -(-nparts // 16) + 16 + 8


def colsum_ref(x, beta=0.0, out_old=None):
    """out[n] = beta out_old[n] + sum_m x[m, n], fp32 sums of the (exactly widened) inputs"""
    x = x.double()
    ref, s_abs = x.sum(0), x.abs().sum(0)
    if beta != 0.0:
        ref, s_abs = ref + beta * out_old.double(), s_abs + (beta * out_old.double()).abs()
    return ref, colsum_depth(x.shape[0]) * U_FP32 * s_abs


def rows_reduce_mod_ref(x, mod):
    """out[r, n] = sum over the rows m = r (mod `mod`): one sequential fp32 chain of M / mod additions per output"""
    M, N = x.shape
    x = x.double().reshape(M // mod, mod, N)
    return x.sum(0), (M // mod + 1) * U_FP32 * x.abs().sum(0)
