// Downstream fine-tuning (docs/DOWNSTREAM.md; model/modeling_slot_fusion.py:23-53, 364-403): everything after the slots of the slot-fusion classifier as ONE
// C-ABI call per direction, and the label-smoothing cross-entropy it trains with.
//
//   devias_fusion_head_fwd   Z = head(slots) -> slot selection -> gather + action_norm / scene_norm -> fc_action_down on 2B rows -> middle chain
//                            (two half-row LayerNorms with fc_action_ln, concat, fc_input_ln, ReLU, dropout mask) -> classifier
//   devias_fusion_head_bwd   the mirror; the gather's backward writes EVERY row of dslots (zero for an unselected slot, the sum where both picks are one slot)
//   devias_softmax_ce_fwd / _bwd   timm's LabelSmoothingCrossEntropy(eps) (eps = 0: plain cross-entropy), one workgroup per row
//
// What the chain is bound by: B workgroups (12 in the recipe) on 256 CUs and two dozen dependent launches -- the number of launches and the host that issues them,
// not bandwidth or arithmetic (a [12, 768] row set is 18 KB).  So the new kernels are one workgroup per row with strided scalar loads (D / 256 <= 4 elements per lane, all in
// registers, no scratch), every statistic a two-pass fp32 block reduction (row_kernels.h: the block reductions and the row LayerNorm's pieces, shared with loss.hip
// and token_head.hip), and the GEMMs / weight gradients / column sums go through the library's small-M launchers as csrc/regions.hip does (region_host.h: those calls,
// the arena carver, the entry points' checks and dtype dispatch).  No atomics: the per-clip partial sums of the four LayerNorm parameter pairs are reduced
// over the clips in index order by one launch (devias_flush_deferred), so results are bitwise equal run to run.
//
// The pre-trained head only selects: Z is not differentiated (head.weight / head.bias get no gradient), fc_scene_down / fc_scene_ln are never read (the reference
// sends BOTH tokens through fc_action_down / fc_action_ln, :43-44), and there is no fc-dropout on the head's input.
#include "common.h"
#include <string.h>
#include "roctx_shim.h"
#include "region_host.h"      // split policies, GEMM / weight-gradient calls, the arena carver, argument checks, dispatch_t
#include "row_kernels.h"       // NT, EPT, block reductions, the row LayerNorm's statistics and backward means, row_stats

namespace {

// ---- gather + action_norm / scene_norm (modeling_slot_fusion.py:391-395) ---------------------------------------------------------------
// row 2b + t of `input` viewed [2B, D] (t = 0: action, 1: scene) = LN(X[b, idx[b, t]]; norm_t).  Statistics two-pass in fp32 (rows with a common offset).
template <typename T>
__global__ __launch_bounds__(NT) void fusion_gather_ln_fwd_kernel(const T* __restrict__ X, const int* __restrict__ idx, int S, int D, float eps,
                                                                  const float* __restrict__ aw, const float* __restrict__ ab, const float* __restrict__ sw,
                                                                  const float* __restrict__ sb, T* __restrict__ input, float* __restrict__ stat /*[2B,2]*/) {
    __shared__ float sm[4];
    const int row = blockIdx.x, b = row >> 1, t = row & 1;
    int s = idx[row];
    s = s < 0 ? 0 : (s >= S ? S - 1 : s);                      // (the selection kernel writes [0, S) only; a foreign index is still never an address out of the clip)
    const T* x = X + ((int64_t)b * S + s) * D;
    const float* gw = t ? sw : aw;
    const float* gb = t ? sb : ab;
    float v[EPT], mean, rstd;
#pragma unroll
    for (int i = 0; i < EPT; ++i) { const int k = threadIdx.x + NT * i; v[i] = k < D ? to_f32(x[k]) : 0.f; }
    row_ln_stats(v, D, eps, sm, mean, rstd);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < D) input[(int64_t)row * D + k] = from_f32<T>((v[i] - mean) * rstd * gw[k] + gb[k]);
    }
    if (threadIdx.x == 0) { stat[2 * row] = mean; stat[2 * row + 1] = rstd; }
}

// ---- gather backward: one workgroup per (clip, slot), every row of dslots written ----------------------------------------------------------
// dX[b, s] = [s = ia] LN'(g_a) + [s = is] LN'(g_s) (summed in fp32, rounded once).  The workgroup of the picked slot writes clip b's partial sums of the norm's
// parameter gradients: part[(2 t) B + b][D] = d weight, part[(2 t + 1) B + b][D] = d bias.
template <typename T>
__global__ __launch_bounds__(NT) void fusion_gather_ln_bwd_kernel(const T* __restrict__ X, const int* __restrict__ idx, const T* __restrict__ dinp /*[2B,D]*/,
                                                                  const float* __restrict__ stat, int B, int S, int D, const float* __restrict__ aw,
                                                                  const float* __restrict__ sw, T* __restrict__ dslots, float* __restrict__ part) {
    __shared__ float sm[8];
    const int b = blockIdx.x / S, s = blockIdx.x % S;
    const T* x = X + (int64_t)blockIdx.x * D;
    float acc[EPT] = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < 2; ++t) {
        int pick = idx[2 * b + t];
        pick = pick < 0 ? 0 : (pick >= S ? S - 1 : pick);      // the forward's clamp: a foreign index selects the row the forward read
        if (pick != s) continue;                                // uniform over the workgroup
        const int row = 2 * b + t;
        const float mean = stat[2 * row], rstd = stat[2 * row + 1];
        const float* gw = t ? sw : aw;
        float* pw = part + ((int64_t)(2 * t) * B + b) * D;
        float* pb = part + ((int64_t)(2 * t + 1) * B + b) * D;
        float xh[EPT], gy[EPT], c1 = 0.f, c2 = 0.f;
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int k = threadIdx.x + NT * i;
            xh[i] = 0.f; gy[i] = 0.f;
            if (k < D) {
                const float g = to_f32(dinp[(int64_t)row * D + k]);
                xh[i] = (to_f32(x[k]) - mean) * rstd;
                pw[k] = g * xh[i]; pb[k] = g;
                gy[i] = g * gw[k];
                c1 += gy[i]; c2 += gy[i] * xh[i];
            }
        }
        row_ln_bwd_means(c1, c2, D, sm);
#pragma unroll
        for (int i = 0; i < EPT; ++i) acc[i] += row_ln_dx(gy[i], xh[i], rstd, c1, c2);
    }
#pragma unroll
    for (int i = 0; i < EPT; ++i) { const int k = threadIdx.x + NT * i; if (k < D) dslots[(int64_t)blockIdx.x * D + k] = from_f32<T>(acc[i]); }
}

// ---- the middle chain (MLPHead.forward :43-51 after the down projection) ----------------------------------------------------------------
// u [B, D] = [fc_action_down(a) | fc_action_down(s)] -> h = [LN(u[:D/2]) | LN(u[D/2:])] (both fc_action_ln) -> LN(h; fc_input_ln) if IN_LN -> ReLU -> * mask -> r.
// Nothing between u and r is rounded to T.  stat[b] = {mean0, rstd0, mean1, rstd1, mean_in, rstd_in}.
template <typename T, bool IN_LN>
__global__ __launch_bounds__(NT) void fusion_mid_fwd_kernel(const T* __restrict__ u, int D, float eps, const float* __restrict__ lw, const float* __restrict__ lb,
                                                            const float* __restrict__ iw, const float* __restrict__ ib, const float* __restrict__ mask,
                                                            T* __restrict__ r, float* __restrict__ stat) {
    __shared__ float sm[8];
    const int b = blockIdx.x, Dh = D >> 1;
    // (the statistics of the two half rows stay written out: they share each pair of barriers through block_sum2, which row_ln_stats would need a flag for)
    float v[EPT], q0 = 0.f, q1 = 0.f;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        v[i] = k < D ? to_f32(u[(int64_t)b * D + k]) : 0.f;
        if (k < Dh) q0 += v[i]; else q1 += v[i];
    }
    block_sum2(q0, q1, sm);
    const float m0 = q0 / (float)Dh, m1 = q1 / (float)Dh;
    q0 = q1 = 0.f;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < Dh) { const float d = v[i] - m0; q0 += d * d; } else if (k < D) { const float d = v[i] - m1; q1 += d * d; }
    }
    block_sum2(q0, q1, sm);
    const float r0 = rsqrtf(q0 / (float)Dh + eps), r1 = rsqrtf(q1 / (float)Dh + eps);
    float h[EPT];
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        h[i] = 0.f;
        if (k < D) { const int j = k < Dh ? k : k - Dh; h[i] = (v[i] - (k < Dh ? m0 : m1)) * (k < Dh ? r0 : r1) * lw[j] + lb[j]; }
    }
    float mi = 0.f, ri = 1.f;
    if constexpr (IN_LN) row_ln_stats(h, D, eps, sm, mi, ri);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < D) {
            float y = h[i];
            if constexpr (IN_LN) y = (y - mi) * ri * iw[k] + ib[k];
            y = fmaxf(y, 0.f);
            if (mask) y *= mask[(int64_t)b * D + k];
            r[(int64_t)b * D + k] = from_f32<T>(y);
        }
    }
    if (threadIdx.x == 0) { float* o = stat + 6 * b; o[0] = m0; o[1] = r0; o[2] = m1; o[3] = r1; o[4] = mi; o[5] = ri; }
}

// backward of the middle chain on the saved forward: the ReLU mask is r > 0 (the stored r), the normalised values are recomputed from the stored u and statistics.
// Partials of clip b: p_in[b][0:D] = d fc_input_ln.weight, p_in[b][D:2D] = d bias; p_lw / p_lb [2b + half][D/2] = d fc_action_ln.weight / bias of each half.
template <typename T, bool IN_LN>
__global__ __launch_bounds__(NT) void fusion_mid_bwd_kernel(const T* __restrict__ dr, const T* __restrict__ r, const T* __restrict__ u, const float* __restrict__ stat,
                                                            int D, const float* __restrict__ lw, const float* __restrict__ lb, const float* __restrict__ iw,
                                                            const float* __restrict__ mask, T* __restrict__ du, float* __restrict__ p_in,
                                                            float* __restrict__ p_lw, float* __restrict__ p_lb) {
    __shared__ float sm[8];
    const int b = blockIdx.x, Dh = D >> 1;
    const float* st = stat + 6 * b;
    const float m0 = st[0], r0 = st[1], m1 = st[2], r1 = st[3], mi = st[4], ri = st[5];
    float g[EPT], xh[EPT], c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        g[i] = 0.f; xh[i] = 0.f;
        if (k < D) {
            const int64_t e = (int64_t)b * D + k;
            float gg = to_f32(r[e]) > 0.f ? to_f32(dr[e]) : 0.f;
            if (mask) gg *= mask[e];
            xh[i] = (to_f32(u[e]) - (k < Dh ? m0 : m1)) * (k < Dh ? r0 : r1);
            if constexpr (IN_LN) {
                const int j = k < Dh ? k : k - Dh;
                const float xin = (xh[i] * lw[j] + lb[j] - mi) * ri;
                p_in[(int64_t)b * 2 * D + k] = gg * xin;
                p_in[(int64_t)b * 2 * D + D + k] = gg;
                gg *= iw[k];
                c1 += gg; c2 += gg * xin;
                g[i] = gg;
                xh[i] = xin;          // (held in xh until the input LayerNorm's backward is done; recomputed below)
            } else {
                g[i] = gg;
            }
        }
    }
    if constexpr (IN_LN) {
        row_ln_bwd_means(c1, c2, D, sm);
#pragma unroll
        for (int i = 0; i < EPT; ++i) {
            const int k = threadIdx.x + NT * i;
            if (k < D) {
                g[i] = row_ln_dx(g[i], xh[i], ri, c1, c2);
                xh[i] = (to_f32(u[(int64_t)b * D + k]) - (k < Dh ? m0 : m1)) * (k < Dh ? r0 : r1);
            }
        }
    }
    // the two half-row LayerNorms (one parameter pair, two rows): written out, their four means take two block_sum2 where row_ln_bwd_means would take a half-row flag
    float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < D) {
            const int j = k < Dh ? k : k - Dh;
            p_lw[(int64_t)b * D + k] = g[i] * xh[i];            // [2b + half][j]
            p_lb[(int64_t)b * D + k] = g[i];
            g[i] *= lw[j];
            if (k < Dh) { a0 += g[i]; b0 += g[i] * xh[i]; } else { a1 += g[i]; b1 += g[i] * xh[i]; }
        }
    }
    block_sum2(a0, b0, sm);
    block_sum2(a1, b1, sm);
    a0 /= (float)Dh; b0 /= (float)Dh; a1 /= (float)Dh; b1 /= (float)Dh;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < D) du[(int64_t)b * D + k] = from_f32<T>(k < Dh ? r0 * (g[i] - a0 - xh[i] * b0) : r1 * (g[i] - a1 - xh[i] * b1));
    }
}

// ---- label-smoothing cross-entropy (timm.loss.LabelSmoothingCrossEntropy) -------------------------------------------------------------------
// row b: (1 - eps) (lse - z_y) + eps (lse - mean_c z_c); a target outside [0, C) is never an index: that row is NaN (the labels_ok convention of loss.hip)
template <typename T>
__global__ __launch_bounds__(NT) void softmax_ce_fwd_kernel(const T* __restrict__ Z, const int64_t* __restrict__ target, int C, float eps, float* __restrict__ per_row) {
    __shared__ float sm[4];
    const int b = blockIdx.x;
    const T* z = Z + (int64_t)b * C;
    float m = -INFINITY;
    for (int c = threadIdx.x; c < C; c += NT) m = fmaxf(m, to_f32(z[c]));
    const float mx = block_max(m, sm);
    float s = 0.f, t = 0.f;
    for (int c = threadIdx.x; c < C; c += NT) { const float v = to_f32(z[c]); s += expf(v - mx); t += v - mx; }
    const float lse = logf(block_sum(s, sm));                 // relative to mx
    const float zm = block_sum(t, sm) / (float)C;             // mean_c (z_c - mx)
    if (threadIdx.x == 0) {
        const int64_t y = target[b];
        per_row[b] = (y >= 0 && y < C) ? (1.f - eps) * (lse - (to_f32(z[y]) - mx)) + eps * (lse - zm) : __builtin_nanf("");
    }
}
__global__ void softmax_ce_final_kernel(const float* __restrict__ per_row, int B, float* __restrict__ loss) {
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += per_row[b];
        loss[0] = s / (float)B;
    }
}
// dz = g / B (p_c - (1 - eps) [c = y] - eps / C); a row whose target is out of range gets zeros
template <typename T>
__global__ __launch_bounds__(NT) void softmax_ce_bwd_kernel(const T* __restrict__ Z, const int64_t* __restrict__ target, int B, int C, float eps,
                                                            const float* __restrict__ g_loss, T* __restrict__ dZ) {
    __shared__ float sm[4];
    const int b = blockIdx.x;
    const T* z = Z + (int64_t)b * C;
    T* dz = dZ + (int64_t)b * C;
    const int64_t y = target[b];
    if (y < 0 || y >= C) {
        for (int c = threadIdx.x; c < C; c += NT) dz[c] = from_f32<T>(0.f);
        return;
    }
    float mx, lse;
    row_stats(z, C, sm, mx, lse);
    const float g = g_loss[0] / (float)B, off = eps / (float)C;
    for (int c = threadIdx.x; c < C; c += NT)
        dz[c] = from_f32<T>(g * (expf(to_f32(z[c]) - lse) - (c == (int)y ? 1.f - eps : 0.f) - off));
}

// ---- host side (GEMM / weight-gradient helpers and split policies: region_host.h, shared with regions.hip) ---------------------------------------------
int gemm_b(const Ctx& c, const void* A, const void* Bm, void* C, int M, int N, int K, int lda, int ldb, int trans_b, const float* bias, const void* res) {
    Epi e; e.bias = bias; e.res = res;
    return gemm(c, A, Bm, C, M, N, K, lda, ldb, 0, trans_b, e);
}

inline bool dims_supported(int B, int S, int D, int nb, int ns, int Cd) {
    return B >= 1 && (int64_t)B * 4 * 1024 < 0x7fffffff && S >= 1 && S <= 4 && row_dim_ok(D) && nb >= 1 && ns >= 1 && Cd >= 2;
}
int64_t kernel_ws_bytes(int B, int S, int D, int C, int Cd, int dtype) {
    const int R = B * S, Dh = D / 2;
    int64_t w = max64(gemm_ws(R, C, D, 0), max64(gemm_ws(2 * B, Dh, D, 0), gemm_ws(B, Cd, D, 0)));
    w = max64(w, max64(gemm_ws(B, D, Cd, 0), gemm_ws(2 * B, D, Dh, 0)));
    w = max64(w, max64(wgrad_ws(Cd, D, B, dtype), wgrad_ws(Dh, D, 2 * B, dtype)));
    w = max64(w, max64(devias_colsum_workspace_bytes(B, Cd), devias_colsum_workspace_bytes(2 * B, Dh)));
    return al256(w) + 256;
}
// what backward reads of the forward: the middle chain's input and output, the statistics of the gather's and the middle chain's LayerNorms
struct Save {
    char *u, *r; float *stat_g, *stat_m;
    Save(Arena& ar, int B, int D, int dtype) {
        const int64_t es = esize(dtype);
        u = ar.take((int64_t)B * D * es); r = ar.take((int64_t)B * D * es);
        stat_g = (float*)ar.take((int64_t)B * 4 * 4); stat_m = (float*)ar.take((int64_t)B * 6 * 4);
    }
};
// what lives behind the kernels' workspace: Z; a Save of its own, which the forward writes where the caller keeps none; the backward's temporaries and partial sums
struct Tmp {
    char* Z; Save s;          // (carved in this order)
    char *dr, *du, *dinp;
    float *p_in, *p_lw, *p_lb, *p_n;
    int64_t bytes;
    Tmp(Arena ar, int B, int S, int D, int C, int dtype) : Z(ar.take((int64_t)B * S * C * esize(dtype))), s(ar, B, D, dtype) {
        const int64_t es = esize(dtype);
        dr = ar.take((int64_t)B * D * es); du = ar.take((int64_t)B * D * es); dinp = ar.take((int64_t)2 * B * D * es);
        p_in = (float*)ar.take((int64_t)B * 2 * D * 4); p_lw = (float*)ar.take((int64_t)B * D * 4); p_lb = (float*)ar.take((int64_t)B * D * 4);
        p_n = (float*)ar.take((int64_t)4 * B * D * 4);
        bytes = ar.off;
    }
};

int fusion_check(const devias_fusion_args* a, const char* who) {
    DEVIAS_REQUIRE(a, "%s: null args", who);
    REQUIRE_STRUCT_SIZE(a, devias_fusion_args, who);
    DEVIAS_REQUIRE(dtype_ok(a->dtype), "%s: bad dtype %d", who, a->dtype);
    if (!dims_supported(a->B, a->S, a->D, a->nb, a->ns, a->Cd))
        return devias_set_error(DEVIAS_EUNSUPPORTED, "%s: unsupported dims B=%d S=%d D=%d nb=%d ns=%d Cd=%d (D in {384, 768, 1024}, 1 <= S <= 4, Cd >= 2, B >= 1, nb, ns >= 1)", who,
                                a->B, a->S, a->D, a->nb, a->ns, a->Cd);
    DEVIAS_REQUIRE(a->eps_norm > 0.f && a->eps_ln > 0.f, "%s: eps_norm / eps_ln must be positive", who);
    DEVIAS_REQUIRE(a->Wh && a->bh && a->an_w && a->an_b && a->sn_w && a->sn_b && a->Wd && a->bd && a->ln_w && a->ln_b && a->Wc && a->bc, "%s: null parameter", who);
    DEVIAS_REQUIRE(!a->use_input_ln || (a->in_w && a->in_b), "%s: use_input_ln needs fc_input_ln's weight and bias", who);
    DEVIAS_REQUIRE(a->ws && aligned16(a->ws), "%s: ws must be 16-byte aligned, non-null", who);
    DEVIAS_REQUIRE(a->ws_bytes >= devias_fusion_head_workspace_bytes(a->B, a->S, a->D, a->nb + a->ns, a->Cd, a->dtype), "%s: workspace too small", who);
    return DEVIAS_OK;
}

}  // namespace

extern "C" int64_t devias_fusion_head_workspace_bytes(int32_t B, int32_t S, int32_t D, int32_t C, int32_t Cd, int32_t dtype) {
    if (!dims_supported(B, S, D, 1, C > 1 ? C - 1 : 0, Cd) || !dtype_ok(dtype)) return 0;
    return kernel_ws_bytes(B, S, D, C, Cd, dtype) + Tmp(Arena(nullptr), B, S, D, C, dtype).bytes;
}
extern "C" int64_t devias_fusion_head_save_bytes(int32_t B, int32_t D, int32_t dtype) {
    if (B < 1 || !row_dim_ok(D) || !dtype_ok(dtype)) return 0;
    Arena ar(nullptr);
    Save(ar, B, D, dtype);          // (carved at address 0: the arena ends at its size)
    return ar.off;
}

extern "C" int devias_fusion_head_fwd(const devias_fusion_args* a, const void* slots, void* input, void* out, int32_t* idx, void* save, void* stream) {
    const char* who = "devias_fusion_head_fwd";
    RUN(fusion_check(a, who));
    DEVIAS_REQUIRE(slots && input && out && idx && aligned16(slots) && aligned16(input) && aligned16(out), "%s: slots / input / out / idx must be non-null (16-byte aligned tensors)", who);
    DEVIAS_REQUIRE(!save || aligned16(save), "%s: save must be 16-byte aligned", who);
    const int B = a->B, S = a->S, D = a->D, Dh = D / 2, C = a->nb + a->ns, Cd = a->Cd, R = B * S;
    hipStream_t st = (hipStream_t)stream;
    const int64_t kw = kernel_ws_bytes(B, S, D, C, Cd, a->dtype);
    const Ctx c{a->dtype, a->ws, kw, nullptr, 0, stream};
    const Tmp t(Arena(reinterpret_cast<char*>(a->ws) + kw), B, S, D, C, a->dtype);
    Arena own(save);
    const Save s = save ? Save(own, B, D, a->dtype) : t.s;          // the caller's arena, or (nothing to keep) the one in the workspace
    devias_range rg("fusion_head_fwd");
    devias_count_region(DEVIAS_RCNT_FUSION_HEAD);
    RUN(gemm_b(c, slots, a->Wh, t.Z, R, C, D, D, D, 0, a->bh, nullptr));                       // the frozen head: selection only
    RUN(devias_slot_select(t.Z, a->dtype, B, S, C, a->nb, idx, stream));
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((fusion_gather_ln_fwd_kernel<T>), dim3(2 * B), dim3(NT), 0, st, (const T*)slots, idx, S, D, a->eps_norm, a->an_w, a->an_b, a->sn_w, a->sn_b, (T*)input, s.stat_g);
    });
    DEVIAS_CHECK_LAUNCH("devias_fusion_head_fwd(gather)");
    RUN(gemm_b(c, input, a->Wd, s.u, 2 * B, Dh, D, D, D, 0, a->bd, nullptr));                  // fc_action_down on both tokens: [2B, D/2] == [B, D]
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((a->use_input_ln ? fusion_mid_fwd_kernel<T, true> : fusion_mid_fwd_kernel<T, false>), dim3(B), dim3(NT), 0, st, (const T*)s.u, D, a->eps_ln, a->ln_w,
                           a->ln_b, a->in_w, a->in_b, a->drop_mask, (T*)s.r, s.stat_m);
    });
    DEVIAS_CHECK_LAUNCH("devias_fusion_head_fwd(middle)");
    RUN(gemm_b(c, s.r, a->Wc, out, B, Cd, D, D, D, 0, a->bc, nullptr));
    return DEVIAS_OK;
}

extern "C" int devias_fusion_head_bwd(const devias_fusion_args* a, const void* slots, const int32_t* idx, const void* input, const void* save, const void* dout,
                                      const void* dinput, void* dslots, const devias_fusion_grads* g, void* stream) {
    const char* who = "devias_fusion_head_bwd";
    RUN(fusion_check(a, who));
    DEVIAS_REQUIRE(slots && idx && input && save && dout && dslots && g && aligned16(save), "%s: null pointer (slots / idx / input / save / dout / dslots / grads)", who);
    REQUIRE_STRUCT_SIZE(g, devias_fusion_grads, who);
    DEVIAS_REQUIRE(g->dan_w && g->dan_b && g->dsn_w && g->dsn_b && g->dWd && g->dbd && g->dln_w && g->dln_b && g->dWc && g->dbc && (!a->use_input_ln || (g->din_w && g->din_b)),
                   "%s: null gradient destination", who);
    const int B = a->B, S = a->S, D = a->D, Dh = D / 2, C = a->nb + a->ns, Cd = a->Cd;
    hipStream_t st = (hipStream_t)stream;
    const int64_t kw = kernel_ws_bytes(B, S, D, C, Cd, a->dtype);
    const Ctx c{a->dtype, a->ws, kw, nullptr, 0, stream};
    const Tmp t(Arena(reinterpret_cast<char*>(a->ws) + kw), B, S, D, C, a->dtype);
    Arena own(save);
    const Save s(own, B, D, a->dtype);
    devias_range rg("fusion_head_bwd");
    devias_count_region(DEVIAS_RCNT_FUSION_HEAD);
    // classifier
    RUN(wgrad(c, dout, s.r, g->dWc, B, Cd, D));
    RUN(colsum(c, dout, B, Cd, g->dbc));
    RUN(gemm_b(c, dout, a->Wc, t.dr, B, D, Cd, Cd, D, 1, nullptr, nullptr));
    // middle chain
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((a->use_input_ln ? fusion_mid_bwd_kernel<T, true> : fusion_mid_bwd_kernel<T, false>), dim3(B), dim3(NT), 0, st, (const T*)t.dr, (const T*)s.r,
                           (const T*)s.u, s.stat_m, D, a->ln_w, a->ln_b, a->in_w, a->drop_mask, (T*)t.du, t.p_in, t.p_lw, t.p_lb);
    });
    DEVIAS_CHECK_LAUNCH("devias_fusion_head_bwd(middle)");
    // down projection on the 2B rows
    RUN(wgrad(c, t.du, input, g->dWd, 2 * B, Dh, D));
    RUN(colsum(c, t.du, 2 * B, Dh, g->dbd));
    RUN(gemm_b(c, t.du, a->Wd, t.dinp, 2 * B, D, Dh, Dh, D, 1, nullptr, dinput));              // + the gradient arriving on the returned `input`, if any
    // scatter through the two norms into the selected slot rows
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((fusion_gather_ln_bwd_kernel<T>), dim3(B * S), dim3(NT), 0, st, (const T*)slots, idx, (const T*)t.dinp, s.stat_g, B, S, D, a->an_w, a->sn_w, (T*)dslots, t.p_n);
    });
    DEVIAS_CHECK_LAUNCH("devias_fusion_head_bwd(gather)");
    // the four LayerNorm parameter pairs: per-clip partials summed over the clips in index order, ONE launch
    DeviasDeferList dl; dl.n = 0;
    auto job = [&](const float* part, int nparts, int n, float* out) { dl.jobs[dl.n++] = DeviasReduceJob{part, nparts, n, n, out, 0.f}; };
    const int64_t BD = (int64_t)B * D;
    job(t.p_n, B, D, g->dan_w); job(t.p_n + BD, B, D, g->dan_b); job(t.p_n + 2 * BD, B, D, g->dsn_w); job(t.p_n + 3 * BD, B, D, g->dsn_b);
    job(t.p_lw, 2 * B, Dh, g->dln_w); job(t.p_lb, 2 * B, Dh, g->dln_b);
    if (a->use_input_ln) {
        dl.jobs[dl.n++] = DeviasReduceJob{t.p_in, B, 2 * D, D, g->din_w, 0.f};
        dl.jobs[dl.n++] = DeviasReduceJob{t.p_in + D, B, 2 * D, D, g->din_b, 0.f};
    }
    RUN(devias_flush_deferred(&dl, st));
    return DEVIAS_OK;
}

// ---- cross-entropy entry points -----------------------------------------------------------------------------------------------------------------
namespace {
int ce_check(const char* who, const void* logits, const int64_t* target, int B, int C, int dtype, float eps) {
    DEVIAS_REQUIRE(logits && target, "%s: null logits / target", who);
    DEVIAS_REQUIRE(dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    DEVIAS_REQUIRE(B >= 1 && C >= 2, "%s: bad dims B=%d C=%d (B >= 1, C >= 2)", who, B, C);
    DEVIAS_REQUIRE(eps >= 0.f && eps < 1.f, "%s: smoothing must be in [0, 1), got %g", who, (double)eps);
    return DEVIAS_OK;
}
}  // namespace

extern "C" int64_t devias_softmax_ce_workspace_bytes(int32_t B) { return B >= 1 ? (int64_t)B * 4 : 0; }

extern "C" int devias_softmax_ce_fwd(const void* logits, const int64_t* target, int32_t B, int32_t C, int32_t dtype, float smoothing, float* loss, float* ws, void* stream) {
    const char* who = "devias_softmax_ce_fwd";
    RUN(ce_check(who, logits, target, B, C, dtype, smoothing));
    DEVIAS_REQUIRE(loss && ws, "%s: null loss / ws", who);
    hipStream_t st = (hipStream_t)stream;
    devias_count_region(DEVIAS_RCNT_SOFTMAX_CE);
    dispatch_t(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((softmax_ce_fwd_kernel<T>), dim3(B), dim3(NT), 0, st, (const T*)logits, target, C, smoothing, ws);
    });
    DEVIAS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(softmax_ce_final_kernel, dim3(1), dim3(64), 0, st, ws, B, loss);
    DEVIAS_CHECK_LAUNCH("devias_softmax_ce_fwd(final)");
    return DEVIAS_OK;
}

extern "C" int devias_softmax_ce_bwd(const void* logits, const int64_t* target, int32_t B, int32_t C, int32_t dtype, float smoothing, const float* g_loss, void* dlogits,
                                     void* stream) {
    const char* who = "devias_softmax_ce_bwd";
    RUN(ce_check(who, logits, target, B, C, dtype, smoothing));
    DEVIAS_REQUIRE(g_loss && dlogits, "%s: null g_loss / dlogits", who);
    hipStream_t st = (hipStream_t)stream;
    devias_count_region(DEVIAS_RCNT_SOFTMAX_CE);
    dispatch_t(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((softmax_ce_bwd_kernel<T>), dim3(B), dim3(NT), 0, st, (const T*)logits, target, B, C, smoothing, g_loss, (T*)dlogits);
    });
    DEVIAS_CHECK_LAUNCH(who);
    return DEVIAS_OK;
}
