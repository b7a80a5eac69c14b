// The two-token multi-task baseline's part after the encoder (model/modeling_multi_task.py: norm(x)[:, 0] and norm(x)[:, -1], fc_dropout on each, head / scene_head)
// as ONE C-ABI call per direction, and the scene head's distillation loss (run_multi_task_finetuning.py: TrainLoss).
//
//   devias_two_token_head_fwd   h [B*Nt, D] -> rows 0 and Nt-1 of each clip -> LayerNorm (norm, shared) -> token_a, token_s [B, D];
//                               a = token's unrounded value * its own mask; logits_a = a_a Wa^T + ba, logits_s = a_s Ws^T + bs (unified: ONE GEMM over the 2B stacked rows)
//   devias_two_token_head_bwd   dlogits_a, dlogits_s (+ dtoken_a, dtoken_s) -> dW / db per head (unified: one pair over the 2B rows), d gamma, d beta, and EVERY row of
//                               dx [B*Nt, D] (the LayerNorm's input gradient in rows 0 and Nt-1 of each clip, zeros elsewhere)
//   devias_distill_fwd / _bwd   KL(teacher || student) on the (left-padded) teacher logits, or cross-entropy against the teacher's argmax; one workgroup per row
//
// The 2B rows are worked on STACKED: row j < B is the action token of clip j, row B + j the scene token of clip j.  Everything between the two token rows and dx is
// [2B, D] or [2B, C]: one-workgroup-per-row kernels from row_kernels.h (as pool_head.hip's) and the library's GEMM / weight-gradient / column-sum launchers
// (region_host.h).  The forward reads 2B rows of h, not B*Nt; the backward writes dx once with 16-byte stores (pool_head.hip's pool_dx_kernel, two live rows per clip).
//
// No atomics: d gamma / d beta are per-row partials summed over the 2B rows in index order by one devias_flush_deferred launch.
// Roundings to T: token, a, logits, dx -- each once, from fp32.  da (the heads' input gradient) stays fp32 (GEMM with an fp32 output).
#include "common.h"
#include <string.h>
#include <atomic>
#include "roctx_shim.h"
#include "region_host.h"
#include "row_kernels.h"

static std::atomic<int64_t> g_two_token_head_calls;
void devias_two_token_head_counter_reset() { g_two_token_head_calls.store(0, std::memory_order_relaxed); }      // api.hip: devias_counters_reset
extern "C" int64_t devias_two_token_head_launches(void) { return g_two_token_head_calls.load(std::memory_order_relaxed); }

namespace {

enum { TOK = DEVIAS_POOL_HEAD_CHUNK, NTS = 384 };      // the dx kernel: token rows per workgroup, most threads

template <typename T> struct Vec16;
template <> struct Vec16<bf16> { typedef bf16x8 type; enum { N = 8 }; };
template <> struct Vec16<float> { typedef f32x4 type; enum { N = 4 }; };

inline int stream_rows(int D, int dtype) { const int vc = D / (dtype == DEVIAS_BF16 ? 8 : 4); return NTS / vc; }

// ---- forward: LayerNorm of the 2B token rows, mask -------------------------------------------------------------------------------------------------
// stacked row j: clip b = j mod B, token row 0 (j < B) or Nt - 1.  token = T(y), a = T(y * mask) with y = x^ gamma + beta in fp32: the mask meets the UNROUNDED y.
// Saved: x^ fp32 [2B, D], rstd fp32 [2B], a T [2B, D].
template <typename T>
__global__ __launch_bounds__(NT) void tt_ln_fwd_kernel(const T* __restrict__ h, int B, int Nt, int D, float eps, const float* __restrict__ gw, const float* __restrict__ gb,
                                                       const float* __restrict__ mask_a, const float* __restrict__ mask_s, T* __restrict__ token_a, T* __restrict__ token_s,
                                                       T* __restrict__ a, float* __restrict__ xhat, float* __restrict__ rstd_out) {
    __shared__ float sm[8];
    const int j = blockIdx.x, scene = j >= B, b = scene ? j - B : j;
    const T* row = h + ((int64_t)b * Nt + (scene ? Nt - 1 : 0)) * D;
    const float* mask = scene ? mask_s : mask_a;
    T* token = scene ? token_s : token_a;
    float v[EPT], mean, rstd;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        v[i] = k < D ? to_f32(row[k]) : 0.f;
    }
    row_ln_stats(v, D, eps, sm, mean, rstd);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < D) {
            const int64_t e = (int64_t)b * D + k, e2 = (int64_t)j * D + k;
            const float xh = (v[i] - mean) * rstd;
            const float y = xh * gw[k] + gb[k];
            xhat[e2] = xh;
            token[e] = from_f32<T>(y);
            a[e2] = from_f32<T>(mask ? y * mask[e] : y);
        }
    }
    if (threadIdx.x == 0) rstd_out[j] = rstd;
}

// ---- backward: LayerNorm backward per stacked row --------------------------------------------------------------------------------------------------------
// g = da * mask + dtoken (fp32); pg[j] = g x^, pb[j] = g; dxrow[j] = T(rstd (g gamma - mean(g gamma) - x^ mean(g gamma x^)))
template <typename T>
__global__ __launch_bounds__(NT) void tt_ln_bwd_kernel(const float* __restrict__ da, const T* __restrict__ dtoken_a, const T* __restrict__ dtoken_s,
                                                       const float* __restrict__ mask_a, const float* __restrict__ mask_s, const float* __restrict__ xhat,
                                                       const float* __restrict__ rstd_in, const float* __restrict__ gw, int B, int D, T* __restrict__ dxrow,
                                                       float* __restrict__ pg, float* __restrict__ pb) {
    __shared__ float sm[8];
    const int j = blockIdx.x, scene = j >= B, b = scene ? j - B : j;
    const float* mask = scene ? mask_s : mask_a;
    const T* dtoken = scene ? dtoken_s : dtoken_a;
    const float rstd = rstd_in[j];
    float xh[EPT], gy[EPT], c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        xh[i] = 0.f; gy[i] = 0.f;
        if (k < D) {
            const int64_t e = (int64_t)b * D + k, e2 = (int64_t)j * D + k;
            float g = da[e2];
            if (mask) g *= mask[e];
            if (dtoken) g += to_f32(dtoken[e]);
            xh[i] = xhat[e2];
            pg[e2] = g * xh[i]; pb[e2] = g;
            gy[i] = g * gw[k];
            c1 += gy[i]; c2 += gy[i] * xh[i];
        }
    }
    row_ln_bwd_means(c1, c2, D, sm);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < D) dxrow[(int64_t)j * D + k] = from_f32<T>(row_ln_dx(gy[i], xh[i], rstd, c1, c2));
    }
}

// ---- backward: every row of dx -------------------------------------------------------------------------------------------------------------------------
// one workgroup per (clip, chunk of TOK token rows): row 0 takes dxrow[b], row Nt - 1 takes dxrow[B + b], every other row zeros
template <typename T>
__global__ __launch_bounds__(NTS) void tt_dx_kernel(const T* __restrict__ dxrow, int B, int Nt, int D, int chunks, int R, T* __restrict__ dx) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = Vec16<T>::N;
    const int Vc = D / VEC;
    const int c = threadIdx.x % Vc, r = threadIdx.x / Vc;       // blockDim.x == R * Vc exactly
    const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int t0 = ch * TOK, t1 = min(Nt, t0 + TOK);
    V zero;
#pragma unroll
    for (int i = 0; i < VEC; ++i) zero[i] = from_f32<T>(0.f);
    T* base = dx + (int64_t)b * Nt * D + c * VEC;
    for (int t = t0 + r; t < t1; t += R) {
        V val = zero;
        if (t == 0) val = *reinterpret_cast<const V*>(dxrow + (int64_t)b * D + c * VEC);
        else if (t == Nt - 1) val = *reinterpret_cast<const V*>(dxrow + (int64_t)(B + b) * D + c * VEC);
        *reinterpret_cast<V*>(base + (int64_t)t * D) = val;
    }
}

// unified head, backward: the two [B, C] gradients one under the other (the weight gradient and the column sums run over the 2B rows)
template <typename T>
__global__ __launch_bounds__(NT) void tt_stack_kernel(const T* __restrict__ top, const T* __restrict__ bottom, int64_t n, T* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i < n) { out[i] = top[i]; out[n + i] = bottom[i]; }
}

// ---- distillation loss ---------------------------------------------------------------------------------------------------------------------------------------
// the minimum of the whole teacher tensor (a minimum is order-independent): one workgroup
__global__ __launch_bounds__(NT) void distill_min_kernel(const float* __restrict__ t, int64_t n, float* __restrict__ out) {
    __shared__ float sm[4];
    float m = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += NT) m = fmaxf(m, -t[i]);
    m = block_max(m, sm);
    if (threadIdx.x == 0) out[0] = -m;
}

// The teacher's row as the student sees it: `pad` columns of (tmin - 1) on the left, then the Ct teacher logits.
struct TeacherRow {
    const float* t; int pad; float padv;
    __device__ __forceinline__ float at(int c) const { return c < pad ? padv : t[c - pad]; }
};
// first index of the row's maximum over the Ct teacher columns (torch.argmax's tie rule); the pad value is below every teacher logit and never wins
__device__ __forceinline__ int teacher_argmax(const float* t, int Ct, float* sm) {
    float m = -INFINITY;
    for (int c = threadIdx.x; c < Ct; c += NT) m = fmaxf(m, t[c]);
    m = block_max(m, sm);
    float first = -INFINITY;                                     // max of -index over the columns that hold m (indices < 2^24 are exact in fp32)
    for (int c = threadIdx.x; c < Ct; c += NT) if (t[c] == m) first = fmaxf(first, -(float)c);
    first = block_max(first, sm);
    return first == -INFINITY ? 0 : (int)(-first);               // (a row of NaNs: column 0, an address inside the row)
}
template <typename T>
__global__ __launch_bounds__(NT) void distill_fwd_kernel(const T* __restrict__ Z, const float* __restrict__ teacher, const float* __restrict__ tmin, int C, int Ct, int ce,
                                                         float* __restrict__ per_row) {
    __shared__ float sm[4];
    const int b = blockIdx.x, pad = C - Ct;
    const T* z = Z + (int64_t)b * C;
    const float* t = teacher + (int64_t)b * Ct;
    float mx, lse;
    row_stats(z, C, sm, mx, lse);
    if (ce) {
        const int y = pad + teacher_argmax(t, Ct, sm);
        if (threadIdx.x == 0) per_row[b] = lse - to_f32(z[y]);
        return;
    }
    const TeacherRow tr{t, pad, pad > 0 ? tmin[0] - 1.f : 0.f};
    float m = -INFINITY;
    for (int c = threadIdx.x; c < C; c += NT) m = fmaxf(m, tr.at(c));
    const float tmx = block_max(m, sm);
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += NT) s += expf(tr.at(c) - tmx);
    const float tlse = tmx + logf(block_sum(s, sm));
    float kl = 0.f;
    for (int c = threadIdx.x; c < C; c += NT) {
        const float lt = tr.at(c) - tlse;
        kl += expf(lt) * (lt - (to_f32(z[c]) - lse));
    }
    kl = block_sum(kl, sm);
    if (threadIdx.x == 0) per_row[b] = kl;
}
// loss = scale * (sum_b per_row[b]) / B, the rows added in index order
__global__ void distill_final_kernel(const float* __restrict__ per_row, int B, float scale, float* __restrict__ loss) {
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += per_row[b];
        loss[0] = s / (float)B * scale;
    }
}
// KL: dz = g w / B (p_s - p_t); CE: dz = g / B (p_s - onehot)
template <typename T>
__global__ __launch_bounds__(NT) void distill_bwd_kernel(const T* __restrict__ Z, const float* __restrict__ teacher, const float* __restrict__ tmin, int B, int C, int Ct,
                                                         int ce, float scale, const float* __restrict__ g_loss, T* __restrict__ dZ) {
    __shared__ float sm[4];
    const int b = blockIdx.x, pad = C - Ct;
    const T* z = Z + (int64_t)b * C;
    T* dz = dZ + (int64_t)b * C;
    const float* t = teacher + (int64_t)b * Ct;
    float mx, lse;
    row_stats(z, C, sm, mx, lse);
    const float g = g_loss[0] * scale / (float)B;
    if (ce) {
        const int y = pad + teacher_argmax(t, Ct, sm);
        for (int c = threadIdx.x; c < C; c += NT) dz[c] = from_f32<T>(g * (expf(to_f32(z[c]) - lse) - (c == y ? 1.f : 0.f)));
        return;
    }
    const TeacherRow tr{t, pad, pad > 0 ? tmin[0] - 1.f : 0.f};
    float m = -INFINITY;
    for (int c = threadIdx.x; c < C; c += NT) m = fmaxf(m, tr.at(c));
    const float tmx = block_max(m, sm);
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += NT) s += expf(tr.at(c) - tmx);
    const float tlse = tmx + logf(block_sum(s, sm));
    for (int c = threadIdx.x; c < C; c += NT) dz[c] = from_f32<T>(g * (expf(to_f32(z[c]) - lse) - expf(tr.at(c) - tlse)));
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
inline bool dims_supported(int B, int Nt, int D, int Ca, int Cs) {
    return B >= 1 && Nt >= 2 && (int64_t)B * Nt <= 0x7fffffff && row_dim_ok(D) && Ca >= 2 && Cs >= 2 && (int64_t)B * 2 * 1024 < 0x7fffffff;
}
int64_t kernel_ws_bytes(int B, int D, int Ca, int Cs, int unified, int dtype) {
    const int M = unified ? 2 * B : B, C = Ca > Cs ? Ca : Cs;      // (every term grows with C)
    int64_t w = max64(gemm_ws(M, C, D, 0), gemm_ws(M, D, C, 0));
    w = max64(w, max64(wgrad_ws(C, D, M, dtype), devias_colsum_workspace_bytes(M, C)));
    return al256(w) + 256;
}
// what backward reads of the forward: the normalised token rows and their rstd in fp32, the heads' input a -- all stacked [2B, ...]
struct Save {
    float *xhat, *rstd; char* a;
    Save(Arena& ar, int B, int D, int dtype) {
        xhat = (float*)ar.take((int64_t)2 * B * D * 4); rstd = (float*)ar.take((int64_t)2 * B * 4); a = ar.take((int64_t)2 * B * D * esize(dtype));
    }
};
// what lives behind the kernels' workspace: a Save of its own, which the forward writes where the caller keeps none; the backward's temporaries and per-row partials
struct Tmp {
    Save s;
    float *da, *pg, *pb;
    char *dxrow, *dl2;
    int64_t bytes;
    Tmp(Arena ar, int B, int D, int Ca, int Cs, int dtype) : s(ar, B, D, dtype) {
        const int64_t es = esize(dtype), BD = (int64_t)2 * B * D;
        da = (float*)ar.take(BD * 4); dxrow = ar.take(BD * es); pg = (float*)ar.take(BD * 4); pb = (float*)ar.take(BD * 4);
        dl2 = ar.take((int64_t)2 * B * (Ca > Cs ? Ca : Cs) * es);
        bytes = ar.off;
    }
};

int tt_check(const devias_two_token_head_args* a, const char* who) {
    DEVIAS_REQUIRE(a, "%s: null args", who);
    REQUIRE_STRUCT_SIZE(a, devias_two_token_head_args, who);
    DEVIAS_REQUIRE(dtype_ok(a->dtype), "%s: bad dtype %d", who, a->dtype);
    DEVIAS_REQUIRE(a->unified == 0 || a->unified == 1, "%s: unified must be 0 or 1, got %d", who, a->unified);
    if (!dims_supported(a->B, a->Nt, a->D, a->Ca, a->Cs))
        return devias_set_error(DEVIAS_EUNSUPPORTED, "%s: unsupported dims B=%d Nt=%d D=%d Ca=%d Cs=%d (D in {384, 768, 1024}, B >= 1, Nt >= 2, B Nt < 2^31, Ca, Cs >= 2)", who,
                                a->B, a->Nt, a->D, a->Ca, a->Cs);
    DEVIAS_REQUIRE(!a->unified || a->Ca == a->Cs, "%s: the unified head gives both tokens the same Ca = Cs columns, got Ca=%d Cs=%d", who, a->Ca, a->Cs);
    DEVIAS_REQUIRE(a->eps > 0.f, "%s: eps must be positive", who);
    DEVIAS_REQUIRE(a->Wa && a->ba && a->ln_w && a->ln_b && (a->unified || (a->Ws && a->bs)), "%s: null parameter", who);
    DEVIAS_REQUIRE(aligned16(a->Wa) && aligned16(a->ba) && aligned16(a->Ws) && aligned16(a->bs), "%s: W / bias must be 16-byte aligned", who);
    DEVIAS_REQUIRE(a->ws && aligned16(a->ws), "%s: ws must be 16-byte aligned, non-null", who);
    DEVIAS_REQUIRE(a->ws_bytes >= devias_two_token_head_workspace_bytes(a->B, a->Nt, a->D, a->Ca, a->Cs, a->unified, a->dtype), "%s: workspace too small", who);
    return DEVIAS_OK;
}

int distill_check(const char* who, const void* student, const float* teacher, int B, int C, int Ct, int dtype, int mode, float weight) {
    DEVIAS_REQUIRE(student && teacher, "%s: null student / teacher", who);
    DEVIAS_REQUIRE(dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    DEVIAS_REQUIRE(mode == DEVIAS_DISTILL_KL || mode == DEVIAS_DISTILL_CE, "%s: bad mode %d (DEVIAS_DISTILL_KL or DEVIAS_DISTILL_CE)", who, mode);
    DEVIAS_REQUIRE(B >= 1 && Ct >= 2 && C >= Ct && C < (1 << 24), "%s: bad dims B=%d C=%d Ct=%d (B >= 1, 2 <= Ct <= C < 2^24)", who, B, C, Ct);
    DEVIAS_REQUIRE(weight == weight, "%s: weight is NaN", who);
    return DEVIAS_OK;
}

}  // namespace

extern "C" int64_t devias_two_token_head_workspace_bytes(int32_t B, int32_t Nt, int32_t D, int32_t Ca, int32_t Cs, int32_t unified, int32_t dtype) {
    if (!dims_supported(B, Nt, D, Ca, Cs) || !dtype_ok(dtype) || (unified && Ca != Cs)) return 0;
    return kernel_ws_bytes(B, D, Ca, Cs, unified, dtype) + Tmp(Arena(nullptr), B, D, Ca, Cs, dtype).bytes;
}
extern "C" int64_t devias_two_token_head_save_bytes(int32_t B, int32_t D, int32_t dtype) {
    if (!dims_supported(B, 2, D, 2, 2) || !dtype_ok(dtype)) return 0;
    Arena ar(nullptr);
    Save(ar, B, D, dtype);          // (carved at address 0: the arena ends at its size)
    return ar.off;
}

extern "C" int devias_two_token_head_fwd(const devias_two_token_head_args* a, const void* h, void* token_a, void* token_s, void* logits_a, void* logits_s, void* save,
                                         void* stream) {
    const char* who = "devias_two_token_head_fwd";
    RUN(tt_check(a, who));
    DEVIAS_REQUIRE(h && token_a && token_s && logits_a && aligned16(h) && aligned16(token_a) && aligned16(token_s) && aligned16(logits_a),
                   "%s: h / token_a / token_s / logits_a must be non-null, 16-byte aligned", who);
    DEVIAS_REQUIRE(a->unified || (logits_s && aligned16(logits_s)), "%s: logits_s must be non-null, 16-byte aligned (separate heads)", who);
    DEVIAS_REQUIRE(!save || aligned16(save), "%s: save must be 16-byte aligned", who);
    const int B = a->B, Nt = a->Nt, D = a->D, Ca = a->Ca, Cs = a->Cs;
    hipStream_t st = (hipStream_t)stream;
    const int64_t kw = kernel_ws_bytes(B, D, Ca, Cs, a->unified, a->dtype);
    const Ctx c{a->dtype, a->ws, kw, nullptr, 0, stream};
    const Tmp t(Arena(reinterpret_cast<char*>(a->ws) + kw), B, D, Ca, Cs, a->dtype);
    Arena own(save);
    const Save s = save ? Save(own, B, D, a->dtype) : t.s;          // the caller's arena, or (nothing to keep) the one in the workspace
    devias_range rg("two_token_head_fwd");
    g_two_token_head_calls.fetch_add(1, std::memory_order_relaxed);
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((tt_ln_fwd_kernel<T>), dim3(2 * B), dim3(NT), 0, st, (const T*)h, B, Nt, D, a->eps, a->ln_w, a->ln_b, a->mask_a, a->mask_s, (T*)token_a, (T*)token_s,
                           (T*)s.a, s.xhat, s.rstd);
    });
    DEVIAS_CHECK_LAUNCH("devias_two_token_head_fwd(layernorm)");
    Epi e; e.bias = a->ba;
    if (a->unified) {
        RUN(gemm(c, s.a, a->Wa, logits_a, 2 * B, Ca, D, D, D, 0, 0, e));          // the one weight read once: logits_a is [2B, Ca], the scene rows below the action rows
    } else {
        RUN(gemm(c, s.a, a->Wa, logits_a, B, Ca, D, D, D, 0, 0, e));
        e.bias = a->bs;
        RUN(gemm(c, s.a + (int64_t)B * D * esize(a->dtype), a->Ws, logits_s, B, Cs, D, D, D, 0, 0, e));
    }
    return DEVIAS_OK;
}

extern "C" int devias_two_token_head_bwd(const devias_two_token_head_args* a, const void* save, const void* dlogits_a, const void* dlogits_s, const void* dtoken_a,
                                         const void* dtoken_s, void* dx, const devias_two_token_head_grads* g, void* stream) {
    const char* who = "devias_two_token_head_bwd";
    RUN(tt_check(a, who));
    DEVIAS_REQUIRE(save && dlogits_a && dlogits_s && dx && g && aligned16(save) && aligned16(dx),
                   "%s: null pointer (save / dlogits_a / dlogits_s / dx / grads), or save / dx not 16-byte aligned", who);
    DEVIAS_REQUIRE(a->unified || (aligned16(dlogits_a) && aligned16(dlogits_s)), "%s: dlogits_a / dlogits_s must be 16-byte aligned (separate heads: GEMM operands)", who);
    REQUIRE_STRUCT_SIZE(g, devias_two_token_head_grads, who);
    DEVIAS_REQUIRE(g->dWa && g->dba && g->dln_w && g->dln_b && (a->unified || (g->dWs && g->dbs)), "%s: null gradient destination", who);
    const int B = a->B, Nt = a->Nt, D = a->D, Ca = a->Ca, Cs = a->Cs, chunks = cdiv(Nt, TOK), R = stream_rows(D, a->dtype),
              nth = R * (D / (a->dtype == DEVIAS_BF16 ? 8 : 4));
    hipStream_t st = (hipStream_t)stream;
    const int64_t kw = kernel_ws_bytes(B, D, Ca, Cs, a->unified, a->dtype), es = esize(a->dtype);
    const Ctx c{a->dtype, a->ws, kw, nullptr, 0, stream};
    const Tmp t(Arena(reinterpret_cast<char*>(a->ws) + kw), B, D, Ca, Cs, a->dtype);
    Arena own(save);
    const Save s(own, B, D, a->dtype);
    devias_range rg("two_token_head_bwd");
    g_two_token_head_calls.fetch_add(1, std::memory_order_relaxed);
    // the heads
    Epi e;
    if (a->unified) {
        const int64_t n = (int64_t)B * Ca;
        dispatch_t(a->dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            hipLaunchKernelGGL((tt_stack_kernel<T>), dim3(cdiv(n, NT)), dim3(NT), 0, st, (const T*)dlogits_a, (const T*)dlogits_s, n, (T*)t.dl2);
        });
        DEVIAS_CHECK_LAUNCH("devias_two_token_head_bwd(stack)");
        RUN(wgrad(c, t.dl2, s.a, g->dWa, 2 * B, Ca, D));
        RUN(colsum(c, t.dl2, 2 * B, Ca, g->dba));
        RUN(gemm(c, t.dl2, a->Wa, t.da, 2 * B, D, Ca, Ca, D, 0, 1, e, 1 /* fp32 output: da is not rounded to T */));
    } else {
        const char* a_s = s.a + (int64_t)B * D * es;
        RUN(wgrad(c, dlogits_a, s.a, g->dWa, B, Ca, D));
        RUN(colsum(c, dlogits_a, B, Ca, g->dba));
        RUN(gemm(c, dlogits_a, a->Wa, t.da, B, D, Ca, Ca, D, 0, 1, e, 1));
        RUN(wgrad(c, dlogits_s, a_s, g->dWs, B, Cs, D));
        RUN(colsum(c, dlogits_s, B, Cs, g->dbs));
        RUN(gemm(c, dlogits_s, a->Ws, t.da + (int64_t)B * D, B, D, Cs, Cs, D, 0, 1, e, 1));
    }
    // LayerNorm backward per stacked row, then every row of dx
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((tt_ln_bwd_kernel<T>), dim3(2 * B), dim3(NT), 0, st, t.da, (const T*)dtoken_a, (const T*)dtoken_s, a->mask_a, a->mask_s, s.xhat, s.rstd, a->ln_w, B, D,
                           (T*)t.dxrow, t.pg, t.pb);
    });
    DEVIAS_CHECK_LAUNCH("devias_two_token_head_bwd(layernorm)");
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((tt_dx_kernel<T>), dim3(B * chunks), dim3(nth), 0, st, (const T*)t.dxrow, B, Nt, D, chunks, R, (T*)dx);
    });
    DEVIAS_CHECK_LAUNCH("devias_two_token_head_bwd(dx)");
    // d gamma / d beta: per-row partials summed over the 2B rows in index order, ONE launch
    DeviasDeferList dl; dl.n = 0;
    dl.jobs[dl.n++] = DeviasReduceJob{t.pg, 2 * B, D, D, g->dln_w, 0.f};
    dl.jobs[dl.n++] = DeviasReduceJob{t.pb, 2 * B, D, D, g->dln_b, 0.f};
    RUN(devias_flush_deferred(&dl, st));
    return DEVIAS_OK;
}

extern "C" int64_t devias_distill_workspace_bytes(int32_t B) { return B >= 1 ? (int64_t)B * 4 : 0; }

extern "C" int devias_distill_fwd(const void* student, const float* teacher, int32_t B, int32_t C, int32_t Ct, int32_t dtype, int32_t mode, float weight, float* tmin,
                                  float* loss, float* ws, void* stream) {
    const char* who = "devias_distill_fwd";
    RUN(distill_check(who, student, teacher, B, C, Ct, dtype, mode, weight));
    DEVIAS_REQUIRE(loss && ws && (C == Ct || tmin), "%s: null loss / ws, or no tmin for a padded teacher", who);
    hipStream_t st = (hipStream_t)stream;
    const int ce = mode == DEVIAS_DISTILL_CE;
    if (C > Ct && !ce) {          // (the CE branch never reads the pad value: it lies below every teacher logit)
        hipLaunchKernelGGL(distill_min_kernel, dim3(1), dim3(NT), 0, st, teacher, (int64_t)B * Ct, tmin);
        DEVIAS_CHECK_LAUNCH("devias_distill_fwd(min)");
    }
    dispatch_t(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((distill_fwd_kernel<T>), dim3(B), dim3(NT), 0, st, (const T*)student, teacher, tmin, C, Ct, ce, ws);
    });
    DEVIAS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(distill_final_kernel, dim3(1), dim3(64), 0, st, ws, B, ce ? 1.f : weight, loss);
    DEVIAS_CHECK_LAUNCH("devias_distill_fwd(final)");
    return DEVIAS_OK;
}

extern "C" int devias_distill_bwd(const void* student, const float* teacher, int32_t B, int32_t C, int32_t Ct, int32_t dtype, int32_t mode, float weight, const float* tmin,
                                  const float* g_loss, void* dlogits, void* stream) {
    const char* who = "devias_distill_bwd";
    RUN(distill_check(who, student, teacher, B, C, Ct, dtype, mode, weight));
    DEVIAS_REQUIRE(g_loss && dlogits && (C == Ct || tmin), "%s: null g_loss / dlogits, or no tmin for a padded teacher", who);
    hipStream_t st = (hipStream_t)stream;
    const int ce = mode == DEVIAS_DISTILL_CE;
    dispatch_t(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((distill_bwd_kernel<T>), dim3(B), dim3(NT), 0, st, (const T*)student, teacher, tmin, B, C, Ct, ce, ce ? 1.f : weight, g_loss, (T*)dlogits);
    });
    DEVIAS_CHECK_LAUNCH(who);
    return DEVIAS_OK;
}
