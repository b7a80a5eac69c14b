// The plain video ViT's part after the encoder (model/modeling_finetune.py: fc_norm(x.mean(1)) or norm(x)[:, 0], fc_dropout, head) as ONE C-ABI call per direction.
//
//   devias_pool_head_fwd   h [B*Nt, D] -> t = mean over the clip's Nt tokens (MEAN) or the clip's row 0 (CLS) -> LayerNorm -> token [B, D];
//                          a = token's unrounded value * mask; logits = a W^T + b
//   devias_pool_head_bwd   dlogits (+ dtoken) -> dW, db, d gamma, d beta, and EVERY row of dx [B*Nt, D] (MEAN: the LayerNorm's input gradient * fl(1/Nt) in each token
//                          row of the clip; CLS: in row 0, zeros elsewhere)
//
// What it is bound by: the two streams.  The forward reads h once (77 MB at B = 32, Nt = 1568, D = 768 in bf16), the backward writes dx once; everything between is
// [B, D] or [B, C].  So two streaming kernels with 16 bytes per lane and access, and around them one-workgroup-per-clip kernels built from row_kernels.h as
// fusion_head.hip's are (strided scalar accesses, two-pass fp32 statistics) plus the library's GEMM / weight-gradient / column-sum launchers (region_host.h).
//
//   pool_partial_kernel   one workgroup per (clip, chunk of DEVIAS_POOL_HEAD_CHUNK tokens): lane (r, c) owns the 16-byte column group c and adds rows r, r + R, ... of
//                         the chunk in that order in fp32 (four loads in flight), the R row sets are combined through LDS in index order, the chunk's sum goes to the
//                         workspace in fp32: part[b][chunk][D]
//   pool_ln_fwd_kernel    one workgroup per clip: the chunks summed in index order, * fl(1/Nt) (a MULTIPLICATION by the rounded reciprocal, not a division), LayerNorm
//   pool_ln_bwd_kernel    one workgroup per clip: LayerNorm backward on the saved x^ / rstd, the clip's d gamma / d beta partials, the dx row rounded ONCE to T
//   pool_dx_kernel        the forward's grid again: every token row of the chunk written with 16-byte stores (the dx row or zeros)
//
// No atomics: the token sum is two fixed-order stages, d gamma / d beta are per-clip partials summed over the clips in index order by one devias_flush_deferred launch.
// Roundings to T: token, a, logits, dx -- each once, from fp32.  da (the classifier's input gradient) stays fp32 (GEMM with an fp32 output).
#include "common.h"
#include <string.h>
#include <atomic>
#include "roctx_shim.h"
#include "region_host.h"      // split policies, GEMM / weight-gradient calls, the arena carver, argument checks, dispatch_t
#include "row_kernels.h"       // the per-clip kernels: NT, EPT, block reductions, the row LayerNorm's statistics and backward means

static std::atomic<int64_t> g_pool_head_calls;
void devias_pool_head_counter_reset() { g_pool_head_calls.store(0, std::memory_order_relaxed); }      // api.hip: devias_counters_reset
extern "C" int64_t devias_pool_head_launches(void) { return g_pool_head_calls.load(std::memory_order_relaxed); }

namespace {

enum { TOK = DEVIAS_POOL_HEAD_CHUNK, NTS = 384 };      // streaming kernels: tokens per workgroup, most threads

template <typename T> struct Vec16;
template <> struct Vec16<bf16> { typedef bf16x8 type; enum { N = 8 }; };
template <> struct Vec16<float> { typedef f32x4 type; enum { N = 4 }; };

// rows of a chunk that the streaming kernels work on side by side: R * (D / VEC) threads, 256 or 384
inline int stream_rows(int D, int dtype) { const int vc = D / (dtype == DEVIAS_BF16 ? 8 : 4); return NTS / vc; }

// ---- forward, stage 1: the chunk sums ---------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTS) void pool_partial_kernel(const T* __restrict__ h, int Nt, int D, int chunks, int R, float* __restrict__ part) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = Vec16<T>::N;
    __shared__ __attribute__((aligned(16))) float sm[3072];      // (R - 1) row sets of D floats: R D <= 3072 for every accepted (D, T)
    const int Vc = D / VEC;
    const int c = threadIdx.x % Vc, r = threadIdx.x / Vc;       // blockDim.x == R * Vc exactly
    const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int t0 = ch * TOK, t1 = min(Nt, t0 + TOK);
    const T* base = h + (int64_t)b * Nt * D + c * VEC;
    float acc[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) acc[i] = 0.f;
    int t = t0 + r;
    for (; t + 3 * R < t1; t += 4 * R) {
        const V v0 = *reinterpret_cast<const V*>(base + (int64_t)t * D);
        const V v1 = *reinterpret_cast<const V*>(base + (int64_t)(t + R) * D);
        const V v2 = *reinterpret_cast<const V*>(base + (int64_t)(t + 2 * R) * D);
        const V v3 = *reinterpret_cast<const V*>(base + (int64_t)(t + 3 * R) * D);
#pragma unroll
        for (int i = 0; i < VEC; ++i) { acc[i] += (float)v0[i]; acc[i] += (float)v1[i]; acc[i] += (float)v2[i]; acc[i] += (float)v3[i]; }
    }
    for (; t < t1; t += R) {
        const V v0 = *reinterpret_cast<const V*>(base + (int64_t)t * D);
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[i] += (float)v0[i];
    }
    if (r > 0) {
#pragma unroll
        for (int i = 0; i < VEC; i += 4) *reinterpret_cast<f32x4*>(&sm[(r - 1) * D + c * VEC + i]) = f32x4{acc[i], acc[i + 1], acc[i + 2], acc[i + 3]};
    }
    __syncthreads();
    if (r == 0) {
        for (int rr = 1; rr < R; ++rr) {
#pragma unroll
            for (int i = 0; i < VEC; i += 4) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(&sm[(rr - 1) * D + c * VEC + i]);
                acc[i] += o[0]; acc[i + 1] += o[1]; acc[i + 2] += o[2]; acc[i + 3] += o[3];
            }
        }
        float* out = part + (int64_t)blockIdx.x * D + c * VEC;
#pragma unroll
        for (int i = 0; i < VEC; i += 4) *reinterpret_cast<f32x4*>(out + i) = f32x4{acc[i], acc[i + 1], acc[i + 2], acc[i + 3]};
    }
}

// ---- forward, stage 2: finish the mean (or take row 0), LayerNorm, mask ------------------------------------------------------------------------
// token = T(y), a = T(y * mask) with y = x^ gamma + beta in fp32: the mask meets the UNROUNDED y.  Saved: x^ fp32 [B, D], rstd fp32 [B], a.
template <typename T>
__global__ __launch_bounds__(NT) void pool_ln_fwd_kernel(const T* __restrict__ h, const float* __restrict__ part, int pool, int Nt, int D, int chunks, float inv_nt, float eps,
                                                         const float* __restrict__ gw, const float* __restrict__ gb, const float* __restrict__ mask, T* __restrict__ token,
                                                         T* __restrict__ a, float* __restrict__ xhat, float* __restrict__ rstd_out) {
    __shared__ float sm[8];
    const int b = blockIdx.x;
    float v[EPT], mean, rstd;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        v[i] = 0.f;
        if (k < D) {
            if (pool == DEVIAS_POOL_CLS) {
                v[i] = to_f32(h[(int64_t)b * Nt * D + k]);
            } else {
                float s = 0.f;
                for (int p = 0; p < chunks; ++p) s += part[((int64_t)b * chunks + p) * D + k];
                v[i] = s * inv_nt;
            }
        }
    }
    row_ln_stats(v, D, eps, sm, mean, rstd);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < D) {
            const int64_t e = (int64_t)b * D + k;
            const float xh = (v[i] - mean) * rstd;
            const float y = xh * gw[k] + gb[k];
            xhat[e] = xh;
            token[e] = from_f32<T>(y);
            a[e] = from_f32<T>(mask ? y * mask[e] : y);
        }
    }
    if (threadIdx.x == 0) rstd_out[b] = rstd;
}

// ---- backward: LayerNorm backward per clip -----------------------------------------------------------------------------------------------------
// g = da * mask + dtoken (fp32); pg[b] = g x^, pb[b] = g; dxrow[b] = T(rstd (g gamma - mean(g gamma) - x^ mean(g gamma x^)) * scale), scale = fl(1/Nt) (MEAN) or 1 (CLS)
template <typename T>
__global__ __launch_bounds__(NT) void pool_ln_bwd_kernel(const float* __restrict__ da, const T* __restrict__ dtoken, const float* __restrict__ mask,
                                                         const float* __restrict__ xhat, const float* __restrict__ rstd_in, const float* __restrict__ gw, int D, float scale,
                                                         T* __restrict__ dxrow, float* __restrict__ pg, float* __restrict__ pb) {
    __shared__ float sm[8];
    const int b = blockIdx.x;
    const float rstd = rstd_in[b];
    float xh[EPT], gy[EPT], c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        xh[i] = 0.f; gy[i] = 0.f;
        if (k < D) {
            const int64_t e = (int64_t)b * D + k;
            float g = da[e];
            if (mask) g *= mask[e];
            if (dtoken) g += to_f32(dtoken[e]);
            xh[i] = xhat[e];
            pg[e] = g * xh[i]; pb[e] = g;
            gy[i] = g * gw[k];
            c1 += gy[i]; c2 += gy[i] * xh[i];
        }
    }
    row_ln_bwd_means(c1, c2, D, sm);
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        if (k < D) dxrow[(int64_t)b * D + k] = from_f32<T>(row_ln_dx(gy[i], xh[i], rstd, c1, c2) * scale);
    }
}

// ---- backward: every row of dx ------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NTS) void pool_dx_kernel(const T* __restrict__ dxrow, int pool, int Nt, int D, int chunks, int R, T* __restrict__ dx) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = Vec16<T>::N;
    const int Vc = D / VEC;
    const int c = threadIdx.x % Vc, r = threadIdx.x / Vc;
    const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int t0 = ch * TOK, t1 = min(Nt, t0 + TOK);
    const V val = *reinterpret_cast<const V*>(dxrow + (int64_t)b * D + c * VEC);
    V zero;
#pragma unroll
    for (int i = 0; i < VEC; ++i) zero[i] = from_f32<T>(0.f);
    T* base = dx + (int64_t)b * Nt * D + c * VEC;
    for (int t = t0 + r; t < t1; t += R) *reinterpret_cast<V*>(base + (int64_t)t * D) = (pool == DEVIAS_POOL_CLS && t != 0) ? zero : val;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
inline bool dims_supported(int B, int Nt, int D, int C) {
    return B >= 1 && Nt >= 1 && (int64_t)B * Nt <= 0x7fffffff && row_dim_ok(D) && C >= 2 && (int64_t)B * 1024 < 0x7fffffff;
}
int64_t kernel_ws_bytes(int B, int D, int C, int dtype) {
    int64_t w = max64(gemm_ws(B, C, D, 0), gemm_ws(B, D, C, 0));
    w = max64(w, max64(wgrad_ws(C, D, B, dtype), devias_colsum_workspace_bytes(B, C)));
    return al256(w) + 256;
}
// what backward reads of the forward: the normalised pooled rows and their rstd in fp32, the classifier's input a
struct Save {
    float *xhat, *rstd; char* a;
    Save(Arena& ar, int B, int D, int dtype) {
        xhat = (float*)ar.take((int64_t)B * D * 4); rstd = (float*)ar.take((int64_t)B * 4); a = ar.take((int64_t)B * D * esize(dtype));
    }
};
// what lives behind the kernels' workspace: the chunk sums; a Save of its own, which the forward writes where the caller keeps none; the backward's temporaries and per-clip partials
struct Tmp {
    float* part; Save s;          // (carved in this order)
    float *da, *pg, *pb;
    char* dxrow;
    int64_t bytes;
    Tmp(Arena ar, int B, int Nt, int D, int dtype) : part((float*)ar.take((int64_t)B * cdiv(Nt, TOK) * D * 4)), s(ar, B, D, dtype) {
        const int64_t es = esize(dtype), BD = (int64_t)B * D;
        da = (float*)ar.take(BD * 4); dxrow = ar.take(BD * es); pg = (float*)ar.take(BD * 4); pb = (float*)ar.take(BD * 4);
        bytes = ar.off;
    }
};

int pool_check(const devias_pool_head_args* a, const char* who) {
    DEVIAS_REQUIRE(a, "%s: null args", who);
    REQUIRE_STRUCT_SIZE(a, devias_pool_head_args, who);
    DEVIAS_REQUIRE(dtype_ok(a->dtype), "%s: bad dtype %d", who, a->dtype);
    DEVIAS_REQUIRE(a->pool == DEVIAS_POOL_MEAN || a->pool == DEVIAS_POOL_CLS, "%s: bad pool %d (DEVIAS_POOL_MEAN or DEVIAS_POOL_CLS)", who, a->pool);
    if (!dims_supported(a->B, a->Nt, a->D, a->C))
        return devias_set_error(DEVIAS_EUNSUPPORTED, "%s: unsupported dims B=%d Nt=%d D=%d C=%d (D in {384, 768, 1024}, B >= 1, Nt >= 1, B Nt < 2^31, C >= 2)", who, a->B, a->Nt,
                                a->D, a->C);
    DEVIAS_REQUIRE(a->eps > 0.f, "%s: eps must be positive", who);
    DEVIAS_REQUIRE(a->W && a->bias && a->ln_w && a->ln_b, "%s: null parameter", who);
    DEVIAS_REQUIRE(aligned16(a->W) && aligned16(a->bias), "%s: W / bias must be 16-byte aligned", who);
    DEVIAS_REQUIRE(a->ws && aligned16(a->ws), "%s: ws must be 16-byte aligned, non-null", who);
    DEVIAS_REQUIRE(a->ws_bytes >= devias_pool_head_workspace_bytes(a->B, a->Nt, a->D, a->C, a->dtype), "%s: workspace too small", who);
    return DEVIAS_OK;
}

}  // namespace

extern "C" int64_t devias_pool_head_workspace_bytes(int32_t B, int32_t Nt, int32_t D, int32_t C, int32_t dtype) {
    if (!dims_supported(B, Nt, D, C) || !dtype_ok(dtype)) return 0;
    return kernel_ws_bytes(B, D, C, dtype) + Tmp(Arena(nullptr), B, Nt, D, dtype).bytes;
}
extern "C" int64_t devias_pool_head_save_bytes(int32_t B, int32_t D, int32_t dtype) {
    if (!dims_supported(B, 1, D, 2) || !dtype_ok(dtype)) return 0;
    Arena ar(nullptr);
    Save(ar, B, D, dtype);          // (carved at address 0: the arena ends at its size)
    return ar.off;
}

extern "C" int devias_pool_head_fwd(const devias_pool_head_args* a, const void* h, void* token, void* logits, void* save, void* stream) {
    const char* who = "devias_pool_head_fwd";
    RUN(pool_check(a, who));
    DEVIAS_REQUIRE(h && token && logits && aligned16(h) && aligned16(token) && aligned16(logits), "%s: h / token / logits must be non-null, 16-byte aligned", who);
    DEVIAS_REQUIRE(!save || aligned16(save), "%s: save must be 16-byte aligned", who);
    const int B = a->B, Nt = a->Nt, D = a->D, C = a->C, chunks = cdiv(Nt, TOK), R = stream_rows(D, a->dtype), nth = R * (D / (a->dtype == DEVIAS_BF16 ? 8 : 4));
    hipStream_t st = (hipStream_t)stream;
    const int64_t kw = kernel_ws_bytes(B, D, C, a->dtype);
    const Ctx c{a->dtype, a->ws, kw, nullptr, 0, stream};
    const Tmp t(Arena(reinterpret_cast<char*>(a->ws) + kw), B, Nt, D, a->dtype);
    Arena own(save);
    const Save s = save ? Save(own, B, D, a->dtype) : t.s;          // the caller's arena, or (nothing to keep) the one in the workspace
    devias_range rg("pool_head_fwd");
    g_pool_head_calls.fetch_add(1, std::memory_order_relaxed);
    const float inv_nt = 1.0f / (float)Nt;
    if (a->pool == DEVIAS_POOL_MEAN) {
        dispatch_t(a->dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            hipLaunchKernelGGL((pool_partial_kernel<T>), dim3(B * chunks), dim3(nth), 0, st, (const T*)h, Nt, D, chunks, R, t.part);
        });
        DEVIAS_CHECK_LAUNCH("devias_pool_head_fwd(partial)");
    }
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((pool_ln_fwd_kernel<T>), dim3(B), dim3(NT), 0, st, (const T*)h, t.part, a->pool, Nt, D, chunks, inv_nt, a->eps, a->ln_w, a->ln_b, a->drop_mask,
                           (T*)token, (T*)s.a, s.xhat, s.rstd);
    });
    DEVIAS_CHECK_LAUNCH("devias_pool_head_fwd(layernorm)");
    Epi e; e.bias = a->bias;
    RUN(gemm(c, s.a, a->W, logits, B, C, D, D, D, 0, 0, e));
    return DEVIAS_OK;
}

extern "C" int devias_pool_head_bwd(const devias_pool_head_args* a, const void* save, const void* dlogits, const void* dtoken, void* dx, const devias_pool_head_grads* g,
                                    void* stream) {
    const char* who = "devias_pool_head_bwd";
    RUN(pool_check(a, who));
    DEVIAS_REQUIRE(save && dlogits && dx && g && aligned16(save) && aligned16(dx), "%s: null pointer (save / dlogits / dx / grads), or save / dx not 16-byte aligned", who);
    REQUIRE_STRUCT_SIZE(g, devias_pool_head_grads, who);
    DEVIAS_REQUIRE(g->dW && g->db && g->dln_w && g->dln_b, "%s: null gradient destination", who);
    const int B = a->B, Nt = a->Nt, D = a->D, C = a->C, chunks = cdiv(Nt, TOK), R = stream_rows(D, a->dtype), nth = R * (D / (a->dtype == DEVIAS_BF16 ? 8 : 4));
    hipStream_t st = (hipStream_t)stream;
    const int64_t kw = kernel_ws_bytes(B, D, C, a->dtype);
    const Ctx c{a->dtype, a->ws, kw, nullptr, 0, stream};
    const Tmp t(Arena(reinterpret_cast<char*>(a->ws) + kw), B, Nt, D, a->dtype);
    Arena own(save);
    const Save s(own, B, D, a->dtype);
    devias_range rg("pool_head_bwd");
    g_pool_head_calls.fetch_add(1, std::memory_order_relaxed);
    // classifier
    RUN(wgrad(c, dlogits, s.a, g->dW, B, C, D));
    RUN(colsum(c, dlogits, B, C, g->db));
    Epi e;
    RUN(gemm(c, dlogits, a->W, t.da, B, D, C, C, D, 0, 1, e, 1 /* fp32 output: da is not rounded to T */));
    // LayerNorm backward per clip, then every row of dx
    const float scale = a->pool == DEVIAS_POOL_MEAN ? 1.0f / (float)Nt : 1.0f;
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((pool_ln_bwd_kernel<T>), dim3(B), dim3(NT), 0, st, t.da, (const T*)dtoken, a->drop_mask, s.xhat, s.rstd, a->ln_w, D, scale, (T*)t.dxrow, t.pg, t.pb);
    });
    DEVIAS_CHECK_LAUNCH("devias_pool_head_bwd(layernorm)");
    dispatch_t(a->dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((pool_dx_kernel<T>), dim3(B * chunks), dim3(nth), 0, st, (const T*)t.dxrow, a->pool, Nt, D, chunks, R, (T*)dx);
    });
    DEVIAS_CHECK_LAUNCH("devias_pool_head_bwd(dx)");
    // d gamma / d beta: per-clip partials summed over the clips in index order, ONE launch
    DeviasDeferList dl; dl.n = 0;
    dl.jobs[dl.n++] = DeviasReduceJob{t.pg, B, D, D, g->dln_w, 0.f};
    dl.jobs[dl.n++] = DeviasReduceJob{t.pb, B, D, D, g->dln_b, 0.f};
    RUN(devias_flush_deferred(&dl, st));
    return DEVIAS_OK;
}
