// The part after the encoder of the two models that classify from one or two token rows per clip, as ONE C-ABI call per direction each:
//
//   devias_pool_head_*        the plain video ViT (model/modeling_finetune.py: fc_norm(x.mean(1)) or norm(x)[:, 0], fc_dropout, head)
//   devias_two_token_head_*   the two-token multi-task baseline (model/modeling_multi_task.py: norm(x)[:, 0] and norm(x)[:, -1], fc_dropout on each, head / scene_head)
//
// Both are the same region.  The rows are worked on STACKED: G groups of B rows, G = 1 (pooled head) or 2 (two-token head); row g B + b belongs to clip b.  Group 0 is the
// clip's row 0 (CLS, two-token: the action token) or the mean of its Nt rows (MEAN); group 1 is its row Nt - 1 (the scene token).
//
//   forward    h [B*Nt, D] -> the G B rows -> LayerNorm (one norm serves every group) -> token per group [B, D]; a = token's unrounded value * the group's mask;
//              logits = a W^T + bias per group, or (unified, G = 2) ONE GEMM over the 2B stacked rows against the group-0 head
//   backward   dlogits (+ dtoken) per group -> dW, db per head (unified: one pair over the 2B rows), d gamma, d beta, and EVERY row of dx [B*Nt, D]: the LayerNorm's input
//              gradient * fl(1/Nt) in each token row of the clip (MEAN), or in row 0 (and, G = 2, row Nt - 1) with zeros elsewhere
//
// What it is bound by: the two streams.  MEAN's forward reads h once (77 MB at B = 32, Nt = 1568, D = 768 in bf16), every backward writes dx once; everything between is
// [G B, D] or [G B, C].  So two streaming kernels with 16 bytes per lane and access, and around them one-workgroup-per-row kernels built from row_kernels.h as
// fusion_head.hip's are (strided scalar accesses, two-pass fp32 statistics) plus the library's GEMM / weight-gradient / column-sum launchers (region_host.h).
//
//   pool_partial_kernel   MEAN only.  One workgroup per (clip, chunk of DEVIAS_POOL_HEAD_CHUNK tokens): lane (r, c) owns the 16-byte column group c and adds rows r, r + R, ...
//                         of the chunk in that order in fp32 (four loads in flight), the R row sets are combined through LDS in index order, the chunk's sum goes to the
//                         workspace in fp32: part[b][chunk][D]
//   head_ln_fwd_kernel    one workgroup per stacked row: the row from h, or (its MEAN instance) the chunks summed in index order * fl(1/Nt) (a MULTIPLICATION by the rounded reciprocal, not a
//                         division); LayerNorm
//   head_ln_bwd_kernel    one workgroup per stacked row: LayerNorm backward on the saved x^ / rstd, the row's d gamma / d beta partials, the dx row rounded ONCE to T
//   head_dx_kernel        pool_partial_kernel's grid: every token row of the chunk written with 16-byte stores (a dx row or zeros)
//   head_stack_kernel     unified only: the two [B, C] logit gradients one under the other
//
// No atomics: the token sum is two fixed-order stages, d gamma / d beta are per-row partials summed over the G B rows in index order by one devias_flush_deferred launch.
// Roundings to T: token, a, logits, dx -- each once, from fp32.  da (the heads' input gradient) stays fp32 (GEMM with an fp32 output).
#include "common.h"
#include <string.h>
#include <atomic>
#include "roctx_shim.h"
#include "region_host.h"      // split policies, GEMM / weight-gradient calls, the arena carver, argument checks, dispatch_t
#include "row_kernels.h"       // the per-row kernels: NT, EPT, block reductions, the row LayerNorm's statistics and backward means

// a call counter per family of entry points (both counter banks are closed); api.hip's devias_counters_reset calls the two resets
static std::atomic<int64_t> g_pool_head_calls, g_two_token_head_calls;
void devias_pool_head_counter_reset() { g_pool_head_calls.store(0, std::memory_order_relaxed); }
void devias_two_token_head_counter_reset() { g_two_token_head_calls.store(0, std::memory_order_relaxed); }
extern "C" int64_t devias_pool_head_launches(void) { return g_pool_head_calls.load(std::memory_order_relaxed); }
extern "C" int64_t devias_two_token_head_launches(void) { return g_two_token_head_calls.load(std::memory_order_relaxed); }

namespace {

enum { TOK = DEVIAS_POOL_HEAD_CHUNK, NTS = 384 };      // streaming kernels: tokens per workgroup, most threads
enum { LIVE_ALL, LIVE_FIRST, LIVE_FIRST_LAST };        // head_dx_kernel: the token rows of a clip that take a dx row (the others take zeros)

template <typename T> struct Vec16;
template <> struct Vec16<bf16> { typedef bf16x8 type; enum { N = 8 }; };
template <> struct Vec16<float> { typedef f32x4 type; enum { N = 4 }; };

// rows of a chunk that the streaming kernels work on side by side: R * (D / VEC) threads, 256 or 384
inline int stream_rows(int D, int dtype) { const int vc = D / (dtype == DEVIAS_BF16 ? 8 : 4); return NTS / vc; }

// ---- forward, MEAN: the chunk sums ---------------------------------------------------------------------------------------------------------------
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

// ---- forward: take the row (or finish the mean), LayerNorm, mask -----------------------------------------------------------------------------------
// stacked row j: clip b = j mod B, group j / B.  Its input is h's row 0 (group 0) or Nt - 1 (group 1) of the clip, or (MEAN, which has one group) the clip's mean.
// MEAN is a template argument: with the row source chosen at run time the mean's path measured 0.06 us over the pooled head's kernel (profiles/token_head.txt).
// token = T(y), a = T(y * mask) with y = x^ gamma + beta in fp32: the mask meets the UNROUNDED y.  token and mask are the group's [B, D]; saved stacked: x^ fp32 [G B, D],
// rstd fp32 [G B], a T [G B, D].
template <typename T, bool MEAN>
__global__ __launch_bounds__(NT) void head_ln_fwd_kernel(const T* __restrict__ h, const float* __restrict__ part, int B, int Nt, int D, int chunks, float inv_nt, float eps,
                                                         const float* __restrict__ gw, const float* __restrict__ gb, const float* __restrict__ mask0,
                                                         const float* __restrict__ mask1, T* __restrict__ token0, T* __restrict__ token1, T* __restrict__ a,
                                                         float* __restrict__ xhat, float* __restrict__ rstd_out) {
    __shared__ float sm[8];
    const int j = blockIdx.x, g1 = !MEAN && j >= B, b = g1 ? j - B : j;
    const T* row = h + ((int64_t)b * Nt + (g1 ? Nt - 1 : 0)) * D;
    const float* mask = g1 ? mask1 : mask0;
    T* token = g1 ? token1 : token0;
    float v[EPT], mean, rstd;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int k = threadIdx.x + NT * i;
        v[i] = 0.f;
        if (k < D) {
            if (!MEAN) {
                v[i] = to_f32(row[k]);
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

// ---- backward: LayerNorm backward per stacked row ----------------------------------------------------------------------------------------------------
// g = da * mask + dtoken (fp32; the group's mask and dtoken); pg[j] = g x^, pb[j] = g; dxrow[j] = T(rstd (g gamma - mean(g gamma) - x^ mean(g gamma x^)) * scale),
// scale = fl(1/Nt) (MEAN) or 1 (a multiplication by 1.0f is exact)
template <typename T>
__global__ __launch_bounds__(NT) void head_ln_bwd_kernel(const float* __restrict__ da, const T* __restrict__ dtoken0, const T* __restrict__ dtoken1,
                                                         const float* __restrict__ mask0, const float* __restrict__ mask1, const float* __restrict__ xhat,
                                                         const float* __restrict__ rstd_in, const float* __restrict__ gw, int B, int D, float scale, T* __restrict__ dxrow,
                                                         float* __restrict__ pg, float* __restrict__ pb) {
    __shared__ float sm[8];
    const int j = blockIdx.x, g1 = j >= B, b = g1 ? j - B : j;
    const float* mask = g1 ? mask1 : mask0;
    const T* dtoken = g1 ? dtoken1 : dtoken0;
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
        if (k < D) dxrow[(int64_t)j * D + k] = from_f32<T>(row_ln_dx(gy[i], xh[i], rstd, c1, c2) * scale);
    }
}

// ---- backward: every row of dx ------------------------------------------------------------------------------------------------------------------------
// one workgroup per (clip, chunk of TOK token rows).  dxrow[b] goes to every row (LIVE_ALL: read once, up front) or to row 0; LIVE_FIRST_LAST: dxrow[B + b] goes to row
// Nt - 1; zeros elsewhere.  LIVE is a template argument: as a kernel argument it cost two VGPRs over either predecessor (profiles/token_head.txt).
template <typename T, int LIVE>
__global__ __launch_bounds__(NTS) void head_dx_kernel(const T* __restrict__ dxrow, int B, int Nt, int D, int chunks, int R, T* __restrict__ dx) {
    typedef typename Vec16<T>::type V;
    constexpr int VEC = Vec16<T>::N;
    const int Vc = D / VEC;
    const int c = threadIdx.x % Vc, r = threadIdx.x / Vc;       // blockDim.x == R * Vc exactly
    const int b = blockIdx.x / chunks, ch = blockIdx.x % chunks;
    const int t0 = ch * TOK, t1 = min(Nt, t0 + TOK);
    V fill;
#pragma unroll
    for (int i = 0; i < VEC; ++i) fill[i] = from_f32<T>(0.f);
    if (LIVE == LIVE_ALL) fill = *reinterpret_cast<const V*>(dxrow + (int64_t)b * D + c * VEC);
    T* base = dx + (int64_t)b * Nt * D + c * VEC;
    for (int t = t0 + r; t < t1; t += R) {
        V val = fill;
        if (LIVE != LIVE_ALL && t == 0) val = *reinterpret_cast<const V*>(dxrow + (int64_t)b * D + c * VEC);
        else if (LIVE == LIVE_FIRST_LAST && t == Nt - 1) val = *reinterpret_cast<const V*>(dxrow + (int64_t)(B + b) * D + c * VEC);
        *reinterpret_cast<V*>(base + (int64_t)t * D) = val;
    }
}

// unified head, backward: the two [B, C] gradients one under the other (the weight gradient and the column sums run over the 2B rows)
template <typename T>
__global__ __launch_bounds__(NT) void head_stack_kernel(const T* __restrict__ top, const T* __restrict__ bottom, int64_t n, T* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i < n) { out[i] = top[i]; out[n + i] = bottom[i]; }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------------------
// One call of either family, as its entry point describes it: G groups of B rows; a head (W, bias, C columns) and a mask per group, or (unified) head 0 over all G B rows.
struct Call {
    const char* who; std::atomic<int64_t>* calls;
    int dtype, B, Nt, D, G, mean, unified;
    float eps; const float *ln_w, *ln_b; float* ws;
    const float* mask[2]; int C[2]; const void* W[2]; const float* bias[2];
    int rows() const { return G * B; }
    int heads() const { return unified ? 1 : G; }
    int M() const { return unified ? G * B : B; }                // rows of one head's products
    int Cmax() const { return C[0] > C[1] ? C[0] : C[1]; }      // (every workspace term grows with C)
};

// (pooled head: Ca = Cs = C)
inline bool dims_supported(int G, int B, int Nt, int D, int Ca, int Cs) {
    return B >= 1 && Nt >= G && (int64_t)B * Nt <= 0x7fffffff && row_dim_ok(D) && Ca >= 2 && Cs >= 2 && (int64_t)G * B * 1024 < 0x7fffffff;
}
int64_t kernel_ws_bytes(int M, int D, int C, int dtype) {
    int64_t w = max64(gemm_ws(M, C, D, 0), gemm_ws(M, D, C, 0));
    w = max64(w, max64(wgrad_ws(C, D, M, dtype), devias_colsum_workspace_bytes(M, C)));
    return al256(w) + 256;
}
// what backward reads of the forward: the normalised rows and their rstd in fp32, the heads' input a -- all stacked [rows, ...]
struct Save {
    float *xhat, *rstd; char* a;
    Save(Arena& ar, int64_t rows, int D, int dtype) {
        xhat = (float*)ar.take(rows * D * 4); rstd = (float*)ar.take(rows * 4); a = ar.take(rows * D * esize(dtype));
    }
};
// what lives behind the kernels' workspace: the chunk sums; a Save of its own, which the forward writes where the caller keeps none; the backward's temporaries and per-row
// partials; the stacked logit gradients.  The first piece is the pooled head's and the last the two-token head's, whatever the mode (the size queries do not know it); the
// other family takes 0 bytes there, which leaves the arena's offset alone.
struct Tmp {
    float* part; Save s;          // (carved in this order)
    float *da, *pg, *pb;
    char *dxrow, *dl2;
    int64_t bytes;
    Tmp(Arena ar, int G, int B, int Nt, int D, int Cmax, int dtype) : part((float*)ar.take(G == 1 ? (int64_t)B * cdiv(Nt, TOK) * D * 4 : 0)), s(ar, (int64_t)G * B, D, dtype) {
        const int64_t es = esize(dtype), BD = (int64_t)G * B * D;
        da = (float*)ar.take(BD * 4); dxrow = ar.take(BD * es); pg = (float*)ar.take(BD * 4); pb = (float*)ar.take(BD * 4);
        dl2 = ar.take(G == 2 ? (int64_t)2 * B * Cmax * es : 0);
        bytes = ar.off;
    }
};

#define CHECK_STAGE(who, stage)                                                                                                               \
    do {                                                                                                                                      \
        hipError_t e__ = hipGetLastError();                                                                                                   \
        if (e__ != hipSuccess) return devias_set_error(DEVIAS_ELAUNCH, "%s(" stage "): launch failed: %s", who, hipGetErrorString(e__));     \
    } while (0)

// the region's workspace behind the checks: the launchers' context, the temporaries, the saved pieces (the caller's arena, or the one in the workspace)
struct Work {
    int64_t kw; Ctx c; Tmp t; Save s;          // (initialised in this order)
    Work(const Call& r, const void* save, void* stream)
        : kw(kernel_ws_bytes(r.M(), r.D, r.Cmax(), r.dtype)), c{r.dtype, r.ws, kw, nullptr, 0, stream},
          t(Arena(reinterpret_cast<char*>(r.ws) + kw), r.G, r.B, r.Nt, r.D, r.Cmax(), r.dtype), s(t.s) {
        Arena own(save);
        if (save) s = Save(own, r.rows(), r.D, r.dtype);
    }
};

int head_fwd(const Call& r, const void* h, void* const token[2], void* const logits[2], void* save, void* stream) {
    const int B = r.B, Nt = r.Nt, D = r.D, chunks = cdiv(Nt, TOK), R = stream_rows(D, r.dtype), nth = R * (D / (r.dtype == DEVIAS_BF16 ? 8 : 4));
    hipStream_t st = (hipStream_t)stream;
    const Work w(r, save, stream);
    devias_range rg(r.who + 7);          // ("devias_" dropped)
    r.calls->fetch_add(1, std::memory_order_relaxed);
    if (r.mean) {
        dispatch_t(r.dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            hipLaunchKernelGGL((pool_partial_kernel<T>), dim3(B * chunks), dim3(nth), 0, st, (const T*)h, Nt, D, chunks, R, w.t.part);
        });
        CHECK_STAGE(r.who, "partial");
    }
    dispatch_t(r.dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const auto kernel = r.mean ? head_ln_fwd_kernel<T, true> : head_ln_fwd_kernel<T, false>;
        hipLaunchKernelGGL(kernel, dim3(r.rows()), dim3(NT), 0, st, (const T*)h, w.t.part, B, Nt, D, chunks, 1.0f / (float)Nt, r.eps, r.ln_w, r.ln_b, r.mask[0], r.mask[1],
                           (T*)token[0], (T*)token[1], (T*)w.s.a, w.s.xhat, w.s.rstd);
    });
    CHECK_STAGE(r.who, "layernorm");
    for (int i = 0; i < r.heads(); ++i) {          // (unified: the one weight read once, logits[0] is [2B, C], the group-1 rows below the group-0 rows)
        Epi e; e.bias = r.bias[i];
        RUN(gemm(w.c, w.s.a + (int64_t)i * B * D * esize(r.dtype), r.W[i], logits[i], r.M(), r.C[i], D, D, D, 0, 0, e));
    }
    return DEVIAS_OK;
}

int head_bwd(const Call& r, const void* save, const void* dlogits0, const void* dlogits1, const void* dtoken0, const void* dtoken1, void* dx, float* const dW[2],
             float* const db[2], float* dln_w, float* dln_b, void* stream) {
    const int B = r.B, Nt = r.Nt, D = r.D, chunks = cdiv(Nt, TOK), R = stream_rows(D, r.dtype), nth = R * (D / (r.dtype == DEVIAS_BF16 ? 8 : 4));
    hipStream_t st = (hipStream_t)stream;
    const Work w(r, save, stream);
    devias_range rg(r.who + 7);
    r.calls->fetch_add(1, std::memory_order_relaxed);
    // the heads: weight gradient, bias gradient, input gradient
    const void* dl[2] = {dlogits0, dlogits1};
    if (r.unified) {
        const int64_t n = (int64_t)B * r.C[0];
        dispatch_t(r.dtype, [&](auto tag) {
            using T = typename decltype(tag)::type;
            hipLaunchKernelGGL((head_stack_kernel<T>), dim3(cdiv(n, NT)), dim3(NT), 0, st, (const T*)dlogits0, (const T*)dlogits1, n, (T*)w.t.dl2);
        });
        CHECK_STAGE(r.who, "stack");
        dl[0] = w.t.dl2;
    }
    for (int i = 0; i < r.heads(); ++i) {
        Epi e;
        RUN(wgrad(w.c, dl[i], w.s.a + (int64_t)i * B * D * esize(r.dtype), dW[i], r.M(), r.C[i], D));
        RUN(colsum(w.c, dl[i], r.M(), r.C[i], db[i]));
        RUN(gemm(w.c, dl[i], r.W[i], w.t.da + (int64_t)i * B * D, r.M(), D, r.C[i], r.C[i], D, 0, 1, e, 1 /* fp32 output: da is not rounded to T */));
    }
    // LayerNorm backward per stacked row, then every row of dx
    const float scale = r.mean ? 1.0f / (float)Nt : 1.0f;
    dispatch_t(r.dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((head_ln_bwd_kernel<T>), dim3(r.rows()), dim3(NT), 0, st, w.t.da, (const T*)dtoken0, (const T*)dtoken1, r.mask[0], r.mask[1], w.s.xhat, w.s.rstd,
                           r.ln_w, B, D, scale, (T*)w.t.dxrow, w.t.pg, w.t.pb);
    });
    CHECK_STAGE(r.who, "layernorm");
    dispatch_t(r.dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        const auto kernel = r.mean ? head_dx_kernel<T, LIVE_ALL> : r.G == 2 ? head_dx_kernel<T, LIVE_FIRST_LAST> : head_dx_kernel<T, LIVE_FIRST>;
        hipLaunchKernelGGL(kernel, dim3(B * chunks), dim3(nth), 0, st, (const T*)w.t.dxrow, B, Nt, D, chunks, R, (T*)dx);
    });
    CHECK_STAGE(r.who, "dx");
    // d gamma / d beta: per-row partials summed over the rows in index order, ONE launch
    DeviasDeferList dl_; dl_.n = 0;
    dl_.jobs[dl_.n++] = DeviasReduceJob{w.t.pg, r.rows(), D, D, dln_w, 0.f};
    dl_.jobs[dl_.n++] = DeviasReduceJob{w.t.pb, r.rows(), D, D, dln_b, 0.f};
    RUN(devias_flush_deferred(&dl_, st));
    return DEVIAS_OK;
}

// ---- the two families' argument checks ------------------------------------------------------------------------------------------------------------------
int pool_check(const devias_pool_head_args* a, const char* who) {
    DEVIAS_REQUIRE(a, "%s: null args", who);
    REQUIRE_STRUCT_SIZE(a, devias_pool_head_args, who);
    DEVIAS_REQUIRE(dtype_ok(a->dtype), "%s: bad dtype %d", who, a->dtype);
    DEVIAS_REQUIRE(a->pool == DEVIAS_POOL_MEAN || a->pool == DEVIAS_POOL_CLS, "%s: bad pool %d (DEVIAS_POOL_MEAN or DEVIAS_POOL_CLS)", who, a->pool);
    if (!dims_supported(1, a->B, a->Nt, a->D, a->C, a->C))
        return devias_set_error(DEVIAS_EUNSUPPORTED, "%s: unsupported dims B=%d Nt=%d D=%d C=%d (D in {384, 768, 1024}, B >= 1, Nt >= 1, B Nt < 2^31, C >= 2)", who, a->B, a->Nt,
                                a->D, a->C);
    DEVIAS_REQUIRE(a->eps > 0.f, "%s: eps must be positive", who);
    DEVIAS_REQUIRE(a->W && a->bias && a->ln_w && a->ln_b, "%s: null parameter", who);
    DEVIAS_REQUIRE(aligned16(a->W) && aligned16(a->bias), "%s: W / bias must be 16-byte aligned", who);
    DEVIAS_REQUIRE(a->ws && aligned16(a->ws), "%s: ws must be 16-byte aligned, non-null", who);
    DEVIAS_REQUIRE(a->ws_bytes >= devias_pool_head_workspace_bytes(a->B, a->Nt, a->D, a->C, a->dtype), "%s: workspace too small", who);
    return DEVIAS_OK;
}
Call pool_call(const devias_pool_head_args* a, const char* who) {
    return Call{who, &g_pool_head_calls, a->dtype, a->B, a->Nt, a->D, 1, a->pool == DEVIAS_POOL_MEAN, 0, a->eps, a->ln_w, a->ln_b, a->ws,
                {a->drop_mask, nullptr}, {a->C, 0}, {a->W, nullptr}, {a->bias, nullptr}};
}

int tt_check(const devias_two_token_head_args* a, const char* who) {
    DEVIAS_REQUIRE(a, "%s: null args", who);
    REQUIRE_STRUCT_SIZE(a, devias_two_token_head_args, who);
    DEVIAS_REQUIRE(dtype_ok(a->dtype), "%s: bad dtype %d", who, a->dtype);
    DEVIAS_REQUIRE(a->unified == 0 || a->unified == 1, "%s: unified must be 0 or 1, got %d", who, a->unified);
    if (!dims_supported(2, a->B, a->Nt, a->D, a->Ca, a->Cs))
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
Call tt_call(const devias_two_token_head_args* a, const char* who) {
    return Call{who, &g_two_token_head_calls, a->dtype, a->B, a->Nt, a->D, 2, 0, a->unified, a->eps, a->ln_w, a->ln_b, a->ws,
                {a->mask_a, a->mask_s}, {a->Ca, a->Cs}, {a->Wa, a->Ws}, {a->ba, a->bs}};
}

}  // namespace

extern "C" int64_t devias_pool_head_workspace_bytes(int32_t B, int32_t Nt, int32_t D, int32_t C, int32_t dtype) {
    if (!dims_supported(1, B, Nt, D, C, C) || !dtype_ok(dtype)) return 0;
    return kernel_ws_bytes(B, D, C, dtype) + Tmp(Arena(nullptr), 1, B, Nt, D, C, dtype).bytes;
}
extern "C" int64_t devias_two_token_head_workspace_bytes(int32_t B, int32_t Nt, int32_t D, int32_t Ca, int32_t Cs, int32_t unified, int32_t dtype) {
    if (!dims_supported(2, B, Nt, D, Ca, Cs) || !dtype_ok(dtype) || (unified && Ca != Cs)) return 0;
    const int C = Ca > Cs ? Ca : Cs;
    return kernel_ws_bytes(unified ? 2 * B : B, D, C, dtype) + Tmp(Arena(nullptr), 2, B, Nt, D, C, dtype).bytes;
}
static int64_t save_bytes(int G, int B, int D, int dtype) {
    if (!dims_supported(G, B, G, D, 2, 2) || !dtype_ok(dtype)) return 0;
    Arena ar(nullptr);
    Save(ar, (int64_t)G * B, D, dtype);          // (carved at address 0: the arena ends at its size)
    return ar.off;
}
extern "C" int64_t devias_pool_head_save_bytes(int32_t B, int32_t D, int32_t dtype) { return save_bytes(1, B, D, dtype); }
extern "C" int64_t devias_two_token_head_save_bytes(int32_t B, int32_t D, int32_t dtype) { return save_bytes(2, B, D, dtype); }

extern "C" int devias_pool_head_fwd(const devias_pool_head_args* a, const void* h, void* token, void* logits, void* save, void* stream) {
    const char* who = "devias_pool_head_fwd";
    RUN(pool_check(a, who));
    DEVIAS_REQUIRE(h && token && logits && aligned16(h) && aligned16(token) && aligned16(logits), "%s: h / token / logits must be non-null, 16-byte aligned", who);
    DEVIAS_REQUIRE(!save || aligned16(save), "%s: save must be 16-byte aligned", who);
    void* const tokens[2] = {token, nullptr};
    void* const out[2] = {logits, nullptr};
    return head_fwd(pool_call(a, who), h, tokens, out, save, stream);
}

extern "C" int devias_pool_head_bwd(const devias_pool_head_args* a, const void* save, const void* dlogits, const void* dtoken, void* dx, const devias_pool_head_grads* g,
                                    void* stream) {
    const char* who = "devias_pool_head_bwd";
    RUN(pool_check(a, who));
    DEVIAS_REQUIRE(save && dlogits && dx && g && aligned16(save) && aligned16(dx), "%s: null pointer (save / dlogits / dx / grads), or save / dx not 16-byte aligned", who);
    REQUIRE_STRUCT_SIZE(g, devias_pool_head_grads, who);
    DEVIAS_REQUIRE(g->dW && g->db && g->dln_w && g->dln_b, "%s: null gradient destination", who);
    float* const dW[2] = {g->dW, nullptr};
    float* const db[2] = {g->db, nullptr};
    return head_bwd(pool_call(a, who), save, dlogits, nullptr, dtoken, nullptr, dx, dW, db, g->dln_w, g->dln_b, stream);
}

extern "C" int devias_two_token_head_fwd(const devias_two_token_head_args* a, const void* h, void* token_a, void* token_s, void* logits_a, void* logits_s, void* save,
                                         void* stream) {
    const char* who = "devias_two_token_head_fwd";
    RUN(tt_check(a, who));
    DEVIAS_REQUIRE(h && token_a && token_s && logits_a && aligned16(h) && aligned16(token_a) && aligned16(token_s) && aligned16(logits_a),
                   "%s: h / token_a / token_s / logits_a must be non-null, 16-byte aligned", who);
    DEVIAS_REQUIRE(a->unified || (logits_s && aligned16(logits_s)), "%s: logits_s must be non-null, 16-byte aligned (separate heads)", who);
    DEVIAS_REQUIRE(!save || aligned16(save), "%s: save must be 16-byte aligned", who);
    void* const tokens[2] = {token_a, token_s};
    void* const out[2] = {logits_a, logits_s};
    return head_fwd(tt_call(a, who), h, tokens, out, save, stream);
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
    float* const dW[2] = {g->dWa, g->dWs};
    float* const db[2] = {g->dba, g->dbs};
    return head_bwd(tt_call(a, who), save, dlogits_a, dlogits_s, dtoken_a, dtoken_s, dx, dW, db, g->dln_w, g->dln_b, stream);
}
