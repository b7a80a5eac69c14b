// Folded form (devias_slotf_*): the K and V projections are never materialised.
//   sim[i,j] = scale * q_i . (Wk c_j) = scale * (Wk^T q_i) . c_j = scale * q'_i . c_j            q' = LN(x_s) (Wk_h^T Wq_h)^T   [B, S, h, D]
//   o_i      = sum_j Abar[i,j] (Wv c_j) = Wv (sum_j Abar[i,j] c_j) = Wv z_i                      z  = sum_j Abar[i,j] c_j       [B, S, h, D]
// (per head h; c = LayerNorm_ctx(features), D = embed dim).  Same arithmetic up to the association order of the sums; what changes is
// the stream: every layer reads the D-wide context rows c (B*N*D elements, shared by the heads) instead of the 2*h*512-wide K|V rows,
// and the [M, D] x [D, 2*h*512] projection GEMM with its dgrad and wgrad disappears -- the composite weights are D x D per head.
// Kernel structure as in slot_unfolded.hip: a wave owns one token at a time, each lane EPL = D / 64 consecutive context dims, per-workgroup partials
// reduced by a small finish kernel in a fixed order.  MAXS <= 4 (register budget); D in {384, 512, 768, 1024}.  The finish kernels also serve slot_mfma.hip.
#include "slot_common.h"

namespace {
template <typename T, int EPL> __device__ __forceinline__ void loadE(const T* p, float (&v)[EPL]);
template <int EPL> __device__ __forceinline__ void loadE_bf16(const bf16* p, float (&v)[EPL]) {
    if constexpr (EPL % 8 == 0) {
#pragma unroll
        for (int u = 0; u < EPL / 8; ++u) {
            bf16x8 x = *reinterpret_cast<const bf16x8*>(p + 8 * u);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[8 * u + e] = (float)x[e];
        }
    } else if constexpr (EPL % 4 == 0) {
#pragma unroll
        for (int u = 0; u < EPL / 4; ++u) {
            bf16x4 x = *reinterpret_cast<const bf16x4*>(p + 4 * u);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * u + e] = (float)x[e];
        }
    } else {
#pragma unroll
        for (int u = 0; u < EPL / 2; ++u) {
            bf16x2 x = *reinterpret_cast<const bf16x2*>(p + 2 * u);
            v[2 * u] = (float)x[0]; v[2 * u + 1] = (float)x[1];
        }
    }
}
template <int EPL> __device__ __forceinline__ void loadE_f32(const float* p, float (&v)[EPL]) {
    if constexpr (EPL % 4 == 0) {
#pragma unroll
        for (int u = 0; u < EPL / 4; ++u) {
            f32x4 x = *reinterpret_cast<const f32x4*>(p + 4 * u);
            v[4 * u] = x[0]; v[4 * u + 1] = x[1]; v[4 * u + 2] = x[2]; v[4 * u + 3] = x[3];
        }
    } else {
#pragma unroll
        for (int u = 0; u < EPL / 2; ++u) {
            f32x2 x = *reinterpret_cast<const f32x2*>(p + 2 * u);
            v[2 * u] = x[0]; v[2 * u + 1] = x[1];
        }
    }
}
template <typename T, int EPL> struct LoadE;
template <int EPL> struct LoadE<bf16, EPL> { static __device__ __forceinline__ void run(const bf16* p, float (&v)[EPL]) { loadE_bf16<EPL>(p, v); } };
template <int EPL> struct LoadE<float, EPL> { static __device__ __forceinline__ void run(const float* p, float (&v)[EPL]) { loadE_f32<EPL>(p, v); } };

template <typename T, int MAXS, int EPL>
__global__ __launch_bounds__(256) void slotf_fwd_kernel(const T* __restrict__ qp, const T* __restrict__ ctx, float* __restrict__ attn,
                                                        float* __restrict__ ws_r, float* __restrict__ ws_z, int S, int N, int h, float scale) {
    constexpr int D = 64 * EPL;
    __shared__ __attribute__((aligned(16))) float sm_z[3][MAXS][D];
    __shared__ float sm_r[3][MAXS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bh = blockIdx.y, b = bh / h, hh = bh % h, chunk = blockIdx.x, nchunks = gridDim.x;
    float qv[MAXS][EPL], zacc[MAXS][EPL], rs[MAXS];
#pragma unroll
    for (int i = 0; i < MAXS; ++i) {
        if (i < S) LoadE<T, EPL>::run(qp + ((int64_t)b * S + i) * h * D + hh * D + lane * EPL, qv[i]);
#pragma unroll
        for (int e = 0; e < EPL; ++e) { if (i >= S) qv[i][e] = 0.f; zacc[i][e] = 0.f; }
        rs[i] = 0.f;
    }
    const int j0 = chunk * TCH, j1 = min(N, j0 + TCH);
    for (int jj = j0 + wave * 2; jj < j1; jj += 8) {               // two tokens per wave iteration
        const int ntok = min(2, j1 - jj);
        float c8[2][EPL];
#pragma unroll
        for (int u = 0; u < 2; ++u) LoadE<T, EPL>::run(ctx + ((int64_t)b * N + min(jj + u, j1 - 1)) * D + lane * EPL, c8[u]);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u >= ntok) break;
            const int j = jj + u;
            float sim[MAXS];
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < MAXS; ++i) {
                if (i < S) {
                    float d = 0.f;
#pragma unroll
                    for (int e = 0; e < EPL; ++e) d += qv[i][e] * c8[u][e];
                    sim[i] = wave_sum(d) * scale;
                    mx = fmaxf(mx, sim[i]);
                }
            }
            float den = 0.f;
#pragma unroll
            for (int i = 0; i < MAXS; ++i) if (i < S) { sim[i] = expf(sim[i] - mx); den += sim[i]; }
            const float inv = 1.0f / den;
#pragma unroll
            for (int i = 0; i < MAXS; ++i) {
                if (i < S) {
                    const float a = sim[i] * inv;
                    if (lane == 0) attn[((int64_t)bh * S + i) * N + j] = a;
                    rs[i] += a;
#pragma unroll
                    for (int e = 0; e < EPL; ++e) zacc[i][e] += a * c8[u][e];
                }
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < MAXS; ++i) if (i < S) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) sm_z[wave - 1][i][lane * EPL + e] = zacc[i][e];
            if (lane == 0) sm_r[wave - 1][i] = rs[i];
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int64_t pb = (int64_t)bh * nchunks + chunk;
#pragma unroll
        for (int i = 0; i < MAXS; ++i) if (i < S) {
            float r = rs[i];
#pragma unroll
            for (int w = 0; w < 3; ++w) r += sm_r[w][i];
            if (lane == 0) ws_r[pb * S + i] = r;
            float* dst = ws_z + (pb * S + i) * D + lane * EPL;
#pragma unroll
            for (int e = 0; e < EPL; ++e)
                dst[e] = zacc[i][e] + sm_z[0][i][lane * EPL + e] + sm_z[1][i][lane * EPL + e] + sm_z[2][i][lane * EPL + e];
        }
    }
}

// sum of n values `stride` floats apart, added in index order with eight loads in flight (a chain of n dependent load latencies otherwise: these finish kernels are all latency)
__device__ __forceinline__ float sum_strided8(const float* __restrict__ p, int n, int64_t stride) {
    float s = 0.f;
    int c = 0;
    for (; c + 7 < n; c += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(c + u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < n; ++c) s += p[(int64_t)c * stride];
    return s;
}

// finish: rsum[bh,i] = sum_chunks ws_r + 1e-7 ; z[b,i,hh*D+d] = sum_chunks ws_z / rsum.  (bf16 path: launched with one thread per column -- with 256 threads a
// thread summed D / 256 columns one after the other, each a round trip to memory: 8.0 -> see DESIGN.md section 5 round 5)
template <typename T>
__global__ void slotf_fwd_finish_kernel(const float* __restrict__ ws_r, const float* __restrict__ ws_z, float* __restrict__ rsum,
                                        T* __restrict__ z, int S, int h, int D, int nchunks) {
    const int bh = blockIdx.x / S, i = blockIdx.x % S, b = bh / h, hh = bh % h;
    float r = sum_strided8(ws_r + (int64_t)bh * nchunks * S + i, nchunks, S);
    r += 1e-7f;
    if (threadIdx.x == 0) rsum[(int64_t)bh * S + i] = r;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const float s = sum_strided8(ws_z + ((int64_t)bh * nchunks * S + i) * D + d, nchunks, (int64_t)S * D);
        z[((int64_t)b * S + i) * h * D + hh * D + d] = from_f32<T>(s / r);
    }
}

// backward of one layer: ds[bh,i,j] and per-chunk dq' partials.  delta_i = dz_i . z_i (= dO_i . o_i of the unfolded form)
template <typename T, int MAXS, int EPL>
__global__ __launch_bounds__(256) void slotf_bwd_kernel(const T* __restrict__ ctx, const float* __restrict__ attn, const float* __restrict__ rsum,
                                                        const T* __restrict__ z, const T* __restrict__ dz, const float* __restrict__ dA_ext,
                                                        float* __restrict__ ds_out, float* __restrict__ ws_q, int S, int N, int h, float scale) {
    constexpr int D = 64 * EPL;
    __shared__ __attribute__((aligned(16))) float sm_q[3][MAXS][D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bh = blockIdx.y, b = bh / h, hh = bh % h, chunk = blockIdx.x, nchunks = gridDim.x;
    float dzv[MAXS][EPL], dq[MAXS][EPL], dl[MAXS], rinv[MAXS];
#pragma unroll
    for (int i = 0; i < MAXS; ++i) {
        dl[i] = 0.f; rinv[i] = 0.f;
        if (i < S) {
            float zv[EPL];
            const int64_t off = ((int64_t)b * S + i) * h * D + hh * D + lane * EPL;
            LoadE<T, EPL>::run(dz + off, dzv[i]);
            LoadE<T, EPL>::run(z + off, zv);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < EPL; ++e) d += dzv[i][e] * zv[e];
            dl[i] = wave_sum(d);
            rinv[i] = 1.0f / rsum[(int64_t)bh * S + i];
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) { if (i >= S) dzv[i][e] = 0.f; dq[i][e] = 0.f; }
    }
    const int j0 = chunk * TCH, j1 = min(N, j0 + TCH);
    for (int jj = j0 + wave * 2; jj < j1; jj += 8) {
        const int ntok = min(2, j1 - jj);
        float c8[2][EPL];
#pragma unroll
        for (int u = 0; u < 2; ++u) LoadE<T, EPL>::run(ctx + ((int64_t)b * N + min(jj + u, j1 - 1)) * D + lane * EPL, c8[u]);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (u >= ntok) break;
            const int j = jj + u;
            float a[MAXS], dA[MAXS];
            float tsum = 0.f;
#pragma unroll
            for (int i = 0; i < MAXS; ++i) {
                if (i < S) {
                    float d = 0.f;
#pragma unroll
                    for (int e = 0; e < EPL; ++e) d += dzv[i][e] * c8[u][e];
                    const float dAbar = wave_sum(d);
                    a[i] = attn[((int64_t)bh * S + i) * N + j];
                    dA[i] = (dAbar - dl[i]) * rinv[i] + (dA_ext ? dA_ext[((int64_t)bh * S + i) * N + j] : 0.f);
                    tsum += a[i] * dA[i];
                }
            }
#pragma unroll
            for (int i = 0; i < MAXS; ++i) {
                if (i < S) {
                    const float ds = a[i] * (dA[i] - tsum);
                    if (lane == 0) ds_out[((int64_t)bh * S + i) * N + j] = ds;
                    const float w = ds * scale;
#pragma unroll
                    for (int e = 0; e < EPL; ++e) dq[i][e] += w * c8[u][e];
                }
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < MAXS; ++i) if (i < S) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) sm_q[wave - 1][i][lane * EPL + e] = dq[i][e];
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int64_t pb = (int64_t)bh * nchunks + chunk;
#pragma unroll
        for (int i = 0; i < MAXS; ++i) if (i < S) {
            float* dst = ws_q + (pb * S + i) * D + lane * EPL;
#pragma unroll
            for (int e = 0; e < EPL; ++e)
                dst[e] = dq[i][e] + sm_q[0][i][lane * EPL + e] + sm_q[1][i][lane * EPL + e] + sm_q[2][i][lane * EPL + e];
        }
    }
}

template <typename T>
__global__ void slotf_bwd_finish_kernel(const float* __restrict__ ws_q, T* __restrict__ dqp, int S, int h, int D, int nchunks) {
    const int bh = blockIdx.x / S, i = blockIdx.x % S, b = bh / h, hh = bh % h;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const float s = sum_strided8(ws_q + ((int64_t)bh * nchunks * S + i) * D + d, nchunks, (int64_t)S * D);
        dqp[((int64_t)b * S + i) * h * D + hh * D + d] = from_f32<T>(s);
    }
}

// Operands of the deferred context gradient of L stacked layers that share the context rows:
//   dc[b, j, :] = sum over k = (l, w, hh, i) of coef[b][k][j] * vec[b][k][:]
//     w = 0: coef = A_l[i,j] / rsum_l[i]   vec = dz_l[b,i,hh,:]        (from z = sum_j Abar c_j)
//     w = 1: coef = scale * ds_l[i,j]      vec = q'_l[b,i,hh,:]        (from sim = scale q' . c_j)
// i.e. one [N, K] x [K, D] product per clip (K = 2 L h S), run as a batched GEMM by the caller.  coef rows are padded to Np tokens (zeros).
template <typename T>
__global__ __launch_bounds__(256) void slotf_pack_kernel(const float* __restrict__ attn_stack, const float* __restrict__ rsum_stack,
                                                         const float* __restrict__ ds_stack, const T* __restrict__ dz_stack,
                                                         const T* __restrict__ qp_stack, T* __restrict__ coef, T* __restrict__ vec,
                                                         int L, int B, int S, int N, int Np, int h, int D, float scale) {
    const int K = 2 * L * h * S;
    const int b = blockIdx.y, k = blockIdx.x;
    const int i = k % S, hh = (k / S) % h, w = (k / (S * h)) % 2, l = k / (2 * S * h);
    const int64_t row = ((int64_t)l * B * h + (int64_t)b * h + hh) * S + i;         // row of the [L, B*h, S, N] stacks
    T* crow = coef + ((int64_t)b * K + k) * Np;
    if (w == 0) {
        const float rinv = 1.0f / rsum_stack[row];
        for (int j = threadIdx.x; j < Np; j += 256) crow[j] = from_f32<T>(j < N ? attn_stack[row * N + j] * rinv : 0.f);
    } else {
        for (int j = threadIdx.x; j < Np; j += 256) crow[j] = from_f32<T>(j < N ? ds_stack[row * N + j] * scale : 0.f);
    }
    const T* src = (w == 0 ? dz_stack : qp_stack) + (((int64_t)l * B + b) * S + i) * h * D + (int64_t)hh * D;
    T* vrow = vec + ((int64_t)b * K + k) * D;
    for (int d = threadIdx.x; d < D; d += 256) vrow[d] = src[d];
}

// ---- host side.  D -> EPL = D / 64 (the entry points admit 384, 512, 768, 1024) and S -> the register form MAXS (2, 4): each ladder once per kernel
template <typename T, int MAXS> auto slotf_fwd_by_d(int D) {
    return D == 384 ? slotf_fwd_kernel<T, MAXS, 6> : D == 512 ? slotf_fwd_kernel<T, MAXS, 8> : D == 768 ? slotf_fwd_kernel<T, MAXS, 12> : slotf_fwd_kernel<T, MAXS, 16>;
}
template <typename T, int MAXS> auto slotf_bwd_by_d(int D) {
    return D == 384 ? slotf_bwd_kernel<T, MAXS, 6> : D == 512 ? slotf_bwd_kernel<T, MAXS, 8> : D == 768 ? slotf_bwd_kernel<T, MAXS, 12> : slotf_bwd_kernel<T, MAXS, 16>;
}
template <typename T> auto slotf_fwd_of(int S, int D) { return S <= 2 ? slotf_fwd_by_d<T, 2>(D) : slotf_fwd_by_d<T, 4>(D); }
template <typename T> auto slotf_bwd_of(int S, int D) { return S <= 2 ? slotf_bwd_by_d<T, 2>(D) : slotf_bwd_by_d<T, 4>(D); }
inline dim3 finish_block(const SlotP& p) { return dim3(p.dtype == DEVIAS_BF16 ? (p.D + 63) / 64 * 64 : 256); }   // bf16: one thread per column (see slotf_fwd_finish_kernel)
}  // namespace

void launch_slotf_fwd(const SlotP& p) {
    by_dtype(p.dtype, [&](auto t) { using T = decltype(t);
        hipLaunchKernelGGL(slotf_fwd_of<T>(p.S, p.D), dim3(p.nchunks, p.B * p.h), dim3(256), 0, p.st, (const T*)p.q, (const T*)p.src, p.attn, p.ws_r, p.ws_w, p.S, p.N, p.h, p.scale); });
}
void launch_slotf_bwd(const SlotP& p) {
    by_dtype(p.dtype, [&](auto t) { using T = decltype(t);
        hipLaunchKernelGGL(slotf_bwd_of<T>(p.S, p.D), dim3(p.nchunks, p.B * p.h), dim3(256), 0, p.st, (const T*)p.src, p.attn, p.rsum, (const T*)p.out, (const T*)p.d_out, p.dA_ext,
                           p.ds, p.ws_w, p.S, p.N, p.h, p.scale); });
}
void launch_slotf_fwd_finish(const SlotP& p) {
    by_dtype(p.dtype, [&](auto t) { using T = decltype(t);
        hipLaunchKernelGGL((slotf_fwd_finish_kernel<T>), dim3(p.B * p.h * p.S), finish_block(p), 0, p.st, p.ws_r, p.ws_w, p.rsum, (T*)p.out, p.S, p.h, p.D, p.nchunks); });
}
void launch_slotf_bwd_finish(const SlotP& p) {
    by_dtype(p.dtype, [&](auto t) { using T = decltype(t);
        hipLaunchKernelGGL((slotf_bwd_finish_kernel<T>), dim3(p.B * p.h * p.S), finish_block(p), 0, p.st, p.ws_w, (T*)p.dq, p.S, p.h, p.D, p.nchunks); });
}
void launch_slotf_pack(int dtype, const float* attn_stack, const float* rsum_stack, const float* ds_stack, const void* dz_stack, const void* qp_stack, void* coef, void* vec,
                       int L, int B, int S, int N, int Np, int h, int D, float scale, hipStream_t st) {
    by_dtype(dtype, [&](auto t) { using T = decltype(t);
        hipLaunchKernelGGL((slotf_pack_kernel<T>), dim3(2 * L * h * S, B), dim3(256), 0, st, attn_stack, rsum_stack, ds_stack, (const T*)dz_stack, (const T*)qp_stack, (T*)coef,
                           (T*)vec, L, B, S, N, Np, h, D, scale); });
}
