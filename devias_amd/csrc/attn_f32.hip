// Attention in fp32 (parity mode; the layout of the attention units: attn_common.h): straightforward VALU kernels, exact fp32 -- forward and dQ with one thread per
// query, dK / dV with two threads per key -- on the plain (block-in-head, head, batch) grid, and their host launchers.
#include "attn_common.h"

using namespace attn_units;

namespace {

// ======================================= fp32 parity kernels ==============================================
// forward: 128 threads, one query per thread (q and o in registers), K/V tiles of 32 keys broadcast from LDS
template <bool DROP = false>
__global__ __launch_bounds__(128) void mhsa_fwd_f32_kernel(const float* __restrict__ qkv, float* __restrict__ o,
                                                           float* __restrict__ lse, int N, int H, float scale, DropP drop = DropP{}) {
    __shared__ __attribute__((aligned(16))) float sk[32][64];
    __shared__ __attribute__((aligned(16))) float sv[32][64];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int D = H * 64;
    const int64_t RS = 3 * (int64_t)D;
    const float* base = qkv + (int64_t)b * N * RS + h * 64;
    const int q = blockIdx.x * 128 + tid;
    const int qc = min(q, N - 1);
    float qr[64], acc[64];
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
        f32x4 v = *reinterpret_cast<const f32x4*>(base + (int64_t)qc * RS + d);
        qr[d] = v[0] * scale; qr[d + 1] = v[1] * scale; qr[d + 2] = v[2] * scale; qr[d + 3] = v[3] * scale;
        acc[d] = acc[d + 1] = acc[d + 2] = acc[d + 3] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    const uint32_t rowkey = DROP ? drop_rowkey(drop, (uint32_t)(b * H + h), (uint32_t)qc) : 0u;
    for (int k0 = 0; k0 < N; k0 += 32) {
        __syncthreads();
        for (int i = tid; i < 32 * 16; i += 128) {
            int r = i >> 4, ch = (i & 15) * 4;
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            bool ok = k0 + r < N;
            *reinterpret_cast<f32x4*>(&sk[r][ch]) = ok ? *reinterpret_cast<const f32x4*>(base + D + (int64_t)(k0 + r) * RS + ch) : z;
            *reinterpret_cast<f32x4*>(&sv[r][ch]) = ok ? *reinterpret_cast<const f32x4*>(base + 2 * D + (int64_t)(k0 + r) * RS + ch) : z;
        }
        __syncthreads();
        const int nk = min(32, N - k0);
        for (int j = 0; j < nk; ++j) {
            float s = 0.f;
#pragma unroll
            for (int d = 0; d < 64; ++d) s += qr[d] * sk[j][d];
            const float mn = fmaxf(m, s);
            const float alpha = expf(m - mn), p = expf(s - mn);
            m = mn;
            l = l * alpha + p;
            const float pd = DROP ? p * drop_scale(drop, rowkey, (uint32_t)(k0 + j)) : p;
#pragma unroll
            for (int d = 0; d < 64; ++d) acc[d] = acc[d] * alpha + pd * sv[j][d];
        }
    }
    if (q < N) {
        const float inv = 1.0f / l;
        float* orow = o + ((int64_t)b * N + q) * D + h * 64;
#pragma unroll
        for (int d = 0; d < 64; d += 4) {
            f32x4 v = {acc[d] * inv, acc[d + 1] * inv, acc[d + 2] * inv, acc[d + 3] * inv};
            *reinterpret_cast<f32x4*>(orow + d) = v;
        }
        lse[((int64_t)b * H + h) * N + q] = m + logf(l);
    }
}

// backward dQ (+ delta): one query per thread
template <bool DROP = false>
__global__ __launch_bounds__(128) void mhsa_bwd_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                              const float* __restrict__ d_o, const float* __restrict__ lse,
                                                              float* __restrict__ delta, float* __restrict__ dqkv,
                                                              int N, int H, float scale, DropP drop = DropP{}) {
    __shared__ __attribute__((aligned(16))) float sk[32][64];
    __shared__ __attribute__((aligned(16))) float sv[32][64];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int D = H * 64;
    const int64_t RS = 3 * (int64_t)D;
    const float* base = qkv + (int64_t)b * N * RS + h * 64;
    const int q = blockIdx.x * 128 + tid;
    const int qc = min(q, N - 1);
    float qr[64], dor[64], dq[64];
    float dl = 0.f;
    const float* orow = o + ((int64_t)b * N + qc) * D + h * 64;
    const float* dorow = d_o + ((int64_t)b * N + qc) * D + h * 64;
#pragma unroll
    for (int d = 0; d < 64; ++d) {
        qr[d] = base[(int64_t)qc * RS + d];
        dor[d] = dorow[d];
        dl += dor[d] * orow[d];
        dq[d] = 0.f;
    }
    const float ls = lse[((int64_t)b * H + h) * N + qc];
    const uint32_t rowkey = DROP ? drop_rowkey(drop, (uint32_t)(b * H + h), (uint32_t)qc) : 0u;
    if (q < N) delta[((int64_t)b * H + h) * N + q] = dl;
    for (int k0 = 0; k0 < N; k0 += 32) {
        __syncthreads();
        for (int i = tid; i < 32 * 16; i += 128) {
            int r = i >> 4, ch = (i & 15) * 4;
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            bool ok = k0 + r < N;
            *reinterpret_cast<f32x4*>(&sk[r][ch]) = ok ? *reinterpret_cast<const f32x4*>(base + D + (int64_t)(k0 + r) * RS + ch) : z;
            *reinterpret_cast<f32x4*>(&sv[r][ch]) = ok ? *reinterpret_cast<const f32x4*>(base + 2 * D + (int64_t)(k0 + r) * RS + ch) : z;
        }
        __syncthreads();
        const int nk = min(32, N - k0);
        for (int j = 0; j < nk; ++j) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < 64; ++d) { s += qr[d] * sk[j][d]; dp += dor[d] * sv[j][d]; }
            const float p = expf(s * scale - ls);
            if constexpr (DROP) dp *= drop_scale(drop, rowkey, (uint32_t)(k0 + j));
            const float ds = p * (dp - dl) * scale;
#pragma unroll
            for (int d = 0; d < 64; ++d) dq[d] += ds * sk[j][d];
        }
    }
    if (q < N) {
        float* row = dqkv + ((int64_t)b * N + q) * RS + h * 64;
#pragma unroll
        for (int d = 0; d < 64; ++d) row[d] = dq[d];
    }
}

// backward dK/dV: two threads per key (each owns 32 of the 64 head dims); 128 threads = 64 keys per workgroup
template <bool DROP = false>
__global__ __launch_bounds__(128) void mhsa_bwd_dkdv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ d_o,
                                                                const float* __restrict__ lse, const float* __restrict__ delta,
                                                                float* __restrict__ dqkv, int N, int H, float scale, DropP drop = DropP{}) {
    __shared__ __attribute__((aligned(16))) float sq[32][64];
    __shared__ __attribute__((aligned(16))) float sdo[32][64];
    __shared__ float sl[32], sd[32];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int D = H * 64;
    const int64_t RS = 3 * (int64_t)D;
    const float* base = qkv + (int64_t)b * N * RS + h * 64;
    const float* dobase = d_o + (int64_t)b * N * D + h * 64;
    const int key = blockIdx.x * 64 + (tid >> 1);
    const int half = (tid & 1) * 32;
    const int kc = min(key, N - 1);
    float kr[32], vr[32], dk[32], dv[32];
#pragma unroll
    for (int d = 0; d < 32; ++d) {
        kr[d] = base[D + (int64_t)kc * RS + half + d];
        vr[d] = base[2 * D + (int64_t)kc * RS + half + d];
        dk[d] = 0.f; dv[d] = 0.f;
    }
    for (int q0 = 0; q0 < N; q0 += 32) {
        __syncthreads();
        for (int i = tid; i < 32 * 16; i += 128) {
            int r = i >> 4, ch = (i & 15) * 4;
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            bool ok = q0 + r < N;
            *reinterpret_cast<f32x4*>(&sq[r][ch]) = ok ? *reinterpret_cast<const f32x4*>(base + (int64_t)(q0 + r) * RS + ch) : z;
            *reinterpret_cast<f32x4*>(&sdo[r][ch]) = ok ? *reinterpret_cast<const f32x4*>(dobase + (int64_t)(q0 + r) * D + ch) : z;
        }
        if (tid < 32) {
            bool ok = q0 + tid < N;
            sl[tid] = ok ? lse[((int64_t)b * H + h) * N + q0 + tid] : INFINITY;
            sd[tid] = ok ? delta[((int64_t)b * H + h) * N + q0 + tid] : 0.f;
        }
        __syncthreads();
        const int nq = min(32, N - q0);
        for (int i = 0; i < nq; ++i) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < 32; ++d) { s += sq[i][half + d] * kr[d]; dp += sdo[i][half + d] * vr[d]; }
            s += __shfl_xor(s, 1, 64);
            dp += __shfl_xor(dp, 1, 64);
            const float p = expf(s * scale - sl[i]);
            float pd = p;
            if constexpr (DROP) {
                const float mk = drop_scale(drop, drop_rowkey(drop, (uint32_t)(b * H + h), (uint32_t)(q0 + i)), (uint32_t)kc);
                dp *= mk; pd = p * mk;
            }
            const float ds = p * (dp - sd[i]) * scale;
#pragma unroll
            for (int d = 0; d < 32; ++d) { dv[d] += pd * sdo[i][half + d]; dk[d] += ds * sq[i][half + d]; }
        }
    }
    if (key < N) {
        float* row = dqkv + ((int64_t)b * N + key) * RS + h * 64 + half;
#pragma unroll
        for (int d = 0; d < 32; ++d) { row[D + d] = dk[d]; row[2 * D + d] = dv[d]; }
    }
}

}  // namespace

namespace attn_units {

// (`per` queries resp. keys of one (batch, head) per workgroup of 128 threads; always the plain 3-D grid)
#define F32_LAUNCH(kernel, per, ...) do { const dim3 grid(cdiv(p.N, per), p.H, p.B);                                              \
        if (p.drop) hipLaunchKernelGGL(kernel<true>, grid, dim3(128), 0, p.st, __VA_ARGS__, p.N, p.H, p.scale, p.dp);            \
        else hipLaunchKernelGGL(kernel<false>, grid, dim3(128), 0, p.st, __VA_ARGS__, p.N, p.H, p.scale, p.dp); } while (0)
void launch_attn_fwd_f32(const AttnP& p) { F32_LAUNCH(mhsa_fwd_f32_kernel, 128, (const float*)p.qkv, (float*)p.o, p.lse); }
void launch_attn_bwd_dq_f32(const AttnP& p) {
    F32_LAUNCH(mhsa_bwd_dq_f32_kernel, 128, (const float*)p.qkv, (const float*)p.o, (const float*)p.d_o, p.lse, p.delta, (float*)p.dqkv);
}
void launch_attn_bwd_dkdv_f32(const AttnP& p) {      // (two threads per key: 64 keys per workgroup)
    F32_LAUNCH(mhsa_bwd_dkdv_f32_kernel, 64, (const float*)p.qkv, (const float*)p.d_o, p.lse, p.delta, (float*)p.dqkv);
}
#undef F32_LAUNCH

}  // namespace attn_units
