// Device helpers of the one-workgroup-per-row kernels (loss.hip, fusion_head.hip, token_head.hip, distill.hip): 256 threads = 4 waves per row, every statistic an fp32 block
// reduction (DPP wave reduction of common.h + a 4-wave LDS combine in the fixed order sm[0] + sm[1] + sm[2] + sm[3]: results are bitwise equal run to run).
// Every unit that includes this file gets its own copy (anonymous namespace).
#pragma once
#include "common.h"

namespace {

enum { NT = 256, EPT = 4 };          // threads per workgroup; elements per thread of a row held in registers (D <= 1024)

// ---- block reductions: every thread of the workgroup calls them, every thread gets the result; `sm` may be reused right after --------------------------
__device__ __forceinline__ float block_sum(float v, float* sm /*[4]*/) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return sm[0] + sm[1] + sm[2] + sm[3];
}
// two sums with one pair of barriers
__device__ __forceinline__ void block_sum2(float& a, float& b, float* sm /*[8]*/) {
    a = wave_sum(a); b = wave_sum(b);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = a; sm[4 + (threadIdx.x >> 6)] = b; }
    __syncthreads();
    a = sm[0] + sm[1] + sm[2] + sm[3];
    b = sm[4] + sm[5] + sm[6] + sm[7];
}
__device__ __forceinline__ float block_max(float v, float* sm /*[4]*/) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// row softmax statistics of z[0..C): max and logsumexp
template <typename T>
__device__ __forceinline__ void row_stats(const T* z, int C, float* sm /*[4]*/, float& mx, float& lse) {
    float m = -INFINITY;
    for (int c = threadIdx.x; c < C; c += NT) m = fmaxf(m, to_f32(z[c]));
    mx = block_max(m, sm);
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += NT) s += expf(to_f32(z[c]) - mx);
    lse = mx + logf(block_sum(s, sm));
}

// ---- LayerNorm of a row of D <= NT * EPT elements held in registers: v[i] = element threadIdx.x + NT * i, 0 where that is >= D ---------------------------
// Statistics in two passes (the mean, then the mean squared distance from it: rows with a large common offset keep their variance), each sum divided by (float)D.
__device__ __forceinline__ void row_ln_stats(const float (&v)[EPT], int D, float eps, float* sm /*[4]*/, float& mean, float& rstd) {
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < EPT; ++i) q += v[i];
    mean = block_sum(q, sm) / (float)D;
    q = 0.f;
#pragma unroll
    for (int i = 0; i < EPT; ++i) { const int k = threadIdx.x + NT * i; const float d = k < D ? v[i] - mean : 0.f; q += d * d; }
    rstd = rsqrtf(block_sum(q, sm) / (float)D + eps);
}
// Backward: with gy = g gamma and the normalised row xh, every thread sums gy into c1 and gy xh into c2 over its elements as it loads them; row_ln_bwd_means makes of
// them the row's c1 = mean(gy), c2 = mean(gy xh), and the input gradient of an element is row_ln_dx.
__device__ __forceinline__ void row_ln_bwd_means(float& c1, float& c2, int D, float* sm /*[8]*/) {
    block_sum2(c1, c2, sm);
    c1 /= (float)D; c2 /= (float)D;
}
__device__ __forceinline__ float row_ln_dx(float gy, float xh, float rstd, float c1, float c2) { return rstd * (gy - c1 - xh * c2); }

}  // namespace
