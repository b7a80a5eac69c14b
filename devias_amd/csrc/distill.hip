// The scene head's distillation loss of the two-token multi-task baseline (run_multi_task_finetuning.py: TrainLoss).
//
//   devias_distill_fwd / _bwd   KL(teacher || student) on the (left-padded) teacher logits, or cross-entropy against the teacher's argmax; one workgroup per row
//
// One-workgroup-per-row kernels from row_kernels.h, fp32 arithmetic, the rows summed in index order: no atomics.  The head region whose logits it takes: token_head.hip.
#include "common.h"
#include "region_host.h"      // argument checks, dispatch_t
#include "row_kernels.h"       // NT, block reductions, row_stats

namespace {

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
int distill_check(const char* who, const void* student, const float* teacher, int B, int C, int Ct, int dtype, int mode, float weight) {
    DEVIAS_REQUIRE(student && teacher, "%s: null student / teacher", who);
    DEVIAS_REQUIRE(dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    DEVIAS_REQUIRE(mode == DEVIAS_DISTILL_KL || mode == DEVIAS_DISTILL_CE, "%s: bad mode %d (DEVIAS_DISTILL_KL or DEVIAS_DISTILL_CE)", who, mode);
    DEVIAS_REQUIRE(B >= 1 && Ct >= 2 && C >= Ct && C < (1 << 24), "%s: bad dims B=%d C=%d Ct=%d (B >= 1, 2 <= Ct <= C < 2^24)", who, B, C, Ct);
    DEVIAS_REQUIRE(weight == weight, "%s: weight is NaN", who);
    return DEVIAS_OK;
}

}  // namespace

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
