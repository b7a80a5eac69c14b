// Mixup / CutMix on the device (utils/transform/mixup.py: Mixup) and the loss the mixed targets train with (timm's SoftTargetCrossEntropy).
//
//   devias_mixup_clips    x [B, P, H, W] mixed in place from a per-clip table; clip i pairs with clip B-1-i in every mode of the reference
//   devias_mixup_target   the dense soft target [B, C] from int64 labels and per-row weights, one launch
//   devias_soft_ce_fwd / _bwd   mean_b sum_c -t log_softmax(z), one workgroup per row (row_kernels.h), rows summed in index order
//
// The clip kernel is a stream: one thread owns a 16-byte piece (or, on the scalar path, one element) of BOTH clips of a pair, loads both, computes both, stores what
// changed -- so in place is safe without the reference's clone / flip copy, and the traffic is one read and one write of what is touched.  The table rows travel as kernel
// arguments: nothing is copied to the device ahead of the launch, so there is no copy to wait for and none to race with.
// The arithmetic is ATen's mul_ / add_ sequence: every product and the sum are rounded to T on their own.  No contraction in this unit: a fused multiply-add would skip
// the product's rounding (__fmul_rn is a plain `*` to the compiler, which the library's -ffp-contract=fast may fuse).
#pragma clang fp contract(off)
#include "common.h"
#include "region_host.h"      // argument checks, dispatch_t
#include "row_kernels.h"       // NT, block reductions, row_stats

namespace {

// ---- clip mix ------------------------------------------------------------------------------------------------------------------------------------------
struct MixRow { int kind; float ws, wo; int yl, yh, xl, xh; };      // the box already clamped to the plane by the host side below
// One active pair: clips i and B-1-i.  What it touches is `nseg` runs of `seg_len` elements, run s starting at element s * H * W + seg_off of a clip:
// the whole clip as one run (a MIXUP row, or boxes over every row), or rows [y0, y1) of each of the P planes (CUTMIX / NONE rows only).
struct MixPair { int i, nseg, seg_len, seg_off, need_xy; MixRow r[2]; };
struct MixPairTable { MixPair p[DEVIAS_MIXUP_PAIRS_PER_LAUNCH]; };

template <typename T, int VEC> struct Pack { typedef T type __attribute__((ext_vector_type(VEC))); };

template <typename T>
__device__ __forceinline__ T mix_one(T xs, T xo, float ws, float wo) {
    const float a = to_f32(from_f32<T>(__fmul_rn(to_f32(xs), ws)));
    const float b = to_f32(from_f32<T>(__fmul_rn(to_f32(xo), wo)));
    return from_f32<T>(__fadd_rn(a, b));
}

// grid (pieces, pairs of this launch).  VEC = 16 / sizeof(T): x and the clip stride are 16-byte aligned and W >= VEC, so that a piece never reaches into two runs
// (two runs are at least one row of W elements apart) and every piece has one owner; VEC = 1: anything.
template <typename T, int VEC, bool NONTEMPORAL>
__global__ __launch_bounds__(256) void mixup_clips_kernel(T* __restrict__ X, int B, int64_t clip, int HW, int W, const MixPairTable tab) {
    const MixPair& pr = tab.p[blockIdx.y];
    const unsigned vps = ((unsigned)pr.seg_len + 2u * (VEC - 1)) / VEC;          // pieces that can meet one run
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    const unsigned s = t / vps, k = t - s * vps;
    if (s >= (unsigned)pr.nseg) return;
    const unsigned start = s * (unsigned)HW + (unsigned)pr.seg_off, end = start + (unsigned)pr.seg_len;
    const unsigned e0 = (start / VEC + k) * VEC;
    if (e0 >= end) return;
    typedef typename Pack<T, VEC>::type V;
    V* pi = reinterpret_cast<V*>(X + (int64_t)pr.i * clip + e0);
    V* pj = reinterpret_cast<V*>(X + (int64_t)(B - 1 - pr.i) * clip + e0);
    V a, b;
    if constexpr (NONTEMPORAL) { a = __builtin_nontemporal_load(pi); b = __builtin_nontemporal_load(pj); } else { a = *pi; b = *pj; }
    V oa = a, ob = b;
    const MixRow ri = pr.r[0], rj = pr.r[1];
    bool si = ri.kind == DEVIAS_MIX_MIXUP, sj = rj.kind == DEVIAS_MIX_MIXUP;
    unsigned y = 0, x = 0;
    if (pr.need_xy) { const unsigned r = e0 % (unsigned)HW; y = r / (unsigned)W; x = r - y * (unsigned)W; }
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        if (ri.kind == DEVIAS_MIX_MIXUP) oa[q] = mix_one<T>(a[q], b[q], ri.ws, ri.wo);
        else if (ri.kind == DEVIAS_MIX_CUTMIX && (int)y >= ri.yl && (int)y < ri.yh && (int)x >= ri.xl && (int)x < ri.xh) { oa[q] = b[q]; si = true; }
        if (rj.kind == DEVIAS_MIX_MIXUP) ob[q] = mix_one<T>(b[q], a[q], rj.ws, rj.wo);
        else if (rj.kind == DEVIAS_MIX_CUTMIX && (int)y >= rj.yl && (int)y < rj.yh && (int)x >= rj.xl && (int)x < rj.xh) { ob[q] = a[q]; sj = true; }
        if (++x == (unsigned)W) { x = 0; if (++y == (unsigned)(HW / W)) y = 0; }
    }
    if constexpr (NONTEMPORAL) {
        if (si) __builtin_nontemporal_store(oa, pi);
        if (sj) __builtin_nontemporal_store(ob, pj);
    } else {
        if (si) *pi = oa;
        if (sj) *pj = ob;
    }
}

// ---- soft target ---------------------------------------------------------------------------------------------------------------------------------------
struct TargetWeights { float ws[DEVIAS_MIXUP_TARGET_ROWS_PER_LAUNCH], wo[DEVIAS_MIXUP_TARGET_ROWS_PER_LAUNCH]; };
// rows [r0, r0 + rows): out[b, c] = fl(v(y_b, c) ws[b]) + fl(v(y_{B-1-b}, c) wo[b]); a label outside [0, C) in either place: the row is NaN (never an index)
__global__ __launch_bounds__(256) void mixup_target_kernel(const int64_t* __restrict__ target, int B, int C, int r0, int rows, float on, float off, const TargetWeights w,
                                                           float* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)rows * C) return;
    const int lr = (int)(idx / C), c = (int)(idx - (int64_t)lr * C), b = r0 + lr;
    const int64_t y1 = target[b], y2 = target[B - 1 - b];
    const bool ok = y1 >= 0 && y1 < C && y2 >= 0 && y2 < C;
    const float v = __fadd_rn(__fmul_rn(c == (int)y1 ? on : off, w.ws[lr]), __fmul_rn(c == (int)y2 ? on : off, w.wo[lr]));
    out[(int64_t)b * C + c] = ok ? v : __builtin_nanf("");
}

// ---- soft-target cross-entropy (timm.loss.SoftTargetCrossEntropy) -----------------------------------------------------------------------------------------
// row b: lse * sum_c t - sum_c t z, both relative to the row maximum (sum_c t is whatever the target holds: a scaled or an all-zero row is served as it is)
template <typename T>
__global__ __launch_bounds__(NT) void soft_ce_fwd_kernel(const T* __restrict__ Z, const float* __restrict__ Tg, int C, float* __restrict__ per_row) {
    __shared__ float sm[8];
    const int b = blockIdx.x;
    const T* z = Z + (int64_t)b * C;
    const float* t = Tg + (int64_t)b * C;
    float m = -INFINITY;
    for (int c = threadIdx.x; c < C; c += NT) m = fmaxf(m, to_f32(z[c]));
    const float mx = block_max(m, sm);
    float s = 0.f, st = 0.f, stz = 0.f;
    for (int c = threadIdx.x; c < C; c += NT) { const float v = to_f32(z[c]) - mx, tc = t[c]; s += expf(v); st += tc; stz += tc * v; }
    const float lse = logf(block_sum(s, sm));                 // relative to mx
    block_sum2(st, stz, sm);
    if (threadIdx.x == 0) per_row[b] = lse * st - stz;
}
__global__ void soft_ce_final_kernel(const float* __restrict__ per_row, int B, float* __restrict__ loss) {
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += per_row[b];
        loss[0] = s / (float)B;
    }
}
// dz = g / B (p_c sum_c t - t_c)
template <typename T>
__global__ __launch_bounds__(NT) void soft_ce_bwd_kernel(const T* __restrict__ Z, const float* __restrict__ Tg, int B, int C, const float* __restrict__ g_loss,
                                                         T* __restrict__ dZ) {
    __shared__ float sm[4];
    const int b = blockIdx.x;
    const T* z = Z + (int64_t)b * C;
    const float* t = Tg + (int64_t)b * C;
    T* dz = dZ + (int64_t)b * C;
    float mx, lse;
    row_stats(z, C, sm, mx, lse);
    float st = 0.f;
    for (int c = threadIdx.x; c < C; c += NT) st += t[c];
    st = block_sum(st, sm);
    const float g = g_loss[0] / (float)B;
    for (int c = threadIdx.x; c < C; c += NT) dz[c] = from_f32<T>(g * (expf(to_f32(z[c]) - lse) * st - t[c]));
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------
inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the row as the kernel reads it: the box clamped to the plane; a CUTMIX row with an empty box changes nothing and becomes NONE
MixRow device_row(const devias_mixup_row& r, int H, int W) {
    MixRow d{r.kind, r.w_self, r.w_other, 0, 0, 0, 0};
    if (r.kind == DEVIAS_MIX_CUTMIX) {
        d.yl = clampi(r.yl, 0, H); d.yh = clampi(r.yh, d.yl, H); d.xl = clampi(r.xl, 0, W); d.xh = clampi(r.xh, d.xl, W);
        if (d.yl == d.yh || d.xl == d.xh) d.kind = DEVIAS_MIX_NONE;
    }
    return d;
}

template <typename T, int VEC>
void launch_clips(void* x, int B, int64_t clip, int HW, int W, const MixPairTable& tab, int npairs, unsigned pieces, hipStream_t st) {
#ifdef DEVIAS_MIXUP_NT
    constexpr bool nt = true;
#else
    constexpr bool nt = false;            // measured both ways (profiles/mixup.txt)
#endif
    hipLaunchKernelGGL((mixup_clips_kernel<T, VEC, nt>), dim3(cdiv(pieces, 256), npairs), dim3(256), 0, st, (T*)x, B, clip, HW, W, tab);
}

int soft_ce_check(const char* who, const void* logits, const float* target, int B, int C, int dtype) {
    DEVIAS_REQUIRE(logits && target, "%s: null logits / target", who);
    DEVIAS_REQUIRE(dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    DEVIAS_REQUIRE(B >= 1 && C >= 2, "%s: bad dims B=%d C=%d (B >= 1, C >= 2)", who, B, C);
    return DEVIAS_OK;
}

}  // namespace

extern "C" int devias_mixup_clips(void* x, int32_t B, int32_t P, int32_t H, int32_t W, int32_t dtype, const devias_mixup_row* table, void* stream) {
    const char* who = "devias_mixup_clips";
    DEVIAS_REQUIRE(x && table, "%s: null x / table", who);
    DEVIAS_REQUIRE(dtype_ok(dtype), "%s: bad dtype %d", who, dtype);
    DEVIAS_REQUIRE(B >= 2 && B % 2 == 0, "%s: B=%d must be even and >= 2 (clip i pairs with clip B-1-i)", who, B);
    DEVIAS_REQUIRE(P >= 1 && H >= 1 && W >= 1 && (int64_t)P * H * W < 0x7fffffff - 64, "%s: bad dims P=%d H=%d W=%d (each >= 1, P*H*W < 2^31)", who, P, H, W);
    for (int b = 0; b < B; ++b) {
        const devias_mixup_row& r = table[b];
        DEVIAS_REQUIRE(r.kind == DEVIAS_MIX_NONE || r.kind == DEVIAS_MIX_MIXUP || r.kind == DEVIAS_MIX_CUTMIX, "%s: table[%d].kind = %d", who, b, r.kind);
        DEVIAS_REQUIRE(r.kind != DEVIAS_MIX_MIXUP || (r.w_self == r.w_self && r.w_other == r.w_other), "%s: table[%d] has a NaN weight", who, b);
    }
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, esize = dtype == DEVIAS_BF16 ? 2 : 4, VEC = 16 / esize;
    const int64_t clip = (int64_t)P * HW;
    const bool vec = aligned16(x) && (clip * esize) % 16 == 0 && W >= VEC;
    MixPairTable tab;
    int n = 0;
    unsigned pieces = 0;
    auto flush = [&]() -> int {
        if (!n) return DEVIAS_OK;
        if (dtype == DEVIAS_BF16) { if (vec) launch_clips<bf16, 8>(x, B, clip, HW, W, tab, n, pieces, st); else launch_clips<bf16, 1>(x, B, clip, HW, W, tab, n, pieces, st); }
        else { if (vec) launch_clips<float, 4>(x, B, clip, HW, W, tab, n, pieces, st); else launch_clips<float, 1>(x, B, clip, HW, W, tab, n, pieces, st); }
        DEVIAS_CHECK_LAUNCH("devias_mixup_clips");
        n = 0; pieces = 0;
        return DEVIAS_OK;
    };
    for (int i = 0; i < B / 2; ++i) {
        MixPair p;
        p.i = i;
        p.r[0] = device_row(table[i], H, W);
        p.r[1] = device_row(table[B - 1 - i], H, W);
        const int k0 = p.r[0].kind, k1 = p.r[1].kind;
        if (k0 == DEVIAS_MIX_NONE && k1 == DEVIAS_MIX_NONE) continue;
        int y0 = H, y1 = 0;
        for (int q = 0; q < 2; ++q) if (p.r[q].kind == DEVIAS_MIX_CUTMIX) { y0 = p.r[q].yl < y0 ? p.r[q].yl : y0; y1 = p.r[q].yh > y1 ? p.r[q].yh : y1; }
        p.need_xy = k0 == DEVIAS_MIX_CUTMIX || k1 == DEVIAS_MIX_CUTMIX;
        if (k0 == DEVIAS_MIX_MIXUP || k1 == DEVIAS_MIX_MIXUP || (y0 == 0 && y1 == H)) { p.nseg = 1; p.seg_len = (int)clip; p.seg_off = 0; }
        else { p.nseg = P; p.seg_len = (y1 - y0) * W; p.seg_off = y0 * W; }
        const unsigned v = vec ? VEC : 1, w = (unsigned)p.nseg * (((unsigned)p.seg_len + 2u * (v - 1)) / v);
        pieces = w > pieces ? w : pieces;
        tab.p[n++] = p;
        if (n == DEVIAS_MIXUP_PAIRS_PER_LAUNCH) RUN(flush());
    }
    return flush();
}

extern "C" int devias_mixup_target(const int64_t* target, int32_t B, int32_t C, float on, float off, const float* w_self, const float* w_other, float* out, void* stream) {
    const char* who = "devias_mixup_target";
    DEVIAS_REQUIRE(target && w_self && w_other && out, "%s: null target / w_self / w_other / out", who);
    DEVIAS_REQUIRE(B >= 1 && C >= 2 && C < (1 << 24), "%s: bad dims B=%d C=%d (B >= 1, 2 <= C < 2^24)", who, B, C);
    hipStream_t st = (hipStream_t)stream;
    for (int r0 = 0; r0 < B; r0 += DEVIAS_MIXUP_TARGET_ROWS_PER_LAUNCH) {
        const int rows = B - r0 < DEVIAS_MIXUP_TARGET_ROWS_PER_LAUNCH ? B - r0 : DEVIAS_MIXUP_TARGET_ROWS_PER_LAUNCH;
        TargetWeights w;
        for (int r = 0; r < DEVIAS_MIXUP_TARGET_ROWS_PER_LAUNCH; ++r) { w.ws[r] = r < rows ? w_self[r0 + r] : 0.f; w.wo[r] = r < rows ? w_other[r0 + r] : 0.f; }
        hipLaunchKernelGGL(mixup_target_kernel, dim3(cdiv((int64_t)rows * C, 256)), dim3(256), 0, st, target, B, C, r0, rows, on, off, w, out);
        DEVIAS_CHECK_LAUNCH(who);
    }
    return DEVIAS_OK;
}

extern "C" int64_t devias_soft_ce_workspace_bytes(int32_t B) { return B >= 1 ? (int64_t)B * 4 : 0; }

extern "C" int devias_soft_ce_fwd(const void* logits, const float* target, int32_t B, int32_t C, int32_t dtype, float* loss, float* ws, void* stream) {
    const char* who = "devias_soft_ce_fwd";
    RUN(soft_ce_check(who, logits, target, B, C, dtype));
    DEVIAS_REQUIRE(loss && ws, "%s: null loss / ws", who);
    hipStream_t st = (hipStream_t)stream;
    dispatch_t(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((soft_ce_fwd_kernel<T>), dim3(B), dim3(NT), 0, st, (const T*)logits, target, C, ws);
    });
    DEVIAS_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(soft_ce_final_kernel, dim3(1), dim3(64), 0, st, ws, B, loss);
    DEVIAS_CHECK_LAUNCH("devias_soft_ce_fwd(final)");
    return DEVIAS_OK;
}

extern "C" int devias_soft_ce_bwd(const void* logits, const float* target, int32_t B, int32_t C, int32_t dtype, const float* g_loss, void* dlogits, void* stream) {
    const char* who = "devias_soft_ce_bwd";
    RUN(soft_ce_check(who, logits, target, B, C, dtype));
    DEVIAS_REQUIRE(g_loss && dlogits, "%s: null g_loss / dlogits", who);
    hipStream_t st = (hipStream_t)stream;
    dispatch_t(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((soft_ce_bwd_kernel<T>), dim3(B), dim3(NT), 0, st, (const T*)logits, target, B, C, g_loss, (T*)dlogits);
    });
    DEVIAS_CHECK_LAUNCH(who);
    return DEVIAS_OK;
}
