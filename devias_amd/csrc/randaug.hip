// RandAugment on the device: the 15 PIL operations of the reference's recipe (utils/transform/rand_augment.py, `--aa rand-m7-n4-mstd0.5-inc1`) on uint8 clips
// [T, H0, W0, 3] in one flat buffer, bit for bit what Pillow computes (include/devias_amd.h writes the arithmetic out per op; tests/golden/randaug_vectors.npz pins it).
//
//   devias_randaug_stats   per frame of every clip whose op needs statistics: the 3 x 256 histogram in LDS (integer atomics: any order gives the same bits) and from
//                          it AutoContrast's or Equalize's table, or the integer luminance sum and from it Contrast's grey level; one workgroup per (clip, frame),
//                          nothing is read back by the host
//   devias_randaug_apply   one layer for every clip whose op is not DEVIAS_RA_NONE: one launch per DEVIAS_RANDAUG_ROWS_PER_LAUNCH such clips, the op uniform per
//                          workgroup (blockIdx.y is the clip) and one body per arithmetic family:
//                            tables   Invert, Posterize, Solarize, SolarizeAdd (computed), AutoContrast, Equalize (read from stats)      in place
//                            blends   Brightness (against black), Contrast (against the frame's grey), Color (against the pixel's luminance), fp32      in place
//                            Sharpness   the blend against the 3 x 3 smooth of the frame, fp32                                          to the row's dst
//                            affine   fp64 coordinates, four bicubic or two bilinear fp64 taps per axis, truncation                     to the row's dst
// The point families own 16 pixels = 48 bytes a thread and move them with three 16-byte loads and stores where the clip's first byte is 16-byte aligned (clips of
// T = 16 frames packed back to back always are); the last, partial group of a clip and every group of an unaligned clip go byte by byte.  The neighbourhood
// families own one output pixel a thread.  No contraction in this unit: every fp32 and fp64 product and sum rounds on its own, as in PIL's C.
// The rows travel as kernel arguments (devias_clip_ingest's way): no table copy, no host synchronisation.
#pragma clang fp contract(off)
#include "common.h"
#include <atomic>
#include <math.h>

static std::atomic<int64_t> g_randaug_launches;
void devias_randaug_counter_reset() { g_randaug_launches.store(0, std::memory_order_relaxed); }
extern "C" int64_t devias_randaug_launches(void) { return g_randaug_launches.load(std::memory_order_relaxed); }

namespace {

struct RaTable {
    devias_randaug_row r[DEVIAS_RANDAUG_ROWS_PER_LAUNCH];
    int32_t b[DEVIAS_RANDAUG_ROWS_PER_LAUNCH];              // the clip's index in the batch: where its frames' statistics live
};

__host__ __device__ constexpr bool needs_stats(int op) { return op == DEVIAS_RA_AUTOCONTRAST || op == DEVIAS_RA_EQUALIZE || op == DEVIAS_RA_CONTRAST; }
__host__ __device__ constexpr bool neighbourhood(int op) { return op == DEVIAS_RA_SHARPNESS || op == DEVIAS_RA_AFFINE; }

__device__ __forceinline__ unsigned luminance(unsigned r, unsigned g, unsigned b) { return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16; }

// Image.blend: fl32(d + fl32(alpha * (i - d))), truncated; CLAMP where alpha lies outside [0, 1]
template <bool CLAMP>
__device__ __forceinline__ unsigned blend(unsigned d, unsigned i, float alpha) {
    const float t = (float)(int)d + alpha * (float)((int)i - (int)d);
    if constexpr (CLAMP) return t <= 0.f ? 0u : t >= 255.f ? 255u : (unsigned)(int)t;
    else return (unsigned)(int)t;
}

// ---- statistics: grid (T, clips of this launch), 512 threads ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void randaug_stats_kernel(const uint8_t* __restrict__ buf, uint8_t* __restrict__ stats, int Tn, const RaTable tab) {
    __shared__ unsigned hist[768];
    __shared__ unsigned pre[768];
    __shared__ int lo[3], hi[3];
    __shared__ unsigned step[3];
    __shared__ unsigned long long lsum;
    const devias_randaug_row& r = tab.r[blockIdx.y];
    const int t = blockIdx.x, tid = threadIdx.x;
    const unsigned npix = (unsigned)r.H0 * (unsigned)r.W0;
    const uint8_t* f = buf + r.src + (int64_t)t * npix * 3;
    uint8_t* out = stats + ((int64_t)tab.b[blockIdx.y] * Tn + t) * DEVIAS_RANDAUG_STATS_BYTES;
    for (int k = tid; k < 768; k += 512) hist[k] = 0;
    if (tid == 0) lsum = 0;
    __syncthreads();
    if (r.op == DEVIAS_RA_CONTRAST) {
        unsigned long long s = 0;
        for (unsigned p = tid; p < npix; p += 512) s += luminance(f[3 * (int64_t)p], f[3 * (int64_t)p + 1], f[3 * (int64_t)p + 2]);
        atomicAdd(&lsum, s);
        __syncthreads();
        if (tid == 0) *reinterpret_cast<int32_t*>(out + 768) = (int32_t)((double)lsum / (double)npix + 0.5);      // int(ImageStat.mean + 0.5)
        return;
    }
    for (unsigned p = tid; p < npix; p += 512)
        for (int c = 0; c < 3; ++c) atomicAdd(&hist[c * 256 + f[3 * (int64_t)p + c]], 1u);
    __syncthreads();
    if (tid < 3) {                                            // one thread per channel: the ends of the histogram, Equalize's step and running sums
        const unsigned* h = hist + tid * 256;
        int l = 0, u = 255;
        while (l < 255 && h[l] == 0) ++l;
        while (u > 0 && h[u] == 0) --u;
        lo[tid] = l; hi[tid] = u;
        unsigned nz = 0, n = 0;
        for (int k = 0; k < 256; ++k) nz += h[k] != 0;
        const unsigned st = nz > 1 ? (npix - h[u]) / 255u : 0u;                 // (sum of the bins - the last non-empty bin) // 255
        step[tid] = st;
        n = st / 2;
        for (int k = 0; k < 256; ++k) { pre[tid * 256 + k] = n; n += h[k]; }
    }
    __syncthreads();
    for (int k = tid; k < 768; k += 512) {
        const int c = k >> 8, ix = k & 255;
        int v = ix;
        if (r.op == DEVIAS_RA_AUTOCONTRAST) {
            if (hi[c] > lo[c]) {
                const double scale = 255.0 / (double)(hi[c] - lo[c]);
                const double offset = (double)(-lo[c]) * scale;
                v = (int)((double)ix * scale + offset);
                v = v < 0 ? 0 : v > 255 ? 255 : v;
            }
        } else if (step[c]) {
            const unsigned q = pre[k] / step[c];
            v = q > 255u ? 255 : (int)q;
        }
        out[k] = (uint8_t)v;
    }
}

// ---- the point families: 16 pixels a thread --------------------------------------------------------------------------------------------------------------
struct PointCtx {
    const uint8_t* stats;        // the clip's first frame's statistics
    unsigned hw;                 // pixels per frame
    int i0, i1;
    float f;
};

template <int OP, bool CLAMP>
__device__ __forceinline__ void point_px(const PointCtx& c, unsigned frame, unsigned& r, unsigned& g, unsigned& b) {
    if constexpr (OP == DEVIAS_RA_INVERT) { r = 255u - r; g = 255u - g; b = 255u - b; }
    else if constexpr (OP == DEVIAS_RA_POSTERIZE) { r &= (unsigned)c.i0; g &= (unsigned)c.i0; b &= (unsigned)c.i0; }
    else if constexpr (OP == DEVIAS_RA_SOLARIZE) {
        r = (int)r < c.i0 ? r : 255u - r; g = (int)g < c.i0 ? g : 255u - g; b = (int)b < c.i0 ? b : 255u - b;
    } else if constexpr (OP == DEVIAS_RA_SOLARIZE_ADD) {
        r = (int)r < c.i1 ? min(255u, r + (unsigned)c.i0) : r; g = (int)g < c.i1 ? min(255u, g + (unsigned)c.i0) : g; b = (int)b < c.i1 ? min(255u, b + (unsigned)c.i0) : b;
    } else if constexpr (OP == DEVIAS_RA_AUTOCONTRAST || OP == DEVIAS_RA_EQUALIZE) {
        const uint8_t* lut = c.stats + (int64_t)frame * DEVIAS_RANDAUG_STATS_BYTES;
        r = lut[r]; g = lut[256 + g]; b = lut[512 + b];
    } else if constexpr (OP == DEVIAS_RA_BRIGHTNESS) {
        r = blend<CLAMP>(0u, r, c.f); g = blend<CLAMP>(0u, g, c.f); b = blend<CLAMP>(0u, b, c.f);
    } else if constexpr (OP == DEVIAS_RA_CONTRAST) {
        const unsigned d = (unsigned)*reinterpret_cast<const int32_t*>(c.stats + (int64_t)frame * DEVIAS_RANDAUG_STATS_BYTES + 768);
        r = blend<CLAMP>(d, r, c.f); g = blend<CLAMP>(d, g, c.f); b = blend<CLAMP>(d, b, c.f);
    } else {                                                  // DEVIAS_RA_COLOR
        const unsigned d = luminance(r, g, b);
        r = blend<CLAMP>(d, r, c.f); g = blend<CLAMP>(d, g, c.f); b = blend<CLAMP>(d, b, c.f);
    }
}

template <int OP, bool CLAMP>
__device__ __forceinline__ void point_body(uint8_t* __restrict__ p, bool vec, unsigned npix, const PointCtx& c) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    if ((uint64_t)g * 16u >= npix) return;
    const unsigned q0 = g * 16u, n = npix - q0 < 16u ? npix - q0 : 16u;
    constexpr bool PER_FRAME = needs_stats(OP);
    unsigned f0 = 0;
    bool one_frame = true;
    if constexpr (PER_FRAME) { f0 = q0 / c.hw; one_frame = q0 + n <= (f0 + 1u) * c.hw; }
    uint8_t* base = p + (int64_t)q0 * 3;
    if (vec && n == 16u) {
        u32x4 w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = reinterpret_cast<const u32x4*>(base)[k];
        unsigned in[12], o[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { in[k] = w[k >> 2][k & 3]; o[k] = 0; }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            unsigned r = (in[(3 * q) >> 2] >> (8 * ((3 * q) & 3))) & 0xffu, gg = (in[(3 * q + 1) >> 2] >> (8 * ((3 * q + 1) & 3))) & 0xffu,
                     b = (in[(3 * q + 2) >> 2] >> (8 * ((3 * q + 2) & 3))) & 0xffu;
            unsigned fr = f0;
            if constexpr (PER_FRAME) { if (!one_frame) fr = (q0 + q) / c.hw; }
            point_px<OP, CLAMP>(c, fr, r, gg, b);
            o[(3 * q) >> 2] |= r << (8 * ((3 * q) & 3));
            o[(3 * q + 1) >> 2] |= gg << (8 * ((3 * q + 1) & 3));
            o[(3 * q + 2) >> 2] |= b << (8 * ((3 * q + 2) & 3));
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) { u32x4 v; v[0] = o[4 * k]; v[1] = o[4 * k + 1]; v[2] = o[4 * k + 2]; v[3] = o[4 * k + 3]; reinterpret_cast<u32x4*>(base)[k] = v; }
    } else {
        for (unsigned q = 0; q < n; ++q) {
            unsigned r = base[3 * q], gg = base[3 * q + 1], b = base[3 * q + 2];
            unsigned fr = f0;
            if constexpr (PER_FRAME) { if (!one_frame) fr = (q0 + q) / c.hw; }
            point_px<OP, CLAMP>(c, fr, r, gg, b);
            base[3 * q] = (uint8_t)r; base[3 * q + 1] = (uint8_t)gg; base[3 * q + 2] = (uint8_t)b;
        }
    }
}

// ---- Sharpness: one output pixel a thread ------------------------------------------------------------------------------------------------------------------
template <bool CLAMP>
__device__ __forceinline__ void sharp_body(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, unsigned npix, int H, int W, float alpha) {
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= npix) return;
    const unsigned hw = (unsigned)H * (unsigned)W, t = q / hw, rem = q - t * hw;
    const int y = (int)(rem / (unsigned)W), x = (int)(rem - (unsigned)y * (unsigned)W);
    const uint8_t* s = src + (int64_t)q * 3;
    uint8_t* o = dst + (int64_t)q * 3;
    if (x == 0 || y == 0 || x == W - 1 || y == H - 1) {      // the filter copies the border; a blend of a pixel with itself is the pixel
        o[0] = s[0]; o[1] = s[1]; o[2] = s[2];
        return;
    }
    constexpr float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    const int64_t row = (int64_t)W * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint8_t* up = s + c - row;
        const uint8_t* mid = s + c;
        const uint8_t* down = s + c + row;
        float ss = 0.5f;                                      // the row below first, as ImagingFilter accumulates
        ss += ((float)down[-3] * k1 + (float)down[0] * k1) + (float)down[3] * k1;
        ss += ((float)mid[-3] * k1 + (float)mid[0] * k5) + (float)mid[3] * k1;
        ss += ((float)up[-3] * k1 + (float)up[0] * k1) + (float)up[3] * k1;
        const int d = (int)ss;
        o[c] = (uint8_t)blend<CLAMP>((unsigned)(d < 0 ? 0 : d > 255 ? 255 : d), mid[0], alpha);
    }
}

// ---- the affine ops: one output pixel a thread ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double cubic(double v1, double v2, double v3, double v4, double d) {
    const double p1 = v2, p2 = -v1 + v3, p3 = 2 * (v1 - v2) + v3 - v4, p4 = -v1 + v2 - v3 + v4;
    return p1 + d * (p2 + d * (p3 + d * p4));
}

template <bool CUBIC>
__device__ __forceinline__ void affine_body(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, unsigned npix, int H, int W, const double* a) {
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= npix) return;
    const unsigned hw = (unsigned)H * (unsigned)W, t = q / hw, rem = q - t * hw;
    const int y = (int)(rem / (unsigned)W), x = (int)(rem - (unsigned)y * (unsigned)W);
    uint8_t* o = dst + (int64_t)q * 3;
    const double xs = (double)x + 0.5, ys = (double)y + 0.5;
    double xin = a[0] * xs + a[1] * ys + a[2];
    double yin = a[3] * xs + a[4] * ys + a[5];
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) {
        o[0] = 128; o[1] = 128; o[2] = 128;                   // the reference's fill colour
        return;
    }
    xin -= 0.5; yin -= 0.5;
    const int fx = (int)floor(xin), fy = (int)floor(yin);
    const double dx = xin - (double)fx, dy = yin - (double)fy;
    const uint8_t* f = src + (int64_t)t * hw * 3;
    constexpr int N = CUBIC ? 4 : 2, FIRST = CUBIC ? -1 : 0;
    int col[N];
    const uint8_t* rowp[N];                                   // a row outside the frame repeats the previous row's value: the clamped row's
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int cx = fx + FIRST + k, cy = fy + FIRST + k;
        col[k] = (cx < 0 ? 0 : cx > W - 1 ? W - 1 : cx) * 3;
        rowp[k] = f + (int64_t)(cy < 0 ? 0 : cy > H - 1 ? H - 1 : cy) * W * 3;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v;
        if constexpr (CUBIC) {
            double rv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                rv[k] = cubic((double)rowp[k][col[0] + c], (double)rowp[k][col[1] + c], (double)rowp[k][col[2] + c], (double)rowp[k][col[3] + c], dx);
            v = cubic(rv[0], rv[1], rv[2], rv[3], dy);
        } else {
            double rv[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const double p0 = (double)rowp[k][col[0] + c], p1 = (double)rowp[k][col[1] + c];
                rv[k] = p0 + (p1 - p0) * dx;
            }
            v = rv[0] + (rv[1] - rv[0]) * dy;
        }
        o[c] = v <= 0.0 ? (uint8_t)0 : v >= 255.0 ? (uint8_t)255 : (uint8_t)(int)v;
    }
}

// grid (work of the largest clip of this launch, clips of this launch)
__global__ __launch_bounds__(256) void randaug_apply_kernel(uint8_t* __restrict__ buf, const uint8_t* __restrict__ stats, int Tn, const RaTable tab) {
    const devias_randaug_row& r = tab.r[blockIdx.y];
    const unsigned hw = (unsigned)r.H0 * (unsigned)r.W0, npix = (unsigned)Tn * hw;
    uint8_t* s = buf + r.src;
    uint8_t* d = buf + r.dst;
    const bool clamp = !(r.f >= 0.f && r.f <= 1.f);
    if (r.op == DEVIAS_RA_AFFINE) {
        if (r.i0 == DEVIAS_RA_BICUBIC) affine_body<true>(s, d, npix, r.H0, r.W0, r.a); else affine_body<false>(s, d, npix, r.H0, r.W0, r.a);
        return;
    }
    if (r.op == DEVIAS_RA_SHARPNESS) {
        if (clamp) sharp_body<true>(s, d, npix, r.H0, r.W0, r.f); else sharp_body<false>(s, d, npix, r.H0, r.W0, r.f);
        return;
    }
    const PointCtx c{stats ? stats + (int64_t)tab.b[blockIdx.y] * Tn * DEVIAS_RANDAUG_STATS_BYTES : nullptr, hw, r.i0, r.i1, r.f};
    const bool vec = (reinterpret_cast<uintptr_t>(s) & 15) == 0;
    switch (r.op) {
    case DEVIAS_RA_INVERT: point_body<DEVIAS_RA_INVERT, false>(s, vec, npix, c); break;
    case DEVIAS_RA_POSTERIZE: point_body<DEVIAS_RA_POSTERIZE, false>(s, vec, npix, c); break;
    case DEVIAS_RA_SOLARIZE: point_body<DEVIAS_RA_SOLARIZE, false>(s, vec, npix, c); break;
    case DEVIAS_RA_SOLARIZE_ADD: point_body<DEVIAS_RA_SOLARIZE_ADD, false>(s, vec, npix, c); break;
    case DEVIAS_RA_AUTOCONTRAST: point_body<DEVIAS_RA_AUTOCONTRAST, false>(s, vec, npix, c); break;
    case DEVIAS_RA_EQUALIZE: point_body<DEVIAS_RA_EQUALIZE, false>(s, vec, npix, c); break;
    case DEVIAS_RA_BRIGHTNESS: if (clamp) point_body<DEVIAS_RA_BRIGHTNESS, true>(s, vec, npix, c); else point_body<DEVIAS_RA_BRIGHTNESS, false>(s, vec, npix, c); break;
    case DEVIAS_RA_CONTRAST: if (clamp) point_body<DEVIAS_RA_CONTRAST, true>(s, vec, npix, c); else point_body<DEVIAS_RA_CONTRAST, false>(s, vec, npix, c); break;
    case DEVIAS_RA_COLOR: if (clamp) point_body<DEVIAS_RA_COLOR, true>(s, vec, npix, c); else point_body<DEVIAS_RA_COLOR, false>(s, vec, npix, c); break;
    default: break;
    }
}

// Everything both entry points check before any launch.  A row with op DEVIAS_RA_NONE is not read further.
int check_rows(const char* who, const void* buf, int64_t bytes, const devias_randaug_row* rows, int B, int T, const void* stats) {
    DEVIAS_REQUIRE(buf && rows, "%s: null buf / rows", who);
    DEVIAS_REQUIRE(B >= 1 && T >= 1, "%s: bad dims B=%d T=%d (each >= 1)", who, B, T);
    DEVIAS_REQUIRE(bytes >= 1, "%s: bytes = %lld", who, (long long)bytes);
    for (int b = 0; b < B; ++b) {
        const devias_randaug_row& r = rows[b];
        DEVIAS_REQUIRE(r.op >= DEVIAS_RA_NONE && r.op <= DEVIAS_RA_AFFINE, "%s: rows[%d].op = %d", who, b, r.op);
        if (r.op == DEVIAS_RA_NONE) continue;
        DEVIAS_REQUIRE(r.H0 >= 1 && r.W0 >= 1 && r.H0 <= DEVIAS_INGEST_MAX_SIDE && r.W0 <= DEVIAS_INGEST_MAX_SIDE, "%s: rows[%d] has a bad frame H0=%d W0=%d (1 .. %d)", who, b,
                       r.H0, r.W0, DEVIAS_INGEST_MAX_SIDE);
        const int64_t npix = (int64_t)T * r.H0 * r.W0, n = npix * 3;
        DEVIAS_REQUIRE(npix < 0x7fffffff - 4096, "%s: rows[%d]: T*H0*W0 = %lld does not fit 2^31", who, b, (long long)npix);
        DEVIAS_REQUIRE(r.src >= 0 && r.src <= bytes - n, "%s: rows[%d]: src %lld + T*H0*W0*3 = %lld exceeds the buffer's %lld bytes", who, b, (long long)r.src, (long long)n,
                       (long long)bytes);
        if (neighbourhood(r.op)) {
            DEVIAS_REQUIRE(r.dst >= 0 && r.dst <= bytes - n, "%s: rows[%d]: dst %lld + T*H0*W0*3 = %lld exceeds the buffer's %lld bytes", who, b, (long long)r.dst, (long long)n,
                           (long long)bytes);
            DEVIAS_REQUIRE(r.dst + n <= r.src || r.src + n <= r.dst, "%s: rows[%d]: a neighbourhood op (%d) needs dst apart from src, got src %lld dst %lld (%lld bytes)", who, b, r.op,
                           (long long)r.src, (long long)r.dst, (long long)n);
        } else DEVIAS_REQUIRE(r.dst == r.src, "%s: rows[%d]: a point op (%d) works in place, got src %lld dst %lld", who, b, r.op, (long long)r.src, (long long)r.dst);
        DEVIAS_REQUIRE(stats || !needs_stats(r.op), "%s: rows[%d]: op %d needs the stats buffer", who, b, r.op);
        DEVIAS_REQUIRE(isfinite(r.f), "%s: rows[%d].f is not finite", who, b);
        if (r.op == DEVIAS_RA_AFFINE) {
            DEVIAS_REQUIRE(r.i0 == DEVIAS_RA_BILINEAR || r.i0 == DEVIAS_RA_BICUBIC, "%s: rows[%d]: resampling %d (DEVIAS_RA_BILINEAR or DEVIAS_RA_BICUBIC)", who, b, r.i0);
            for (int k = 0; k < 6; ++k) DEVIAS_REQUIRE(isfinite(r.a[k]), "%s: rows[%d].a[%d] is not finite", who, b, k);
        }
        if (r.op == DEVIAS_RA_POSTERIZE || r.op == DEVIAS_RA_SOLARIZE_ADD) DEVIAS_REQUIRE(r.i0 >= 0 && r.i0 <= 255, "%s: rows[%d].i0 = %d (0 .. 255)", who, b, r.i0);
        if (r.op == DEVIAS_RA_SOLARIZE) DEVIAS_REQUIRE(r.i0 >= 0 && r.i0 <= 256, "%s: rows[%d].i0 = %d (0 .. 256)", who, b, r.i0);
        if (r.op == DEVIAS_RA_SOLARIZE_ADD) DEVIAS_REQUIRE(r.i1 >= 0 && r.i1 <= 256, "%s: rows[%d].i1 = %d (0 .. 256)", who, b, r.i1);
        // no two clips of one launch touch the same bytes: a clip's src and dst runs lie apart from every earlier clip's
        for (int e = 0; e < b; ++e) {
            const devias_randaug_row& p = rows[e];
            if (p.op == DEVIAS_RA_NONE) continue;
            const int64_t pn = (int64_t)T * p.H0 * p.W0 * 3;
            const int64_t mine[2] = {r.src, r.dst}, theirs[2] = {p.src, p.dst};
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2; ++j)
                    DEVIAS_REQUIRE(mine[i] + n <= theirs[j] || theirs[j] + pn <= mine[i], "%s: rows[%d] and rows[%d] overlap (%lld + %lld, %lld + %lld)", who, b, e,
                                   (long long)mine[i], (long long)n, (long long)theirs[j], (long long)pn);
        }
    }
    return DEVIAS_OK;
}

}  // namespace

extern "C" int devias_randaug_stats(const void* buf, int64_t bytes, const devias_randaug_row* rows, int32_t B, int32_t T, void* stats, void* stream) {
    const char* who = "devias_randaug_stats";
    int rc = check_rows(who, buf, bytes, rows, B, T, stats);
    if (rc) return rc;
    DEVIAS_REQUIRE(stats, "%s: null stats", who);
    RaTable tab;
    int n = 0;
    for (int b = 0; b <= B; ++b) {
        if (b < B && needs_stats(rows[b].op)) { tab.r[n] = rows[b]; tab.b[n] = b; ++n; }
        if (n == DEVIAS_RANDAUG_ROWS_PER_LAUNCH || (b == B && n > 0)) {
            for (int k = n; k < DEVIAS_RANDAUG_ROWS_PER_LAUNCH; ++k) { tab.r[k] = tab.r[0]; tab.b[k] = tab.b[0]; }
            hipLaunchKernelGGL(randaug_stats_kernel, dim3(T, n), dim3(512), 0, (hipStream_t)stream, (const uint8_t*)buf, (uint8_t*)stats, T, tab);
            DEVIAS_CHECK_LAUNCH(who);
            g_randaug_launches.fetch_add(1, std::memory_order_relaxed);
            n = 0;
        }
    }
    return DEVIAS_OK;
}

extern "C" int devias_randaug_apply(void* buf, int64_t bytes, const devias_randaug_row* rows, int32_t B, int32_t T, const void* stats, void* stream) {
    const char* who = "devias_randaug_apply";
    int rc = check_rows(who, buf, bytes, rows, B, T, stats);
    if (rc) return rc;
    RaTable tab;
    int n = 0;
    int64_t blocks = 0;
    for (int b = 0; b <= B; ++b) {
        if (b < B && rows[b].op != DEVIAS_RA_NONE) {
            const int64_t npix = (int64_t)T * rows[b].H0 * rows[b].W0;
            const int64_t need = neighbourhood(rows[b].op) ? (npix + 255) / 256 : ((npix + 15) / 16 + 255) / 256;
            blocks = need > blocks ? need : blocks;
            tab.r[n] = rows[b]; tab.b[n] = b; ++n;
        }
        if (n == DEVIAS_RANDAUG_ROWS_PER_LAUNCH || (b == B && n > 0)) {
            for (int k = n; k < DEVIAS_RANDAUG_ROWS_PER_LAUNCH; ++k) { tab.r[k] = tab.r[0]; tab.b[k] = tab.b[0]; }
            hipLaunchKernelGGL(randaug_apply_kernel, dim3((unsigned)blocks, n), dim3(256), 0, (hipStream_t)stream, (uint8_t*)buf, (const uint8_t*)stats, T, tab);
            DEVIAS_CHECK_LAUNCH(who);
            g_randaug_launches.fetch_add(1, std::memory_order_relaxed);
            n = 0; blocks = 0;
        }
    }
    return DEVIAS_OK;
}
