// Clip ingest on the device: the stretch between the decoder and the model (dataset/kinetics.py:_aug_frame after RandAugment -- ToTensor, tensor_normalize,
// random_resized_crop, horizontal_flip -- and the validation / test CenterCrop / window, ClipToTensor, Normalize).
//
//   devias_clip_ingest    uint8 frames [T, H0, W0, 3] of B clips in one flat buffer -> out [B, 3, T, S_h, S_w] fp32 or bf16: normalised, cropped to a box per clip,
//                         bilinearly resized (half-pixel rule, align_corners=False) and flipped, one launch per DEVIAS_INGEST_ROWS_PER_LAUNCH clips
//
// A normalised tap has 256 x 3 possible values, fl(fl(fl(u / 255) - m_c) / s_c): the 768-entry table the host built with those three fp32 operations is copied to
// LDS by every workgroup, and a tap is one byte of a load and one LDS read (the two taps of a source row come with ONE unaligned 8-byte load: load_pair).  Source rows and columns come from integers: ((2d + 1) n_in - n_out) / (2 n_out) has the
// first tap as its quotient and the weight of the second as its remainder over 2 n_out, rounded once; then only the interpolation rounds:
//   out = fl(fl(wy0 fl(fl(wx0 a) + fl(wx1 b))) + fl(wy1 fl(fl(wx0 c) + fl(wx1 d)))),  w1 = lambda, w0 = fl(1 - lambda)
// so a box with h = S_h, w = S_w (every lambda 0) returns the taps themselves, bit for bit.  No contraction in this unit: a fused multiply-add would skip a product's rounding.
// The kernel is a stream: one thread owns VEC output columns of one (clip, frame, row) for all three channels and stores each plane
// with one 16-byte store (VEC = 16 / sizeof(T): S_w % VEC == 0 and a 16-byte aligned out); VEC = 1 serves everything else.  The table rows travel as kernel
// arguments (devias_mixup_clips's way): no per-step table copy, no host synchronisation.  Measured (profiles/ingest.txt): bound by the tap loads, the table reads and the
// integer divisions, not by the stores.
#pragma clang fp contract(off)
#include "common.h"
#include "region_host.h"      // argument checks, RUN

namespace {

struct IngestTable { devias_ingest_row r[DEVIAS_INGEST_ROWS_PER_LAUNCH]; };

template <typename T, int VEC> struct OutPack { typedef T type __attribute__((ext_vector_type(VEC))); };

// first tap and the weight of the second for output index d of n_out over a source run of n_in: src = max((d + 0.5) n_in / n_out - 0.5, 0)
__device__ __forceinline__ void tap_of(unsigned d, unsigned n_in, unsigned n_out, unsigned& i0, unsigned& i1, float& lam) {
    const int num = (int)((2u * d + 1u) * n_in) - (int)n_out;               // < 2^31: the host checked (2 n_out + 1) n_in
    if (num <= 0) { i0 = 0; lam = 0.f; }
    else {
        const unsigned den = 2u * n_out, q = (unsigned)num / den, r = (unsigned)num - q * den;
        i0 = q;
        lam = __fdiv_rn((float)r, (float)den);                               // both below 2^24: exact operands, one rounding
    }
    i1 = i0 + 1 < n_in ? i0 + 1 : n_in - 1;
}

__device__ __forceinline__ float lerp2(float a, float b, float c, float d, float wx0, float wx1, float wy0, float wy1) {
    const float top = __fadd_rn(__fmul_rn(wx0, a), __fmul_rn(wx1, b));
    const float bot = __fadd_rn(__fmul_rn(wx0, c), __fmul_rn(wx1, d));
    return __fadd_rn(__fmul_rn(wy0, top), __fmul_rn(wy1, bot));
}

// The two taps of one source row, pixels c0 and c0 + 1 (or c0 alone at a clamped edge), in the low bytes of the result: three bytes a pixel.
// WIDE: ONE unaligned 8-byte load instead of six byte loads -- the kernel is bound by the number of load instructions, not by their bytes.  The load never leaves the
// buffer: where fewer than 8 bytes remain behind `a` it starts at last8 = src_bytes - 8 and the value is shifted down; the three (six) bytes that are used lie inside the
// clip, so at most five (two) bytes are shifted out and all that are used are there.  !WIDE (a buffer below 8 bytes): byte loads.
template <bool WIDE>
__device__ __forceinline__ uint64_t load_pair(const uint8_t* __restrict__ src, int64_t a, bool two, int64_t last8) {
    if constexpr (WIDE) {
        const int64_t b = a < last8 ? a : last8;
        uint64_t v;
        __builtin_memcpy(&v, src + b, 8);
        return v >> ((unsigned)(a - b) * 8u);
    } else {
        uint64_t v = 0;
        const int n = two ? 6 : 3;
        for (int k = 0; k < n; ++k) v |= (uint64_t)src[a + k] << (8 * k);
        return v;
    }
}

// grid (pieces of one clip, clips of this launch); a piece: VEC output columns of one (frame, row)
template <typename T, int VEC, bool WIDE>
__global__ __launch_bounds__(256) void clip_ingest_kernel(const uint8_t* __restrict__ src, int64_t last8, const float* __restrict__ lut, T* __restrict__ out, int b0, int Tn,
                                                          int Sh, int Sw, const IngestTable tab) {
    __shared__ float tbl[768];
    for (int k = threadIdx.x; k < 768; k += 256) tbl[k] = lut[k];
    __syncthreads();
    const devias_ingest_row& r = tab.r[blockIdx.y];
    const unsigned ppr = (unsigned)Sw / VEC;                                 // pieces per output row
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= (unsigned)Tn * (unsigned)Sh * ppr) return;
    const unsigned row = p / ppr, x0 = (p - row * ppr) * VEC;
    const unsigned t = row / (unsigned)Sh, y = row - t * (unsigned)Sh;
    unsigned r0, r1;
    float ly;
    tap_of(y, (unsigned)r.h, (unsigned)Sh, r0, r1, ly);
    const float wy0 = __fsub_rn(1.f, ly);
    const int64_t frame = r.offset + (int64_t)t * r.H0 * r.W0 * 3;
    const int64_t p0 = frame + ((int64_t)(r.i + (int)r0) * r.W0 + r.j) * 3;            // byte index of the box's first column in the two source rows
    const int64_t p1 = frame + ((int64_t)(r.i + (int)r1) * r.W0 + r.j) * 3;
    const bool two_rows = ly != 0.f;                                        // lambda 0 (an identity box, a clamped edge): the second row has weight 0 and is not loaded
    float v[3][VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        const unsigned x = x0 + q, d = r.flip ? (unsigned)Sw - 1u - x : x;   // the flip acts on the output column, after the resize
        unsigned c0, c1;
        float lx;
        tap_of(d, (unsigned)r.w, (unsigned)Sw, c0, c1, lx);
        const float wx0 = __fsub_rn(1.f, lx);
        const unsigned sh = c1 != c0 ? 24u : 0u;                             // where the second tap's three bytes sit in the pair
        const uint64_t u0 = load_pair<WIDE>(src, p0 + c0 * 3, c1 != c0, last8);
        const uint64_t u1 = two_rows ? load_pair<WIDE>(src, p1 + c0 * 3, c1 != c0, last8) : u0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a = tbl[c * 256 + (unsigned)((u0 >> (8 * c)) & 0xff)], b = tbl[c * 256 + (unsigned)((u0 >> (sh + 8 * c)) & 0xff)];
            const float cc = tbl[c * 256 + (unsigned)((u1 >> (8 * c)) & 0xff)], dd = tbl[c * 256 + (unsigned)((u1 >> (sh + 8 * c)) & 0xff)];
            v[c][q] = lerp2(a, b, cc, dd, wx0, lx, wy0, ly);
        }
    }
    const int64_t plane = (int64_t)Tn * Sh * Sw;
    T* o = out + ((int64_t)(b0 + (int)blockIdx.y) * 3) * plane + ((int64_t)t * Sh + y) * Sw + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if constexpr (VEC == 1) o[c * plane] = from_f32<T>(v[c][0]);
        else {
            typename OutPack<T, VEC>::type pk;
#pragma unroll
            for (int q = 0; q < VEC; ++q) pk[q] = from_f32<T>(v[c][q]);
            *reinterpret_cast<typename OutPack<T, VEC>::type*>(o + c * plane) = pk;
        }
    }
}

template <typename T, int VEC>
void launch_ingest(const uint8_t* src, int64_t src_bytes, const float* lut, void* out, int b0, int n, int T_, int Sh, int Sw, const IngestTable& tab, hipStream_t st) {
    const int64_t pieces = (int64_t)T_ * Sh * (Sw / VEC);
    const dim3 grid(cdiv(pieces, 256), n);
    if (src_bytes >= 8) hipLaunchKernelGGL((clip_ingest_kernel<T, VEC, true>), grid, dim3(256), 0, st, src, src_bytes - 8, lut, (T*)out, b0, T_, Sh, Sw, tab);
    else hipLaunchKernelGGL((clip_ingest_kernel<T, VEC, false>), grid, dim3(256), 0, st, src, (int64_t)0, lut, (T*)out, b0, T_, Sh, Sw, tab);
}

}  // namespace

extern "C" int devias_clip_ingest(const void* src, int64_t src_bytes, const float* table, const devias_ingest_row* rows, int32_t B, int32_t T, int32_t S_h, int32_t S_w,
                                  int32_t out_dtype, void* out, void* stream) {
    const char* who = "devias_clip_ingest";
    DEVIAS_REQUIRE(src && table && rows && out, "%s: null src / table / rows / out", who);
    DEVIAS_REQUIRE(dtype_ok(out_dtype), "%s: bad out_dtype %d", who, out_dtype);
    DEVIAS_REQUIRE(B >= 1 && T >= 1, "%s: bad dims B=%d T=%d (each >= 1)", who, B, T);
    DEVIAS_REQUIRE(S_h >= 1 && S_w >= 1 && S_h <= DEVIAS_INGEST_MAX_SIDE && S_w <= DEVIAS_INGEST_MAX_SIDE, "%s: bad crop size S_h=%d S_w=%d (1 .. %d)", who, S_h, S_w,
                   DEVIAS_INGEST_MAX_SIDE);
    DEVIAS_REQUIRE((int64_t)T * S_h * S_w < 0x7fffffff - 256, "%s: T*S_h*S_w = %lld does not fit 2^31", who, (long long)T * S_h * S_w);
    DEVIAS_REQUIRE(src_bytes >= 1, "%s: src_bytes = %lld", who, (long long)src_bytes);
    for (int b = 0; b < B; ++b) {
        const devias_ingest_row& r = rows[b];
        DEVIAS_REQUIRE(r.H0 >= 1 && r.W0 >= 1 && r.H0 <= DEVIAS_INGEST_MAX_SIDE && r.W0 <= DEVIAS_INGEST_MAX_SIDE, "%s: rows[%d] has a bad frame H0=%d W0=%d (1 .. %d)", who, b,
                       r.H0, r.W0, DEVIAS_INGEST_MAX_SIDE);
        DEVIAS_REQUIRE(r.h >= 1 && r.w >= 1, "%s: rows[%d] has an empty box h=%d w=%d", who, b, r.h, r.w);
        DEVIAS_REQUIRE(r.i >= 0 && r.j >= 0 && (int64_t)r.i + r.h <= r.H0 && (int64_t)r.j + r.w <= r.W0, "%s: rows[%d]'s box i=%d j=%d h=%d w=%d leaves its %d x %d frame", who, b,
                       r.i, r.j, r.h, r.w, r.H0, r.W0);
        DEVIAS_REQUIRE(r.flip == 0 || r.flip == 1, "%s: rows[%d].flip = %d", who, b, r.flip);
        const int64_t bytes = (int64_t)T * r.H0 * r.W0 * 3;                  // < 2^31 * 2^28 * 3: no overflow
        DEVIAS_REQUIRE(r.offset >= 0 && r.offset <= src_bytes - bytes, "%s: rows[%d]: offset %lld + T*H0*W0*3 = %lld exceeds the buffer's %lld bytes", who, b,
                       (long long)r.offset, (long long)bytes, (long long)src_bytes);
    }
    hipStream_t st = (hipStream_t)stream;
    const int esize = out_dtype == DEVIAS_BF16 ? 2 : 4, VEC = 16 / esize;
    const bool vec = aligned16(out) && S_w % VEC == 0;                      // then every output row of every plane starts on 16 bytes
    for (int b0 = 0; b0 < B; b0 += DEVIAS_INGEST_ROWS_PER_LAUNCH) {
        const int n = B - b0 < DEVIAS_INGEST_ROWS_PER_LAUNCH ? B - b0 : DEVIAS_INGEST_ROWS_PER_LAUNCH;
        IngestTable tab;
        for (int k = 0; k < DEVIAS_INGEST_ROWS_PER_LAUNCH; ++k) tab.r[k] = rows[b0 + (k < n ? k : 0)];
        const uint8_t* s = (const uint8_t*)src;
        if (out_dtype == DEVIAS_BF16) { if (vec) launch_ingest<bf16, 8>(s, src_bytes, table, out, b0, n, T, S_h, S_w, tab, st); else launch_ingest<bf16, 1>(s, src_bytes, table, out, b0, n, T, S_h, S_w, tab, st); }
        else { if (vec) launch_ingest<float, 4>(s, src_bytes, table, out, b0, n, T, S_h, S_w, tab, st); else launch_ingest<float, 1>(s, src_bytes, table, out, b0, n, T, S_h, S_w, tab, st); }
        DEVIAS_CHECK_LAUNCH(who);
    }
    return DEVIAS_OK;
}
