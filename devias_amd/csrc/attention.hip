// Encoder multi-head self-attention core, host side: the devias_mhsa_* entry points -- validation, the choice of kernel form, counters and workspace arithmetic.
// The kernels and their launchers live in attn_fwd.hip, attn_mfma16.hip, attn_bwd1w.hip and attn_f32.hip; what they share, and the design, is in attn_common.h.
// Every entry point fills one AttnP (attn_common.h); forward and backward each validate it once, choose, launch.
#include "attn_common.h"

using namespace attn_units;

namespace {

// (the fields the host side derives are filled by attn_derive, after validation)
AttnP fwd_args(const void* qkv, void* o, float* lse, int32_t B, int32_t N, int32_t H, float scale, int32_t dtype, float keep, uint64_t seed, int32_t flags, void* stream) {
    return AttnP{qkv, o, nullptr, lse, nullptr, nullptr, B, N, H, scale, dtype, keep, seed, flags, nullptr, nullptr, nullptr, (hipStream_t)stream, 0, false, DropP{}, 0};
}
AttnP bwd_args(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, void* dqkv, int32_t B, int32_t N, int32_t H, float scale, int32_t dtype,
               float keep, uint64_t seed, int32_t flags, float* stat, void* stream) {
    return AttnP{qkv, const_cast<void*>(o), d_o, const_cast<float*>(lse), delta, dqkv, B, N, H, scale, dtype, keep, seed, flags, nullptr, nullptr, stat, (hipStream_t)stream,
                 0, false, DropP{}, 0};
}

inline int attn_npad(int N) { return (N + 31) & ~31; }
// xcd bit 0: XCD-aware linear grid (needs B*H % 8 == 0; option attn_xcd = 0 restores the plain 3-D grid).  Dropout: keep >= 1 is none; thresh = floor(keep * 2^32)
// (at most 2^32 - 1), seed = (s1 << 32) | s0
void attn_derive(AttnP& p) {
    p.xcd = (p.B << 16) | ((devias_options()[OPT_ATTN_XCD] && ((p.B * p.H) % 8 == 0)) ? 1 : 0) | ((p.flags & DEVIAS_ATTN_Q_PRESCALED) ? ATTN_QPRE : 0);
    p.npad = attn_npad(p.N);
    p.drop = p.keep < 1.0f;
    if (p.drop) {
        const double t = floor((double)p.keep * 4294967296.0);
        p.dp.thresh = t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
        p.dp.s0 = (uint32_t)p.seed; p.dp.s1 = (uint32_t)(p.seed >> 32);
        p.dp.inv_keep = 1.0f / p.keep;
    }
}

// Row statistics for the one-wave-per-SIMD dK / dV kernel (attn_bwd1w.hip): [B, H, Npad / 32, 2, 32] fp32 (per 32-query slice -lse * log2 e | -delta), Npad = N
// rounded up to a slice; written by the dQ kernel, streamed by LDS-DMA by the dK / dV kernel.
inline int64_t attn_stat_bytes(int B, int N, int H) { return (((int64_t)B * H * 2 * attn_npad(N) * 4) + 255) & ~(int64_t)255; }
// the q_bias / v_bias gradient partials of the bf16 backward kernels: one [H * 64] row per (batch entry, 128-row block)
inline int64_t attn_bias_part_bytes(int B, int N, int H) { return (((int64_t)B * cdiv(N, 128) * H * 64 * 4) + 255) & ~(int64_t)255; }
// (A one-wave-per-SIMD dQ kernel was built the same way and is SLOWER than the three-waves-per-SIMD kernel of attn_mfma16.hip after its vector-instruction diet -- 445 us
// against 337 per layer: tools/exp/attn_bwd1w_dq.hip.txt, profiles/r5_dkdv1w_development.txt.  One wave overlaps its own MFMAs and vector instructions only inside
// the MFMA's shadow; three waves overlap each other's.  The dK / dV kernel wins as one wave because its 128 accumulator registers leave no room for a second.)
// true = devias_mhsa_bwd* runs the one-wave-per-SIMD dK / dV kernel for this call (bf16, no attention dropout, option attn_dkdv != 0, room for the statistics)
inline bool attn_use_dkdv1w(int dtype, float keep) { return dtype == DEVIAS_BF16 && !(keep < 1.0f) && devias_options()[OPT_ATTN_DKDV] != 0; }

int mhsa_fwd(AttnP p) {
    DEVIAS_REQUIRE(p.qkv && p.o && p.lse && p.B > 0 && p.N > 0 && p.H > 0, "devias_mhsa_fwd: bad args");
    DEVIAS_REQUIRE(aligned16(p.qkv) && aligned16(p.o), "devias_mhsa_fwd: qkv/o must be 16-byte aligned");
    DEVIAS_REQUIRE(p.H <= 65535 && p.B <= 65535, "devias_mhsa_fwd: H and B must be <= 65535");
    DEVIAS_REQUIRE((p.flags & ~DEVIAS_ATTN_Q_PRESCALED) == 0 && (p.flags == 0 || p.dtype == DEVIAS_BF16), "devias_mhsa_fwd: bad flags %d (DEVIAS_ATTN_Q_PRESCALED: bf16 only)", p.flags);
    DEVIAS_REQUIRE(p.dtype == DEVIAS_BF16 || p.dtype == DEVIAS_F32, "devias_mhsa_fwd: bad dtype %d", p.dtype);
    attn_derive(p);
    if (p.dtype == DEVIAS_BF16) {
        const int cfg = devias_options()[OPT_ATTN_CFG];
        devias_count(DEVIAS_CNT_MHSA_FWD_BF16);
        if (p.xcd & ATTN_QPRE) devias_count(DEVIAS_CNT_MHSA_QPRE);
        launch_attn_fwd_bf16(cfg == 6 ? ATTN_FWD16 : cfg == 7 ? ATTN_FWD32_2W : ATTN_FWD32_4W, p);
    } else {
        devias_count(DEVIAS_CNT_MHSA_FWD_F32);
        launch_attn_fwd_f32(p);
    }
    DEVIAS_CHECK_LAUNCH("devias_mhsa_fwd");
    return DEVIAS_OK;
}

int mhsa_bwd(AttnP p) {
    DEVIAS_REQUIRE(p.qkv && p.o && p.d_o && p.lse && p.delta && p.dqkv && p.B > 0 && p.N > 0 && p.H > 0, "devias_mhsa_bwd: bad args");
    DEVIAS_REQUIRE(aligned16(p.qkv) && aligned16(p.o) && aligned16(p.d_o) && aligned16(p.dqkv), "devias_mhsa_bwd: unaligned pointer");
    DEVIAS_REQUIRE(p.H <= 65535 && p.B <= 65535, "devias_mhsa_bwd: H and B must be <= 65535");
    DEVIAS_REQUIRE((p.flags & ~DEVIAS_ATTN_Q_PRESCALED) == 0 && (p.flags == 0 || p.dtype == DEVIAS_BF16), "devias_mhsa_bwd: bad flags %d (DEVIAS_ATTN_Q_PRESCALED: bf16 only)", p.flags);
    DEVIAS_REQUIRE(p.dtype == DEVIAS_BF16 || p.dtype == DEVIAS_F32, "devias_mhsa_bwd: bad dtype %d", p.dtype);
    attn_derive(p);
    if (p.dtype == DEVIAS_F32) {
        devias_count(DEVIAS_CNT_MHSA_BWD_F32);
        launch_attn_bwd_dq_f32(p);
        DEVIAS_CHECK_LAUNCH("devias_mhsa_bwd(dq)");
        launch_attn_bwd_dkdv_f32(p);
        DEVIAS_CHECK_LAUNCH("devias_mhsa_bwd(dkdv)");
        return DEVIAS_OK;
    }
    const int* opt = devias_options();
    const int cfg = opt[OPT_ATTN_CFG];
    devias_count(DEVIAS_CNT_MHSA_BWD_BF16);
    if (p.xcd & ATTN_QPRE) devias_count(DEVIAS_CNT_MHSA_QPRE);
    // dK / dV by the one-wave-per-SIMD kernel when the caller gave room for the row statistics it streams (option attn_dkdv = 0: the two-waves-per-SIMD
    // kernel, which also serves attention dropout); otherwise the dQ kernel writes none
    const bool w1 = p.stat && attn_use_dkdv1w(p.dtype, p.keep);
    DEVIAS_REQUIRE(!(w1 && p.part_v), "devias_mhsa_bwd: the one-wave-per-SIMD dK / dV kernel emits no v_bias partials (internal)");
    if (!w1) p.stat = nullptr;
    // the dQ shapes of option attn_cfg emit no q_bias partials: a call that wants them gets the default shape
    launch_attn_bwd_dq_bf16(p.part_q ? ATTN_DQ_2x4 : cfg == 1 ? ATTN_DQ_4x2 : cfg == 2 ? ATTN_DQ_4x4 : cfg == 3 ? ATTN_DQ_2x2 : ATTN_DQ_2x4, p);
    DEVIAS_CHECK_LAUNCH("devias_mhsa_bwd(dq)");
    if (w1) {
        // attn_dkdv = 2: one persistent workgroup per CU instead of one per 256-key block (the kernel alone -2 %, the step +-0: DESIGN.md section 5 round 5)
        const int rc = devias_attn_dkdv1w_launch(p.qkv, p.d_o, p.stat, p.dqkv, p.B, p.N, p.npad, p.H, p.scale, p.xcd, opt[OPT_ATTN_DKDV] == 2, p.st);
        if (rc != DEVIAS_OK) return rc;
    } else {
        devias_count(DEVIAS_CNT_DKDV2W);
        launch_attn_bwd_dkdv2w_bf16(p);
    }
    DEVIAS_CHECK_LAUNCH("devias_mhsa_bwd(dkdv)");
    return DEVIAS_OK;
}

// Backward + the q_bias / v_bias gradients (the column sums of the dQ and dV thirds of dqkv over all B * N rows; modeling_slot.py:97-99).  bf16: the two kernels
// emit one [H * 64] partial per (batch entry, 128-row block) from their fp32 accumulators (bias_partials, attn_common.h) and the fixed-order second stage sums the
// B * ceil(N / 128) partials -- no pass over the stored tensor.  fp32 (parity mode): the plain backward followed by two column-sum passes.  ws_q / ws_v: scratch of
// devias_mhsa_bwd_bias_workspace_bytes() bytes each.  keep < 1: with the attention dropout of devias_mhsa_bwd_dropout.  (ABI 162)
int mhsa_bwd_bias(AttnP a, float* dbq, float* dbv, float* ws_q, float* ws_v) {
    DEVIAS_REQUIRE(dbq && ws_q && ws_v, "devias_mhsa_bwd_bias: null bias-gradient / workspace pointer");
    DEVIAS_REQUIRE(a.keep > 0.f && a.keep <= 1.f, "devias_mhsa_bwd_bias: keep must be in (0, 1]");
    DEVIAS_REQUIRE(!(a.flags != 0 && a.keep < 1.f), "devias_mhsa_bwd_bias_flags: DEVIAS_ATTN_Q_PRESCALED is not offered with attention dropout (no forward entry point takes both)");
    const int B = a.B, N = a.N, D = a.H * 64;
    if (attn_use_dkdv1w(a.dtype, a.keep)) {
        // One-wave-per-SIMD dK / dV kernel.  Its row statistics live behind the q partials in ws_q.  It emits no v partials: without dropout every softmax row sums
        // to one, so sum_keys dV = sum_keys sum_queries P dO = sum_queries dO -- the v_bias gradient IS the column sum of d_o.  A caller that has those column sums
        // from the producer of d_o (the projection's dgrad GEMM: devias_gemm's colsum epilogue, csrc/regions.hip) passes dbv = NULL; otherwise one pass over d_o here.
        a.part_q = ws_q;
        a.stat = reinterpret_cast<float*>(reinterpret_cast<char*>(ws_q) + attn_bias_part_bytes(B, N, a.H));
        const int rc = mhsa_bwd(a);
        if (rc != DEVIAS_OK) return rc;
        const int r1 = devias_colsum_finish(ws_q, B * cdiv(N, 128), D, dbq, 0.f, a.st);
        if (r1 != DEVIAS_OK || !dbv) return r1;
        return devias_colsum(a.d_o, a.dtype, B * N, D, D, dbv, 0.f, ws_v, a.st);
    }
    DEVIAS_REQUIRE(dbv, "devias_mhsa_bwd_bias: dbv may be NULL only where devias_mhsa_bwd_bias_dv_from_do() says so");
    if (a.dtype == DEVIAS_BF16 && devias_options()[OPT_ATTN_BIAS_FUSED]) {
        a.part_q = ws_q; a.part_v = ws_v;
        const int rc = mhsa_bwd(a);
        if (rc != DEVIAS_OK) return rc;
        const int rows = B * cdiv(N, 128);
        const int r1 = devias_colsum_finish(ws_q, rows, D, dbq, 0.f, a.st);
        return r1 != DEVIAS_OK ? r1 : devias_colsum_finish(ws_v, rows, D, dbv, 0.f, a.st);
    }
    const int rc = mhsa_bwd(a);
    if (rc != DEVIAS_OK) return rc;
    const int64_t es = a.dtype == DEVIAS_BF16 ? 2 : 4;
    const int r1 = devias_colsum(a.dqkv, a.dtype, B * N, D, 3 * D, dbq, 0.f, ws_q, a.st);
    return r1 != DEVIAS_OK ? r1 : devias_colsum(static_cast<const char*>(a.dqkv) + (int64_t)2 * D * es, a.dtype, B * N, D, 3 * D, dbv, 0.f, ws_v, a.st);
}

}  // namespace

extern "C" int devias_mhsa_fwd(const void* qkv, void* o, float* lse, int32_t B, int32_t N, int32_t H, float scale,
                               int32_t dtype, void* stream) {
    return mhsa_fwd(fwd_args(qkv, o, lse, B, N, H, scale, dtype, 1.0f, 0, 0, stream));
}
extern "C" int devias_mhsa_fwd_flags(const void* qkv, void* o, float* lse, int32_t B, int32_t N, int32_t H, float scale,
                                     int32_t dtype, int32_t flags, void* stream) {
    return mhsa_fwd(fwd_args(qkv, o, lse, B, N, H, scale, dtype, 1.0f, 0, flags, stream));
}
extern "C" int devias_mhsa_fwd_dropout(const void* qkv, void* o, float* lse, int32_t B, int32_t N, int32_t H, float scale,
                                       int32_t dtype, float keep, uint64_t seed, void* stream) {
    DEVIAS_REQUIRE(keep > 0.f && keep <= 1.f, "devias_mhsa_fwd_dropout: keep must be in (0, 1]");
    return mhsa_fwd(fwd_args(qkv, o, lse, B, N, H, scale, dtype, keep, seed, 0, stream));
}

// The workspace of devias_mhsa_bwd / _flags: the row statistics of the one-wave-per-SIMD dK / dV kernel.  (ABI 140's single-pass backward needed one too; ABI 150
// removed that kernel -- see DESIGN.md -- and needed none; the query stayed for hosts written against the older header and has a use again.)
extern "C" int64_t devias_mhsa_bwd_workspace_bytes(int32_t B, int32_t N, int32_t H) { return attn_stat_bytes(B, N, H); }
extern "C" int devias_mhsa_bwd(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, void* dqkv,
                               int32_t B, int32_t N, int32_t H, float scale, int32_t dtype, void* ws, void* stream) {
    DEVIAS_REQUIRE(!ws || aligned16(ws), "devias_mhsa_bwd: unaligned workspace");
    return mhsa_bwd(bwd_args(qkv, o, d_o, lse, delta, dqkv, B, N, H, scale, dtype, 1.0f, 0, 0, (float*)ws, stream));
}
extern "C" int devias_mhsa_bwd_flags(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, void* dqkv,
                                     int32_t B, int32_t N, int32_t H, float scale, int32_t dtype, void* ws, int32_t flags, void* stream) {
    DEVIAS_REQUIRE(!ws || aligned16(ws), "devias_mhsa_bwd: unaligned workspace");
    return mhsa_bwd(bwd_args(qkv, o, d_o, lse, delta, dqkv, B, N, H, scale, dtype, 1.0f, 0, flags, (float*)ws, stream));
}
extern "C" int devias_mhsa_bwd_dropout(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, void* dqkv,
                                       int32_t B, int32_t N, int32_t H, float scale, int32_t dtype, float keep, uint64_t seed, void* stream) {
    DEVIAS_REQUIRE(keep > 0.f && keep <= 1.f, "devias_mhsa_bwd_dropout: keep must be in (0, 1]");
    return mhsa_bwd(bwd_args(qkv, o, d_o, lse, delta, dqkv, B, N, H, scale, dtype, keep, seed, 0, nullptr, stream));
}

extern "C" int64_t devias_mhsa_bwd_bias_workspace_bytes(int32_t B, int32_t N, int32_t H) {
    const int64_t a = attn_bias_part_bytes(B, N, H) + attn_stat_bytes(B, N, H), c = devias_colsum_workspace_bytes(B * N, H * 64);
    return a > c ? a : c;
}
extern "C" int32_t devias_mhsa_bwd_bias_dv_from_do(int32_t dtype, float keep) { return attn_use_dkdv1w(dtype, keep) ? 1 : 0; }
extern "C" int devias_mhsa_bwd_bias(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, void* dqkv, int32_t B, int32_t N, int32_t H,
                                    float scale, int32_t dtype, float keep, uint64_t seed, float* dbq, float* dbv, float* ws_q, float* ws_v, void* stream) {
    return mhsa_bwd_bias(bwd_args(qkv, o, d_o, lse, delta, dqkv, B, N, H, scale, dtype, keep, seed, 0, nullptr, stream), dbq, dbv, ws_q, ws_v);
}
extern "C" int devias_mhsa_bwd_bias_flags(const void* qkv, const void* o, const void* d_o, const float* lse, float* delta, void* dqkv, int32_t B, int32_t N, int32_t H,
                                          float scale, int32_t dtype, float keep, uint64_t seed, float* dbq, float* dbv, float* ws_q, float* ws_v, int32_t flags, void* stream) {
    return mhsa_bwd_bias(bwd_args(qkv, o, d_o, lse, delta, dqkv, B, N, H, scale, dtype, keep, seed, flags, nullptr, stream), dbq, dbv, ws_q, ws_v);
}
