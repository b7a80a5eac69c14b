// The attention kernels on 16x16x32 MFMAs (bf16; shared pieces and the layout of the attention units: attn_common.h).  In all three the score tile is computed so
// that a query (forward, dQ) resp. a key (dK / dV) is a lane COLUMN, and the operand tiles of 64 rows arrive by LDS-DMA into a two-stage ring, one barrier per tile:
//   mhsa_fwd_bf16_kernel       forward, QT 16-query tiles per wave (option attn_cfg = 6; the default forward is the 32x32x16 kernel of attn_fwd.hip)
//   mhsa_bwd_dq_bf16_kernel    backward dQ; also delta = rowsum(dO * O), the row statistics the one-wave-per-SIMD dK / dV kernel streams (attn_bwd1w.hip) and, on
//                              request, the q_bias gradient partials.  Five instantiations <16-query tiles per wave, waves> (option attn_cfg)
//   mhsa_bwd_dkdv_bf16_kernel  backward dK / dV, two waves per SIMD: workgroup = 4 waves x 32 keys, K / V fragments resident in registers.  The form of rounds 2-4: it
//                              serves option attn_dkdv = 0, attention dropout and the fused v_bias partials; the default is the kernel of attn_bwd1w.hip
// and one host launcher each.  They share a unit because their code depends on it: the compiler specialises the helpers of attn_common.h for the callers it sees in
// a unit, and the forward and the dK / dV kernel compile to other code without the dQ kernel beside them ("The attention's files").
#include "attn_common.h"
#include <type_traits>

using namespace attn_units;

namespace {

// ======================================= forward (bf16), 16x16x32 MFMAs ====================================
template <int QT, int NW>
__global__ __launch_bounds__(NW * 64, 1) void mhsa_fwd_bf16_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ o,
                                                          float* __restrict__ lse, int N, int H, float scale, int xcd) {
    __shared__ __attribute__((aligned(16))) char smem[32768];   // two stages of (K row image | V transposed-read image)
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const HeadMap hm = head_map((N + NW * 16 * QT - 1) / (NW * 16 * QT), H, xcd >> 16, (xcd & 1) != 0);
    const int h = hm.h, b = hm.b;
    const int D = H * 64;
    const int64_t RS = 3 * (int64_t)D;
    const bf16* base = qkv + (int64_t)b * N * RS + h * 64;
    const int q0 = hm.blk * (NW * 16 * QT) + wave * (16 * QT);
    const float sl2 = (xcd & ATTN_QPRE) ? 1.0f : scale * LOG2E;      // (Q already holds q * scale * log2 e: DEVIAS_ATTN_Q_PRESCALED)

    bf16x8 qf[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        int q = min(q0 + 16 * qt + c, N - 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            qf[qt][ks] = *reinterpret_cast<const bf16x8*>(base + (int64_t)q * RS + 32 * ks + 8 * g);
    }
    f32x4 acc_o[4][QT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < QT; ++j) acc_o[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrow[QT], lrow[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) { mrow[j] = -INFINITY; lrow[j] = 0.f; }

    const int nkv = (N + 63) / 64;
    TileDma<NW, 0> dK;
    TileDma<NW, 1> dV;
    {
        const int64_t left = ((int64_t)(xcd >> 16) - b) * N * RS - h * 64;      // elements from `base` to the end of qkv
        dK.init(base + D, RS, left - D, wave, lane);
        dV.init(base + 2 * D, RS, left - 2 * D, wave, lane);
        dK.issue(0, smem, wave);
        dV.issue(0, smem + 8192, wave);
    }
    for (int t = 0; t < nkv; ++t) {
        // one barrier per tile: tile t has landed for every wave, and everyone is done reading tile t-1's stage
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* imgK = smem + (t & 1) * 16384;      // row image of K tile  [key][d]
        const char* imgV = imgK + 8192;                 // transposed-read image of V tile [key][d]
        if (t + 1 < nkv) {
            char* nxt = smem + ((t + 1) & 1) * 16384;
            dK.issue((t + 1) * 64, nxt, wave);
            dV.issue((t + 1) * 64, nxt + 8192, wave);
        }
        // a wave whose 16*QT queries all lie beyond N (the last workgroup of a head at N = 1568: 3 of its 4 waves) has staged its share of the
        // tile and takes part in the barrier; it leaves the matrix cores to the co-resident workgroups
        if (q0 >= N) continue;
        // S^T tile: acc_s[kt][qt] holds keys 16kt + 4g + r (rows) x query c (col)
        f32x4 acc_s[4][QT];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < QT; ++j) acc_s[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                bf16x8 kf = frag_rows(imgK, 16 * kt, ks, lane);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) acc_s[kt][qt] = mfma(kf, qf[qt][ks], acc_s[kt][qt]);
            }
        const int k0 = t * 64;
        if (k0 + 64 > N) {                    // ragged last tile only (wave-uniform branch): mask keys >= N
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (k0 + 16 * kt + 4 * g + r >= N) {
#pragma unroll
                        for (int qt = 0; qt < QT; ++qt) acc_s[kt][qt][r] = -INFINITY;
                    }
        }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
            // running max is kept in RAW score units; scale*log2(e) is folded into the exponent's FMA
            // chains of max(max(m, a), b): each pair folds into one v_max3_f32
            float mx = fmaxf(fmaxf(acc_s[0][qt][0], acc_s[0][qt][1]), acc_s[0][qt][2]);
            mx = fmaxf(fmaxf(mx, acc_s[0][qt][3]), acc_s[1][qt][0]);
            mx = fmaxf(fmaxf(mx, acc_s[1][qt][1]), acc_s[1][qt][2]);
            float mx2 = fmaxf(fmaxf(acc_s[1][qt][3], acc_s[2][qt][0]), acc_s[2][qt][1]);
            mx2 = fmaxf(fmaxf(mx2, acc_s[2][qt][2]), acc_s[2][qt][3]);
            mx2 = fmaxf(fmaxf(mx2, acc_s[3][qt][0]), acc_s[3][qt][1]);
            mx = fmaxf(fmaxf(mx, acc_s[3][qt][2]), acc_s[3][qt][3]);
            mx = fmaxf(mx, mx2);
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            if (__any(mx > mrow[qt])) {       // some row's max grew: rescale (rare after the first tiles)
                const float mnew = fmaxf(mrow[qt], mx);
                const float alpha = fast_exp2((mrow[qt] - mnew) * sl2);
                mrow[qt] = mnew;
                lrow[qt] *= alpha;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) acc_o[dt][qt] *= alpha;
            }
            const float nb = -mrow[qt] * sl2;
            const f32x2 sl2v = {sl2, sl2}, nbv = {nb, nb};
            f32x2 ps2 = {0.f, 0.f};                       // packed fp32: one v_pk_fma_f32 / v_pk_add_f32 per two scores
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; r += 2) {
                    const f32x2 e = f32x2{acc_s[kt][qt][r], acc_s[kt][qt][r + 1]} * sl2v + nbv;
                    const f32x2 p = {fast_exp2(e[0]), fast_exp2(e[1])};
                    acc_s[kt][qt][r] = p[0]; acc_s[kt][qt][r + 1] = p[1];
                    ps2 += p;
                }
            lrow[qt] += ps2[0] + ps2[1];
        }
        // O^T += V^T P^T
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 pf[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) pf[qt] = pack8(acc_s[2 * s][qt], acc_s[2 * s + 1][qt]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                bf16x8 vf = frag_tr(imgV, 16 * dt, s, lane);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) acc_o[dt][qt] = mfma(vf, pf[qt], acc_o[dt][qt]);
            }
        }
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        float l = lrow[qt];
        l += __shfl_xor(l, 16, 64);
        l += __shfl_xor(l, 32, 64);
        const int q = q0 + 16 * qt + c;
        if (q < N) {
            const float inv = 1.0f / l;
            bf16* orow = o + ((int64_t)b * N + q) * D + h * 64 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) store4(orow + 16 * dt, acc_o[dt][qt] * inv);
            if (g == 0) lse[((int64_t)b * H + h) * N + q] = (mrow[qt] * sl2 + log2f(l)) * LN2;
        }
    }
}

// ======================================= backward dQ (bf16) ==============================================
template <int QT, int NW, bool DROP = false>
__global__ __launch_bounds__(NW * 64) void mhsa_bwd_dq_bf16_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ o,
                                                               const bf16* __restrict__ d_o, const float* __restrict__ lse,
                                                               float* __restrict__ delta, bf16* __restrict__ dqkv,
                                                               int N, int H, float scale, int xcd, DropP drop = DropP{}, float* __restrict__ part_q = nullptr,
                                                               float* __restrict__ stat = nullptr, int Npad = 0) {
    __shared__ __attribute__((aligned(16))) char smem[32768];     // two stages of (K image | V image), filled by LDS-DMA one tile ahead
    // per stage: K, one image for both uses -- row reads (S^T = K Q^T) and transposed reads (dQ^T = K^T dS^T) -- | V rows (dP^T = V dO^T)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
    const HeadMap hm = head_map((N + NW * 16 * QT - 1) / (NW * 16 * QT), H, xcd >> 16, (xcd & 1) != 0);
    const int h = hm.h, b = hm.b;
    const int D = H * 64;
    const int64_t RS = 3 * (int64_t)D;
    const bf16* base = qkv + (int64_t)b * N * RS + h * 64;
    const int q0 = hm.blk * (NW * 16 * QT) + wave * (16 * QT);
    const float sl2 = (xcd & ATTN_QPRE) ? 1.0f : scale * LOG2E;      // (Q already holds q * scale * log2 e: DEVIAS_ATTN_Q_PRESCALED)

    bf16x8 qf[QT][2], dof[QT][2];
    float lse2[QT], dl[QT];
    uint32_t rowkey[QT];                                               // DROP: the mask rows of this lane's queries
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        int q = min(q0 + 16 * qt + c, N - 1);
        rowkey[qt] = DROP ? drop_rowkey(drop, (uint32_t)(b * H + h), (uint32_t)q) : 0u;
        const bf16* orow = o + ((int64_t)b * N + q) * D + h * 64;
        const bf16* dorow = d_o + ((int64_t)b * N + q) * D + h * 64;
        float part = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[qt][ks] = *reinterpret_cast<const bf16x8*>(base + (int64_t)q * RS + 32 * ks + 8 * g);
            dof[qt][ks] = *reinterpret_cast<const bf16x8*>(dorow + 32 * ks + 8 * g);
            bf16x8 of = *reinterpret_cast<const bf16x8*>(orow + 32 * ks + 8 * g);
#pragma unroll
            for (int j = 0; j < 8; ++j) part += (float)dof[qt][ks][j] * (float)of[j];
        }
        part += __shfl_xor(part, 16, 64);
        part += __shfl_xor(part, 32, 64);
        dl[qt] = part;
        lse2[qt] = lse[((int64_t)b * H + h) * N + q] * LOG2E;
        if constexpr (!DROP) {                                        // Q pre-multiplied by scale * log2 e (as the forward kernel does): with the row constants below no per-score arithmetic is left before the v_exp
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int j = 0; j < 8; ++j) qf[qt][ks][j] = (bf16)((float)qf[qt][ks][j] * sl2);
        }
        if (g == 0 && q0 + 16 * qt + c < N) delta[((int64_t)b * H + h) * N + q] = part;
        // the row statistics in the form the one-wave-per-SIMD dK / dV kernel (attn_bwd1w.hip) streams them by LDS-DMA: [B, H, Npad / 32, 2, 32], per 32-query
        // slice -lse * log2 e | -delta, the padding rows N .. Npad - 1 as -inf | 0 (their probabilities are then exactly zero without masking code)
        if (stat && g == 0 && q0 + 16 * qt + c < Npad) {
            const int qq = q0 + 16 * qt + c;
            const bool in = qq < N;
            float* sp = stat + ((int64_t)b * H + h) * 2 * Npad + (qq >> 5) * 64 + (qq & 31);
            sp[0] = in ? -lse2[qt] : -INFINITY;
            sp[32] = in ? -part : 0.f;
        }
    }
    f32x4 acc_dq[4][QT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < QT; ++j) acc_dq[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 cl4[QT], cd4[QT];                                           // the row constants as MFMA C operands (no dropout)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) { cl4[qt] = f32x4{-lse2[qt], -lse2[qt], -lse2[qt], -lse2[qt]}; cd4[qt] = f32x4{-dl[qt], -dl[qt], -dl[qt], -dl[qt]}; }

    const int nkv = (N + 63) / 64;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    TileDma<NW, 1> dK;
    TileDma<NW, 0> dV;
    {
        const int64_t left = ((int64_t)(xcd >> 16) - b) * N * RS - h * 64;      // elements from `base` to the end of qkv
        dK.init(base + D, RS, left - D, wv, lane);
        dV.init(base + 2 * D, RS, left - 2 * D, wv, lane);
    }
    dK.issue(0, smem, wv);
    dV.issue(0, smem + 8192, wv);
    // (two tiles per trip, the LDS stage a compile-time constant in each: every fragment address is then lane offset + immediate -- the run-time stage cost ~36
    // vector instructions of address arithmetic per tile, in a kernel bound by vector issue)
    auto tile = [&](int t, auto STG) {
        // one barrier per tile: tile t has landed for every wave, and everyone is done reading tile t-1's stage (rows past N re-read row N-1:
        // finite data whose probabilities are exactly zero)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* imgKt = smem + decltype(STG)::value * 16384;
        const char* imgV = imgKt + 8192;
        if (t + 1 < nkv) {
            char* nxt = smem + (1 - decltype(STG)::value) * 16384;
            dK.issue((t + 1) * 64, nxt, wv);
            dV.issue((t + 1) * 64, nxt + 8192, wv);
        }
        if (q0 < N) {                         // (waves without a valid query only stage and synchronise: see the forward kernel)
        // The 64-key tile in two halves of 32 keys (16-key tiles kt = 2s, 2s + 1), each run to completion -- S^T and dP^T (8 QT MFMAs), the softmax arithmetic,
        // dQ^T += K^T dS^T (4 QT MFMAs) -- so that only HALF a tile of scores and dP is ever live: 32 registers fewer than the whole-tile form, which is what
        // takes the kernel from 194 to 162 registers = three waves per SIMD instead of two: -6.5 % on the kernel, -0.32 ms on the step.  Same MFMAs on the same operands in the same accumulation order:
        // bitwise equal to the whole-tile form.
        const int k0 = t * 64;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            // Without dropout the row constants ride in the MFMAs' C operand (a query is a lane COLUMN of these tiles: the constant is the same in all four
            // accumulator registers): S' = s * scale * log2 e - lse2 and dP - delta come out of the matrix cores, and a score costs v_exp, v_mul and half a
            // v_cvt_pk instead of six vector instructions (these kernels are bound by vector issue, profiles/r3_attn_pmc.txt)
            f32x4 acc_s[2][QT], acc_dp[2][QT];
            if constexpr (DROP) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < QT; ++j) { acc_s[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; acc_dp[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const int kt = 2 * s + h2;
                    bf16x8 kf = frag_rows_tr(imgKt, 16 * kt, ks, lane);
                    bf16x8 vf = frag_rows(imgV, 16 * kt, ks, lane);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) {
                        if (!DROP && ks == 0) {
                            acc_s[h2][qt] = mfma(kf, qf[qt][ks], cl4[qt]);
                            acc_dp[h2][qt] = mfma(vf, dof[qt][ks], cd4[qt]);
                        } else {
                            acc_s[h2][qt] = mfma(kf, qf[qt][ks], acc_s[h2][qt]);
                            acc_dp[h2][qt] = mfma(vf, dof[qt][ks], acc_dp[h2][qt]);
                        }
                    }
                }
            if (k0 + 64 > N) {                // ragged last tile only: p = exp2(-inf) = 0 for keys >= N
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (k0 + 16 * (2 * s + h2) + 4 * g + r >= N) {
#pragma unroll
                            for (int qt = 0; qt < QT; ++qt) acc_s[h2][qt][r] = -INFINITY;
                        }
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                const f32x2 sl2v = {sl2, sl2}, nl = {-lse2[qt], -lse2[qt]}, dlv = {dl[qt], dl[qt]};   // packed fp32: two scores per VALU op
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
#pragma unroll
                        for (int u = 0; u < 2; ++u) {                  // (scalar on purpose: packed fp32 instructions beside MFMAs cost more issue time than the two they replace)
                            if constexpr (!DROP) {
                                acc_s[h2][qt][r + u] = fast_exp2(acc_s[h2][qt][r + u]) * acc_dp[h2][qt][r + u];                            // p (dP - delta) = dS^T / scale
                            } else {
                            const float p1 = fast_exp2(acc_s[h2][qt][r + u] * sl2v[0] + nl[0]);
                            float dp1 = acc_dp[h2][qt][r + u];
                            dp1 *= drop_scale(drop, rowkey[qt], (uint32_t)(k0 + 16 * (2 * s + h2) + 4 * g + r + u));   // dP_ij = mask_ij (dO_i . V_j)
                            acc_s[h2][qt][r + u] = p1 * (dp1 - dlv[0]);                                                                     // dS^T / scale (scale applied once at the end)
                            }
                        }
                    }
            }
            bf16x8 dsf[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) dsf[qt] = pack8(acc_s[0][qt], acc_s[1][qt]);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                bf16x8 kf = frag_tr(imgKt, 16 * dt, s, lane);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) acc_dq[dt][qt] = mfma(kf, dsf[qt], acc_dq[dt][qt]);
            }
        }
        }
    };
    for (int t = 0; t < nkv; t += 2) {
        tile(t, std::integral_constant<int, 0>{});
        if (t + 1 < nkv) tile(t + 1, std::integral_constant<int, 1>{});
    }
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
        const int q = q0 + 16 * qt + c;
        if (q < N) {
            bf16* row = dqkv + ((int64_t)b * N + q) * RS + h * 64 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) store4(row + 16 * dt, acc_dq[dt][qt] * scale);
        }
    }
    if (part_q) {                                                 // (workgroup-uniform) q_bias gradient partials
        __syncthreads();                                          // every wave is done with the last tile's LDS stage
        // everything the epilogue needs is derived again from the (laundered) ids: nothing of it stays live across the key loop, whose register budget
        // (three waves per SIMD) and schedule are then those of the kernel without the epilogue
        int bid = blockIdx.x, by = blockIdx.y, bz = blockIdx.z, t2 = threadIdx.x;
        asm volatile("" : "+s"(bid), "+s"(by), "+s"(bz), "+v"(t2));
        const int nblk = (N + NW * 16 * QT - 1) / (NW * 16 * QT);
        int blk2, h2, b2;
        if (xcd & 1) { const int x = bid & 7, slot = bid >> 3, hidx = (slot / nblk) * 8 + x; blk2 = slot - (slot / nblk) * nblk; h2 = hidx % H; b2 = hidx / H; }
        else { blk2 = bid; h2 = by; b2 = bz; }
        const int lane2 = t2 & 63, wave2 = t2 >> 6, q02 = blk2 * (NW * 16 * QT) + wave2 * (16 * QT);
        bool valid[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) valid[qt] = q02 + 16 * qt + (lane2 & 15) < N;
        bias_partials<QT>(acc_dq, valid, scale, smem, part_q, ((int64_t)b2 * nblk + blk2) * (H * 64) + h2 * 64, t2, lane2, wave2);
    }
}

// ======================================= backward dK, dV (bf16) ==========================================
// KT = 16-key tiles per wave.  2 = 32 keys per wave, 128 per workgroup, 252 registers, two waves per SIMD: the shipped form.  1 (16 / 64 keys: 114 registers, four
// waves per SIMD) was measured and is not instantiated: the step is 0.38 ms SLOWER -- every wave still streams the whole Q / dO tile through LDS for half the
// keys (profiles/r4_attn_occupancy.txt)
template <bool DROP = false, int KT = 2>
__global__ __launch_bounds__(256) void mhsa_bwd_dkdv_bf16_kernel(const bf16* __restrict__ qkv, const bf16* __restrict__ d_o,
                                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                                 bf16* __restrict__ dqkv, int N, int H, float scale, int xcd, DropP drop = DropP{}, float* __restrict__ part_v = nullptr) {
    __shared__ __attribute__((aligned(16))) char smem[2 * 16384 + 2 * 512];   // two stages of (Q image | dO image) filled by LDS-DMA one tile ahead, + their row statistics
    char* imgQt = smem;             // Q, one image: row reads (S = Q K^T) and transposed reads (dK^T = Q^T dS)
    char* imgOt = smem + 8192;      // dO, one image: row reads (dP = dO V^T) and transposed reads (dV^T = dO^T P)
    float* s_stat = reinterpret_cast<float*>(smem + 32768);  // per stage: [64] log2-domain logsumexp (+inf for invalid rows) | [64] delta
    const float* s_lse = s_stat;
    const float* s_dl = s_stat + 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
    const HeadMap hm = head_map((N + 64 * KT - 1) / (64 * KT), H, xcd >> 16, (xcd & 1) != 0);
    const int h = hm.h, b = hm.b;
    const int D = H * 64;
    const int64_t RS = 3 * (int64_t)D;
    const bf16* base = qkv + (int64_t)b * N * RS + h * 64;
    const bf16* dobase = d_o + (int64_t)b * N * D + h * 64;
    const int key0 = hm.blk * (64 * KT) + wave * (16 * KT);
    const float sl2 = (xcd & ATTN_QPRE) ? 1.0f : scale * LOG2E;      // (Q already holds q * scale * log2 e: DEVIAS_ATTN_Q_PRESCALED)

    bf16x8 kreg[KT][2], vreg[KT][2];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        int key = min(key0 + 16 * kt + c, N - 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            kreg[kt][ks] = *reinterpret_cast<const bf16x8*>(base + D + (int64_t)key * RS + 32 * ks + 8 * g);
            vreg[kt][ks] = *reinterpret_cast<const bf16x8*>(base + 2 * D + (int64_t)key * RS + 32 * ks + 8 * g);
        }
    }
    f32x4 acc_dk[4][KT], acc_dv[4][KT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < KT; ++j) { acc_dk[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; acc_dv[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    const int nq = (N + 63) / 64;
    const float* lse_bh = lse + ((int64_t)b * H + h) * N;
    const float* dl_bh = delta + ((int64_t)b * H + h) * N;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    // row statistics of query tile r0 / 64 for thread tid < 128 (rows past N: p = exp2(-inf) = 0 whatever the re-read Q / dO rows hold)
    auto stat_load = [&](int r0) -> float {
        if (tid < 64) return r0 + tid < N ? lse_bh[r0 + tid] * LOG2E : INFINITY;
        return r0 + tid - 64 < N ? dl_bh[r0 + tid - 64] : 0.f;
    };
    float rstat = 0.f;
    TileDma<4, 1> dQ_, dO_;
    dQ_.init(base, RS, ((int64_t)(xcd >> 16) - b) * N * RS - h * 64, wv, lane);
    dO_.init(dobase, D, ((int64_t)(xcd >> 16) - b) * N * D - h * 64, wv, lane);
    dQ_.issue(0, smem, wv);
    dO_.issue(0, smem + 8192, wv);
    if (tid < 128) {
        s_stat[tid] = stat_load(0);
        if (nq > 1) rstat = stat_load(64);      // always one tile ahead of the LDS copy
    }
    for (int t = 0; t < nq; ++t) {
        // one barrier per tile: tile t (images by LDS-DMA, statistics by the ds_write below / above) is complete for every wave, and
        // everyone is done reading tile t-1's stage
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        imgQt = smem + (t & 1) * 16384;
        imgOt = imgQt + 8192;
        s_lse = s_stat + (t & 1) * 128;
        s_dl = s_lse + 64;
        if (t + 1 < nq) {
            char* nxt = smem + ((t + 1) & 1) * 16384;
            dQ_.issue((t + 1) * 64, nxt, wv);
            dO_.issue((t + 1) * 64, nxt + 8192, wv);
            if (tid < 128) {
                s_stat[((t + 1) & 1) * 128 + tid] = rstat;
                if (t + 2 < nq) rstat = stat_load((t + 2) * 64);
            }
        }
        if (key0 < N) {                       // (waves without a valid key only stage and synchronise: see the forward kernel)
        // S and dP tiles: acc[qt][kt] holds queries 16qt + 4g + r (rows) x key c (col)
        f32x4 acc_s[4][KT], acc_dp[4][KT];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < KT; ++j) { acc_s[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; acc_dp[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int qt = 0; qt < 4; ++qt) {
                bf16x8 qfr = frag_rows_tr(imgQt, 16 * qt, ks, lane);
                bf16x8 dofr = frag_rows_tr(imgOt, 16 * qt, ks, lane);
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    acc_s[qt][kt] = mfma(qfr, kreg[kt][ks], acc_s[qt][kt]);
                    acc_dp[qt][kt] = mfma(dofr, vreg[kt][ks], acc_dp[qt][kt]);
                }
            }
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            const f32x4 l4 = *reinterpret_cast<const f32x4*>(s_lse + 16 * qt + 4 * g);
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(s_dl + 16 * qt + 4 * g);
            const f32x2 sl2v = {sl2, sl2};
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; r += 2) {                                    // packed fp32: two scores per VALU op
#pragma unroll
                    for (int u = 0; u < 2; ++u) {                      // (scalar on purpose: see the dQ kernel)
                        const float p1 = fast_exp2(acc_s[qt][kt][r + u] * sl2v[0] - l4[r + u]);
                        float dp1 = acc_dp[qt][kt][r + u], pd1 = p1;
                        if constexpr (DROP) {                          // query 64 t + 16 qt + 4 g + r + u, key key0 + 16 kt + c: dV takes P * mask, dP = mask (dO . V)
                            const float m1 = drop_scale(drop, drop_rowkey(drop, (uint32_t)(b * H + h), (uint32_t)min(t * 64 + 16 * qt + 4 * g + r + u, N - 1)), (uint32_t)(key0 + 16 * kt + c));
                            dp1 *= m1; pd1 = p1 * m1;
                        }
                        acc_s[qt][kt][r + u] = pd1;
                        acc_dp[qt][kt][r + u] = p1 * (dp1 - d4[r + u]);                                          // dS / scale
                    }
                }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 pf[KT], dsf[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                pf[kt] = pack8(acc_s[2 * s][kt], acc_s[2 * s + 1][kt]);
                dsf[kt] = pack8(acc_dp[2 * s][kt], acc_dp[2 * s + 1][kt]);
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                bf16x8 dot = frag_tr(imgOt, 16 * dt, s, lane);
                bf16x8 qt_ = frag_tr(imgQt, 16 * dt, s, lane);
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    acc_dv[dt][kt] = mfma(dot, pf[kt], acc_dv[dt][kt]);
                    acc_dk[dt][kt] = mfma(qt_, dsf[kt], acc_dk[dt][kt]);
                }
            }
        }
        }
    }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        const int key = key0 + 16 * kt + c;
        if (key < N) {
            bf16* row = dqkv + ((int64_t)b * N + key) * RS + h * 64 + 4 * g;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                store4(row + D + 16 * dt, acc_dk[dt][kt] * ((xcd & ATTN_QPRE) ? LN2 : scale));      // (dK = scale dS^T q = ln 2 dS^T q' with q' = q scale log2 e)
                store4(row + 2 * D + 16 * dt, acc_dv[dt][kt]);
            }
        }
    }
    if (part_v) {                                                 // (workgroup-uniform) v_bias gradient partials (ids derived again: see the dQ kernel)
        __syncthreads();
        int bid = blockIdx.x, by = blockIdx.y, bz = blockIdx.z, t2 = threadIdx.x;
        asm volatile("" : "+s"(bid), "+s"(by), "+s"(bz), "+v"(t2));
        const int nblk = (N + 64 * KT - 1) / (64 * KT);
        int blk2, h2, b2;
        if (xcd & 1) { const int x = bid & 7, slot = bid >> 3, hidx = (slot / nblk) * 8 + x; blk2 = slot - (slot / nblk) * nblk; h2 = hidx % H; b2 = hidx / H; }
        else { blk2 = bid; h2 = by; b2 = bz; }
        const int lane2 = t2 & 63, wave2 = t2 >> 6, key02 = blk2 * (64 * KT) + wave2 * (16 * KT);
        bool valid[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) valid[kt] = key02 + 16 * kt + (lane2 & 15) < N;
        bias_partials<KT>(acc_dv, valid, 1.0f, smem, part_v, ((int64_t)b2 * nblk + blk2) * (H * 64) + h2 * 64, t2, lane2, wave2);
    }
}

}  // namespace

namespace attn_units {

void launch_attn_fwd16_bf16(const AttnP& p) {
    hipLaunchKernelGGL((mhsa_fwd_bf16_kernel<2, 4>), attn_grid(p, 128), dim3(256), 0, p.st, (const bf16*)p.qkv, (bf16*)p.o, p.lse, p.N, p.H, p.scale, p.xcd);
}

void launch_attn_bwd_dq_bf16(AttnDqForm form, const AttnP& p) {
    // <QT, NW>: 16 QT NW queries per workgroup, 64 NW threads
#define DQ_LAUNCH(QT, NW, DROP) hipLaunchKernelGGL((mhsa_bwd_dq_bf16_kernel<QT, NW, DROP>), attn_grid(p, 16 * QT * NW), dim3(64 * NW), 0, p.st, (const bf16*)p.qkv, (const bf16*)p.o, \
                                                   (const bf16*)p.d_o, p.lse, p.delta, (bf16*)p.dqkv, p.N, p.H, p.scale, p.xcd, p.dp, p.part_q, p.stat, p.npad)
    if (p.drop) DQ_LAUNCH(2, 4, true);
    else if (form == ATTN_DQ_4x2) DQ_LAUNCH(4, 2, false);
    else if (form == ATTN_DQ_4x4) DQ_LAUNCH(4, 4, false);
    else if (form == ATTN_DQ_2x2) DQ_LAUNCH(2, 2, false);
    else DQ_LAUNCH(2, 4, false);
#undef DQ_LAUNCH
}

void launch_attn_bwd_dkdv2w_bf16(const AttnP& p) {
#define DKDV_LAUNCH(DROP) hipLaunchKernelGGL(mhsa_bwd_dkdv_bf16_kernel<DROP>, attn_grid(p, 128), dim3(256), 0, p.st, (const bf16*)p.qkv, (const bf16*)p.d_o, p.lse, p.delta, \
                                             (bf16*)p.dqkv, p.N, p.H, p.scale, p.xcd, p.dp, p.part_v)      /* KT = 2: 128 keys per workgroup */
    if (p.drop) DKDV_LAUNCH(true);
    else DKDV_LAUNCH(false);
#undef DKDV_LAUNCH
}

}  // namespace attn_units
