// =====================================================================================================================
// Small-M GEMM (M <= 128 rows: the B*S slot rows of the aggregation block and the head), bf16, B in nn.Linear layout [N, K]:
// C[M, N] = epilogue(A[M, K] W^T).  These products stream a weight matrix of a few MB once and do almost no arithmetic; through the 128 x 128
// kernel they needed split-K to reach more than a handful of CUs, i.e. two launches (product + reduce, ~8 + 6.5 us in the step) for ~1 us of
// memory traffic.  Here: one workgroup per 16 output columns (N / 16 workgroups: 48 ... 256), its four waves split K four ways, every operand
// fragment is ONE 16-byte global load per lane straight into the MFMA operand registers (A rows and W rows are both k-contiguous: no LDS
// staging), PD k-steps of loads in flight per wave; the waves' partial tiles meet in LDS in a fixed order (deterministic) and wave 0 applies
// the epilogue of splitk_reduce_kernel (same arithmetic, same order).
// =====================================================================================================================
// TB: W is stored [K, N] (the dgrad twins of the same layers: dX = dY W with W in nn.Linear layout [out, in] = [K, N]).  A lane then cannot load its fragment -- eight
// consecutive k of ONE column -- directly; the wave loads the [32 k][16 columns] block by rows (16 bytes per lane), drops it into a 1 KiB LDS block of its own and
// reads it back with the transposing ds_read_b64_tr_b16 (LDS executes a wave's instructions in order: no barrier).  These products used to take the 128 x 128 kernel
// plus a split-K reduce (two launches, 12-15 us in the step).
#include "gemm_common.h"

using namespace gemm_units;

namespace {

template <int MT, int SM_PD = 4, bool TB = false>      // MT = 16-row tiles of the output per workgroup; SM_PD = k-steps of loads in flight per wave (a launch of these is a latency chain: K / (4 * 32 * SM_PD) round trips to memory)
__global__ __launch_bounds__(256) void gemm_smallm_kernel(GemmP p) {
    __shared__ __attribute__((aligned(16))) f32x4 red[3][MT][64];
    __shared__ __attribute__((aligned(16))) char wstage[TB ? 4 : 1][TB ? 1024 : 16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lm = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int mbase = blockIdx.y * (16 * MT);                // (grid.y > 1: every MT row tiles their own workgroup -- the launch policy for few column groups)
    const int kw = p.K / 4;                                  // this wave's share of K (a multiple of 32: host)
    const int k0 = wave * kw;
    const bf16* A = reinterpret_cast<const bf16*>(p.A);
    const bf16* W = reinterpret_cast<const bf16*>(p.B);
    const bf16* wrow = TB ? W + (int64_t)(k0 + (lane >> 1)) * p.ldb + n0 + 8 * (lane & 1)      // row k0 + lane / 2 of the block, its left or right eight columns
                          : W + (int64_t)(n0 + lm) * p.ldb + k0 + 8 * g;
    const bf16* arow[MT];
    bool aok[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = mbase + t * 16 + lm;
        aok[t] = m < p.M;
        arow[t] = A + (int64_t)(aok[t] ? m : 0) * p.lda + k0 + 8 * g;
    }
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // what the epilogue reads is requested before the K loop (wave 0): these launches are latency chains, not bandwidth
    const bf16* res = reinterpret_cast<const bf16*>(p.res);
    const bf16* aux_in = reinterpret_cast<const bf16*>(p.aux_in);
    const int n = n0 + 4 * g;                               // this lane's four output columns
    f32x4 bias = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x4 resv[MT], auxv[MT];
    const bool dact = p.act == DEVIAS_ACT_DGELU || p.act == DEVIAS_ACT_DRELU;
    if (wave == 0) {
        if (p.bias) bias = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = mbase + t * 16 + lm;
            if (res && m < p.M) resv[t] = *reinterpret_cast<const bf16x4*>(res + (int64_t)(p.res_mod > 0 ? m % p.res_mod : m) * p.ldr + n);
            if (dact && m < p.M) auxv[t] = *reinterpret_cast<const bf16x4*>(aux_in + (int64_t)m * p.ld_aux + n);
        }
    }
    const int nks = kw / 32;
    bf16x8 fb[SM_PD], fa[SM_PD][MT];
    auto issue = [&](int slot, int ks) {
        fb[slot] = *reinterpret_cast<const bf16x8*>(wrow + (TB ? (int64_t)ks * 32 * p.ldb : (int64_t)ks * 32));
#pragma unroll
        for (int t = 0; t < MT; ++t) fa[slot][t] = *reinterpret_cast<const bf16x8*>(arow[t] + ks * 32);
    };
#pragma unroll
    for (int d = 0; d < SM_PD; ++d) if (d < nks) issue(d, d);
    for (int ks0 = 0; ks0 < nks; ks0 += SM_PD) {
#pragma unroll
        for (int d = 0; d < SM_PD; ++d) {
            const int ks = ks0 + d;
            if (ks < nks) {
                bf16x8 wf = fb[d];
                if constexpr (TB) {          // rows -> this lane's column: through the wave's LDS block
                    char* blk = wstage[wave];
                    *reinterpret_cast<bf16x8*>(blk + lane * 16) = fb[d];
                    typedef __attribute__((address_space(3))) bf16x4* lp;
                    const int q = lm >> 2, pp = lm & 3;
                    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lp)(blk + (8 * g + q) * 32 + 8 * pp));
                    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lp)(blk + (8 * g + q + 4) * 32 + 8 * pp));
                    wf = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[t] = mfma16(wf, fa[d][t], acc[t]);
                if (ks + SM_PD < nks) issue(d, ks + SM_PD);
            }
        }
    }
    // rows beyond M were computed from row 0's data: they are never stored.  Partial tiles of waves 1..3 -> LDS; wave 0 adds them in that order
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < MT; ++t) red[wave - 1][t][lane] = acc[t];
    }
    __syncthreads();
    if (wave != 0) return;
    bf16* aux_out = reinterpret_cast<bf16*>(p.aux_out);
    bf16* C = reinterpret_cast<bf16*>(p.C);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = mbase + t * 16 + lm;
        f32x4 v = acc[t];
#pragma unroll
        for (int w = 0; w < 3; ++w) v += red[w][t][lane];
        if (m >= p.M) continue;
        if (p.bias) v += bias;
        if (p.act == DEVIAS_ACT_GELU) {
            if (aux_out) store4(aux_out + (int64_t)m * p.ld_aux + n, v);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = gelu_t<bf16>(v[e]);
        } else if (p.act == DEVIAS_ACT_RELU) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        } else if (p.act == DEVIAS_ACT_SIGMOID) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = 1.0f / (1.0f + expf(-v[e]));
        } else if (dact) {
            const f32x4 a4 = {(float)auxv[t][0], (float)auxv[t][1], (float)auxv[t][2], (float)auxv[t][3]};
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = p.act == DEVIAS_ACT_DGELU ? v[e] * dgelu_t<bf16>(a4[e]) : (a4[e] > 0.f ? v[e] : 0.f);
        }
        if (p.row_scale) v *= p.row_scale[m / p.rows_per_scale];
        if (res) v += f32x4{(float)resv[t][0], (float)resv[t][1], (float)resv[t][2], (float)resv[t][3]};
        store4(C + (int64_t)m * p.ldc + n, v);
    }
}

}  // namespace

// row_tile_grid: one workgroup per 16-row tile as well as per 16 columns (the host's policy for few column groups); W stored [K, N] (tb) always runs that way
void gemm_units::launch_gemm_smallm(const GemmP& p, bool tb, bool row_tile_grid, hipStream_t st) {
    const int mt = cdiv(p.M, 16);
    dim3 grid(p.N / 16), block(256);
    if (tb) { grid = dim3(p.N / 16, mt); hipLaunchKernelGGL((gemm_smallm_kernel<1, 12, true>), grid, block, 0, st, p); }
    else if (row_tile_grid) { grid = dim3(p.N / 16, mt); hipLaunchKernelGGL((gemm_smallm_kernel<1, 12>), grid, block, 0, st, p); }
    else if (mt <= 1) hipLaunchKernelGGL((gemm_smallm_kernel<1, 12>), grid, block, 0, st, p);
    else if (mt <= 2) hipLaunchKernelGGL((gemm_smallm_kernel<2>), grid, block, 0, st, p);
    else if (mt <= 4) hipLaunchKernelGGL((gemm_smallm_kernel<4>), grid, block, 0, st, p);      // (all six k-steps of a K = 768 wave in flight, <4, 6>: no gain in the step)
    else if (mt <= 6) hipLaunchKernelGGL((gemm_smallm_kernel<6>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((gemm_smallm_kernel<8>), grid, block, 0, st, p);
}
