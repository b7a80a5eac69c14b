// gemm256_kernel: the 256 x 256 two-stage LDS-DMA kernel (gemm_tile256.h), one tile per workgroup; all four operand layouts, split-K.
// The unit also holds the dynamic-queue instantiations of the persistent kernel (gemm256p.h; the static-list ones: gemm256p.hip).  Not for tidiness: compiled
// in a unit without any gemm256p_kernel, gemm256_kernel comes out different (address arithmetic of the prologue, and through register numbering the K loop and the
// epilogue: the optimizer then knows more about the arguments of the helpers both kernels call) -- tools/kernel_isa_diff.py; with either half of the persistent
// kernel's instantiations beside it, it is the code it always was.
#include "gemm256p.h"

namespace {

template <bool TA, bool TB, int PIN = 0>
__global__ __launch_bounds__(NT2) void gemm256_kernel(GemmP p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int ntiles = p.tiles_m * p.tiles_n;
    int t, z;
    if (gridDim.y == 1 && p.split_k > 1) {
        // Split-K launched as ONE list of (slab z, tile) pairs in XCD-major order: XCD x (block ids congruent to x mod 8) takes the x-th eighth of the list, i.e. ~32
        // consecutive tiles of ONE slab.  Workgroups of a slab read the same K range (rows of both operands, for the weight gradient) and differ only in the column blocks:
        // 32 tiles of one slab are ~11 x 3 column blocks, 14 operand blocks for 32 workgroups, held by the XCD's L2 while the workgroups stream through K together.
        // The (tile, slab) grid put ~4.5 tiles of EVERY slab on each XCD: seven K ranges per L2, 2.7 x the operand bytes from the fabric (profiles/r4_wgrad_xcd.txt).
        const int total = ntiles * p.split_k, per = (total + 7) >> 3;
        const int j = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
        if (j >= total || (int)(blockIdx.x >> 3) >= per) return;
        z = j / ntiles; t = j - z * ntiles;
    } else {
        t = xcd_remap(blockIdx.x, ntiles);
        z = blockIdx.y;
    }
    int tm, tn;
    tile_coords(t, p.tiles_m, p.tiles_n, p.group_m, tm, tn);
    const int m0 = tm * T2, n0 = tn * T2;
    const int kbeg = z * p.k_per_split;
    const int kend = min(p.K, kbeg + p.k_per_split);
    int nk = (kend - kbeg) / 64;
    if (GDBG(1)) nk = min(nk, 1);
    const bf16* A = reinterpret_cast<const bf16*>(p.A);
    const bf16* B = reinterpret_cast<const bf16*>(p.B);

#ifdef DEVIAS_GEMM_DEBUG
    unsigned long long st0 = 0, st1 = 0, st2 = 0, st3 = 0;
    if (GDBG(8)) st0 = __builtin_amdgcn_s_memrealtime();
#endif
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nk > 0) {
        glds_tile<TA>(A, p.lda, m0, kbeg, smem, wave, lane);
        glds_tile<TB>(B, p.ldb, n0, kbeg, smem + 32768, wave, lane);
    }
    for (int kt = 0; kt < nk; ++kt) {
#ifdef DEVIAS_GEMM_DEBUG
        if (GDBG(8) && kt == 0) st1 = __builtin_amdgcn_s_memrealtime();
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's LDS-DMA for tile kt has landed
        __syncthreads();
#ifdef DEVIAS_GEMM_DEBUG
        if (GDBG(8) && kt == 0) st2 = __builtin_amdgcn_s_memrealtime();
#endif
        char* cur = smem + (kt & 1) * STAGE2;
        char* nxt = smem + ((kt + 1) & 1) * STAGE2;
        if constexpr (!TA && !TB && PIN != 0) {
            const int kn = kbeg + (kt + 1 < nk ? kt + 1 : kt) * 64;       // last tile: harmless re-read into the free stage
            ktile_nt_pinned(acc, cur, nxt, A + (int64_t)m0 * p.lda + kn, p.lda, B + (int64_t)n0 * p.ldb + kn, p.ldb, wave, lane, wm, wn);
        } else {
            if (kt + 1 < nk && !GDBG(4)) {
                glds_tile<TA>(A, p.lda, m0, kbeg + (kt + 1) * 64, nxt, wave, lane);
                glds_tile<TB>(B, p.ldb, n0, kbeg + (kt + 1) * 64, nxt + 32768, wave, lane);
            }
            ktile_generic<TA, TB>(acc, cur, lane, wm, wn);
        }
    }

    // ---- epilogue ------------------------------------------------------------------------------------------------
    // The MFMA layout gives each lane 4 columns of 16 different rows: stored directly that is 16 partial 128-B lines per
    // wave-instruction and the store path, not HBM, bounds the kernel (measured: 105 of 260 us on the QKV shape).  Default: the
    // register-transposed epilogue (epilogue_swap); option gemm_epi = 0: through LDS (the operand ring is dead by now: one 16 KiB
    // fp32 region per wave, two passes of 64 rows), every global access row-contiguous, 16 bytes per lane.
#ifdef DEVIAS_GEMM_DEBUG
    if (GDBG(8)) {
        st3 = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            unsigned long long* d = reinterpret_cast<unsigned long long*>(p.ws) + (size_t)blockIdx.x * 6;
            d[0] = st0; d[1] = st1; d[2] = st2; d[3] = st3;
            d[4] = __builtin_amdgcn_s_getreg(0x1800 | 20) /* HW_REG_XCC_ID */; d[5] = t;
        }
    }
    if (GDBG(2) && acc[0][0][0] != 12345.678f) return;
#endif
    if constexpr (PIN == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the trailing re-read must land before the LDS is released
    if (p.epi_swap) { epilogue_swap<8>(p, acc, m0 + wm * 128, n0 + wn * 64, z, lane); return; }
    __syncthreads();                                   // every wave is done reading the operand stages
    epilogue_staged<8, 4>(p, acc, smem + wave * 16384, m0 + wm * 128, n0 + wn * 64, z, lane);
}

}  // namespace

void gemm_units::launch_gemm256(const GemmP& p, int ta, int tb, bool splitk_xcd_list, hipStream_t st) {
    const int nt = p.tiles_m * p.tiles_n;
    dim3 grid(nt, p.split_k), block(NT2);
    if (p.split_k > 1 && splitk_xcd_list) grid = dim3(8 * ((nt * p.split_k + 7) / 8));      // (slab, tile) pairs in XCD-major order (gemm256_kernel)
    if (!ta && !tb) hipLaunchKernelGGL((gemm256_kernel<false, false, 1>), grid, block, 0, st, p);
    else if (!ta && tb) hipLaunchKernelGGL((gemm256_kernel<false, true>), grid, block, 0, st, p);
    else if (ta && tb) hipLaunchKernelGGL((gemm256_kernel<true, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((gemm256_kernel<true, false>), grid, block, 0, st, p);
}

void gemm_units::launch_gemm256p_dyn(const GemmP& p, bool tb, int side, int epi, int cus, hipStream_t st) { pers_launch<true>(tb, side, epi, dim3(cus), st, p); }
