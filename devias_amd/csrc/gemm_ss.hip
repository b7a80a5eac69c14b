// =====================================================================================================================
// 256 x 128 x 64 tile, 256 threads (4 waves as 2(M) x 2(N), 128 x 64 per wave), ONE 48 KiB LDS stage filled by LDS-DMA,
// three workgroups per CU: load/compute overlap and -- the point -- epilogue/compute overlap come from the co-resident
// workgroups (independent waves, independent vmcnt), not from an in-kernel software pipeline.
// =====================================================================================================================
#include "gemm_tile256.h"      // (off_kc2: the k-contiguous image is the 256 x 256 kernels')

using namespace gemm_units;

namespace {

enum { SS_NT = 256, SS_ABYTES = 32768, SS_BBYTES = 16384 };

template <bool KSTRIDED, int ROWS>      // ROWS = extent of the non-K dim of the tile (256 for A, 128 for B)
__device__ __forceinline__ void glds_tile_ss(const bf16* __restrict__ ptr, int ld, int r0, int k0, char* lds, int wave, int lane) {
    constexpr int NI = ROWS * 128 / 1024 / 4;          // 1-KiB instructions per wave (4 waves)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if constexpr (!KSTRIDED) {
            const int r8 = (wave * NI + i) * 8;
            const int row = r8 + (lane >> 3);
            const int chunk = (lane & 7) ^ (row & 7);
            const bf16* src = ptr + (int64_t)(r0 + row) * ld + k0 + chunk * 8;
            __builtin_amdgcn_global_load_lds((glb_void_ptr)src, (lds_void_ptr)(lds + r8 * 128), 16, 0, 0);
        } else {
            constexpr int RB = ROWS * 2;                 // bytes per k-row
            constexpr int KPI = 1024 / RB;               // k-rows per instruction (2 for 256 cols, 4 for 128 cols)
            const int kb = (wave * NI + i) * KPI;
            const int k = kb + lane / (64 / KPI);
            const int slot = lane % (64 / KPI);          // 16-byte slot inside the row
            const int col = (((slot >> 1) ^ ks_f(k)) << 4) + (slot & 1) * 8;
            const bf16* src = ptr + (int64_t)(k0 + k) * ld + r0 + col;
            __builtin_amdgcn_global_load_lds((glb_void_ptr)src, (lds_void_ptr)(lds + kb * RB), 16, 0, 0);
        }
    }
}

template <bool KSTRIDED, int ROWS>
__device__ __forceinline__ bf16x8 read_frag_ss(const char* lds, int base16, int ks, int lane) {
    if constexpr (!KSTRIDED) {
        int row = base16 + (lane & 15);
        return *reinterpret_cast<const bf16x8*>(lds + off_kc2(row, ks * 4 + (lane >> 4)));
    } else {
        int g = lane >> 4, t = lane & 15, q = t >> 2, p = t & 3;
        int k = ks * 32 + g * 8 + q;
        int col = base16 + 4 * p;
        typedef __attribute__((address_space(3))) bf16x4* lp;
        constexpr int RB = ROWS * 2;
        bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lp)(lds + k * RB + ((((col >> 4) ^ ks_f(k))) << 5) + (col & 15) * 2));
        bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lp)(lds + (k + 4) * RB + ((((col >> 4) ^ ks_f(k + 4))) << 5) + (col & 15) * 2));
        bf16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return r;
    }
}

template <bool TA, bool TB, int OCC>
__global__ __launch_bounds__(SS_NT, OCC) void gemm_ss_kernel(GemmP p) {
    __shared__ __attribute__((aligned(16))) char smem[SS_ABYTES + SS_BBYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int ntiles = p.tiles_m * p.tiles_n;
    const int t = xcd_remap(blockIdx.x, ntiles);
    int tm, tn;
    tile_coords(t, p.tiles_m, p.tiles_n, p.group_m, tm, tn);
    const int m0 = tm * SS_BM, n0 = tn * SS_BN;
    const int z = blockIdx.y;
    const int kbeg = z * p.k_per_split;
    const int kend = min(p.K, kbeg + p.k_per_split);
    const int nk = (kend - kbeg) / 64;
    const bf16* A = reinterpret_cast<const bf16*>(p.A);
    const bf16* B = reinterpret_cast<const bf16*>(p.B);
    char* ldsA = smem;
    char* ldsB = smem + SS_ABYTES;

    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kt = 0; kt < nk; ++kt) {
        if (kt > 0) __syncthreads();                         // every wave is done reading the previous K-tile
        glds_tile_ss<TA, SS_BM>(A, p.lda, m0, kbeg + kt * 64, ldsA, wave, lane);
        glds_tile_ss<TB, SS_BN>(B, p.ldb, n0, kbeg + kt * 64, ldsB, wave, lane);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = read_frag_ss<TB, SS_BN>(ldsB, wn * 64 + j * 16, ks, lane);
#pragma unroll
            for (int ih = 0; ih < 2; ++ih) {
                bf16x8 fa[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) fa[i] = read_frag_ss<TA, SS_BM>(ldsA, wm * 128 + (ih * 4 + i) * 16, ks, lane);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[ih * 4 + i][j] = mfma16(fb[j], fa[i], acc[ih * 4 + i][j]);
            }
        }
    }
    if (p.epi_swap) { epilogue_swap<8>(p, acc, m0 + wm * 128, n0 + wn * 64, z, lane); return; }
    __syncthreads();
    epilogue_staged<8, 2>(p, acc, smem + wave * 12288, m0 + wm * 128, n0 + wn * 64, z, lane);
}

}  // namespace

void gemm_units::launch_gemm_ss(const GemmP& p, int ta, int tb, hipStream_t st) {
    dim3 grid(p.tiles_m * p.tiles_n, p.split_k), block(SS_NT);
    if (!ta && !tb) hipLaunchKernelGGL((gemm_ss_kernel<false, false, 2>), grid, block, 0, st, p);
    else if (!ta && tb) hipLaunchKernelGGL((gemm_ss_kernel<false, true, 2>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((gemm_ss_kernel<true, true, 2>), grid, block, 0, st, p);
}
