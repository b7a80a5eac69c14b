// =====================================================================================================================
// 256 x 256 x 64 tile, 512 threads (8 waves as 2(M) x 4(N), 128 x 64 per wave), bf16 only, full tiles only.
// Operands go global -> LDS directly with global_load_lds_dwordx4 (LDS-DMA: no VGPR staging, no ds_write pass) into a
// 2-stage ring (2 x (32 KiB A + 32 KiB B) = 128 KiB, one workgroup per CU); ONE barrier per K-tile: the loads of tile
// t+1 are issued right after the barrier that publishes tile t and fly during its 64 MFMAs per wave.
// LDS-DMA writes 64 lanes x 16 B linearly, so the XOR swizzles of the two images are applied to the per-lane SOURCE
// address (and again on the fragment reads): same images / same conflict-free reads as the 128 x 128 kernel.
// =====================================================================================================================
// Shared by gemm256_kernel, gemm256p_kernel and gemm256w_kernel: the LDS images, the LDS-DMA addressing, the fragment reads and the two K-tile bodies.
#pragma once
#include "gemm_common.h"

namespace gemm_units {

__device__ __forceinline__ int off_kc2(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
__device__ __forceinline__ int off_ks2(int k, int col) { return k * 512 + ((((col >> 4) ^ ks_f(k))) << 5) + (col & 15) * 2; }

// issue the 4 LDS-DMA instructions this wave owns for one 256 x 64 operand tile.  Addressing: everything that varies per instruction
// (tile origin, K-tile, piece index, wave) is wave-uniform and lives in a scalar base; the per-lane part is ONE 32-bit byte offset per
// operand layout (two for the k-strided one) -> global_load_lds v_off, s[base] and no 64-bit per-lane pointers held across the K loop.
__device__ __forceinline__ uint32_t glds_voff_kc(int ld, int lane) {       // 8 rows x 128 B per instruction; chunk XOR (row & 7)
    return (uint32_t)(((lane >> 3) * ld + (((lane & 7) ^ ((lane >> 3) & 7)) * 8)) * 2);
}
__device__ __forceinline__ uint32_t glds_voff_ks(int ld, int lane, int kpar, int i) {   // 2 k-rows x 512 B per instruction; k = 8*wave + 2*i + (lane >> 5)
    const int klo = (2 * i + (lane >> 5)) & 3;                  // k & 3
    const int f = klo | (kpar << 2);                            // ks_f(k): (k & 3) | (((k >> 3) & 1) << 2), (k >> 3) & 1 == wave & 1
    const int slot = lane & 31;
    return (uint32_t)(((lane >> 5) * ld + ((((slot >> 1) ^ f)) << 4) + (slot & 1) * 8) * 2);
}
template <bool KSTRIDED>
__device__ __forceinline__ void glds_tile(const bf16* __restrict__ ptr, int ld, int r0, int k0, char* lds, int wave, int lane) {
    if constexpr (!KSTRIDED) {
        const uint32_t vo = glds_voff_kc(ld, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r8 = wave * 32 + i * 8;                    // 8 rows x 128 B = 1 KiB per instruction
            const char* ub = reinterpret_cast<const char*>(ptr + (int64_t)(r0 + r8) * ld + k0);
            __builtin_amdgcn_global_load_lds((glb_void_ptr)(ub + vo), (lds_void_ptr)(lds + r8 * 128), 16, 0, 0);
        }
    } else {
        const uint32_t vo0 = glds_voff_ks(ld, lane, wave & 1, 0), vo1 = glds_voff_ks(ld, lane, wave & 1, 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k2 = wave * 8 + i * 2;                     // 2 k-rows x 512 B = 1 KiB per instruction
            const char* ub = reinterpret_cast<const char*>(ptr + (int64_t)(k0 + k2) * ld + r0);
            __builtin_amdgcn_global_load_lds((glb_void_ptr)(ub + ((i & 1) ? vo1 : vo0)), (lds_void_ptr)(lds + k2 * 512), 16, 0, 0);
        }
    }
}

template <bool KSTRIDED>
__device__ __forceinline__ bf16x8 read_frag2(const char* lds, int base16, int ks, int lane) {
    if constexpr (!KSTRIDED) {
        int row = base16 + (lane & 15);
        return *reinterpret_cast<const bf16x8*>(lds + off_kc2(row, ks * 4 + (lane >> 4)));
    } else {
        int g = lane >> 4, t = lane & 15, q = t >> 2, p = t & 3;
        int k = ks * 32 + g * 8 + q;
        int col = base16 + 4 * p;
        typedef __attribute__((address_space(3))) bf16x4* lp;
        bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lp)(lds + off_ks2(k, col)));
        bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lp)(lds + off_ks2(k + 4, col)));
        bf16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        return r;
    }
}

// Transposing LDS read issued from inline asm.  Why: the compiler cannot see which LDS bytes an in-flight LDS-DMA writes, and for the
// ds_read_tr builtin (unlike plain C++ LDS loads) it protects itself with s_waitcnt vmcnt(0) before the first such read -- which waits
// for the NEXT K-tile's DMA and turns a 2-stage ring into a single-stage one.  The asm read is invisible to that logic; the price is
// that its result is not tracked either: tr_fence() below is the (only) point where the values become usable.
__device__ __forceinline__ u32x2 ds_read_tr_asm(const char* lds_ptr) {
    u32x2 r;
    const unsigned addr = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)lds_ptr;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(r) : "v"(addr) : "memory");
    return r;
}
// One k-strided fragment = two transposing reads.  The halves stay separate register pairs until tr_fence has run: nothing (not even
// a register copy that assembles the 128-bit operand) may touch them while the reads are in flight.
struct TrFrag { u32x2 lo, hi; };
__device__ __forceinline__ TrFrag read_frag2a(const char* lds, int base16, int ks, int lane) {
    int g = lane >> 4, t = lane & 15, q = t >> 2, pp = t & 3;
    int k = ks * 32 + g * 8 + q;
    int col = base16 + 4 * pp;
    TrFrag f;
    f.lo = ds_read_tr_asm(lds + off_ks2(k, col));
    f.hi = ds_read_tr_asm(lds + off_ks2(k + 4, col));
    return f;
}
__device__ __forceinline__ bf16x8 tr_assemble(const TrFrag& f) {
    const u32x4 r = {f.lo[0], f.lo[1], f.hi[0], f.hi[1]};
    return *reinterpret_cast<const bf16x8*>(&r);
}
// wait for every outstanding LDS read; the raw halves are operands so that nothing that reads them can be scheduled above the wait
template <int N>
__device__ __forceinline__ void tr_fence(TrFrag (&f)[N]) {
    static_assert(N == 4 || N == 8, "fragment groups of 4 (B) or 8 (A)");
    if constexpr (N == 4)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0].lo), "+v"(f[0].hi), "+v"(f[1].lo), "+v"(f[1].hi), "+v"(f[2].lo), "+v"(f[2].hi), "+v"(f[3].lo), "+v"(f[3].hi) :: "memory");
    else
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0].lo), "+v"(f[0].hi), "+v"(f[1].lo), "+v"(f[1].hi), "+v"(f[2].lo), "+v"(f[2].hi), "+v"(f[3].lo), "+v"(f[3].hi),
                     "+v"(f[4].lo), "+v"(f[4].hi), "+v"(f[5].lo), "+v"(f[5].hi), "+v"(f[6].lo), "+v"(f[6].hi), "+v"(f[7].lo), "+v"(f[7].hi) :: "memory");
}
// plain (compiler-tracked) fragments ride through the same wait so that they, too, are complete after it
template <int N>
__device__ __forceinline__ void plain_fence(bf16x8 (&f)[N]) {
    static_assert(N == 4 || N == 8, "fragment groups of 4 (B) or 8 (A)");
    if constexpr (N == 4) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f[0]), "+v"(f[1]), "+v"(f[2]), "+v"(f[3]), "+v"(f[4]), "+v"(f[5]), "+v"(f[6]), "+v"(f[7]) :: "memory");
}

// (Round 6, measured and removed -- profiles/r6_wgrad_kloop.txt: two re-schedules of the k-strided K-tile of the weight-gradient kernel, both bitwise equal, both SLOWER in the
//  step: progressive counted lgkmcnt waits, row tile i's MFMAs as soon as B and A[0..i] have returned, +0.17 / +0.23 ms; waves 4-7 running half a K-tile behind waves 0-3 so
//  that the read phase of one wave of a SIMD falls under the MFMA phase of the other, +0.43 / +0.48 ms.  As in round 4, the compiler's schedule stands: what holds this loop at
//  2.0 us per K-tile is not the order of reads and MFMAs inside a wave or between the two waves of a SIMD.)
// ---- one K-tile (64 deep) of the 256 x 256 tile: 64 MFMAs per wave ---------------------------------------------------------------------
// NT layout, order pinned by hand: 16 steps of 4 MFMAs (one A row-tile x 4 B column-tiles); the 8 LDS-DMA instructions of the NEXT K-tile
// (source origins a_next / b_next = first row of the tile at the K-tile's first k; nullptr = nothing to load) go one per step over the
// first 8 steps, fragment reads run two steps ahead of their use.  Measured and NOT adopted (profiles/r2e_gemm_kloop_experiments.txt):
// issuing the 8 LDS-DMA instructions 2 / 4 / 8 per step (+0.4 ... +1.3 % block time), and a rotated schedule with the workgroup barrier
// after step 12 and the next K-tile's first fragments preloaded under the last 16 MFMAs (fc1 +-0 %, qkv -5 %, 28 more registers).  The K
// loop runs at 1.55 us per K-tile = 70 % of its MFMA bound at the clock the CUs hold under this load (1.9 GHz, tools/gemm_pstamps.py).
__device__ __forceinline__ void ktile_nt_pinned(f32x4 (&acc)[8][4], const char* cur, char* nxt, const bf16* a_next, int lda,
                                                const bf16* b_next, int ldb, int wave, int lane, int wm, int wn) {
    const char* sA = cur; const char* sB = cur + 32768;
    const uint32_t vo_a = glds_voff_kc(lda, lane), vo_b = glds_voff_kc(ldb, lane);
    bf16x8 fb0[4], fb1[4], fa0[4], fa1[4];
#define G_RA(ks, ih, i) read_frag2<false>(sA, wm * 128 + ((ih) * 4 + (i)) * 16, ks, lane)
#define G_RB(ks, j) read_frag2<false>(sB, wn * 64 + (j) * 16, ks, lane)
#define G_MM4(ih, i, fb, fa) _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[(ih) * 4 + (i)][j] = mfma16(fb[j], fa[i], acc[(ih) * 4 + (i)][j]);
#define G_SB __builtin_amdgcn_sched_barrier(0);
#define G_DMA(n) { const int r8 = wave * 32 + ((n) & 3) * 8; \
                   const char* ub = reinterpret_cast<const char*>((n) < 4 ? a_next + (int64_t)r8 * lda : b_next + (int64_t)r8 * ldb); \
                   __builtin_amdgcn_global_load_lds((glb_void_ptr)(ub + ((n) < 4 ? vo_a : vo_b)), (lds_void_ptr)(nxt + ((n) < 4 ? 0 : 32768) + r8 * 128), 16, 0, 0); }
    G_SB
#pragma unroll
    for (int j = 0; j < 4; ++j) fb0[j] = G_RB(0, j);
#pragma unroll
    for (int i = 0; i < 4; ++i) fa0[i] = G_RA(0, 0, i);
    G_SB
    G_MM4(0, 0, fb0, fa0) G_DMA(0) fa1[0] = G_RA(0, 1, 0); fb1[0] = G_RB(1, 0); G_SB
    G_MM4(0, 1, fb0, fa0) G_DMA(1) fa1[1] = G_RA(0, 1, 1); fb1[1] = G_RB(1, 1); G_SB
    G_MM4(0, 2, fb0, fa0) G_DMA(2) fa1[2] = G_RA(0, 1, 2); fb1[2] = G_RB(1, 2); G_SB
    G_MM4(0, 3, fb0, fa0) G_DMA(3) fa1[3] = G_RA(0, 1, 3); fb1[3] = G_RB(1, 3); G_SB
    G_MM4(1, 0, fb0, fa1) G_DMA(4) fa0[0] = G_RA(1, 0, 0); G_SB
    G_MM4(1, 1, fb0, fa1) G_DMA(5) fa0[1] = G_RA(1, 0, 1); G_SB
    G_MM4(1, 2, fb0, fa1) G_DMA(6) fa0[2] = G_RA(1, 0, 2); G_SB
    G_MM4(1, 3, fb0, fa1) G_DMA(7) fa0[3] = G_RA(1, 0, 3); G_SB
    G_MM4(0, 0, fb1, fa0) fa1[0] = G_RA(1, 1, 0); G_SB
    G_MM4(0, 1, fb1, fa0) fa1[1] = G_RA(1, 1, 1); G_SB
    G_MM4(0, 2, fb1, fa0) fa1[2] = G_RA(1, 1, 2); G_SB
    G_MM4(0, 3, fb1, fa0) fa1[3] = G_RA(1, 1, 3); G_SB
    G_MM4(1, 0, fb1, fa1) G_SB
    G_MM4(1, 1, fb1, fa1) G_SB
    G_MM4(1, 2, fb1, fa1) G_SB
    G_MM4(1, 3, fb1, fa1) G_SB
#undef G_RA
#undef G_RB
#undef G_MM4
#undef G_SB
#undef G_DMA
}

// any layout, compiler-scheduled: fragments of one 32-deep k-step, then its 32 MFMAs; k-strided operands use the asm transposing reads
template <bool TA, bool TB>
__device__ __forceinline__ void ktile_generic(f32x4 (&acc)[8][4], const char* cur, int lane, int wm, int wn) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 fa[8], fb[4];
        if constexpr (TA || TB) {
            // plain (compiler-tracked) reads first, the asm transposing reads after them, then the waits; fragments are assembled
            // only after their wait
            TrFrag ta[TA ? 8 : 1], tb[TB ? 4 : 1];
            if constexpr (!TB) { _Pragma("unroll") for (int j = 0; j < 4; ++j) fb[j] = read_frag2<false>(cur + 32768, wn * 64 + j * 16, ks, lane); }
            if constexpr (!TA) { _Pragma("unroll") for (int i = 0; i < 8; ++i) fa[i] = read_frag2<false>(cur, wm * 128 + i * 16, ks, lane); }
            if constexpr (TB) { _Pragma("unroll") for (int j = 0; j < 4; ++j) tb[j] = read_frag2a(cur + 32768, wn * 64 + j * 16, ks, lane); }
            if constexpr (TA) { _Pragma("unroll") for (int i = 0; i < 8; ++i) ta[i] = read_frag2a(cur, wm * 128 + i * 16, ks, lane); }
            if constexpr (TB) { tr_fence(tb); _Pragma("unroll") for (int j = 0; j < 4; ++j) fb[j] = tr_assemble(tb[j]); } else plain_fence(fb);
            if constexpr (TA) { tr_fence(ta); _Pragma("unroll") for (int i = 0; i < 8; ++i) fa[i] = tr_assemble(ta[i]); } else plain_fence(fa);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) fb[j] = read_frag2<TB>(cur + 32768, wn * 64 + j * 16, ks, lane);
#pragma unroll
            for (int i = 0; i < 8; ++i) fa[i] = read_frag2<TA>(cur, wm * 128 + i * 16, ks, lane);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(fb[j], fa[i], acc[i][j]);
    }
}

}  // namespace gemm_units
