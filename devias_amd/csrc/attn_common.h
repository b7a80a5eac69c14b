// What more than one attention unit needs (encoder multi-head self-attention core for gfx950: head dim 64, non-causal, arbitrary sequence length N;
// reference semantics softmax((q * dh^-0.5) k^T) v, model/modeling_slot.py:102-112).  The N x N matrix is never materialised: online softmax forward,
// recompute-from-logsumexp backward.  qkv layout is [B, N, 3, H, 64] exactly as produced by the fused QKV GEMM; o / d_o are [B, N, H*64].
//
// The kernels live in four units, each with its kernels, the helpers only they use and their host launchers:
//   attn_fwd.hip     forward, bf16: the 32x32x16 kernel (default), and the forward's launcher
//   attn_mfma16.hip  the bf16 kernels on 16x16x32 MFMAs: forward (option attn_cfg = 6), backward dQ (also produces delta = rowsum(dO * O) and the row statistics of the
//                    one-wave dK / dV kernel), backward dK / dV with two waves per SIMD (option attn_dkdv = 0, attention dropout, fused v_bias partials)
//   attn_bwd1w.hip   backward dK / dV, bf16, one wave per SIMD (default; its own shared pieces in attn1w.h)
//   attn_f32.hip     the three fp32 parity kernels
// attention.hip holds the host side: the entry points, validation, the choice of kernel form, counters and workspace arithmetic.
//
// The bf16 16x16x32 kernels compute "key-major" score tiles.  The score tile is computed TRANSPOSED, S^T = K Q^T, so that after the MFMA each lane owns ONE
// query column (lane & 15) and 4 keys per 16-key tile (rows 4*(lane>>4)+r): the online-softmax row statistics are lane-local plus two cross-lane shuffles,
// and the probability tile is directly the B operand of the next MFMA (O^T = V^T P^T) with a fixed k-permutation
// (element j of lane-group g <-> key 16*(2s + (j>>2)) + 4g + (j&3)), matched on the A side by reading V^T with the transposing LDS read
// ds_read_b64_tr_b16.  No probability tile ever goes through LDS.  K / V (forward, dQ) resp. Q / dO (dK / dV) tiles of 64 rows arrive by LDS-DMA through a
// buffer descriptor (TileDma) into a two-stage ring, one barrier per tile.
#pragma once
#include "common.h"

// the one-wave-per-SIMD dK / dV kernel's launcher (attn_bwd1w.hip): the whole 256-key blocks of every head, then the ragged rest; it bumps its own counters and
// checks its own launches (DEVIAS_OK or the error)
int devias_attn_dkdv1w_launch(const void* qkv, const void* d_o, const float* stat, void* dqkv, int B, int N, int Npad, int H, float scale, int xcd_flag,
                              int persistent, hipStream_t st);

namespace attn_units {    // named, not anonymous: the launchers below have external linkage and take an AttnP.  The kernels stay in each unit's anonymous namespace.

constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
// bit 1 of the kernels' `xcd` argument (bit 0: XCD-aware linear grid, bits 16..: B): the q third of qkv already holds q * scale * log2 e, rounded ONCE by its producer
// (DEVIAS_ATTN_Q_PRESCALED, ABI 167).  Forward, dQ and dK / dV kernels then multiply the SAME bf16 operands -- the backward's scores are the forward's, the saved lse fits
// them exactly -- where otherwise forward / dQ round q * c and the one-wave dK / dV kernel rounds k * c (~2x the dK / dV error at peaked logits)
enum { ATTN_QPRE = 2 };

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((address_space(3))) bf16x4* lds_bf16x4_ptr;
typedef __attribute__((address_space(3))) void* lds_void_ptr;

// ---- attention dropout (Attention.attn_drop, model/modeling_slot.py:90,110: nn.Dropout on the softmax matrix) ---------------------------------
// The N x N matrix never exists, so neither does its mask: element (b, h, query i, key j) is kept when a 32-bit hash of (seed, b * H + h, i, j) is below
// keep * 2^32, and kept elements are scaled by 1 / keep.  The same function is evaluated by the forward and by both backward kernels (and restated in
// numpy by the oracle: oracle/ref_cpu.py attn_drop_mask).  Row sums (the softmax normaliser, logsumexp) are over the UN-dropped probabilities;
// delta = rowsum(dO * O) with the dropped-out O is still sum_j P_ij dP_ij, so the recompute-from-logsumexp backward carries over with
// dP_ij = mask_ij (dO_i . V_j) and dV = (P * mask)^T dO.
struct DropP { uint32_t thresh, s0, s1; float inv_keep; };
__device__ __forceinline__ uint32_t drop_mix(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
__device__ __forceinline__ uint32_t drop_rowkey(const DropP& d, uint32_t bh, uint32_t i) { return drop_mix(drop_mix(d.s0 ^ (bh * 0x9E3779B1u)) + d.s1 + i * 0x85EBCA6Bu); }
// 0 or 1 / keep
__device__ __forceinline__ float drop_scale(const DropP& d, uint32_t rowkey, uint32_t j) { return drop_mix(rowkey + j * 0xC2B2AE35u) < d.thresh ? d.inv_keep : 0.f; }

// ---- one attention call, as the entry points fill it (attention.hip: validate, choose, launch) and the launchers read it --------------------------------------
struct AttnP {
    const void* qkv; void* o; const void* d_o; float* lse; float* delta; void* dqkv;      // T = dtype; o and lse are written by the forward and read by the backward, which also has d_o, delta, dqkv
    int B, N, H; float scale; int dtype;
    float keep; uint64_t seed;      // attention dropout (keep >= 1: none)
    int flags;                      // DEVIAS_ATTN_Q_PRESCALED
    float* part_q; float* part_v;   // backward, optional: q_bias / v_bias gradient partials from the kernels' accumulators
    float* stat;                    // backward, optional: the row statistics the dQ kernel leaves for the one-wave-per-SIMD dK / dV kernel, [B, H, npad / 32, 2, 32]
    hipStream_t st;
    // derived by the host side before it launches
    int xcd;                        // the bf16 kernels' packed argument: bit 0 XCD-aware linear grid, ATTN_QPRE, bits 16.. B
    bool drop; DropP dp;            // keep < 1, and its mask: a run-time fact for a launcher, a template flag of the kernels
    int npad;                       // N rounded up to a 32-query slice
};
// ---- the host launchers: the unit of a kernel owns its template ladder, grid and block size; each enqueues one kernel on p.st, the caller checks the launch ----
// which forward kernel: the 32x32x16 kernel on four waves (128 queries per workgroup; the only form with dropout: p.drop overrides the others), on two (64), the 16x16x32 kernel
enum AttnFwdForm { ATTN_FWD32_4W, ATTN_FWD32_2W, ATTN_FWD16 };
// which dQ shape <16-query tiles per wave, waves>: <2, 4> serves dropout and the q_bias partials (p.drop overrides the others; the caller asks for part_q only with it)
enum AttnDqForm { ATTN_DQ_2x4, ATTN_DQ_4x2, ATTN_DQ_4x4, ATTN_DQ_2x2 };
void launch_attn_fwd_bf16(AttnFwdForm form, const AttnP& p);      // attn_fwd.hip ...
void launch_attn_fwd16_bf16(const AttnP& p);                      // ... which hands ATTN_FWD16 to attn_mfma16.hip
void launch_attn_bwd_dq_bf16(AttnDqForm form, const AttnP& p);
void launch_attn_bwd_dkdv2w_bf16(const AttnP& p);
void launch_attn_fwd_f32(const AttnP& p);
void launch_attn_bwd_dq_f32(const AttnP& p);
void launch_attn_bwd_dkdv_f32(const AttnP& p);
// grid of the bf16 kernels: `per` rows of one (batch, head) per workgroup; linear under the XCD-aware order (head_map below)
static inline dim3 attn_grid(const AttnP& p, int per) { return (p.xcd & 1) ? dim3(cdiv(p.N, per) * p.H * p.B) : dim3(cdiv(p.N, per), p.H, p.B); }

// ---- LDS images of a [64 rows][64 cols] bf16 tile (8 KiB each) ------------------------------------------
// row image: 128-byte rows, 16-byte chunk index XOR (row & 7)  -> conflict-free ds_read_b128 of [row][8 cols]
__device__ __forceinline__ int img_row_off(int row, int chunk) { return row * 128 + ((chunk ^ (row & 7)) << 4); }
// transposed-read image: 128-byte rows, 32-byte window XOR ((row >> 1) & 3) -> conflict-free ds_read_b64_tr_b16
__device__ __forceinline__ int img_tr_off(int row, int col) {
    return row * 128 + ((((col >> 4) ^ ((row >> 1) & 3))) << 5) + (col & 15) * 2;
}

// The 32x32x16 forward kernel reads V^T with 32 lanes on rows 4 hi .. + 4 of TWO adjacent windows (16 lanes each) per ds_read_b64_tr_b16 where the 16x16x32
// kernels read rows 0..7 of ONE window: under img_tr_off's swizzle rows r and r + 2 then meet in the same banks (window w of row r + 2 sits where window
// w ^ 1 of row r does) -- SQ_LDS_BANK_CONFLICT = half of the kernel's LDS cycles (profiles/r4_lds_conflicts.txt).  This swizzle moves rows r, r + 2 two
// windows apart and r, r + 4 one: the eight (row, window) pairs of a 32-lane group cover all 64 banks.
// ... and its K row image: a ds_read_b128 serves lanes i and i + 16 in the same cycle (the 16x16x32 kernels' fragments put the SAME row's next chunk there;
// here lane i + 16 holds row i + 16 with the same chunk, i.e. the same banks under `chunk ^ (row & 7)`): rows 16..31 of a 32-key block take the odd
// permutation.  Measured per launch at B = 32, N = 1568, H = 12: SQ_LDS_BANK_CONFLICT 3.01e7 -> 1.51e7 (V image) -> 0 (K image), SQ_LDS_IDX_ACTIVE 6.2e7 -> 3.2e7.
// (Here, not in attn_fwd.hip, because TileDma applies both swizzles on the source address.)
__device__ __forceinline__ int row_swz2(int row) { return (row & 7) ^ ((row >> 4) & 1); }
__device__ __forceinline__ int img_row_off2(int row, int chunk) { return row * 128 + ((chunk ^ row_swz2(row)) << 4); }
__device__ __forceinline__ int tr_swz2(int row) { return (((row >> 1) & 1) << 1) | ((row >> 2) & 1); }
__device__ __forceinline__ int img_tr_off2(int row, int col) {
    return row * 128 + ((((col >> 4) ^ tr_swz2(row))) << 5) + (col & 15) * 2;
}

// fragment of the row image: lane holds tile[row = base + (lane&15)][32*ks + 8*(lane>>4) .. +8]
__device__ __forceinline__ bf16x8 frag_rows(const char* img, int base, int ks, int lane) {
    int row = base + (lane & 15);
    return *reinterpret_cast<const bf16x8*>(img + img_row_off(row, ks * 4 + (lane >> 4)));
}
// the SAME fragment as frag_rows, read from the transposed-read image: its 32-byte-window swizzle also keeps ds_read_b128 conflict free
// (a 16-lane group of that instruction covers 16 rows x one window: 8 rows take its low half, 8 its high half, and (row & 1, (row >> 1) & 3)
// is distinct within each eight) -- so a tile that is consumed both row-wise and transposed needs ONE image, one pass of LDS writes
__device__ __forceinline__ bf16x8 frag_rows_tr(const char* img, int base, int ks, int lane) {
    int row = base + (lane & 15);
    return *reinterpret_cast<const bf16x8*>(img + img_tr_off(row, 32 * ks + 8 * (lane >> 4)));
}
// fragment of the transposed image for the product over ROWS of the tile (k = tile row, permuted as in the header):
// lane holds tile[row = 16*(2s + (j>>2)) + 4g + (j&3)][col = cbase + (lane&15)], j = 0..7
__device__ __forceinline__ bf16x8 frag_tr(const char* img, int cbase, int s, int lane) {
    int g = lane >> 4, c = lane & 15;
    int r0 = 32 * s + 4 * g + (c >> 2);
    int col = cbase + 4 * (c & 3);
    bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(img + img_tr_off(r0, col)));
    bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(img + img_tr_off(r0 + 16, col)));
    bf16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return r;
}
__device__ __forceinline__ bf16x8 pack8(f32x4 a, f32x4 b) {
    bf16x8 r = {(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
    return r;
}
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {
    const bf16x2 t = {(bf16)a, (bf16)b};
    return *reinterpret_cast<const unsigned*>(&t);
}
// raw v_exp_f32: arguments here are <= 0 (or -inf), results below the normal range may flush to 0 -- harmless for softmax
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ f32x4 mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// Block -> (block-in-head, head, batch).  Every block of one (batch, head) streams the same K/V (forward, dQ) or Q/dO (dK/dV) rows.  Workgroups go
// to the 8 XCDs round-robin by linear id, and each XCD has a private L2: with the plain (x = block-in-head, y = head, z = batch) order the ~13
// blocks of a head land on 8 different L2s and each fetches the head's rows from the Infinity Cache again.  With `xcd` the grid is linear
// and all blocks of a head get ids congruent mod 8: one XCD, one fetch.  (Speed only; any mapping is correct.)
struct HeadMap { int blk, h, b; };
__device__ __forceinline__ HeadMap head_map(int nblk, int H, int B, bool xcd) {
    HeadMap m;
    if (!xcd) { m.blk = blockIdx.x; m.h = blockIdx.y; m.b = blockIdx.z; return m; }
    const int bid = blockIdx.x, x = bid & 7, slot = bid >> 3;
    const int hidx = (slot / nblk) * 8 + x;
    m.blk = slot - (slot / nblk) * nblk;
    m.h = hidx % H; m.b = hidx / H;
    return m;
}

// LDS-DMA staging of a [64 rows][64 cols] bf16 tile (8 x 1 KiB buffer_load ... lds, shared by NW waves) straight into an LDS image; the image's XOR swizzle is
// applied on the per-lane SOURCE address.  Through a buffer descriptor: descriptor + SCALAR tile offset + a loop-invariant per-lane offset, i.e. no
// vector arithmetic per tile (per-lane 64-bit source pointers for global_load_lds cost 12-15 vector instructions per wave-instruction, and these
// kernels are bound by their vector instruction count: rocprofv3 PMC, profiles/r3_attn_pmc.txt).  Rows past `nrows` are not clamped: they belong
// to the next batch entry (finite) or lie beyond the tensor (read as zero); every consumer zeroes their probabilities.
// TR: 0 = row image, 1 = transposed-read image, 2 = transposed-read image with the window swizzle of img_tr_off2 (forward kernel's V),
// 3 = row image with the chunk swizzle of img_row_off2 (forward kernel's K)
template <int NW, int TR>
struct TileDma {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t vo[8 / NW];
    int stride_bytes;
    __device__ __forceinline__ void init(const bf16* p, int64_t row_stride, int64_t elems_left, int wave, int lane) {
        const int64_t bytes = elems_left * 2;
        rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p), 0, (int)(bytes < 0x7fffffff ? bytes : 0x7fffffff), 0x00020000);
        stride_bytes = (int)row_stride * 2;
#pragma unroll
        for (int i = 0; i < 8 / NW; ++i) {
            const int row = (wave * (8 / NW) + i) * 8 + (lane >> 3), slot = lane & 7;
            const int wswz = TR == 2 ? tr_swz2(row) : ((row >> 1) & 3);
            const int chunk = TR == 0 ? (slot ^ (row & 7)) : TR == 3 ? (slot ^ row_swz2(row)) : ((((slot >> 1) ^ wswz) << 1) | (slot & 1));
            vo[i] = (uint32_t)((row * (int)row_stride + chunk * 8) * 2);
        }
    }
    __device__ __forceinline__ void issue(int row0, char* img, int wave) const {
#if defined(__HIP_DEVICE_COMPILE__)      // (the host pass does not know the builtin)
#pragma unroll
        for (int i = 0; i < 8 / NW; ++i) {
            const int r8 = (wave * (8 / NW) + i) * 8;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_ptr)(img + r8 * 128), 16, vo[i], row0 * stride_bytes, 0, 0);
        }
#else
        (void)row0; (void)img; (void)wave;
#endif
    }
};

// Column sums of a gradient tile for the bias gradient (q_bias / v_bias: the sum of dQ / dV over all rows), taken from the fp32 accumulators BEFORE they are
// rounded and stored: lane (g, c) holds, per 16-wide d-tile dt, the 4 values d = 16 dt + 4 g + r of row c of each of its NT row tiles.  Sum over the valid row
// tiles, over the 16 lanes c of a group (xor 1, 2, 4, 8), over the 4 waves through LDS in wave order: one [64] partial per workgroup, written to
// part[(b * nblk + blk) * D + h * 64 + d] and reduced over (b, blk) in a fixed order by the caller's second stage (devias_colsum_finish): deterministic, no atomics.
// Replaces two column-sum passes over the stored tensor per encoder block (77 MB read each at ViT-B).  `smem` is free: the caller has synchronised after its last tile.
template <int NT>
__device__ __forceinline__ void bias_partials(const f32x4 (&acc)[4][NT], const bool (&valid)[NT], float mul, char* smem, float* __restrict__ part, int64_t slot,
                                              int tid, int lane, int wave) {
    // every lane drops its 16 row-tile sums into LDS ([wave][d = 16 dt + 4 g + r][c], 16 KB), then thread d < 64 of the workgroup adds the 4 x 16 entries of its
    // column in a fixed order (cross-lane shuffles cost this epilogue more than the 64 LDS reads do)
    float* red = reinterpret_cast<float*>(smem);
    const int g = lane >> 4, c = lane & 15;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (valid[t]) v += acc[dt][t] * mul;
#pragma unroll
        for (int r = 0; r < 4; ++r) red[(wave * 64 + 16 * dt + 4 * g + r) * 17 + c] = v[r];      // (17: the 16 lanes of a group write 16 different banks, the 4 groups too)
    }
    __syncthreads();
    if (tid < 64) {
        float t4[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float* p = red + (w * 64 + tid) * 17;
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) a += p[i];
            t4[w] = a;
        }
        part[slot + tid] = (t4[0] + t4[1]) + (t4[2] + t4[3]);
    }
}

}  // namespace attn_units
