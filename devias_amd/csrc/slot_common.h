// What more than one slot cross-attention unit needs.  The kernels live in three units, each with its kernels, the helpers only they use and their host launchers:
//   slot_unfolded.hip  the reference formulation over the K|V stream (up to 8 slots, dh = 512), its finish kernels and the deferred K/V gradient
//   slot_valu.hip      the folded form in VALU arithmetic (fp32 parity mode, S = 3, D = 384), the deferred context gradient's pack kernel, and the two folded finish
//                      kernels: both folded families write their partials in one layout, so one pair of finish kernels serves both
//   slot_mfma.hip      the folded form on the matrix cores (bf16, S in {1, 2, 4}, h S <= 16, D in {512, 768, 1024})
// slot_attn.hip holds the host side: the entry points, validation, the choice of family, counters and workspace arithmetic.
// (No namespace: only these four units include this, and the kernels stay in each unit's anonymous namespace.)
#pragma once
#include "common.h"

enum { MAXS_LIMIT = 8, DH = 512, TCH = 64, TCHM = 128 };   // TCH, TCHM: tokens per workgroup chunk, of the matrix-core kernel (4 tiles of 32)

// The partials of one pass: B h nchunks S row sums, rounded up to 4 floats (the second array stays 16-byte aligned), then as many rows of `width` floats
// (ws_o / ws_z; the backward's ws_q is the second array alone, at offset 0).  bytes = what the *_workspace_bytes queries return: + 64 covers the rounding.
struct SlotPartials { int64_t second, bytes; };      // offset of the second array in floats; size of the whole buffer
static inline SlotPartials slot_partials(int B, int h, int nchunks, int S, int width) {
    const int64_t rows = (int64_t)B * h * nchunks * S;
    return {(rows + 3) & ~(int64_t)3, rows * (width + 1) * 4 + 64};
}
// devias_slotf_workspace_bytes cannot know which folded family will serve the call, so it sizes for the VALU chunk: the smaller chunk, more chunks, the larger buffer
static_assert(TCHM >= TCH, "the folded workspace query sizes for TCH; the matrix-core kernel carves the same buffer by TCHM and must not need more chunks");

// ---- one forward or backward pass of a layer, as the entry points fill it (slot_attn.hip: validate, choose, carve) and the launchers read it.  T = dtype behind every void*;
// names are the unfolded form's, the folded form's in brackets
struct SlotP {
    int dtype;
    const void* q; const void* src;        // q [q'] (not given to the folded backward), kv [ctx]
    float* attn; float* rsum; void* out;   // A, its row sums + 1e-7, o [z]: written by the forward, read by the backward
    const void* d_out; const float* dA_ext; void* dq; float* ds;      // backward: d_o [dz], the optional gradient that arrives at A itself, dq [dq'], ds
    float* ws_r; float* ws_w;              // partials: the forward's row sums; the wide rows ws_o [ws_z] of the forward, ws_q of the backward
    int B, S, N, h, D, nchunks;            // D: dh [context dim]; nchunks = cdiv(N, TCH), for slotm cdiv(N, TCHM): the grid's x, and what ws was carved by
    float scale; hipStream_t st;
};
// the dtype branch of every launcher: f(T{}) with T = bf16 or float (the entry points have checked that dtype is one of the two)
template <typename F> static inline void by_dtype(int dtype, F&& f) { if (dtype == DEVIAS_BF16) f(bf16{}); else f(float{}); }

// ---- the host launchers: the unit of a kernel owns its template ladder, grid and block size; each enqueues one kernel on st, the caller checks the launch
void launch_slot_fwd(const SlotP& p), launch_slot_fwd_finish(const SlotP& p), launch_slot_bwd(const SlotP& p), launch_slot_bwd_finish(const SlotP& p);      // slot_unfolded.hip
void launch_slotf_fwd(const SlotP& p), launch_slotf_bwd(const SlotP& p);                                                                                    // slot_valu.hip
void launch_slotf_fwd_finish(const SlotP& p), launch_slotf_bwd_finish(const SlotP& p);                                                                      // ... after either folded family
void launch_slotm_fwd(const SlotP& p), launch_slotm_bwd(const SlotP& p);                                                                                    // slot_mfma.hip, bf16
void launch_slot_kv_grad(int dtype, const void* q_stack, const void* do_stack, const float* ds_stack, const float* attn_stack, const float* rsum_stack, void* dkv, int L, int B, int S, int N, int h, float scale, hipStream_t st);
void launch_slotf_pack(int dtype, const float* attn_stack, const float* rsum_stack, const float* ds_stack, const void* dz_stack, const void* qp_stack, void* coef, void* vec,
                       int L, int B, int S, int N, int Np, int h, int D, float scale, hipStream_t st);
