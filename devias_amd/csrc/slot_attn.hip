// Slot cross-attention, host side (agg_block/attention.py:128-140 of the reference): every forward / backward entry point validates, chooses the kernel family, fills one
// SlotP (slot_common.h, which also says which unit holds which kernels) with the carved workspace, and runs the pass.
#include "slot_common.h"

// one pass: the family's kernel over the tokens, then its finish kernel over the partials, each launch checked under its own tag; then the family's counter
static int slot_pass(const SlotP& p, void (*kernel)(const SlotP&), const char* tag, void (*finish)(const SlotP&), const char* finish_tag, int counter) {
    kernel(p);
    DEVIAS_CHECK_LAUNCH(tag);
    finish(p);
    DEVIAS_CHECK_LAUNCH(finish_tag);
    devias_count(counter);
    return DEVIAS_OK;
}

extern "C" int64_t devias_slot_attn_workspace_bytes(int32_t B, int32_t S, int32_t N, int32_t h, int32_t dh) {
    return slot_partials(B, h, cdiv(N, TCH), S, dh).bytes;
}

#define SLOT_COMMON_CHECKS(name)                                                                              \
    DEVIAS_REQUIRE(dh == DH, name ": only dim_head == 512 is built (agg_block/agg_block.py:83), got %d", dh); \
    DEVIAS_REQUIRE(S >= 1 && S <= MAXS_LIMIT, name ": 1 <= num_latents <= 8 supported, got %d", S);                \
    DEVIAS_REQUIRE(B > 0 && N > 0 && h > 0 && (int64_t)B * h <= 65535, name ": bad B/N/h");                  \
    DEVIAS_REQUIRE(dtype == DEVIAS_BF16 || dtype == DEVIAS_F32, name ": bad dtype %d", dtype)

extern "C" int devias_slot_attn_fwd(const void* q, const void* kv, float* attn, float* rsum, void* o, int32_t B, int32_t S,
                                    int32_t N, int32_t h, int32_t dh, float scale, int32_t dtype, float* ws, void* stream) {
    SLOT_COMMON_CHECKS("devias_slot_attn_fwd");
    DEVIAS_REQUIRE(q && kv && attn && rsum && o && ws, "devias_slot_attn_fwd: null pointer");
    DEVIAS_REQUIRE(aligned16(q) && aligned16(kv) && aligned16(o) && aligned16(ws), "devias_slot_attn_fwd: unaligned pointer");
    const int nchunks = cdiv(N, TCH);
    const SlotP p = {dtype, q, kv, attn, rsum, o, nullptr, nullptr, nullptr, nullptr, ws, ws + slot_partials(B, h, nchunks, S, DH).second, B, S, N, h, DH, nchunks, scale, (hipStream_t)stream};
    return slot_pass(p, launch_slot_fwd, "devias_slot_attn_fwd", launch_slot_fwd_finish, "devias_slot_attn_fwd(finish)", DEVIAS_CNT_SLOT);
}

extern "C" int devias_slot_attn_bwd(const void* q, const void* kv, const float* attn, const float* rsum, const void* o, const void* d_o, const float* d_attn_ext, void* dq,
                                    float* ds, int32_t B, int32_t S, int32_t N, int32_t h, int32_t dh, float scale, int32_t dtype, float* ws, void* stream) {
    SLOT_COMMON_CHECKS("devias_slot_attn_bwd");
    DEVIAS_REQUIRE(q && kv && attn && rsum && o && d_o && dq && ds && ws, "devias_slot_attn_bwd: null pointer");
    DEVIAS_REQUIRE(aligned16(q) && aligned16(kv) && aligned16(o) && aligned16(d_o) && aligned16(dq) && aligned16(ws), "devias_slot_attn_bwd: unaligned pointer");
    const SlotP p = {dtype, q, kv, const_cast<float*>(attn), const_cast<float*>(rsum), const_cast<void*>(o), d_o, d_attn_ext, dq, ds, nullptr, ws,
                     B, S, N, h, DH, cdiv(N, TCH), scale, (hipStream_t)stream};
    return slot_pass(p, launch_slot_bwd, "devias_slot_attn_bwd", launch_slot_bwd_finish, "devias_slot_attn_bwd(finish)", DEVIAS_CNT_SLOT);
}

extern "C" int devias_slot_attn_kv_grad(const void* q_stack, const void* do_stack, const float* ds_stack, const float* attn_stack, const float* rsum_stack, void* dkv,
                                        int32_t L, int32_t B, int32_t S, int32_t N, int32_t h, int32_t dh, float scale, int32_t dtype, void* stream) {
    SLOT_COMMON_CHECKS("devias_slot_attn_kv_grad");
    DEVIAS_REQUIRE(L >= 1 && q_stack && do_stack && ds_stack && attn_stack && rsum_stack && dkv, "devias_slot_attn_kv_grad: bad args");
    DEVIAS_REQUIRE(aligned16(q_stack) && aligned16(do_stack) && aligned16(dkv), "devias_slot_attn_kv_grad: unaligned pointer");
    launch_slot_kv_grad(dtype, q_stack, do_stack, ds_stack, attn_stack, rsum_stack, dkv, L, B, S, N, h, scale, (hipStream_t)stream);
    DEVIAS_CHECK_LAUNCH("devias_slot_attn_kv_grad");
    devias_count(DEVIAS_CNT_SLOT);
    return DEVIAS_OK;
}

// ---- folded form ----------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t devias_slotf_workspace_bytes(int32_t B, int32_t S, int32_t N, int32_t h, int32_t D) {
    return slot_partials(B, h, cdiv(N, TCH), S, D).bytes;      // for either family: TCHM >= TCH (slot_common.h)
}

// the matrix-core kernels: bf16, h * S <= 16 slot-head rows, S a power of two (softmax across S aligned adjacent lanes), D = 256 * {2, 3, 4}
static bool slotm_ok(int B, int S, int h, int D, int dtype) {
    return devias_options()[OPT_SLOT_MFMA] && dtype == DEVIAS_BF16 && h * S <= 16 && (S == 1 || S == 2 || S == 4) && (D == 512 || D == 768 || D == 1024) && B <= 65535;
}

#define SLOTF_CHECKS(name)                                                                                                  \
    DEVIAS_REQUIRE(D == 384 || D == 512 || D == 768 || D == 1024, name ": context dim must be 384, 512, 768 or 1024, got %d", D); \
    DEVIAS_REQUIRE(S >= 1 && S <= 4, name ": 1 <= num_latents <= 4 in the folded form, got %d", S);                          \
    DEVIAS_REQUIRE(B > 0 && N > 0 && h > 0 && (int64_t)B * h <= 65535, name ": bad B/N/h");                                 \
    DEVIAS_REQUIRE(dtype == DEVIAS_BF16 || dtype == DEVIAS_F32, name ": bad dtype %d", dtype)

extern "C" int devias_slotf_fwd(const void* qp, const void* ctx, float* attn, float* rsum, void* z, int32_t B, int32_t S, int32_t N,
                                int32_t h, int32_t D, float scale, int32_t dtype, float* ws, void* stream) {
    SLOTF_CHECKS("devias_slotf_fwd");
    DEVIAS_REQUIRE(qp && ctx && attn && rsum && z && ws, "devias_slotf_fwd: null pointer");
    DEVIAS_REQUIRE(aligned16(qp) && aligned16(ctx) && aligned16(z) && aligned16(ws), "devias_slotf_fwd: unaligned pointer");
    const bool mfma = slotm_ok(B, S, h, D, dtype);
    const int nchunks = cdiv(N, mfma ? TCHM : TCH);
    const SlotP p = {dtype, qp, ctx, attn, rsum, z, nullptr, nullptr, nullptr, nullptr, ws, ws + slot_partials(B, h, nchunks, S, D).second, B, S, N, h, D, nchunks, scale, (hipStream_t)stream};
    return slot_pass(p, mfma ? launch_slotm_fwd : launch_slotf_fwd, mfma ? "devias_slotf_fwd(mfma)" : "devias_slotf_fwd", launch_slotf_fwd_finish, "devias_slotf_fwd(finish)",
                     mfma ? DEVIAS_CNT_SLOTM : DEVIAS_CNT_SLOTF_VALU);
}

extern "C" int devias_slotf_bwd(const void* ctx, const float* attn, const float* rsum, const void* z, const void* dz, const float* d_attn_ext, void* dqp, float* ds,
                                int32_t B, int32_t S, int32_t N, int32_t h, int32_t D, float scale, int32_t dtype, float* ws, void* stream) {
    SLOTF_CHECKS("devias_slotf_bwd");
    DEVIAS_REQUIRE(ctx && attn && rsum && z && dz && dqp && ds && ws, "devias_slotf_bwd: null pointer");
    DEVIAS_REQUIRE(aligned16(ctx) && aligned16(z) && aligned16(dz) && aligned16(dqp) && aligned16(ws), "devias_slotf_bwd: unaligned pointer");
    const bool mfma = slotm_ok(B, S, h, D, dtype);
    const SlotP p = {dtype, nullptr, ctx, const_cast<float*>(attn), const_cast<float*>(rsum), const_cast<void*>(z), dz, d_attn_ext, dqp, ds, nullptr, ws,
                     B, S, N, h, D, cdiv(N, mfma ? TCHM : TCH), scale, (hipStream_t)stream};
    return slot_pass(p, mfma ? launch_slotm_bwd : launch_slotf_bwd, mfma ? "devias_slotf_bwd(mfma)" : "devias_slotf_bwd", launch_slotf_bwd_finish, "devias_slotf_bwd(finish)",
                     mfma ? DEVIAS_CNT_SLOTM : DEVIAS_CNT_SLOTF_VALU);
}

extern "C" int devias_slotf_pack(const float* attn_stack, const float* rsum_stack, const float* ds_stack, const void* dz_stack, const void* qp_stack, void* coef, void* vec,
                                 int32_t L, int32_t B, int32_t S, int32_t N, int32_t Np, int32_t h, int32_t D, float scale, int32_t dtype, void* stream) {
    DEVIAS_REQUIRE(attn_stack && rsum_stack && ds_stack && dz_stack && qp_stack && coef && vec, "devias_slotf_pack: null pointer");
    DEVIAS_REQUIRE(L >= 1 && B > 0 && B <= 65535 && S >= 1 && N > 0 && Np >= N && h > 0 && D > 0, "devias_slotf_pack: bad dims");
    DEVIAS_REQUIRE(dtype == DEVIAS_BF16 || dtype == DEVIAS_F32, "devias_slotf_pack: bad dtype %d", dtype);
    launch_slotf_pack(dtype, attn_stack, rsum_stack, ds_stack, dz_stack, qp_stack, coef, vec, L, B, S, N, Np, h, D, scale, (hipStream_t)stream);
    DEVIAS_CHECK_LAUNCH("devias_slotf_pack");
    return DEVIAS_OK;
}
