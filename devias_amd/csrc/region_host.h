// Host-side helpers shared by the fused-region units (regions.hip, fusion_head.hip, token_head.hip, distill.hip): the entry points' argument checks and dtype dispatch, the arena carver,
// the Python host's automatic split-K choices restated, and the GEMM / weight-gradient / LayerNorm / column-sum calls a region makes with them.  Every unit that includes
// this file gets its own copy (anonymous namespace); devias_policy_* (regions.hip) export the policies.  The device side of the head units' row kernels: row_kernels.h.
#pragma once
#include "common.h"
#include <stdlib.h>
#include <string.h>

namespace {

inline int64_t al256(int64_t n) { return (n + 255) & ~(int64_t)255; }
inline int esize(int dtype) { return dtype == DEVIAS_BF16 ? 2 : 4; }

// ---- argument checks and the dtype dispatch of the entry points ------------------------------------------------------------------------------------------
inline bool dtype_ok(int dtype) { return dtype == DEVIAS_BF16 || dtype == DEVIAS_F32; }
inline bool row_dim_ok(int D) { return D == 384 || D == 768 || D == 1024; }      // what the one-workgroup-per-row kernels of the head regions hold in registers
// a struct that carries its own size: a caller compiled against another version of the header is refused
#define REQUIRE_STRUCT_SIZE(p, type, who)                                                                                                               \
    DEVIAS_REQUIRE((p)->struct_size == (int32_t)sizeof(type), "%s: " #type ".struct_size is %d, this library's struct has %d bytes (recompile the caller)", who, \
                   (p)->struct_size, (int)sizeof(type))
// f(TypeTag<bf16>{}) or f(TypeTag<float>{}) for a dtype that dtype_ok accepted; inside the generic lambda: using T = typename decltype(tag)::type
template <typename T> struct TypeTag { typedef T type; };
template <typename F> inline void dispatch_t(int dtype, F&& f) {
    if (dtype == DEVIAS_BF16) f(TypeTag<bf16>{}); else f(TypeTag<float>{});
}

// ---- the arena carver: consecutive pieces of a caller-owned buffer, each starting on a 256-byte step ------------------------------------------------------
// Integer arithmetic: the size queries lay the arena out at address 0 (base = nullptr) and read `off`.
struct Arena {
    uintptr_t base; int64_t off = 0;
    explicit Arena(const void* p) : base(reinterpret_cast<uintptr_t>(p)) {}
    char* take(int64_t bytes) { char* q = reinterpret_cast<char*>(base + (uintptr_t)off); off += al256(bytes); return q; }
};

// ---- the split policies of the Python host (devias_amd/ops.py: gemm / wgrad / auto_split_k), restated; tests/test_regions_cpu.py keeps them equal ----
int small_m_split(int M, int N, int K, int trans_a) {
    // (measured in the step, bench.py interleaved: never splitting these costs +2.2 ms, splitting only from K = 1024 up +0.7 ms)
    if (!(M <= 256 && K >= 512 && !trans_a)) return 1;
    const int tiles = cdiv(M, 128) * cdiv(N, 128);
    int s = K / 128;
    const int t = (256 + tiles - 1) / tiles;
    if (t < s) s = t;
    return s > 1 ? s : 1;
}
int wgrad_split(int Nout, int Kin, int Mrows, int dtype) {      // C is [Nout, Kin], the reduction runs over Mrows
    const int bk = dtype == DEVIAS_BF16 ? 64 : 16;
    const int cus = devias_policy_gemm_cus();                   // 256 on MI355X; fewer when CUs are reserved for a concurrent kernel (gemm_reserve_cus)
    int tiles, slots;
    if (bk == 64 && Nout % 256 == 0 && Kin % 128 == 0) { tiles = (Nout / 256) * (Kin / 128); slots = 2 * cus; }     // (tiles x splits) fills ONE round of the 256^2 kernel
    else { tiles = cdiv(Nout, 128) * cdiv(Kin, 128); slots = 3 * cus; }
    if (tiles >= slots || Mrows < 8 * bk) return 1;
    int s = slots / tiles;
    if (Mrows / (4 * bk) < s) s = Mrows / (4 * bk);
    if (s > 64) s = 64;
    return s > 1 ? s : 1;
}

struct Ctx {
    int dtype;
    float* ws; int64_t ws_bytes;
    void* sk_ws; int64_t sk_ws_bytes;
    void* st;
};

// C[M,N] = epi(op(A) op(B)) with the Python host's automatic choices (small-M split-K)
struct Epi {
    const float* bias = nullptr; int act = DEVIAS_ACT_NONE;
    const void* aux_in = nullptr; void* aux_out = nullptr;
    const void* res = nullptr; int res_mod = 0;
    float* colsum = nullptr; float colsum_beta = 0.f;
    const float* row_scale = nullptr; int rows_per_scale = 0;
};
int gemm(const Ctx& c, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int trans_a, int trans_b, const Epi& e,
         int c_f32 = 0, float beta = 0.f, int split_k = 1) {
    devias_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.B = B; a.C = C; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = N;
    a.trans_a = trans_a; a.trans_b = trans_b; a.dtype = c.dtype; a.c_f32 = c_f32;
    a.bias = e.bias; a.act = e.act; a.aux_in = e.aux_in; a.aux_out = e.aux_out; a.ld_aux = N;
    a.res = e.res; a.ldr = N; a.res_mod = e.res_mod; a.beta = beta;
    a.row_scale = e.row_scale; a.rows_per_scale = e.rows_per_scale;
    if (split_k == 1) split_k = small_m_split(M, N, K, trans_a);
    if (e.colsum) { split_k = 1; a.colsum = e.colsum; a.colsum_beta = e.colsum_beta; a.ws = c.ws; }
    a.split_k = split_k;
    if (split_k > 1) {
        if (devias_gemm_workspace_bytes(M, N, split_k) > c.ws_bytes) return devias_set_error(DEVIAS_EINVAL, "fused region: workspace too small for a split-K GEMM (%d x %d x %d)", M, N, split_k);
        a.ws = c.ws;
    }
    return devias_gemm(&a, c.st);
}
// dW[Nout,Kin] (fp32) = beta * dW + dY[M,Nout]^T X[M,Kin]
int wgrad(const Ctx& c, const void* dY, const void* X, float* dW, int M, int Nout, int Kin, float beta = 0.f) {
    Epi e;
    return gemm(c, dY, X, dW, Nout, Kin, M, Nout, Kin, 1, 1, e, 1, beta, wgrad_split(Nout, Kin, M, c.dtype));
}
int gemm_batched(const Ctx& c, const void* A, const void* B, void* C, int c_f32, int M, int N, int K, int lda, int ldb, int ldc, int64_t sa, int64_t sb, int64_t sc,
                 int batch, int trans_a, int trans_b) {
    devias_gemm_args a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.B = B; a.C = C; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.ldc = ldc;
    a.trans_a = trans_a; a.trans_b = trans_b; a.dtype = c.dtype; a.c_f32 = c_f32; a.split_k = 1;
    a.batch = batch; a.stride_a = sa; a.stride_b = sb; a.stride_c = sc;
    return devias_gemm(&a, c.st);
}
int ln_fwd(const Ctx& c, const void* x, const float* g, const float* b, void* y, float* mean, float* rstd, int M, int D, float eps) {
    return devias_layernorm_fwd(x, g, b, y, mean, rstd, M, D, eps, c.dtype, c.st);
}
int ln_bwd(const Ctx& c, const void* dy, const void* x, const float* g, const float* mean, const float* rstd, const void* dres, void* dx, float* dg, float* db,
           float beta_acc, float* dx_colsum, int M, int D) {
    return devias_layernorm_bwd(dy, x, g, mean, rstd, dres, dx, dg, db, beta_acc, dx_colsum, M, D, c.dtype, c.ws, c.st);
}
int colsum(const Ctx& c, const void* x, int M, int N, float* out, float beta = 0.f) { return devias_colsum(x, c.dtype, M, N, N, out, beta, c.ws, c.st); }

#define RUN(call) do { int rc__ = (call); if (rc__) return rc__; } while (0)

int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
int64_t gemm_ws(int M, int N, int K, int trans_a) { return devias_gemm_workspace_bytes(M, N, small_m_split(M, N, K, trans_a)); }
int64_t wgrad_ws(int Nout, int Kin, int M, int dtype) { return devias_gemm_workspace_bytes(Nout, Kin, wgrad_split(Nout, Kin, M, dtype)); }
int64_t colsum_gemm_ws(int M, int N) { return max64((int64_t)cdiv(M, 128) * N * 4, devias_colsum_workspace_bytes(M, N)); }

}  // namespace
