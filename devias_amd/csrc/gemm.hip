// devias_gemm for gfx950: C[M,N] = epi( op(A)[M,K] * op(B)[K,N] ).  The host side: validation, the choice of a kernel family and its launch (each family's
// kernel and template ladder live in units of their own: gemm128.h, gemm256.hip, gemm256p.h, gemm256w.hip, gemm_ss.hip, gemm_smallm.hip; what they
// share: gemm_common.h, gemm_tile256.h), the dynamic tile queue's ring, the split-K / column-sum reduction kernels and the in-step timer.
#include "gemm_common.h"
#include <mutex>
#include <atomic>

using namespace gemm_units;

namespace {

// the tile-queue ring (layout: gemm_common.h).  No kernel names it: the host finds it with hipGetSymbolAddress (tile_queue_slot below) and hands a launch its slot
// in GemmP, so it is defined HERE and nowhere else -- a definition in a shared header would give every unit's code object a ring of its own.
__device__ unsigned int g_tile_queue[TQ_RING][TQ_SLOT];

// C[i] = epilogue(sum_s ws[s][i])   (fixed summation order -> bitwise reproducible); the full fused epilogue is available
// here too so that small-M, long-K GEMMs (the B*S = 64-row slot MLPs) can be split along K to fill the chip
template <typename T>
__global__ void splitk_reduce_kernel(GemmP p) {
    const int64_t total = (int64_t)p.M * p.N;
    const T* res = reinterpret_cast<const T*>(p.res);
    const T* aux_in = reinterpret_cast<const T*>(p.aux_in);
    T* aux_out = reinterpret_cast<T*>(p.aux_out);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        float v = 0.f;
        for (int z = 0; z < p.split_k; ++z) v += p.ws[(int64_t)z * total + i];
        const int m = (int)(i / p.N), n = (int)(i % p.N);
        if (p.bias) v += p.bias[n];
        if (p.act == DEVIAS_ACT_GELU) {
            if (aux_out) aux_out[(int64_t)m * p.ld_aux + n] = from_f32<T>(v);
            v = gelu_t<T>(v);
        } else if (p.act == DEVIAS_ACT_RELU) v = fmaxf(v, 0.f);
        else if (p.act == DEVIAS_ACT_SIGMOID) v = 1.0f / (1.0f + expf(-v));
        else if (p.act == DEVIAS_ACT_DGELU) v *= dgelu_t<T>(to_f32(aux_in[(int64_t)m * p.ld_aux + n]));
        else if (p.act == DEVIAS_ACT_DRELU) v = to_f32(aux_in[(int64_t)m * p.ld_aux + n]) > 0.f ? v : 0.f;
        if (p.row_scale) v *= p.row_scale[m / p.rows_per_scale];
        if (res) v += to_f32(res[(int64_t)(p.res_mod > 0 ? m % p.res_mod : m) * p.ldr + n]);
        if (p.c_f32) {
            float* c = reinterpret_cast<float*>(p.C) + (int64_t)m * p.ldc + n;
            *c = v + (p.beta != 0.f ? p.beta * *c : 0.f);
        } else {
            reinterpret_cast<T*>(p.C)[(int64_t)m * p.ldc + n] = from_f32<T>(v);
        }
    }
}

// the weight-gradient case of the reduce (fp32 C with ldc == N, no epilogue beyond beta): 16 bytes per lane, no per-element div/mod
__global__ __launch_bounds__(256) void splitk_reduce_plain_kernel(const float* __restrict__ ws, int split_k, int64_t total4, float* __restrict__ C, float beta) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (int64_t)gridDim.x * 256) {
        f32x4 v = *reinterpret_cast<const f32x4*>(ws + i * 4);
        for (int z = 1; z < split_k; ++z) v += *reinterpret_cast<const f32x4*>(ws + ((int64_t)z * total4 + i) * 4);
        if (beta != 0.f) v += beta * *reinterpret_cast<const f32x4*>(C + i * 4);
        *reinterpret_cast<f32x4*>(C + i * 4) = v;
    }
}

// out[n] = beta*out[n] + sum_p part[p][n]; block (64 columns, 16 partial lanes), fixed order
__global__ void gemm_colsum_final_kernel(const float* __restrict__ part, int nparts, int N, float* __restrict__ out, float beta) {
    __shared__ float sm[16][64];
    int n = blockIdx.x * 64 + threadIdx.x;
    float s = 0.f;
    if (n < N)
        for (int i = threadIdx.y; i < nparts; i += 16) s += part[(int64_t)i * N + n];
    sm[threadIdx.y][threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.y == 0 && n < N) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += sm[k][threadIdx.x];
        out[n] = t + (beta != 0.f ? beta * out[n] : 0.f);
    }
}

}  // namespace

extern "C" int64_t devias_gemm_workspace_bytes(int32_t M, int32_t N, int32_t split_k) {
    return split_k > 1 ? (int64_t)split_k * M * N * 4 : 0;
}

// The tile-queue ring of the CURRENT device's copy of the code object, and this launch's place in it.  The ring's protocol (launch n zeroes the slot of
// launch n + TQ_RING / 2) is only sound while the launches that use one ring are ordered among themselves: the ring therefore belongs to ONE stream per
// device -- the first that launches a dynamic-queue GEMM on it -- and has its own launch counter.  A launch on any other stream of that device gets no slot
// (nullptr) and walks the static tile lists instead: same tiles, same bits (one process-wide counter let a second stream or a second GPU reach a
// slot that was never zeroed, or have it zeroed mid-launch -- tiles silently not computed).  devias_gemm_release_queue_stream() hands the ring to a new owner.
namespace {
struct TileQueueRing { unsigned int* base; hipStream_t owner; bool owned; unsigned seq; };
std::mutex g_tq_mutex;
TileQueueRing g_tq_ring[16];
}
static bool tile_queue_slot(hipStream_t st, unsigned int** slot, unsigned int** clear) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
    std::lock_guard<std::mutex> lock(g_tq_mutex);
    TileQueueRing& r = g_tq_ring[dev];
    if (!r.base) {
        void* sym = nullptr;
        if (hipGetSymbolAddress(&sym, HIP_SYMBOL(g_tile_queue)) != hipSuccess || !sym) { (void)hipGetLastError(); return false; }
        r.base = reinterpret_cast<unsigned int*>(sym);
    }
    if (!r.owned) { r.owner = st; r.owned = true; }
    if (r.owner != st) return false;
    const unsigned n = r.seq++;
    *slot = r.base + (size_t)(n % TQ_RING) * TQ_SLOT;
    *clear = r.base + (size_t)((n + TQ_RING / 2) % TQ_RING) * TQ_SLOT;
    return true;
}
// The caller promises that every dynamic-queue launch of the current device's owner stream has completed (e.g. after a device synchronise): the whole ring
// is zeroed on `stream`, which becomes the new owner.
extern "C" int devias_gemm_release_queue_stream(void* stream) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return devias_set_error(DEVIAS_EINVAL, "devias_gemm_release_queue_stream: no current device");
    std::lock_guard<std::mutex> lock(g_tq_mutex);
    TileQueueRing& r = g_tq_ring[dev];
    if (r.base && hipMemsetAsync(r.base, 0, sizeof(unsigned int) * TQ_RING * TQ_SLOT, (hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return devias_set_error(DEVIAS_EINVAL, "devias_gemm_release_queue_stream: cannot zero the ring");
    }
    r.owner = (hipStream_t)stream; r.owned = true; r.seq = 0;
    return DEVIAS_OK;
}

// CUs the big-tile grids may count on: the device's, minus the reserve (option gemm_reserve_cus), in whole XCD rows.  The persistent kernels' static tile
// lists assume one resident workgroup per CU of the grid: with K CUs held by another kernel (RCCL during backward at N > 1) the K workgroups that find no
// CU run AFTER the others -- a doubled tail, measured +17 % on the step with 8-32 CUs held (bench.py --cu-hog)
extern "C" int32_t devias_policy_gemm_cus(void) {
    const int ncu = devias_device_cus(), reserve = devias_options()[OPT_GEMM_RESERVE_CUS];
    return (ncu - reserve > 8 ? ncu - reserve : 8) & ~7;
}

static int gemm_impl(const devias_gemm_args* a, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    // ---- 1. validate, fill GemmP -----------------------------------------------------------------------------------------------------------
    DEVIAS_REQUIRE(a && a->A && a->B && a->C, "devias_gemm: null operand");
    DEVIAS_REQUIRE(a->M > 0 && a->N > 0 && a->K > 0, "devias_gemm: bad dims M=%d N=%d K=%d", a->M, a->N, a->K);
    DEVIAS_REQUIRE(a->dtype == DEVIAS_F32 || a->dtype == DEVIAS_BF16, "devias_gemm: bad dtype %d", a->dtype);
    DEVIAS_REQUIRE(a->act >= 0 && a->act <= DEVIAS_ACT_DRELU, "devias_gemm: bad act %d", a->act);
    if (a->act == DEVIAS_ACT_DGELU || a->act == DEVIAS_ACT_DRELU)
        DEVIAS_REQUIRE(a->aux_in, "devias_gemm: act %d needs aux_in", a->act);
    // leading dimensions: a row stride holds at least the row it strides over (include/devias_amd.h, devias_gemm_args)
    const int a_row = a->trans_a ? a->M : a->K, b_row = a->trans_b ? a->N : a->K;
    DEVIAS_REQUIRE(a->lda >= a_row, "devias_gemm: lda %d is smaller than a row of A (%d, trans_a %d)", a->lda, a_row, a->trans_a);
    DEVIAS_REQUIRE(a->ldb >= b_row, "devias_gemm: ldb %d is smaller than a row of B (%d, trans_b %d)", a->ldb, b_row, a->trans_b);
    DEVIAS_REQUIRE(a->ldc >= a->N, "devias_gemm: ldc %d is smaller than N %d", a->ldc, a->N);
    if (a->aux_in || a->aux_out) DEVIAS_REQUIRE(a->ld_aux >= a->N, "devias_gemm: ld_aux %d is smaller than N %d", a->ld_aux, a->N);
    if (a->res) DEVIAS_REQUIRE(a->ldr >= a->N, "devias_gemm: ldr %d is smaller than N %d", a->ldr, a->N);
    const int* opt = devias_options();
    const int es = a->dtype == DEVIAS_BF16 ? 2 : 4;
    const int ch = 16 / es;
    GemmP p;
    p.A = a->A; p.B = a->B; p.C = a->C;
    p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldb = a->ldb; p.ldc = a->ldc;
    p.bias = a->bias; p.act = a->act; p.aux_in = a->aux_in; p.aux_out = a->aux_out; p.ld_aux = a->ld_aux;
    p.res = a->res; p.ldr = a->ldr; p.res_mod = a->res_mod;
    p.c_f32 = (a->c_f32 || a->dtype == DEVIAS_F32) ? 1 : 0;
    p.beta = p.c_f32 ? a->beta : 0.f;
    p.tiles_m = cdiv(a->M, BM); p.tiles_n = cdiv(a->N, BN);
    const int BK = a->dtype == DEVIAS_BF16 ? 64 : 16;
    int split = a->split_k > 1 ? a->split_k : 1;
    if (split > 1) {
        DEVIAS_REQUIRE(a->ws, "devias_gemm: split_k needs a workspace");
        int kps = cdiv(cdiv(a->K, split), BK) * BK;
        split = cdiv(a->K, kps);
        p.k_per_split = kps;
    } else {
        p.k_per_split = a->K;
    }
    p.split_k = split; p.ws = a->ws;
    p.colsum_part = nullptr;
    p.row_scale = a->row_scale; p.rows_per_scale = a->rows_per_scale > 0 ? a->rows_per_scale : 1;
    // vector (16-byte) staging needs aligned bases / leading dims and whole chunks along the contiguous dim
    bool vec = aligned16(a->A) && aligned16(a->B) && (a->lda % ch == 0) && (a->ldb % ch == 0);
    vec = vec && (a->trans_a ? (a->M % ch == 0) : (a->K % ch == 0));
    vec = vec && (a->trans_b ? (a->N % ch == 0) : (a->K % ch == 0));
    if (a->batch > 1) vec = vec && (a->stride_a % ch == 0) && (a->stride_b % ch == 0);
    // 4-wide epilogue accesses
    bool vc = (a->N % 4 == 0) && (a->ldc % 4 == 0) && (p.c_f32 ? aligned16(a->C) : aligned8(a->C));
    if (a->bias) vc = vc && aligned16(a->bias);
    if (a->res) vc = vc && (a->ldr % 4 == 0) && aligned8(a->res);
    if (a->aux_in) vc = vc && (a->ld_aux % 4 == 0) && aligned8(a->aux_in);
    if (a->aux_out) vc = vc && (a->ld_aux % 4 == 0) && aligned8(a->aux_out);
    if (es == 4) vc = vc && (!a->res || aligned16(a->res)) && (!a->aux_in || aligned16(a->aux_in)) &&
                      (!a->aux_out || aligned16(a->aux_out)) && aligned16(a->C);
    if (a->batch > 1) vc = vc && (a->stride_c % 4 == 0);
    p.vec_c = vc ? 1 : 0;
    const int batch = a->batch > 1 ? a->batch : 1;
    p.sA = batch > 1 ? a->stride_a : 0; p.sB = batch > 1 ? a->stride_b : 0; p.sC = batch > 1 ? a->stride_c : 0;
    if (batch > 1)
        DEVIAS_REQUIRE(split == 1 && !a->colsum && !a->res && !a->aux_in && !a->aux_out && batch <= 65535,
                       "devias_gemm: batched launches support bias / activation epilogues only (no split-K, residual, aux, colsum)");
    if (a->colsum)
        DEVIAS_REQUIRE(split == 1 && a->ws && !(a->c_f32 && a->dtype == DEVIAS_BF16),
                       "devias_gemm: colsum needs split_k == 1, a workspace (M/128 * N floats) and a T-typed C");
    p.debug = opt[OPT_GEMM_DEBUG];
    p.tail_split = opt[OPT_GEMM_TAIL_SPLIT];
    p.aux_nt = opt[OPT_GEMM_AUX_NT];
    // C non-temporal too (bit 2) for the GELU launch with a second output: fc1 writes 2 x 308 MB per launch at B = 32, more than any cache keeps for its consumer, and written
    // through the XCDs' L2s they displace the operand panels (the fat tail of fc1's K loops, profiles/r6_gemm_pstamps.txt).  In-process A/B (profiles/r6_ab_inproc.txt): the second
    // output alone -0.03 ... -0.17 ms, BOTH -0.34 ... -0.41 ms on top (C alone +0.30); the same for qkv's output (+0.08) or dfc2's (+0.20, its consumers are the next two launches): no.
    p.c_nt = ((opt[OPT_GEMM_AUX_NT] & 4) && a->aux_out) ? 1 : 0;
    p.epi_swap = opt[OPT_GEMM_EPI];
    p.tq = nullptr; p.tq_clear = nullptr; p.tq_nwhole[0] = p.tq_nwhole[1] = p.tq_items[0] = p.tq_items[1] = 0;
    // rasterisation (measured, tools/gemm_ablate.py): wide outputs (N >= 2048) gain 7-10 % from 8-row-tile groups (the
    // weight panel set of a group stays in the XCD's L2); narrow ones and the wgrad reductions are best n-fastest
    p.group_m = opt[OPT_GEMM_GROUPM] > 0 ? opt[OPT_GEMM_GROUPM] : ((!a->trans_a && a->N >= 2048) ? 8 : 1);
    // 16 bytes per lane in the staged epilogue (8 bf16 / 2 x 4 fp32): leading dims % 8 and 16-byte aligned bases
    const bool v16 = vc && (a->N % 8 == 0) && (a->ldc % 8 == 0) && aligned16(a->C) && (!a->bias || aligned16(a->bias)) &&
                     (!a->res || ((a->ldr % 8 == 0) && aligned16(a->res))) &&
                     (!a->aux_in || ((a->ld_aux % 8 == 0) && aligned16(a->aux_in))) &&
                     (!a->aux_out || ((a->ld_aux % 8 == 0) && aligned16(a->aux_out))) && (split == 1 || aligned16(a->ws));
    p.vec16 = (v16 && a->dtype == DEVIAS_BF16) ? 1 : 0;

    // ---- 2. choose the kernel family and its form ------------------------------------------------------------------------------------------
    // Measured on MI355X at the ViT-B shapes (M = 50176; tools/gemm_block_shapes.py, tools/ab_bench.py):
    //   * 256x256 two-stage LDS-DMA kernel (1 workgroup/CU): every shape it can tile, all four operand layouts; its persistent form
    //     (gemm256p_kernel) when there is more than one round of tiles, no split-K and a bf16 output (forward and dgrad GEMMs);
    //   * 256x128 single-stage kernel (2 workgroups/CU): N a multiple of 128 but not of 256;
    //   * 128x128 register-staged kernel: ragged / unaligned / fp32 shapes.
    const int ta = a->trans_a, tb = a->trans_b;
    bool big = opt[OPT_GEMM256] && a->dtype == DEVIAS_BF16 && vec && vc && (a->M % T2 == 0) && (a->N % T2 == 0) && (a->K % 64 == 0) &&
               (p.k_per_split % 64 == 0) && v16 && batch == 1;
    bool ss = opt[OPT_GEMM_SS] != 0 && a->dtype == DEVIAS_BF16 && vec && v16 && (a->M % SS_BM == 0) && (a->N % SS_BN == 0) && (a->K % 64 == 0) &&
              (p.k_per_split % 64 == 0) && batch == 1 && !(ta && !tb);      // (A k-strided with B k-contiguous: no caller; that
                                                                            //  instantiation spilled registers and was removed)
    if (ss && big && (opt[OPT_GEMM_SS] < 0 || (!ta && !tb))) ss = false;
    if (ss) big = false;
    // small-M products (the aggregation block's and the head's B*S-row GEMMs): one launch, no split-K (gemm_smallm_kernel); chosen before the tiled families
    const bool smallm = opt[OPT_GEMM_SMALLM] && a->dtype == DEVIAS_BF16 && !ta && (!tb || opt[OPT_GEMM_SMALLM] == 1) && a->M <= 128 && batch == 1 && !p.c_f32 && !a->colsum && vec && vc &&
                        (a->N % 16 == 0) && (a->K % 128 == 0) && (a->lda % 8 == 0) && (a->ldb % 8 == 0) && (a->ldc % 4 == 0) && aligned8(a->C) &&
                        (!a->bias || aligned16(a->bias)) && (!a->res || (a->ldr % 4 == 0 && aligned8(a->res))) &&
                        (!a->aux_in || (a->ld_aux % 4 == 0 && aligned8(a->aux_in))) && (!a->aux_out || (a->ld_aux % 4 == 0 && aligned8(a->aux_out)));
    // few column groups (N = 768: 48 workgroups on 256 CUs, each streaming all M rows of A over a long K): one workgroup per 16-row tile as well -- the same
    // arithmetic in the same order per output element (bitwise equal), four times the workgroups, a quarter of the A bytes per workgroup.  In the step
    // (R = 64 rows, K = 3072, N = 768: the slot MLP's second layer and the composite output projection; 16 launches of 17.5 us per step):
    // -0.13 ms with the split alone, -0.25 ms with twelve instead of four k-steps of loads in flight per wave (a wave's 24 k-steps are then two round trips to
    // memory instead of six) -- tools/ab_inproc.py gemm_smallm=2,1.  W stored [K, N]: always a workgroup per row tile (the launcher)
    const bool smallm_row_tiles = opt[OPT_GEMM_SMALLM] == 1 && a->M > 16 && a->N / 16 < 128;
    const bool colsum_fused = a->colsum && (ss || big);      // the full-tile kernels fold the column sums into their epilogue
    if (colsum_fused) p.colsum_part = a->ws;
    // The 256x256 family's forms.  Grid of the persistent ones: one workgroup per CU the policy counts on.  With the dynamic queues a reserve is pointless for THEM
    // (a workgroup that finds no CU pulls nothing): they launch on every CU, and gemm_reserve_cus then only sizes the weight-gradient split-K (one round of the CUs left)
    // gemm_dynamic (profiles/r4_cu_hog.txt): the queues are robust to CUs held or slowed by a concurrent kernel, -2.5 ms per step with 16 CUs held during backward; the static
    // lists are 0.3 ms per step faster when the GPU is the step's alone -- hence -1 (default): queues exactly when the host has announced concurrent kernels (gemm_concurrent)
    const int nt = (a->M / T2) * (a->N / T2);
    bool dyn = false, pers = false, w4_ok = false;
    int gp = 0, side = 0;
    if (big && !smallm) {
        dyn = opt[OPT_GEMM_DYNAMIC] > 0 || (opt[OPT_GEMM_DYNAMIC] < 0 && opt[OPT_GEMM_CONCURRENT] != 0);      // (round 6: queues only for fc1, or fc1 + dfc2 -- the launches whose tiles vary most --: -0.09 / -0.03 / -0.04 ms, noise)
        gp = dyn ? (devias_device_cus() & ~7) : devias_policy_gemm_cus();
        // persistent form (more than one round of tiles, no split-K, bf16 output): measured per shape at M = 50176 (tools/gemm_block_shapes.py, same
        // box, one-tile-per-workgroup -> persistent): qkv 226 -> 204 us, fc1 278 -> 243, dfc2 + dGELU + colsum 415 -> 349, dfc2 plain 275 -> 248,
        // dproj 81 -> 72; the long-K dgrad shapes unchanged (dfc1 252, dqkv 192)
        const bool dact = a->act == DEVIAS_ACT_DGELU || a->act == DEVIAS_ACT_DRELU;
        side = a->res ? 1 : (dact ? 2 : 0);      // rows the epilogue reads: a compile-time fact of the persistent kernels
        const bool pers_ok = !ta && split == 1 && !p.c_f32 && p.epi_swap && gp >= 8 && !(a->res && dact) && !(tb && side == 1) &&
                             (!a->row_scale || p.rows_per_scale >= 128) && !(side == 2 && a->bias) && !(side == 1 && a->colsum) &&
                             !(side != 0 && a->aux_out);
        pers = opt[OPT_GEMM_PERSISTENT] && pers_ok && nt > gp;
        // Four-wave form (gemm256w_kernel).  gemm_w4 is a mask over its four instantiations: 1 = B k-contiguous, no side rows; 2 = B k-contiguous + residual;
        // 4 = B k-strided, no side rows; 8 = B k-strided + saved pre-activation; -1 (default) = the measured policy (rounds 4-5: all four where K >= 1024 and N >= 1024 -- every GEMM of ViT-L, none of ViT-B; since round 6: none, below).  Measured IN the step, one process,
        // the option toggled between blocks of ten steps (tools/ab_inproc.py, profiles/r4_dormant_kernels.txt): ViT-L/16 16x224^2 (K = 1024 / 4096) -3.0 ms of
        // 155.8 with all four forms, -2.4 with the k-contiguous two; ViT-B/16 32x320^2 (6400 tokens) -0.4 of 94.3; ViT-B/16 16x224^2 +-0.0 of 53.4 (round 3: +0.3):
        // with "all four where K >= 1024" (ViT-B: fc2, dfc1, dqkv) ViT-B 16x224^2 +0.06 / +0.11 ms, 6400 tokens -0.5, ViT-L -2.45: where the K loop dominates
        // the store drain it wins, at ViT-B's shapes its faster launches are paid back by the clock the part then grants the next kernels.  Timed alone it wins on every k-contiguous shape (qkv -11 %, fc1 -9 %, fc2 -8 %).  It walks static tile lists: when the host
        // announces concurrent kernels the eight-wave kernel with the dynamic queues serves instead.
        // (The stream-K schedule of rounds 2-3 -- gemm256sk_kernel, options gemm_streamk / gemm_sk_* -- is gone: in the same A/B it gained nothing on any
        // BASELINE configuration once the tail split existed: ViT-L -0.2 ms of 153.7 (noise), 6400 tokens +1.5 ms, ViT-B +-0.0; git history has it.)
        const int w4_form = (tb ? 2 : 0) + (side != 0 ? 1 : 0);
        // Round 6, second session: with the eight-wave kernel's specialised epilogues, tail thirds and non-temporal fc1 outputs the measured policy (-1) is NONE -- ViT-L in
        // process (tools/ab_inproc.py --model vit_large gemm_w4=-1,0, the old policy "all four where K >= 1024 and N >= 1024" against none): -0.84 / -0.52 ms of 137.2; forms 1 / 2
        // alone against none +0.22 / -0.01 (profiles/r6_side_configs.txt).  Its N = 1024 shapes have 3.06 rounds of tiles and the four-wave kernel has no tail split.
        const int w4_mask = opt[OPT_GEMM_W4] >= 0 ? opt[OPT_GEMM_W4] : 0;
        w4_ok = pers && !dyn && ((w4_mask >> w4_form) & 1) && !(!tb && side == 2) && a->K >= 128 &&      // (B k-contiguous + saved pre-activation -- dfc2 on a transposed weight copy -- has no four-wave form)
                (a->act == DEVIAS_ACT_NONE || a->act == DEVIAS_ACT_GELU || a->act == DEVIAS_ACT_DGELU || a->act == DEVIAS_ACT_DRELU);
    }
    // the persistent eight-wave kernel's instantiation (launch_gemm256p): the epilogue's switches of this call (EPI of epilogue_swap, option gemm_epi_spec, on by default);
    // -1 = the generic form
    const int epi = !opt[OPT_GEMM_EPI_SPEC] ? -1 : (a->act | (a->bias ? EPI_BIAS : 0) | (a->aux_out ? EPI_AUX : 0) | (a->row_scale ? EPI_RS : 0) | (p.colsum_part ? EPI_CS : 0));

    // ---- 3. launch ------------------------------------------------------------------------------------------------------------------------
    if (smallm) {
        p.split_k = 1; p.k_per_split = a->K;
        launch_gemm_smallm(p, tb != 0, smallm_row_tiles, st);
        devias_count(DEVIAS_CNT_GEMM_SMALLM);
        DEVIAS_CHECK_LAUNCH("devias_gemm(small M)");
        return DEVIAS_OK;
    }
    if (ss) {
        p.tiles_m = a->M / SS_BM; p.tiles_n = a->N / SS_BN;
        launch_gemm_ss(p, ta, tb, st);
        devias_count(DEVIAS_CNT_GEMM_SS);
    } else if (big) {
        p.tiles_m = a->M / T2; p.tiles_n = a->N / T2;
        if (w4_ok) {
            launch_gemm256w(p, tb != 0, side, gp, st);
            devias_count(DEVIAS_CNT_GEMM256P);
            devias_count(DEVIAS_CNT_GEMM256W);
        } else if (pers) {
            // dynamic queue: every XCD queue has at least one (reserved) item per workgroup, at most 32 workgroups per XCD (one claim-mask word)
            unsigned int *tq = nullptr, *tq_clear = nullptr;
            if (dyn && a->K >= 128 && (gp >> 3) <= 32 && (nt >> 3) >= (gp >> 3) && tile_queue_slot(st, &tq, &tq_clear)) {
                // the item list of an XCD queue of cnt tiles -- whole tiles, then the halves of a split partial round -- for the two queue lengths that
                // occur; this launch's ring slot and the one it zeroes (both from the ring of this device AND this stream)
                p.tq = tq;
                p.tq_clear = tq_clear;
                const int stride = gp >> 3;
                for (int v = 0; v < 2; ++v) {
                    const int cnt = (nt >> 3) + (v == 0 ? 1 : 0);
                    const int rfull = cnt / stride, rem = cnt - rfull * stride;
                    const bool tail = opt[OPT_GEMM_TAIL_SPLIT] != 0 && rfull >= 1 && rem > 0 && 2 * rem <= stride;
                    p.tq_nwhole[v] = tail ? rfull * stride : cnt;
                    p.tq_items[v] = tail ? rfull * stride + 2 * rem : cnt;
                }
                devias_count(DEVIAS_CNT_GEMM256D);
            }
            if (p.tq) launch_gemm256p_dyn(p, tb != 0, side, epi, gp, st);
            else launch_gemm256p(p, tb != 0, side, epi, gp, st);
            devias_count(DEVIAS_CNT_GEMM256P);
        } else {
            launch_gemm256(p, ta, tb, opt[OPT_GEMM_SPLITK_XCD] != 0, st);
            devias_count(DEVIAS_CNT_GEMM256);
        }
    } else if (a->dtype == DEVIAS_BF16) {
        launch_gemm128_bf16(p, vec, ta, tb, batch, st);
        devias_count(DEVIAS_CNT_GEMM128_BF16);
    } else {
        launch_gemm128_f32(p, vec, ta, tb, batch, st);
        devias_count(DEVIAS_CNT_GEMM128_F32);
    }
    DEVIAS_CHECK_LAUNCH("devias_gemm");
    if (a->colsum) {
        const DeviasReduceJob cj = {a->ws, a->M / 128, a->N, a->N, a->colsum, a->colsum_beta};
        if (colsum_fused && devias_defer(&cj, 1)) {
            // (second stage taken over by the collecting region)
        } else if (colsum_fused) {
            hipLaunchKernelGGL(gemm_colsum_final_kernel, dim3(cdiv(a->N, 64)), dim3(64, 16), 0, st, a->ws, a->M / 128, a->N, a->colsum, a->colsum_beta);
            DEVIAS_CHECK_LAUNCH("devias_gemm(colsum)");
        } else {
            int rc = devias_colsum(a->C, a->dtype, a->M, a->N, a->ldc, a->colsum, a->colsum_beta, a->ws, stream);
            if (rc) return rc;
        }
    }
    if (split > 1) {
        int64_t total = (int64_t)a->M * a->N;
        int blocks = (int)((total + 255) / 256); if (blocks > 2048) blocks = 2048;
        const bool plain = p.c_f32 && a->ldc == a->N && (total % 4 == 0) && !a->bias && a->act == DEVIAS_ACT_NONE && !a->res && !a->row_scale &&
                           aligned16(a->ws) && aligned16(a->C);
        if (plain) {
            int b4 = (int)((total / 4 + 255) / 256); if (b4 > 2048) b4 = 2048;
            hipLaunchKernelGGL(splitk_reduce_plain_kernel, dim3(b4), dim3(256), 0, st, a->ws, split, total / 4, reinterpret_cast<float*>(a->C), a->beta);
        } else if (a->dtype == DEVIAS_BF16) hipLaunchKernelGGL((splitk_reduce_kernel<bf16>), dim3(blocks), dim3(256), 0, st, p);
        else hipLaunchKernelGGL((splitk_reduce_kernel<float>), dim3(blocks), dim3(256), 0, st, p);
        devias_count(DEVIAS_CNT_SPLITK_REDUCE);
        DEVIAS_CHECK_LAUNCH("devias_gemm(split-k reduce)");
    }
    return DEVIAS_OK;
}

// ---- measurement aid: HIP events around the devias_gemm launches of ONE shape, wherever they are issued from (a fused region in the middle of a real step) --------
// bench.py's roofline.dominant_kernel / probe_fc1_fwd: the kernel's duration as it runs IN the step (operands and caches as the step leaves them, the clock the step
// holds), not in a back-to-back loop on fresh random data (0.396 ms in the loop against ~0.30 ms in the step).  Armed for one shape at a time; a
// launch of that shape is bracketed by an event pair on its own stream (product + split-K reduce + column-sum second stage when they follow inside devias_gemm); at
// most 64 pairs are kept.  Not armed (the default): one predictable branch per call.
namespace {
struct GemmTimer {
    std::mutex mu;
    bool armed = false;
    int M = 0, N = 0, K = 0, ta = 0, tb = 0, n = 0;
    hipEvent_t e0[64], e1[64];
};
GemmTimer& gemm_timer() { static GemmTimer t; return t; }
std::atomic<int> g_gemm_timer_armed{0};
}
extern "C" int devias_debug_gemm_timer_arm(int32_t M, int32_t N, int32_t K, int32_t trans_a, int32_t trans_b) {
    GemmTimer& t = gemm_timer();
    std::lock_guard<std::mutex> lock(t.mu);
    for (int i = 0; i < t.n; ++i) { (void)hipEventDestroy(t.e0[i]); (void)hipEventDestroy(t.e1[i]); }
    t.n = 0;
    t.armed = M > 0;
    t.M = M; t.N = N; t.K = K; t.ta = trans_a != 0; t.tb = trans_b != 0;
    g_gemm_timer_armed.store(t.armed ? 1 : 0);
    return DEVIAS_OK;
}
extern "C" int devias_debug_gemm_timer_read(int32_t* count, float* total_ms) {
    DEVIAS_REQUIRE(count && total_ms, "devias_debug_gemm_timer_read: null output");
    GemmTimer& t = gemm_timer();
    std::lock_guard<std::mutex> lock(t.mu);
    float sum = 0.f;
    for (int i = 0; i < t.n; ++i) {
        float ms = 0.f;
        if (hipEventSynchronize(t.e1[i]) != hipSuccess || hipEventElapsedTime(&ms, t.e0[i], t.e1[i]) != hipSuccess) {
            (void)hipGetLastError();
            return devias_set_error(DEVIAS_ELAUNCH, "devias_debug_gemm_timer_read: event %d not readable", i);
        }
        sum += ms;
    }
    *count = t.n; *total_ms = sum;
    return DEVIAS_OK;
}

extern "C" int devias_debug_gemm_timer_read_each(int32_t* count, float* each_ms, int32_t cap) {
    DEVIAS_REQUIRE(count && each_ms && cap > 0, "devias_debug_gemm_timer_read_each: null output");
    GemmTimer& t = gemm_timer();
    std::lock_guard<std::mutex> lock(t.mu);
    for (int i = 0; i < t.n && i < cap; ++i) {
        float ms = 0.f;
        if (hipEventSynchronize(t.e1[i]) != hipSuccess || hipEventElapsedTime(&ms, t.e0[i], t.e1[i]) != hipSuccess) {
            (void)hipGetLastError();
            return devias_set_error(DEVIAS_ELAUNCH, "devias_debug_gemm_timer_read_each: event %d not readable", i);
        }
        each_ms[i] = ms;
    }
    *count = t.n < cap ? t.n : cap;
    return DEVIAS_OK;
}

extern "C" int devias_gemm(const devias_gemm_args* a, void* stream) {
    if (!g_gemm_timer_armed.load(std::memory_order_relaxed) || !a) return gemm_impl(a, stream);
    GemmTimer& t = gemm_timer();
    int slot = -1;
    {
        std::lock_guard<std::mutex> lock(t.mu);
        if (t.armed && a->M == t.M && a->N == t.N && a->K == t.K && (a->trans_a != 0) == (t.ta != 0) && (a->trans_b != 0) == (t.tb != 0) && t.n < 64 &&
            hipEventCreate(&t.e0[t.n]) == hipSuccess) {
            if (hipEventCreate(&t.e1[t.n]) == hipSuccess) slot = t.n++;
            else (void)hipEventDestroy(t.e0[t.n]);
        }
    }
    if (slot < 0) return gemm_impl(a, stream);
    (void)hipEventRecord(t.e0[slot], (hipStream_t)stream);
    const int rc = gemm_impl(a, stream);
    (void)hipEventRecord(t.e1[slot], (hipStream_t)stream);
    return rc;
}
