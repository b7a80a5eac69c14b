// devias_wgrad_group: the weight gradients of several products, dW_j[Nout_j, Kin_j] (fp32) = beta_j dW_j + dY_j^T X_j over the SAME M rows, as ONE grouped split-K launch
// (+ one table-driven combine).  Why: a weight-gradient launch of the step costs ~20 us + 1.83 us per K-tile of its longest workgroup; an encoder block's four products
// have 9-36 tiles of 256^2 each and had to be cut into 7-28 short slabs to fill 256 CUs four separate times (1008 partial slabs of 256 KB per block, four reduces).  All
// tiles of all products cost the same (one K range of M rows), so the host plans a short list of ROUNDS (tiles x split, tiles * split <= CUs) over the concatenated tile
// list exactly: long slabs, most tiles unsplit when several blocks are grouped.  One workgroup per CU walks its unit of every round; the body is gemm256_kernel<true, true>'s
// (glds_tile / ktile_generic<true, true> / the same epilogues), a split-1 unit writes dW itself (beta honoured), a split unit its fp32 partial tile; the combine sums the
// partials of every split tile in slab order with splitk_reduce_plain_kernel's arithmetic.  No atomics, no flags, no waiting between workgroups: bitwise reproducible.
// A unit of its own: instantiations beside gemm256_kernel change that kernel's code (gemm256.hip).
#include "gemm_tile256.h"
#include <mutex>
#include <vector>

using namespace gemm_units;

namespace {

enum { WG_MAX_JOBS = 64, WG_MAX_ROUNDS = 64, WG_ROUND_COST = 8 /* K-tiles a further round is charged: its ramp, first operand fetch and epilogue */ };

// one slot of the unit table, [round][workgroup]: job < 0 = nothing to do in this round.  kbeg / nk in K-tiles of 64 rows; part = index of the 256 x 256 fp32 partial
// tile this unit writes, -1 = the unit covers all of K and writes dW
struct WgUnit { int job, tile, kbeg, nk, part, round; };
struct WgTile { int job, tile, part0, split; };                      // one split tile of the combine: its partials are part0 .. part0 + split - 1, in slab order
struct WgJob { const bf16* dY; const bf16* X; float* dW; int ldy, ldx, ldw, tiles_n; float beta; };
struct WgParams { const WgUnit* units; float* ws; int rounds, epi_swap, debug; WgJob jobs[WG_MAX_JOBS]; };
struct WgCombine { const WgTile* tiles; const float* ws; WgJob jobs[WG_MAX_JOBS]; };

__global__ __launch_bounds__(NT2) void wgrad_group_kernel(WgParams q) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    for (int r = 0; r < q.rounds; ++r) {
        // (wave-uniform by construction; said so explicitly, so that the operand bases stay scalar after the first round's stores)
        const WgUnit* up = q.units + (r * (int)gridDim.x + (int)blockIdx.x);
        WgUnit u;
        u.job = __builtin_amdgcn_readfirstlane(up->job); u.tile = __builtin_amdgcn_readfirstlane(up->tile); u.kbeg = __builtin_amdgcn_readfirstlane(up->kbeg);
        u.nk = __builtin_amdgcn_readfirstlane(up->nk); u.part = __builtin_amdgcn_readfirstlane(up->part);
        if (u.job < 0) continue;                               // (the same for every wave of the workgroup)
        const WgJob& job = q.jobs[u.job];
        const int tm = u.tile / job.tiles_n, tn = u.tile - tm * job.tiles_n;       // n fastest, as gemm256_kernel rasterises the weight-gradient tiles
        const int m0 = tm * T2, n0 = tn * T2, kbeg = u.kbeg * 64, nk = u.nk;
        const bf16* A = job.dY;
        const bf16* B = job.X;
        f32x4 acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        glds_tile<true>(A, job.ldy, m0, kbeg, smem, wave, lane);
        glds_tile<true>(B, job.ldx, n0, kbeg, smem + 32768, wave, lane);
        for (int kt = 0; kt < nk; ++kt) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's LDS-DMA for tile kt has landed
            __syncthreads();
            char* cur = smem + (kt & 1) * STAGE2;
            char* nxt = smem + ((kt + 1) & 1) * STAGE2;
            if (kt + 1 < nk) {
                glds_tile<true>(A, job.ldy, m0, kbeg + (kt + 1) * 64, nxt, wave, lane);
                glds_tile<true>(B, job.ldx, n0, kbeg + (kt + 1) * 64, nxt + 32768, wave, lane);
            }
            ktile_generic<true, true>(acc, cur, lane, wm, wn);
        }
        // the epilogues of gemm256_kernel on this unit's destination: a partial tile is a split-K slab of a 256 x 256 product (slab index = part), dW a plain fp32 C
        GemmP p = {};
        p.debug = q.debug;
        p.act = DEVIAS_ACT_NONE; p.c_f32 = 1; p.vec_c = 1; p.vec16 = 1; p.rows_per_scale = 1; p.group_m = 1; p.epi_swap = q.epi_swap;
        int em0 = wm * 128, en0 = wn * 64;
        if (u.part >= 0) { p.split_k = 2; p.ws = q.ws; p.M = T2; p.N = T2; p.ldc = T2; }
        else { p.split_k = 1; p.C = job.dW; p.M = 0; p.N = job.ldw; p.ldc = job.ldw; p.beta = job.beta; em0 += m0; en0 += n0; }
        if (q.epi_swap) epilogue_swap<8>(p, acc, em0, en0, u.part, lane);
        else {
            __syncthreads();                                   // every wave is done reading the operand stages
            epilogue_staged<8, 4>(p, acc, smem + wave * 16384, em0, en0, u.part, lane);
        }
        __syncthreads();                                       // the next round's first LDS-DMA overwrites the stages (and the staged epilogue's regions)
    }
}

// dW tile = beta * dW tile + sum of its partial tiles in slab order (splitk_reduce_plain_kernel's arithmetic); block (x = split tile, y = sixteenth of it)
__global__ __launch_bounds__(256) void wgrad_group_combine_kernel(WgCombine q) {
    const WgTile t = q.tiles[blockIdx.x];
    const WgJob& job = q.jobs[t.job];
    const int tm = t.tile / job.tiles_n, tn = t.tile - tm * job.tiles_n;
    float* C0 = job.dW + (int64_t)tm * T2 * job.ldw + tn * T2;
    const float* w0 = q.ws + (int64_t)t.part0 * (T2 * T2);
    const float beta = job.beta;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int i4 = ((int)blockIdx.y * 4 + it) * 256 + (int)threadIdx.x;      // 16-byte piece of the tile: row i4 / 64, columns 4 * (i4 % 64) ...
        f32x4 v = *reinterpret_cast<const f32x4*>(w0 + (int64_t)i4 * 4);
        for (int z = 1; z < t.split; ++z) v += *reinterpret_cast<const f32x4*>(w0 + ((int64_t)z * (T2 * T2 / 4) + i4) * 4);
        float* c = C0 + (int64_t)(i4 >> 6) * job.ldw + (i4 & 63) * 4;
        if (beta != 0.f) v += beta * *reinterpret_cast<const f32x4*>(c);
        *reinterpret_cast<f32x4*>(c) = v;
    }
}

// ---- the planner (host only) --------------------------------------------------------------------------------------------------------------------------
// T equal tiles, `kt` K-tiles each, `cus` workgroups.  A round gives `tiles` consecutive tiles of the list `split` slabs each (tiles * split <= cus) and lasts
// cdiv(kt, split) K-tiles; rounds run one after the other on every CU.  Minimise sum(cdiv(kt, split) + WG_ROUND_COST): for a round of t tiles the best split is the
// largest that fits, and with a given split taking as many tiles as fit is never worse (the optimum is monotone in the tiles left), so the dynamic programme runs
// over (tiles left, tiles of the next round).  Splits are canonical under gemm_impl's slab rule: per = cdiv(kt, split) K-tiles per slab, split = cdiv(kt, per).
struct Round { int tiles, split; };
int canon_split(int kt, int s) { if (s > kt) s = kt; if (s < 1) s = 1; const int per = (kt + s - 1) / s; return (kt + per - 1) / per; }
std::vector<Round> plan_rounds(int T, int kt, int cus) {
    std::vector<int> cost(T + 1, 0), pick(T + 1, 0);
    for (int n = 1; n <= T; ++n) {
        int best = -1, bt = 0;
        for (int t = 1; t <= n && t <= cus; ++t) {
            const int s = canon_split(kt, cus / t);
            if (t < n && t < cus && canon_split(kt, cus / (t + 1)) == s) continue;      // more tiles at the same split: never worse
            const int c = (kt + s - 1) / s + WG_ROUND_COST + cost[n - t];
            if (best < 0 || c < best) { best = c; bt = t; }
        }
        cost[n] = best; pick[n] = bt;
    }
    std::vector<Round> rounds;
    for (int n = T; n > 0; n -= pick[n]) rounds.push_back(Round{pick[n], canon_split(kt, cus / pick[n])});
    // long slabs first: the rounds without a split write dW and their tiles' operands are the freshest
    for (size_t i = 1; i < rounds.size(); ++i)
        for (size_t j = i; j > 0 && rounds[j].split < rounds[j - 1].split; --j) std::swap(rounds[j], rounds[j - 1]);
    return rounds;
}

struct Plan { std::vector<Round> rounds; std::vector<WgUnit> units; std::vector<WgTile> tiles; int parts = 0; };
// the unit table of a plan: within a round the units are (slab, tile) pairs in XCD-major order exactly as gemm256_kernel orders a split-K launch -- workgroup b takes
// pair (b & 7) * per + (b >> 3), per = cdiv(pairs, 8): the ~cus / 8 workgroups of an XCD stream ONE K range together (profiles/r4_wgrad_xcd.txt)
bool build_plan(const int* job_tiles, int n_jobs, int kt, int cus, Plan& pl) {
    if (n_jobs < 1 || n_jobs > WG_MAX_JOBS || kt < 1 || cus < 8 || (cus & 7)) return false;
    int T = 0;
    for (int j = 0; j < n_jobs; ++j) { if (job_tiles[j] < 1) return false; T += job_tiles[j]; }
    pl.rounds = plan_rounds(T, kt, cus);
    if ((int)pl.rounds.size() > WG_MAX_ROUNDS) return false;
    std::vector<int> tjob(T), ttile(T);
    for (int j = 0, g = 0; j < n_jobs; ++j)
        for (int t = 0; t < job_tiles[j]; ++t, ++g) { tjob[g] = j; ttile[g] = t; }
    pl.units.assign(pl.rounds.size() * (size_t)cus, WgUnit{-1, 0, 0, 0, -1, 0});
    int first = 0;
    for (size_t r = 0; r < pl.rounds.size(); ++r) {
        const int nt = pl.rounds[r].tiles, s = pl.rounds[r].split, per_slab = (kt + s - 1) / s;
        const int total = nt * s, per = (total + 7) >> 3;
        if (s > 1)
            for (int t = 0; t < nt; ++t) pl.tiles.push_back(WgTile{tjob[first + t], ttile[first + t], pl.parts + t * s, s});
        for (int b = 0; b < cus; ++b) {
            const int j = (b & 7) * per + (b >> 3);
            if ((b >> 3) >= per || j >= total) continue;
            const int z = j / nt, t = j - z * nt;
            const int kb = z * per_slab, ke = kb + per_slab < kt ? kb + per_slab : kt;
            pl.units[r * (size_t)cus + b] = WgUnit{tjob[first + t], ttile[first + t], kb, ke - kb, s > 1 ? pl.parts + t * s + z : -1, (int)r};
        }
        if (s > 1) pl.parts += nt * s;
        first += nt;
    }
    return true;
}

// plans and the device copies of their tables, per signature (device, CUs, K-tiles, the jobs' tile counts): a plan is a pure function of it, so the size query and the
// launch of a step that repeats plan once.  At most WG_PLAN_CACHE signatures are kept, oldest out first (its tables are freed: hipFree waits for the device).
enum { WG_PLAN_CACHE = 32 };
struct CachedPlan { std::vector<int> key; Plan plan; WgUnit* d_units; WgTile* d_tiles; };
std::mutex g_plan_mutex;
std::vector<CachedPlan*> g_plans;

// the cached plan of `key` = {device, cus, kt, tiles of job 0, ...} (g_plan_mutex held), built on first use; upload: its tables must be on the device
CachedPlan* find_plan(const std::vector<int>& key, bool upload) {
    CachedPlan* cp = nullptr;
    for (CachedPlan* c : g_plans)
        if (c->key == key) { cp = c; break; }
    if (!cp) {
        cp = new CachedPlan;
        cp->key = key; cp->d_units = nullptr; cp->d_tiles = nullptr;
        if (!build_plan(key.data() + 3, (int)key.size() - 3, key[2], key[1], cp->plan)) { delete cp; return nullptr; }
        if (g_plans.size() >= WG_PLAN_CACHE) {
            CachedPlan* old = g_plans.front();
            g_plans.erase(g_plans.begin());
            if (old->d_units) (void)hipFree(old->d_units);
            if (old->d_tiles) (void)hipFree(old->d_tiles);
            delete old;
        }
        g_plans.push_back(cp);
    }
    if (upload && !cp->d_units) {
        bool ok = hipMalloc(&cp->d_units, cp->plan.units.size() * sizeof(WgUnit)) == hipSuccess &&
                  hipMemcpy(cp->d_units, cp->plan.units.data(), cp->plan.units.size() * sizeof(WgUnit), hipMemcpyHostToDevice) == hipSuccess;
        if (ok && !cp->plan.tiles.empty())
            ok = hipMalloc(&cp->d_tiles, cp->plan.tiles.size() * sizeof(WgTile)) == hipSuccess &&
                 hipMemcpy(cp->d_tiles, cp->plan.tiles.data(), cp->plan.tiles.size() * sizeof(WgTile), hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (cp->d_units) (void)hipFree(cp->d_units);
            if (cp->d_tiles) (void)hipFree(cp->d_tiles);
            cp->d_units = nullptr; cp->d_tiles = nullptr;
            return nullptr;
        }
    }
    return cp;
}
std::vector<int> plan_key(const devias_wgrad_job* jobs, int n_jobs, int cus) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    std::vector<int> key = {dev, cus, jobs[0].M / 64};
    for (int j = 0; j < n_jobs; ++j) key.push_back((jobs[j].Nout / T2) * (jobs[j].Kin / T2));
    return key;
}

int check_jobs(const devias_wgrad_job* jobs, int n_jobs, const char* who) {
    DEVIAS_REQUIRE(jobs && n_jobs >= 1 && n_jobs <= WG_MAX_JOBS, "%s: 1 .. %d jobs, got %d", who, (int)WG_MAX_JOBS, n_jobs);
    DEVIAS_REQUIRE(devias_options()[OPT_GEMM256] != 0, "%s: the 256 x 256 kernels are switched off (option gemm256 = 0)", who);
    for (int j = 0; j < n_jobs; ++j) {
        const devias_wgrad_job& b = jobs[j];
        DEVIAS_REQUIRE(b.M == jobs[0].M, "%s: job %d reduces over %d rows, job 0 over %d", who, j, b.M, jobs[0].M);
        DEVIAS_REQUIRE(b.M > 0 && b.M % 64 == 0 && b.Nout > 0 && b.Nout % T2 == 0 && b.Kin > 0 && b.Kin % T2 == 0 && b.ldy >= b.Nout && b.ldx >= b.Kin &&
                       b.ldy % 8 == 0 && b.ldx % 8 == 0, "%s: job %d (M=%d Nout=%d Kin=%d ldy=%d ldx=%d) is not a whole-tile bf16 weight gradient", who, j, b.M, b.Nout, b.Kin, b.ldy, b.ldx);
    }
    return DEVIAS_OK;
}
int plan_cus(int cus_override) { return cus_override > 0 ? cus_override : devias_policy_gemm_cus(); }

}  // namespace

extern "C" int32_t devias_policy_wgrad_group_plan(const int32_t* job_tiles, int32_t n_jobs, int32_t k_tiles, int32_t cus, int32_t* rounds, int32_t rounds_cap,
                                                  int32_t* units, int32_t units_cap) {
    Plan pl;
    if (!job_tiles || !build_plan(job_tiles, n_jobs, k_tiles, cus, pl)) return devias_set_error(DEVIAS_EINVAL, "devias_policy_wgrad_group_plan: bad arguments"), -1;
    const int nr = (int)pl.rounds.size();
    if (rounds) {
        if (rounds_cap < nr) return devias_set_error(DEVIAS_EINVAL, "devias_policy_wgrad_group_plan: %d rounds, room for %d", nr, rounds_cap), -1;
        for (int r = 0; r < nr; ++r) { rounds[2 * r] = pl.rounds[r].tiles; rounds[2 * r + 1] = pl.rounds[r].split; }
    }
    if (units) {
        if (units_cap < nr * cus) return devias_set_error(DEVIAS_EINVAL, "devias_policy_wgrad_group_plan: %d units, room for %d", nr * cus, units_cap), -1;
        for (size_t i = 0; i < pl.units.size(); ++i) {
            const WgUnit& u = pl.units[i];
            int32_t* o = units + 6 * i;
            o[0] = u.job; o[1] = u.tile; o[2] = u.kbeg; o[3] = u.nk; o[4] = u.part; o[5] = u.round;
        }
    }
    return nr;
}

extern "C" int64_t devias_wgrad_group_workspace_bytes(const devias_wgrad_job* jobs, int32_t n_jobs, int32_t cus_override) {
    if (check_jobs(jobs, n_jobs, "devias_wgrad_group_workspace_bytes")) return -1;
    std::lock_guard<std::mutex> lock(g_plan_mutex);
    const CachedPlan* cp = find_plan(plan_key(jobs, n_jobs, plan_cus(cus_override)), false);
    if (!cp) return devias_set_error(DEVIAS_EINVAL, "devias_wgrad_group_workspace_bytes: no plan"), -1;
    return (int64_t)cp->plan.parts * T2 * T2 * 4;
}

extern "C" int devias_wgrad_group(const devias_wgrad_job* jobs, int32_t n_jobs, int32_t cus_override, void* ws, int64_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc = check_jobs(jobs, n_jobs, "devias_wgrad_group");
    if (rc) return rc;
    for (int j = 0; j < n_jobs; ++j)
        DEVIAS_REQUIRE(jobs[j].dY && jobs[j].X && jobs[j].dW && aligned16(jobs[j].dY) && aligned16(jobs[j].X) && aligned16(jobs[j].dW), "devias_wgrad_group: job %d: null / unaligned operand", j);
    const int cus = plan_cus(cus_override), kt = jobs[0].M / 64;
    DEVIAS_REQUIRE(cus >= 8 && cus % 8 == 0 && cus <= (devias_device_cus() & ~7), "devias_wgrad_group: %d workgroups (a multiple of 8, at most the device's CUs)", cus);
    // (the launch below happens under the lock: an eviction by another thread frees tables only after waiting for the device, never between lookup and launch)
    std::lock_guard<std::mutex> lock(g_plan_mutex);
    const CachedPlan* cp = find_plan(plan_key(jobs, n_jobs, cus), true);
    if (!cp) return devias_set_error(DEVIAS_EINVAL, "devias_wgrad_group: cannot plan or upload the unit table (%d jobs, %d K-tiles, %d workgroups)", n_jobs, kt, cus);
    const Plan& pl = cp->plan;
    DEVIAS_REQUIRE(pl.parts == 0 || (ws && aligned16(ws) && ws_bytes >= (int64_t)pl.parts * T2 * T2 * 4), "devias_wgrad_group: workspace too small (%lld bytes needed)",
                   (long long)pl.parts * T2 * T2 * 4);
    const int* opt = devias_options();
    WgParams q;
    q.units = cp->d_units; q.ws = reinterpret_cast<float*>(ws); q.rounds = (int)pl.rounds.size(); q.epi_swap = opt[OPT_GEMM_EPI]; q.debug = 0;
    WgCombine cq;
    cq.tiles = cp->d_tiles; cq.ws = reinterpret_cast<const float*>(ws);
    for (int j = 0; j < n_jobs; ++j) {
        const WgJob jb = {reinterpret_cast<const bf16*>(jobs[j].dY), reinterpret_cast<const bf16*>(jobs[j].X), jobs[j].dW, jobs[j].ldy, jobs[j].ldx, jobs[j].Kin,
                          jobs[j].Kin / T2, jobs[j].beta};
        q.jobs[j] = jb; cq.jobs[j] = jb;
    }
    for (int j = n_jobs; j < WG_MAX_JOBS; ++j) { q.jobs[j] = q.jobs[0]; cq.jobs[j] = q.jobs[0]; }
    hipLaunchKernelGGL(wgrad_group_kernel, dim3(cus), dim3(NT2), 0, st, q);
    DEVIAS_CHECK_LAUNCH("devias_wgrad_group");
    for (int j = 0; j < n_jobs; ++j) devias_count(DEVIAS_CNT_GEMM256);      // which kernel family served each product
    if (!pl.tiles.empty()) {
        hipLaunchKernelGGL(wgrad_group_combine_kernel, dim3((unsigned)pl.tiles.size(), 16), dim3(256), 0, st, cq);
        DEVIAS_CHECK_LAUNCH("devias_wgrad_group(combine)");
        devias_count(DEVIAS_CNT_SPLITK_REDUCE);
    }
    return DEVIAS_OK;
}
