// gemm256p_kernel: the persistent eight-wave form of the 256 x 256 LDS-DMA kernel (gemm_tile256.h), static tile lists or dynamic tile queues.
// Included by exactly two units, one per DYN: gemm256p.hip (static lists, the default path) and gemm256.hip (dynamic queues), which keeps either's compile time
// under a third of the former single file's.
#pragma once
#include "gemm_tile256.h"

using namespace gemm_units;

namespace {

// ---- pieces of a split tail tile (gemm256p_kernel) --------------------------------------------------------------------------------------------------------------
// piece code: -1 = the whole tile; 0 / 1 = the two 128-row halves (round 3); 16 + i = third i (row tiles [0, 5) [5, 11) [11, 16) of the tile's sixteen 16-row tiles: at most
// five per wave row, the middle third three in each); 32 + i = quarter i (four row tiles each).  A wave row (wm) owns row tiles [8 wm, 8 wm + 8): its share [il, ih).
__device__ __forceinline__ void piece_rows(int code, int& lo, int& hi) {
    if (code < 0) { lo = 0; hi = 16; }
    else if (code < 16) { lo = 8 * code; hi = lo + 8; }
    else if (code < 32) { const int i = code - 16; lo = i == 0 ? 0 : (i == 1 ? 5 : 11); hi = i == 0 ? 5 : (i == 1 ? 11 : 16); }
    else { lo = 4 * (code - 32); hi = lo + 4; }
}
__device__ __forceinline__ void piece_wave_rows(int code, int wm, int& il, int& ih) {
    int lo, hi;
    piece_rows(code, lo, hi);
    il = max(lo - 8 * wm, 0); ih = min(hi - 8 * wm, 8);
    if (ih < il) ih = il;
}
// does a piece multiply any of the 32 A rows wave w stages (row tiles 2 w, 2 w + 1)?
__device__ __forceinline__ bool piece_needs_wave_rows(int code, int w) {
    int lo, hi;
    piece_rows(code, lo, hi);
    return 2 * w < hi && 2 * w + 2 > lo;
}
// one K-tile of a wave that multiplies only row tiles [IL, IH) of its eight into accumulators of their own (B k-contiguous; compiler-scheduled: a tail piece's K loop is
// bound by the operand stream -- the whole B tile and a part of A for a part of the MFMAs).  A compile-time range: MFMAs under a run-time condition, anywhere in the
// kernel, make the register allocator copy accumulators (256 registers + scratch in every instantiation when this was one routine with a run-time range).
template <int IL, int IH>
__device__ __forceinline__ void ktile_nt_rows(f32x4 (&acc)[IH - IL][4], const char* cur, int lane, int wm, int wn) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[j] = read_frag2<false>(cur + 32768, wn * 64 + j * 16, ks, lane);
#pragma unroll
        for (int i = IL; i < IH; ++i) {
            const bf16x8 fa = read_frag2<false>(cur, wm * 128 + i * 16, ks, lane);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i - IL][j] = mfma16(fb[j], fa, acc[i - IL][j]);
        }
    }
}

// =====================================================================================================================
// Persistent form of the 256 x 256 kernel (split_k == 1, A k-contiguous): one workgroup per CU walks a static list of tiles and the
// K-tile stream of the 2-stage LDS-DMA ring runs ACROSS tile boundaries -- the first K-tile of the next tile is requested before the
// last K-tile of the current one is multiplied, so its fetch (an HBM / L2 round trip that nothing hides in the one-tile-per-workgroup
// kernel) lands under those MFMAs and the register-only epilogue (epilogue_swap).  The epilogue's stores are left in flight:
// the wait at the top of the next tile's first K-tile is a COUNTED vmcnt that covers the LDS-DMA only (vmcnt is in issue order and
// every wave issues >= 16 stores after the DMA), so the output drains under the next tile's MFMAs.
// Tile order: XCD x (block ids congruent to x mod 8) owns the same contiguous range of logical tiles as in xcd_remap; its G/8 workgroups
// stride through it together, so at any moment an XCD works on ~32 consecutive tiles (operand panels shared in its L2).
// =====================================================================================================================
// ---- dynamic tile queue (DYN): queue words, the published-item word, the dequeue (the ring and its constants: gemm_common.h) -----------------------
// Returning agent-scope atomics by lane 0 (or lanes 0-15) of the calling wave, issued from inline asm under a hand-set EXEC mask: invisible to the compiler's
// wait insertion (a visible pending load would turn the K loop's counted waits into vmcnt(0) drains); the result is usable after the caller's next
// s_waitcnt vmcnt(0) that names it.  Wave 0 only, all 64 lanes active at the call.  Each block starts with s_nop 4: the slot pointer may have just been
// reloaded from a lane of the SGPR-spill VGPR (v_readlane = a VALU write of an SGPR), and a vector-memory instruction that reads an SGPR written by the
// VALU needs 5 wait states which the compiler's hazard recogniser does not insert inside inline asm (found as a memory fault at an address with a stale
// high half in the -DDEVIAS_GEMM_DEBUG build, where the pointer lives in a spill lane).
// The dequeue: ticket = head[queue]++, by lane 0.  (Measured and not kept: the same instruction on 16 lanes, the other 15 adding 0 to the other heads and the
// claim masks, so that the ticket arrives with a snapshot of every queue and an empty-handed workgroup knows without a waited look that nothing is left: the
// look it saves costs 1.7 us once per workgroup and launch, the 16-fold atomic traffic cost the step +0.4 ms.)
__device__ __forceinline__ void tq_issue(unsigned& ticket, unsigned int* slot, int queue) {
    const unsigned voff = (unsigned)queue * (TQ_LINE * 4), one = 1u;
    asm volatile("s_nop 4\n\ts_mov_b64 exec, 1\n\tglobal_atomic_add %0, %1, %2, %3 sc0\n\ts_mov_b64 exec, -1" : "+v"(ticket) : "v"(voff), "v"(one), "s"(slot) : "memory");
}
__device__ __forceinline__ void tq_issue_claim(unsigned& old, unsigned int* slot, int queue, unsigned bit) {   // old = mask[queue]; mask[queue] |= bit
    const unsigned voff = TQ_MASKS + (unsigned)queue * (TQ_LINE * 4);
    asm volatile("s_nop 4\n\ts_mov_b64 exec, 1\n\tglobal_atomic_or %0, %1, %2, %3 sc0\n\ts_mov_b64 exec, -1" : "+v"(old) : "v"(voff), "v"(bit), "s"(slot) : "memory");
}
__device__ __forceinline__ void tq_issue_peek(unsigned& snap, unsigned int* slot, int lane) {             // lanes 0-7: the heads, 8-15: the masks (add 0)
    const unsigned voff = (unsigned)(lane & 15) * (TQ_LINE * 4), zero = 0u;
    asm volatile("s_nop 4\n\ts_mov_b64 exec, 0xffff\n\tglobal_atomic_add %0, %1, %2, %3 sc0\n\ts_mov_b64 exec, -1" : "+v"(snap) : "v"(voff), "v"(zero), "s"(slot) : "memory");
}
// WAIT = false: the readers poll for the tag, nobody needs the write to have completed at any particular point
template <bool WAIT>
__device__ __forceinline__ void tq_publish(char* word, unsigned seq, int code) {
    const unsigned v = ((seq & 15u) << 28) | ((unsigned)code & 0x0fffffffu);
    const unsigned addr = (unsigned)(size_t)(__attribute__((address_space(3))) char*)word;
    if constexpr (WAIT) asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" ::"v"(addr), "v"(v) : "memory");
    else asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory");
}
// the item published for position `seq` of this workgroup's item stream: >= 0 (queue << 20 | index), TQ_NONE, or -2 = not published (yet)
__device__ __forceinline__ int tq_read(const char* word, unsigned seq) {
    unsigned v;
    const unsigned addr = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)word;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    v = __builtin_amdgcn_readfirstlane(v);
    return (v >> 28) == (seq & 15u) ? (int)(v & 0x0fffffffu) : -2;
}

template <bool TB, int SIDE, bool DYN, int EPI = -1>
__global__ __launch_bounds__(NT2) void gemm256p_kernel(GemmP p) {
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE2 + (DYN ? 16 : 0)];     // (+ the published next item: ONE LDS object -- a second __shared__ object makes the compiler fence every LDS read behind the LDS-DMA in flight)
    const int tid = threadIdx.x, lane = tid & 63;
#ifdef DEVIAS_GEMM_DEBUG
    const unsigned long long t_entry = __builtin_amdgcn_s_memrealtime();
#endif
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;
    const int ntiles = p.tiles_m * p.tiles_n;
    const int nk = p.K / 64;
    const bf16* A = reinterpret_cast<const bf16*>(p.A);
    const bf16* B = reinterpret_cast<const bf16*>(p.B);
    // this XCD-group's logical tile range and this workgroup's stride through it (gridDim.x is a multiple of 8)
    const int xcd = blockIdx.x & 7, stride = gridDim.x >> 3;
    const int q = ntiles >> 3, r = ntiles & 7;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    const int cnt = q + (xcd < r ? 1 : 0);
    const int li0 = blockIdx.x >> 3;
    int li = li0;
    if constexpr (!DYN) { if (li >= cnt) return; }
    auto coords = [&](int l, int& m0, int& n0) {
        int tm, tn;
        tile_coords(base + l, p.tiles_m, p.tiles_n, p.group_m, tm, tn);
        m0 = tm * T2; n0 = tn * T2;
    };
    // Tail split: the last, partial round of the group (rem tiles for `stride` workgroups) leaves stride - rem CUs idle for a whole tile time.  When
    // 2 rem <= stride every tail tile goes to TWO workgroups, each computing one 128-row half: in the other half's waves (wm != half) only the operand
    // staging and the barriers run.  The two wave rows of a workgroup share the SIMDs pairwise, so the active row has the matrix cores to itself and the
    // tile's K loop takes a bit more than half its time; every output element is computed by the same wave code as before (bitwise equal).
    const int rfull = cnt / stride, rem = cnt - rfull * stride;
    const bool split = p.tail_split != 0 && rfull >= 1 && rem > 0 && 2 * rem <= stride;
    // Round 6: thirds and quarters.  A half tile costs 0.7 of a tile, not 0.5 (its K loop streams the whole B tile and half of A for half the MFMAs, its epilogue is the
    // active waves' full one: profiles/r6_gemm_pstamps.txt); with 3 rem <= stride (the 588-tile shapes: 9-10 tail tiles for 32 workgroups) the tail tiles go to THREE
    // workgroups, with 4 rem <= stride (fc1: 6 tail tiles) to FOUR: less K-loop stream per piece and a third / a quarter of the epilogue.  Static lists, B k-contiguous,
    // no column sums (option gemm_tail_split >= 3 / 4; 2 = halves only).
    const int parts = (!split || DYN || TB || p.colsum_part != nullptr || p.tail_split < 3) ? 2 : min(min(p.tail_split, 4), stride / rem);
    // STATIC list (DYN = false): this workgroup's k-th tile: (logical index, piece code: -1 = whole tile, see piece_rows); false = none
    auto tile_at = [&](int k, int& l, int& half) -> bool {
        half = -1;
        if (k < rfull) { l = li0 + k * stride; return true; }
        if (k > rfull) return false;
        if (split) {
            if (li0 >= parts * rem) return false;
            l = rfull * stride + li0 / parts;
            half = (parts == 2 ? 0 : (parts == 3 ? 16 : 32)) + li0 % parts;
            return true;
        }
        if (li0 >= rem) return false;
        l = rfull * stride + li0;
        return true;
    };
    // DYNAMIC queue (DYN = true).  Item i of XCD queue y: the whole tile base_y + i for i < nwhole_y, then the two 128-row halves of each tail tile (the same
    // items the static list hands out; only WHO computes an item is decided at run time).  Which workgroup computes a tile does not change a bit of it.
    //   * The first `stride` items of a queue are RESERVED, one per workgroup of that XCD: a workgroup starts on its own (no round trip before the first
    //     LDS-DMA) and claims it with an atomic OR on the queue's mask word, whose answer arrives with that first K-tile.
    //   * The items behind them are handed out by tickets of the queue's head word.  A workgroup always holds its current item and the next one (whose
    //     first K-tile the stream prefetches); the dequeue for the one after is issued by wave 0 during the last K-tile of a tile, is OLDER than that
    //     iteration's LDS-DMA (so the counted wait of the tile switch covers it) and is read a whole tile later, again under the last K-tile: wave 0
    //     publishes the item through the LDS word behind the ring and every wave picks it up after its epilogue.  The K loop is the static kernel's.
    //   * A workgroup whose queue is empty looks at all eight heads and masks at once (one 16-lane instruction), pulls from another XCD's queue, and when
    //     every head is used up takes reserved items nobody has claimed -- those of workgroups that have not found a CU yet because another kernel holds
    //     it (RCCL's during backward; bench.py --cu-hog).  Such a workgroup later finds its claim refused and every queue empty, and leaves: a held or
    //     slowed CU costs its share of the work, not a straggler's tile list.  Only these end-of-launch searches are waited for.
    char* const tq_word = smem + 2 * STAGE2;
    // the queue geometry and the slot pointer as OPAQUE scalars: otherwise every use re-loads them from the kernel-argument segment (an s_load round
    // trip on wave 0's critical path once per tile); opaque values stay in SGPRs or in a lane of the spill VGPR (one v_readlane)
    int nwhole_a = p.tq_nwhole[0], nwhole_b = p.tq_nwhole[1], items_a = p.tq_items[0], items_b = p.tq_items[1];
    unsigned int* tq = p.tq;
    if constexpr (DYN) asm volatile("" : "+s"(nwhole_a), "+s"(nwhole_b), "+s"(items_a), "+s"(items_b), "+s"(tq));
    auto qgeom = [&](int y, int& qbase, int& nwhole, int& items) {
        qbase = y < r ? y * (q + 1) : r * (q + 1) + (y - r) * q;
        nwhole = y < r ? nwhole_a : nwhole_b;
        items = y < r ? items_a : items_b;
    };
    auto decode = [&](int code, int& m0, int& n0, int& half) {
        const int y = code >> 20, i = code & 0xfffff;
        int qbase, nwhole, items;
        qgeom(y, qbase, nwhole, items);
        const int l = i < nwhole ? i : nwhole + ((i - nwhole) >> 1);
        half = i < nwhole ? -1 : ((i - nwhole) & 1);
        int tm, tn;
        tile_coords(qbase + l, p.tiles_m, p.tiles_n, p.group_m, tm, tn);
        m0 = tm * T2; n0 = tn * T2;
    };
    int fq = xcd;                                          // wave 0: the queue whose head the outstanding dequeue went to
    bool fdead = false;                                    // wave 0: nothing is left anywhere
    unsigned ticket = 0, seq = 0;                          // seq = items published to this workgroup so far
    // wave 0, after a wait that covers the dequeue from queue fq: the item (>= 0), or -2 = that queue's head is used up
    auto settle = [&]() -> int {
        const int t = stride + (int)__builtin_amdgcn_readfirstlane(ticket);
        int qbase, nwhole, items;
        qgeom(fq, qbase, nwhole, items);
        return t < items ? ((fq << 20) | t) : -2;
    };
    // wave 0, waited round trips (end of a launch only): look at every head and mask, pull from the first queue that still has tickets (own XCD's
    // neighbours first), else claim an unclaimed reserved item; TQ_NONE when there is nothing
    auto find_elsewhere = [&]() -> int {
        const int lane_f = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        const unsigned wmask = stride >= 32 ? 0xffffffffu : ((1u << stride) - 1u);
        for (int attempt = 0; attempt < 256 && !fdead; ++attempt) {
            unsigned snap = 0;
            tq_issue_peek(snap, tq, lane_f);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(snap) :: "memory");
            int pick = -1, kind = 0;
            unsigned bit = 0;
            for (int d = 1; d <= 8 && pick < 0; ++d) {
                const int y = (xcd + d) & 7;
                int qbase, nwhole, items;
                qgeom(y, qbase, nwhole, items);
                if (stride + (int)__builtin_amdgcn_readlane(snap, y) < items) pick = y;
            }
            for (int d = 0; d < 8 && pick < 0 && !(p.debug & 512); ++d) {     // (gemm_debug & 512: reserved items are not taken over -- bisecting aid)
                const int y = (xcd + d) & 7;
                const unsigned avail = ~(unsigned)__builtin_amdgcn_readlane(snap, 8 + y) & wmask;
                if (avail) { pick = y; kind = 1; bit = avail & (0u - avail); }
            }
            if (pick < 0) { fdead = true; break; }
            if (kind == 0) {
                fq = pick;
                tq_issue(ticket, tq, fq);
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(ticket) :: "memory");
                const int c = settle();
                if (c != -2) return c;
            } else {
                unsigned old = 0;
                tq_issue_claim(old, tq, pick, bit);
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(old) :: "memory");
                if (!((unsigned)__builtin_amdgcn_readfirstlane(old) & bit)) return (pick << 20) | (int)__builtin_ctz(bit);
            }
        }
        fdead = true;
        return (int)TQ_NONE;
    };
    if constexpr (DYN) {
        if (blockIdx.x == 0 && tid < 16)                   // (from asm: the compiler's wait insertion never sees a store pending)
            asm volatile("s_nop 4\n\tglobal_store_dword %0, %1, %2 sc1" ::"v"((unsigned)tid * (TQ_LINE * 4)), "v"(0u), "s"(p.tq_clear) : "memory");
    }
    int tk = 0, half = -1, halfn = -1;
    int m0 = 0, n0 = 0, m0n = 0, n0n = 0;
    bool has_next = false;
    int ncode = -2;
#ifdef DEVIAS_GEMM_DEBUG
    // gemm_debug & 8: thread 0 logs (100 MHz clock << 4 | code) into ws + 64 * blockIdx.x: 1 = first K-tile of a tile about to be multiplied,
    // 2 = K loop done, 3 = epilogue done (stores issued), 4 = first K-iteration of the next tile done (its wait passed)
    int nlog = 0;
    // (with fused column sums the partials own the head of ws: the stamps then live behind them, at float offset M / 128 * N)
    unsigned long long* const stamp_base = reinterpret_cast<unsigned long long*>(p.ws + (p.colsum_part ? (size_t)(p.M / 128) * p.N : 0));
    auto stamp = [&](int code) {
        if (GDBG(8) && tid == 0 && nlog < 64) {
            // codes >= 8 log the SHADER clock counter instead (s_memtime): with the matching 100 MHz stamps that gives the clock the CU really runs at
            const unsigned long long v = ((code >= 8 ? __builtin_amdgcn_s_memtime() : __builtin_amdgcn_s_memrealtime()) << 4) | (unsigned long long)code;
            asm volatile("global_store_dwordx2 %0, %1, %2" ::"v"((uint32_t)nlog * 8), "v"(v), "s"(stamp_base + (size_t)blockIdx.x * 64) : "memory");
        }
        ++nlog;
    };
#define PSTAMP(c) stamp(c)
    if (GDBG(8) && tid == 0) {           // slot 63: the workgroup's entry time
        const unsigned long long v = (t_entry << 4) | 7ull;
        asm volatile("global_store_dwordx2 %0, %1, %2" ::"v"((uint32_t)63 * 8), "v"(v), "s"(stamp_base + (size_t)blockIdx.x * 64) : "memory");
    }
#else
#define PSTAMP(c)
#endif
    f32x4 acc[8][4];
    {
        unsigned claim = 0;
        if constexpr (!DYN) {
            (void)tile_at(0, li, half);
            coords(li, m0, n0);
        } else {
            // start on the reserved item; the claim and the dequeue of the second item travel with the first K-tile's LDS-DMA
            if (wave == 0) {
                tq_issue_claim(claim, tq, xcd, 1u << li0);
                tq_issue(ticket, tq, fq);
            }
            decode((xcd << 20) | li0, m0, n0, half);
        }
        glds_tile<false>(A, p.lda, m0, 0, smem, wave, lane);
        glds_tile<TB>(B, p.ldb, n0, 0, smem + 32768, wave, lane);
        if constexpr (!DYN) {
            int ln = li;
            has_next = tile_at(1, ln, halfn);
            m0n = m0; n0n = n0;
            if (has_next) coords(ln, m0n, n0n);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (!DYN) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(claim), "+v"(ticket) :: "memory");
            if (wave == 0) {
                int c0 = ((unsigned)__builtin_amdgcn_readfirstlane(claim) >> li0) & 1u ? -2 : ((xcd << 20) | li0);    // refused: somebody took it while this
                int c1 = settle();                                                                              // workgroup was waiting for a CU
                if (c0 == -2) { c0 = c1 != -2 ? c1 : find_elsewhere(); c1 = -2; }
                if (c0 == (int)TQ_NONE) c1 = c0;
                else if (c1 == -2) c1 = find_elsewhere();
                tq_publish<true>(tq_word, 0, c0);
                tq_publish<true>(tq_word + 4, 1, c1);
                if (c1 != (int)TQ_NONE && !fdead) tq_issue(ticket, tq, fq);
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            const int code = tq_read(tq_word, 0);
            if (code == (int)TQ_NONE) return;              // every queue was empty: this workgroup came too late to be needed (its DMA has landed)
            if (code != ((xcd << 20) | li0)) {             // (rare) the reserved item was gone: restage the first K-tile of the item found instead
                decode(code, m0, n0, half);
                __builtin_amdgcn_s_barrier();
                glds_tile<false>(A, p.lda, m0, 0, smem, wave, lane);
                glds_tile<TB>(B, p.ldb, n0, 0, smem + 32768, wave, lane);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            ncode = tq_read(tq_word + 4, 1);
            has_next = ncode != (int)TQ_NONE;
            m0n = m0; n0n = n0;
            if (has_next) decode(ncode, m0n, n0n, halfn);
            seq = 2;
        }
        bool act = half < 0 || wm == half;                    // (wave-uniform; thirds / quarters never run in this loop: see `tail_piece` below)
        bool tail_piece = false;
        int gtail = 0;
        // ONE flat loop over the K-tile stream (ring stage = g & 1); the wait for K-tile g + 1 sits at the END of iteration g so that the loop has
        // no first-iteration special case (a peeled copy is where the compiler re-inserts full vmcnt drains)
        for (int g = 0, kt = 0;; ++g) {
            __builtin_amdgcn_s_barrier();                      // K-tile g has landed for every wave, and everyone is done reading stage (g + 1) & 1
            asm volatile("" ::: "memory");
            if (kt == 0) { PSTAMP(1); PSTAMP(9); }
            char* cur = smem + (g & 1) * STAGE2;
            char* nxt = smem + ((g + 1) & 1) * STAGE2;
            // source of K-tile g + 1: this tile's next one, or the next tile's first; at the very end a harmless re-read
            const bool same = kt + 1 < nk;
            const int am = (same || !has_next) ? m0 : m0n, bn = (same || !has_next) ? n0 : n0n;
            const int kn = same ? (kt + 1) * 64 : (has_next ? 0 : kt * 64);
            // the lane id is recomputed per K-tile (v_mbcnt) and made opaque: the per-lane LDS / LDS-DMA offsets derived from it are then cheap VALU work of
            // every iteration instead of registers that stay live across the epilogue, whose register peak is the kernel's (-14 registers)
            int lane_k = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(lane_k));
            // does K-tile g + 1 need the A rows this wave stages?  Not if it belongs to a half tile of the OTHER wave row (nobody multiplies them; tail_split >= 2).
            // With the static lists a half tile is a workgroup's last item; with the queues it can have a successor, whose first K-tile is staged by ITS halves
            // (a wave that multiplies the current tile stages its rows in any case)
            // (K-tile g + 1 belongs to the current item, or to the next one's first K-tile; a wave that multiplies all of its row tiles stages its rows in any case)
            const bool stage_a = p.tail_split < 2 || act || (DYN && !same && has_next && (halfn < 0 || wm == halfn));
            if constexpr (!TB) {
                if (act) ktile_nt_pinned(acc, cur, nxt, A + (int64_t)am * p.lda + kn, p.lda, B + (int64_t)bn * p.ldb + kn, p.ldb, wave, lane_k, wm, wn);
                else {                                       // the other half's waves of a split tail tile: staging only -- and of B only: the A rows a wave
                                                               // stages (32 wave + ...) are the rows of ITS half, which nobody multiplies (tail_split >= 2)
                    if (stage_a) glds_tile<false>(A, p.lda, am, kn, nxt, wave, lane_k);
                    glds_tile<false>(B, p.ldb, bn, kn, nxt + 32768, wave, lane_k);
                }
            } else {
                if (stage_a) glds_tile<false>(A, p.lda, am, kn, nxt, wave, lane_k);
                glds_tile<true>(B, p.ldb, bn, kn, nxt + 32768, wave, lane_k);
                if (act) ktile_generic<false, true>(acc, cur, lane_k, wm, wn);
            }
            if (same) {
                ++kt;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's LDS-DMA for K-tile g + 1 has landed (and, DYN, wave 0's dequeue has returned)
                if (kt == 1) PSTAMP(4);
                continue;
            }
            PSTAMP(2); PSTAMP(10);
            int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            asm volatile("" : "+v"(lane_e));                   // opaque: keeps the epilogue's per-lane address arithmetic out of the registers that live across the K loop
            if (act) epilogue_swap<8, true, SIDE, EPI>(p, acc, m0 + wm * 128, n0 + wn * 64, 0, lane_e);
            if (!has_next) break;
            int m0x = 0, n0x = 0, halfx = -1;
            bool issued = false;                               // (wave 0) one dequeue was issued BEHIND the epilogue's stores
            if constexpr (DYN) {
                PSTAMP(5);
                // The item after `next`, found while the epilogue's stores drain (every wave is about to sit in the counted wait below for that long anyway):
                // its dequeue was issued at the previous tile switch and every K-iteration's vmcnt(0) since has covered it (>= 2 K-tiles per tile, checked by
                // the host).  Wave 0 reads the ticket, publishes the item and issues the following dequeue; every wave then reads the word -- no barrier
                // orders that, so until the tag matches -- and decodes it
                if (wave == 0) {
                    asm volatile("" : "+v"(ticket));           // (the ticket is read here, not where the compiler last saw it written)
                    int c = fdead ? (int)TQ_NONE : settle();
                    if (c == -2) c = find_elsewhere();
                    tq_publish<false>(tq_word, seq, c);
                    issued = c != (int)TQ_NONE && !fdead;
                    if (issued) tq_issue(ticket, tq, fq);
                }
                do { ncode = tq_read(tq_word, seq); } while (ncode == -2);
                ++seq;
                if (ncode != (int)TQ_NONE) decode(ncode, m0x, n0x, halfx);
                PSTAMP(6);
            }
            // the epilogue issued >= 16 stores per wave AFTER the DMA of the next tile's first K-tile: wait for the DMA only, the stores drain under the next MFMAs.
            // (Static list: a tile with a successor is a whole tile, every wave has run the epilogue.  Dynamic queue: a half tile can be followed by an item
            // pulled from another XCD's queue; the waves that only staged it have no stores behind their DMA and wait for everything.)
            // (wave 0's dequeue is one more operation behind the DMA: counted too, or the wait would be for the first store)
            if (DYN && !act) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#if !defined(TQ_EXP) || TQ_EXP != 1
            else if (DYN && issued) asm volatile("s_waitcnt vmcnt(17)" ::: "memory");
#endif
            else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            PSTAMP(3);
            kt = 0;
            ++tk;
            m0 = m0n; n0 = n0n; half = halfn;
            if (!DYN && !TB && half >= 16) { tail_piece = true; gtail = g + 1; break; }      // a third / a quarter of a tail tile: its own loop below (its first K-tile has landed)
            act = half < 0 || wm == half;
            if constexpr (!DYN) {
                int ln = li;
                has_next = tile_at(tk + 1, ln, halfn);
                if (has_next) coords(ln, m0n, n0n);
            } else {
                has_next = ncode != (int)TQ_NONE;
                if (has_next) { m0n = m0x; n0n = n0x; halfn = halfx; }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        // ---- a third / a quarter of a tail tile (static lists, B k-contiguous, no column sums: `parts` above) -------------------------------------------------------------
        // The workgroup's last item, run by its own K loop on accumulators of its own, the wave's row tiles a compile-time range: the K-tile stream continues (the piece's
        // first K-tile was requested under the previous tile's last K-tile and has landed), every wave stages B and the A rows some wave multiplies, a wave with row tiles
        // multiplies them and runs the epilogue over just those; waves of one workgroup take different branches here with the same barriers in each.
        if constexpr (!DYN && !TB && !(EPI >= 0 && (EPI & EPI_CS))) {
            if (tail_piece) {
                int il, ih;
                piece_wave_rows(half, wm, il, ih);
                auto run = [&](auto ilc, auto ihc) {
                    constexpr int IL = decltype(ilc)::value, IH = decltype(ihc)::value, NR = IH > IL ? IH - IL : 1;
                    f32x4 tacc[NR][4];
#pragma unroll
                    for (int i = 0; i < NR; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) tacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const bool stage_a = p.tail_split < 2 || piece_needs_wave_rows(half, wave);
                    for (int kt = 0, g = gtail; kt < nk; ++kt, ++g) {
                        __builtin_amdgcn_s_barrier();          // K-tile g has landed for every wave, and everyone is done reading stage (g + 1) & 1
                        asm volatile("" ::: "memory");
                        char* cur = smem + (g & 1) * STAGE2;
                        char* nxt = smem + ((g + 1) & 1) * STAGE2;
                        int lane_k = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                        asm volatile("" : "+v"(lane_k));
                        if (kt + 1 < nk) {
                            if (stage_a) glds_tile<false>(A, p.lda, m0, (kt + 1) * 64, nxt, wave, lane_k);
                            glds_tile<false>(B, p.ldb, n0, (kt + 1) * 64, nxt + 32768, wave, lane_k);
                        }
                        if constexpr (IH > IL) ktile_nt_rows<IL, IH>(tacc, cur, lane_k, wm, wn);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's LDS-DMA for K-tile g + 1 has landed
                    }
                    if constexpr (IH > IL) {
                        int lane_e = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
                        asm volatile("" : "+v"(lane_e));
                        epilogue_swap<NR, true, SIDE, EPI>(p, tacc, m0 + wm * 128 + IL * 16, n0 + wn * 64, 0, lane_e);
                    }
                };
                using std::integral_constant;
                if (il >= ih) run(integral_constant<int, 0>{}, integral_constant<int, 0>{});
                else if (il == 0 && ih == 5) run(integral_constant<int, 0>{}, integral_constant<int, 5>{});
                else if (il == 5 && ih == 8) run(integral_constant<int, 5>{}, integral_constant<int, 8>{});
                else if (il == 0 && ih == 3) run(integral_constant<int, 0>{}, integral_constant<int, 3>{});
                else if (il == 3 && ih == 8) run(integral_constant<int, 3>{}, integral_constant<int, 8>{});
                else if (il == 0 && ih == 4) run(integral_constant<int, 0>{}, integral_constant<int, 4>{});
                else run(integral_constant<int, 4>{}, integral_constant<int, 8>{});
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the trailing re-read must land before the LDS is released
    }
}
#undef PSTAMP

// The eight-wave persistent kernel's instantiation for a call: operand layout, the rows its epilogue reads (SIDE), static lists or dynamic queues, and -- option
// gemm_epi_spec, on by default -- the epilogue's switches as compile-time facts (EPI, see epilogue_swap) where the call's combination has an instantiation:
// the encoder block's seven (qkv: bias; fc1: bias + GELU + saved pre-activation; proj / fc2 / patch embedding: bias + residual; and, on TRANSPOSED weight copies
// (devias_block_args.W*T: the dgrad GEMMs then read both operands k-contiguous, 9-17 % less K-loop time than with transposing LDS reads), dfc1 / dqkv: nothing; dproj: column
// sums; dfc2: dGELU + column sums).  Everything else (stochastic depth's row scale, ReLU / Sigmoid heads, B k-strided ...) runs the generic form.
template <bool TB, int SIDE, bool DYN, int EPI>
void pers_launch1(dim3 grid, hipStream_t st, const GemmP& p) { hipLaunchKernelGGL((gemm256p_kernel<TB, SIDE, DYN, EPI>), grid, dim3(NT2), 0, st, p); }
template <bool DYN>
void pers_launch(bool tb, int side, int epi, dim3 grid, hipStream_t st, const GemmP& p) {
    if (!tb && side == 0) {
        if (epi == EPI_BIAS) pers_launch1<false, 0, DYN, EPI_BIAS>(grid, st, p);                                                                        // qkv
        else if (epi == (DEVIAS_ACT_GELU | EPI_BIAS | EPI_AUX)) pers_launch1<false, 0, DYN, DEVIAS_ACT_GELU | EPI_BIAS | EPI_AUX>(grid, st, p);         // fc1
        else if (epi == 0) pers_launch1<false, 0, DYN, 0>(grid, st, p);                                                                                 // dfc1, dqkv on a transposed weight copy
        else if (epi == EPI_CS) pers_launch1<false, 0, DYN, EPI_CS>(grid, st, p);                                                                       // dproj
        else pers_launch1<false, 0, DYN, -1>(grid, st, p);
    } else if (!tb && side == 1) {
        if (epi == EPI_BIAS) pers_launch1<false, 1, DYN, EPI_BIAS>(grid, st, p);                                                                        // proj, fc2, patch embedding
        else pers_launch1<false, 1, DYN, -1>(grid, st, p);
    } else if (!tb) {
        if (epi == (DEVIAS_ACT_DGELU | EPI_CS)) pers_launch1<false, 2, DYN, DEVIAS_ACT_DGELU | EPI_CS>(grid, st, p);                                     // dfc2 on a transposed weight copy
        else pers_launch1<false, 2, DYN, -1>(grid, st, p);
    } else if (side == 0) pers_launch1<true, 0, DYN, -1>(grid, st, p);       // B k-strided (a dgrad without a transposed weight copy: hosts of ABI <= 165, the per-kernel path): generic epilogues
    else pers_launch1<true, 2, DYN, -1>(grid, st, p);
}

}  // namespace
