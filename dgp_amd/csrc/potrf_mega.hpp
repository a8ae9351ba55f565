// The factorisation as ONE persistent launch (potrf mode 1, the default): potrf_mega_kernel -- the pivot chains and the
// workers that pull a host-built task table -- its table on the device and its launch.  What the host decides about a launch
// (potrf_plan.hpp: mega_plan, mega_flatten, the workspace layout) is plain C++ and is checked without a device by
// tools/potrf_table_check.cpp; the tile helpers and the waits are chol_tile.hpp's.
// Compiled by potrf.hip, in one unit with potrf_step.hpp (see there).
#pragma once
#include "chol_tile.hpp"

// ----------------------------------------------------------------------------
// The whole factorisation (with or without the fused inverse) as ONE persistent launch: dataflow over tile versions.
//
// Workgroups 0 .. batch-1 are the pivot CHAINS, one per matrix, alive for all block steps; every other workgroup is a
// WORKER that pulls 64x64-tile tasks from one queue (an agent-scope counter) in the order of a host-built table.
// A chain never hands its critical data to another workgroup: after factoring block k it publishes W_k, solves the
// first panel tile P = A[k+1][k] W_k^T itself, applies it to the next diagonal tile, D = A[k+1][k+1] - P P^T, keeps D
// in registers and factors on.  What it needs from the workers -- A[k+1][k] and A[k+1][k+1] with the panels <= k-1
// applied -- depends only on block k-1, so it is produced while the chain factors block k (look-ahead of one block,
// no launch boundary, no hand-off on the critical path).
// Every tile has a VERSION word: the number of finished visits, or VER_FINAL once nobody will write it again.  A task
// waits (one wave, one flag per lane, bounded) until its output tile has seen all earlier visits and its operand tiles
// are final, takes ONE agent-scope acquire, works with plain loads, stores its tile WRITE-THROUGH (sc1) and publishes
// the new version after every storing wave has drained (MI355X_MICROARCH.md, hand-off recipe R1).  Panel tasks wait
// for the chain's W_k the same way.  Deadlock freedom: the table is a topological order of the task graph and is
// pulled in order, so the oldest unfinished task always has its inputs finished or in progress on a resident
// workgroup; the chains are the first workgroups of the grid.  Every spin is bounded (status word -> DGPAMD_HANDOFF).
// Workers that share a CU with a chain leave at once (the chain is issue- and LDS-bound; see the CU guard above).
// ----------------------------------------------------------------------------

struct MTask {   // potrf_plan.hpp's MegaTask as the kernel loads it
    int4 a;   // as the per-launch tables: what / where (make_task)
    int4 b;   // x: visits of the output tile before this one; y: 1 = this visit makes it final; z: block whose inverse a
              // SOLVE / TDIAG task multiplies with
};
static_assert(sizeof(Task4) == sizeof(int4) && alignof(Task4) == alignof(int4) && offsetof(Task4, y) == offsetof(int4, y) &&
              offsetof(Task4, z) == offsetof(int4, z) && offsetof(Task4, w) == offsetof(int4, w), "Task4 is uploaded as int4");
static_assert(sizeof(Need2) == sizeof(int2) && alignof(Need2) == alignof(int2) && offsetof(Need2, y) == offsetof(int2, y), "Need2 is uploaded as int2");
static_assert(sizeof(MegaTask) == sizeof(MTask) && alignof(MegaTask) == alignof(MTask) && offsetof(MegaTask, b) == offsetof(MTask, b),
              "MegaTask is uploaded as MTask");

struct MegaArgs {
    double *buf[3];
    double *ws;
    int64_t ld, stride_a, stride_ws, n;
    int nbk, batch, inv;
    const MTask *tasks;
    int ntask;               // per matrix
    int nut;                 // the first nut entries of `tasks` form the CRITICAL queue (per block step the look-ahead pair, the first
                             // solve and the catch-up updates: what the chain waits for next), the rest the bulk queue
    int ncrit;               // workers per matrix that serve the critical queue first
    const int2 *chain_need;  // per block k: worker visits of A[k+1][k] and of A[k+1][k+1] the chain waits for
    MegaSync *sync;
    int32_t *ver;            // [batch][VER_PLANES][nbk * nbk]: versions of the tiles of A, T, S; auxiliary words (see T_LOOKD)
    double *logdet;
    int32_t *info;
    long long *trace;
    long long *tlog;         // debug (dgpamd_debug_tasklog): every chain step's and every task's stamps, or null
    const int32_t *pred;     // null, or a device word: the launch does nothing when it is non-zero
    double *piv;             // [batch][ld]: the pivots (second chain form: their logarithms are summed at the end)
    int split;               // 1 (default): a visit whose newest panel has not arrived applies the older ones first (DGPAMD_MEGA_SPLIT=0: off)
    int nowait;              // debug (timing only, results invalid; the host passes 0): the chain does not wait for the workers
    int ngroups;             // The matrices are dealt into this many groups (matrix b: group b % ngroups), the XCDs as well
                             // (XCD x: group x % ngroups; 1, 2, 4 or 8), and a worker takes the tasks of its own group's
                             // matrices first: every XCD has its own L2, so with one queue for all a panel tile was fetched
                             // into all eight of them (PMC: ~4x the algorithmic HBM-side traffic at 12 matrices).
};

// ---- the chain ------------------------------------------------------------------------------------------------------------
// The arithmetic of the chain of rounds 2-3 in the same order (bit-identical results), arranged around what bounded its block
// step (profiles/r03_potrf_phase_trace.txt: 7.0 factor + 0.8 publish + 2.0 wait + 1.7 solve + 3.5 update):
//   * the solve produces P^T in the accumulator layout, P^T = W_k Q^T (operands swapped: the same products in the same order).
//     An accumulator tile is, register for register, an MFMA operand of the next product (the layout duality diagfac.hpp
//     uses), so the update D -= P P^T takes its B operand straight from the wave's own registers and its A operand from the
//     other waves' registers, exchanged through LDS AS THEY STAND: one barrier, no transposition, no staging by halves;
//   * Q and W_k are staged whole (LDQ = 66), so the 40 MFMAs of the solve run without a barrier in between;
//   * only the tiles t <= w of the next diagonal block are updated (the factor reads no others), and NO barrier separates
//     the update from the next factorisation: wave 0 (16 MFMAs) starts eliminating while wave 3 (64) is still updating --
//     it is not needed before the first 16-block's barrier;
//   * W_k is published behind the wait for the panel tile's loads (vmcnt counts in order: the older W stores have drained
//     when the younger loads have landed), not behind a drain of its own;
//   * the panel tile's version word, the log-determinant of block k and the drain of the panel stores ride in the shadow
//     of the next factorisation's first elimination (DiagShadow).
#define LDQ 66   // LDS leading dimension of a whole 64x64 f64 tile: bank(4 row + 2 k), conflict-free ds_read_b64 fragments
// The lower factor L = U^T of a block factored by diag_factor, stored ROW-contiguously: wave w writes rows 16w .. 16w + 15
// of the tile (the 16x16 tiles (w, t), t <= w, transposed inside the wave through `scratch` -- 16 x 16 doubles of LDS per
// wave -- and zeros right of the diagonal): four full 128-byte lines per store instruction where the transposed 8-byte
// stores of diag_store_factor touch sixteen.  Blocks with carried rows (the last one) take diag_store_factor.
template <int wave>
__device__ __forceinline__ void diag_store_factor_rows(const Tile64 &tile, double *Ab, int64_t ld, int lane, double *scratch) {
    const int lm = lane & 15, lu = lane >> 4;
    vlds_double *S = (vlds_double *)scratch + wave * 256;   // element (i, j) at i * 16 + (j ^ i): both passes conflict-free
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t <= wave) {   // L[16w + lu + 4r][16t + lm] = U[16t + lm][16w + lu + 4r]
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(lu + 4 * r) * 16 + (lm ^ (lu + 4 * r))] = tile.v[t][r];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double trv = S[lm * 16 + ((lu + 4 * r) ^ lm)];   // U[16t + lm][16w + lu + 4r]
                Ab[(int64_t)(16 * wave + lu + 4 * r) * ld + 16 * t + lm] = (t == wave && lm > lu + 4 * r) ? 0.0 : trv;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) Ab[(int64_t)(16 * wave + lu + 4 * r) * ld + 16 * t + lm] = 0.0;
        }
    }
}

// P (64x64, row-major in global memory) from P^T in the accumulator layout -- lane l of wave w holds
// P[16w + lm][16t + lu + 4r] in register (t, r) -- as write-through 16-byte stores: the lanes of DPP rows lu and lu ^ 1 hold
// neighbouring columns, so each pair of registers (r0, r1) is exchanged across the two rows (v_permlane16_swap: odd rows of
// the first operand with even rows of the second): the even row ends up with columns (lu, lu + 1) of r0, the odd row with
// columns (lu - 1, lu) of r1.
__device__ __forceinline__ void store_pt_sc1(const d4 (&P)[4], double *Pg, int64_t ld, int wave, int lane) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)Pg, 0, 0x7fffffff, 0x00020000);
    const int lm = lane & 15, lu = lane >> 4, odd = lu & 1;
    const int base = (int)(((int64_t)(16 * wave + lm) * ld + (lu & ~1) + 4 * odd) * 8);   // row 16w + lm, column (lu & ~1) + 4 odd
    // All eight 16-byte values first, each in registers of its own, then the eight stores, then wait states before any of the
    // registers may be rewritten.  (The first form built every value in the same four registers; the compiler rewrote them right
    // behind each store -- with the store's offset in an SGPR it inserts no wait state, LLVM's rule for stores of more than 8
    // bytes -- and with the memory pipeline under load from other processes the store had not read all of its data yet: the first
    // double of the lanes read last held the NEXT pair's value.  Two ranks sharing one GPU: a few wrong factors per thousand
    // launches, tools/gpu_mega_stress_shared.sh; never seen with the device to itself.)
    // Round 5: the constant part of the address rides in the instruction's immediate offset field (voffset + constant) and the soffset
    // operand is the literal 0 -- the form for which LLVM's hazard recogniser inserts the wait states itself (it skips a store whose
    // soffset is a register: the constants above 64 used to be materialised in SGPRs).  The registers of their own and the
    // wait states below stay; tests/test_isa_hazards.py reads the shipped code and fails when a data register of any 16-byte store
    // of the kernel is rewritten too early, or when a store's soffset is a register again.
    u32x4 v[8];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
            const double x = P[t][2 * rp], y = P[t][2 * rp + 1];
            const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
            const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
            v[2 * t + rp].x = lo[0]; v[2 * t + rp].y = hi[0]; v[2 * t + rp].z = lo[1]; v[2 * t + rp].w = hi[1];
        }
#pragma unroll
    for (int q = 0; q < 8; ++q)   // (every value is complete, in registers of its own, before the first store is issued)
        asm volatile("" : "+v"(v[q].x), "+v"(v[q].y), "+v"(v[q].z), "+v"(v[q].w));
#pragma unroll
    for (int q = 0; q < 8; ++q)
        // (one per-lane base offset; the tile / register-pair part is a constant that folds into the instruction's offset field)
        __builtin_amdgcn_raw_buffer_store_b128(v[q], rs, base + (16 * (q >> 1) + 8 * (q & 1)) * 8, 0, 16);
#pragma unroll
    for (int q = 0; q < 4; ++q)   // (alive until here: four more stores have been issued behind each of these)
        asm volatile("" : "+v"(v[q].x), "+v"(v[q].y), "+v"(v[q].z), "+v"(v[q].w));
    // (the last four values stay untouched for sixteen more wait states: the registers are operands of the statement that waits)
    asm volatile("s_nop 7\n\ts_nop 7"
                 : "+v"(v[4].x), "+v"(v[4].y), "+v"(v[4].z), "+v"(v[4].w), "+v"(v[5].x), "+v"(v[5].y), "+v"(v[5].z), "+v"(v[5].w),
                   "+v"(v[6].x), "+v"(v[6].y), "+v"(v[6].z), "+v"(v[6].w), "+v"(v[7].x), "+v"(v[7].y), "+v"(v[7].z), "+v"(v[7].w)
                 :: "memory");
}

// ---- the per-wave parts of the chain's block step as static programs (W = wave: every role decision is a compile-time
// constant; left as run-time conditions on the wave index they became a basic block per instruction, each with its own
// full wait) ----
// W_k -> LDS, row-major (the blocks on and below the diagonal: the solve reads no others)
template <int W>
__device__ __forceinline__ void chain_stage_w(const Tile64 &winv, double *Ws, int lm, int lu) {
#pragma unroll
    for (int I = W; I < 4; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) Ws[(16 * I + lu + 4 * r) * LDQ + 16 * W + lm] = winv.v[I][r];
}
// The next diagonal tile's request (lower 16x16 tiles of row block W, row-contiguous loads).  Its update is dealt so that
// waves 1-3 carry three tiles each and wave 0, which starts the next elimination, one: tile (0, 3) of wave 3's column
// block is computed by wave 1 -- in wave 3's layout, loaded transposed straight from the lower triangle (H) -- and handed
// over through LDS behind the next factorisation's first barrier.
template <int W>
__device__ __forceinline__ void chain_request_next(d4 (&nat)[4], d4 &H, const double *Cn, int64_t ld, int lm, int lu) {
#pragma unroll
    for (int t = (W == 3 ? 1 : 0); t <= W; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            nat[t][r] = __hip_atomic_load(Cn + (int64_t)(16 * W + lu + 4 * r) * ld + 16 * t + lm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (W == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            H[r] = __hip_atomic_load(Cn + (int64_t)(48 + lm) * ld + lu + 4 * r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ void store_pt_sc1(const d4 (&P)[4], double *Pg, int64_t ld, int wave, int lane);
// D = A[k+1][k+1] - P P^T in the column-block layout: wave W's tiles (see chain_request_next), the operands of the other
// waves from the exchange buffer Xc two k-steps ahead of their MFMAs (one wave per SIMD: a read waited for in front of
// its MFMA exposes the LDS latency, ~90 cycles per 64-cycle MFMA).
template <int W>
__device__ __forceinline__ void chain_update(Tile64 &Dn, const d4 (&P)[4], const d4 (&nat)[4], d4 &H, vlds_double *Xc, double *scratch,
                                             vlds_double *hand, double *Pg, int64_t ld, int lane, int *pcount, int ptarget, int32_t *pflag) {
    const int lm = lane & 15, lu = lane >> 4;
    constexpr int T0 = (W == 3 ? 1 : 0);   // wave 3's tile 0 comes from wave 1
    // The panel tile, final, as write-through stores.  Wave 0 goes straight on to the next elimination and stores nothing:
    // its rows are wave 1's (from the exchange buffer: the same registers, lane for lane).
    if (W != 0) store_pt_sc1(P, Pg, ld, W, lane);
    if (W == 1) {
        d4 P0[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) P0[t][r] = Xc[((0 * 4 + t) * 4 + r) * 64 + lane];
        store_pt_sc1(P0, Pg, ld, 0, lane);
    }
    vlds_double *S = (vlds_double *)scratch + W * 256;   // element (i, j) at i * 16 + (j ^ i): both passes conflict-free
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t >= T0 && t <= W) {
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(lu + 4 * r) * 16 + (lm ^ (lu + 4 * r))] = nat[t][r];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double trv = S[lm * 16 + ((lu + 4 * r) ^ lm)];
                Dn.v[t][r] = (t == W && lu + 4 * r >= lm) ? nat[t][r] : trv;
            }
        } else {
            Dn.v[t] = (d4){0.0, 0.0, 0.0, 0.0};
        }
    }
    if (W != 0) {
        // The tile's version word as soon as the stores have drained: waves 1-3 count themselves in LDS when theirs have (the
        // wait costs them ~0.5 us they have -- wave 0 eliminates for 1.2 us after its single tile), the last one publishes.
        // (Round 4's first form published from the next factorisation's first barrier, 1 us later: the look-ahead task waits
        // for this word before it can update the tile the chain needs next.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0 && atomicAdd(pcount, 1) == ptarget)
            __hip_atomic_store(pflag, VER_FINAL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    double xa[3][4], xh[3];   // a ring of three k-steps (sched_barrier: the scheduler must not gather all the reads up front)
    auto rd = [&](int s_) {
        const int o = s_ % 3;
#pragma unroll
        for (int t = T0; t < W; ++t) xa[o][t] = Xc[(t * 16 + s_) * 64 + lane];
        if (W == 1) xh[o] = Xc[(3 * 16 + s_) * 64 + lane];
    };
    rd(0);
    rd(1);
#pragma unroll
    for (int s_ = 0; s_ < 16; ++s_) {   // k-step (c, r) = (s_ / 4, s_ % 4): columns 16 c + 4 r .. + 3 of the panel tile
        if (s_ + 2 < 16) rd(s_ + 2);
        __builtin_amdgcn_sched_barrier(0);
        const double pv = P[s_ >> 2][s_ & 3], bv = -pv;
#pragma unroll
        for (int t = T0; t <= W; ++t)
            Dn.v[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(t == W ? pv : xa[s_ % 3][t], bv, Dn.v[t], 0, 0, 0);
        if (W == 1)   // tile (0, 3): rows of block 0 against the rows of block 3, both from the exchange buffer
            H = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s_ % 3][0], -xh[s_ % 3], H, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (W == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) hand[r * 64 + lane] = H[r];
    }
}

__device__ __forceinline__ void mega_chain2(const MegaArgs &g, const int b, double *Qs, double *Ws, DiagShared &sh) {
    // (wave in a scalar register: the per-wave roles below are then scalar branches, not sixteen exec-masked blocks)
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane0 = tid & 63;
    const int64_t ld = g.ld;
    double *A = g.buf[BUF_A] + (int64_t)b * g.stride_a;
    int32_t *ver = g.ver + (int64_t)b * VER_PLANES * g.nbk * g.nbk;   // buffer A's versions first
    int32_t *wflag = &g.sync->wflag[b].v;
    long long *tr = (g.trace && b == 0 && tid == 0) ? g.trace : nullptr;
    long long *tl = (g.tlog && tid == 0) ? g.tlog + 64 + 8 * (int64_t)b * g.nbk : nullptr;   // (full log: every matrix)
    if (tl && b == 0) g.tlog[0] = wall_clock64();
    double *scratch = &sh.u[0][0][0];   // (wave-private 16 x 16 transposition areas; the factor writes sh.u only behind its first barrier)
    __builtin_amdgcn_s_setprio(3);
    if (tid == 0) __hip_atomic_store(&g.sync->cukey[b], cu_key(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tr) __hip_atomic_store(&g.trace[5999], wall_clock64(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    Tile64 D;
    load_cb_lower(D.v, A, ld, wave, lane0, scratch);
    DiagShadow shw;
    shw.hand = nullptr; shw.wout = nullptr;
    if (tid == 0) {
        sh.pcount = 0;   // (visible to the other waves behind the first factorisation's barriers)
        sh.look = 0;
    }
    double *pivots = g.piv + (int64_t)b * g.ld;   // every block's pivots: their logarithms are summed when the chain has ended
    int info = 0;
    vlds_double *hand = (vlds_double *)Ws;   // (Ws is idle between the solve and the next block's W_k)
    const vlds_double *Qp = (const vlds_double *)Qs, *Wp = (const vlds_double *)Ws;
    vlds_double *Xc = (vlds_double *)Qs;   // exchange of the P^T registers: Xc[((w * 4 + t) * 4 + r) * 64 + lane] (32 KB, over Qs)
    for (int k = 0; k < g.nbk; ++k) {
        // (opaque to the optimiser: the dozens of per-lane offsets below are loop invariants that would otherwise be hoisted
        //  out of the block loop and held in registers across the factorisation, where the pressure peaks -- spills)
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const int lm = lane & 15, lu = lane >> 4;
        if (tr) tr[16 * k + 0] = wall_clock64();
        if (tl) tl[8 * k + 0] = wall_clock64();
        const int64_t rem = g.n - (int64_t)k * 64;
        const int ncol = rem >= 64 ? 64 : (rem > 0 ? (int)rem : 0);
        double *Wk = g.ws + (int64_t)b * g.stride_ws + (int64_t)k * 4096;
        Tile64 winv;
        // (whether the workers' tiles for the next block have arrived is asked during the factorisation: DiagPoll)
        const int2 need = g.chain_need[k < g.nbk - 1 ? k : 0];
        DiagPoll poll;
        // A[k+1][k] (lane 0), A[k+1][k+1] (lane 1); no poll in the last block (a null word: the struct itself is always handed
        // over -- a select between its address and null kept it in scratch memory)
        poll.f = k + 1 < g.nbk ? ver + (k + 1) * g.nbk + k + (lane == 0 ? 0 : 1) : nullptr;
        poll.need = lane == 0 ? need.x : need.y;
        const int bad = diag_factor(D, winv, sh, ncol, (g.trace && b == 0) ? g.trace + 1024 + 16 * k : nullptr,
                                    &poll, &shw);
        const int ready = g.nowait ? 3 : sh.ready;
        if (tr) tr[16 * k + 1] = wall_clock64();
        if (tl) tl[8 * k + 1] = wall_clock64();
        if (bad && !info) info = k * 64 + bad;
        if (wave == 3) __hip_atomic_store(pivots + 64 * k + lane, sh.piv[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        shw.hand = nullptr;
        // (W_k row block by row block from inside the factorisation -- DiagShadow::wout -- published it 0.4 us earlier and cost
        //  the factorisation 0.8 us: measured, not used)
        diag_store_inverse<true>(winv, Wk);
        if (k + 1 == g.nbk) {
            diag_store_factor(D, A + ((int64_t)k * 64) * ld + (int64_t)k * 64, ld, ncol);
            wg_publish(wflag, k + 1, tid);   // (the last block's inverse: T tasks of the fused inverse)
            break;
        }
        // ---- the next block's inputs from the workers: A[k+1][k] and A[k+1][k+1] with the panels <= k-1 applied ----
        // (bit 0: the panel tile A[k+1][k] had arrived when the factorisation polled, bit 1: the diagonal tile A[k+1][k+1] --
        //  the second is needed one solve later and is waited for separately)
        // A tile that had not arrived at the factorisation's poll usually has by now (the look-ahead tasks publish the panel tile
        // ~10 us after W_k-1, the poll is 1.7 us before this point): ONE more look -- a write-through load of the word by one
        // lane, handed to the others through LDS -- and the step goes on as if the poll had seen it.  No acquire here: every
        // load of these tiles below bypasses L1 (sc1), every store of them was write-through and drained ahead of the word,
        // and this CU holds the chain alone (MI355X_MICROARCH.md, hand-offs with sc1 loads in place of the acquire, first row).
        // (The bits go into a word of their own.  Written into sh.ready they raced with the other waves' read of it above: nothing
        //  orders a slow wave's read before wave 0's update, the waves then disagreed about `ready != 3`, one side took a barrier
        //  the other did not, and from there on every LDS hand-over of the step was off by one barrier.  With the chain alone on
        //  its CU the four waves run in step and it never happened; with another process's waves on the same SIMDs -- two ranks
        //  sharing a GPU -- it gave wrong factors a few times per thousand launches.)
        int ready2 = ready;
        if (ready != 3) {
            if (tid < 2 && !((ready >> tid) & 1)) {
                const int got = __hip_atomic_load(ver + (k + 1) * g.nbk + k + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (got >= (tid == 0 ? need.x : need.y)) atomicOr(&sh.look, 1 << tid);
            }
            lds_barrier();
            ready2 = g.nowait ? 3 : (ready | sh.look);
        }
        bool published = false;
        if (!(ready2 & 1)) {
            wg_publish(wflag, k + 1, tid);   // (the panel tasks of this block must not wait for the chain's own inputs)
            published = true;
            wg_wait_flags<true>(tid == 0 ? ver + (k + 1) * g.nbk + k : nullptr, need.x, 100 + k, &g.sync->status, tid);
            if (__hip_atomic_load(&g.sync->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;   // (a lost hand-off ends the launch)
        }
        double *Pg = A + ((int64_t)(k + 1) * 64) * ld + (int64_t)k * 64;
        const double *Cn = A + ((int64_t)(k + 1) * 64) * ld + (int64_t)(k + 1) * 64;
        const HalfTile a0 = fetch_mk_sc1(Pg, ld, tid, 0), a1 = fetch_mk_sc1(Pg, ld, tid, 1);
        // while the panel tile is on its way: W_k into LDS, and the factor's own tile (nobody's input) to memory
        {
            double *Akk = A + ((int64_t)k * 64) * ld + (int64_t)k * 64;
            switch (wave) {
                case 0: chain_stage_w<0>(winv, Ws, lm, lu); diag_store_factor_rows<0>(D, Akk, ld, lane, scratch); break;
                case 1: chain_stage_w<1>(winv, Ws, lm, lu); diag_store_factor_rows<1>(D, Akk, ld, lane, scratch); break;
                case 2: chain_stage_w<2>(winv, Ws, lm, lu); diag_store_factor_rows<2>(D, Akk, ld, lane, scratch); break;
                default: chain_stage_w<3>(winv, Ws, lm, lu); diag_store_factor_rows<3>(D, Akk, ld, lane, scratch); break;
            }
        }
        // the panel tile has landed -- and with it, vmcnt counting in order, this wave's older W_k stores have drained
        if (tl) tl[8 * k + 7] = wall_clock64();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        {
            const int c2 = (tid & 15) * 2;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int r = (tid >> 4) + 16 * it;
                Qs[r * LDQ + c2] = a0.v[it].x; Qs[r * LDQ + c2 + 1] = a0.v[it].y;
                Qs[r * LDQ + 32 + c2] = a1.v[it].x; Qs[r * LDQ + 32 + c2 + 1] = a1.v[it].y;
            }
        }
        lds_barrier();
        if (tid == 0) sh.look = 0;   // (every wave has read it: the next block's second look starts from zero, three barriers from here)
        if (tid == 0 && !published) __hip_atomic_store(wflag, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the panel tasks of this block can run
        if (tr) tr[16 * k + 2] = tr[16 * k + 3] = wall_clock64();
        if (tl) { tl[8 * k + 2] = wall_clock64(); tl[8 * k + 6] = ready2; }
        if (!(ready2 & 2)) {
            wg_wait_flags<true>(tid == 0 ? ver + (k + 1) * g.nbk + k + 1 : nullptr, need.y, 200 + k, &g.sync->status, tid);
            if (__hip_atomic_load(&g.sync->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        }
        // the next diagonal tile: requested now, in flight during the solve
        d4 nat[4];
        d4 H = (d4){0.0, 0.0, 0.0, 0.0};
        switch (wave) {
            case 0: chain_request_next<0>(nat, H, Cn, ld, lm, lu); break;
            case 1: chain_request_next<1>(nat, H, Cn, ld, lm, lu); break;
            case 2: chain_request_next<2>(nat, H, Cn, ld, lm, lu); break;
            default: chain_request_next<3>(nat, H, Cn, ld, lm, lu); break;
        }
        if (tr) tr[16 * k + 6] = wall_clock64();
        if (tl) tl[8 * k + 3] = wall_clock64();
        // ---- P^T = W_k Q^T: tile t of wave w is P[16w.., 16t..]^T; W_k is LOWER triangular, so tile t sums the 16-blocks kb <= t ----
        d4 P[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) P[t] = (d4){0.0, 0.0, 0.0, 0.0};
        // (one wave per SIMD: an operand read waited for in front of its MFMA exposes the LDS latency, ~90 cycles per 64-cycle
        //  MFMA -- the fragments of k-step s + 2 are requested before the MFMAs of step s are issued)
        {
            double qv[3], wv[3][4];   // a ring of three k-steps (sched_barrier: the scheduler must not gather all the reads up front)
            auto rd = [&](int s) {
                const int k0 = 4 * s, kb = s >> 2, o = s % 3;
                qv[o] = Qp[(16 * wave + lm) * LDQ + k0 + lu];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t >= kb) wv[o][t] = Wp[(16 * t + lm) * LDQ + k0 + lu];
            };
            rd(0);
            rd(1);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                if (s + 2 < 16) rd(s + 2);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t >= (s >> 2)) P[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[s % 3][t], qv[s % 3], P[t], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (tr) tr[16 * k + 4] = wall_clock64();
        if (tl) tl[8 * k + 4] = wall_clock64();
        lds_barrier();   // (Qs / Ws are no longer read: the exchange buffer lies over Qs)
        if (tr) tr[16 * k + 7] = wall_clock64();
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) Xc[((wave * 4 + t) * 4 + r) * 64 + lane] = P[t][r];
        shw.hand = (const double *)Ws;
        lds_barrier();
        if (tr) tr[16 * k + 8] = wall_clock64();
        // ---- D = A[k+1][k+1] - P P^T in the column-block layout ----
        Tile64 Dn;
        switch (wave) {
            case 0: chain_update<0>(Dn, P, nat, H, Xc, scratch, hand, Pg, ld, lane, &sh.pcount, 3 * k + 2, ver + (k + 1) * g.nbk + k); break;
            case 1: chain_update<1>(Dn, P, nat, H, Xc, scratch, hand, Pg, ld, lane, &sh.pcount, 3 * k + 2, ver + (k + 1) * g.nbk + k); break;
            case 2: chain_update<2>(Dn, P, nat, H, Xc, scratch, hand, Pg, ld, lane, &sh.pcount, 3 * k + 2, ver + (k + 1) * g.nbk + k); break;
            default: chain_update<3>(Dn, P, nat, H, Xc, scratch, hand, Pg, ld, lane, &sh.pcount, 3 * k + 2, ver + (k + 1) * g.nbk + k); break;
        }
        D = Dn;
        if (tr) tr[16 * k + 5] = wall_clock64();
        if (tl) tl[8 * k + 5] = wall_clock64();
    }
    // The log-determinant: per 64-block the logarithms of its pivots summed over the lanes (the same tree, then the same
    // running sum over the blocks as diag_logdet: the same bits).  Kept out of the block steps -- the double-precision
    // logarithm costs the wave that evaluates it ~0.5 us and twenty registers of polynomial constants that the compiler
    // holds across the whole loop -- and done here for all blocks at once, the four waves taking every fourth block.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    vlds_double *vs = (vlds_double *)Qs;
    for (int kk = wave; kk < g.nbk; kk += 4) {
        const int64_t rem = g.n - (int64_t)kk * 64;
        const int ncol = rem >= 64 ? 64 : (rem > 0 ? (int)rem : 0);
        const double pv = __hip_atomic_load(pivots + 64 * kk + lane0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        double v = (lane0 < ncol && pv > 0.0) ? log(pv) : 0.0;   // (a failed pivot is reported through info)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane0 == 0) vs[kk] = v;
    }
    lds_barrier();
    if (tid == 0) {
        double logdet = 0.0;
        for (int kk = 0; kk < g.nbk; ++kk) logdet += vs[kk];
        __hip_atomic_store(g.logdet + b, logdet, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(g.info + b, info, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();   // (Qs becomes a worker's staging tile next)
}

// One ticket for a worker (called by thread 0 only): of the critical queue, of the bulk queue with bit 30 set, or -1 when both queues
// of the group are empty.  role 0 asks the critical queue first, role 1 the bulk queue.  No look at the heads before the atomic:
// the words are the hottest lines of the launch and a load of one costs as much as the atomic itself; a queue found empty once
// is not asked again (qempty).  Not inlined: six call sites, and its state must not live in the worker loop's registers.
__device__ __noinline__ int mega_pull(MegaSync *sync, int grp, int nbg, int nut, int ntask, int role, int32_t *qempty) {
    const int ucap = nut * nbg, bcap = (ntask - nut) * nbg;
    for (int attempt = 0; attempt < 2; ++attempt) {
        const int eu = qempty[0], eb = qempty[1];
        const int pick = (role == 0 ? !eu : eb) ? 0 : 1;   // 0: critical queue
        if (pick == 0 ? eu : eb) break;
        const int t = __hip_atomic_fetch_add(pick == 0 ? &sync->uhead[grp].v : &sync->ghead[grp].v, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t < (pick == 0 ? ucap : bcap)) return pick == 0 ? t : (t | (1 << 30));
        qempty[pick] = 1;
    }
    return -1;
}

__global__ __launch_bounds__(256, 2) void potrf_mega_kernel(MegaArgs g) {
    __shared__ double tiles[2 * 64 * LDM];   // As | Bs (workers); the chain's whole panel tile Q, then its register exchange
    __shared__ int32_t bc[4];
    double *As = tiles, *Bs = tiles + 64 * LDM;
    // the chain keeps W_k and the factor's LDS beside the panel tile (79.8 KB per workgroup: two workgroups per CU still fit 160 KB)
    __shared__ double wtile[64 * LDQ];
    __shared__ DiagShared dsh;
    static_assert(64 * LDQ <= 2 * 64 * LDM, "the chain's panel tile must fit the workers' staging tiles");
    static_assert(2 * (sizeof(double) * (2 * 64 * LDM + 64 * LDQ) + sizeof(DiagShared) + 16) <= 160 * 1024, "two workgroups per CU");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
    const int batch = g.batch;
    if (g.pred && *g.pred) return;   // (a speculative batch that an earlier one has made unnecessary: dgpamd_ess_queue)
    if ((int)blockIdx.x < batch) {
        mega_chain2(g, blockIdx.x, tiles, wtile, dsh);
    } else {
        // a worker beside a chain leaves (bounded wait for the chains' keys: they are dispatched first)
        if (tid < 64) {
            int key = 0, spins = 0;
            const bool mine = tid < batch;
            while (mine && (key = __hip_atomic_load(&g.sync->cukey[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 && ++spins < 2000)
                __builtin_amdgcn_s_sleep(4);
            const bool beside = __any(mine && key == cu_key());
            if (tid == 0) bc[0] = beside ? 1 : 0;
        }
        __syncthreads();
        if (bc[0]) return;
    }
    // ---- worker loop (the chains join it when their matrix is factored) ----
    const int64_t ld = g.ld;
    const int64_t rem_last = g.n - (int64_t)(g.nbk - 1) * 64;
    const int ncol_last = rem_last > 0 ? (int)rem_last : 0;
    // debug (dgpamd_debug_trace): the first 80 tasks of one worker, 5 stamps each, from trace[2048]: pulled, inputs ready,
    // computed, stored, published (+ the task's kind / panels in the sixth word)
    long long *wst = (g.trace && tid == 0 && (int)blockIdx.x == batch + 40) ? g.trace + 2048 : nullptr;
    int nst = 0;
    // this workgroup's group of matrices: those of its XCD's group first, then -- when that queue is empty -- the others'
    const int G = g.ngroups;
    const int home = (int)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 7u) % G;   // HW_REG_XCC_ID
    int grp = home, tried = 0;
    auto group_size = [&](int gi) { return (batch - gi + G - 1) / G; };
    // Two queues per group of matrices.  CRITICAL: per block step the look-ahead pair, the first solve of the panel column and the
    // catch-up updates behind it -- the lane that hands the chain its next inputs (six tasks per block step and matrix).  It is
    // served by workers of its own (`ncrit` per matrix, taken from the group's XCDs), which pull it in order and wait inside
    // their tasks.  With one queue these tasks sat behind what was left of the previous block step's bulk whenever the engine was
    // busy (tools/analyze_tasklog.py: "pulled late", 12 us per look-ahead task at ten matrices, and the chain's loop -- factor,
    // publish, look-ahead -- was 27 us per block step where the chain alone takes 12.6).  BULK: everything else, in the old order,
    // for all other workers; each kind of worker helps with the other queue once its own is empty.  Both queues are topological
    // orders of their own tasks and each has workers that take nothing else first, so the earliest unfinished task of the launch
    // is always held, or about to be pulled, by a worker that can run it.
    // The pull of the NEXT task is issued behind the stores of a task's tile and lands while they drain.
    const int widx = (int)blockIdx.x - batch;
    // (never more than a quarter of an XCD's ~64 workers: with 32-64 matrices `ncrit` per matrix would leave nobody who takes bulk work first,
    //  and critical workers that run ahead wait inside their tasks for bulk results nobody computes)
    const int crit_want = g.nut > 0 ? (g.ncrit * group_size(home) * G + 7) / 8 : 0;
    const int crit_per_xcd = crit_want > 16 ? 16 : crit_want;
    const int role = (widx >= 0 && (widx >> 3) < crit_per_xcd) ? 0 : 1;   // 0: critical queue first, 1: bulk queue first
    __shared__ int32_t qempty[2];   // (thread 0's notes: this group's critical / bulk queue has been found empty)
    if (tid == 0) { qempty[0] = g.nut > 0 ? 0 : 1; qempty[1] = 0; }
    auto pull_take = [&]() -> int { return mega_pull(g.sync, grp, group_size(grp), g.nut, g.ntask, role, qempty); };
    if (tid == 0) bc[1] = pull_take();
    for (;;) {
        __syncthreads();
        int q = __builtin_amdgcn_readfirstlane(bc[1]);
        __syncthreads();
        while (q < 0) {   // this group's queues are empty: on to the next group (all empty: done)
            if (++tried >= G) break;
            grp = grp + 1 == G ? 0 : grp + 1;
            if (tid == 0) {
                qempty[0] = g.nut > 0 ? 0 : 1;
                qempty[1] = 0;
                bc[1] = pull_take();
            }
            __syncthreads();
            q = __builtin_amdgcn_readfirstlane(bc[1]);
            __syncthreads();
        }
        if (tried >= G) break;
        const int nbg = group_size(grp);
        const int qt = q & ~(1 << 30), qs = qt / nbg;
        const int slot = (q >> 30) ? g.nut + qs : qs, b = grp + G * (qt - qs * nbg);
        const MTask mt = g.tasks[slot];
        long long *st = (wst && nst < 80) ? wst + 8 * nst++ : nullptr;
        // debug: every worker adds its waiting / arithmetic / remaining time to 100-us buckets of the launch (trace[6000..6095])
        const bool agg = g.trace != nullptr && tid == 0;
        long long a0 = 0, a1 = 0, a2 = 0;
        if (agg) a0 = wall_clock64();
        // debug (dgpamd_debug_tasklog): pulled, inputs seen, arithmetic done, W_k seen, stored, published, workgroup
        long long *tl = (g.tlog && tid == 0) ? g.tlog + 64 + 8 * ((int64_t)batch * g.nbk + (int64_t)b * g.ntask + slot) : nullptr;
        if (tl) { tl[0] = wall_clock64(); tl[6] = blockIdx.x; }
        if (st) { st[0] = wall_clock64(); st[5] = task_post(mt.a.x) | (task_hi(mt.a.w) << 8) | ((long long)slot << 16); }
        const int4 tk = mt.a;
        const int post = task_post(tk.x), first = task_first(tk.x), plus = task_plus(tk.x), mask_last = task_mask_last(tk.x);
        const int bufC = task_bufC(tk.x), bufL = task_bufL(tk.x), bufR = task_bufR(tk.x);
        const int ci = task_lo(tk.y), cj = task_hi(tk.y), li = task_lo(tk.z), ri = task_hi(tk.z);
        const int kb0 = task_lo(tk.w), nkb = task_hi(tk.w);
        const int need_c = mt.b.x, fin = mt.b.y & 1, wk = mt.b.z;
        const int64_t mo = (int64_t)b * g.stride_a;
        const int nb2 = g.nbk * g.nbk;
        int32_t *ver = g.ver + (int64_t)b * VER_PLANES * nb2;
        int32_t *vC = ver + bufC * nb2 + ci * g.nbk + cj;
        double *C = g.buf[bufC] + mo + ((int64_t)ci * 64) * ld + (int64_t)cj * 64;
        double *Wk = g.ws + (int64_t)b * g.stride_ws + (int64_t)wk * 4096;
        int32_t *wflag = &g.sync->wflag[b].v;
        const int newver = fin ? VER_FINAL : need_c + 1;
        int qn = 0;
        auto pull_next = [&]() {
            if (tid == 0) qn = pull_take();
        };
        auto finish = [&](int32_t *vflag, int vvalue) {   // drain (the tile's stores and the pull), publish, hand the next task to the loop's head
            wg_publish(vflag, vvalue, tid);
            if (tid == 0) bc[1] = qn;
            if (st) st[4] = wall_clock64();
            if (tl) tl[5] = wall_clock64();
            if (agg) {
                const long long a4 = wall_clock64(), t00 = g.trace[5999];
                long long bk = t00 > 0 ? (a0 - t00) / 10000 : 0;
                bk = bk < 0 ? 0 : (bk > 31 ? 31 : bk);
                if (a1 == 0) a1 = a2 = a0;   // (a task without separate phases: all of it counts as the rest)
                atomicAdd((unsigned long long *)g.trace + 6000 + bk, (unsigned long long)(a1 - a0));
                atomicAdd((unsigned long long *)g.trace + 6032 + bk, (unsigned long long)(a2 - a1));
                atomicAdd((unsigned long long *)g.trace + 6064 + bk, (unsigned long long)(a4 - a2));
                // ... and by kind of task: [buffer A / T / S][update, solve]: waiting, arithmetic, rest, count (trace[6100..6123])
                const int kd = 4 * (2 * bufC + (post == T_SOLVE ? 1 : 0));
                atomicAdd((unsigned long long *)g.trace + 6100 + kd, (unsigned long long)(a1 - a0));
                atomicAdd((unsigned long long *)g.trace + 6101 + kd, (unsigned long long)(a2 - a1));
                atomicAdd((unsigned long long *)g.trace + 6102 + kd, (unsigned long long)(a4 - a2));
                atomicAdd((unsigned long long *)g.trace + 6103 + kd, 100ull);
            }
        };

        if (post == T_TDIAG) {   // T[k][k] = W_k^T, rows of the carried right-hand sides zeroed
            wg_wait_flags<true>(tid == 0 ? wflag : nullptr, wk + 1, 2000 + wk, &g.sync->status, tid);
            if (tl) tl[1] = tl[2] = tl[3] = wall_clock64();
            const int nrow = (wk == g.nbk - 1) ? ncol_last : 64;
            for (int idx = tid; idx < 4096; idx += 256)
                tiles[(idx >> 6) * 65 + (idx & 63)] = __hip_atomic_load(Wk + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            pull_next();
            for (int idx = tid; idx < 4096; idx += 256) {
                const int r = idx >> 6, c = idx & 63;
                __hip_atomic_store(C + (int64_t)r * ld + c, r < nrow ? tiles[c * 65 + r] : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            finish(vC, newver);
            continue;
        }
        // ---- inputs: the output tile's earlier visits, the operand tiles final ----
        // The NEWEST panel of a visit is usually the one that arrives last -- its operand tile was solved one block step ago, and
        // along a row of tiles every solve waits for the previous column's (the recursion that bounds the whole launch when the
        // engine is not saturated: 13-20 us per column with all of a visit's panels applied behind the last arrival).  So the
        // newest panel's words are optional in the first wait: if they have not arrived, the older panels are applied first
        // and only the last panel's products follow the arrival (the same products in the same order: the same bits).
        int split = 0;
        {
            const int32_t *addr = nullptr;
            int nd = VER_FINAL;
            if (tid == 0) { addr = vC; nd = need_c; }
            else if (tid <= nkb) addr = ver + bufL * nb2 + li * g.nbk + kb0 + tid - 1;
            else if (tid <= 2 * nkb) addr = ver + bufR * nb2 + ri * g.nbk + kb0 + tid - 1 - nkb;
            if (nkb >= 2 && g.split)
                split = !wg_wait_flags_opt(addr, nd, tid == nkb || tid == 2 * nkb, 1000 + slot % 1000, &g.sync->status, tid, &bc[2]);
            else
                wg_wait_flags<true>(addr, nd, 1000 + slot % 1000, &g.sync->status, tid);
        }
        if (st) st[1] = wall_clock64();
        if (agg) a1 = wall_clock64();
        if (tl) tl[1] = wall_clock64();
        Tile64 acc;
        const double *Lp0 = g.buf[bufL] + mo + ((int64_t)li * 64) * ld + (int64_t)kb0 * 64;
        const double *Rp0 = g.buf[bufR] + mo + ((int64_t)ri * 64) * ld + (int64_t)kb0 * 64;
        tile_update<true, true>(acc.v, first ? nullptr : C, Lp0, Rp0, ld, split ? nkb - 1 : nkb, plus ? 1.0 : -1.0,
                          mask_last ? g.nbk - 1 - kb0 : -1, ncol_last, As, Bs, tid, wave, lane);
        if (split) {
            const int kl = kb0 + nkb - 1;
            const int32_t *addr = tid == 0 ? ver + bufL * nb2 + li * g.nbk + kl : (tid == 1 ? ver + bufR * nb2 + ri * g.nbk + kl : nullptr);
            wg_wait_flags<true>(addr, VER_FINAL, 6000 + slot % 1000, &g.sync->status, tid);
            if (tl) tl[7] = wall_clock64();
            tile_update<true, true, true>(acc.v, nullptr, Lp0 + (int64_t)(nkb - 1) * 64, Rp0 + (int64_t)(nkb - 1) * 64, ld, 1, plus ? 1.0 : -1.0,
                                          mask_last ? g.nbk - 1 - kl : -1, ncol_last, As, Bs, tid, wave, lane);
        }
        if (st) st[2] = wall_clock64();
        if (agg) a2 = wall_clock64();
        if (tl) tl[2] = wall_clock64();
        if (post == T_STORE) {
            store_acc_sc1(acc.v, C, ld, crow, ccol);
            pull_next();   // (behind the stores: the ticket's round trip delayed wave 0's stores, and with them the publication, by 1-2 us)
            if (st) st[3] = wall_clock64();
            if (tl) tl[4] = wall_clock64();
            finish(vC, newver);
            continue;
        }
        // T_SOLVE / T_LOOK / T_LOOKD: wait for W_k, then tile <- tile * W_k^T
        // debug: the look-ahead tasks of every block of matrix 0 stamp their phases into trace[7000 + 8 k ..]
        long long *lk = ((post == T_LOOK || post == T_LOOKD) && g.trace && b == 0 && tid == 0 && wk < 120) ? g.trace + 7000 + 8 * wk : nullptr;
        if (lk && post == T_LOOK) { lk[0] = a0; lk[1] = wall_clock64(); }
        int32_t *vX = ver + 3 * nb2 + ci * g.nbk + cj;   // auxiliary word of the tile: T_LOOK has read it (T_LOOKD may overwrite it)
        if (post == T_LOOK) {   // (acc holds everything this task reads of the tile)
            __syncthreads();
            if (tid == 0) __hip_atomic_store(vX, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        wg_wait_flags<true>(tid == 0 ? wflag : nullptr, wk + 1, 3000 + wk, &g.sync->status, tid);
        if (lk && post == T_LOOK) lk[2] = wall_clock64();
        if (tl) tl[3] = wall_clock64();
        d4 out[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) out[t] = (d4){0.0, 0.0, 0.0, 0.0};
        mul_acc_bt<true>(out, acc.v, Wk, 64, As, Bs, tid, wave, lane);
        if (post == T_SOLVE) {
            store_acc_sc1(out, C, ld, crow, ccol);
            pull_next();
            if (st) st[3] = wall_clock64();
            if (tl) tl[4] = wall_clock64();
            finish(vC, newver);
            continue;
        }
        // ---- T_LOOK / T_LOOKD: the chain's look-ahead.  S = A[k+2][k] is final now and stays in registers; panel k is applied
        // with it to one of the two tiles the chain picks up after its next factorisation: T_LOOK  Q = A[k+2][k+1] -= S P^T
        // (P = A[k+1][k], the chain's own panel tile; this task also stores S), T_LOOKD  D = A[k+2][k+2] -= S S^T.  As three
        // tasks (solve, two updates) the chain's inputs were two worker hand-offs behind W_k (store, drain, publish, poll,
        // acquire, reload of S: ~15 us against a 15-us block step); the same products in the same order, so the same bits.
        {
            int32_t *vA = ver + BUF_A * nb2;
            double *Ab = g.buf[BUF_A] + mo;
            const int need2 = mt.b.w;   // earlier visits of the tile this task updates
            if (post == T_LOOK) {
                int32_t *vQ = vA + ci * g.nbk + cj + 1;
                // lanes 0 / 1: the chain's panel tile A[k+1][k] final; the earlier visits of Q (the catch-up tasks of the block
                // before: two hand-offs behind W_k-1, so NOT waited for ahead of the solve)
                const int32_t *addr = tid == 0 ? vA + (ci - 1) * g.nbk + cj : (tid == 1 ? vQ : nullptr);
                const int nd = tid == 0 ? VER_FINAL : need2;
                if (lk) lk[3] = wall_clock64();
                wg_wait_flags<true>(addr, nd, 4000 + wk, &g.sync->status, tid);
                if (lk) lk[4] = wall_clock64();
                if (tl) tl[7] = wall_clock64();
                const double *Pg = Ab + ((int64_t)(ci - 1) * 64) * ld + (int64_t)cj * 64;
                double *Qg = Ab + ((int64_t)ci * 64) * ld + (int64_t)(cj + 1) * 64;
                const HalfTile p0 = fetch_mk_sc1(Pg, ld, tid, 0), p1 = fetch_mk_sc1(Pg, ld, tid, 1);
                Tile64 qt;
                load_acc_sc1(qt.v, Qg, ld, crow, ccol);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    __syncthreads();
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) As[(crow + 4 * r) * LDM + 16 * t + ccol] = out[2 * h + t][r];
                    commit_mk(h == 0 ? p0 : p1, Bs, tid);
                    __syncthreads();
                    mfma_tile_ahead<OP_MK, OP_MK, true>(As, Bs, qt.v, wave, lane, -1.0);
                }
                store_acc_sc1(qt.v, Qg, ld, crow, ccol);
                pull_next();
                if (st) st[3] = wall_clock64();
                if (tl) tl[4] = wall_clock64();
                finish(vQ, need2 + 1);
                if (lk) lk[5] = wall_clock64();
            } else {
                int32_t *vD = vA + ci * g.nbk + ci;
                // lane 0: the earlier visits of D; lane 1: T_LOOK has read the tile that S replaces
                wg_wait_flags<true>(tid == 0 ? vD : (tid == 1 ? vX : nullptr), tid == 0 ? need2 : 1, 5000 + wk, &g.sync->status, tid);
                if (tl) tl[7] = wall_clock64();
                store_acc_sc1(out, C, ld, crow, ccol);   // the solved tile, final
                double *Dg = Ab + ((int64_t)ci * 64) * ld + (int64_t)ci * 64;
                Tile64 d;
                load_acc_sc1(d.v, Dg, ld, crow, ccol);
                // ... published as soon as it has drained (the wait covers D's loads as well): the next block's catch-up tasks need it
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) __hip_atomic_store(vC, newver, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lk) lk[7] = wall_clock64();
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    __syncthreads();
#pragma unroll
                    for (int t = 0; t < 2; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) As[(crow + 4 * r) * LDM + 16 * t + ccol] = out[2 * h + t][r];
                    __syncthreads();
                    mfma_tile_ahead<OP_MK, OP_MK, true>(As, As, d.v, wave, lane, -1.0);
                }
                store_acc_sc1(d.v, Dg, ld, crow, ccol);
                pull_next();
                if (st) st[3] = wall_clock64();
                if (tl) tl[4] = wall_clock64();
                finish(vD, need2 + 1);
                if (lk) lk[6] = wall_clock64();
            }
        }
    }
}


// ---- host: table, plan, launch ---------------------------------------------------------------------------------------------
struct MegaTable {
    MTask *dev = nullptr;        // urgent tasks first (nut of them), then the bulk tasks
    int2 *need_dev = nullptr;
    int ntask = 0, nut = 0;
};

static int mega_wgs_per_cu() {
    static int n = 0;
    if (!n) {
        int q = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, potrf_mega_kernel, 256, 0) != hipSuccess || q < 1) q = 2;
        n = q > 4 ? 4 : q;
    }
    return n;
}

// the plan's table on the device, flattened and uploaded on first use
static int get_mega_tasks(dgpamd_ctx *ctx, const MegaPlan &p, MegaTable *&out) {
    static std::map<std::pair<dgpamd_ctx *, MegaKey>, MegaTable> cache;   // contexts are few and long-lived
    MegaTable &mt = cache[{ctx, p.key}];
    if (!mt.dev) {
        const MegaFlat f = mega_flatten(p);
        if (f.refused) BAD_ARG(ctx, "task table: a visit applies more panels than one wave can wait for");
        mt.nut = f.nut;
        mt.ntask = f.ntask;
        HIP_TRY(ctx, hipMalloc((void **)&mt.dev, (f.tasks.size() + 1) * sizeof(MTask)));
        HIP_TRY(ctx, hipMemcpy(mt.dev, f.tasks.data(), f.tasks.size() * sizeof(MTask), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMalloc((void **)&mt.need_dev, f.need.size() * sizeof(int2)));
        HIP_TRY(ctx, hipMemcpy(mt.need_dev, f.need.data(), f.need.size() * sizeof(int2), hipMemcpyHostToDevice));
    }
    out = &mt;
    return DGPAMD_OK;
}

extern "C" int dgpamd_debug_mega_table(dgpamd_ctx *ctx, int64_t n, int inv, int batch, int32_t *host_out, int64_t cap_words) {
    if (!ctx || !host_out || n <= 0 || batch <= 0) return -DGPAMD_BAD_ARG;
    const int nbk = (int)(padded_dim(n) / 64);
    MegaTable *mt = nullptr;
    if (get_mega_tasks(ctx, mega_plan(ctx->tune, nbk, inv != 0, batch, ctx->num_cu, mega_wgs_per_cu()), mt)) return -DGPAMD_BAD_ARG;
    if ((int64_t)mt->ntask * 8 + 2 * nbk > cap_words) return -DGPAMD_BAD_ARG;
    if (hipMemcpy(host_out, mt->dev, (size_t)mt->ntask * sizeof(MTask), hipMemcpyDeviceToHost) != hipSuccess) return -DGPAMD_HIP_ERROR;
    if (hipMemcpy(host_out + (int64_t)mt->ntask * 8, mt->need_dev, (size_t)nbk * sizeof(int2), hipMemcpyDeviceToHost) != hipSuccess) return -DGPAMD_HIP_ERROR;
    return mt->ntask;
}

int potrf_mega_launch(dgpamd_ctx *ctx, int64_t n, double *A, double *T, double *S, int64_t stride_a, int batch, double *logdet,
                      int32_t *info, double *ws, bool sync_cleared) {
    const int64_t Np = padded_dim(n);
    const int nbk = (int)(Np / 64);
    MegaPlan p = mega_plan(ctx->tune, nbk, T != nullptr, batch, ctx->num_cu, mega_wgs_per_cu());
    MegaTable *mt = nullptr;
    int rc = get_mega_tasks(ctx, p, mt);   // (uploads the table on first use)
    if (rc) return rc;
    p.set_grid(mt->ntask);
    void *syncmem = reinterpret_cast<char *>(ws) + mega_sync_offset(n, batch);
    if (!sync_cleared) HIP_TRY(ctx, hipMemsetAsync(syncmem, 0, mega_sync_bytes(nbk, batch), ctx->stream));
    MegaArgs g;
    g.buf[BUF_A] = A; g.buf[BUF_T] = T; g.buf[BUF_S] = S;
    g.ws = ws; g.ld = Np; g.stride_a = stride_a; g.stride_ws = (int64_t)nbk * 4096; g.n = n; g.nbk = nbk; g.batch = batch;
    g.inv = T != nullptr;
    g.tasks = mt->dev; g.ntask = mt->ntask; g.chain_need = mt->need_dev;
    g.nut = mt->nut;
    g.ncrit = p.ncrit;
    g.sync = reinterpret_cast<MegaSync *>(syncmem);
    g.ver = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(syncmem) + sizeof(MegaSync));
    g.logdet = logdet; g.info = info; g.trace = ctx->trace; g.pred = ctx->pred;
    g.piv = reinterpret_cast<double *>(reinterpret_cast<char *>(ws) + mega_piv_offset(n, batch));
    g.tlog = (ctx->tlog && 64 + 8 * ((int64_t)batch * nbk + (int64_t)batch * mt->ntask) <= ctx->tlog_words) ? ctx->tlog : nullptr;
    g.nowait = 0;
    g.split = (int)ctx->tune.mega_split;
    g.ngroups = p.ngroups;
    // algorithmic flops of the launch: n^3/3 per matrix, n^3 with the fused inverse
    PROF_BEGIN(ctx, PROF_SYRK, (double)batch * (double)n * (double)n * (double)n * (T ? 1.0 : 1.0 / 3.0));
    hipLaunchKernelGGL(potrf_mega_kernel, dim3((unsigned)p.grid), dim3(256), 0, ctx->stream, g);
    PROF_END(ctx, PROF_SYRK);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
