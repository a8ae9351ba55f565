// Device helpers shared by the two factorisation kernels (potrf_step.hpp, potrf_mega.hpp): accumulator tiles to and from
// memory, the tile update, the chain's diagonal tile, the product with a block inverse, and the waits / publications of the
// hand-offs between workgroups.  The task encoding the kernels decode is potrf_plan.hpp's.
#pragma once
#include "common.hpp"
#include "tile.hpp"
#include "diagfac.hpp"
#include "potrf_plan.hpp"

__device__ __forceinline__ void load_acc(d4 (&acc)[4], const double *C, int64_t ld, int crow, int ccol) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] = C[(int64_t)(crow + 4 * r) * ld + 16 * t + ccol];
}
__device__ __forceinline__ void load_acc_sc1(d4 (&acc)[4], const double *C, int64_t ld, int crow, int ccol) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            acc[t][r] = __hip_atomic_load(C + (int64_t)(crow + 4 * r) * ld + 16 * t + ccol, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_acc(const d4 (&acc)[4], double *C, int64_t ld, int crow, int ccol) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) C[(int64_t)(crow + 4 * r) * ld + 16 * t + ccol] = acc[t][r];
}
// acc = (C ? C : 0) + sign * sum over nkb consecutive 64-blocks  L_kb R_kb^T.  Software pipelined: the global loads of
// the next half tile are in flight (registers) while the MFMAs of the current one run.  The products of each half tile are
// summed from zero and added to acc once (tile.hpp, FROM_ZERO; the look-ahead tasks of the one-launch kernel do the same, so
// the two modes stay equal bit for bit).  In the 64-block number
// mask_kb (relative to the first) the columns >= klim of both operands read as zero.
// SC1: every global load bypasses L1 (operands handed over inside a launch: the one-launch kernel).
// KEEP: acc is carried over from an earlier call (the panels of a visit applied in two runs, see the one-launch kernel's workers).
template <bool SC1 = false, bool AHEAD = false, bool KEEP = false>
__device__ __forceinline__ void tile_update(d4 (&acc)[4], const double *C, const double *Lp, const double *Rp, int64_t ld,
                                            int nkb, double sign, int mask_kb, int klim, double *As, double *Bs, int tid,
                                            int wave, int lane) {
    const int c2 = (tid & 15) * 2, r0 = tid >> 4;
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
    double2 pa[4], pb[4];
    const int nh = 2 * nkb;
    const __amdgpu_buffer_rsrc_t rsL = __builtin_amdgcn_make_buffer_rsrc((void *)Lp, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc((void *)Rp, 0, 0x7fffffff, 0x00020000);
    auto fetch = [&](int hh) {
        const int64_t off = 32 * hh;   // consecutive half tiles are consecutive 32-column slabs
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            if (SC1) {
                const int bo = (int)(((int64_t)(r0 + 16 * it) * ld + off + c2) * 8);
                const u32x4 va = __builtin_amdgcn_raw_buffer_load_b128(rsL, bo, 0, 16);
                const u32x4 vb = __builtin_amdgcn_raw_buffer_load_b128(rsR, bo, 0, 16);
                pa[it] = make_double2(__hiloint2double(va.y, va.x), __hiloint2double(va.w, va.z));
                pb[it] = make_double2(__hiloint2double(vb.y, vb.x), __hiloint2double(vb.w, vb.z));
            } else {
                pa[it] = *reinterpret_cast<const double2 *>(Lp + (int64_t)(r0 + 16 * it) * ld + off + c2);
                pb[it] = *reinterpret_cast<const double2 *>(Rp + (int64_t)(r0 + 16 * it) * ld + off + c2);
            }
        }
    };
    if (nh > 0) fetch(0);
    if (KEEP) {
    } else if (C) {
        if (SC1) load_acc_sc1(acc, C, ld, crow, ccol);
        else load_acc(acc, C, ld, crow, ccol);
    } else {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
    }
    for (int hh = 0; hh < nh; ++hh) {
        __syncthreads();
        if ((hh >> 1) == mask_kb) {
            const int c = 32 * (hh & 1) + c2;
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                if (c >= klim) pa[it].x = pb[it].x = 0.0;
                if (c + 1 >= klim) pa[it].y = pb[it].y = 0.0;
            }
        }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int r = r0 + 16 * it;
            As[r * LDM + c2] = pa[it].x; As[r * LDM + c2 + 1] = pa[it].y;
            Bs[r * LDM + c2] = pb[it].x; Bs[r * LDM + c2 + 1] = pb[it].y;
        }
        if (hh + 1 < nh) fetch(hh + 1);
        __syncthreads();
        // (AHEAD: the one-launch kernel's workers, two waves per SIMD -- the operand fragments requested two k-steps ahead gave
        //  the fused inverse 1-2.5 % at 6-12 matrices; the per-step kernel's four waves per SIMD hide the LDS latency themselves)
        if (AHEAD) mfma_tile_ahead<OP_MK, OP_MK, true>(As, Bs, acc, wave, lane, sign);
        else mfma_tile<OP_MK, OP_MK, true>(As, Bs, acc, wave, lane, sign);
    }
}
// The pivot chain's diagonal tile in the COLUMN-BLOCK layout of diagfac.hpp (wave w: acc[t][r] = S[16t + lu + 4r][16w + lm]),
// read from the LOWER triangle of the stored tile (the last block's upper part does not mirror the carried rows): the
// 16x16 tiles (w, t), t <= w, are loaded row-contiguously (four full 128-byte lines per load instruction; the transposed
// access touches sixteen) and transposed inside the wave through `scratch` (16 x 16 doubles of LDS per wave).
template <bool SC1 = false>
__device__ __forceinline__ void load_cb_lower(d4 (&acc)[4], const double *C, int64_t ld, int wave, int lane, double *scratch) {
    const int lm = lane & 15, lu = lane >> 4;
    d4 nat[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double *p = C + (int64_t)(16 * wave + lu + 4 * r) * ld + 16 * t + lm;
            nat[t][r] = (t <= wave) ? (SC1 ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p) : 0.0;
        }
    vlds_double *S = (vlds_double *)scratch + wave * 256;   // element (i, j) at i * 16 + (j ^ i): both passes conflict-free
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (t <= wave) {
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(lu + 4 * r) * 16 + (lm ^ (lu + 4 * r))] = nat[t][r];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double tr = S[lm * 16 + ((lu + 4 * r) ^ lm)];
                acc[t][r] = (t == wave && lu + 4 * r >= lm) ? nat[t][r] : tr;
            }
        } else {
            acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
        }
    }
}
// ... and its update acc = C - P P^T with ONE panel tile P = A[k][k-1] that serves as both operands.  It sits on the
// critical path of every block step and its loads are first touches (the tile was written by another CU in the previous
// launch), so C and BOTH halves of P are requested at once -- one exposed memory latency instead of two.
__device__ __forceinline__ void diag_update_cb(d4 (&acc)[4], const double *C, const double *P, int64_t ld, double *As, double *Bs,
                                               int tid, int wave, int lane) {
    const HalfTile p0 = fetch_mk(P, ld, tid, 0), p1 = fetch_mk(P, ld, tid, 1);
    load_cb_lower(acc, C, ld, wave, lane, Bs);
    const vlds_double *Ap = (const vlds_double *)As;
    const int m = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
        commit_mk(h == 0 ? p0 : p1, As, tid);
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < KC; k0 += 4) {
            const double bv = -Ap[(16 * wave + m) * LDM + k0 + kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double av = Ap[(16 * t + m) * LDM + k0 + kk];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
            }
        }
    }
}
// out += in * Bg^T   (in: accumulator-layout 64x64 tile, Bg: 64x64 row-major LOWER-TRIANGULAR tile in global memory: the
// inverse W_k of a diagonal block's factor).  Both halves of Bg are requested up front: one exposed load latency instead
// of two on the panel's critical path.  Column tile t of the product takes the 16-blocks kb <= t of the sum only (40
// instead of 64 MFMAs per wave: the blocks above W_k's diagonal are exact zeros, and the f64 MFMA runs at the vector
// rate on gfx950, so the skipped zeros are time).
template <bool SC1 = false>
__device__ __forceinline__ void mul_acc_bt(d4 (&out)[4], const d4 (&in)[4], const double *Bg, int64_t ldb,
                                           double *As, double *Bs, int tid, int wave, int lane) {
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
    const HalfTile b0 = SC1 ? fetch_mk_sc1(Bg, ldb, tid, 0) : fetch_mk(Bg, ldb, tid, 0);
    const HalfTile b1 = SC1 ? fetch_mk_sc1(Bg, ldb, tid, 1) : fetch_mk(Bg, ldb, tid, 1);
    const vlds_double *Ap = (const vlds_double *)As, *Bp = (const vlds_double *)Bs;
    const int m = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) As[(crow + 4 * r) * LDM + 16 * t + ccol] = in[2 * h + t][r];
        commit_mk(h == 0 ? b0 : b1, Bs, tid);
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < KC; k0 += 4) {
            const int kb = 2 * h + (k0 >> 4);
            const double av = Ap[(16 * wave + m) * LDM + k0 + kk];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t >= kb) out[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bp[(16 * t + m) * LDM + k0 + kk], out[t], 0, 0, 0);
        }
    }
}
__device__ __forceinline__ void wg_release_store(int32_t *flag, int value, int tid) {
    // every storing wave drains its stores, one agent-scope release, then the flag
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__device__ __forceinline__ void wg_wait_acquire(int32_t *flag, int target, int32_t *info, int tid) {
    if (tid == 0) {
        int spins = 0;
        while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(4);
            if (++spins > (1 << 24)) {
                *info = -1;
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
}

// The CU this workgroup runs on: XCC_ID[2:0] and HW_ID[15:8] (SE / SH / CU ids) -- measured on MI355X
// (tools/ubench/hwid.hip): 256 distinct keys, and workgroups i and i + 256 of a launch share one.
__device__ __forceinline__ int cu_key() {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_REG_HW_ID
    const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
    return (int)(((xcc & 7u) << 8) | ((hw >> 8) & 0xffu)) + 1;
}

// ---- hand-offs by version words (the one-launch kernel) ---------------------------------------------------------------------
#define MEGA_SPIN_LIMIT (1 << 20)   // polls of ~1 us: a lost hand-off gives up after about a second

// Write-through (sc1) store of an accumulator tile, 16 bytes per lane: neighbouring lanes hold neighbouring columns of the
// same rows, so each pair swaps one value (DPP quad_perm [1,0,3,2]) -- the even lane ends up with two columns of row r0, the odd
// lane with two columns of row r1 -- and every store instruction still writes whole 128-byte lines (8-byte sc1 stores cost
// 2.7x the time per byte: MI355X_MICROARCH.md, stores of each flavour).
__device__ __forceinline__ double swap_pair(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0xB1, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0xB1, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ void store_acc_sc1(const d4 (&acc)[4], double *C, int64_t ld, int crow, int ccol) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void *)C, 0, 0x7fffffff, 0x00020000);
    const bool odd = ccol & 1;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int rp = 0; rp < 2; ++rp) {
            const double a0 = acc[t][2 * rp], a1 = acc[t][2 * rp + 1];
            const double got = swap_pair(odd ? a0 : a1);
            const double lo = odd ? got : a0, hi = odd ? a1 : got;
            const int row = crow + 4 * (2 * rp + (odd ? 1 : 0)), col = 16 * t + (ccol & ~1);
            u32x4 v;
            v.x = __double2loint(lo); v.y = __double2hiint(lo); v.z = __double2loint(hi); v.w = __double2hiint(hi);
            __builtin_amdgcn_raw_buffer_store_b128(v, rs, (int)(((int64_t)row * ld + col) * 8), 0, 16);
        }
    // (eight 16-byte stores in a row: their data registers stay untouched for 16 wait states, as behind the chain's panel-tile stores --
    //  tests/test_isa_hazards.py; the callers used to drain right behind them, now the next ticket is pulled first)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15");
    __builtin_amdgcn_sched_barrier(0);
}
// every storing wave drains its stores, then one lane publishes
__device__ __forceinline__ void wg_publish(int32_t *flag, int value, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Wave 0: lane l < nflag polls flag[l] until it reaches need[l] (relaxed, bounded), then ONE agent-scope acquire;
// the workgroup's barrier follows.  Returns (to every thread, through LDS word `bc`) 0 or the give-up code.
// ACQ false would rely on sc1 loads alone (L1 bypassed, no acquire); it is measured valid only for one workgroup per CU
// (MI355X_MICROARCH.md, valid forms) and saves ~1 us per task here -- not used: the acquire stays.
template <bool ACQ>
__device__ __forceinline__ void wg_wait_flags(const int32_t *addr, int need, int code, int32_t *status, int tid) {
    if (tid < 64) {
        bool ok = (addr == nullptr);
        int spins = 0;
        for (;;) {
            if (!ok) ok = __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
            if (__all(ok)) break;
            __builtin_amdgcn_s_sleep(2);
            ++spins;
            // give up after the limit -- or at once when another workgroup already has (its inputs may never come)
            if (spins > MEGA_SPIN_LIMIT || ((spins & 255) == 0 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                if (tid == 0) atomicCAS(status, 0, code);
                break;
            }
        }
        if (ACQ) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    __syncthreads();
}

// The same wait with OPTIONAL words (lanes with opt set): the wait ends when every other lane's word has reached its value; the
// return value (the same in every thread, through LDS word `bcw`) says whether the optional ones had as well at that moment.
__device__ __forceinline__ int wg_wait_flags_opt(const int32_t *addr, int need, bool opt, int code, int32_t *status, int tid, int32_t *bcw) {
    if (tid < 64) {
        bool ok = (addr == nullptr);
        int spins = 0;
        for (;;) {
            if (!ok) ok = __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
            if (__all(ok || opt)) break;
            __builtin_amdgcn_s_sleep(2);
            ++spins;
            if (spins > MEGA_SPIN_LIMIT || ((spins & 255) == 0 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                if (tid == 0) atomicCAS(status, 0, code);
                break;
            }
        }
        const bool all_ok = __all(ok);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) *bcw = all_ok ? 1 : 0;
    }
    __syncthreads();
    return *bcw;
}
