// What the files of the linked-GP predictor share (linkgp.hip, linkgp_direct.hip, linkgp_sexp.hip, linkgp_matern.hip): its
// constants, the LDS layout of every pair kernel -- written once, read by the kernel for its pointers and by linkgp_plan.hpp
// for the launch's bytes -- the argument block, and the steps every pair kernel begins and ends with.  The device steps are
// forced inline: a kernel that uses one compiles to what it did with a copy of its own.
// The constants and the layouts are plain C++: a host program (tools/linkgp_plan_check.cpp) includes this file without HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include "common.hpp"
#include "tile.hpp"
#include "wave.hpp"
#define LINKGP_HD __host__ __device__
static_assert(LDK == 80 && EXPN_TAB == 256 && LDS_CU_BYTES == 160 * 1024, "restated below for host programs");
#else
#include "../../include/dgp_amd.h"
#define LINKGP_HD
#define LDK 80                      // tile.hpp
#define EXPN_TAB 256                // common.hpp
#define LDS_CU_BYTES (160 * 1024)   // common.hpp
#endif

#define MC_MAX 2048   // test points per workspace chunk
#define TCH 32        // test points per linked-GP workgroup
#define TCHS 32    // test points per workgroup of linkgp_Jsep_kernel
#define TCH2 128   // test points per workgroup of the second SExp form (256 where that still leaves >= 32 rounds of workgroups: sexp_tch2): the tile's weights and base exponents (a 32-KB tile of
                   // R^-1 read, 16 x Dw LDS reads per lane) are set up once per TCH2 test points -- at 32 that was 40 % of the run time
#define SX_KS 4   // k-steps held in registers: Dw + 2 <= 16
#define REC 30   // S[0..11] T[12..26] f2[27] x[28] 0[29]: the record as the pair kernel holds it in LDS (stride 30 doubles -> conflict-free
                 // column reads; the zero pads the 3-term erf-difference products to an MFMA k-step of 4)
#define PST REC
#define MC_SEP 256
#define JSEP_LOG_STEPS 48
#define JSEP_LOG_WORDS (8 + JSEP_LOG_STEPS * 4 * 2)

// ---- LDS layouts ----------------------------------------------------------------------------------------------------------
// One struct per pair kernel: offsets in doubles from the start of the kernel's dynamic LDS.  The kernel takes its pointers from
// the members, the plan takes bytes(), what a launch asks for.
// linkgp_J_kernel<KIND, LOO, TC>
struct JDirectLds {
    int WiT, WjT;        // [DT][64] each
    int tm, tv, tz;      // [tc][Dw], [tc][Dw], [tc][Dz]
    int red;             // [tc][4]
    int Cs;              // [64][65]  (matern only)
    int ui, uj;          // LOO only: [tc][64] u rows / columns of the tile
    int ryi, ryj;        // [64] each
    int ct, gt;          // [tc] c and wt scale / rho
    int end;
    LINKGP_HD JDirectLds(int kind, int Dw, int Dz, int tc, bool loo) {
        const int DT = Dw + Dz;
        WiT = 0;
        WjT = WiT + DT * 64;
        tm = WjT + DT * 64;
        tv = tm + tc * Dw;
        tz = tv + tc * Dw;
        red = tz + tc * Dz;
        Cs = red + tc * 4;
        ui = Cs + (kind == DGPAMD_MATERN25 ? 64 * 65 : 0);
        uj = ui + tc * 64;
        ryi = uj + tc * 64;
        ryj = ryi + 64;
        ct = ryj + 64;
        gt = ct + tc;
        end = loo ? gt + tc : ui;
    }
    LINKGP_HD size_t bytes() const { return (size_t)end * sizeof(double); }
};

// linkgp_Jsexp_kernel (TCH test points per workgroup)
struct JSexpLds {
    int KP, LDU;         // k padded to the MFMA's 4; row stride = 2 (mod 4) doubles: conflict-free ds_read_b64 A fragments
    int WiT, WjT;        // [DT][64] each
    int WjB;             // [KP][LDK]   B operand: w_jk, k-major, zero padded
    int tm, tv, tz;      // [TCH][Dw], [TCH][Dw], [TCH][Dz]
    int red;             // [TCH][4]
    int U;               // [2][64][LDU]  A operand of a test point: 2 c1_k (w_ik - 2 m_k)
    int R, S;            // [2][64] row terms, [2][64] column terms
    int ilg;             // [Dz] reciprocal lengthscales of the global dimensions
    int end;
    LINKGP_HD JSexpLds(int Dw, int Dz) {
        const int DT = Dw + Dz;
        KP = (Dw + 3) & ~3;
        LDU = KP + 2;
        WiT = 0;
        WjT = WiT + DT * 64;
        WjB = WjT + DT * 64;
        tm = WjB + KP * LDK;
        tv = tm + TCH * Dw;
        tz = tv + TCH * Dw;
        red = tz + TCH * Dz;
        U = red + TCH * 4;
        R = U + 2 * 64 * LDU;
        S = R + 2 * 64;
        ilg = S + 2 * 64;
        end = ilg + Dz;
    }
    LINKGP_HD size_t bytes() const { return (size_t)end * sizeof(double); }
};

// linkgp_Jsexp2_kernel<KS, TAB> (tch test points per workgroup)
struct JSexp2Lds {
    int WiT, WjT;        // [Dw][64] each
    int red;             // [tch][4]
    int etab;            // [EXPN_TAB]: 2^(j/EXPN_TAB), exp_negated_tab's table
    int end;
    LINKGP_HD JSexp2Lds(int Dw, int tch) {
        WiT = 0;
        WjT = WiT + Dw * 64;
        red = WjT + Dw * 64;
        etab = red + tch * 4;
        end = etab + EXPN_TAB;
    }
    LINKGP_HD size_t bytes() const { return (size_t)end * sizeof(double); }
};

// linkgp_Jsep_kernel<PIPE, LOG> (tch test points per workgroup)
struct JSepLds {
    int WiT, WjT;        // [DT][64] each
    int tz;              // [tch][Dz]
    int red;             // [tch][4]
    int PT;              // [2][128][PST]
    int smode;           // ints from here on: [Dw][4] per (dimension, wave) the order class of its rows against the tile's columns
    int nmode, slog;     // ints of smode; offset in ints behind smode of the step log (LOG: JSEP_LOG_STEPS x 4 x 2 stamps behind the kernel's own LDS)
    LINKGP_HD JSepLds(int Dw, int Dz, int tch) {
        const int DT = Dw + Dz;
        WiT = 0;
        WjT = WiT + DT * 64;
        tz = WjT + DT * 64;
        red = tz + tch * Dz;
        PT = red + tch * 4;
        smode = PT + 2 * 128 * PST;
        nmode = Dw * 4;
        slog = nmode + (Dw & 1) * 4;
    }
    LINKGP_HD size_t bytes(bool log) const {
        return (size_t)smode * sizeof(double) + (size_t)nmode * sizeof(int) + (log ? 16 + JSEP_LOG_STEPS * 8 * sizeof(long long) : 0);
    }
};

#ifdef __HIPCC__
// ---------------------------------------------------------------------------
// linked GP: closed forms of E[k(x,Z)] and E[k(x,Z) k(x',Z)], Z ~ N(m, v)
// ---------------------------------------------------------------------------
struct LinkArgs {
    int kind, Dw, Dz;
    int64_t n, M, t0, Mc;
    const double *m, *v, *z;
    const double *W, *Wg;
    double len[DGPAMD_MAXD];
    const double *Rinv;
    int64_t ldr;
    const double *ry;
    double scale, nugget;
    double *partial;   // [ntiles][Mc]
    double *recs;      // [Mc][Dw][npad][REC] separable Matern records (linkgp_Jsep)
    double *gfac;      // [Mc][npad] Matern factor of the deterministic global inputs (linkgp_Jsep)
    int64_t npad;
    double *mean, *var;
    const int32_t *drop;   // leave-one-out: training point left out of the conditioning set of test point t (else null)
    int no_order_classes;// linkgp_Jsep: treat every sub-tile as mixed (DGPAMD_JSEP_NOCLASS: the comparison run of the tools)
    int tch;             // linkgp_Jsep: test points per workgroup
    long long *dbg;        // linkgp_Jsep_kernel<2, true> (DGPAMD_JSEP_LOG=1 with dgpamd_debug_tasklog's buffer set): per-workgroup and per-step stamps, or null
};

// ---- the steps every pair kernel begins and ends with ---------------------------------------------------------------------
// The workgroup's place: lower tile (bi, bj) of C, its first rows / columns, its first test point and how many of its `tc`
// test points exist (clipped to M and to the chunk).
struct TilePlace {
    int bi, bj, nt;
    int64_t i0, j0, tbase;
};
__device__ __forceinline__ TilePlace tile_place(const LinkArgs &a, int tc) {
    TilePlace p;
    tri_decode(blockIdx.x, p.bi, p.bj);
    p.i0 = (int64_t)p.bi * 64;
    p.j0 = (int64_t)p.bj * 64;
    p.tbase = a.t0 + (int64_t)blockIdx.y * tc;
    p.nt = tc;
    if (p.tbase + p.nt > a.M) p.nt = (int)(a.M - p.tbase);
    if (p.tbase + p.nt > a.t0 + a.Mc) p.nt = (int)(a.t0 + a.Mc - p.tbase);
    return p;
}

// WiT / WjT [d][64] <- the tile's 64 rows and 64 columns of [W | Wg] (zero past n).  GLOBALS = false: W alone.
// CENTRE: the local columns relative to the first training point, w_k - W[0][k].  The expanded SExp forms build their
// exponent from products of the staged coordinates themselves (row term, column term, dot product: each of size c1 w^2,
// cancelling to the exponent), so they lose eps (|w| / l)^2 where the forms that difference first lose eps |w| / l; with
// the centre taken out |w| is at most the data's diameter.  W[0] needs no reduction and no launch, and it is the same in
// every chunk and launch of a call; the forms take it from m likewise (where they form 2 m, and in sexp_records_kernel),
// so that w - m and w_i - w_j stay what they were.  The global inputs enter as differences already.
template <bool GLOBALS = true, bool CENTRE = false>
__device__ __forceinline__ void stage_tile_inputs(const LinkArgs &a, const TilePlace &p, double *WiT, double *WjT) {
    const int Dw = a.Dw, Dz = a.Dz, DT = GLOBALS ? Dw + Dz : Dw;
    const int64_t n = a.n;
    for (int idx = threadIdx.x; idx < 64 * DT; idx += 256) {
        int row = idx / DT, d = idx - row * DT;
        int64_t gi = p.i0 + row, gj = p.j0 + row;
        double vi = 0.0, vj = 0.0;
        if (!GLOBALS || d < Dw) {
            const double c = CENTRE ? a.W[d] : 0.0;
            if (gi < n) vi = CENTRE ? a.W[gi * Dw + d] - c : a.W[gi * Dw + d];
            if (gj < n) vj = CENTRE ? a.W[gj * Dw + d] - c : a.W[gj * Dw + d];
        } else {
            if (gi < n) vi = a.Wg[gi * Dz + d - Dw];
            if (gj < n) vj = a.Wg[gj * Dz + d - Dw];
        }
        WiT[d * 64 + row] = vi;
        WjT[d * 64 + row] = vj;
    }
}

// tm, tv [nt][Dw] (MV) and tz [nt][Dz] <- m, v, z of the workgroup's test points
template <bool MV = true>
__device__ __forceinline__ void stage_test_points(const LinkArgs &a, const TilePlace &p, double *tm, double *tv, double *tz) {
    const int Dw = a.Dw, Dz = a.Dz;
    if (MV)
        for (int idx = threadIdx.x; idx < p.nt * Dw; idx += 256) {
            tm[idx] = a.m[p.tbase * Dw + idx];
            tv[idx] = a.v[p.tbase * Dw + idx];
        }
    for (int idx = threadIdx.x; idx < p.nt * Dz; idx += 256) tz[idx] = a.z[p.tbase * Dz + idx];
}

// MFMA accumulator layout of the 64x64 tile: wave w owns rows 16w..16w+15; element (tile tt, reg r) of a lane is
// row mrow + 4r, column 16tt + mcol with mrow = 16w + (lane>>4), mcol = lane&15  (v_mfma_f64_16x16x4_f64 C/D map).
// Cr[tt][r] = wt (ry_i ry_j - scale Rinv_ij) in that layout, zero past n
__device__ __forceinline__ void pair_weight_mfma(const LinkArgs &a, const TilePlace &p, double wt, int mrow, int mcol, d4 (&Cr)[4]) {
    const int64_t n = a.n;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t gi = p.i0 + mrow + 4 * r, gj = p.j0 + 16 * tt + mcol;
            Cr[tt][r] = (gi < n && gj < n) ? wt * (a.ry[gi] * a.ry[gj] - a.scale * a.Rinv[gi * a.ldr + gj]) : 0.0;
        }
}

// base[tt][r] = the t-independent part of the SExp exponent, sum_k (w_ik - w_jk)^2 / (2 l_k^2)  (= -log R2sexp,
// kernel_class.py:761-763), in that layout
__device__ __forceinline__ void base_exponent_mfma(const LinkArgs &a, const double *WiT, const double *WjT, int mrow, int mcol, d4 (&base)[4]) {
#pragma unroll
    for (int tt = 0; tt < 4; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double b = 0.0;
            for (int k = 0; k < a.Dw; ++k) {
                const double d = WiT[k * 64 + mrow + 4 * r] - WjT[k * 64 + 16 * tt + mcol];
                b = fma(d * d, 1.0 / (2.0 * a.len[k] * a.len[k]), b);
            }
            base[tt][r] = b;
        }
}

// partial[tile][t] <- the four waves' sums red[t][0..3] of the workgroup's test points (behind the caller's barrier)
__device__ __forceinline__ void store_partials(const LinkArgs &a, const TilePlace &p, const double *red) {
    const int tid = threadIdx.x;
    if (tid < p.nt)
        a.partial[(int64_t)blockIdx.x * a.Mc + (p.tbase - a.t0) + tid] = red[tid * 4] + red[tid * 4 + 1] + red[tid * 4 + 2] + red[tid * 4 + 3];
}
#endif
