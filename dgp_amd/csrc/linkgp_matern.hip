// Matern-2.5 J through the separable S/T form (linkfun.hpp).
//   matern_records_kernel : once per (test point, dimension, training point): S[0..11] T[12..26] f2[27] x[28] 0[29]  (REC = 30)
//   linkgp_Jsep_kernel    : one WG per (lower 64x64 tile of C) x (chunk of TCH test points); per (t, k) the 128
//                           records of its two point blocks are streamed global -> registers -> LDS one step
//                           ahead of the pair phase; every pair costs 30 FMAs (both orientations) and a select
//                           instead of 3 erf + 5 exp + ~300 flops.  The grid runs tiles fastest so that a
//                           test-chunk's records (TCH*Dw*n*240 B) are re-read from the Infinity Cache.
#include "linkgp_plan.hpp"
#include "linkfun.hpp"

#include <math.h>

__global__ __launch_bounds__(256) void matern_records_kernel(LinkArgs a) {
    // 128 points x (S role | T role) per workgroup; the 128 records are staged in LDS and leave as one contiguous
    // 30.7 KB block (a thread writing its own 240-byte record touched 64 cache lines per store instruction)
    __shared__ double stage[128 * (REC + 1)];
    const int tid = threadIdx.x, pp = tid & 127, role = tid >> 7;
    const int64_t i0 = (int64_t)blockIdx.x * 128, i = i0 + pp;
    const int k = blockIdx.y;
    const int64_t tt = blockIdx.z, t = a.t0 + tt;
    if (t >= a.M) return;
    const double x = (i < a.n) ? a.W[i * a.Dw + k] : 0.0;
    const double l = a.len[k], zm = a.m[t * a.Dw + k], zv = a.v[t * a.Dw + k];
    double *rec = stage + pp * (REC + 1);
    if (zv != 0.0) {
        MaternDimConst kc;
        matern_dim_const(zm, zv, l, kc);
        if (role == 0) {
            double f2;
            double out[12];
            matern_role_S(x, kc, out, f2);
#pragma unroll
            for (int c = 0; c < 12; ++c) rec[c] = out[c];
            rec[27] = f2;
            rec[28] = x;
        } else {
            double out[15];
            matern_role_T(x, kc, out);
#pragma unroll
            for (int c = 0; c < 15; ++c) rec[12 + c] = out[c];
            rec[29] = 0.0;
        }
    } else {   // deterministic input in this dimension: J factor = k(x_i, m) k(x_j, m)  (functions.py:488-491)
        const double pt = matern_point(zm - x, l);
        if (role == 0) {
            rec[0] = pt;
#pragma unroll
            for (int c = 1; c < 12; ++c) rec[c] = 0.0;
            rec[27] = 0.0;
            rec[28] = x;
        } else {
            rec[12] = pt;
#pragma unroll
            for (int c = 13; c < 27; ++c) rec[c] = 0.0;
            rec[29] = 0.0;
        }
    }
    __syncthreads();
    const int64_t npts = a.npad - i0 < 128 ? a.npad - i0 : 128;
    double *dst = a.recs + ((tt * a.Dw + k) * a.npad + i0) * REC;
    for (int e = tid; e < (int)npts * REC; e += 256) dst[e] = stage[(e / REC) * (REC + 1) + e % REC];
}

// Deterministic global inputs: the separable Matern factor k(Wg_i, z_t) of (training point, test point)
// (functions.py:413-420), once per pair of points instead of once per tile pair in the J kernel.
__global__ __launch_bounds__(256) void global_factor_kernel(LinkArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t tt = blockIdx.y, t = a.t0 + tt;
    if (i >= a.npad || t >= a.M) return;
    double pr = 1.0, sm = 0.0;
    if (i < a.n)
        for (int g = 0; g < a.Dz; ++g)
            corr_accum_matern((a.Wg[i * a.Dz + g] - a.z[t * a.Dz + g]) / a.len[a.Dw + g], pr, sm);
    a.gfac[tt * a.npad + i] = pr * exp(-SQRT5 * sm);
}

template <int PIPE, bool LOG>
__global__ __launch_bounds__(256, 2) void linkgp_Jsep_kernel(LinkArgs a) {
    extern __shared__ double lds[];
    const long long t_entry = LOG ? wall_clock64() : 0;   // (step log: when the workgroup began, ahead of its set-up)
    const int Dw = a.Dw, Dz = a.Dz;
    const int tch = a.tch;
    const JSepLds L(Dw, Dz, tch);
    double *WiT = lds + L.WiT, *WjT = lds + L.WjT, *tz = lds + L.tz, *red = lds + L.red, *PT = lds + L.PT;
    int *smode = reinterpret_cast<int *>(lds + L.smode);
    const TilePlace pl = tile_place(a, tch);
    const int bi = pl.bi, bj = pl.bj, nt = pl.nt;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t i0 = pl.i0, j0 = pl.j0, tbase = pl.tbase;

    stage_tile_inputs(a, pl, WiT, WjT);
    stage_test_points<false>(a, pl, nullptr, nullptr, tz);
    // (the MFMA accumulator layout: linkgp.hpp)
    const int mrow = 16 * wave + (lane >> 4), mcol = lane & 15, kq = lane >> 4, mi = lane & 15;
    const double wt = (bi == bj) ? 1.0 : 2.0;
    d4 Cr[4];
    pair_weight_mfma(a, pl, wt, mrow, mcol, Cr);
    // The 2 x 64 records of step (t, k) go from global memory straight into LDS (global_load_lds_dwordx4: one wave-instruction
    // moves 1 KB; the record in memory IS the LDS record, so the two blocks' 15 KB each are plain copies): 30 wave-loads per
    // step, issued right after the step's barrier into the buffer the previous step read, landed by the next barrier.  No
    // registers, no LDS stores, no address arithmetic per element (the register-staged version spent a fifth of the kernel
    // on its 7 loads + 16 LDS stores per thread and step).
    // (debug, timing only: no_order_classes & 2 makes every workgroup read the records of the first point block -- what the pair phase costs
    //  when its records come from the XCD's L2 instead of the fabric)
    const int64_t irec = (a.no_order_classes & 2) ? 0 : i0, jrec = (a.no_order_classes & 2) ? 0 : j0;
    // (addresses: the records of step s = t Dw + k of this chunk start at rec0 + s x npad x REC, so a step costs one scalar multiply-add; the wave number is made
    //  uniform so that the KB numbers, the LDS destinations (M0) and the `q < 30` tests are scalar -- computed per lane they were 16 VALU instructions, four
    //  readfirstlanes and four exec-masked branches per step, between the barrier and the first fragment read)
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const double *rec0 = a.recs + (tbase - a.t0) * Dw * a.npad * REC + lane * 2;
    const int64_t sstride = a.npad * REC;
    const int qlim = (a.no_order_classes & 32) ? 15 : 30;
    auto stage = [&](int s1, double *P, int u0 = 0, int u1 = 8) {
        const double *base = rec0 + s1 * sstride;
#pragma unroll
        for (int u = u0; u < u1; ++u) {
            const int q = wv + 4 * u;   // KB number q of the 30-KB image: 0..14 the row block, 15..29 the column block
            if (q < qlim) {
                const double *src = base + (q >= 15 ? jrec * REC + (q - 15) * 128 : irec * REC + q * 128);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(P + q * 128), 16, 0, 0);
            }
        }
    };
    const int iSd = kq < 3 ? 6 + kq : 29, iTd = kq < 3 ? 24 + kq : 29;   // (unconditional loads: no exec-masked branches in the pair loop)
    __syncthreads();
    // Order classes.  The J factor of a pair is <S(x_lo), T(x_hi)> + (f2_hi - f2_lo) <S'(x_lo), T'(x_hi)> with lo / hi the pair's
    // smaller / larger coordinate in dimension k: a wave's 16 rows whose coordinates all lie at or below those of the tile's 64
    // columns (class 1) or all above them (class 2) need ONE of the two record products, 4 MFMAs per 16 x 16 sub-tile instead
    // of 8 and no select.  Training points that arrive ordered by cells (dgp_amd.ops.cell_order) make about half of the (rows,
    // tile, dimension) triples such; any other order is class 0 throughout and costs what it did.  (Padding rows / columns are staged as x = 0 and
    // take part in the bounds, so that every element -- also the ones C zeroes -- gets the orientation the select would pick.)
    for (int idx = tid; idx < Dw * 4; idx += 256) {
        const int k = idx >> 2, w = idx & 3;
        double rlo = WiT[k * 64 + 16 * w], rhi = rlo, clo = WjT[k * 64], chi = clo;
        for (int r = 1; r < 16; ++r) {
            const double x = WiT[k * 64 + 16 * w + r];
            rlo = x < rlo ? x : rlo;
            rhi = x > rhi ? x : rhi;
        }
        for (int c = 1; c < 64; ++c) {
            const double x = WjT[k * 64 + c];
            clo = x < clo ? x : clo;
            chi = x > chi ? x : chi;
        }
        smode[idx] = (a.no_order_classes & 4) ? 1 : ((a.no_order_classes & 1) ? 0 : (rhi <= clo ? 1 : (rlo > chi ? 2 : 0)));
    }
    __syncthreads();
    // The records of step (t, k) are double buffered in LDS: ONE barrier per step.
    double *PT1 = PT + 128 * PST;
    const int nstep = nt * Dw;
    if (nstep > 0) stage(0, PT);
    int step = 0;
    int mw_next = __builtin_amdgcn_readfirstlane(smode[wave]);
    // (diagnostics, LOG only: workgroup start / end on the 100-MHz clock and in shader cycles, where it ran, and for its first
    //  JSEP_LOG_STEPS steps every wave's arrival at and departure from the step's barrier -- tools/gpu_pair_steplog.py)
    long long *lg = nullptr;
    long long *slog = reinterpret_cast<long long *>(smode + L.slog);
    if (LOG && a.dbg) {
        for (int e = tid; e < JSEP_LOG_STEPS * 8; e += 256) slog[e] = 0;
        lg = a.dbg + 64 + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * JSEP_LOG_WORDS;
        if (tid == 0) {
            lg[0] = wall_clock64();
            lg[2] = clock64();
            lg[4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
            lg[5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
            lg[6] = ((long long)bi << 16) | bj;
            lg[7] = t_entry;   // (the steps of a full chunk: a.tch x Dw)
        }
    }
    for (int t = 0; t < nt; ++t) {
        d4 prod[4];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) prod[tt] = (d4){1.0, 1.0, 1.0, 1.0};
#pragma unroll 1
        for (int k = 0; k < Dw; ++k, ++step) {
            double *P = (step & 1) ? PT1 : PT;
            if (LOG && lg && step < JSEP_LOG_STEPS && lane == 0) slog[(step * 4 + wave) * 2] = clock64();   // (kept in LDS: a global store here would be waited for by the barrier's vmcnt(0))
            // records of this step landed; every wave is done with the other buffer.  The drain is explicit: a workgroup-scope fence orders LDS and scalar
            // traffic only (lgkmcnt), and the other waves read this wave's DMA right behind the barrier -- the compiler happens to put its own vmcnt(0)
            // here, nothing obliges it to (tests/test_isa_hazards.py checks the emitted code)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (LOG && lg && step < JSEP_LOG_STEPS && lane == 0) slog[(step * 4 + wave) * 2 + 1] = clock64() | ((long long)mw_next << 60);
            // the next step's records into the other buffer.  Past the end the last step is staged again (harmless).
            const int s1 = step + 1 < nstep ? step + 1 : nstep - 1;
            const bool nostage = (a.no_order_classes & 8) != 0;   // (timing only)
            if (PIPE == 0 && !nostage) stage(s1, (step & 1) ? PT : PT1);   // (comparison build: all eight right behind the barrier)
            // volatile: keeps these fragment reads as ds_read_b64 (2 LDS cycles, 64 banks: conflict-free with PST = 30); merged
            // into ds_read2_b64 by the compiler they take 8 cycles and bank modulo 32 (2-way conflicts here)
            const vlds_double *Arow = (const vlds_double *)(P + (16 * wave + mi) * PST);   // this lane's row record as an MFMA A operand (i = lane&15)
            double f2r[4], xr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                f2r[r] = P[(mrow + 4 * r) * PST + 27];
                xr[r] = P[(mrow + 4 * r) * PST + 28];
            }
            const int mw = mw_next;   // (read one step ahead: the LDS round trip + readfirstlane sat between the barrier and the first MFMA)
            const int mraw = ((const volatile int *)smode)[(k + 1 < Dw ? k + 1 : 0) * 4 + wave];
            if (mw == 0) {   // mixed: both record products, selected per pair
                // A fragments (rows): S[0..11] and T[0..11] in three k-steps each, the erf-difference pair in one (k=3 padded with 0)
                double aS[3], aT[3];
#pragma unroll
                for (int ks = 0; ks < 3; ++ks) {
                    aS[ks] = Arow[4 * ks + kq];
                    aT[ks] = Arow[12 + 4 * ks + kq];
                }
                const double aSd = Arow[iSd], aTd = Arow[iTd];
                // Column tiles software pipelined by hand: the 8 MFMAs of tile tt+1 are issued in pairs between the four
                // row groups of tile tt's (VALU) epilogue; the sched_barrier() fences pin that order (on its own the compiler
                // issues all 32 MFMAs first and all epilogues afterwards).
                d4 o1[2], o2[2], e1[2], e2[2];
                // The column fragments are read TWO tiles ahead (two register sets) and a tile's f2 / x one tile ahead: the LDS round trip of a
                // fragment read sat in front of every MFMA group otherwise (read, wait, MFMA), and with two waves per SIMD nobody hides it.
                double bf[2][8], f2c[2], xc[2];
                auto loadB = [&](int tt, int s) {   // column records as MFMA B operands (j = lane&15)
                    const vlds_double *Bcol = (const vlds_double *)(P + (64 + 16 * tt + mi) * PST);
#pragma unroll
                    for (int ks = 0; ks < 3; ++ks) {
                        bf[s][ks] = Bcol[12 + 4 * ks + kq];
                        bf[s][3 + ks] = Bcol[4 * ks + kq];
                    }
                    bf[s][6] = Bcol[iTd];
                    bf[s][7] = Bcol[iSd];
                };
                auto loadC = [&](int tt, int s) {
                    const vlds_double *Ccol = (const vlds_double *)(P + (64 + 16 * tt + mcol) * PST);
                    f2c[s] = Ccol[27];
                    xc[s] = Ccol[28];
                };
                auto mm2 = [&](int c, int slot) {   // MFMA pair c of a tile: S_row . T_col and T_row . S_col, then the erf pair
                    const d4 z = {0.0, 0.0, 0.0, 0.0};
                    if (c < 3) {
                        o1[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(aS[c], bf[slot][c], c ? o1[slot] : z, 0, 0, 0);
                        o2[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(aT[c], bf[slot][3 + c], c ? o2[slot] : z, 0, 0, 0);
                    } else {
                        e1[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(aSd, bf[slot][6], z, 0, 0, 0);
                        e2[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(aTd, bf[slot][7], z, 0, 0, 0);
                    }
                };
                loadB(0, 0);
                loadC(0, 0);
#pragma unroll
                for (int c = 0; c < 4; ++c) mm2(c, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int sl = tt & 1;
                    if (PIPE == 2 && !nostage) stage(s1, (step & 1) ? PT : PT1, 2 * tt, 2 * tt + 2);
                    if (tt < 3) loadC(tt + 1, sl ^ 1);
                    if (tt < 3) loadB(tt + 1, sl ^ 1);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (tt < 3) mm2(r, sl ^ 1);
                        const double d = f2c[sl] - f2r[r];
                        const double j1 = fma(d, e1[sl][r], o1[sl][r]), j2 = fma(-d, e2[sl][r], o2[sl][r]);
                        prod[tt][r] *= (xr[r] <= xc[sl]) ? j1 : j2;
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            } else {
                // one orientation for the whole 16 x 64 strip.  Class 1 (rows at or below columns): <S_row, T_col> + d <S'_row, T'_col>;
                // class 2 (rows above columns): <T_row, S_col> - d <T'_row, S'_col>, d = f2_col - f2_row.  The two differ in record
                // offsets and one sign only; the pipelining is the mixed path's with four MFMAs per sub-tile.
                const bool c1 = mw == 1;
                const int offA = c1 ? 0 : 12, offB = c1 ? 12 : 0, iAd = c1 ? iSd : iTd, iBd = c1 ? iTd : iSd;
                const double aX0 = Arow[offA + kq], aX1 = Arow[offA + 4 + kq], aX2 = Arow[offA + 8 + kq], aD = Arow[iAd];
                double g2r[4];   // (-d = f2_row - f2_col exactly: the signs go onto the two differences' operands)
#pragma unroll
                for (int r = 0; r < 4; ++r) g2r[r] = c1 ? f2r[r] : -f2r[r];
                d4 oo[2], ee[2];
                double bx[2][4], g2c[2];
                auto loadBc = [&](int tt, int s) {
                    const vlds_double *Bcol = (const vlds_double *)(P + (64 + 16 * tt + mi) * PST);
                    bx[s][0] = Bcol[offB + kq];
                    bx[s][1] = Bcol[offB + 4 + kq];
                    bx[s][2] = Bcol[offB + 8 + kq];
                    bx[s][3] = Bcol[iBd];
                };
                auto loadCc = [&](int tt, int s) {
                    const vlds_double *Ccol = (const vlds_double *)(P + (64 + 16 * tt + mcol) * PST);
                    g2c[s] = Ccol[27];
                };
                auto mmc = [&](int c, int slot) {
                    const d4 z = {0.0, 0.0, 0.0, 0.0};
                    if (c == 0) oo[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(aX0, bx[slot][0], z, 0, 0, 0);
                    else if (c == 1) ee[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(aD, bx[slot][3], z, 0, 0, 0);
                    else if (c == 2) oo[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(aX1, bx[slot][1], oo[slot], 0, 0, 0);
                    else oo[slot] = __builtin_amdgcn_mfma_f64_16x16x4f64(aX2, bx[slot][2], oo[slot], 0, 0, 0);
                };
                loadBc(0, 0);
                loadCc(0, 0);
#pragma unroll
                for (int c = 0; c < 4; ++c) mmc(c, 0);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int sl = tt & 1;
                    if (PIPE == 2 && !nostage) stage(s1, (step & 1) ? PT : PT1, 2 * tt, 2 * tt + 2);
                    if (tt < 3) loadCc(tt + 1, sl ^ 1);
                    if (tt < 3) loadBc(tt + 1, sl ^ 1);
                    const double g2 = c1 ? g2c[sl] : -g2c[sl];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (tt < 3) mmc(r, sl ^ 1);
                        prod[tt][r] *= fma(g2 - g2r[r], ee[sl][r], oo[sl][r]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            mw_next = __builtin_amdgcn_readfirstlane(mraw);
        }
        // deterministic global inputs: separable Matern factor (functions.py:413-420), precomputed per point
        double gr[4], gc[4];
        if (Dz) {
            const double *gf = a.gfac + ((tbase - a.t0) + t) * a.npad;
#pragma unroll
            for (int r = 0; r < 4; ++r) gr[r] = gf[i0 + mrow + 4 * r];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) gc[tt] = gf[j0 + 16 * tt + mcol];
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) gr[r] = gc[r] = 1.0;
        }
        double acc = 0.0;
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = fma(Cr[tt][r], prod[tt][r] * gr[r] * gc[tt], acc);
        acc = wave_sum(acc);
        if (lane == 0) red[t * 4 + wave] = acc;
    }
    // (the compiler's barrier waits for LDS and scalar traffic only -- s_waitcnt lgkmcnt(0); s_barrier; s_endpgm in the emitted code: the last step's redundant
    //  DMA, still in flight, would land in the LDS of whichever workgroup is given that space next)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (LOG && lg) {
        if (tid == 0) {
            lg[1] = wall_clock64();
            lg[3] = clock64();
        }
        for (int e = tid; e < JSEP_LOG_STEPS * 8; e += 256) lg[8 + e] = slog[e];
    }
    store_partials(a, pl, red);
}

// one chunk of `mc` test points: the records, the global factors, then the pair kernel of the plan's variant
int linkgp_launch_matern_sep(dgpamd_ctx *ctx, LinkArgs a, const LinkPlan &p, int64_t mc) {
    void (*fn)(LinkArgs) = p.plog ? linkgp_Jsep_kernel<2, true> : (p.pipe == 0 ? linkgp_Jsep_kernel<0, false> : linkgp_Jsep_kernel<2, false>);
    const unsigned tb = (unsigned)((mc + p.tc - 1) / p.tc);
    a.no_order_classes = p.no_order_classes;
    a.dbg = (p.plog && ctx->tlog_words >= 64 + (long long)p.ntiles * tb * JSEP_LOG_WORDS) ? ctx->tlog : nullptr;
    int rc = set_lds(ctx, (const void *)fn, p.lds);
    if (rc) return rc;
    hipLaunchKernelGGL(matern_records_kernel, dim3((unsigned)((a.npad + 127) / 128), a.Dw, (unsigned)mc), dim3(256), 0, ctx->stream, a);
    if (a.Dz)
        hipLaunchKernelGGL(global_factor_kernel, dim3((unsigned)((a.npad + 255) / 256), (unsigned)mc), dim3(256), 0, ctx->stream, a);
    PROF_BEGIN(ctx, PROF_LINKGP_J, (double)mc * (double)a.n * (double)a.n * 0.5 * a.Dw * 30.0 * 2.0);
    hipLaunchKernelGGL(fn, dim3(p.ntiles, tb), dim3(256), p.lds, ctx->stream, a);
    PROF_END(ctx, PROF_LINKGP_J);
    return DGPAMD_OK;
}
