// Linked-GP pair kernels of the squared-exponential kernel: the first form (MFMA over LDS operands) and the second
// (per-point records, operands in registers).
#include "linkgp_plan.hpp"

#include <math.h>

// SExp J with the pair loop on MFMA (functions.py:432-451 restated).  For test point t the exponent of pair (i, j) is
//   base_ij + ei_i(t) + ej_j(t) + sum_k c1_k(t) (w_ik - 2 m_k(t) + w_jk)^2,    c1_k = 1 / (8 v_k + 2 l_k^2),
// and the square expands into a row term, a column term and the dot product sum_k [2 c1_k (w_ik - 2 m_k)] w_jk: per
// test point the 64 x 64 x Dw products of a tile are a handful of v_mfma_f64_16x16x4 (accumulated on top of base_ij,
// which sits in the accumulator layout), and the VALU work per pair drops from 3 Dw + exp to 2 adds + exp.  The row /
// column terms and the A operand of test point t+1 are staged (double buffered in LDS) while t is evaluated.
// The three terms cancel to the exponent, so w and m are taken relative to W[0] where they are staged (stage_tile_inputs,
// CENTRE; m where 2 m is formed below) -- the exponent depends on w_i + w_j - 2 m alone -- which keeps each term at the size of
// (the data's diameter / l)^2 wherever the inputs lie.
__global__ __launch_bounds__(256, 3) void linkgp_Jsexp_kernel(LinkArgs a) {
    extern __shared__ double lds[];
    const int Dw = a.Dw, Dz = a.Dz;
    const JSexpLds L(Dw, Dz);
    const int KP = L.KP, LDU = L.LDU;
    double *WiT = lds + L.WiT, *WjT = lds + L.WjT, *WjB = lds + L.WjB, *tm = lds + L.tm, *tv = lds + L.tv, *tz = lds + L.tz;
    double *red = lds + L.red, *U = lds + L.U, *R = lds + L.R, *S = lds + L.S, *ilg = lds + L.ilg;
    const TilePlace pl = tile_place(a, TCH);
    const int bi = pl.bi, bj = pl.bj, nt = pl.nt;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

    stage_tile_inputs<true, true>(a, pl, WiT, WjT);   // (w relative to W[0]: linkgp.hpp; m below)
    stage_test_points(a, pl, tm, tv, tz);
    for (int g = tid; g < Dz; g += 256) ilg[g] = 1.0 / a.len[Dw + g];
    __syncthreads();
    for (int idx = tid; idx < KP * 64; idx += 256) {
        const int k = idx >> 6, j = idx & 63;
        WjB[k * LDK + j] = k < Dw ? WjT[k * 64 + j] : 0.0;
    }
    // accumulator layout: wave w owns rows 16w..16w+15; element (tile tt, reg r) of a lane = row 16w + (lane>>4) + 4r,
    // column 16tt + (lane&15)
    const int mrow = 16 * wave + (lane >> 4), mcol = lane & 15, kq = lane >> 4, mi = lane & 15;
    const double wt = (bi == bj) ? 1.0 : 2.0;
    d4 Cr[4], base[4];
    pair_weight_mfma(a, pl, wt, mrow, mcol, Cr);
    base_exponent_mfma(a, WiT, WjT, mrow, mcol, base);
    // per-test-point constants, once: tv <- c1_k(t) = 1 / (8 v_k + 2 l_k^2), tm <- 2 m_k(t); reciprocal lengthscales of the
    // global dimensions (no divisions in the staging below)
    for (int idx = tid; idx < nt * Dw; idx += 256) {
        const double l = a.len[idx % Dw];
        tv[idx] = 1.0 / (8.0 * tv[idx] + 2.0 * l * l);
        tm[idx] = 2.0 * (tm[idx] - a.W[idx % Dw]);   // (relative to W[0], as the staged w)
    }
    // staging of test point t: 128 point tasks (64 row points: A operand + row term; 64 column points: column term)
    // on the even threads, so that the four waves share them evenly
    auto stage = [&](int t, int buf) {
        if (tid & 1) return;
        const int task = tid >> 1;
        const double *c1 = tv + t * Dw, *m2 = tm + t * Dw, *zt = tz + t * Dz;
        if (task < 64) {
            double rr = 0.0;
            double *u = U + (buf * 64 + task) * LDU;
            for (int k = 0; k < Dw; ++k) {
                const double wi = WiT[k * 64 + task] - m2[k], cw = c1[k] * wi;
                u[k] = 2.0 * cw;
                rr = fma(cw, wi, rr);
            }
            for (int k = Dw; k < KP; ++k) u[k] = 0.0;
            for (int g = 0; g < Dz; ++g) {
                const double di = (WiT[(Dw + g) * 64 + task] - zt[g]) * ilg[g];
                rr = fma(di, di, rr);
            }
            R[buf * 64 + task] = rr;
        } else {
            const int j = task - 64;
            double ss = 0.0;
            for (int k = 0; k < Dw; ++k) {
                const double wj = WjT[k * 64 + j];
                ss = fma(c1[k] * wj, wj, ss);
            }
            for (int g = 0; g < Dz; ++g) {
                const double dj = (WjT[(Dw + g) * 64 + j] - zt[g]) * ilg[g];
                ss = fma(dj, dj, ss);
            }
            S[buf * 64 + j] = ss;
        }
    };
    __syncthreads();
    if (nt > 0) stage(0, 0);
    for (int t = 0; t < nt; ++t) {
        const int buf = t & 1;
        __syncthreads();   // stage(t) visible; everybody is done with the other buffer
        if (t + 1 < nt) stage(t + 1, buf ^ 1);
        const vlds_double *Ur = (const vlds_double *)(U + (buf * 64 + 16 * wave + mi) * LDU);
        const vlds_double *Bv = (const vlds_double *)WjB;
        d4 e[4] = {base[0], base[1], base[2], base[3]};
        for (int k0 = 0; k0 < KP; k0 += 4) {
            const double av = Ur[k0 + kq];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
                e[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bv[(k0 + kq) * LDK + 16 * tt + mi], e[tt], 0, 0, 0);
        }
        double rr[4], acc = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) rr[r] = R[buf * 64 + mrow + 4 * r];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const double ss = S[buf * 64 + 16 * tt + mcol];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = fma(Cr[tt][r], exp_negated(e[tt][r] + rr[r] + ss), acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) red[t * 4 + wave] = acc;
    }
    __syncthreads();
    store_partials(a, pl, red);
}

// ---- SExp J, second form: per-(test point, training point) records + a pair loop without LDS -------------------------
// The exponent of pair (i, j) at test point t is  base_ij + sum_k u_ik(t) w_jk + rr_i(t) + ss_j(t)  (see above).  The t-
// dependent per-point quantities -- u (Dw values), rr, ss -- are computed ONCE per (t, point) by sexp_records_kernel
// instead of once per tile pair inside the pair kernel (where that staging was a quarter of its VALU instructions), and the
// two additive terms ride in the MFMA as two more k-columns:  A_i = [u_i | rr_i | 1 | 0..],  B_j = [w_j ; 1 ; ss_j ; 0..]
// (k padded to a multiple of 4).  The B operand's rows are t-independent except the ss row, so a lane keeps its B fragments
// in REGISTERS for all test points of the chunk and the lanes that hold the ss row load theirs from the records; the A
// fragments of a test point are three or four 8-byte loads per lane from the records (L2 / Infinity Cache resident: the
// grid runs the tiles of a test chunk back to back), prefetched one test point ahead.  The MFMA's C input is base_ij, its
// output the whole exponent: per pair the VALU work is the exponential and one multiply-add.  No LDS traffic, no barrier
// in the loop over test points.  For Dw <= 14 (four k-steps); wider nodes keep linkgp_Jsexp_kernel.
__global__ __launch_bounds__(256) void sexp_records_kernel(LinkArgs a, int KPA) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t tt = blockIdx.y, t = a.t0 + tt;
    if (i >= a.npad || t >= a.M) return;
    double *ra = a.recs + (tt * a.npad + i) * KPA;
    double rr = 0.0, ss = 0.0;
    if (i < a.n) {
        for (int k = 0; k < a.Dw; ++k) {
            // (w and m relative to W[0], as the pair kernel stages its B operand: linkgp.hpp, stage_tile_inputs)
            const double l = a.len[k], c1 = 1.0 / (8.0 * a.v[t * a.Dw + k] + 2.0 * l * l), c = a.W[k], w = a.W[i * a.Dw + k] - c;
            const double d = w - 2.0 * (a.m[t * a.Dw + k] - c), cw = c1 * d;
            ra[k] = 2.0 * cw;
            rr = fma(cw, d, rr);
            ss = fma(c1 * w, w, ss);
        }
        // (a point sees the same global-input term in its row and in its column role; added in the first form's order)
        for (int g = 0; g < a.Dz; ++g) {
            const double di = (a.Wg[i * a.Dz + g] - a.z[t * a.Dz + g]) * (1.0 / a.len[a.Dw + g]);
            rr = fma(di, di, rr);
            ss = fma(di, di, ss);
        }
    } else {
        for (int k = 0; k < a.Dw; ++k) ra[k] = 0.0;
    }
    ra[a.Dw] = rr;
    ra[a.Dw + 1] = 1.0;
    for (int k = a.Dw + 2; k < KPA; ++k) ra[k] = 0.0;
    a.gfac[tt * a.npad + i] = ss;
}

// KS = k-steps (compile time: no branches in the loop over test points).  The MFMAs of test point t + 1 are issued between
// the four column-tile groups of test point t's exponentials.  The loop is unrolled by two so that the exponent tiles of
// consecutive test points alternate between two register sets without copies.
template <int KS, bool TAB>
__global__ __launch_bounds__(256, 2) void linkgp_Jsexp2_kernel(LinkArgs a) {
    extern __shared__ double lds[];
    constexpr int KPA = 4 * KS;
    const int Dw = a.Dw;
    const int tch2 = a.tch;               // (this kernel's test points per workgroup)
    const JSexp2Lds L(Dw, tch2);
    double *WiT = lds + L.WiT, *WjT = lds + L.WjT, *red = lds + L.red, *etab = lds + L.etab;
    const TilePlace pl = tile_place(a, tch2);
    const int bi = pl.bi, bj = pl.bj, nt = pl.nt;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int j = tid; j < EXPN_TAB; j += 256) etab[j] = exp2((double)j * (1.0 / EXPN_TAB));
    const int64_t i0 = pl.i0, j0 = pl.j0, n = a.n;
    const int64_t tt0 = (int64_t)blockIdx.y * tch2;
    stage_tile_inputs<false, true>(a, pl, WiT, WjT);   // (the global inputs' terms come in the records; w relative to W[0] as in the records)
    __syncthreads();
    const int mrow = 16 * wave + (lane >> 4), mcol = lane & 15, kq = lane >> 4, mi = lane & 15;
    const int kqS = (Dw + 1) & 3;   // (the ss row: k = Dw + 1, in k-step (Dw + 1) >> 2 == KS - 1)
    const bool dyn = kq == kqS;   // this lane holds the ss row in its B fragment of the last k-step
    const double wt = (bi == bj) ? 1.0 : 2.0;
    d4 Cr[4], base[4];
    // The tile's weights: all 24 loads go out back to back, at clamped indices with the bound applied to the value, and land under the base exponents'
    // arithmetic.  (Written as a conditional load inside the element loop every element was a branch with a load round trip of its own -- s_waitcnt
    // vmcnt(1), vmcnt(0), sixteen times, ~15 us of a workgroup's 130-260.  No LDS-DMA in this kernel: register loads in flight together are safe.)
    {
        double ryr[4], ryc[4];
        int64_t cir[4], cjc[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t gi = i0 + mrow + 4 * r;
            cir[r] = gi < n ? gi : n - 1;
            ryr[r] = a.ry[cir[r]];
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int64_t gj = j0 + 16 * tt + mcol;
            cjc[tt] = gj < n ? gj : n - 1;
            ryc[tt] = a.ry[cjc[tt]];
        }
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) Cr[tt][r] = a.Rinv[cir[r] * a.ldr + cjc[tt]];
        base_exponent_mfma(a, WiT, WjT, mrow, mcol, base);
#pragma unroll
        for (int tt = 0; tt < 4; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool in = i0 + mrow + 4 * r < n && j0 + 16 * tt + mcol < n;
                Cr[tt][r] = in ? wt * (ryr[r] * ryc[tt] - a.scale * Cr[tt][r]) : 0.0;
            }
    }
    // static B fragments: B[k][j], k = 4 ks + kq, j = 16 tt + mi (the ss row's lanes get theirs per test point)
    double bst[KS][4];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int k = 4 * ks + kq;
            bst[ks][tt] = k < Dw ? WjT[k * 64 + 16 * tt + mi] : (k == Dw ? 1.0 : 0.0);
        }
    const double *recA = a.recs + (tt0 * a.npad + i0 + 16 * wave + mi) * KPA + kq;   // + t * npad * KPA + 4 ks
    const double *recS = a.gfac + tt0 * a.npad + j0 + mi;                               // + t * npad + 16 tt
    const int64_t strA = a.npad * KPA, strS = a.npad;
    struct Frag { double av[KS], bd[4]; };
    auto fetch = [&](int t) {
        Frag f;
        t = t < nt ? t : nt - 1;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) f.av[ks] = recA[t * strA + 4 * ks];
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) f.bd[tt] = dyn ? recS[t * strS + 16 * tt] : bst[KS - 1][tt];   // (the ss row lies in the LAST k-step: (Dw + 1) >> 2 == KS - 1)
        return f;
    };
    // one k-step of test point f's exponent tiles into `en` (four independent MFMAs)
    auto kstep = [&](const Frag &f, int ks, d4 (&en)[4]) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const double bv = (ks == KS - 1) ? f.bd[tt] : bst[ks][tt];   // (selected once per test point, in fetch: three selects per k-step and tile here otherwise)
            en[tt] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.av[ks], bv, ks == 0 ? base[tt] : en[tt], 0, 0, 0);
        }
    };
    // exponentials of column tile g of `e`, weights Cr.  TAB: the table reads of tile g + 1 are issued (begin) before tile g's arithmetic and pinned there,
    // so that their LDS round trip runs under it (they sat, one by one, directly in front of their use).
    double kfa[4], ta[4], kfb[4], tb[4];
    auto begin = [&](const d4 (&e)[4], int g, double (&kf)[4], double (&t)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) exp_negated_tab_begin(e[g][r], etab, kf[r], t[r]);
    };
    auto group = [&](const d4 (&e)[4], int g, double &acc, const double (&kf)[4], const double (&t)[4]) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc = fma(Cr[g][r], TAB ? exp_negated_tab_end(e[g][r], kf[r], t[r]) : exp_negated(e[g][r]), acc);
    };
    // test point t from `e`, while test point t + 1 (fragments f1) goes into `en`; f2 <- fragments of t + 2
    auto step = [&](int t, const d4 (&e)[4], d4 (&en)[4], const Frag &f1, Frag &f2) {
        f2 = fetch(t + 2);
        if (TAB) begin(e, 0, kfa, ta);
        __builtin_amdgcn_sched_barrier(0);
        double acc = 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            // k-step g of the NEXT test point (four independent MFMAs) and the four exponentials of column tile g of THIS one
            // in one scheduling region, the scheduler asked for  MFMA, ~20 VALU, MFMA, ~20 VALU, ...  (inside the VALU slots the
            // four exponentials still interleave; a barrier after every exponential serialised their dependent chains: 4x
            // slower).  Measured: the f64 MFMA and the f64 VALU work do NOT overlap on gfx950 whatever the order -- the run time
            // is the sum of the two (41 ms = 29 without the products + 12; 78.6 TFLOP/s is the matrix AND the vector f64 peak:
            // one set of double-precision units) -- so the order only keeps the products' operands off the critical path.
            if (TAB && g < 3) {
                if (g & 1) begin(e, g + 1, kfa, ta);
                else begin(e, g + 1, kfb, tb);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (g < KS) kstep(f1, g, en);
            if (g & 1) group(e, g, acc, kfb, tb);
            else group(e, g, acc, kfa, ta);
            if (g < KS) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // one MFMA
                    __builtin_amdgcn_sched_group_barrier(0x002, TAB ? 16 : 21, 0);   // the VALU instructions of about one exponential
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        acc = wave_sum(acc);
        if (lane == 0) red[t * 4 + wave] = acc;
    };
    if (nt > 0) {
        Frag fa = fetch(0), fb = fetch(1), fc;
        d4 e0[4], e1[4];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kstep(fa, ks, e0);
        for (int t = 0; t < nt; t += 2) {
            step(t, e0, e1, fb, fc);        // t from e0; t + 1 -> e1 (fragments fb); fc <- t + 2
            if (t + 1 < nt) step(t + 1, e1, e0, fc, fb);   // t + 1 from e1; t + 2 -> e0 (fragments fc); fb <- t + 3
        }
    }
    __syncthreads();
    store_partials(a, pl, red);
}

// one chunk of `mc` test points, first form
int linkgp_launch_sexp_mfma(dgpamd_ctx *ctx, const LinkArgs &a, const LinkPlan &p, int64_t mc) {
    int rc = set_lds(ctx, (const void *)linkgp_Jsexp_kernel, p.lds);
    if (rc) return rc;
    hipLaunchKernelGGL(linkgp_Jsexp_kernel, dim3(p.ntiles, (unsigned)((mc + p.tc - 1) / p.tc)), dim3(256), p.lds, ctx->stream, a);
    return DGPAMD_OK;
}

// ... second form: the records, then the pair kernel of the plan's k-steps and exponential
int linkgp_launch_sexp_records(dgpamd_ctx *ctx, const LinkArgs &a, const LinkPlan &p, int64_t mc) {
    static void (*const JSEXP2[4][2])(LinkArgs) = {   // [KPA / 4 - 1][the table form]
        {linkgp_Jsexp2_kernel<1, false>, linkgp_Jsexp2_kernel<1, true>}, {linkgp_Jsexp2_kernel<2, false>, linkgp_Jsexp2_kernel<2, true>},
        {linkgp_Jsexp2_kernel<3, false>, linkgp_Jsexp2_kernel<3, true>}, {linkgp_Jsexp2_kernel<SX_KS, false>, linkgp_Jsexp2_kernel<SX_KS, true>}};
    void (*fn)(LinkArgs) = JSEXP2[p.KPA / 4 - 1][p.poly ? 0 : 1];
    int rc = set_lds(ctx, (const void *)fn, p.lds);
    if (rc) return rc;
    hipLaunchKernelGGL(sexp_records_kernel, dim3((unsigned)((a.npad + 255) / 256), (unsigned)mc), dim3(256), 0, ctx->stream, a, p.KPA);
    PROF_BEGIN(ctx, PROF_LINKGP_J, (double)mc * (double)a.n * (double)(a.n + 1) * 0.5);   // pair evaluations (one exponential each)
    hipLaunchKernelGGL(fn, dim3(p.ntiles, (unsigned)((mc + p.tc - 1) / p.tc)), dim3(256), p.lds, ctx->stream, a);
    PROF_END(ctx, PROF_LINKGP_J);
    return DGPAMD_OK;
}
