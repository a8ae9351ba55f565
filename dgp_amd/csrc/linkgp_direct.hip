// Linked-GP pair kernel, direct form: the reference's J factor evaluated per pair -- the comparison form of
// dgpamd_set_linkgp_direct, every leave-one-out call, and SExp nodes too wide for the MFMA form's LDS.
#include "linkgp_plan.hpp"
#include "linkfun.hpp"

#include <math.h>

// partial[tile][t] = sum_{(i,j) in tile} wt (ry_i ry_j - scale Rinv_ij) Jhat_ij(t)
// (sexp: Jhat = J / J_coef1, the prefactor is applied in the finalize kernel)
// LOO: test point t conditions on every training point but d = drop[t].  With u = Rinv[:, d], rho = u_d the inverse of
// the reduced correlation matrix (embedded, zero row / column d) is Rinv - u u^T / rho, so the pair weight becomes
//   wt [ (ry_i - c u_i)(ry_j - c u_j) - scale (Rinv_ij - u_i u_j / rho) ],   c = ry_d / rho.
// TC: test points per workgroup (TCH; half of it where the Matern leave-one-out form would not fit in a CU's LDS)
template <int KIND, bool LOO, int TC = TCH>
__global__ __launch_bounds__(256) void linkgp_J_kernel(LinkArgs a) {
    extern __shared__ double lds[];
    const int Dw = a.Dw, Dz = a.Dz;
    const JDirectLds L(KIND, Dw, Dz, TC, LOO);
    double *WiT = lds + L.WiT, *WjT = lds + L.WjT, *tm = lds + L.tm, *tv = lds + L.tv, *tz = lds + L.tz, *red = lds + L.red;
    double *Cs = lds + L.Cs, *ui = lds + L.ui, *uj = lds + L.uj, *ryi = lds + L.ryi, *ryj = lds + L.ryj, *ct = lds + L.ct, *gt = lds + L.gt;
    const TilePlace pl = tile_place(a, TC);
    const int bi = pl.bi, bj = pl.bj, nt = pl.nt;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, wave = tid >> 6, lane = tid & 63;
    const int64_t i0 = pl.i0, j0 = pl.j0, tbase = pl.tbase, n = a.n;

    stage_tile_inputs(a, pl, WiT, WjT);
    stage_test_points(a, pl, tm, tv, tz);

    const double wt = (bi == bj) ? 1.0 : 2.0;
    if (LOO) {
        if (tid < 64) ryi[tid] = i0 + tid < n ? a.ry[i0 + tid] : 0.0;
        else if (tid < 128) ryj[tid - 64] = j0 + tid - 64 < n ? a.ry[j0 + tid - 64] : 0.0;
        for (int idx = tid; idx < nt * 64; idx += 256) {
            const int t = idx >> 6, r = idx & 63;
            const double *u = a.Rinv + (int64_t)a.drop[tbase + t] * a.ldr;
            ui[idx] = i0 + r < n ? u[i0 + r] : 0.0;
            uj[idx] = j0 + r < n ? u[j0 + r] : 0.0;
        }
        if (tid < nt) {
            const int64_t d = a.drop[tbase + tid];
            const double rho = a.Rinv[d * a.ldr + d];
            ct[tid] = a.ry[d] / rho;
            gt[tid] = wt * a.scale / rho;
        }
    }
    // Cr: the pair weight (LOO: only its t-independent part wt scale Rinv_ij, subtracted per test point)
    double Cr[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t gi = i0 + ty + 16 * p;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t gj = j0 + tx + 16 * q;
            double c = 0.0;
            if (gi < n && gj < n)
                c = LOO ? wt * a.scale * a.Rinv[gi * a.ldr + gj] : wt * (a.ry[gi] * a.ry[gj] - a.scale * a.Rinv[gi * a.ldr + gj]);
            Cr[p][q] = c;
            if (KIND == DGPAMD_MATERN25) Cs[(ty + 16 * p) * 65 + tx + 16 * q] = c;
        }
    }
    __syncthreads();

    if (KIND == DGPAMD_SEXP) {
        // t-independent part of the exponent: sum_k (w_ik - w_jk)^2 / (2 l_k^2)  (= -log R2sexp, kernel_class.py:761-763)
        double base[4][4];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) base[p][q] = 0.0;
        for (int k = 0; k < Dw; ++k) {
            const double c2 = 1.0 / (2.0 * a.len[k] * a.len[k]);
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    double d = WiT[k * 64 + ty + 16 * p] - WjT[k * 64 + tx + 16 * q];
                    base[p][q] = fma(d * d, c2, base[p][q]);
                }
        }
        for (int t = 0; t < nt; ++t) {
            double e[4][4], ei[4], ej[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                ei[p] = 0.0;
                ej[p] = 0.0;
            }
            for (int g = 0; g < Dz; ++g) {
                const double il = 1.0 / a.len[Dw + g], zz = tz[t * Dz + g];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    double di = (WiT[(Dw + g) * 64 + ty + 16 * p] - zz) * il;
                    double dj = (WjT[(Dw + g) * 64 + tx + 16 * p] - zz) * il;
                    ei[p] = fma(di, di, ei[p]);
                    ej[p] = fma(dj, dj, ej[p]);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) e[p][q] = base[p][q] + ei[p] + ej[q];
            for (int k = 0; k < Dw; ++k) {
                const double l = a.len[k];
                const double c1 = 1.0 / (8.0 * tv[t * Dw + k] + 2.0 * l * l), m2 = 2.0 * tm[t * Dw + k];
                double wi[4], wj[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    wi[p] = WiT[k * 64 + ty + 16 * p] - m2;
                    wj[p] = WjT[k * 64 + tx + 16 * p];
                }
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        double sgm = wi[p] + wj[q];
                        e[p][q] = fma(sgm * sgm, c1, e[p][q]);
                    }
            }
            double acc = 0.0;
            if (LOO) {
                double ai[4], aj[4], gi_[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const double u1 = ui[t * 64 + ty + 16 * p], u2 = uj[t * 64 + tx + 16 * p];
                    ai[p] = wt * (ryi[ty + 16 * p] - ct[t] * u1);
                    aj[p] = ryj[tx + 16 * p] - ct[t] * u2;
                    gi_[p] = gt[t] * u1;
                    ej[p] = u2;
                }
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        acc = fma(fma(ai[p], aj[q], fma(gi_[p], ej[q], -Cr[p][q])), exp(-e[p][q]), acc);
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc = fma(Cr[p][q], exp(-e[p][q]), acc);
            }
            acc = wave_sum(acc);
            if (lane == 0) red[t * 4 + wave] = acc;
        }
    } else {
        for (int t = 0; t < nt; ++t) {
            double acc = 0.0;
#pragma unroll 1
            for (int e = 0; e < 16; ++e) {
                const int r = ty + 16 * (e >> 2), c = tx + 16 * (e & 3);
                double cij = Cs[r * 65 + c];
                if (LOO ? (i0 + r >= n || j0 + c >= n) : cij == 0.0) continue;
                if (LOO) {
                    const double u1 = ui[t * 64 + r], u2 = uj[t * 64 + c];
                    cij = fma(wt * (ryi[r] - ct[t] * u1), ryj[c] - ct[t] * u2, fma(gt[t] * u1, u2, -cij));
                }
                const bool diag = (i0 + r == j0 + c);
                double prod = 1.0;
                for (int k = 0; k < Dw; ++k) {
                    const double l = a.len[k], zm = tm[t * Dw + k], zv = tv[t * Dw + k];
                    const double xi = WiT[k * 64 + r], xj = WjT[k * 64 + c];
                    if (zv != 0.0)
                        prod *= diag ? matern_Jd0(xi, zm, zv, l) : matern_Jd(xj, xi, zm, zv, l);
                    else
                        prod *= matern_point(zm - xi, l) * matern_point(zm - xj, l);
                }
                double pi_ = 1.0, si = 0.0, pj = 1.0, sj = 0.0;
                for (int g = 0; g < Dz; ++g) {
                    const double il = 1.0 / a.len[Dw + g], zz = tz[t * Dz + g];
                    corr_accum_matern((WiT[(Dw + g) * 64 + r] - zz) * il, pi_, si);
                    corr_accum_matern((WjT[(Dw + g) * 64 + c] - zz) * il, pj, sj);
                }
                if (Dz) prod *= pi_ * pj * exp(-SQRT5 * (si + sj));
                acc = fma(cij, prod, acc);
            }
            acc = wave_sum(acc);
            if (lane == 0) red[t * 4 + wave] = acc;
        }
    }
    __syncthreads();
    store_partials(a, pl, red);
}

// one chunk of `mc` test points
int linkgp_launch_direct(dgpamd_ctx *ctx, const LinkArgs &a, const LinkPlan &p, int64_t mc) {
    void (*fn)(LinkArgs);
    if (a.kind == DGPAMD_SEXP)
        fn = p.loo ? linkgp_J_kernel<DGPAMD_SEXP, true> : linkgp_J_kernel<DGPAMD_SEXP, false>;
    else if (!p.loo)
        fn = linkgp_J_kernel<DGPAMD_MATERN25, false>;
    else
        fn = p.tc == TCH ? linkgp_J_kernel<DGPAMD_MATERN25, true> : linkgp_J_kernel<DGPAMD_MATERN25, true, TCH / 2>;
    int rc = set_lds(ctx, (const void *)fn, p.lds);
    if (rc) return rc;
    hipLaunchKernelGGL(fn, dim3(p.ntiles, (unsigned)((mc + p.tc - 1) / p.tc)), dim3(256), p.lds, ctx->stream, a);
    return DGPAMD_OK;
}
