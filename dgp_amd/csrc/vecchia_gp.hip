// Vecchia predictions (reference dgpsi/vecchia.py:635-907): the host entries and the kernels that hold
// the conditioning block in LDS (csrc/vblock.hpp), one wave per test point.  The register-resident kernels the entries
// prefer are csrc/vecchia_pred.hip and csrc/vecchia_pred_link_*.hip.
#include "common.hpp"
#include "linkfun.hpp"
#include "vblock.hpp"
#include "vecchia_pred.hpp"

#include <math.h>

// ---------------------------------------------------------------------------
// a22  gp_vecch (vecchia.py:635-654): block = [pm neighbours ; test point], rhs row y
// ---------------------------------------------------------------------------

template <int KIND>
__global__ __launch_bounds__(VW) void vecchia_gp_kernel(VGpArgs a) {
    extern __shared__ double lds[];
    const int pm = a.pm, D = a.vp.D, lda = pm + 3;
    double *A = lds;                       // [(pm+2)][lda]
    double *xs = A + (pm + 2) * lda;       // [pm+1][D]
    int *idx = reinterpret_cast<int *>(xs + (pm + 1) * D);
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int b = load_nn<false>(a.NN + t * pm, pm, idx, lane);
    __syncthreads();
    for (int e = lane; e < (b + 1) * D; e += VW) {
        int r = e / D, d = e - r * D;
        xs[e] = (r < b ? a.w[(int64_t)idx[r] * D + d] : a.x[t * D + d]) * a.vp.inv_len[d];
    }
    __syncthreads();
    const int bb = b + 1;
    fill_lower<KIND, VExpLib>(A, lda, bb, xs, D, 1.0, [&](int r) { return 1.0 + a.vp.nugget * (r < b ? a.nugget_diag[idx[r]] : 1.0); }, lane);
    for (int c = lane; c <= bb; c += VW) A[bb * lda + c] = c < b ? a.y[idx[c]] : 0.0;
    lds_chol(A, lda, bb + 1, b, lane);
    if (lane == 0) {
        // after eliminating the b neighbour columns: Schur complement of the test point and -l21.w
        a.mean[t] = -A[bb * lda + b];
        a.var[t] = a.scale * A[b * lda + b];
    }
}

extern "C" int dgpamd_vecchia_gp(dgpamd_ctx *ctx, int kind, int64_t M, int64_t n, int D, int pm, const double *x,
                                 const double *w, const int64_t *NN, const double *y, double scale,
                                 const double *length_h, int nlen, double nugget, const double *nugget_diag,
                                 double *mean, double *var) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (M <= 0 || n <= 0 || pm <= 0 || !x || !w || !NN || !y || !nugget_diag || !mean || !var) BAD_ARG(ctx, "bad arguments");
    VGpArgs a;
    int rc = fill_vparams(ctx, a.vp, kind, D, length_h, nlen, nugget);
    if (rc) return rc;
    a.M = M; a.n = n; a.pm = pm; a.x = x; a.w = w; a.y = y; a.nugget_diag = nugget_diag; a.NN = NN; a.scale = scale;
    a.mean = mean; a.var = var;
    {
        if (pm <= VG_BC && D <= 16 && !ctx->tune.vecchia_lds) {   // (DGPAMD_VECCHIA_LDS=1: the LDS version for every size -- the tests compare the two)
            launch_vecchia_gp_reg(ctx, a);
            LAUNCH_CHECK(ctx);
            return DGPAMD_OK;
        }
    }
    const size_t shm = ((size_t)(pm + 2) * (pm + 3) + (size_t)(pm + 1) * D) * sizeof(double) + (size_t)pm * sizeof(int);
    return launch_by_kind(ctx, kind, vecchia_gp_kernel<DGPAMD_SEXP>, vecchia_gp_kernel<DGPAMD_MATERN25>, dim3((unsigned)M), dim3(VW), shm, a, a.x);
}

// ---------------------------------------------------------------------------
// a23  link_gp_vecch (vecchia.py:758-796) with IJ_nb (vecchia.py:838-907)
// ---------------------------------------------------------------------------


#define VREC 29   // doubles per separable Matern record of a neighbour in LDS (28 used; odd stride)
template <int KIND>
__global__ __launch_bounds__(VW) void vecchia_linkgp_kernel(VLinkArgs a) {
    extern __shared__ double lds[];
    const int pm = a.pm, Dw = a.Dw, Dz = a.Dz, DT = Dw + Dz, lda = pm + 2;
    double *A = lds;                      // [(pm+1)][lda]   K block + rhs row y
    double *J = A + (pm + 1) * lda;       // [pm][lda]       J, then L^-1 J, then L^-1 (L^-1 J)^T
    double *xs = J + pm * lda;            // [pm][DT]        raw (unscaled) neighbour inputs
    double *Iv = xs + pm * DT;            // [pm]
    double *Ry = Iv + pm;                 // [lda]
    int *idx = reinterpret_cast<int *>(Ry + lda);
    const int lane = threadIdx.x;
    const int64_t t = blockIdx.x;
    const int b = load_nn<false>(a.NN + t * pm, pm, idx, lane);
    __syncthreads();
    for (int e = lane; e < b * DT; e += VW) {
        int r = e / DT, d = e - r * DT;
        xs[e] = d < Dw ? a.w1[(int64_t)idx[r] * Dw + d] : a.wg[(int64_t)idx[r] * Dz + d - Dw];
    }
    __syncthreads();
    const double *mt = a.m + t * Dw, *vt = a.v + t * Dw;
    const double *zt = Dz ? a.z + t * Dz : nullptr;
    // I and the global-input factor
    for (int r = lane; r < b; r += VW) {
        double I, Iz = 1.0;
        if (KIND == DGPAMD_SEXP) {
            double e = 0.0, c1 = 1.0;
            for (int k = 0; k < Dw; ++k) {
                double l = a.len[k], d = xs[r * DT + k] - mt[k];
                e += d * d / (2.0 * vt[k] + l * l);
                c1 *= 1.0 + 2.0 * vt[k] / (l * l);
            }
            I = exp(-e) / sqrt(c1);
            double s = 0.0;
            for (int g = 0; g < Dz; ++g) {
                double d = (xs[r * DT + Dw + g] - zt[g]) / a.len[Dw + g];
                s = fma(d, d, s);
            }
            if (Dz) Iz = exp(-s);
        } else {
            I = 1.0;
            for (int k = 0; k < Dw; ++k) I *= matern_I_dim(xs[r * DT + k], mt[k], vt[k], a.len[k]);
            double pr = 1.0, s = 0.0;
            for (int g = 0; g < Dz; ++g) corr_accum_matern((xs[r * DT + Dw + g] - zt[g]) / a.len[Dw + g], pr, s);
            if (Dz) Iz = pr * exp(-SQRT5 * s);
        }
        Iv[r] = I * Iz;
        Ry[r] = Iz;   // park the global factor
    }
    __syncthreads();
    // K block (all DT columns) and J (local columns, times the global factors)
    double jc1 = 1.0;
    if (KIND == DGPAMD_SEXP) {
        for (int k = 0; k < Dw; ++k) jc1 *= 1.0 + 4.0 * vt[k] / (a.len[k] * a.len[k]);
        jc1 = 1.0 / sqrt(jc1);
    }
    for (int e = lane; e < b * (b + 1) / 2; e += VW) {   // the lower triangle only (over b * b with the upper half skipped, half the lanes idled)
        int r, c;
        tri_decode(e, r, c);
        double s = 0.0, pr = 1.0;
        for (int d = 0; d < DT; ++d) {
            double df = (xs[r * DT + d] - xs[c * DT + d]) / a.len[d];
            if (KIND == DGPAMD_SEXP)
                corr_accum_sexp(df, s);
            else
                corr_accum_matern(df, pr, s);
        }
        double kv = (KIND == DGPAMD_SEXP) ? exp(-s) : pr * exp(-SQRT5 * s);
        if (r == c) kv = 1.0 + a.nugget * a.nugget_diag[idx[r]];
        A[r * lda + c] = kv;
        double jv;
        if (KIND == DGPAMD_SEXP) {
            double ex = 0.0;
            for (int k = 0; k < Dw; ++k) {
                double l = a.len[k], ai = xs[r * DT + k] - mt[k], aj = xs[c * DT + k] - mt[k];
                ex += (ai + aj) * (ai + aj) / (8.0 * vt[k] + 2.0 * l * l) + (ai - aj) * (ai - aj) / (2.0 * l * l);
            }
            jv = jc1 * exp(-ex);
        } else {
            jv = 1.0;   // (the Matern factors follow dimension by dimension, below)
        }
        jv *= Ry[r] * Ry[c];
        J[r * lda + c] = jv;
        J[c * lda + r] = jv;
    }
    if (KIND != DGPAMD_SEXP) {
        // Matern-2.5 J factors through the separable form of csrc/linkfun.hpp (Jd = <S(x_lo), T(x_hi)> + (f2_hi - f2_lo) <S', T'>):
        // per dimension every neighbour's record (S[0..11] T[12..26] f2[27], ~500 instructions of erf / exp) is evaluated ONCE,
        // and a pair costs 30 multiply-adds and a select instead of matern_Jd's 3 erf + 5 exp -- with 50 neighbours 1275 pairs
        // share 50 records.  (A dimension with zero input variance has S[0] = T[0] = k(x, m), the rest zero: the product of the
        // two point correlations, functions.py:488-491.)
        double *rec = reinterpret_cast<double *>(idx + ((pm + 1) & ~1));   // [pm][VREC], behind idx (the launch sizes the LDS for it)
        for (int k = 0; k < Dw; ++k) {
            __syncthreads();
            {
                for (int r = lane; r < b; r += VW) {
                    double *rr = rec + r * VREC;
                    const double x = xs[r * DT + k];
                    if (vt[k] != 0.0) {
                        MaternDimConst kc;
                        matern_dim_const(mt[k], vt[k], a.len[k], kc);
                        double f2, so[12], to[15];
                        matern_role_S(x, kc, so, f2);
                        matern_role_T(x, kc, to);
                        for (int q = 0; q < 12; ++q) rr[q] = so[q];
                        for (int q = 0; q < 15; ++q) rr[12 + q] = to[q];
                        rr[27] = f2;
                    } else {
                        const double pt = matern_point(mt[k] - x, a.len[k]);
                        for (int q = 0; q < 28; ++q) rr[q] = 0.0;
                        rr[0] = pt;
                        rr[12] = pt;
                    }
                }
            }
            __syncthreads();
            for (int e = lane; e < b * (b + 1) / 2; e += VW) {
                int r, c;
                tri_decode(e, r, c);
                const double *ri = rec + r * VREC, *rj = rec + c * VREC;
                const double xi = xs[r * DT + k], xj = xs[c * DT + k];
                const double *lo = xi <= xj ? ri : rj, *hi = xi <= xj ? rj : ri;   // the record of the smaller / larger coordinate
                double o = 0.0, ed = 0.0;
                for (int q = 0; q < 12; ++q) o = fma(lo[q], hi[12 + q], o);
                for (int q = 0; q < 3; ++q) ed = fma(lo[6 + q], hi[24 + q], ed);
                const double f = fma(hi[27] - lo[27], ed, o);
                J[r * lda + c] *= f;
            }
        }
        __syncthreads();
        for (int e = lane; e < b * (b + 1) / 2; e += VW) {
            int r, c;
            tri_decode(e, r, c);
            J[c * lda + r] = J[r * lda + c];
        }
    }
    for (int c = lane; c <= b; c += VW) A[b * lda + c] = c < b ? a.y[idx[c]] : 0.0;
    lds_chol(A, lda, b + 1, b, lane);
    // Rinv_y = L^-T w
    for (int c = lane; c < b; c += VW) Ry[c] = A[b * lda + c];
    lds_backsolve_T(A, lda, b, Ry, lda, 1, lane);
    // mean and Ry^T J Ry on the untouched J
    double mu = 0.0, qd = 0.0;
    for (int r = lane; r < b; r += VW) {
        mu = fma(Iv[r], Ry[r], mu);
        double s = 0.0;
        for (int c = 0; c < b; ++c) s = fma(J[r * lda + c], Ry[c], s);
        qd = fma(Ry[r], s, qd);
    }
    mu = wave_sum_all(mu);
    qd = wave_sum_all(qd);
    __syncthreads();
    // tr(K^-1 J) = tr(L^-1 (L^-1 J)^T): two rounds of column-parallel forward substitutions
    for (int c = lane; c < b; c += VW)
        for (int r = 0; r < b; ++r) {
            double s = J[r * lda + c];
            for (int k = 0; k < r; ++k) s = fma(-A[r * lda + k], J[k * lda + c], s);
            J[r * lda + c] = s / A[r * lda + r];
        }
    __syncthreads();
    double tr = 0.0;
    for (int c = lane; c < b; c += VW) {
        // column c of G^T is row c of G; solve L h = G[c,:]^T and keep h_c
        double hc = 0.0;
        for (int r = 0; r <= c; ++r) {
            double s = J[c * lda + r];
            for (int k = 0; k < r; ++k) s = fma(-A[r * lda + k], J[c * lda + k], s);
            s /= A[r * lda + r];
            J[c * lda + r] = s;   // row c is private to this lane from here on
            hc = s;
        }
        tr += hc;
    }
    tr = wave_sum_all(tr);
    if (lane == 0) {
        a.mean[t] = mu;
        a.var[t] = fabs(qd - mu * mu + a.scale * (1.0 + a.nugget - tr));
    }
}

extern "C" int dgpamd_vecchia_linkgp(dgpamd_ctx *ctx, int kind, int64_t M, int64_t n, int Dw, int Dz, int pm,
                                     const double *m, const double *v, const double *z, const double *w1,
                                     const double *wg, const int64_t *NN, const double *y, double scale,
                                     const double *length_h, int nlen, double nugget, const double *nugget_diag,
                                     double *mean, double *var) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (M <= 0 || n <= 0 || pm <= 0 || !m || !v || !w1 || !NN || !y || !nugget_diag || !mean || !var || !length_h)
        BAD_ARG(ctx, "bad arguments");
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) BAD_ARG(ctx, "kind must be 0 or 1");
    if (Dw <= 0 || Dz < 0 || Dw + Dz > DGPAMD_MAXD || (nlen != 1 && nlen != Dw + Dz)) BAD_ARG(ctx, "bad dimensions");
    if (Dz > 0 && (!z || !wg)) BAD_ARG(ctx, "Dz > 0 needs z and wg");
    VLinkArgs a;
    a.kind = kind; a.Dw = Dw; a.Dz = Dz; a.pm = pm; a.M = M; a.n = n; a.m = m; a.v = v; a.z = z; a.w1 = w1; a.wg = wg;
    a.y = y; a.nugget_diag = nugget_diag; a.NN = NN; a.scale = scale; a.nugget = nugget; a.mean = mean; a.var = var;
    for (int d = 0; d < Dw + Dz; ++d) a.len[d] = length_h[nlen == 1 ? 0 : d];
    {
        if (pm <= VL_BC && Dw <= 8 && Dz <= 8 && !ctx->tune.vecchia_lds) {   // (DGPAMD_VECCHIA_LDS=1: the LDS version for every size -- the tests compare the two)
            if (kind == DGPAMD_SEXP)
                launch_vecchia_linkgp_sexp_reg(ctx, a);
            else
                launch_vecchia_linkgp_matern_reg(ctx, a);
            LAUNCH_CHECK(ctx);
            return DGPAMD_OK;
        }
    }
    const int lda = pm + 2;
    const size_t shm = ((size_t)(pm + 1) * lda + (size_t)pm * lda + (size_t)pm * (Dw + Dz) + pm + lda) * sizeof(double) +
                       (size_t)((pm + 1) & ~1) * sizeof(int) + (kind == DGPAMD_SEXP ? 0 : (size_t)pm * VREC * sizeof(double));
    return launch_by_kind(ctx, kind, vecchia_linkgp_kernel<DGPAMD_SEXP>, vecchia_linkgp_kernel<DGPAMD_MATERN25>, dim3((unsigned)M), dim3(VW), shm,
                          a, a.y);
}
