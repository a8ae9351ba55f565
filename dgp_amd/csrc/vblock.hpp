// The conditioning block of the Vecchia kernels, every shared step written once: the correlation of two scaled points, the
// neighbour-list load, the lower-triangle fill, the in-LDS Cholesky and back substitution (one wave per block), and the
// register-resident block (one row per lane) with its column fill, its LDL^T elimination and the link_gp kernels' Gauss-Jordan finish.  Everything here is forced
// inline, as in wave.hpp: a kernel that uses one compiles to what it did with a copy of its own.
#pragma once
#include "common.hpp"
#include "vecchia_pred.hpp"
#include "wave.hpp"

#include <math.h>

#define VW 64   // threads per item (one wave)

// exp(-x) and exp(-sqrt5 x), x >= 0, as a template parameter: every kernel keeps the exponential it was written with (other
// bits), down to the expression (the Matern kernels compile to other instructions with exp(-(SQRT5 * x)) for exp(-SQRT5 * x))
struct VExpLib {    // the device library's
    static __device__ __forceinline__ double neg(double x) { return exp(-x); }
    static __device__ __forceinline__ double neg_sqrt5(double x) { return exp(-SQRT5 * x); }
};
struct VExpFast {   // exp_negated: full-rate instructions only
    static __device__ __forceinline__ double neg(double x) { return exp_negated(x); }
    static __device__ __forceinline__ double neg_sqrt5(double x) { return exp_negated(SQRT5 * x); }
};

// correlation of two SCALED points
template <int KIND, class EXP>
__device__ __forceinline__ double corr_pts(const double *xa, const double *xb, int D) {
    double s = 0.0, pr = 1.0;
    for (int d = 0; d < D; ++d) {
        double df = xa[d] - xb[d];
        if (KIND == DGPAMD_SEXP)
            corr_accum_sexp(df, s);
        else
            corr_accum_matern(df, pr, s);
    }
    return (KIND == DGPAMD_SEXP) ? EXP::neg(s) : pr * EXP::neg_sqrt5(s);
}

// The valid entries of a neighbour row (they come first, -1 padded) into LDS, in the row's order or REVersed (the ordered
// arrays are index-descending: reversed is ascending, self last); returns their number
template <bool REV, class I>
__device__ __forceinline__ int load_nn(const int64_t *row, int len, I *idx, int lane) {
    int b = 0;
    for (int a = 0; a < len; ++a) b += (row[a] >= 0);
    for (int a = lane; a < b; a += VW) idx[a] = (I)row[REV ? b - 1 - a : a];
    return b;
}

// Lower triangle of the nb x nb block over the scaled points xs[nb][D] (the lower triangle only: no idle lanes):
// diag(r) on the diagonal, offscale * correlation below it
template <int KIND, class EXP, class DIAG>
__device__ __forceinline__ void fill_lower(double *A, int lda, int nb, const double *xs, int D, double offscale, DIAG diag, int lane) {
    for (int e = lane; e < nb * (nb + 1) / 2; e += VW) {
        int r, c;
        tri_decode(e, r, c);
        A[r * lda + c] = r == c ? diag(r) : offscale * corr_pts<KIND, EXP>(xs + r * D, xs + c * D, D);
    }
}

// In-LDS right-looking Cholesky of the leading npiv columns of a `rows` x `rows` lower matrix (ld = lda).
// Rows beyond npiv are carried (right-hand sides / prediction rows).  Returns 0 or 1+index of a bad pivot.
__device__ __forceinline__ int lds_chol(double *A, int lda, int rows, int npiv, int lane) {
    int bad = 0;
    for (int j = 0; j < npiv; ++j) {
        __syncthreads();
        double d = A[j * lda + j];
        if (!(d > 0.0)) {
            if (!bad) bad = j + 1;
            d = 1.0;
        }
        const double sd = sqrt(d), inv = 1.0 / sd;
        __syncthreads();
        for (int r = j + 1 + lane; r < rows; r += VW) A[r * lda + j] *= inv;
        if (lane == 0) A[j * lda + j] = sd;
        __syncthreads();
        for (int r = j + 1 + lane; r < rows; r += VW) {
            const double lr = A[r * lda + j];
            const int cmax = r < rows ? r : rows - 1;
            for (int c = j + 1; c <= cmax; ++c) A[r * lda + c] = fma(-lr, A[c * lda + j], A[r * lda + c]);
        }
    }
    __syncthreads();
    return bad;
}

// x <- L^-T x for nrhs vectors stored as rows X[q][.] (ld = ldx); column-oriented back substitution
__device__ __forceinline__ void lds_backsolve_T(const double *L, int lda, int b, double *X, int ldx, int nrhs, int lane) {
    for (int c = b - 1; c >= 0; --c) {
        __syncthreads();
        if (lane < nrhs) X[lane * ldx + c] /= L[c * lda + c];
        __syncthreads();
        for (int q = 0; q < nrhs; ++q) {
            const double xc = X[q * ldx + c];
            for (int r = lane; r < c; r += VW) X[q * ldx + r] = fma(-L[c * lda + r], xc, X[q * ldx + r]);
        }
    }
    __syncthreads();
}

// ---- the block in registers: one wave per block, lane r holds row r, its point's scaled coordinates in xr[] ----
// (The column's correlations stay in each kernel's own `column`: moved into a function here, the Matern instances of both
//  kernels came out with another register allocation -- 139 / 155 VGPRs for 147 / 179 -- and ran 2 % slower.)
// reg[c] = column(c) for the b leading columns (zeros beyond), last = column(b)
// (static_for: every reg[] index is a compile-time constant -- left to `#pragma unroll` the compiler keeps the loops and the
//  array goes to scratch)
template <int BC, class COL>
__device__ __forceinline__ void vreg_fill(double (&reg)[BC], double &last, const int b, COL column) {
    static_for<0, BC>([&](auto ic) {
        constexpr int c = decltype(ic)::value;
        reg[c] = 0.0;
        if (c < b) reg[c] = column(c);
    });
    last = column(b);
}

// The pivot's reciprocal, as each kernel takes it
struct VPivotNewton {   // hardware estimate + two Newton rounds, pivots not checked
    __device__ __forceinline__ double rcp(double d) { return rcp_newton(d); }
};
struct VPivotDivide {   // division; remembers a pivot that is not positive
    bool bad = false;
    __device__ __forceinline__ double rcp(double d) {
        bad = bad || !(d > 0.0);
        return 1.0 / d;
    }
};

// LDL^T elimination of the b leading columns: pivot j's row is broadcast entry by entry, reg[c] -= (reg[j] / d_j) * A[j][c] for
// the rows below j, and `last` (the column behind the block) takes the same row operations.  Columns beyond b hold zeros
// and stay zero: skipped in groups of eight.
template <int BC, class PIVOT>
__device__ __forceinline__ void vreg_eliminate(double (&reg)[BC], double &last, const int b, const int lane, PIVOT &pivot) {
    static_for<0, BC>([&](auto ij) {
        constexpr int j = decltype(ij)::value;
        if (j < b) {
            const double rd = pivot.rcp(readlane_f64(reg[j], j));
            const double mi = lane > j ? reg[j] * rd : 0.0;
            static_for<(j + 1) / 8, (BC + 7) / 8>([&](auto ig) {
                constexpr int c0 = 8 * decltype(ig)::value;
                if (c0 < b) {
                    static_for<0, 8>([&](auto iq) {
                        constexpr int c = c0 + decltype(iq)::value;
                        if constexpr (c > j && c < BC) reg[c] = fma(-mi, readlane_f64(reg[c], j), reg[c]);
                    });
                }
            });
            last = fma(-mi, readlane_f64(last, j), last);
        }
    });
}

// After vreg_eliminate lane r < b holds row r of U = D L^T in reg[] and (L^-1 a)_r in `last`.  Returns, in lane j < b, entry j
// of U^-1 (L^-1 a) = A^-1 a (0 in the lanes beyond): back substitution over the lanes, pivot j broadcast from lane j.
template <int BC>
__device__ __forceinline__ double vreg_backsolve(const double (&reg)[BC], const double last, const int b, const int lane) {
    double coef = 0.0, res = lane < b ? last : 0.0;
    static_for<0, BC>([&](auto ik) {
        constexpr int j = BC - 1 - decltype(ik)::value;
        if (j < b) {
            const double xj = readlane_f64(res, j) / readlane_f64(reg[j], j);
            coef = lane == j ? xj : coef;
            res = lane < j ? fma(-reg[j], xj, res) : res;
        }
    });
    return coef;
}

// The second half of both register-resident link_gp kernels: Gauss-Jordan elimination of K | N with J, y and I riding along, then
// the mean and the variance (see the squared-exponential kernel, csrc/vecchia_pred_link_sexp.hip, for the algebra).
__device__ __forceinline__ void linkgp_reg_finish(double (&reg)[VL_BC], double (&jm)[VL_BC], double yv, double Iv, const bool act,
                                                  const int b, const int lane, const VLinkArgs &a, const int64_t t) {
    // elimination: rows below the pivot take  row_i -= (a_ij / d_j) row_j  in K | N, in J, in y and in I
    double dmine = 1.0;
    static_for<0, VL_BC>([&](auto ij) {
        constexpr int j = decltype(ij)::value;
        if (j < b) {
            const double d = readlane_f64(reg[j], j);
            dmine = lane == j ? d : dmine;
            const double rd = rcp_newton(d);
            const double mi = (lane > j && act) ? reg[j] * rd : 0.0;
            static_for<0, (VL_BC + 7) / 8>([&](auto ig) {
                constexpr int c0 = 8 * decltype(ig)::value;
                if (c0 < b) {
                    static_for<0, 8>([&](auto iq) {
                        constexpr int c = c0 + decltype(iq)::value;
                        if constexpr (c < VL_BC) {
                            if constexpr (c != j) reg[c] = fma(-mi, readlane_f64(reg[c], j), reg[c]);
                            jm[c] = fma(-mi, readlane_f64(jm[c], j), jm[c]);
                        }
                    });
                }
            });
            reg[j] = lane > j ? -mi : reg[j];
            yv = fma(-mi, readlane_f64(yv, j), yv);
            Iv = fma(-mi, readlane_f64(Iv, j), Iv);
        }
    });
    const double rdi = act ? rcp_newton(dmine) : 0.0;
    const double v = yv * rdi;
    // t = L^-T v (column sums of N scaled by v), then the lane's share of v . (M t) and of the trace
    double mt = 0.0, trp = 0.0;
    static_for<0, VL_BC>([&](auto ic) {
        constexpr int c = decltype(ic)::value;
        if (c < b) {
            const double nic = lane > c ? reg[c] : (lane == c ? 1.0 : 0.0);
            const double tc = wave_sum_all(act ? nic * v : 0.0);
            mt = fma(jm[c], tc, mt);
            trp = fma(jm[c], nic, trp);
        }
    });
    const double mu = wave_sum_all(Iv * v), qd = wave_sum_all(v * mt), tr = wave_sum_all(trp * rdi);
    if (lane == 0) {
        a.mean[t] = mu;
        a.var[t] = fabs(qd - mu * mu + a.scale * (1.0 + a.nugget - tr));
    }
}
