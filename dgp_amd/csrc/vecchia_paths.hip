// Vecchia joint sample paths (DESIGN I.11): the nearest-neighbour factorisation of the joint predictive distribution of
// one GP node at M test rows taken in an order pi.  Position i of a path conditions on c(i), the min(m, n + i) nearest of
// the n training rows and the path's test rows at positions 0..i-1, in (distance, combined index) order; the combined
// index of training row j is j, that of test position i' is n + i'.  With A the correlation block over c(i) (diagonal
// 1 + nugget * omega_j on training members, 1 + nugget on test members) and a = k(c(i), u_i):
//   b_i = A^-1 a,   d_i = scale (1 + nugget - a^T b_i),   v_i = sum_train b_ij y_j + sum_test b_ij v_j + sqrt(d_i) z_i.
// dgpamd_vpaths_nn finds the sets, dgpamd_vpaths_rows emits each row in dgpamd_vecchia_spsolve's layout and the
// substitution is dgpamd_vecchia_levels + dgpamd_vecchia_spsolve_levels.
#include "common.hpp"
#include "vblock.hpp"
#include "vecchia_pred.hpp"

#include <climits>
#include <math.h>

// ---------------------------------------------------------------------------
// Neighbour search.  One wave per (path, position): the candidates are scanned 64 at a time (training rows first, then the
// earlier test rows, in combined-index order) and a candidate below the current m-th best is inserted into the sorted list
// the wave holds in registers -- entry k in lane k % 64 of slot k / 64 -- by one ballot (its rank) and one shift of the
// entries behind it.  Exact: the list is the brute-force (distance, index) order.
// ---------------------------------------------------------------------------
struct VPNnArgs {
    int64_t P, M, n;
    int D, m;
    const double *q, *x;
    const int32_t *group;
    int64_t *NN;
};

template <int R>
__global__ __launch_bounds__(256) void vpaths_nn_kernel(VPNnArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.P * a.M) return;   // (wave-uniform)
    const int D = a.D, m = a.m;
    const int64_t p = w / a.M, i = w - p * a.M, n = a.n;
    const int64_t g = a.group ? a.group[p] : 0;
    const double *qp = a.q + p * a.M * D, *xg = a.x + g * n * D, *qi = qp + i * D;
    double bd[R];
    int bi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        bd[r] = INFINITY;
        bi[r] = INT_MAX;
    }
    const int ws = (m - 1) >> 6, wl = (m - 1) & 63;   // slot and lane of entry m - 1
    double worst_d = INFINITY;
    int worst_i = INT_MAX;
    const int64_t nc = n + i;
    for (int64_t j0 = 0; j0 < nc; j0 += 64) {
        const int64_t j = j0 + lane;
        double s = INFINITY;
        if (j < nc) {
            const double *c = j < n ? xg + j * D : qp + (j - n) * D;
            s = 0.0;
            for (int d = 0; d < D; ++d) {
                const double df = c[d] - qi[d];
                s = fma(df, df, s);
            }
        }
        uint64_t mask = __ballot(j < nc && pair_less(s, (int)j, worst_d, worst_i));
        while (mask) {
            const int l = __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            const double cd = readlane_f64(s, l);
            const int ci = (int)(j0 + l);
            if (!pair_less(cd, ci, worst_d, worst_i)) continue;   // (uniform: the list moved on since the ballot)
            int pos = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) pos += __popcll(__ballot(pair_less(bd[r], bi[r], cd, ci)));
#pragma unroll
            for (int r = R - 1; r >= 0; --r) {
                double ud = __shfl_up(bd[r], 1, 64);
                int ui = __shfl_up(bi[r], 1, 64);
                if (r > 0) {
                    const double pd = readlane_f64(bd[r - 1], 63);
                    const int pi = __builtin_amdgcn_readlane(bi[r - 1], 63);
                    if (lane == 0) {
                        ud = pd;
                        ui = pi;
                    }
                }
                const int k = r * 64 + lane;
                if (k > pos) {
                    bd[r] = ud;
                    bi[r] = ui;
                } else if (k == pos) {
                    bd[r] = cd;
                    bi[r] = ci;
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r == ws) {
                    worst_d = readlane_f64(bd[r], wl);
                    worst_i = __builtin_amdgcn_readlane(bi[r], wl);
                }
        }
    }
    const int64_t k_valid = nc < m ? nc : m;
    int64_t *out = a.NN + w * m;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = r * 64 + lane;
        if (k < m) out[k] = k < k_valid ? (int64_t)bi[r] : -1;
    }
}

// ---------------------------------------------------------------------------
// Conditioning rows.  Output of row (p, i), in dgpamd_vecchia_spsolve's layout with unit scale:
//   Lrows[0] = 1 / sd,  NNl[0] = i;  then for each TEST member j of c(i), in list order: Lrows = -b_ij / sd, NNl = its test
//   position;  the rest 0 / -1.   t[p][r][i] = sum over TRAINING members of b_ij y_r[j];  sd[p][i] = sqrt(d_i).
// Then x_i = (rhs_i - sum_j Lrows_ij x_j) / Lrows_i0 with rhs_i = z_i + t_i / sd_i is the draw v_i of the header.
// ---------------------------------------------------------------------------
struct VPRowArgs {
    int D, m, nrhs;
    int64_t P, M, n;
    const double *q, *x, *omega, *y;
    const int32_t *group;
    const int64_t *NN;
    double nugget, jitter, scale;
    double *Lrows, *t, *sd;
    int64_t *NNl;
    int32_t *info;
};

// Register-resident (m <= VG_BC, D <= 16): the design of vecchia_gp_reg_kernel (csrc/vecchia_pred.hip) -- one wave per row,
// lane r holds row r of the block [c(i) ; u_i] (the test point in lane b), columns built by broadcasting a point's scaled
// coordinates, LDL^T elimination by broadcasting the pivot row entry by entry.  Afterwards lane r < b holds row r of
// U = D L^T and (L^-1 a)_r, lane b the Schur complement 1 + nugget - a^T A^-1 a; a back substitution over the lanes gives b_i.
template <int KIND, int DM>
__global__ __launch_bounds__(256) void vpaths_rows_reg_kernel(VPRowArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.P * a.M) return;   // (wave-uniform)
    const int m = a.m, D = a.D;
    const int64_t p = w / a.M, i = w - p * a.M, n = a.n;
    const int64_t g = a.group ? a.group[p] : 0;
    const double *qp = a.q + p * a.M * D, *xg = a.x + g * n * D;
    const int64_t nnv = lane < m ? a.NN[w * m + lane] : -1;
    const int b = __builtin_amdgcn_readfirstlane(__popcll(__ballot(nnv >= 0)));   // (the valid entries come first)
    const bool tr = lane < b && nnv < n, te = lane < b && nnv >= n;
    double xr[DM];
    {
        const double *src = tr ? xg + nnv * D : (te ? qp + (nnv - n) * D : qp + i * D);
#pragma unroll
        for (int d = 0; d < DM; ++d) xr[d] = (d < D && lane <= b) ? src[d] : 0.0;
    }
    const double dg = 1.0 + a.jitter + a.nugget * (tr && a.omega ? a.omega[nnv] : 1.0);
    double reg[VG_BC], last;
    vreg_fill(reg, last, b, [&](int c) {
        double s = 0.0, pr = 1.0;
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            const double df = xr[d] - readlane_f64(xr[d], c);
            if (KIND == DGPAMD_SEXP)
                corr_accum_sexp(df, s);
            else
                corr_accum_matern(df, pr, s);
        }
        const double v = (KIND == DGPAMD_SEXP) ? exp_negated(s) : pr * exp_negated(SQRT5 * s);
        return lane == c ? dg : v;
    });
    VPivotDivide pivot;
    vreg_eliminate(reg, last, b, lane, pivot);
    const double schur = readlane_f64(last, b);
    const bool bad = pivot.bad || !(schur > 0.0);
    const double coef = vreg_backsolve(reg, last, b, lane);   // b_i = U^-1 (L^-1 a)
    const double sdv = sqrt(a.scale * schur);
    for (int r = 0; r < a.nrhs; ++r) {
        const double tv = wave_sum_all(tr ? coef * a.y[(g * a.nrhs + r) * n + nnv] : 0.0);
        if (lane == 0) a.t[(p * a.nrhs + r) * a.M + i] = tv;
    }
    const uint64_t tmask = __ballot(te);
    const int nte = __popcll(tmask);
    double *Lr = a.Lrows + w * (m + 1);
    int64_t *Nr = a.NNl + w * (m + 1);
    const double isd = 1.0 / sdv;
    if (lane == 0) {
        Lr[0] = isd;
        Nr[0] = i;
        a.sd[w] = sdv;
        if (bad) atomicCAS(a.info, 0, (int32_t)(w + 1));
    }
    if (te) {
        const int slot = 1 + __popcll(tmask & ((1ull << lane) - 1ull));
        Lr[slot] = -coef * isd;
        Nr[slot] = nnv - n;
    }
    if (lane >= 1 + nte && lane <= m) {
        Lr[lane] = 0.0;
        Nr[lane] = -1;
    }
}

// The same rows with the block in LDS (any m whose block fits a CU's LDS, D <= DGPAMD_MAXD): one wave per row, a
// right-looking Cholesky of [c(i) ; u_i], then b_i = L11^-T l21 and d_i = scale * l22^2.
static inline size_t vpaths_rows_lds_bytes(int m, int D) {
    const size_t mp1 = (size_t)m + 1, lda = (size_t)m + 2;
    return (mp1 * lda + mp1 * D + lda) * sizeof(double) + mp1 * sizeof(int64_t);
}

template <int KIND>
__global__ __launch_bounds__(64) void vpaths_rows_lds_kernel(VPRowArgs a) {
    extern __shared__ double lds[];
    const int m = a.m, D = a.D, lda = m + 2, lane = threadIdx.x;
    double *A = lds;                          // [m+1][lda] lower triangle of the block
    double *xs = A + (m + 1) * lda;           // [m+1][D] scaled coordinates
    double *V = xs + (m + 1) * D;             // [lda] b_i
    int64_t *idx = reinterpret_cast<int64_t *>(V + lda);   // [m+1]
    const int64_t w = blockIdx.x;
    const int64_t p = w / a.M, i = w - p * a.M, n = a.n;
    const int64_t g = a.group ? a.group[p] : 0;
    const double *qp = a.q + p * a.M * D, *xg = a.x + g * n * D;
    const int b = load_nn<false>(a.NN + w * m, m, idx, lane);
    __syncthreads();
    for (int e = lane; e < (b + 1) * D; e += 64) {
        const int r = e / D, d = e - r * D;
        const int64_t v = r < b ? idx[r] : -1;
        xs[e] = r == b ? qp[i * D + d] : (v < n ? xg[v * D + d] : qp[(v - n) * D + d]);
    }
    __syncthreads();
    const int bb = b + 1;
    fill_lower<KIND, VExpFast>(A, lda, bb, xs, D, 1.0,
                               [&](int r) { return 1.0 + a.jitter + a.nugget * (r < b && idx[r] < n && a.omega ? a.omega[idx[r]] : 1.0); }, lane);
    const int bad = lds_chol(A, lda, bb, bb, lane);
    for (int c = lane; c < b; c += 64) V[c] = A[b * lda + c];   // l21 = L11^-1 a
    lds_backsolve_T(A, lda, b, V, lda, 1, lane);              // V <- L11^-T V
    const double l22 = A[b * lda + b];
    const double sdv = sqrt(a.scale) * l22, isd = 1.0 / sdv;
    for (int r = 0; r < a.nrhs; ++r) {
        double s = 0.0;
        for (int c = lane; c < b; c += 64)
            if (idx[c] < n) s = fma(V[c], a.y[(g * a.nrhs + r) * n + idx[c]], s);
        s = wave_sum_all(s);
        if (lane == 0) a.t[(p * a.nrhs + r) * a.M + i] = s;
    }
    if (lane == 0) {
        double *Lr = a.Lrows + w * (m + 1);
        int64_t *Nr = a.NNl + w * (m + 1);
        Lr[0] = isd;
        Nr[0] = i;
        int slot = 1;
        for (int c = 0; c < b; ++c)
            if (idx[c] >= n) {
                Lr[slot] = -V[c] * isd;
                Nr[slot] = idx[c] - n;
                ++slot;
            }
        for (; slot <= m; ++slot) {
            Lr[slot] = 0.0;
            Nr[slot] = -1;
        }
        a.sd[w] = sdv;
        if (bad) atomicCAS(a.info, 0, (int32_t)(w + 1));
    }
}

extern "C" int dgpamd_vpaths_nn(dgpamd_ctx *ctx, int64_t P, int64_t M, int64_t n, int D, int m, const double *q,
                                const double *x, const int32_t *group, int64_t *NN) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (P <= 0 || M <= 0 || n <= 0 || D <= 0 || D > DGPAMD_MAXD || m < 1 || !q || !x || !NN) BAD_ARG(ctx, "bad arguments");
    if (m > 256) BAD_ARG(ctx, "conditioning sets of more than 256 points");
    if (n + M > INT_MAX) BAD_ARG(ctx, "more than 2^31 - 1 candidate rows");
    VPNnArgs a{P, M, n, D, m, q, x, group, NN};
    const unsigned grid = (unsigned)((P * M + 3) / 4);
    if (m <= 64)
        hipLaunchKernelGGL(vpaths_nn_kernel<1>, dim3(grid), dim3(256), 0, ctx->stream, a);
    else if (m <= 128)
        hipLaunchKernelGGL(vpaths_nn_kernel<2>, dim3(grid), dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(vpaths_nn_kernel<4>, dim3(grid), dim3(256), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_vpaths_rows(dgpamd_ctx *ctx, int kind, int64_t P, int64_t M, int64_t n, int D, int m, int nrhs,
                                  const double *q, const double *x, const int32_t *group, const int64_t *NN,
                                  const double *omega, const double *y, double scale, double nugget, double jitter,
                                  double *Lrows, int64_t *NNl, double *t, double *sd, int32_t *info) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) BAD_ARG(ctx, "kind must be 0 or 1");
    if (P <= 0 || M <= 0 || n <= 0 || D <= 0 || D > DGPAMD_MAXD || m < 1 || nrhs < 1 || !q || !x || !NN || !y || !Lrows ||
        !NNl || !t || !sd || !info)
        BAD_ARG(ctx, "bad arguments");
    VPRowArgs a;
    a.D = D; a.m = m; a.nrhs = nrhs; a.P = P; a.M = M; a.n = n; a.q = q; a.x = x; a.omega = omega; a.y = y; a.group = group;
    a.NN = NN; a.nugget = nugget; a.jitter = jitter; a.scale = scale; a.Lrows = Lrows; a.t = t; a.sd = sd; a.NNl = NNl;
    a.info = info;
    HIP_TRY(ctx, hipMemsetAsync(info, 0, sizeof(int32_t), ctx->stream));
    if (m > VG_BC || D > 16 || ctx->tune.vecchia_lds)
        return launch_by_kind(ctx, kind, vpaths_rows_lds_kernel<DGPAMD_SEXP>, vpaths_rows_lds_kernel<DGPAMD_MATERN25>, dim3((unsigned)(P * M)),
                              dim3(64), vpaths_rows_lds_bytes(m, D), a, q);
    const dim3 grid4((unsigned)((P * M + 3) / 4));
    if (D <= 8)
        return launch_by_kind(ctx, kind, vpaths_rows_reg_kernel<DGPAMD_SEXP, 8>, vpaths_rows_reg_kernel<DGPAMD_MATERN25, 8>, grid4, dim3(256), 0, a, q);
    return launch_by_kind(ctx, kind, vpaths_rows_reg_kernel<DGPAMD_SEXP, 16>, vpaths_rows_reg_kernel<DGPAMD_MATERN25, 16>, grid4, dim3(256), 0, a, q);
}
