// Function-valued posterior draws by local conditioning (emulator.sample_functions_vecchia, gp.sample_functions_vecchia;
// DESIGN I.14): the pathwise update of a draw through the Vecchia predictor.  One GP node, R rows; row i has the conditioning
// set N(i), its b <= pm nearest training rows (NN: valid entries first, -1 padded).  With A the correlation block over N(i),
// diagonal 1 + jitter + nugget * omega_j, and a = c(W_N, x_i):
//   b_i = A^-1 a,    out = sqrt(scale) (prior + sum_j b_ij r[N_j]),
// r the path's residual y / sqrt(scale) - Phi(W) theta - sqrt(nugget omega) * eps and prior its random-Fourier-feature part at
// unit scale (dgpamd_pathfun_eval with n = 0).  All coordinates arrive divided by the lengthscales.
//   shared rows   (rows_per_path == 0: a first-layer node, a gp)  every row serves all P paths: the block is factored once
//       per row and applied with the lanes over the paths -- r is (n x P), prior and out are (R x P), so that the 64 residuals
//       of training row N_j and the 64 outputs of a row are consecutive doubles;
//   per-path rows (rows_per_path = M > 0: deeper nodes)           row i belongs to path i / M and uses that path's residuals,
//       r (P x n), prior and out (R) = (P x M).
// The block lives in registers (pm <= VG_BC, D <= 16: one wave per row, four rows per workgroup, the design of
// vpaths_rows_reg_kernel) or in LDS (everything else, DGPAMD_VECCHIA_LDS=1: one wave per row and workgroup).
// Jitter is a property of the row: a block with a non-positive pivot or Schur complement is rebuilt with the next rung of the
// ladder jit[0..nj) by the wave that owns it, so a row's value does not depend on the rows that share its call.  In both
// forms and both storages out is ONE chain  acc = prior; acc = fma(b_ij, r[N_j], acc) for j = 0 .. b-1 in list order;
// out = sqrt(scale) * acc: no cross-lane reduction, the same bits for the same row in any call, block or position.
#include "common.hpp"
#include "vblock.hpp"
#include "vecchia_pred.hpp"

#include <climits>
#include <math.h>

#define VPF_MAXJIT 4   // rungs of the jitter ladder a call can pass
#define VPF_PC 2       // 64-path chunks a wave applies side by side (b_ij and N_j are broadcast once for all of them)

struct VPFunArgs {
    int D, pm, nj;
    int64_t R, n, P, M;   // M: rows per path, 0 = shared rows
    const double *x, *w, *omega, *r, *prior;
    const int64_t *NN;
    double nugget, sscale;
    double jit[VPF_MAXJIT];
    double *out;
    int32_t *info;
};

// info[0]: rows that needed a rung beyond the first; info[1]: 1 + the smallest row that failed every rung (the word starts
// with all bits set and takes an unsigned minimum: whichever wave arrives first, the same row is named)
__device__ __forceinline__ void vpfun_note(int32_t *info, int rung, bool bad, int64_t row) {
    if (bad)
        atomicMin(reinterpret_cast<unsigned int *>(info + 1), (unsigned int)(row + 1));
    else if (rung > 0)
        atomicAdd(info, 1);
}

// The apply with the lanes over the paths: b_ij and N_j come as wave-uniform values from coef(j) / nbr(j)
template <class COEF, class NBR>
__device__ __forceinline__ void vpfun_apply_shared(const VPFunArgs &a, const int64_t row, const int b, const int lane, COEF coef, NBR nbr) {
    const int64_t P = a.P;
    for (int64_t p0 = 0; p0 < P; p0 += 64 * VPF_PC) {
        double acc[VPF_PC];
#pragma unroll
        for (int q = 0; q < VPF_PC; ++q) {
            const int64_t p = p0 + 64 * q + lane;
            acc[q] = p < P ? a.prior[row * P + p] : 0.0;
        }
        for (int j = 0; j < b; ++j) {
            const double bj = coef(j);
            const double *rj = a.r + nbr(j) * P;
#pragma unroll
            for (int q = 0; q < VPF_PC; ++q) {
                const int64_t p = p0 + 64 * q + lane;
                if (p < P) acc[q] = fma(bj, rj[p], acc[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < VPF_PC; ++q) {
            const int64_t p = p0 + 64 * q + lane;
            if (p < P) a.out[row * P + p] = a.sscale * acc[q];
        }
    }
}

template <int KIND, int DM>
__global__ __launch_bounds__(256) void vpathfun_reg_kernel(VPFunArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.R) return;   // (wave-uniform)
    const int pm = a.pm, D = a.D;
    const int64_t nnv = lane < pm ? a.NN[w * pm + lane] : -1;
    const int b = __builtin_amdgcn_readfirstlane(__popcll(__ballot(nnv >= 0)));   // (the valid entries come first)
    const bool tr = lane < b;
    double xr[DM];
    {
        const double *src = tr ? a.w + nnv * D : a.x + w * D;
#pragma unroll
        for (int d = 0; d < DM; ++d) xr[d] = (d < D && lane <= b) ? src[d] : 0.0;
    }
    const double dg0 = 1.0 + a.nugget * (tr && a.omega ? a.omega[nnv] : 1.0);
    double reg[VG_BC], last;
    int rung = 0;
    bool bad;
#pragma unroll 1
    for (;;) {
        // (a rung is rare.  The loop sees its own copies of `lane` and `b`: the hundreds of lane masks the unrolled fill and
        //  elimination compare them into are loop invariants otherwise, hoisted in front of the loop and spilled)
        int ln = lane, bl = b;
        asm volatile("" : "+v"(ln), "+s"(bl));
        const double dg = dg0 + a.jit[rung];
        vreg_fill(reg, last, bl, [&](int c) {
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
            return ln == c ? dg : v;
        });
        VPivotDivide pivot;
        vreg_eliminate(reg, last, bl, ln, pivot);
        const double schur = readlane_f64(last, bl);
        bad = __builtin_amdgcn_readfirstlane((int)(pivot.bad || !(schur > 0.0))) != 0;
        if (!bad || rung + 1 >= a.nj) break;
        ++rung;
    }
    if (lane == 0) vpfun_note(a.info, rung, bad, w);
    const double coef = vreg_backsolve(reg, last, b, lane);
    if (a.M == 0) {
        const int nlo = (int)nnv, nhi = (int)(nnv >> 32);
        vpfun_apply_shared(a, w, b, lane, [&](int j) { return readlane_f64(coef, j); },
                           [&](int j) {
                               return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(nhi, j) << 32) |
                                                (uint32_t)__builtin_amdgcn_readlane(nlo, j));
                           });
    } else {
        const double rv = tr ? a.r[(w / a.M) * a.n + nnv] : 0.0;
        double acc = a.prior[w];
        for (int j = 0; j < b; ++j) acc = fma(readlane_f64(coef, j), readlane_f64(rv, j), acc);
        if (lane == 0) a.out[w] = a.sscale * acc;
    }
}

// The same rows with the block in LDS (any pm whose block fits a CU's LDS, D <= DGPAMD_MAXD): a right-looking Cholesky of
// [N(i) ; x_i], then b_i = L11^-T l21.
static inline size_t vpathfun_lds_bytes(int pm, int D) {
    const size_t mp1 = (size_t)pm + 1, lda = (size_t)pm + 2;
    return (mp1 * lda + mp1 * D + 2 * lda) * sizeof(double) + mp1 * sizeof(int64_t);
}

template <int KIND>
__global__ __launch_bounds__(64) void vpathfun_lds_kernel(VPFunArgs a) {
    extern __shared__ double lds[];
    const int pm = a.pm, D = a.D, lda = pm + 2, lane = threadIdx.x;
    double *A = lds;                          // [pm+1][lda] lower triangle of the block
    double *xs = A + (pm + 1) * lda;          // [pm+1][D] scaled coordinates
    double *V = xs + (pm + 1) * D;            // [lda] b_i
    double *RV = V + lda;                     // [lda] the path's residuals at N(i) (per-path rows)
    int64_t *idx = reinterpret_cast<int64_t *>(RV + lda);   // [pm+1]
    const int64_t w = blockIdx.x;
    const int b = load_nn<false>(a.NN + w * pm, pm, idx, lane);
    __syncthreads();
    for (int e = lane; e < (b + 1) * D; e += 64) {
        const int r = e / D, d = e - r * D;
        xs[e] = r < b ? a.w[idx[r] * D + d] : a.x[w * D + d];
    }
    if (a.M)
        for (int c = lane; c < b; c += 64) RV[c] = a.r[(w / a.M) * a.n + idx[c]];
    __syncthreads();
    const int bb = b + 1;
    int rung = 0;
    bool bad;
    for (;;) {
        const double jit = a.jit[rung];
        fill_lower<KIND, VExpFast>(A, lda, bb, xs, D, 1.0,
                                   [&](int r) { return 1.0 + jit + a.nugget * (r < b && a.omega ? a.omega[idx[r]] : 1.0); }, lane);
        bad = lds_chol(A, lda, bb, bb, lane) != 0;   // (read from LDS by every lane alike: wave-uniform)
        if (!bad || rung + 1 >= a.nj) break;
        ++rung;
    }
    if (lane == 0) vpfun_note(a.info, rung, bad, w);
    for (int c = lane; c < b; c += 64) V[c] = A[b * lda + c];   // l21 = L11^-1 a
    lds_backsolve_T(A, lda, b, V, lda, 1, lane);              // V <- L11^-T V
    if (a.M == 0) {
        vpfun_apply_shared(a, w, b, lane, [&](int j) { return V[j]; }, [&](int j) { return idx[j]; });
    } else if (lane == 0) {
        double acc = a.prior[w];
        for (int j = 0; j < b; ++j) acc = fma(V[j], RV[j], acc);
        a.out[w] = a.sscale * acc;
    }
}

extern "C" int dgpamd_vpathfun_update(dgpamd_ctx *ctx, int kind, int64_t R, int64_t n, int D, int pm, int64_t P,
                                      int64_t rows_per_path, const double *x, const double *w, const int64_t *NN,
                                      const double *omega, const double *r, const double *prior, double scale, double nugget,
                                      const double *jitter_h, int njitter, double *out, int32_t *info) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) BAD_ARG(ctx, "kind must be 0 or 1");
    if (R <= 0 || n <= 0 || D <= 0 || D > DGPAMD_MAXD || pm < 1 || P < 1 || rows_per_path < 0 || !x || !w || !NN || !r || !prior ||
        !out || !info || !jitter_h)
        BAD_ARG(ctx, "bad arguments");
    if (njitter < 1 || njitter > VPF_MAXJIT) BAD_ARG(ctx, "the jitter ladder has 1 to 4 rungs");
    if (rows_per_path > 0 && R != P * rows_per_path) BAD_ARG(ctx, "per-path rows: R must be P * rows_per_path");
    if (R >= INT_MAX || n > INT_MAX) BAD_ARG(ctx, "more than 2^31 - 2 rows");
    const bool use_lds = pm > VG_BC || D > 16 || ctx->tune.vecchia_lds;
    const size_t shm = vpathfun_lds_bytes(pm, D);
    if (use_lds && shm > LDS_CU_BYTES) BAD_ARG(ctx, "the conditioning block does not fit a CU's LDS (pm or D too large)");
    VPFunArgs a;
    a.D = D; a.pm = pm; a.nj = njitter; a.R = R; a.n = n; a.P = P; a.M = rows_per_path; a.x = x; a.w = w; a.omega = omega; a.r = r;
    a.prior = prior; a.NN = NN; a.nugget = nugget; a.sscale = sqrt(scale); a.out = out; a.info = info;
    for (int k = 0; k < VPF_MAXJIT; ++k) a.jit[k] = k < njitter ? jitter_h[k] : 0.0;
    HIP_TRY(ctx, hipMemsetAsync(info, 0, sizeof(int32_t), ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(info + 1, 0xff, sizeof(int32_t), ctx->stream));
    if (use_lds)
        return launch_by_kind(ctx, kind, vpathfun_lds_kernel<DGPAMD_SEXP>, vpathfun_lds_kernel<DGPAMD_MATERN25>, dim3((unsigned)R), dim3(64), shm, a, x);
    const dim3 grid4((unsigned)((R + 3) / 4));
    if (D <= 8)
        return launch_by_kind(ctx, kind, vpathfun_reg_kernel<DGPAMD_SEXP, 8>, vpathfun_reg_kernel<DGPAMD_MATERN25, 8>, grid4, dim3(256), 0, a, x);
    return launch_by_kind(ctx, kind, vpathfun_reg_kernel<DGPAMD_SEXP, 16>, vpathfun_reg_kernel<DGPAMD_MATERN25, 16>, grid4, dim3(256), 0, a, x);
}
