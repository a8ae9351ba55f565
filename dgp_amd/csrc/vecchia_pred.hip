// Register-resident Vecchia prediction kernel (a22 gp_vecch vecchia.py:635-654; the link_gp kernels of the same design are
// csrc/vecchia_pred_link_*.hip).  One wave per test point, one row of the conditioning block per lane, rows broadcast entry by
// entry with v_readlane; every register index is a compile-time constant (static_for), which is why this file takes a minute to compile.
#include "vecchia_pred.hpp"
#include "linkfun.hpp"
#include "vblock.hpp"

// The same prediction with the block in REGISTERS (pm <= VG_BC, D <= 16): one wave per test point, one ROW of the
// (b + 2) x (b + 1) block [neighbours ; test point ; y] per lane -- lane r holds row r's b neighbour columns in reg[] and the
// test point's column in `last`.  A column of the block is built by broadcasting point c's scaled coordinates from lane c
// (v_readlane: an SGPR operand for every lane) and evaluating the correlation in all lanes at once; pivot j's elimination
// broadcasts row j entry by entry the same way: reg[c] -= (reg[j] / d_j) * A[j][c] for the rows below j.  No LDS, no barrier,
// no dependent LDS round trips; four test points per workgroup.  (LDL^T without square roots: the Schur complement of the test
// point and the eliminated y row are the same numbers as with gp_vecch's Cholesky, vecchia.py:635-654.)  The LDS kernel above
// ran one wave per point at 3-6 workgroups per CU on chains of dependent LDS reads: 8.3 ms per 100 000 points at pm = 50, D = 8.
template <int KIND, int DM>
__global__ __launch_bounds__(256) void vecchia_gp_reg_kernel(VGpArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.M) return;   // (wave-uniform)
    const int pm = a.pm, D = a.vp.D;
    const int64_t nnv = lane < pm ? a.NN[t * pm + lane] : -1;
    const int b = __builtin_amdgcn_readfirstlane(__popcll(__ballot(nnv >= 0)));   // the valid neighbours come first
    const int bb = b + 1;
    double xr[DM];
    {
        const double *src = lane < b ? a.w + nnv * D : a.x + t * D;
#pragma unroll
        for (int d = 0; d < DM; ++d) xr[d] = (d < D && lane <= b) ? src[d] * a.vp.inv_len[d] : 0.0;
    }
    const double yv = lane < b ? a.y[nnv] : 0.0;
    const double dg = 1.0 + a.vp.nugget * (lane < b ? a.nugget_diag[nnv] : 1.0);
    auto column = [&](int c) {   // column c of the block for every row at once
        double s = 0.0, pr = 1.0;
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            const double df = xr[d] - readlane_f64(xr[d], c);
            if (KIND == DGPAMD_SEXP)
                corr_accum_sexp(df, s);
            else
                corr_accum_matern(df, pr, s);
        }
        double v = (KIND == DGPAMD_SEXP) ? exp_negated(s) : pr * exp_negated(SQRT5 * s);
        v = lane == c ? dg : v;
        return lane == bb ? readlane_f64(yv, c) : v;   // (the y row; yv is 0 in the test point's lane)
    };
    double reg[VG_BC], last;
    vreg_fill(reg, last, b, column);
    VPivotNewton pivot;
    vreg_eliminate(reg, last, b, lane, pivot);   // the b neighbour columns
    const double var = readlane_f64(last, b), mean = readlane_f64(last, bb);
    if (lane == 0) {
        a.mean[t] = -mean;
        a.var[t] = a.scale * var;
    }
}

template <int KIND>
static void launch_vgp_reg(dgpamd_ctx *ctx, const VGpArgs &a) {
    const unsigned grid = (unsigned)((a.M + 3) / 4);
    if (a.vp.D <= 8)
        hipLaunchKernelGGL((vecchia_gp_reg_kernel<KIND, 8>), dim3(grid), dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL((vecchia_gp_reg_kernel<KIND, 16>), dim3(grid), dim3(256), 0, ctx->stream, a);
}
void launch_vecchia_gp_reg(dgpamd_ctx *ctx, const VGpArgs &a) {
    if (a.vp.kind == DGPAMD_SEXP)
        launch_vgp_reg<DGPAMD_SEXP>(ctx, a);
    else
        launch_vgp_reg<DGPAMD_MATERN25>(ctx, a);
}
