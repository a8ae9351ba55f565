// Register-resident Vecchia link_gp kernel of the squared-exponential correlation (a23 link_gp_vecch vecchia.py:758-796 with IJ_nb
// :838-907), the design of csrc/vecchia_pred.hip: one wave per test point, one row of the conditioning block per lane, every
// register index a compile-time constant (static_for) -- minutes to compile, hence a translation unit per kind.
#include "linkfun.hpp"
#include "vblock.hpp"

// link_gp_vecch for the squared-exponential kernel with everything in REGISTERS (pm <= VL_BC, Dw <= 8, Dz in {0} or <= 8):
// one wave per test point, lane r = neighbour r.  reg[c] holds row r of K and, in the columns the elimination has passed, of
// N = (unit lower factor)^-1 -- Gauss-Jordan in place: pivot j's row operation  row_i -= (a_ij / d_j) row_j  applied to the
// identity puts N[i][c] where K's eliminated entries were, with the same fma for every column (row j is broadcast entry by
// entry with v_readlane).  jm[c] holds row r of J and takes the same row operations, M = L^-1 J.  With K = L D L^T:
//   R^-1 y = L^-T v,  v = D^-1 L^-1 y              (y and I ride along as per-lane scalars)
//   mean   = (L^-1 I) . v
//   y' R^-1 J R^-1 y = v . (M t),  t = L^-T v      (column sums over the lanes: wave reductions)
//   tr(K^-1 J) = sum_i (1 / d_i) sum_c M[i][c] N[i][c]
// -- the quantities of vecchia.py:758-796 / IJ_nb :838-907 without a transposition and without LDS.  The coordinates are
// held relative to the test point and scaled (u = (w - m) / l, ug = (wg - z) / l): differences are unchanged, and the
// exponents of I, J and of the global factor become sums of squares of u, u_r + u_c and ug.
template <int DGM>
__global__ __launch_bounds__(256) void vecchia_linkgp_sexp_reg_kernel(VLinkArgs a) {
    constexpr int DLM = 8;
    const int lane = threadIdx.x & 63;
    const int64_t t = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (t >= a.M) return;
    const int pm = a.pm, Dw = a.Dw, Dz = a.Dz;
    const int64_t nnv = lane < pm ? a.NN[t * pm + lane] : -1;
    const int b = __builtin_amdgcn_readfirstlane(__popcll(__ballot(nnv >= 0)));
    const bool act = lane < b;
    // per test point (uniform): weights of the exponents
    double wk[DLM], wi[DLM], c1 = 1.0, jc = 1.0;
#pragma unroll
    for (int k = 0; k < DLM; ++k) {
        wk[k] = 0.0; wi[k] = 0.0;
        if (k < Dw) {
            const double l = a.len[k], v = a.v[t * Dw + k], l2 = l * l;
            wk[k] = l2 / (8.0 * v + 2.0 * l2);
            wi[k] = l2 / (2.0 * v + l2);
            c1 *= 1.0 + 2.0 * v / l2;
            jc *= 1.0 + 4.0 * v / l2;
        }
    }
    jc = 1.0 / sqrt(jc);
    double u[DLM], ug[DGM > 0 ? DGM : 1];
#pragma unroll
    for (int k = 0; k < DLM; ++k) u[k] = (k < Dw && act) ? (a.w1[nnv * Dw + k] - a.m[t * Dw + k]) / a.len[k] : 0.0;
#pragma unroll
    for (int g = 0; g < DGM; ++g) ug[g] = (g < Dz && act) ? (a.wg[nnv * Dz + g] - a.z[t * Dz + g]) / a.len[Dw + g] : 0.0;
    // I (times the factor of the global inputs), y, the nugget's weight
    double Iz = 1.0, Iv, yv = act ? a.y[nnv] : 0.0;
    {
        double e = 0.0, sg = 0.0;
#pragma unroll
        for (int k = 0; k < DLM; ++k) e = fma(u[k] * u[k], wi[k], e);
#pragma unroll
        for (int g = 0; g < DGM; ++g) sg = fma(ug[g], ug[g], sg);
        if (DGM > 0) Iz = exp(-sg);
        Iv = act ? exp(-e) / sqrt(c1) * Iz : 0.0;
    }
    const double dg = 1.0 + a.nugget * (act ? a.nugget_diag[nnv] : 1.0);
    double reg[VL_BC], jm[VL_BC];
    static_for<0, VL_BC>([&](auto ic) {
        constexpr int c = decltype(ic)::value;
        reg[c] = 0.0;
        jm[c] = 0.0;
        if (c < b) {
            double s = 0.0, ex = 0.0;
#pragma unroll
            for (int k = 0; k < DLM; ++k) {
                const double uc = readlane_f64(u[k], c), df = u[k] - uc, sm = u[k] + uc;
                s = fma(df, df, s);
                ex = fma(sm * sm, wk[k], ex);
            }
            ex = fma(0.5, s, ex);
#pragma unroll
            for (int g = 0; g < DGM; ++g) {
                const double df = ug[g] - readlane_f64(ug[g], c);
                s = fma(df, df, s);
            }
            const double kv = lane == c ? dg : exp_negated(s);
            const double jv = jc * exp_negated(ex) * Iz * readlane_f64(Iz, c);
            reg[c] = act ? kv : 0.0;
            jm[c] = act ? jv : 0.0;
        }
    });
    linkgp_reg_finish(reg, jm, yv, Iv, act, b, lane, a, t);
}

void launch_vecchia_linkgp_sexp_reg(dgpamd_ctx *ctx, const VLinkArgs &a) {
    const unsigned grid = (unsigned)((a.M + 3) / 4);
    if (a.Dz == 0)
        hipLaunchKernelGGL(vecchia_linkgp_sexp_reg_kernel<0>, dim3(grid), dim3(256), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(vecchia_linkgp_sexp_reg_kernel<8>, dim3(grid), dim3(256), 0, ctx->stream, a);
}
