// Linked-GP prediction.
//   link_gp (functions.py:396-430)  m = I.ry , v = |sum_ij J_ij (ry_i ry_j - scale Rinv_ij) - m^2 + scale(1+eta)|
//           one workgroup per (lower 64x64 tile of C = ry ry^T - scale Rinv) x (chunk of test points);
//           Psexp / R2sexp (functions.py:259-272, kernel_class.py:752-764) are never materialised.
// Per chunk of test points: mean -> the pair kernel of the plan's form (linkgp_plan.hpp; the forms live in linkgp_direct.hip,
// linkgp_sexp.hip and linkgp_matern.hip, each launched from its own file) -> finalize.
#include "linkgp_plan.hpp"
#include "linkfun.hpp"

#include <math.h>

// mean_t = sum_i I_i(t) ry_i : one workgroup per test point (the training points strided over its 256 threads)
template <int KIND>
__global__ __launch_bounds__(256) void linkgp_mean_kernel(LinkArgs a) {
    __shared__ double part[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t t = a.t0 + (int64_t)blockIdx.x;
    if (t >= a.M || t >= a.t0 + a.Mc) return;
    const double *mt = a.m + t * a.Dw, *vt = a.v + t * a.Dw;
    const double *zt = a.Dz ? a.z + t * a.Dz : nullptr;
    // leave-one-out: (R_-d)^-1 y = Rinv y - u (Rinv y)_d / u_d with u = Rinv[:, d], zero at d itself
    const int64_t dr = a.drop ? a.drop[t] : -1;
    const double *ud = a.drop ? a.Rinv + dr * a.ldr : nullptr;
    const double cd = a.drop ? a.ry[dr] / ud[dr] : 0.0;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < a.n; i += 256) {
        if (i == dr) continue;
        double I;
        if (KIND == DGPAMD_SEXP) {
            double e = 0.0;
            for (int k = 0; k < a.Dw; ++k) {
                double l = a.len[k], d = a.W[i * a.Dw + k] - mt[k];
                e += d * d / (2.0 * vt[k] + l * l);
            }
            for (int g = 0; g < a.Dz; ++g) {
                double d = (a.Wg[i * a.Dz + g] - zt[g]) / a.len[a.Dw + g];
                e += d * d;
            }
            I = exp(-e);
        } else {
            I = 1.0;
            for (int k = 0; k < a.Dw; ++k) I *= matern_I_dim(a.W[i * a.Dw + k], mt[k], vt[k], a.len[k]);
            double pr = 1.0, s = 0.0;
            for (int g = 0; g < a.Dz; ++g) corr_accum_matern((a.Wg[i * a.Dz + g] - zt[g]) / a.len[a.Dw + g], pr, s);
            I *= pr * exp(-SQRT5 * s);
        }
        acc = fma(I, ud ? a.ry[i] - cd * ud[i] : a.ry[i], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        acc = (part[0] + part[1]) + (part[2] + part[3]);
        if (KIND == DGPAMD_SEXP) {
            double c = 1.0;
            for (int k = 0; k < a.Dw; ++k) c *= 1.0 + 2.0 * vt[k] / (a.len[k] * a.len[k]);
            acc *= 1.0 / sqrt(c);
        }
        a.mean[t] = acc;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void linkgp_finalize_kernel(LinkArgs a, int ntiles) {   // one wave per test point
    const int lane = threadIdx.x & 63;
    const int64_t tt = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t t = a.t0 + tt;
    if (tt >= a.Mc || t >= a.M) return;
    double s = 0.0;
    for (int b = lane; b < ntiles; b += 64) s += a.partial[(int64_t)b * a.Mc + tt];
    s = wave_sum(s);
    if (lane) return;
    if (KIND == DGPAMD_SEXP) {
        double c = 1.0;
        for (int k = 0; k < a.Dw; ++k) c *= 1.0 + 4.0 * a.v[t * a.Dw + k] / (a.len[k] * a.len[k]);
        s *= 1.0 / sqrt(c);
    }
    const double mu = a.mean[t];
    a.var[t] = fabs(s - mu * mu + a.scale * (1.0 + a.nugget));
}

extern "C" size_t dgpamd_linkgp_workspace(int64_t n, int64_t M, int Dw) { return linkgp_workspace_bytes(n, M, Dw); }

static int linkgp_run(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int Dw, int Dz, const double *m, const double *v,
                      const double *z, const double *Wtr, const double *Wg, const double *length_h, int nlen,
                      const double *Rinv, int64_t ldr, const double *ry, const int32_t *drop, double scale,
                      double nugget, double *mean, double *var, void *work) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || M <= 0 || !m || !v || !Wtr || !length_h || !Rinv || !ry || !mean || !var || !work)
        BAD_ARG(ctx, "null pointer or empty problem");
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) BAD_ARG(ctx, "kind must be 0 or 1");
    if (Dw <= 0 || Dz < 0 || Dw + Dz > DGPAMD_MAXD) BAD_ARG(ctx, "bad Dw / Dz");
    if (Dz > 0 && (!z || !Wg)) BAD_ARG(ctx, "Dz > 0 needs z and Wg");
    if (nlen != 1 && nlen != Dw + Dz) BAD_ARG(ctx, "nlen must be 1 or Dw+Dz");
    if (ldr < n) BAD_ARG(ctx, "ldr < n");
    LinkArgs a;
    a.kind = kind; a.Dw = Dw; a.Dz = Dz; a.n = n; a.M = M; a.m = m; a.v = v; a.z = z; a.W = Wtr; a.Wg = Wg;
    for (int d = 0; d < Dw + Dz; ++d) a.len[d] = length_h[nlen == 1 ? 0 : d];   // functions.py:402-410 broadcast
    a.Rinv = Rinv; a.ldr = ldr; a.ry = ry; a.scale = scale; a.nugget = nugget; a.mean = mean; a.var = var;
    a.partial = (double *)work;
    a.drop = drop;
    a.no_order_classes = 0;
    a.dbg = nullptr;
    const LinkPlan p = linkgp_plan(ctx->tune, kind, n, M, Dw, Dz, drop != nullptr, ctx->linkgp_direct != 0, ctx->tlog != nullptr);
    if (p.refused()) return set_lds(ctx, nullptr, p.lds);   // (its refusal, before any launch)
    a.tch = p.tc;
    a.Mc = p.Mc;
    a.npad = (int64_t)p.nb * 64;
    a.recs = a.partial + p.partial_doubles;
    a.gfac = a.recs + p.gfac_off;
    for (int64_t t0 = 0; t0 < M; t0 += p.Mc) {
        a.t0 = t0;
        const int64_t mc = M - t0 < p.Mc ? M - t0 : p.Mc;
        int rc = DGPAMD_OK;
        if (kind == DGPAMD_SEXP)
            hipLaunchKernelGGL(linkgp_mean_kernel<DGPAMD_SEXP>, dim3((unsigned)mc), dim3(256), 0, ctx->stream, a);
        else
            hipLaunchKernelGGL(linkgp_mean_kernel<DGPAMD_MATERN25>, dim3((unsigned)mc), dim3(256), 0, ctx->stream, a);
        switch (p.form) {
            case LINK_DIRECT: rc = linkgp_launch_direct(ctx, a, p, mc); break;
            case LINK_SEXP_MFMA: rc = linkgp_launch_sexp_mfma(ctx, a, p, mc); break;
            case LINK_SEXP_RECORDS: rc = linkgp_launch_sexp_records(ctx, a, p, mc); break;
            case LINK_MATERN_SEP: rc = linkgp_launch_matern_sep(ctx, a, p, mc); break;
        }
        if (rc) return rc;
        if (kind == DGPAMD_SEXP)
            hipLaunchKernelGGL(linkgp_finalize_kernel<DGPAMD_SEXP>, dim3((unsigned)((mc + 3) / 4)), dim3(256), 0, ctx->stream, a, p.ntiles);
        else
            hipLaunchKernelGGL(linkgp_finalize_kernel<DGPAMD_MATERN25>, dim3((unsigned)((mc + 3) / 4)), dim3(256), 0, ctx->stream, a, p.ntiles);
    }
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_linkgp_predict(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int Dw, int Dz, const double *m,
                                     const double *v, const double *z, const double *Wtr, const double *Wg,
                                     const double *length_h, int nlen, const double *Rinv, int64_t ldr,
                                     const double *ry, double scale, double nugget, double *mean, double *var,
                                     void *work) {
    return linkgp_run(ctx, kind, n, M, Dw, Dz, m, v, z, Wtr, Wg, length_h, nlen, Rinv, ldr, ry, nullptr, scale, nugget,
                      mean, var, work);
}

extern "C" int dgpamd_linkgp_loo(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int Dw, int Dz, const double *m,
                                 const double *v, const double *z, const double *Wtr, const double *Wg,
                                 const double *length_h, int nlen, const double *Rinv, int64_t ldr, const double *ry,
                                 const int32_t *drop, double scale, double nugget, double *mean, double *var,
                                 void *work) {
    if (ctx && !drop) BAD_ARG(ctx, "drop is null");
    return linkgp_run(ctx, kind, n, M, Dw, Dz, m, v, z, Wtr, Wg, length_h, nlen, Rinv, ldr, ry, drop, scale, nugget, mean,
                      var, work);
}
