// Imputed-GP prediction.
//   gp      (functions.py:379-394)  m = ry.r , v = |scale(1+eta - r^T Rinv r)|
//           as  cross_corr -> symmetric MFMA quadratic form (lower tiles of Rinv, x2) -> finalize
//   and the moments over imputations.  (link_gp: linkgp.hip.)
#include "common.hpp"
#include "tile.hpp"
#include "linkgp.hpp"   // MC_MAX

#include <math.h>

// ---------------------------------------------------------------------------
// r[i][t] = k(W_i, x_t)   (K_vec_nb, vecchia.py:244-265)
// ---------------------------------------------------------------------------
struct CrossArgs {
    int kind, D;
    double inv_len[DGPAMD_MAXD];
    int64_t n, M, t0, Mc;
    const double *W, *x;
    double *R;   // [npad][Mc]
};

template <int KIND>
__global__ __launch_bounds__(256) void cross_corr_kernel(CrossArgs a) {
    extern __shared__ double lds[];
    const int D = a.D;
    double *WT = lds, *XT = lds + D * 64;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
    for (int idx = tid; idx < 64 * D; idx += 256) {
        int row = idx / D, d = idx - row * D;
        int64_t gi = i0 + row, gt = a.t0 + c0 + row;
        // relative to the first training point: scaled raw coordinates lose eps |w| / l of every difference below
        const double c = a.W[d];
        WT[d * 64 + row] = (gi < a.n ? a.W[gi * D + d] - c : 0.0) * a.inv_len[d];
        XT[d * 64 + row] = (gt < a.M ? a.x[gt * D + d] - c : 0.0) * a.inv_len[d];
    }
    __syncthreads();
    double s[4][4], pr[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[p][q] = 0.0;
            pr[p][q] = 1.0;
        }
    for (int d = 0; d < D; ++d) {
        double xi[4], xj[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            xi[p] = WT[d * 64 + ty + 16 * p];
            xj[p] = XT[d * 64 + tx + 16 * p];
        }
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double df = xi[p] - xj[q];
                if (KIND == DGPAMD_SEXP)
                    corr_accum_sexp(df, s[p][q]);
                else
                    corr_accum_matern(df, pr[p][q], s[p][q]);
            }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int64_t gi = i0 + ty + 16 * p;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double v = (KIND == DGPAMD_SEXP) ? exp(-s[p][q]) : pr[p][q] * exp(-SQRT5 * s[p][q]);
            if (gi >= a.n) v = 0.0;
            a.R[gi * a.Mc + c0 + tx + 16 * q] = v;
        }
    }
}

// partial[bi][t] = sum_{i in block bi} r_it * ( Rinv[bi][bi] r_bi + 2 sum_{kb<bi} Rinv[bi][kb] r_kb )_it
struct GpQuadArgs {
    const double *Rinv;
    int64_t ldr, n, Mc;
    const double *R;
    double *partial;
};

__global__ __launch_bounds__(256) void gp_quad_kernel(GpQuadArgs a) {
    __shared__ double As[64 * LDM];
    __shared__ double Bs[KC * LDK];
    __shared__ double red[4][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int bi = blockIdx.x, tj = blockIdx.y;
    d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
    const int64_t rlim = a.n - (int64_t)bi * 64;
    for (int kb = 0; kb <= bi; ++kb) {
        const double *Ag = a.Rinv + ((int64_t)bi * 64) * a.ldr + (int64_t)kb * 64;
        const double *Bg = a.R + ((int64_t)kb * 64) * a.Mc + (int64_t)tj * 64;
        const int64_t clim = a.n - (int64_t)kb * 64;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __syncthreads();
            load_mk_masked(Ag, a.ldr, As, tid, h, rlim > 64 ? 64 : (int)rlim, clim > 64 ? 64 : (int)clim);
            load_km(Bg, a.Mc, Bs, tid, h, 64);
            __syncthreads();
            mfma_tile<OP_MK, OP_KM>(As, Bs, acc, wave, lane, kb < bi ? 2.0 : 1.0);
        }
    }
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            v = fma(acc[t][r], a.R[((int64_t)bi * 64 + crow + 4 * r) * a.Mc + (int64_t)tj * 64 + 16 * t + ccol], v);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 16) red[wave][16 * t + lane] = v;
    }
    __syncthreads();
    if (tid < 64) a.partial[(int64_t)bi * a.Mc + (int64_t)tj * 64 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

__global__ __launch_bounds__(256) void gp_finalize_kernel(const double *R, const double *partial, const double *ry,
                                                          int nry, int64_t n, int nb, int64_t Mc, int64_t t0, int64_t M,
                                                          double scale, double nugget, double *mean, double *var) {
    // 64 test points per workgroup (coalesced over t), the training points in 4 interleaved slices (one per wave)
    __shared__ double part[4][64];
    const int slice = threadIdx.x >> 6, tl = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 64 + tl;
    const bool live = t < Mc && t0 + t < M;
    for (int s = blockIdx.y; s < nry; s += gridDim.y) {
        const double *rys = ry + (int64_t)s * n;
        double m = 0.0;
        if (live)
            for (int64_t i = slice; i < n; i += 4) m = fma(rys[i], R[i * Mc + t], m);
        part[slice][tl] = m;
        __syncthreads();
        if (slice == 0 && live) mean[(int64_t)s * M + t0 + t] = (part[0][tl] + part[1][tl]) + (part[2][tl] + part[3][tl]);
        __syncthreads();
    }
    if (blockIdx.y == 0) {
        double q = 0.0;
        if (live)
            for (int b = slice; b < nb; b += 4) q += partial[(int64_t)b * Mc + t];
        part[slice][tl] = q;
        __syncthreads();
        if (slice == 0 && live) var[t0 + t] = fabs(scale * (1.0 + nugget - ((part[0][tl] + part[1][tl]) + (part[2][tl] + part[3][tl]))));
    }
}

extern "C" size_t dgpamd_gp_workspace(int64_t n, int64_t M) {
    int64_t nb = (n + 63) / 64;
    int64_t Mc = ((M + 63) / 64) * 64;
    if (Mc > MC_MAX) Mc = MC_MAX;
    return (size_t)((nb * 64 + nb) * Mc) * sizeof(double);
}

extern "C" int dgpamd_gp_predict(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int D, const double *x,
                                 const double *Wtr, const double *length_h, int nlen, const double *Rinv, int64_t ldr,
                                 const double *ry, int nry, double scale, double nugget, double *mean, double *var,
                                 void *work) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || M <= 0 || nry <= 0 || !x || !Wtr || !length_h || !Rinv || !ry || !mean || !var || !work)
        BAD_ARG(ctx, "null pointer or empty problem");
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) BAD_ARG(ctx, "kind must be 0 or 1");
    if (D <= 0 || D > DGPAMD_MAXD || (nlen != 1 && nlen != D)) BAD_ARG(ctx, "bad D / nlen");
    if (ldr < n) BAD_ARG(ctx, "ldr < n");
    const int nb = (int)((n + 63) / 64);
    int64_t Mc = ((M + 63) / 64) * 64;
    if (Mc > MC_MAX) Mc = MC_MAX;
    double *R = (double *)work, *partial = R + (int64_t)nb * 64 * Mc;
    CrossArgs c;
    c.kind = kind; c.D = D; c.n = n; c.M = M; c.Mc = Mc; c.W = Wtr; c.x = x; c.R = R;
    for (int d = 0; d < D; ++d) c.inv_len[d] = 1.0 / length_h[nlen == 1 ? 0 : d];
    GpQuadArgs q;
    q.Rinv = Rinv; q.ldr = ldr; q.n = n; q.Mc = Mc; q.R = R; q.partial = partial;
    const size_t shm = (size_t)2 * D * 64 * sizeof(double);   // (64 KB at D = DGPAMD_MAXD)
    int rc = set_lds(ctx, kind == DGPAMD_SEXP ? (const void *)cross_corr_kernel<DGPAMD_SEXP> : (const void *)cross_corr_kernel<DGPAMD_MATERN25>, shm);
    if (rc) return rc;
    for (int64_t t0 = 0; t0 < M; t0 += Mc) {
        c.t0 = t0;
        int64_t mc = M - t0 < Mc ? M - t0 : Mc;
        unsigned tb = (unsigned)((mc + 63) / 64);
        if (kind == DGPAMD_SEXP)
            hipLaunchKernelGGL(cross_corr_kernel<DGPAMD_SEXP>, dim3(nb, tb), dim3(256), shm, ctx->stream, c);
        else
            hipLaunchKernelGGL(cross_corr_kernel<DGPAMD_MATERN25>, dim3(nb, tb), dim3(256), shm, ctx->stream, c);
        // algorithmic flops of r^T R^-1 r for mc test points as the reference forms it (functions.py:379-394: R^-1 r, then the dot
        // product): 2 n^2 mc; the kernel reads the lower tiles of R^-1 only and executes half of that
        PROF_BEGIN(ctx, PROF_GP_QUAD, 2.0 * (double)n * (double)n * (double)mc);
        hipLaunchKernelGGL(gp_quad_kernel, dim3(nb, tb), dim3(256), 0, ctx->stream, q);
        PROF_END(ctx, PROF_GP_QUAD);
        hipLaunchKernelGGL(gp_finalize_kernel, dim3((unsigned)((mc + 63) / 64), (unsigned)(nry < 64 ? nry : 64)),
                           dim3(256), 0, ctx->stream, (const double *)R, (const double *)partial, ry, nry, n, nb, Mc,
                           t0, M, scale, nugget, mean, var);
    }
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

// ---------------------------------------------------------------------------
// a15  moments over imputations (emulation.py:846-847)
// ---------------------------------------------------------------------------
__global__ void moments_acc_kernel(int64_t count, const double *mu, const double *var, double *s1, double *s2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        double m = mu[i];
        s1[i] += m;
        s2[i] += m * m + var[i];
    }
}
__global__ void moments_fin_kernel(int64_t count, double S, double *s1, double *s2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        double m = s1[i] / S;
        s1[i] = m;
        s2[i] = s2[i] / S - m * m;
    }
}

extern "C" int dgpamd_moments_accumulate(dgpamd_ctx *ctx, int64_t count, const double *mu, const double *var,
                                         double *sum_mu, double *sum_m2) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (count <= 0 || !mu || !var || !sum_mu || !sum_m2) BAD_ARG(ctx, "null pointer or empty");
    int64_t blocks = (count + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(moments_acc_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, count, mu, var, sum_mu, sum_m2);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_moments_finalize(dgpamd_ctx *ctx, int64_t count, double S, double *sum_mu_to_mu,
                                       double *sum_m2_to_var) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (count <= 0 || !(S > 0.0) || !sum_mu_to_mu || !sum_m2_to_var) BAD_ARG(ctx, "bad arguments");
    int64_t blocks = (count + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(moments_fin_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, count, S, sum_mu_to_mu, sum_m2_to_var);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
