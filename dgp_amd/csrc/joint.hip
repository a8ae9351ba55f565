// Joint posterior covariance of GP test points and joint posterior sample paths (emulator.sample_paths, gp.sample_paths).
//   dgpamd_joint_cov   per item b (test inputs x_b) and its group g (training inputs W_g, factor inverse L^-1_g, rows y_g):
//       [V | w] = L^-1 [K(W, x_b) | y^T]                          (kext_kernel -> trmm_kernel)
//       Sigma_b = scale (K(x_b, x_b) + nugget I - V^T V) ,  mean_b = V^T w       (joint_syrk_kernel)
//   dgpamd_mvn_paths   out_b = mean_b + L_b E_b with L_b the factor of Sigma_b   (trmm_kernel on MFMA, or trmv for one column)
// The V^T V form instead of K*^T R^-1 K*: V^T V is positive semi-definite by construction and no entry of R^-1 (which reach
// ~1/nugget) enters, so Sigma keeps scale * nugget on its diagonal up to rounding.
#include "common.hpp"
#include "tile.hpp"

#include <math.h>

#define JMAX_PACK 4   // items of one group that share the staged L^-1 tile in trmm_kernel

static inline int64_t pad64(int64_t v) { return (v + 63) / 64 * 64; }

// ---------------------------------------------------------------------------
// Kext_b[k][c] (npad x Mc): c < M: k(W_k, x_c); Mp <= c < Mp + r: y[c - Mp][k]; zero elsewhere and in rows k >= n
// ---------------------------------------------------------------------------
struct KextArgs {
    int kind, D, r;
    double inv_len[DGPAMD_MAXD];
    int64_t n, M, Mp, Mc, npad;
    const double *x;
    int64_t stride_x;
    const double *W, *y;
    int64_t stride_w, stride_y;
    int32_t group[DGPAMD_MAXB];
    double *K;   // batch x npad x Mc
};

template <int KIND>
__global__ __launch_bounds__(256) void kext_kernel(KextArgs a) {
    extern __shared__ double lds[];
    const int D = a.D, b = blockIdx.z, g = a.group[b];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * 64, c0 = (int64_t)blockIdx.y * 64;
    double *Kb = a.K + (int64_t)b * a.npad * a.Mc;
    if (c0 >= a.Mp) {   // right-hand-side columns: y^T
        const double *yg = a.y + (int64_t)g * a.stride_y;
        for (int idx = tid; idx < 4096; idx += 256) {
            const int64_t k = i0 + (idx >> 6), q = c0 - a.Mp + (idx & 63);
            Kb[k * a.Mc + c0 + (idx & 63)] = (k < a.n && q < a.r) ? yg[q * a.n + k] : 0.0;
        }
        return;
    }
    const double *W = a.W + (int64_t)g * a.stride_w, *x = a.x + (int64_t)b * a.stride_x;
    double *WT = lds, *XT = lds + D * 64;
    for (int idx = tid; idx < 64 * D; idx += 256) {
        int row = idx / D, d = idx - row * D;
        int64_t gi = i0 + row, gt = c0 + row;
        WT[d * 64 + row] = (gi < a.n ? W[gi * D + d] : 0.0) * a.inv_len[d];
        XT[d * 64 + row] = (gt < a.M ? x[gt * D + d] : 0.0) * a.inv_len[d];
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
            const int64_t gt = c0 + tx + 16 * q;
            double v = (KIND == DGPAMD_SEXP) ? exp(-s[p][q]) : pr[p][q] * exp(-SQRT5 * s[p][q]);
            if (gi >= a.n || gt >= a.M) v = 0.0;
            Kb[gi * a.Mc + gt] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// C_b = mean_b(:, col / rep) + L_g(b) B_b : lower-triangular (nl x nl, lower 64x64 tiles read, entries above the diagonal
// ignored) times dense (nl x cols).  One workgroup per 64x64 tile of C and pack of up to JMAX_PACK items with the same L:
// each L tile is staged once for the whole pack.
// ---------------------------------------------------------------------------
struct TrmmArgs {
    const double *L;
    int64_t ldl, stride_l;   // stride between the L of consecutive groups
    int64_t nl;              // dimension of L (rows of B and C)
    const double *B;
    int64_t ldb, stride_b, cols;
    double *C;
    int64_t ldc, stride_c;
    const double *mean;      // null, or (nl x cols / rep) per item
    int64_t ldm, stride_m;
    int rep;
    int32_t group[DGPAMD_MAXB];
    int32_t pack_first[DGPAMD_MAXB], pack_count[DGPAMD_MAXB];
};

// MK half tile of L (rows = m, k contiguous); rows >= rlim, columns >= clim and (diagonal tile) columns above the diagonal read as zero
__device__ __forceinline__ void load_tri_mk(const double *__restrict__ g, int64_t ldg, double *__restrict__ s, int tid, int h,
                                            int rlim, int clim, bool diag) {
    const int c2 = (tid & 15) * 2;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = (tid >> 4) + 16 * it;
        const int c = 32 * h + c2;
        double v0 = 0.0, v1 = 0.0;
        if (r < rlim) {
            if (c < clim && (!diag || c <= r)) v0 = g[(int64_t)r * ldg + c];
            if (c + 1 < clim && (!diag || c + 1 <= r)) v1 = g[(int64_t)r * ldg + c + 1];
        }
        s[r * LDM + c2] = v0;
        s[r * LDM + c2 + 1] = v1;
    }
}
// KM half tile (rows = k 32h.., 64 columns) with row and column limits, element loads (any ld)
__device__ __forceinline__ void load_km_masked(const double *__restrict__ g, int64_t ldg, double *__restrict__ s, int tid, int h,
                                               int rlim, int clim) {
    const int c2 = (tid & 31) * 2;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = (tid >> 5) + 8 * it;
        const int k = 32 * h + r;
        double v0 = 0.0, v1 = 0.0;
        if (k < rlim) {
            if (c2 < clim) v0 = g[(int64_t)k * ldg + c2];
            if (c2 + 1 < clim) v1 = g[(int64_t)k * ldg + c2 + 1];
        }
        s[r * LDK + c2] = v0;
        s[r * LDK + c2 + 1] = v1;
    }
}

__global__ __launch_bounds__(256) void trmm_kernel(TrmmArgs a) {
    __shared__ double As[64 * LDM];
    __shared__ double Bs[KC * LDK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int bi = blockIdx.x, tj = blockIdx.y;
    const int first = a.pack_first[blockIdx.z], cnt = a.pack_count[blockIdx.z];
    const double *L = a.L + (int64_t)a.group[first] * a.stride_l;
    const int64_t rl = a.nl - (int64_t)bi * 64, cl = a.cols - (int64_t)tj * 64;
    const int rlim = rl > 64 ? 64 : (int)rl, clim = cl > 64 ? 64 : (int)cl;
    d4 acc[JMAX_PACK][4];
#pragma unroll
    for (int p = 0; p < JMAX_PACK; ++p)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[p][t] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb <= bi; ++kb) {
        const double *Ag = L + ((int64_t)bi * 64) * a.ldl + (int64_t)kb * 64;
        const int64_t kl = a.nl - (int64_t)kb * 64;
        const int klim = kl > 64 ? 64 : (int)kl;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            __syncthreads();
            load_tri_mk(Ag, a.ldl, As, tid, h, rlim, klim, kb == bi);
#pragma unroll
            for (int p = 0; p < JMAX_PACK; ++p) {
                if (p < cnt) {   // (uniform over the workgroup)
                    if (p > 0) __syncthreads();
                    const double *Bg = a.B + (int64_t)(first + p) * a.stride_b + ((int64_t)kb * 64) * a.ldb + (int64_t)tj * 64;
                    load_km_masked(Bg, a.ldb, Bs, tid, h, klim, clim);
                    __syncthreads();
                    mfma_tile<OP_MK, OP_KM>(As, Bs, acc[p], wave, lane, 1.0);
                }
            }
        }
    }
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
#pragma unroll
    for (int p = 0; p < JMAX_PACK; ++p) {
        if (p >= cnt) break;
        const int b = first + p;
        double *C = a.C + (int64_t)b * a.stride_c;
        const double *mn = a.mean ? a.mean + (int64_t)b * a.stride_m : nullptr;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = crow + 4 * r, j = 16 * t + ccol;
                if (i < rlim && j < clim) {
                    const int64_t gi = (int64_t)bi * 64 + i, gj = (int64_t)tj * 64 + j;
                    double v = acc[p][t][r];
                    if (mn) v += mn[gi * a.ldm + gj / a.rep];
                    C[gi * a.ldc + gj] = v;
                }
            }
    }
}

// ---------------------------------------------------------------------------
// Sigma_b lower tiles (bi >= bj over the padded dimension, padding zero as dgpamd_kmatrix leaves it) and mean_b tiles:
//   tile t < ntri: Sigma(bi, bj) = scale (K** + nugget I - V(:, bi)^T V(:, bj));   else mean(bi, q-tile) = V(:, bi)^T w
// ---------------------------------------------------------------------------
struct SyrkArgs {
    int kind, D, r;
    double inv_len[DGPAMD_MAXD];
    int64_t n, M, Mp, Mc, npad;
    const double *x;
    int64_t stride_x;
    const double *V;         // batch x npad x Mc
    double scale, nugget;
    double *A;
    int64_t lda, stride_a;
    double *mean;            // batch x M x r
    int ntri, nbm, nbr;
};

template <int KIND>
__global__ __launch_bounds__(256) void joint_syrk_kernel(SyrkArgs a) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, b = blockIdx.y;
    const int t = blockIdx.x;
    int bi, bj;
    bool is_mean = t >= a.ntri;
    if (!is_mean) {
        tri_decode(t, bi, bj);
    } else {
        bi = (t - a.ntri) / a.nbr;
        bj = (t - a.ntri) % a.nbr;
    }
    const double *V = a.V + (int64_t)b * a.npad * a.Mc;
    const int64_t colA = (int64_t)bi * 64, colB = is_mean ? a.Mp + (int64_t)bj * 64 : (int64_t)bj * 64;
    d4 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = (d4){0.0, 0.0, 0.0, 0.0};
    const bool live = bi < a.nbm && (is_mean || bj < a.nbm);   // (tiles of the padding beyond Mp have no V columns)
    if (live) {
        double *As = lds, *Bs = lds + KC * LDK;
        const int nkb = (int)(a.npad / 64);
        for (int kb = 0; kb < nkb; ++kb) {
            const int64_t kl = a.n - (int64_t)kb * 64;
            const int klim = kl > 64 ? 64 : (int)kl;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                __syncthreads();
                load_km(V + ((int64_t)kb * 64) * a.Mc + colA, a.Mc, As, tid, h, klim);
                load_km(V + ((int64_t)kb * 64) * a.Mc + colB, a.Mc, Bs, tid, h, klim);
                __syncthreads();
                mfma_tile<OP_KM, OP_KM>(As, Bs, acc, wave, lane, 1.0);
            }
        }
    }
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
    if (is_mean) {
        double *mn = a.mean + (int64_t)b * a.M * a.r;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gi = colA + crow + 4 * r, gq = (int64_t)bj * 64 + 16 * q + ccol;
                if (gi < a.M && gq < a.r) mn[gi * a.r + gq] = acc[q][r];
            }
        return;
    }
    // K** from the scaled test inputs of rows bi and columns bj (the staging space is free again)
    const int D = a.D;
    const double *x = a.x + (int64_t)b * a.stride_x;
    double *XI = lds, *XJ = lds + D * 64;
    __syncthreads();
    for (int idx = tid; idx < 64 * D; idx += 256) {
        int row = idx / D, d = idx - row * D;
        int64_t gi = (int64_t)bi * 64 + row, gj = (int64_t)bj * 64 + row;
        XI[d * 64 + row] = (gi < a.M ? x[gi * D + d] : 0.0) * a.inv_len[d];
        XJ[d * 64 + row] = (gj < a.M ? x[gj * D + d] : 0.0) * a.inv_len[d];
    }
    __syncthreads();
    double *Ab = a.A + (int64_t)b * a.stride_a;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int il = crow + 4 * r, jl = 16 * q + ccol;
            const int64_t gi = (int64_t)bi * 64 + il, gj = (int64_t)bj * 64 + jl;
            double s = 0.0, pr = 1.0;
            for (int d = 0; d < D; ++d) {
                const double df = XI[d * 64 + il] - XJ[d * 64 + jl];
                if (KIND == DGPAMD_SEXP)
                    corr_accum_sexp(df, s);
                else
                    corr_accum_matern(df, pr, s);
            }
            double k = (KIND == DGPAMD_SEXP) ? exp(-s) : pr * exp(-SQRT5 * s);
            if (gi == gj) k = 1.0 + a.nugget;
            double v = a.scale * (k - acc[q][r]);
            if (gi >= a.M || gj >= a.M) v = 0.0;
            Ab[gi * a.lda + gj] = v;
        }
}

static void joint_dims(int64_t n, int64_t M, int r, int64_t &npad, int64_t &Mp, int64_t &Mc) {
    npad = pad64(n);
    Mp = pad64(M);
    Mc = Mp + (r > 0 ? pad64(r) : 0);
}

extern "C" size_t dgpamd_joint_workspace(int64_t n, int64_t M, int r, int batch) {
    if (n <= 0 || M <= 0 || r < 0 || batch <= 0) return 0;
    int64_t npad, Mp, Mc;
    joint_dims(n, M, r, npad, Mp, Mc);
    return (size_t)2 * batch * npad * Mc * sizeof(double);   // Kext and V of every item
}

// packs of consecutive items with the same group (at most JMAX_PACK per pack)
static int make_packs(const int32_t *group, int batch, int32_t *first, int32_t *count) {
    int np = 0;
    for (int b = 0; b < batch;) {
        int c = 1;
        while (b + c < batch && c < JMAX_PACK && group[b + c] == group[b]) ++c;
        first[np] = b;
        count[np] = c;
        ++np;
        b += c;
    }
    return np;
}

extern "C" int dgpamd_joint_cov(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int D, int r, int batch, const double *x,
                                int64_t stride_x, const int32_t *group_h, int ngroups, const double *W, int64_t stride_w,
                                const double *Linv, int64_t ldl, int64_t stride_l, const double *y, int64_t stride_y,
                                const double *length_h, int nlen, double scale, double nugget, double *A, int64_t stride_a,
                                double *mean, void *work) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || M <= 0 || r < 0 || !x || !W || !Linv || !length_h || !A || !work) BAD_ARG(ctx, "null pointer or empty problem");
    if (r > 0 && (!y || !mean)) BAD_ARG(ctx, "r > 0 needs y and mean");
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) BAD_ARG(ctx, "kind must be 0 or 1");
    if (D <= 0 || D > DGPAMD_MAXD || (nlen != 1 && nlen != D)) BAD_ARG(ctx, "bad D / nlen");
    if (batch <= 0 || batch > DGPAMD_MAXB) BAD_ARG(ctx, "need 1 <= batch <= DGPAMD_MAXB");
    if (ngroups <= 0) BAD_ARG(ctx, "need ngroups >= 1");
    if (ldl < pad64(n)) BAD_ARG(ctx, "ldl < n rounded up to 64");
    const int64_t lda = padded_dim(M);
    if (batch > 1 && stride_a < lda * lda) BAD_ARG(ctx, "stride_a < padded_dim(M)^2");
    int32_t group[DGPAMD_MAXB];
    for (int b = 0; b < batch; ++b) {
        group[b] = group_h ? group_h[b] : 0;
        if (group[b] < 0 || group[b] >= ngroups) BAD_ARG(ctx, "group index out of range");
    }
    int64_t npad, Mp, Mc;
    joint_dims(n, M, r, npad, Mp, Mc);
    double *Kx = (double *)work, *V = Kx + (int64_t)batch * npad * Mc;
    // (1) Kext = [K(W, x) | y^T]
    KextArgs k;
    k.kind = kind; k.D = D; k.r = r; k.n = n; k.M = M; k.Mp = Mp; k.Mc = Mc; k.npad = npad;
    k.x = x; k.stride_x = stride_x; k.W = W; k.y = y; k.stride_w = stride_w; k.stride_y = stride_y; k.K = Kx;
    for (int d = 0; d < D; ++d) k.inv_len[d] = 1.0 / length_h[nlen == 1 ? 0 : d];
    for (int b = 0; b < batch; ++b) k.group[b] = group[b];
    const size_t shm = (size_t)2 * D * 64 * sizeof(double);   // (64 KB at D = DGPAMD_MAXD)
    const void *kf = kind == DGPAMD_SEXP ? (const void *)kext_kernel<DGPAMD_SEXP> : (const void *)kext_kernel<DGPAMD_MATERN25>;
    int rc = set_lds(ctx, kf, shm);
    if (rc) return rc;
    dim3 g1((unsigned)(npad / 64), (unsigned)(Mc / 64), (unsigned)batch);
    if (kind == DGPAMD_SEXP)
        hipLaunchKernelGGL(kext_kernel<DGPAMD_SEXP>, g1, dim3(256), shm, ctx->stream, k);
    else
        hipLaunchKernelGGL(kext_kernel<DGPAMD_MATERN25>, g1, dim3(256), shm, ctx->stream, k);
    // (2) [V | w] = L^-1 Kext, items of one group in packs
    TrmmArgs t;
    t.L = Linv; t.ldl = ldl; t.stride_l = stride_l; t.nl = n;
    t.B = Kx; t.ldb = Mc; t.stride_b = npad * Mc; t.cols = Mc;
    t.C = V; t.ldc = Mc; t.stride_c = npad * Mc;
    t.mean = nullptr; t.ldm = 0; t.stride_m = 0; t.rep = 1;
    for (int b = 0; b < batch; ++b) t.group[b] = group[b];
    const int np = make_packs(group, batch, t.pack_first, t.pack_count);
    hipLaunchKernelGGL(trmm_kernel, dim3((unsigned)(npad / 64), (unsigned)(Mc / 64), (unsigned)np), dim3(256), 0, ctx->stream, t);
    // (3) Sigma and mean
    SyrkArgs s;
    s.kind = kind; s.D = D; s.r = r; s.n = n; s.M = M; s.Mp = Mp; s.Mc = Mc; s.npad = npad;
    s.x = x; s.stride_x = stride_x; s.V = V; s.scale = scale; s.nugget = nugget;
    s.A = A; s.lda = lda; s.stride_a = stride_a; s.mean = mean;
    for (int d = 0; d < D; ++d) s.inv_len[d] = k.inv_len[d];
    const int nbA = (int)(lda / 64);
    s.ntri = nbA * (nbA + 1) / 2;
    s.nbm = (int)(Mp / 64);
    s.nbr = r > 0 ? (int)(pad64(r) / 64) : 0;
    const size_t shm3 = (size_t)(2 * KC * LDK > 2 * 64 * D ? 2 * KC * LDK : 2 * 64 * D) * sizeof(double);
    const void *sf = kind == DGPAMD_SEXP ? (const void *)joint_syrk_kernel<DGPAMD_SEXP> : (const void *)joint_syrk_kernel<DGPAMD_MATERN25>;
    rc = set_lds(ctx, sf, shm3);
    if (rc) return rc;
    dim3 g3((unsigned)(s.ntri + s.nbm * s.nbr), (unsigned)batch);
    if (kind == DGPAMD_SEXP)
        hipLaunchKernelGGL(joint_syrk_kernel<DGPAMD_SEXP>, g3, dim3(256), shm3, ctx->stream, s);
    else
        hipLaunchKernelGGL(joint_syrk_kernel<DGPAMD_MATERN25>, g3, dim3(256), shm3, ctx->stream, s);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

// out_b[i] = mean_b[i] + sum_{j <= i} L_b[i][j] e_b[j]: one wave per row (trmv_lower_kernel's pattern)
__global__ __launch_bounds__(256) void mvn_trmv_kernel(const double *L, int64_t ld, int64_t stride_l, int64_t M,
                                                       const double *mean, int64_t stride_m, const double *E, int64_t stride_e,
                                                       double *out, int64_t stride_o) {
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= M) return;
    const double *row = L + (int64_t)b * stride_l + i * ld;
    const double *e = E + (int64_t)b * stride_e;
    double s = 0.0;
    for (int64_t j = lane; j <= i; j += 64) s = fma(row[j], e[j], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) out[(int64_t)b * stride_o + i] = (mean ? mean[(int64_t)b * stride_m + i] : 0.0) + s;
}

extern "C" int dgpamd_mvn_paths(dgpamd_ctx *ctx, int64_t M, int c, int rep, int batch, const double *L, int64_t stride_l,
                                const double *mean, int64_t stride_m, const double *E, int64_t stride_e, double *out,
                                int64_t stride_o) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (M <= 0 || c <= 0 || !L || !E || !out) BAD_ARG(ctx, "null pointer or empty problem");
    if (rep <= 0 || c % rep) BAD_ARG(ctx, "rep must divide c");
    if (batch <= 0 || batch > DGPAMD_MAXB) BAD_ARG(ctx, "need 1 <= batch <= DGPAMD_MAXB");
    const int64_t ld = padded_dim(M);
    if (c == 1) {
        hipLaunchKernelGGL(mvn_trmv_kernel, dim3((unsigned)((M + 3) / 4), (unsigned)batch), dim3(256), 0, ctx->stream, L, ld,
                           stride_l, M, mean, stride_m, E, stride_e, out, stride_o);
        LAUNCH_CHECK(ctx);
        return DGPAMD_OK;
    }
    TrmmArgs t;
    t.L = L; t.ldl = ld; t.stride_l = stride_l; t.nl = M;
    t.B = E; t.ldb = c; t.stride_b = stride_e; t.cols = c;
    t.C = out; t.ldc = c; t.stride_c = stride_o;
    t.mean = mean; t.ldm = c / rep; t.stride_m = stride_m; t.rep = rep;
    for (int b = 0; b < batch; ++b) {   // (every item its own factor: packs of one)
        t.group[b] = b;
        t.pack_first[b] = b;
        t.pack_count[b] = 1;
    }
    hipLaunchKernelGGL(trmm_kernel, dim3((unsigned)((M + 63) / 64), (unsigned)((c + 63) / 64), (unsigned)batch), dim3(256), 0,
                       ctx->stream, t);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
