// Vecchia per-row kernels (reference dgpsi/vecchia.py) with the likelihood, gradient, sparse-factor and
// heteroskedastic entries.
//
// Thousands of tiny (m+1)x(m+1) problems: ONE WAVE (a 64-thread workgroup) per row, the block matrix lives in LDS
// (csrc/vblock.hpp), the right-hand side rides along as an extra row of the factorisation (same trick as chol.hip), so
// forward solves cost nothing extra; conditioning sets of at most 31 points are held in registers, four rows per wave.
#include "vblock.hpp"
#include "vecchia_row4.hpp"

#include <math.h>

// ---------------------------------------------------------------------------
// a19-a21  per-row kernels on the ordered data
// ---------------------------------------------------------------------------
template <int KIND, int MODE>
__global__ __launch_bounds__(VW) void vecchia_row_kernel(VRowArgs a) {
    extern __shared__ double lds[];
    if (a.pred && *a.pred) return;
    const int mp1 = a.m + 1, D = a.vp.D, lda = mp1 + 2;
    double *A = lds;                         // [(mp1+1)][lda]  block + one right-hand-side row
    double *xs = A + (mp1 + 1) * lda;        // [mp1][D] scaled inputs
    double *V = xs + mp1 * D;                // [2][lda]  u = L^-T e_last, alpha = L^-T w
    int *idx = reinterpret_cast<int *>(V + 2 * lda);
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int b = load_nn<true>(a.NN + i * mp1, mp1, idx, lane);   // ascending index, self last: idx[idx>=0][::-1]
    __syncthreads();
    for (int e = lane; e < b * D; e += VW) {
        int r = e / D, d = e - r * D;
        xs[e] = a.X[(int64_t)idx[r] * D + d] * a.vp.inv_len[d];
    }
    __syncthreads();
    fill_lower<KIND, VExpLib>(A, lda, b, xs, D, 1.0,
                              [&](int r) { return 1.0 + a.vp.nugget * (MODE == V_LMAT ? 1.0 : a.nugget_diag[idx[r]]); }, lane);
    const int rows = (MODE == V_LMAT) ? b : b + 1;
    if (MODE != V_LMAT)
        for (int c = lane; c <= b; c += VW) A[b * lda + c] = c < b ? a.y[idx[c]] : 0.0;
    lds_chol(A, lda, rows, b, lane);

    if (MODE == V_LLIK) {
        if (lane == 0) {
            const double wl = A[b * lda + b - 1], ll = A[(b - 1) * lda + b - 1];
            a.partial[i * 2] = wl * wl;                 // (L^-1 y)_last^2      vecchia.py:177
            a.partial[i * 2 + 1] = 2.0 * log(fabs(ll)); // 2 log L_last,last   vecchia.py:178
        }
        return;
    }
    // u = L^-T e_last (and alpha = L^-T w for the gradient)
    for (int c = lane; c < b; c += VW) {
        V[c] = (c == b - 1) ? 1.0 : 0.0;
        if (MODE == V_NLLIK) V[lda + c] = A[b * lda + c];
    }
    lds_backsolve_T(A, lda, b, V, lda, MODE == V_NLLIK ? 2 : 1, lane);
    if (MODE == V_LMAT) {
        for (int c = lane; c < mp1; c += VW) a.Lmat[i * mp1 + c] = c < b ? V[b - 1 - c] : 0.0;   // reversed, self first
        return;
    }
    // vecchia.py:216-219 restated: t_last = u^T dK u ; s = alpha^T dK u
    //   dquad_k = 2 s w_last - t_last w_last^2 ; dlogdet_k = t_last
    const int P = a.P, npl = (a.vp.nlen == 1) ? 1 : D;
    const double wl = A[b * lda + b - 1];
    double *out = a.partial + i * (2 + 2 * P);
    if (lane == 0) {
        out[0] = wl * wl;
        out[1] = 2.0 * log(fabs(A[(b - 1) * lda + b - 1]));
    }
    const double *u = V, *al = V + lda;
    for (int k = 0; k < npl; ++k) {
        double tl = 0.0, s = 0.0;
        for (int e = lane; e < b * (b - 1) / 2; e += VW) {   // (strictly lower triangle: row r + 1, column c of the decoded pair)
            int r, c;
            tri_decode(e, r, c);
            ++r;
            double kv = corr_pts<KIND, VExpLib>(xs + r * D, xs + c * D, D), cf = 0.0;
            if (a.vp.nlen == 1)
                for (int d = 0; d < D; ++d) cf += dcoef_v<KIND>(xs[r * D + d] - xs[c * D + d]);
            else
                cf = dcoef_v<KIND>(xs[r * D + k] - xs[c * D + k]);
            const double dk = cf * kv;
            tl = fma(2.0 * dk, u[r] * u[c], tl);
            s = fma(dk, al[r] * u[c] + al[c] * u[r], s);
        }
        tl = wave_sum_all(tl);
        s = wave_sum_all(s);
        if (lane == 0) {
            out[2 + k] = 2.0 * s * wl - tl * wl * wl;
            out[2 + P + k] = tl;
        }
    }
    if (a.nugget_est) {   // dK/dlog eta = diag(nugget * nugget_diag)   vecchia.py:329-332
        double tl = 0.0, s = 0.0;
        for (int r = lane; r < b; r += VW) {
            const double dk = a.vp.nugget * a.nugget_diag[idx[r]];
            tl = fma(dk, u[r] * u[r], tl);
            s = fma(dk, al[r] * u[r], s);
        }
        tl = wave_sum_all(tl);
        s = wave_sum_all(s);
        if (lane == 0) {
            out[2 + npl] = 2.0 * s * wl - tl * wl * wl;
            out[2 + P + npl] = tl;
        }
    }
}

// deterministic column sums of partial[batch][n][w] -> out[batch][w]  (grid: w x batch)
__global__ __launch_bounds__(1024) void colsum_kernel(const double *partial, int64_t n, int w, double *out) {
    __shared__ double sm[16];
    const int c = blockIdx.x, tid = threadIdx.x;
    partial += (int64_t)blockIdx.y * n * w;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    int64_t r = tid;
    for (; r + 3072 < n; r += 4096) {   // four loads in flight per thread
        v0 += partial[r * w + c];
        v1 += partial[(r + 1024) * w + c];
        v2 += partial[(r + 2048) * w + c];
        v3 += partial[(r + 3072) * w + c];
    }
    for (; r < n; r += 1024) v0 += partial[r * w + c];
    double v = (v0 + v1) + (v2 + v3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((tid & 63) == 0) sm[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int q = 0; q < 16; ++q) t += sm[q];
        out[(int64_t)blockIdx.y * w + c] = t;
    }
}

static size_t vrow_lds(int m, int D) {
    const int mp1 = m + 1, lda = mp1 + 2;
    return ((size_t)(mp1 + 1) * lda + (size_t)mp1 * D + 2 * lda) * sizeof(double) + (size_t)mp1 * sizeof(int);
}

// Debugging aid (DGPAMD_POISON_LDS=1): fill the LDS of every CU with NaNs before a launch, so that a read of LDS the
// kernel has not written shows up in the results whatever ran on the device before (tests/test_gpu_ops.py uses it).
__global__ __launch_bounds__(256) void lds_poison_kernel(double *sink) {
    extern __shared__ double lds[];
    for (int i = threadIdx.x; i < 8192; i += 256) lds[i] = __builtin_nan("");
    __syncthreads();
    if (lds[(threadIdx.x * 31) & 8191] == 1.0) sink[0] = 1.0;   // (never true: keeps the stores alive)
}

int maybe_poison_lds(dgpamd_ctx *ctx, const double *any_device_ptr) {
    if (ctx->tune.poison_lds) {
        HIP_TRY(ctx, hipFuncSetAttribute((const void *)lds_poison_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
        hipLaunchKernelGGL(lds_poison_kernel, dim3(8 * ctx->num_cu), dim3(256), 65536, ctx->stream, (double *)any_device_ptr);
    }
    return DGPAMD_OK;
}

// Fill every CU's LDS with NaNs now (whatever the environment says): Engine._enter calls it before EVERY library call under
// DGPAMD_POISON_LDS=2, which puts the whole test suite under the same check.
extern "C" int dgpamd_debug_poison_lds(dgpamd_ctx *ctx) {
    if (!ctx) return DGPAMD_BAD_ARG;
    double *sink = nullptr;
    HIP_TRY(ctx, hipMallocAsync((void **)&sink, sizeof(double), ctx->stream));
    HIP_TRY(ctx, hipFuncSetAttribute((const void *)lds_poison_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 65536));
    hipLaunchKernelGGL(lds_poison_kernel, dim3(8 * ctx->num_cu), dim3(256), 65536, ctx->stream, sink);
    HIP_TRY(ctx, hipFreeAsync(sink, ctx->stream));
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

template <int MODE>
static int launch_vrow(dgpamd_ctx *ctx, VRowArgs &a, int batch = 1) {
    if (a.m + 1 <= VR_MAXB && !ctx->tune.vecchia_lds) {   // (DGPAMD_VECCHIA_LDS=1: the LDS version for every size -- the tests compare the two)   // register-resident factorisation, two rows per wave
        int prc = maybe_poison_lds(ctx, a.X);
        if (prc) return prc;
        return a.vp.kind == DGPAMD_SEXP ? launch_vrow4<DGPAMD_SEXP, MODE>(ctx, a, batch) : launch_vrow4<DGPAMD_MATERN25, MODE>(ctx, a, batch);
    }
    VRowArgs one = a;
    for (int bb = 0; bb < batch; ++bb) {   // (LDS version: one launch per input set)
        int rc = launch_by_kind(ctx, a.vp.kind, vecchia_row_kernel<DGPAMD_SEXP, MODE>, vecchia_row_kernel<DGPAMD_MATERN25, MODE>,
                                dim3((unsigned)a.n), dim3(VW), vrow_lds(a.m, a.vp.D), one, a.X);
        if (rc) return rc;
        one.X += a.x_stride;
        one.partial += a.n * 2;
    }
    return DGPAMD_OK;
}

// scratch for the per-row partials lives behind the public outputs: the caller passes device buffers sized for the reduced
// result only; the context keeps one growable buffer for them (ctx_scratch).
static int with_partials(dgpamd_ctx *ctx, size_t bytes, double **p) {
    return ctx_scratch(ctx, 0, bytes, reinterpret_cast<void **>(p));   // (row kernel writes, column sums read: stream order)
}

int vecchia_llik_batch_into(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X, int64_t x_stride, int batch,
                            const double *y, const int64_t *NNarray, const double *length_h, int nlen, double nugget,
                            const double *nugget_diag, double *partial, double *out) {
    VRowArgs a;
    int rc = fill_vparams(ctx, a.vp, kind, D, length_h, nlen, nugget);
    if (rc) return rc;
    a.n = n; a.m = m; a.X = X; a.y = y; a.nugget_diag = nugget_diag; a.NN = NNarray; a.nugget_est = 0; a.P = 0;
    a.Lmat = nullptr; a.x_stride = x_stride; a.partial = partial; a.pred = ctx->pred;
    rc = launch_vrow<V_LLIK>(ctx, a, batch);
    if (rc) return rc;
    hipLaunchKernelGGL(colsum_kernel, dim3(2, (unsigned)batch), dim3(1024), 0, ctx->stream, (const double *)partial, n, 2, out);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_vecchia_llik_batch(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X, int64_t x_stride,
                                         int batch, const double *y, const int64_t *NNarray, const double *length_h, int nlen,
                                         double nugget, const double *nugget_diag, double *out_llik) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || m < 0 || batch <= 0 || batch > 65535 || !X || !y || !NNarray || !nugget_diag || !out_llik)
        BAD_ARG(ctx, "bad arguments");
    double *partial = nullptr;
    int rc = with_partials(ctx, (size_t)batch * n * 2 * sizeof(double), &partial);
    if (rc) return rc;
    return vecchia_llik_batch_into(ctx, kind, n, D, m, X, x_stride, batch, y, NNarray, length_h, nlen, nugget, nugget_diag, partial, out_llik);
}

extern "C" int dgpamd_vecchia_llik(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X, const double *y,
                                   const int64_t *NNarray, const double *length_h, int nlen, double nugget,
                                   const double *nugget_diag, double *out_llik) {
    return dgpamd_vecchia_llik_batch(ctx, kind, n, D, m, X, 0, 1, y, NNarray, length_h, nlen, nugget, nugget_diag, out_llik);
}

extern "C" int dgpamd_vecchia_nllik(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X,
                                    const double *y, const int64_t *NNarray, const double *length_h, int nlen,
                                    double nugget, const double *nugget_diag, int nugget_est, double *out_nllik) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || m < 0 || !X || !y || !NNarray || !nugget_diag || !out_nllik) BAD_ARG(ctx, "bad arguments");
    VRowArgs a;
    int rc = fill_vparams(ctx, a.vp, kind, D, length_h, nlen, nugget);
    if (rc) return rc;
    a.n = n; a.m = m; a.X = X; a.y = y; a.nugget_diag = nugget_diag; a.NN = NNarray; a.nugget_est = nugget_est ? 1 : 0;
    a.P = (nlen == 1 ? 1 : D) + a.nugget_est;
    a.Lmat = nullptr; a.x_stride = 0; a.pred = nullptr;
    const int w = 2 + 2 * a.P;
    rc = with_partials(ctx, (size_t)n * w * sizeof(double), &a.partial);
    if (rc) return rc;
    rc = launch_vrow<V_NLLIK>(ctx, a);
    if (rc) return rc;
    hipLaunchKernelGGL(colsum_kernel, dim3(w), dim3(1024), 0, ctx->stream, (const double *)a.partial, n, w, out_nllik);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_vecchia_lmatrix(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X,
                                      const int64_t *NNarray, const double *length_h, int nlen, double nugget,
                                      double *Lmat) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || m < 0 || !X || !NNarray || !Lmat) BAD_ARG(ctx, "bad arguments");
    VRowArgs a;
    int rc = fill_vparams(ctx, a.vp, kind, D, length_h, nlen, nugget);
    if (rc) return rc;
    a.n = n; a.m = m; a.X = X; a.y = nullptr; a.nugget_diag = nullptr; a.NN = NNarray; a.nugget_est = 0; a.P = 0;
    a.partial = nullptr; a.Lmat = Lmat; a.x_stride = 0; a.pred = nullptr;
    return launch_vrow<V_LMAT>(ctx, a);
}

// ---------------------------------------------------------------------------
// Hetero likelihood, exact conditional posterior of the mean latent under Vecchia (imputation.py:143-160,
// vecchia.U_matrix :426-446, U_matrix_sp :599-610, Hetero.post_het_vecch likelihood_class.py:166-182).
// Row i of impNN (kernel_class.py:268-274) conditions the LATENT of ordered point i on, in the stacked vector
// [observations 0..n-1 ; latents n..2n-1], its own latent (n+i), its own observation (i) and its nearest other
// points (latent if earlier in the ordering, observation otherwise).  u_i = L_i^-T e_last of the block
// scale*corr + diag(gamma on observation entries + 1e-10) is column i of the sparse factor U; the reference
// assembles U (2n x n) with scipy.sparse and solves with U_l^T.  Here every row is emitted directly in the layout
// dgpamd_vecchia_spsolve consumes: Lrows[i] = [diagonal, latent-neighbour entries, 0..], NNl[i] = [i, their
// columns, 0..], and t_i = sum over the observation entries of u * y  (= (U_ol^T y)_i).
// ---------------------------------------------------------------------------
struct VHetArgs {
    VParams vp;
    int64_t n;
    int m;
    const double *X, *gamma, *y;
    const int64_t *NN;
    double scale;
    double *Lrows, *t;
    int64_t *NNl;
    int32_t *info;
};

template <int KIND>
__global__ __launch_bounds__(VW) void vecchia_het_rows_kernel(VHetArgs a) {
    extern __shared__ double lds[];
    const int mp1 = a.m + 1, D = a.vp.D, lda = mp1 + 2;
    double *A = lds;                         // [(mp1+1)][lda]
    double *xs = A + (mp1 + 1) * lda;        // [mp1][D] scaled inputs
    double *V = xs + mp1 * D;                // [2][lda]  u = L^-T e_last
    int *idx = reinterpret_cast<int *>(V + 2 * lda);
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x, n = a.n;
    const int b = load_nn<true>(a.NN + i * mp1, mp1, idx, lane);   // reversed: own observation, own latent last
    __syncthreads();
    for (int e = lane; e < b * D; e += VW) {
        const int r = e / D, d = e - r * D;
        const int64_t p = idx[r] >= n ? idx[r] - n : idx[r];
        xs[e] = a.X[p * D + d] * a.vp.inv_len[d];
    }
    __syncthreads();
    fill_lower<KIND, VExpLib>(A, lda, b, xs, D, a.scale,
                              [&](int r) { return a.scale + (idx[r] >= n ? 0.0 : a.gamma[idx[r]]) + 1e-10; }, lane);
    const int bad = lds_chol(A, lda, b, b, lane);
    for (int c = lane; c < b; c += VW) V[c] = (c == b - 1) ? 1.0 : 0.0;
    lds_backsolve_T(A, lda, b, V, lda, 1, lane);
    if (lane == 0) {
        if (bad) atomicCAS(a.info, 0, (int)(i + 1));   // a block that is not positive definite (numpy raises LinAlgError)
        double *Lr = a.Lrows + i * mp1;
        int64_t *Nr = a.NNl + i * mp1;
        Lr[0] = V[b - 1];
        Nr[0] = i;
        int slot = 1;
        double t = 0.0;
        for (int c = 0; c < b - 1; ++c) {
            if (idx[c] >= n) {
                Lr[slot] = V[c];
                Nr[slot] = idx[c] - n;
                ++slot;
            } else {
                t = fma(V[c], a.y[idx[c]], t);
            }
        }
        for (; slot < mp1; ++slot) {
            Lr[slot] = 0.0;
            Nr[slot] = 0;
        }
        a.t[i] = t;
    }
}

extern "C" int dgpamd_vecchia_het_rows(dgpamd_ctx *ctx, int kind, int64_t n, int D, int m, const double *X,
                                       const int64_t *impNN, const double *length_h, int nlen, double scale,
                                       const double *gamma, const double *y, double *Lrows, int64_t *NNl, double *t,
                                       int32_t *info) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || m < 1 || !X || !impNN || !gamma || !y || !Lrows || !NNl || !t || !info) BAD_ARG(ctx, "bad arguments");
    HIP_TRY(ctx, hipMemsetAsync(info, 0, sizeof(int32_t), ctx->stream));
    VHetArgs a;
    int rc = fill_vparams(ctx, a.vp, kind, D, length_h, nlen, 0.0);
    if (rc) return rc;
    a.n = n; a.m = m; a.X = X; a.gamma = gamma; a.y = y; a.NN = impNN; a.scale = scale; a.Lrows = Lrows; a.NNl = NNl; a.t = t; a.info = info;
    return launch_by_kind(ctx, kind, vecchia_het_rows_kernel<DGPAMD_SEXP>, vecchia_het_rows_kernel<DGPAMD_MATERN25>, dim3((unsigned)n),
                          dim3(VW), vrow_lds(m, D), a, a.X);
}
