// Blocked Cholesky / triangular inverse on augmented buffers (SURVEY 8 a3,a5,a8,a10).
// Replaces the LAPACK potrf/potrs call sites of the reference
// (kernel_class.py:417-423,483-487,746-748; functions.py:109,119).
//
// Right-looking, 64-wide block columns.  Per block column k:
//   potrf_diag   one workgroup per matrix: the 64x64 diagonal block is held in
//                registers (4x4 strided micro-tiles), each pivot column is
//                broadcast through LDS with ONE barrier per pivot, and the same
//                loop applies the eliminations to an identity -> the block's
//                inverse comes out for free (used instead of a triangular solve);
//   tile_gemm    TRSM as  P_i = A_ik * Linv_kk^T   (f64 MFMA 16x16x4),
//                SYRK as  A_ij -= P_i P_j^T        (lower tiles only).
// The same tile_gemm engine runs the blocked triangular inverse (recursive
// doubling over block pairs) and K^-1 = L^-T L^-1.
//
// This file: the entry points and their dispatch (run_potrf), the tile GEMM engine of potri and the small side kernels.  The
// factorisation's two kernels live in potrf_step.hpp (one launch per block step) and potrf_mega.hpp (one persistent launch),
// their shared device helpers in chol_tile.hpp, and what the host decides about them -- task tables, the plan of a launch, the
// workspace layout -- in potrf_plan.hpp.
#include "common.hpp"
#include "tile.hpp"
#include "potrf_plan.hpp"

// ----------------------------------------------------------------------------
// 64x64x64 tile GEMM engine on f64 MFMA
// ----------------------------------------------------------------------------
enum { G_TRTRI1 = 2, G_TRTRI2 = 3, G_LAUUM = 4 };

struct GemmArgs {
    double *A;        // Np x Np buffers
    double *B;        // second buffer (temp / inverse)
    const double *ws; // diagonal-block inverses
    int64_t ld, stride_a, stride_ws;
    int64_t n;
    int nbk;   // blocks per dimension
    int k;     // block column (TRSM / SYRK)
    int s;     // half-size of the pair in blocks (TRTRI)
};

template <int MODE>
__global__ __launch_bounds__(256) void tile_gemm_kernel(GemmArgs g) {
    constexpr int OPA = (MODE == G_LAUUM) ? OP_KM : OP_MK;
    constexpr int OPB = OP_KM;
    __shared__ double As[(OPA == OP_MK) ? 64 * LDM : KC * LDK];
    __shared__ double Bs[(OPB == OP_MK) ? 64 * LDM : KC * LDK];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t ld = g.ld;
    double *A = g.A + (int64_t)blockIdx.z * g.stride_a;
    double *B = g.B ? g.B + (int64_t)blockIdx.z * g.stride_a : nullptr;

    int bi, bj, kb0, kb1;          // output tile, k-block range [kb0, kb1)
    double *C;                     // output buffer
    double sign = 1.0;
    if (MODE == G_TRTRI1 || MODE == G_TRTRI2) {
        const int s = g.s, per = s * s;
        const int p = blockIdx.x / per, rem = blockIdx.x - p * per;
        const int base = 2 * p * s;
        bi = base + s + rem / s; bj = base + rem % s;
        if (bi >= g.nbk) return;
        if (MODE == G_TRTRI1) {           // T = L21 * Linv11   (Linv11 lower: kb >= bj)
            kb0 = bj; kb1 = base + s; C = B;
        } else {                          // X21 = -Linv22 * T  (Linv22 lower: kb <= bi)
            kb0 = base + s; kb1 = bi + 1; C = A; sign = -1.0;
        }
    } else {                              // LAUUM: Kinv_ij = sum_{kb >= bi} Linv[kb][bi]^T Linv[kb][bj]
        tri_decode(blockIdx.x, bi, bj);
        kb0 = bi; kb1 = (int)((g.n + 63) / 64); C = B;
    }

    d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (d4){0.0, 0.0, 0.0, 0.0};
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
    // operands of k-block kb
    auto operands = [&](int kb, const double *&Ag, const double *&Bg, int64_t &lda, int64_t &ldb, int &lim) {
        lda = ld; ldb = ld; lim = 64;
        if (MODE == G_TRTRI1) {
            Ag = A + ((int64_t)bi * 64) * ld + (int64_t)kb * 64;
            Bg = A + ((int64_t)kb * 64) * ld + (int64_t)bj * 64;
        } else if (MODE == G_TRTRI2) {
            Ag = A + ((int64_t)bi * 64) * ld + (int64_t)kb * 64;
            Bg = B + ((int64_t)kb * 64) * ld + (int64_t)bj * 64;
        } else {
            Ag = A + ((int64_t)kb * 64) * ld + (int64_t)bi * 64;
            Bg = A + ((int64_t)kb * 64) * ld + (int64_t)bj * 64;
            int64_t l = g.n - (int64_t)kb * 64;   // rows >= n (right-hand sides) do not belong to L^-1
            lim = l >= 64 ? 64 : (int)l;
        }
    };
    auto fetch = [&](int st, HalfTile &fa, HalfTile &fb) {
        const double *Ag, *Bg;
        int64_t lda, ldb;
        int lim;
        operands(kb0 + (st >> 1), Ag, Bg, lda, ldb, lim);
        fa = (OPA == OP_MK) ? fetch_mk(Ag, lda, tid, st & 1) : fetch_km(Ag, lda, tid, st & 1, lim);
        fb = (OPB == OP_MK) ? fetch_mk(Bg, ldb, tid, st & 1) : fetch_km(Bg, ldb, tid, st & 1, lim);
    };
    // software pipeline over the 32-deep stages: the loads of stage st+1 are in flight during the MFMAs of stage st
    const int nst = 2 * (kb1 - kb0);
    HalfTile fa, fb;
    if (nst > 0) fetch(0, fa, fb);
    for (int st = 0; st < nst; ++st) {
        __syncthreads();
        if (OPA == OP_MK) commit_mk(fa, As, tid); else commit_km(fa, As, tid);
        if (OPB == OP_MK) commit_mk(fb, Bs, tid); else commit_km(fb, Bs, tid);
        if (st + 1 < nst) fetch(st + 1, fa, fb);
        __syncthreads();
        mfma_tile<OPA, OPB>(As, Bs, acc, wave, lane, sign);
    }

#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t gr = (int64_t)bi * 64 + crow + 4 * r, gc = (int64_t)bj * 64 + 16 * t + ccol;
            C[gr * ld + gc] = acc[t][r];
            if (MODE == G_LAUUM && bi != bj) C[gc * ld + gr] = acc[t][r];
        }
}

// column n of T holds -K^-1 y: copy it into row n of S (the layout dgpamd_potri leaves: row n of Ainv = -alpha^T)
__global__ void copy_alpha_kernel(const double *T, double *S, int64_t ld, int64_t n, int64_t stride_a) {
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    T += (int64_t)blockIdx.y * stride_a;
    S += (int64_t)blockIdx.y * stride_a;
    S[n * ld + j] = T[j * ld + n];
}

// place the diagonal-block inverses on the diagonal of the (to be inverted) factor
__global__ __launch_bounds__(256) void put_diag_inverse_kernel(double *A, int64_t ld, const double *ws,
                                                               int64_t stride_a, int64_t stride_ws) {
    const int kb = blockIdx.x, tid = threadIdx.x;
    double *Ab = A + (int64_t)blockIdx.y * stride_a + ((int64_t)kb * 64) * ld + (int64_t)kb * 64;
    const double *W = ws + (int64_t)blockIdx.y * stride_ws + (int64_t)kb * 4096;
    for (int idx = tid; idx < 4096; idx += 256) Ab[(int64_t)(idx >> 6) * ld + (idx & 63)] = W[idx];
}

// rows [n, n+r) of L^-1 (columns < n) are -alpha^T: copy them beside K^-1
__global__ void copy_aug_rows_kernel(const double *A, double *B, int64_t ld, int64_t n, int r, int64_t stride_a) {
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    A += (int64_t)blockIdx.y * stride_a;
    B += (int64_t)blockIdx.y * stride_a;
    for (int q = 0; q < r; ++q) B[(n + q) * ld + j] = A[(n + q) * ld + j];
}

__global__ void aug_quad_kernel(const double *A, int64_t ld, int64_t stride_a, int64_t n, int r, double *quad) {
    int b = blockIdx.x, t = threadIdx.x;
    if (t < r * r) {
        int q = t / r, q2 = t % r;
        quad[(int64_t)b * r * r + t] = -A[(int64_t)b * stride_a + (n + q) * ld + n + q2];
    }
}

// out[b][i] = sqrt(scale_b) * sum_{j<=i} L[i][j] z[b][j]; one wave per row
struct TrmvArgs {
    const double *L;
    int64_t ld, stride_a, n;
    const double *z;
    double *out;
    double sscale[DGPAMD_MAXB];
};
__global__ __launch_bounds__(256) void trmv_lower_kernel(TrmvArgs a) {
    const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= a.n) return;
    const double *row = a.L + (int64_t)b * a.stride_a + i * a.ld;
    const double *z = a.z + (int64_t)b * a.n;
    double s = 0.0;
    for (int64_t j = lane; j <= i; j += 64) s = fma(row[j], z[j], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) a.out[(int64_t)b * a.n + i] = a.sscale[b] * s;
}

// ----------------------------------------------------------------------------
// host drivers
// ----------------------------------------------------------------------------
extern "C" size_t dgpamd_potrf_workspace(int64_t n, int batch) {
    return potrf_workspace_bytes(n, batch);
}

// status: the one-launch kernel's give-up word (null for the per-step launches, whose spins write info = -1 themselves).
// A lost hand-off is reported as info = -1 for every matrix of the call: not a numerical failure (ops.py raises
// DgpAmdError for it, not LinAlgError).
__global__ void potrf_copy_out_kernel(const double *ld_ws, const int32_t *info_ws, double *logdet, int32_t *info, int batch,
                                      const int32_t *status) {
    const int b = threadIdx.x;
    if (b < batch) {
        logdet[b] = __hip_atomic_load(ld_ws + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int st = status ? __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        info[b] = st ? -1 : __hip_atomic_load(info_ws + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

static bool potrf_uses_mega(const dgpamd_ctx *ctx) {
    // mode 1 (default): the one persistent launch; mode 0: one launch per block step (no in-kernel waits between workgroups: the
    // fallback when the device is shared -- HandoffError -- and the same-run reference of the tools).  The device queue's
    // predicated launches exist for the one-launch kernel only.  (Round 2's mode 2, chosen per call by batch size, had no advantage
    // at any batch size and is gone.)
    return ctx->potrf_mode == 1;
}

void potrf_sync_area(dgpamd_ctx *ctx, int64_t n, int batch, bool inv, double *ws, int32_t **ptr, int *words) {
    *ptr = nullptr;
    *words = 0;
    (void)inv;
    if (!potrf_uses_mega(ctx)) return;
    *ptr = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(ws) + mega_sync_offset(n, batch));
    *words = (int)(mega_sync_bytes(padded_dim(n) / 64, batch) / sizeof(int32_t));
}

int run_potrf(dgpamd_ctx *ctx, int64_t n, double *A, int64_t stride_a, int batch, double *logdet, int32_t *info,
              double *ws, double *T, double *S, PotrfPost *post, bool sync_cleared) {
    // One launch per 64-column block step with a static shape: replayed as one hipGraph.  The graph writes
    // logdet/info into the workspace tail (fixed addresses -> the cached graph does not depend on where the
    // caller wants them); a tiny kernel outside the graph copies them out.
    const int64_t nbk = padded_dim(n) / 64;
    double *ld_ws = ws + (size_t)batch * nbk * 4096 + DGPAMD_MAXB;
    int32_t *info_ws = reinterpret_cast<int32_t *>(ws + (size_t)batch * nbk * 4096 + 2 * DGPAMD_MAXB);
    int32_t *flags = info_ws + DGPAMD_MAXB;
    // -alpha into row n of the inverse, behind either form of the factorisation
    auto copy_alpha = [&]() {
        hipLaunchKernelGGL(copy_alpha_kernel, dim3((unsigned)((n + 255) / 256), batch), dim3(256), 0, ctx->stream,
                           (const double *)T, S, padded_dim(n), n, stride_a);
        LAUNCH_CHECK(ctx);
        return DGPAMD_OK;
    };
    if (potrf_uses_mega(ctx)) {
        void *syncmem = reinterpret_cast<char *>(ws) + mega_sync_offset(n, batch);
        int rc = potrf_mega_launch(ctx, n, A, T, S, stride_a, batch, ld_ws, info_ws, ws, sync_cleared);
        if (rc) return rc;
        if (T && !post && (rc = copy_alpha())) return rc;
        if (post) {
            post->pending = 1;
            post->ld_ws = ld_ws;
            post->info_ws = info_ws;
            post->status = &reinterpret_cast<MegaSync *>(syncmem)->status;
            post->spare = &reinterpret_cast<MegaSync *>(syncmem)->pad[0];
            return DGPAMD_OK;
        }
        hipLaunchKernelGGL(potrf_copy_out_kernel, dim3(1), dim3(DGPAMD_MAXB), 0, ctx->stream, (const double *)ld_ws,
                           (const int32_t *)info_ws, logdet, info, batch, (const int32_t *)&reinterpret_cast<MegaSync *>(syncmem)->status);
        LAUNCH_CHECK(ctx);
        return DGPAMD_OK;
    }
    TaskTable *tt = nullptr;
    int rc = get_tasks(ctx, (int)nbk, T != nullptr, tt);   // (uploads the table on first use, with the occupancy query: outside the capture)
    if (rc) return rc;
    const std::array<uint64_t, 10> key = {1, (uint64_t)n, (uint64_t)batch, (uint64_t)A, (uint64_t)stride_a, (uint64_t)ws,
                                          (uint64_t)T, (uint64_t)S, 0, 0};
    rc = graph_run(ctx, key, [&]() {
        const int rl = potrf_launches(ctx, n, A, T, S, stride_a, batch, ld_ws, info_ws, ws, flags, tt);
        return rl || !T ? rl : copy_alpha();
    });
    if (rc) return rc;
    hipLaunchKernelGGL(potrf_copy_out_kernel, dim3(1), dim3(DGPAMD_MAXB), 0, ctx->stream, (const double *)ld_ws,
                       (const int32_t *)info_ws, logdet, info, batch, (const int32_t *)nullptr);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_set_potrf_mode(dgpamd_ctx *ctx, int mode) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (mode < 0 || mode > 1) BAD_ARG(ctx, "mode must be 0 (one launch per block step) or 1 (one persistent launch)");
    ctx->potrf_mode = mode;
    return DGPAMD_OK;
}

extern "C" int dgpamd_potrf(dgpamd_ctx *ctx, int64_t n, double *A, int64_t stride_a, int batch, double *logdet,
                            int32_t *info, void *work) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || !A || !logdet || !info || !work) BAD_ARG(ctx, "null pointer or n <= 0");
    if (batch <= 0 || batch > DGPAMD_MAXB) BAD_ARG(ctx, "need 1 <= batch <= DGPAMD_MAXB");
    const int64_t Np = padded_dim(n);
    if (batch > 1 && stride_a < Np * Np) BAD_ARG(ctx, "stride_a < Np*Np");
    return run_potrf(ctx, n, A, stride_a, batch, logdet, info, (double *)work, nullptr, nullptr);
}

extern "C" int dgpamd_potrf_inv(dgpamd_ctx *ctx, int64_t n, double *A, double *T, double *S, int64_t stride_a, int batch,
                                double *logdet, int32_t *info, void *work) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || !A || !T || !S || !logdet || !info || !work) BAD_ARG(ctx, "null pointer or n <= 0");
    if (batch <= 0 || batch > DGPAMD_MAXB) BAD_ARG(ctx, "need 1 <= batch <= DGPAMD_MAXB");
    const int64_t Np = padded_dim(n);
    if (n + 1 > Np) BAD_ARG(ctx, "no room for the right-hand-side row");
    if (batch > 1 && stride_a < Np * Np) BAD_ARG(ctx, "stride_a < Np*Np");
    return run_potrf(ctx, n, A, stride_a, batch, logdet, info, (double *)work, T, S);
}

extern "C" int dgpamd_aug_quad(dgpamd_ctx *ctx, int64_t n, const double *A, int64_t stride_a, int batch, int r,
                               double *quad) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (!A || !quad || r <= 0 || r * r > 256 || n + r > padded_dim(n)) BAD_ARG(ctx, "bad arguments");
    hipLaunchKernelGGL(aug_quad_kernel, dim3(batch), dim3(256), 0, ctx->stream, A, padded_dim(n), stride_a, n, r, quad);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

// out[i] = sum_j A[i][j] x[j]; one wave per row
__global__ __launch_bounds__(256) void gemv_kernel(const double *A, int64_t ld, int64_t rows, int64_t cols, const double *x,
                                                   double *out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= rows) return;
    const double *row = A + i * ld;
    double s = 0.0;
    for (int64_t j = lane; j < cols; j += 64) s = fma(row[j], x[j], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) out[i] = s;
}

extern "C" int dgpamd_gemv(dgpamd_ctx *ctx, int64_t rows, int64_t cols, const double *A, int64_t ld, const double *x,
                           double *out) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (rows <= 0 || cols <= 0 || !A || !x || !out || ld < cols) BAD_ARG(ctx, "bad arguments");
    hipLaunchKernelGGL(gemv_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, ctx->stream, A, ld, rows, cols, x, out);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_trmv_lower(dgpamd_ctx *ctx, int64_t n, const double *L, int64_t stride_a, const double *scale_h,
                                 const double *z, double *out, int batch) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || !L || !z || !out || !scale_h) BAD_ARG(ctx, "null pointer or n <= 0");
    if (batch <= 0 || batch > DGPAMD_MAXB) BAD_ARG(ctx, "need 1 <= batch <= DGPAMD_MAXB");
    TrmvArgs a;
    a.L = L; a.ld = padded_dim(n); a.stride_a = stride_a; a.n = n; a.z = z; a.out = out;
    for (int b = 0; b < batch; ++b) a.sscale[b] = sqrt(scale_h[b]);
    hipLaunchKernelGGL(trmv_lower_kernel, dim3((unsigned)((n + 3) / 4), batch), dim3(256), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

static int potri_launches(dgpamd_ctx *ctx, int64_t n, double *A, double *Ainv, int64_t stride_a, int r, int batch,
                          void *work);

extern "C" int dgpamd_potri_batched(dgpamd_ctx *ctx, int64_t n, double *A, double *Ainv, int64_t stride_a, int r,
                                    int batch, void *work) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n <= 0 || !A || !Ainv || !work || r < 0) BAD_ARG(ctx, "null pointer or n <= 0");
    if (batch <= 0 || batch > DGPAMD_MAXB) BAD_ARG(ctx, "need 1 <= batch <= DGPAMD_MAXB");
    const int64_t Np = padded_dim(n);
    if (n + r > Np) BAD_ARG(ctx, "too many right-hand sides");
    if (batch > 1 && stride_a < Np * Np) BAD_ARG(ctx, "stride_a < Np*Np");
    const std::array<uint64_t, 10> key = {2, (uint64_t)n, (uint64_t)r, (uint64_t)A, (uint64_t)Ainv, (uint64_t)work,
                                          (uint64_t)batch, (uint64_t)stride_a, 0, 0};
    return graph_run(ctx, key, [&]() { return potri_launches(ctx, n, A, Ainv, stride_a, r, batch, work); });
}

extern "C" int dgpamd_potri(dgpamd_ctx *ctx, int64_t n, double *A, double *Ainv, int r, void *work) {
    return dgpamd_potri_batched(ctx, n, A, Ainv, 0, r, 1, work);
}

static int potri_launches(dgpamd_ctx *ctx, int64_t n, double *A, double *Ainv, int64_t stride_a, int r, int batch,
                          void *work) {
    const int64_t Np = padded_dim(n);
    const int nbk = (int)(Np / 64);
    const int64_t stride_ws = (int64_t)nbk * 4096;
    GemmArgs g;
    g.A = A; g.B = Ainv; g.ws = (const double *)work; g.ld = Np; g.stride_a = stride_a; g.stride_ws = stride_ws;
    g.n = n; g.nbk = nbk; g.k = 0; g.s = 0;
    hipLaunchKernelGGL(put_diag_inverse_kernel, dim3(nbk, batch), dim3(256), 0, ctx->stream, A, Np, (const double *)work,
                       stride_a, stride_ws);
    for (int s = 1; s < nbk; s *= 2) {
        const int np = (nbk + 2 * s - 1) / (2 * s);
        g.s = s;
        hipLaunchKernelGGL(tile_gemm_kernel<G_TRTRI1>, dim3(np * s * s, 1, batch), dim3(256), 0, ctx->stream, g);
        hipLaunchKernelGGL(tile_gemm_kernel<G_TRTRI2>, dim3(np * s * s, 1, batch), dim3(256), 0, ctx->stream, g);
    }
    const int nbn = (int)((n + 63) / 64);
    hipLaunchKernelGGL(tile_gemm_kernel<G_LAUUM>, dim3(nbn * (nbn + 1) / 2, 1, batch), dim3(256), 0, ctx->stream, g);
    if (r > 0)
        hipLaunchKernelGGL(copy_aug_rows_kernel, dim3((unsigned)((n + 255) / 256), batch), dim3(256), 0, ctx->stream, A,
                           Ainv, Np, n, r, stride_a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
