// Function-valued posterior draws of GP nodes (emulator.sample_functions, gp.sample_functions; DESIGN I.12): a path is
//   f_p(x) = sqrt(scale) ( sqrt(2/F) sum_f theta[p][f] cos(Omega_f . x + b_f) + sum_i v[p][i] c(x, W_g(p)[i]) ),
// a random-Fourier-feature prior draw plus its pathwise (Matheron) update.  dgpamd_pathfun_eval evaluates P paths at M rows
// without storing c(x, W) or the features:
//   shared x   (stride_x == 0: a first-layer node, a gp)  pathfun_mfma_kernel: the 64 x 32 tile of [Phi(x) | c(x, W)] is
//       generated once into LDS and multiplied on v_mfma_f64_16x16x4 with the coefficients of up to 128 paths;
//   per-path x (deeper nodes)                             pathfun_lane_kernel: one lane per row, its scaled coordinates in
//       registers, Omega / W rows staged in LDS and read by broadcast, the sum kept in the lane.
// Both work on x / length: W is staged as W / length and Omega as Omega * length, so one set of registers serves both sums.
// Every output element is a fixed sequence of operations on its own row: results do not depend on which rows share a call.
#include "pathfun.hpp"

// ---------------------------------------------------------------------------
// per-path inputs: workgroup = 256 rows of one path
// ---------------------------------------------------------------------------
template <int KIND, int DT>
__global__ __launch_bounds__(256) void pathfun_lane_kernel(PathfunArgs a) {
    __shared__ __attribute__((aligned(16))) double T[LANE_TR * DT];
    __shared__ double cb[2 * LANE_TR];   // the tile's coefficients, and its phases b
    const int tid = threadIdx.x, p = blockIdx.y, D = a.D;
    const int64_t m = (int64_t)blockIdx.x * 256 + tid;
    double xs[DT];
    {
        const double *xr = a.x + (int64_t)p * a.stride_x + (m < a.M ? m : 0) * D;
#pragma unroll
        for (int d = 0; d < DT; ++d) xs[d] = (d < D && m < a.M) ? xr[d] * a.inv_len[d] : 0.0;
    }
    const double *th = a.theta + (int64_t)p * a.F;
    double accf = 0.0, acck = 0.0;
    for (int64_t f0 = 0; f0 < a.F; f0 += LANE_TR) {
        __syncthreads();
        stage_rows<DT, LANE_TR>(a.Omega, f0, a.F, D, a.len, T, tid);
        if (tid < LANE_TR) {
            const bool in = f0 + tid < a.F;
            cb[tid] = in ? th[f0 + tid] : 0.0;
            cb[LANE_TR + tid] = in ? a.b[f0 + tid] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < LANE_TR; ++r) accf = fma(cb[r], feature_row<DT>(xs, T + r * DT, cb[LANE_TR + r]), accf);
    }
    if (a.n > 0) {
        const double *W = a.W + (int64_t)a.group[p] * a.stride_w, *vp = a.v + (int64_t)p * a.n;
        for (int64_t i0 = 0; i0 < a.n; i0 += LANE_TR) {
            __syncthreads();
            stage_rows<DT, LANE_TR>(W, i0, a.n, D, a.inv_len, T, tid);
            if (tid < LANE_TR) cb[tid] = i0 + tid < a.n ? vp[i0 + tid] : 0.0;
            __syncthreads();
            for (int r = 0; r < LANE_TR; ++r) acck = fma(cb[r], corr_row<KIND, DT>(xs, T + r * DT), acck);
        }
    }
    if (m < a.M) a.out[(int64_t)p * a.M + m] = a.sscale * fma(a.cf, accf, acck);
}

// ---------------------------------------------------------------------------
// shared inputs: workgroup = 64 rows x up to 128 paths; k runs over the F features, then over the n training rows
// ---------------------------------------------------------------------------
#define MFMA_PT 2   // 64-path column tiles per workgroup (the generated tile is used by all of them)

template <int KIND, int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DT <= 16 ? 2 : 1))) void pathfun_mfma_kernel(PathfunArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *T = lds, *bt = T + KC * DT, *As = bt + KC, *Bs0 = As + 64 * LDM;   // rows' tile, phases, generated tile, coefficients
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, D = a.D;
    const int64_t m0 = (int64_t)blockIdx.x * 64, p0 = (int64_t)blockIdx.y * (64 * MFMA_PT);
    const int npt = a.P - p0 > 64 ? MFMA_PT : 1;
    double xs[DT];
    {
        const int64_t m = m0 + lane;
        const double *xr = a.x + (m < a.M ? m : 0) * D;
#pragma unroll
        for (int d = 0; d < DT; ++d) xs[d] = (d < D && m < a.M) ? xr[d] * a.inv_len[d] : 0.0;
    }
    d4 acc[MFMA_PT][4];
#pragma unroll
    for (int pt = 0; pt < MFMA_PT; ++pt)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[pt][t] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int phase = 0; phase < 2; ++phase) {
        const int64_t K = phase == 0 ? a.F : a.n;
        const double *rows = phase == 0 ? a.Omega : a.W, *coef = phase == 0 ? a.theta : a.v;
        for (int64_t k0 = 0; k0 < K; k0 += KC) {
            __syncthreads();
            stage_rows<DT, KC>(rows, k0, K, D, phase == 0 ? a.len : a.inv_len, T, tid);
            if (phase == 0 && tid < KC) bt[tid] = k0 + tid < K ? a.b[k0 + tid] : 0.0;
#pragma unroll
            for (int pt = 0; pt < MFMA_PT; ++pt)
                if (pt < npt) load_coef(coef, K, p0 + 64 * pt, a.P, k0, Bs0 + pt * 64 * LDM, tid);
            __syncthreads();
#pragma unroll 1
            for (int q = 0; q < KC / 4; ++q) {   // wave w generates columns 8w .. 8w + 7 of the rows' tile
                const int k = (KC / 4) * wave + q;
                As[lane * LDM + k] = phase == 0 ? feature_row<DT>(xs, T + k * DT, bt[k]) : corr_row<KIND, DT>(xs, T + k * DT);
            }
            __syncthreads();
#pragma unroll
            for (int pt = 0; pt < MFMA_PT; ++pt)
                if (pt < npt) mfma_tile<OP_MK, OP_MK>(As, Bs0 + pt * 64 * LDM, acc[pt], wave, lane, 1.0);
        }
        if (phase == 0)
#pragma unroll
            for (int pt = 0; pt < MFMA_PT; ++pt)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[pt][t] *= a.cf;
    }
    const int crow = 16 * wave + (lane >> 4), ccol = lane & 15;
#pragma unroll
    for (int pt = 0; pt < MFMA_PT; ++pt)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + crow + 4 * r, p = p0 + 64 * pt + 16 * t + ccol;
                if (m < a.M && p < a.P) a.out[p * a.M + m] = a.sscale * acc[pt][t][r];
            }
}

template <int KIND, int DT>
static int launch_pathfun_mfma(dgpamd_ctx *ctx, PathfunArgs &a, int P) {
    a.P = P;
    const size_t shm = (size_t)(KC * DT + KC + (1 + MFMA_PT) * 64 * LDM) * sizeof(double);   // (67.3 KB at DT = 64)
    const int rc = set_lds(ctx, (const void *)pathfun_mfma_kernel<KIND, DT>, shm);
    if (rc) return rc;
    dim3 grid((unsigned)((a.M + 63) / 64), (unsigned)((P + 64 * MFMA_PT - 1) / (64 * MFMA_PT)));
    hipLaunchKernelGGL((pathfun_mfma_kernel<KIND, DT>), grid, dim3(256), shm, ctx->stream, a);
    return DGPAMD_OK;
}

template <int KIND>
static int dispatch_pathfun(dgpamd_ctx *ctx, PathfunArgs &a, bool shared, const int32_t *group, int P) {
    return pathfun_width(a.D, [&](auto dt) -> int {
        constexpr int DT = decltype(dt)::value;
        if (shared) return launch_pathfun_mfma<KIND, DT>(ctx, a, P);
        launch_lane(ctx, pathfun_lane_kernel<KIND, DT>, a, group, P);
        return DGPAMD_OK;
    });
}

int pathfun_launch_values(dgpamd_ctx *ctx, int kind, PathfunArgs a, bool shared, const int32_t *group, int P) {
    return kind == DGPAMD_SEXP ? dispatch_pathfun<DGPAMD_SEXP>(ctx, a, shared, group, P)
                               : dispatch_pathfun<DGPAMD_MATERN25>(ctx, a, shared, group, P);
}

extern "C" int dgpamd_pathfun_eval(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int D, int64_t F, int P, const double *x,
                                   int64_t stride_x, const int32_t *group_h, int ngroups, const double *W, int64_t stride_w,
                                   const double *Omega, const double *b, const double *theta, const double *v,
                                   const double *length_h, int nlen, double scale, double *out) {
    PathfunArgs a;
    bool shared;
    const int bad = pathfun_args(ctx, __func__, a, shared, kind, n, M, D, F, P, x, stride_x, group_h, ngroups, W, stride_w, Omega, b,
                                 theta, v, length_h, nlen, scale, out, nullptr);
    if (bad) return bad;
    const int rc = pathfun_launch_values(ctx, kind, a, shared, group_h, P);
    if (rc) return rc;
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
