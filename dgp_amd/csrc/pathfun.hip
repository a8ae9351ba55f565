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
#include "common.hpp"
#include "tile.hpp"

#include <math.h>

#ifndef PATHFUN_LIBM_COS
#define PATHFUN_LIBM_COS 0   // 1: the library's cos in place of cos_reduced (A/B builds of tools/gpu_pathfun_bench.py)
#endif

// cos(a) = sin(a + pi/2) = (-1)^k sin(r), k = round(a / pi + 1/2), r = a - (k - 1/2) pi in [-pi/2, pi/2].  The reduction is two
// fused multiply-adds against pi = PI_HI + PI_LO (each rounds a value below 1.6 once: |error of r| <= 2^-52 for |a| < 2^30, where
// (k - 1/2) PI_HI is still exact inside the fma and (k - 1/2) times the 1e-33 left of pi is nothing); sin is its Taylor polynomial
// to r^21 (the r^23 term is 1.3e-18 at pi/2).  k's parity is the low bit of the "1.5 * 2^52" sum, as in exp_negated.  Arguments of
// 2^30 and beyond (and NaN) go to the library's cos.
__device__ __forceinline__ double cos_reduced(double a) {
#if PATHFUN_LIBM_COS
    return cos(a);
#else
    if (!(fabs(a) < 1073741824.0)) return cos(a);
    const double MAGIC = 6755399441055744.0;   // 1.5 * 2^52
    const double kf = fma(a, 3.18309886183790671538e-01, 0.5) + MAGIC;
    const double h = (kf - MAGIC) - 0.5;
    double r = fma(-h, 3.14159265358979311600e+00, a);
    r = fma(-h, 1.22464679914735317723e-16, r);
    const double s = r * r;
    double p = 1.95729410633912612308e-20;            //  1/21!
    p = fma(p, s, -8.22063524662432971696e-18);       // -1/19!
    p = fma(p, s, 2.81145725434552076320e-15);        //  1/17!
    p = fma(p, s, -7.64716373181981647590e-13);       // -1/15!
    p = fma(p, s, 1.60590438368216145994e-10);        //  1/13!
    p = fma(p, s, -2.50521083854417187751e-08);       // -1/11!
    p = fma(p, s, 2.75573192239858906526e-06);        //  1/9!
    p = fma(p, s, -1.98412698412698412698e-04);       // -1/7!
    p = fma(p, s, 8.33333333333333333333e-03);        //  1/5!
    p = fma(p, s, -1.66666666666666666667e-01);       // -1/3!
    const double v = fma(r * s, p, r);
    return __hiloint2double(__double2hiint(v) ^ ((int)((unsigned)__double2loint(kf) << 31)), __double2loint(v));
#endif
}

// c(x, w) from the scaled rows xs (registers) and w (LDS, read by broadcast)
template <int KIND, int DT>
__device__ __forceinline__ double corr_row(const double (&xs)[DT], const double *__restrict__ w) {
    double s = 0.0, pr = 1.0;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        const double df = xs[d] - w[d];
        if (KIND == DGPAMD_SEXP)
            corr_accum_sexp(df, s);
        else
            corr_accum_matern(df, pr, s);
    }
    return (KIND == DGPAMD_SEXP) ? exp_negated(s) : pr * exp_negated(SQRT5 * s);
}
template <int DT>
__device__ __forceinline__ double feature_row(const double (&xs)[DT], const double *__restrict__ om, double b) {
    double a = b;
#pragma unroll
    for (int d = 0; d < DT; ++d) a = fma(om[d], xs[d], a);
    return cos_reduced(a);
}

struct PathfunArgs {
    int D, P;
    int64_t n, M, F;
    double inv_len[DGPAMD_MAXD], len[DGPAMD_MAXD];
    const double *x;
    int64_t stride_x;            // between the paths' inputs (lane kernel)
    const double *W;
    int64_t stride_w;            // between the groups' training inputs
    const double *Omega, *b;     // F x D, F
    const double *theta, *v;     // P x F, P x n
    double cf, sscale;           // sqrt(2 / F), sqrt(scale)
    double *out;                 // P x M
    int32_t group[DGPAMD_MAXB];  // lane kernel: the group of each path of the launch
};

// rows r0 .. r0 + TR - 1 of src (ld D) times mul[d] into T[TR][DT]; rows >= nrows and columns >= D read as zero
template <int DT, int TR>
__device__ __forceinline__ void stage_rows(const double *__restrict__ src, int64_t r0, int64_t nrows, int D,
                                           const double *mul, double *__restrict__ T, int tid) {
    for (int idx = tid; idx < TR * DT; idx += 256) {
        const int row = idx / DT, d = idx - row * DT;
        T[idx] = (d < D && r0 + row < nrows) ? src[(r0 + row) * D + d] * mul[d] : 0.0;
    }
}

// ---------------------------------------------------------------------------
// per-path inputs: workgroup = 256 rows of one path
// ---------------------------------------------------------------------------
#define LANE_TR 64   // Omega / W rows per staged tile (32 KB at DT = 64)

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

// coefficient half tile in MK form: rows = paths p0 .. p0 + 63 (limit P), columns k0 .. k0 + 31 (limit K) of C (ld K)
__device__ __forceinline__ void load_coef(const double *__restrict__ C, int64_t K, int64_t p0, int P, int64_t k0,
                                          double *__restrict__ s, int tid) {
    const int c2 = (tid & 15) * 2;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int r = (tid >> 4) + 16 * it;
        const int64_t p = p0 + r, k = k0 + c2;
        s[r * LDM + c2] = (p < P && k < K) ? C[p * K + k] : 0.0;
        s[r * LDM + c2 + 1] = (p < P && k + 1 < K) ? C[p * K + k + 1] : 0.0;
    }
}

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
static int launch_pathfun(dgpamd_ctx *ctx, PathfunArgs &a, bool shared, const int32_t *group, int P) {
    if (shared) {
        a.P = P;
        const size_t shm = (size_t)(KC * DT + KC + (1 + MFMA_PT) * 64 * LDM) * sizeof(double);   // (67.3 KB at DT = 64)
        const int rc = set_lds(ctx, (const void *)pathfun_mfma_kernel<KIND, DT>, shm);
        if (rc) return rc;
        dim3 grid((unsigned)((a.M + 63) / 64), (unsigned)((P + 64 * MFMA_PT - 1) / (64 * MFMA_PT)));
        hipLaunchKernelGGL((pathfun_mfma_kernel<KIND, DT>), grid, dim3(256), shm, ctx->stream, a);
        return DGPAMD_OK;
    }
    const double *x = a.x, *theta = a.theta, *v = a.v;
    double *out = a.out;
    for (int q0 = 0; q0 < P; q0 += DGPAMD_MAXB) {   // (the groups travel by value: DGPAMD_MAXB paths per launch)
        const int pc = P - q0 < DGPAMD_MAXB ? P - q0 : DGPAMD_MAXB;
        a.P = pc;
        a.x = x + (int64_t)q0 * a.stride_x;
        a.theta = theta + (int64_t)q0 * a.F;
        a.v = v ? v + (int64_t)q0 * a.n : nullptr;
        a.out = out + (int64_t)q0 * a.M;
        for (int q = 0; q < pc; ++q) a.group[q] = group ? group[q0 + q] : 0;
        hipLaunchKernelGGL((pathfun_lane_kernel<KIND, DT>), dim3((unsigned)((a.M + 255) / 256), (unsigned)pc), dim3(256), 0,
                           ctx->stream, a);
    }
    return DGPAMD_OK;
}

template <int KIND>
static int dispatch_pathfun(dgpamd_ctx *ctx, PathfunArgs &a, bool shared, const int32_t *group, int P) {
    // The rows are padded with zero columns to the next width compiled (a zero column changes neither sum; the work grows with the
    // padded width).  Powers of two, plus 6 and 10: the bench model's first layer has 5 inputs and its output node 5 + 5, and a DGP
    // node behind layer 1 sees (nodes below) + (connected inputs) columns, typically in this range.
    if (a.D <= 2) return launch_pathfun<KIND, 2>(ctx, a, shared, group, P);
    else if (a.D <= 4) return launch_pathfun<KIND, 4>(ctx, a, shared, group, P);
    else if (a.D <= 6) return launch_pathfun<KIND, 6>(ctx, a, shared, group, P);
    else if (a.D <= 8) return launch_pathfun<KIND, 8>(ctx, a, shared, group, P);
    else if (a.D <= 10) return launch_pathfun<KIND, 10>(ctx, a, shared, group, P);
    else if (a.D <= 16) return launch_pathfun<KIND, 16>(ctx, a, shared, group, P);
    else if (a.D <= 32) return launch_pathfun<KIND, 32>(ctx, a, shared, group, P);
    return launch_pathfun<KIND, 64>(ctx, a, shared, group, P);
}

extern "C" int dgpamd_pathfun_eval(dgpamd_ctx *ctx, int kind, int64_t n, int64_t M, int D, int64_t F, int P, const double *x,
                                   int64_t stride_x, const int32_t *group_h, int ngroups, const double *W, int64_t stride_w,
                                   const double *Omega, const double *b, const double *theta, const double *v,
                                   const double *length_h, int nlen, double scale, double *out) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n < 0 || M <= 0 || F <= 0 || P <= 0 || !x || !Omega || !b || !theta || !length_h || !out)
        BAD_ARG(ctx, "null pointer or empty problem");
    if (n > 0 && (!W || !v)) BAD_ARG(ctx, "n > 0 needs W and v");
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) BAD_ARG(ctx, "kind must be 0 or 1");
    if (D <= 0 || D > DGPAMD_MAXD || (nlen != 1 && nlen != D)) BAD_ARG(ctx, "bad D / nlen");
    if (!(scale >= 0.0)) BAD_ARG(ctx, "scale must be non-negative");
    if (ngroups <= 0) BAD_ARG(ctx, "need ngroups >= 1");
    if (stride_x != 0 && stride_x < M * D) BAD_ARG(ctx, "stride_x must be 0 (shared inputs) or at least M * D");
    if (M > (int64_t)0x7fffffff * 64) BAD_ARG(ctx, "too many rows for one call");
    const bool shared = stride_x == 0;
    for (int p = 0; p < P; ++p) {
        const int g = group_h ? group_h[p] : 0;
        if (g < 0 || g >= ngroups) BAD_ARG(ctx, "group index out of range");
        if (shared && g != (group_h ? group_h[0] : 0)) BAD_ARG(ctx, "shared inputs (stride_x == 0) need one group for every path");
    }
    PathfunArgs a;
    a.D = D; a.P = P; a.n = n; a.M = M; a.F = F;
    for (int d = 0; d < DGPAMD_MAXD; ++d) {
        a.len[d] = d < D ? length_h[nlen == 1 ? 0 : d] : 0.0;
        a.inv_len[d] = d < D ? 1.0 / a.len[d] : 0.0;
    }
    a.x = x; a.stride_x = stride_x;
    a.W = (shared && W && group_h) ? W + (int64_t)group_h[0] * stride_w : W;
    a.stride_w = stride_w;
    a.Omega = Omega; a.b = b; a.theta = theta; a.v = v;
    a.cf = sqrt(2.0 / (double)F); a.sscale = sqrt(scale);
    a.out = out;
    memset(a.group, 0, sizeof(a.group));
    const int rc = kind == DGPAMD_SEXP ? dispatch_pathfun<DGPAMD_SEXP>(ctx, a, shared, group_h, P)
                                       : dispatch_pathfun<DGPAMD_MATERN25>(ctx, a, shared, group_h, P);
    if (rc) return rc;
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
