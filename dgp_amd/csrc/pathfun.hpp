// Generation code shared by the values of function-valued posterior draws (pathfun.hip, DESIGN I.12) and their input gradients
// (pathfun_grad.hip, DESIGN I.13): the cosine, the rows of features and correlations, the staging of Omega / W tiles and of the
// coefficients, the argument block, and on the host the choice of the compiled width and the lane kernels' launches.  Both files
// generate the values with exactly this code, in the same order over k: the values dgpamd_pathfun_grad returns are
// dgpamd_pathfun_eval's bit for bit.
#pragma once
#include "common.hpp"
#include "tile.hpp"

#include <math.h>
#include <type_traits>

#ifndef PATHFUN_LIBM_COS
#define PATHFUN_LIBM_COS 0   // 1: the library's cos in place of cos_reduced (A/B builds of tools/gpu_pathfun_bench.py)
#endif

// cos(a) = sin(a + pi/2) = (-1)^k sin(r), k = round(a / pi + 1/2), r = a - (k - 1/2) pi in [-pi/2, pi/2].  The reduction is two
// fused multiply-adds against pi = PI_HI + PI_LO (each rounds a value below 1.6 once: |error of r| <= 2^-52 for |a| < 2^30, where
// (k - 1/2) PI_HI is still exact inside the fma and (k - 1/2) times the 1e-33 left of pi is nothing); sin is its Taylor polynomial
// to r^21 (the r^23 term is 1.3e-18 at pi/2).  k's parity is the low bit of the "1.5 * 2^52" sum, as in exp_negated.  Arguments of
// 2^30 and beyond (and NaN) go to the library's cos.
// WITH_SIN: *msin = -sin(a) from the same r and k: sin(a) = (-1)^k sin(r - pi/2) = -(-1)^k cos(r), so -sin(a) = (-1)^k cos(r), cos(r)
// its Taylor polynomial to r^24 (the r^26 term is 3e-22 at pi/2).  The cosine's own operations are the same with and without it.
template <bool WITH_SIN>
__device__ __forceinline__ double cos_reduced_impl(double a, double *msin) {
#if PATHFUN_LIBM_COS
    if (WITH_SIN) *msin = -sin(a);
    return cos(a);
#else
    if (!(fabs(a) < 1073741824.0)) {
        if (WITH_SIN) *msin = -sin(a);
        return cos(a);
    }
    const double MAGIC = 6755399441055744.0;   // 1.5 * 2^52
    const double kf = fma(a, 3.18309886183790671538e-01, 0.5) + MAGIC;
    const double h = (kf - MAGIC) - 0.5;
    double r = fma(-h, 3.14159265358979311600e+00, a);
    r = fma(-h, 1.22464679914735317723e-16, r);
    const double s = r * r;
    const int flip = (int)((unsigned)__double2loint(kf) << 31);
    if (WITH_SIN) {
        double q = 1.61173757109611840000e-24;           //  1/24!
        q = fma(q, s, -8.89679139245057328675e-22);       // -1/22!
        q = fma(q, s, 4.11031762331216485848e-19);        //  1/20!
        q = fma(q, s, -1.56192069685862264622e-16);       // -1/18!
        q = fma(q, s, 4.77947733238738529744e-14);        //  1/16!
        q = fma(q, s, -1.14707455977297247139e-11);       // -1/14!
        q = fma(q, s, 2.08767569878680989792e-09);        //  1/12!
        q = fma(q, s, -2.75573192239858906526e-07);       // -1/10!
        q = fma(q, s, 2.48015873015873015873e-05);        //  1/8!
        q = fma(q, s, -1.38888888888888888889e-03);       // -1/6!
        q = fma(q, s, 4.16666666666666666667e-02);        //  1/4!
        q = fma(q, s, -0.5);
        q = fma(q, s, 1.0);
        *msin = __hiloint2double(__double2hiint(q) ^ flip, __double2loint(q));
    }
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
    return __hiloint2double(__double2hiint(v) ^ flip, __double2loint(v));
#endif
}
__device__ __forceinline__ double cos_reduced(double a) { return cos_reduced_impl<false>(a, nullptr); }

// q(t) = d log(factor) / dt of one dimension's factor of the correlation, t the scaled difference (pathfun_grad.hip)
template <int KIND>
__device__ __forceinline__ double dlog_factor(double t) {
    if (KIND == DGPAMD_SEXP) return -2.0 * t;
    const double r = fabs(t);
    const double poly = fma(r, fma(r, 5.0 / 3.0, SQRT5), 1.0), lin = fma(r, SQRT5, 1.0);
    double y = __builtin_amdgcn_rcp(poly);
    y = fma(fma(-poly, y, 1.0), y, y);
    y = fma(fma(-poly, y, 1.0), y, y);
    return (-5.0 / 3.0 * t) * (lin * y);
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
__device__ __forceinline__ double feature_arg(const double (&xs)[DT], const double *__restrict__ om, double b) {
    double a = b;
#pragma unroll
    for (int d = 0; d < DT; ++d) a = fma(om[d], xs[d], a);
    return a;
}
template <int DT>
__device__ __forceinline__ double feature_row(const double (&xs)[DT], const double *__restrict__ om, double b) {
    return cos_reduced(feature_arg<DT>(xs, om, b));
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
    double *out_g;               // P x M x D (dgpamd_pathfun_grad)
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

#define LANE_TR 64   // Omega / W rows per staged tile of the lane kernels (32 KB at DT = 64)

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

// The argument checks and the argument block of dgpamd_pathfun_eval and dgpamd_pathfun_grad (fn: the entry's name for the message;
// out_g is null for the values alone).
#define PATHFUN_BAD(msg)                                           \
    do {                                                           \
        snprintf(ctx->err, sizeof(ctx->err), "%s: %s", fn, msg);   \
        return DGPAMD_BAD_ARG;                                     \
    } while (0)
static inline int pathfun_args(dgpamd_ctx *ctx, const char *fn, PathfunArgs &a, bool &shared, int kind, int64_t n, int64_t M, int D,
                               int64_t F, int P, const double *x, int64_t stride_x, const int32_t *group_h, int ngroups,
                               const double *W, int64_t stride_w, const double *Omega, const double *b, const double *theta,
                               const double *v, const double *length_h, int nlen, double scale, double *out, double *out_g) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (n < 0 || M <= 0 || F <= 0 || P <= 0 || !x || !Omega || !b || !theta || !length_h || !out)
        PATHFUN_BAD("null pointer or empty problem");
    if (n > 0 && (!W || !v)) PATHFUN_BAD("n > 0 needs W and v");
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) PATHFUN_BAD("kind must be 0 or 1");
    if (D <= 0 || D > DGPAMD_MAXD || (nlen != 1 && nlen != D)) PATHFUN_BAD("bad D / nlen");
    if (!(scale >= 0.0)) PATHFUN_BAD("scale must be non-negative");
    if (ngroups <= 0) PATHFUN_BAD("need ngroups >= 1");
    if (stride_x != 0 && stride_x < M * D) PATHFUN_BAD("stride_x must be 0 (shared inputs) or at least M * D");
    if (M > (int64_t)0x7fffffff * 64) PATHFUN_BAD("too many rows for one call");
    shared = stride_x == 0;
    for (int p = 0; p < P; ++p) {
        const int g = group_h ? group_h[p] : 0;
        if (g < 0 || g >= ngroups) PATHFUN_BAD("group index out of range");
        if (shared && g != (group_h ? group_h[0] : 0)) PATHFUN_BAD("shared inputs (stride_x == 0) need one group for every path");
    }
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
    a.out = out; a.out_g = out_g;
    memset(a.group, 0, sizeof(a.group));
    return DGPAMD_OK;
}
#undef PATHFUN_BAD

// fn(std::integral_constant<int, DT>) at the narrowest compiled width DT >= D.  The rows are padded with zero columns to that width
// (a zero column changes neither sum; the work grows with the padded width).  Powers of two, plus 6 and 10: the bench model's first
// layer has 5 inputs and its output node 5 + 5, and a DGP node behind layer 1 sees (nodes below) + (connected inputs) columns,
// typically in this range.
template <class Fn>
static inline int pathfun_width(int D, Fn fn) {
    if (D <= 2) return fn(std::integral_constant<int, 2>());
    else if (D <= 4) return fn(std::integral_constant<int, 4>());
    else if (D <= 6) return fn(std::integral_constant<int, 6>());
    else if (D <= 8) return fn(std::integral_constant<int, 8>());
    else if (D <= 10) return fn(std::integral_constant<int, 10>());
    else if (D <= 16) return fn(std::integral_constant<int, 16>());
    else if (D <= 32) return fn(std::integral_constant<int, 32>());
    return fn(std::integral_constant<int, 64>());
}

// A lane kernel (one lane per row, blockIdx.y the path) over P paths: the groups travel by value, DGPAMD_MAXB paths per launch.
static inline void launch_lane(dgpamd_ctx *ctx, void (*kernel)(PathfunArgs), PathfunArgs a, const int32_t *group, int P) {
    const PathfunArgs all = a;
    for (int q0 = 0; q0 < P; q0 += DGPAMD_MAXB) {
        const int pc = P - q0 < DGPAMD_MAXB ? P - q0 : DGPAMD_MAXB;
        a.P = pc;
        a.x = all.x + (int64_t)q0 * a.stride_x;
        a.theta = all.theta + (int64_t)q0 * a.F;
        a.v = all.v ? all.v + (int64_t)q0 * a.n : nullptr;
        a.out = all.out ? all.out + (int64_t)q0 * a.M : nullptr;
        a.out_g = all.out_g ? all.out_g + (int64_t)q0 * a.M * a.D : nullptr;
        for (int q = 0; q < pc; ++q) a.group[q] = group ? group[q0 + q] : 0;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((a.M + 255) / 256), (unsigned)pc), dim3(256), 0, ctx->stream, a);
    }
}

// The launches of dgpamd_pathfun_eval for a filled argument block (pathfun.hip): dgpamd_pathfun_grad takes its values from here
// where its own kernel would sum them in another order (shared x beyond the widths of its matrix form).
int pathfun_launch_values(dgpamd_ctx *ctx, int kind, PathfunArgs a, bool shared, const int32_t *group, int P);
