// dgpamd_debug_mathfn: the hand-written device math functions of the library on arrays of arguments, one lane per element, for
// tests/test_gpu_mathfn.py.  The kernel calls the functions the hot kernels inline (common.hpp, pathfun.hpp, diagfac.hpp), not
// copies of them; what it sees is each function as compiled in this translation unit (their arithmetic is explicit fma, so the
// operations are those the kernels run).  The two cosine cases are in mathprobe_trig.hip, built as the kernels that use them are.
#include "pathfun.hpp"
#include "diagfac.hpp"
#include "linkfun.hpp"

void mathprobe_launch_trig(dgpamd_ctx *ctx, bool with_sin, int64_t count, const double *a, double *out0, double *out1);

template <int FN>
__global__ __launch_bounds__(256) void mathprobe_kernel(int64_t count, const double *__restrict__ a, double *__restrict__ out0,
                                                        double *__restrict__ out1) {
    __shared__ double etab[EXPN_TAB];
    constexpr bool TAB = FN == DGPAMD_FN_EXP_NEGATED_TAB || FN == DGPAMD_FN_EXP_NEGATED_TAB2 || FN == DGPAMD_FN_EXP_TABLE;
    if (TAB) {   // exactly kmatrix_body's table
        for (int j = threadIdx.x; j < EXPN_TAB; j += 256) etab[j] = exp2((double)j * (1.0 / EXPN_TAB));
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const double x = a[i];
    double r0 = 0.0, r1 = 0.0;
    if (FN == DGPAMD_FN_EXP_NEGATED) r0 = exp_negated(x);
    if (FN == DGPAMD_FN_EXP_NEGATED_V3) r0 = exp_negated_v3(x);
    if (FN == DGPAMD_FN_EXP_NEGATED_TAB) r0 = exp_negated_tab(x, etab);
    if (FN == DGPAMD_FN_EXP_NEGATED_TAB2) {
        double kf, t;
        exp_negated_tab_begin(x, etab, kf, t);
        r0 = exp_negated_tab_end(x, kf, t);
    }
    if (FN == DGPAMD_FN_RSQRT) r0 = rsqrt_f64(x);
    if (FN == DGPAMD_FN_RSQRT_SQRT) rsqrt_sqrt(x, r0, r1);
    if (FN == DGPAMD_FN_RCP) r0 = rcp_f64(x);
    if (FN == DGPAMD_FN_DLOG_MATERN25) r0 = dlog_factor<DGPAMD_MATERN25>(x);
    if (FN == DGPAMD_FN_DLOG_SEXP) r0 = dlog_factor<DGPAMD_SEXP>(x);
    if (FN == DGPAMD_FN_EXP_TABLE) r0 = etab[(int)x & (EXPN_TAB - 1)];
    if (FN == DGPAMD_FN_TRI_DECODE) {
        const int t = (int)x;   // (saturating; tri_decode takes tile indices: t >= 0)
        int bi, bj;
        tri_decode(t < 0 ? 0 : t, bi, bj);
        r0 = (double)bi;
        r1 = (double)bj;
    }
    out0[i] = r0;
    if (out1) out1[i] = r1;
}

extern "C" int dgpamd_debug_mathfn(dgpamd_ctx *ctx, int fn, int64_t count, const double *a, double *out0, double *out1) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (fn < 0 || fn >= DGPAMD_FN_COUNT) BAD_ARG(ctx, "unknown fn");
    if (count <= 0 || count > (int64_t)0x7fffffff * 256) BAD_ARG(ctx, "need 0 < count <= 2^31 * 256");
    const bool two = fn == DGPAMD_FN_COS_SIN_REDUCED || fn == DGPAMD_FN_RSQRT_SQRT || fn == DGPAMD_FN_TRI_DECODE;
    if (!a || !out0 || (two && !out1)) BAD_ARG(ctx, "null pointer");
    const dim3 grid((unsigned)((count + 255) / 256));
#define PROBE(FN) \
    case FN: hipLaunchKernelGGL(mathprobe_kernel<FN>, grid, dim3(256), 0, ctx->stream, count, a, out0, out1); break
    switch (fn) {
        PROBE(DGPAMD_FN_EXP_NEGATED);
        PROBE(DGPAMD_FN_EXP_NEGATED_V3);
        PROBE(DGPAMD_FN_EXP_NEGATED_TAB);
        PROBE(DGPAMD_FN_EXP_NEGATED_TAB2);
        case DGPAMD_FN_COS_REDUCED:
        case DGPAMD_FN_COS_SIN_REDUCED: mathprobe_launch_trig(ctx, fn == DGPAMD_FN_COS_SIN_REDUCED, count, a, out0, out1); break;
        PROBE(DGPAMD_FN_RSQRT);
        PROBE(DGPAMD_FN_RSQRT_SQRT);
        PROBE(DGPAMD_FN_RCP);
        PROBE(DGPAMD_FN_DLOG_MATERN25);
        PROBE(DGPAMD_FN_DLOG_SEXP);
        PROBE(DGPAMD_FN_EXP_TABLE);
        default: PROBE(DGPAMD_FN_TRI_DECODE);
    }
#undef PROBE
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

// dgpamd_debug_linkfn: the Matern-2.5 linked-GP factors of linkfun.hpp on rows of (X1, X2, m, v, l), one lane per row, for
// tests/test_gpu_linkfn.py.  v == 0 takes the product of point correlations, as every caller of these functions does.
template <int FN>
__global__ __launch_bounds__(256) void linkprobe_kernel(int64_t count, const double *__restrict__ args, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const double X1 = args[i * 5], X2 = args[i * 5 + 1], m = args[i * 5 + 2], v = args[i * 5 + 3], l = args[i * 5 + 4];
    double r = 0.0;
    if (FN == DGPAMD_LINK_ERFCX) {
        r = erfcx(X1);
    } else if (FN == DGPAMD_LINK_I) {
        r = matern_I_dim(X1, m, v, l);
    } else if (v == 0.0) {
        const double p = matern_point(m - X1, l);
        r = p * ((FN == DGPAMD_LINK_JD || FN == DGPAMD_LINK_JSEP) ? matern_point(m - X2, l) : p);
    } else if (FN == DGPAMD_LINK_JD) {
        r = matern_Jd(X1, X2, m, v, l);
    } else if (FN == DGPAMD_LINK_JD0) {
        r = matern_Jd0(X1, m, v, l);
    } else {   // the separable form as the pair kernels combine it (the record layout of linkgp.hpp's REC); JSEP0: both roles on one point
        const double lo = FN == DGPAMD_LINK_JSEP ? fmin(X1, X2) : X1, hi = FN == DGPAMD_LINK_JSEP ? fmax(X1, X2) : X1;
        MaternDimConst kc;
        matern_dim_const(m, v, l, kc);
        double S[12], T[15], Sh[12], f2lo, f2hi;
        matern_role_S(lo, kc, S, f2lo);
        matern_role_S(hi, kc, Sh, f2hi);
        matern_role_T(hi, kc, T);
        double o = 0.0, e = 0.0;
        for (int c = 0; c < 12; ++c) o = fma(S[c], T[c], o);
        for (int a = 0; a < 3; ++a) e = fma(S[6 + a], T[12 + a], e);
        r = fma(f2hi - f2lo, e, o);
    }
    out[i] = r;
}

extern "C" int dgpamd_debug_linkfn(dgpamd_ctx *ctx, int fn, int64_t count, const double *args, double *out) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (fn < 0 || fn >= DGPAMD_LINK_COUNT) BAD_ARG(ctx, "unknown fn");
    if (count <= 0 || count > (int64_t)0x7fffffff * 256) BAD_ARG(ctx, "need 0 < count <= 2^31 * 256");
    if (!args || !out) BAD_ARG(ctx, "null pointer");
    const dim3 grid((unsigned)((count + 255) / 256));
#define PROBE(FN) \
    case FN: hipLaunchKernelGGL(linkprobe_kernel<FN>, grid, dim3(256), 0, ctx->stream, count, args, out); break
    switch (fn) {
        PROBE(DGPAMD_LINK_I);
        PROBE(DGPAMD_LINK_JD);
        PROBE(DGPAMD_LINK_JD0);
        PROBE(DGPAMD_LINK_JSEP);
        PROBE(DGPAMD_LINK_JSEP0);
        default: PROBE(DGPAMD_LINK_ERFCX);
    }
#undef PROBE
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
