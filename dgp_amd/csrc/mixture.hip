// The exact predictive distribution of a DGP emulator at a point: the equal-weight mixture of the S per-imputation Gaussians
// N(mu_s, var_s) (DESIGN I.15).  cdf / upper tail / log density, quantiles and the CRPS, all f64, for gfx950.
//
// Layout: mu, var (S, count), count = M * K point-outputs, as emulator._layer_moments leaves them; weights 1 / S.  A component with
// var <= 0 is a point mass at mu.  Every output is ONE fixed sequence of operations on the components of its own entry (no
// cross-lane sums; the only atomic counts searches at their limit): a slice of a call reproduces the call bit for bit, and the LDS and the global form of a kernel run
// the same arithmetic on the same numbers (the staged value is sqrt(2 var), the one the global form computes on every read).
#include "common.hpp"

#define MIX_WAVE 64                 // threads of a workgroup: one wave, one (entry, t) or entry per lane
// The staged kernels are the default while eight waves of them fit a CU's LDS (S <= 20): measured faster than re-reading global memory
// at S = 10 (16 waves per CU), slower at S = 50 (3 waves per CU: the erfc chains want the occupancy more than the reads want LDS).
#define MIX_LDS_MAX_BYTES (LDS_CU_BYTES / 8)
#define MIX_QUANTILE_CAP 400        // safeguarded-Newton iterations of a quantile before it is counted in info[0]
#define MIX_INV_SQRT_PI 0.56418958354775628695
#define MIX_LOG_SQRT_PI 0.57236494292470008707

// sqrt(2 var): the component's scale in the variable x = (q - mu) / sqrt(2 var) of erfc; 0 marks a point mass (var <= 0).
__device__ __forceinline__ double mix_scale(double var) { return var > 0.0 ? sqrt(2.0 * var) : 0.0; }

// The components of one entry, read from global memory (mu[s * count + e]) ...
struct CompGlobal {
    const double *mu, *var;
    int64_t count, e;
    __device__ __forceinline__ void get(int s, double &m, double &s2) const {
        m = mu[(int64_t)s * count + e];
        s2 = mix_scale(var[(int64_t)s * count + e]);
    }
};
// ... or from the workgroup's staged copy: lds[(2 s) * 64 + j] = mu, lds[(2 s + 1) * 64 + j] = sqrt(2 var) of its j-th entry.
struct CompLds {
    const double *lds;
    int j;
    __device__ __forceinline__ void get(int s, double &m, double &s2) const {
        m = lds[(2 * s) * MIX_WAVE + j];
        s2 = lds[(2 * s + 1) * MIX_WAVE + j];
    }
};

// Stage the components of entries e0 .. e0 + ne - 1 (ne <= 64), coalesced along count.
__device__ __forceinline__ void mix_stage(double *lds, const double *mu, const double *var, int S, int64_t count, int64_t e0, int ne) {
    for (int idx = threadIdx.x; idx < S * MIX_WAVE; idx += MIX_WAVE) {
        const int s = idx / MIX_WAVE, j = idx % MIX_WAVE;
        if (j < ne) {
            lds[(2 * s) * MIX_WAVE + j] = mu[(int64_t)s * count + e0 + j];
            lds[(2 * s + 1) * MIX_WAVE + j] = mix_scale(var[(int64_t)s * count + e0 + j]);
        }
    }
    __syncthreads();
}

// sum_s Phi((q - mu_s) / sigma_s) (upper: the upper tails) and, with PDF, sum_s phi(.) / sigma_s; a point mass adds the
// right-continuous step (upper tail: its complement) and no density.
template <bool UPPER, bool PDF, typename Comp>
__device__ __forceinline__ void mix_sums(const Comp &c, int S, double q, double &F, double &f) {
    F = 0.0;
    f = 0.0;
    for (int s = 0; s < S; ++s) {
        double m, s2;
        c.get(s, m, s2);
        if (s2 > 0.0) {
            const double x = (q - m) / s2;
            F += 0.5 * erfc(UPPER ? x : -x);
            if (PDF) f += exp_negated(x * x) * (MIX_INV_SQRT_PI / s2);
        } else {
            F += (UPPER ? !(q >= m) : (q >= m)) ? 1.0 : 0.0;
        }
    }
}

// log density by log-sum-exp, the maximum taken first: l_s = -x^2 - log(sqrt(2 var)) - log(sqrt(pi)); -inf without a positive variance.
template <typename Comp>
__device__ __forceinline__ double mix_logpdf(const Comp &c, int S, double q) {
    double top = -INFINITY;
    for (int s = 0; s < S; ++s) {
        double m, s2;
        c.get(s, m, s2);
        if (s2 > 0.0) {
            const double x = (q - m) / s2;
            top = fmax(top, -(x * x) - log(s2));
        }
    }
    if (!(top > -INFINITY)) return isnan(top) ? top : -INFINITY;
    double sum = 0.0;
    for (int s = 0; s < S; ++s) {
        double m, s2;
        c.get(s, m, s2);
        if (s2 > 0.0) {
            const double x = (q - m) / s2;
            sum += exp_negated(top - (-(x * x) - log(s2)));
        }
    }
    return top + (log(sum) - log((double)S) - MIX_LOG_SQRT_PI);
}

// ---- cdf / sf / logpdf: one lane per (entry, t) ------------------------------------------------------------------------------
__global__ __launch_bounds__(MIX_WAVE) void mixture_eval_kernel(int what, int S, int64_t count, int T, const double *mu,
                                                               const double *var, const double *y, int64_t y_stride, double *out) {
    const int64_t g = (int64_t)blockIdx.x * MIX_WAVE + threadIdx.x;
    if (g >= count * T) return;
    const int64_t e = g / T;
    const int t = (int)(g % T);
    const CompGlobal c{mu, var, count, e};
    const double q = y[e * y_stride + t];
    double F, f;
    if (what == DGPAMD_MIX_CDF) {
        mix_sums<false, false>(c, S, q, F, f);
        out[g] = F / (double)S;
    } else if (what == DGPAMD_MIX_SF) {
        mix_sums<true, false>(c, S, q, F, f);
        out[g] = F / (double)S;
    } else {
        out[g] = mix_logpdf(c, S, q);
    }
}

// ---- quantile: one lane per (entry, t) ------------------------------------------------------------------------------------------
// inf{q : F(q) >= p}.  Bracket: a = min_s, b = max_s of mu_s + zp sigma_s (every component's own p-quantile: at a every component
// cdf is <= p, at b every one is >= p).  The search runs on the tail sum G that is small: the lower tails with target p for
// p <= 1/2, the upper tails with target 1 - p (exact) above it -- F(q) >= p is G_upper(q) <= 1 - p -- so the tail is resolved to its
// own relative precision on either side.  Invariant: a below the answer, b at or above it.  Newton steps on log G - log target
// (in a Gaussian tail log G is close to a parabola where G itself is flat) from the last evaluated point, taken only if they
// land strictly inside (a, b), else the midpoint, which is also taken every eighth iteration; one end moves every iteration.
// Done when b - a <= tol = 2^-52 max(|a|, |b|, max_s |mu_s|) or the midpoint is an end; the answer is b.  A Newton step shorter
// than tol / 2 is replaced by a probe 0.75 tol beyond the iterate: it closes the bracket from the side Newton does not come from.
// The bracket's ends come from var itself, fma(zp, sqrt(var), mu): with one component (or S equal ones) that is the answer.
__device__ __forceinline__ void mix_bracket(const double *mu, const double *var, int S, int64_t count, int64_t e, double zp, double &a,
                                            double &b, double &mumax) {
    a = INFINITY;
    b = -INFINITY;
    mumax = 0.0;
    double poison = 0.0;                        // NaN once a component's quantile is NaN or infinite (fmin / fmax would drop it)
    for (int s = 0; s < S; ++s) {
        const double m = mu[(int64_t)s * count + e], v = var[(int64_t)s * count + e];
        const double qs = v > 0.0 ? fma(zp, sqrt(v), m) : m;
        a = fmin(a, qs);
        b = fmax(b, qs);
        mumax = fmax(mumax, fabs(m));
        poison = fma(qs, 0.0, poison);
    }
    a += poison;
    b += poison;
}

template <bool UPPER, typename Comp>
__device__ __forceinline__ double mix_quantile_side(const Comp &c, int S, double target, double a, double b, double mumax, int &capped) {
    const double tS = target * (double)S;
    double G, f;
    mix_sums<UPPER, true>(c, S, a, G, f);
    if (UPPER ? G <= tS : G >= tS) return a;    // (a jump at the lower end, or rounding: a is a lower bound of the answer)
    double q = a + 0.5 * (b - a);
    for (int it = 0; it < MIX_QUANTILE_CAP; ++it) {
        if (!(q > a && q < b)) return b;        // the midpoint is an end: a and b are neighbours
        mix_sums<UPPER, true>(c, S, q, G, f);
        const bool up = UPPER ? G <= tS : G >= tS;
        if (up) b = q; else a = q;
        const double tol = 2.220446049250313e-16 * fmax(fmax(fabs(a), fabs(b)), mumax);
        if (b - a <= tol) return b;
        const double step = (G / f) * log(G / tS);
        double qn = UPPER ? q + step : q - step;
        if (fabs(qn - q) < 0.5 * tol) qn = up ? q - 0.75 * tol : q + 0.75 * tol;
        if (!(qn > a && qn < b) || (it & 7) == 7) qn = a + 0.5 * (b - a);
        q = qn;
    }
    capped = 1;
    return b;
}

template <typename Comp>
__device__ __forceinline__ double mix_quantile(const Comp &c, int S, double p, double a, double b, double mumax, int &capped) {
    capped = 0;
    if (!(a < b)) return b;                     // one component, or S equal ones: its own quantile (a NaN bracket leaves here)
    return p > 0.5 ? mix_quantile_side<true>(c, S, 1.0 - p, a, b, mumax, capped) : mix_quantile_side<false>(c, S, p, a, b, mumax, capped);
}

struct MixProbs {   // the call's probabilities and their standard normal quantiles, by value in the kernel arguments
    double p[DGPAMD_MIX_MAXT], zp[DGPAMD_MIX_MAXT];
};

template <bool LDS>
__global__ __launch_bounds__(MIX_WAVE) void mixture_quantile_kernel(int S, int64_t count, int T, const double *mu, const double *var,
                                                                   MixProbs pr, double *out, int32_t *info) {
    extern __shared__ __attribute__((aligned(16))) double mix_lds[];
    const int64_t g0 = (int64_t)blockIdx.x * MIX_WAVE, total = count * T;
    const int64_t g = g0 + threadIdx.x;
    const int64_t e0 = g0 / T;
    if (LDS) {
        const int64_t glast = (g0 + MIX_WAVE - 1 < total ? g0 + MIX_WAVE - 1 : total - 1);
        mix_stage(mix_lds, mu, var, S, count, e0, (int)(glast / T - e0) + 1);
    }
    if (g >= total) return;
    const int64_t e = g / T;
    const int t = (int)(g % T);
    int capped;
    double q, a, b, mumax;
    mix_bracket(mu, var, S, count, e, pr.zp[t], a, b, mumax);
    if (LDS) q = mix_quantile(CompLds{mix_lds, (int)(e - e0)}, S, pr.p[t], a, b, mumax, capped);
    else q = mix_quantile(CompGlobal{mu, var, count, e}, S, pr.p[t], a, b, mumax, capped);
    out[g] = q;
    if (capped) atomicAdd(info, 1);
}

// ---- CRPS: one lane per entry -------------------------------------------------------------------------------------------------------
// A(m, v) = 2 sqrt(v) phi(m / sqrt(v)) + m (2 Phi(m / sqrt(v)) - 1) = E|N(m, v)|; both terms are >= 0 (2 Phi - 1 = erf(x), x = m / sqrt(2 v)).
__device__ __forceinline__ double mix_A(double m, double s2) {
    if (!(s2 > 0.0)) return fabs(m);
    const double x = m / s2;
    return fma(s2 * MIX_INV_SQRT_PI, exp_negated(x * x), m * erf(x));
}

// CRPS = (1/S) sum_s A(y - mu_s, var_s) - (1 / 2S^2) [sum_s A(0, 2 var_s) + 2 sum_{s<t} A(mu_s - mu_t, var_s + var_t)], summed in
// that order (s ascending, t ascending inside).  sqrt(2 (var_s + var_t)) = sqrt(s2_s^2 + s2_t^2) from the staged scales.
template <typename Comp>
__device__ __forceinline__ double mix_crps(const Comp &c, int S, double y) {
    double first = 0.0, diag = 0.0, pairs = 0.0;
    for (int s = 0; s < S; ++s) {
        double ms, ss;
        c.get(s, ms, ss);
        first += mix_A(y - ms, ss);
        diag += mix_A(0.0, sqrt(2.0) * ss);
        for (int t = s + 1; t < S; ++t) {
            double mt, st;
            c.get(t, mt, st);
            pairs += mix_A(ms - mt, sqrt(fma(ss, ss, st * st)));
        }
    }
    const double dS = (double)S;
    return first / dS - (diag + 2.0 * pairs) / (2.0 * dS * dS);
}

template <bool LDS>
__global__ __launch_bounds__(MIX_WAVE) void mixture_crps_kernel(int S, int64_t count, const double *mu, const double *var,
                                                               const double *y, double *out) {
    extern __shared__ __attribute__((aligned(16))) double mix_lds[];
    const int64_t e0 = (int64_t)blockIdx.x * MIX_WAVE;
    const int64_t e = e0 + threadIdx.x;
    if (LDS) mix_stage(mix_lds, mu, var, S, count, e0, (int)(count - e0 < MIX_WAVE ? count - e0 : MIX_WAVE));
    if (e >= count) return;
    if (LDS) out[e] = mix_crps(CompLds{mix_lds, (int)threadIdx.x}, S, y[e]);
    else out[e] = mix_crps(CompGlobal{mu, var, count, e}, S, y[e]);
}

// ---- C entries -------------------------------------------------------------------------------------------------------------------------
static inline size_t mix_lds_bytes(int S) { return (size_t)S * 2 * MIX_WAVE * sizeof(double); }

// 1 the staged kernel, 0 the one that re-reads global memory; `path` 0 lets the size decide, 1 / 2 ask for LDS / global.
static int mix_choose(dgpamd_ctx *ctx, int S, int path, int *lds) {
    if (path < 0 || path > 2) BAD_ARG(ctx, "path must be 0 (by size), 1 (LDS) or 2 (global)");
    if (path == 1 && mix_lds_bytes(S) > LDS_CU_BYTES) BAD_ARG(ctx, "path 1 (LDS) needs S <= 160");
    *lds = path == 1 || (path == 0 && mix_lds_bytes(S) <= MIX_LDS_MAX_BYTES);
    return DGPAMD_OK;
}

static int mix_blocks(dgpamd_ctx *ctx, int64_t lanes, unsigned *blocks) {
    const int64_t nb = (lanes + MIX_WAVE - 1) / MIX_WAVE;
    if (nb > 0x7fffffffLL) BAD_ARG(ctx, "count * T is beyond 2^37");
    *blocks = (unsigned)nb;
    return DGPAMD_OK;
}

extern "C" int dgpamd_mixture_eval(dgpamd_ctx *ctx, int what, int S, int64_t count, int T, const double *mu, const double *var,
                                   const double *y, int64_t y_stride, double *out) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (what != DGPAMD_MIX_CDF && what != DGPAMD_MIX_SF && what != DGPAMD_MIX_LOGPDF) BAD_ARG(ctx, "what must be DGPAMD_MIX_CDF, _SF or _LOGPDF");
    if (S < 1 || T < 1 || count < 0) BAD_ARG(ctx, "need S >= 1, T >= 1, count >= 0");
    if (y_stride != 0 && y_stride != T) BAD_ARG(ctx, "y_stride must be T (y per entry) or 0 (shared thresholds)");
    if (count == 0) return DGPAMD_OK;
    if (!mu || !var || !y || !out) BAD_ARG(ctx, "null pointer");
    unsigned blocks;
    if (int rc = mix_blocks(ctx, count * T, &blocks)) return rc;
    hipLaunchKernelGGL(mixture_eval_kernel, dim3(blocks), dim3(MIX_WAVE), 0, ctx->stream, what, S, count, T, mu, var, y, y_stride, out);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_mixture_quantile(dgpamd_ctx *ctx, int S, int64_t count, int T, const double *mu, const double *var,
                                       const double *p, const double *zp, int path, double *out, int32_t *info) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (S < 1 || T < 1 || count < 0) BAD_ARG(ctx, "need S >= 1, T >= 1, count >= 0");
    if (T > DGPAMD_MIX_MAXT) BAD_ARG(ctx, "at most DGPAMD_MIX_MAXT probabilities per call");
    if (!p || !zp) BAD_ARG(ctx, "null pointer");
    for (int t = 0; t < T; ++t)
        if (!(p[t] > 0.0 && p[t] < 1.0) || !(zp[t] > -40.0 && zp[t] < 40.0)) BAD_ARG(ctx, "need 0 < p < 1 and zp its standard normal quantile");
    int lds;
    if (int rc = mix_choose(ctx, S, path, &lds)) return rc;
    if (count == 0) return DGPAMD_OK;
    if (!mu || !var || !out || !info) BAD_ARG(ctx, "null pointer");
    unsigned blocks;
    if (int rc = mix_blocks(ctx, count * T, &blocks)) return rc;
    MixProbs pr;
    memset(&pr, 0, sizeof(pr));
    for (int t = 0; t < T; ++t) pr.p[t] = p[t], pr.zp[t] = zp[t];
    HIP_TRY(ctx, hipMemsetAsync(info, 0, sizeof(int32_t), ctx->stream));
    if (lds) {
        if (int rc = set_lds(ctx, (const void *)mixture_quantile_kernel<true>, mix_lds_bytes(S))) return rc;
        hipLaunchKernelGGL(mixture_quantile_kernel<true>, dim3(blocks), dim3(MIX_WAVE), mix_lds_bytes(S), ctx->stream, S, count, T, mu, var,
                           pr, out, info);
    } else {
        hipLaunchKernelGGL(mixture_quantile_kernel<false>, dim3(blocks), dim3(MIX_WAVE), 0, ctx->stream, S, count, T, mu, var, pr,
                           out, info);
    }
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_mixture_crps(dgpamd_ctx *ctx, int S, int64_t count, const double *mu, const double *var, const double *y,
                                   int path, double *out) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (S < 1 || count < 0) BAD_ARG(ctx, "need S >= 1, count >= 0");
    int lds;
    if (int rc = mix_choose(ctx, S, path, &lds)) return rc;
    if (count == 0) return DGPAMD_OK;
    if (!mu || !var || !y || !out) BAD_ARG(ctx, "null pointer");
    unsigned blocks;
    if (int rc = mix_blocks(ctx, count, &blocks)) return rc;
    if (lds) {
        if (int rc = set_lds(ctx, (const void *)mixture_crps_kernel<true>, mix_lds_bytes(S))) return rc;
        hipLaunchKernelGGL(mixture_crps_kernel<true>, dim3(blocks), dim3(MIX_WAVE), mix_lds_bytes(S), ctx->stream, S, count, mu, var, y, out);
    } else {
        hipLaunchKernelGGL(mixture_crps_kernel<false>, dim3(blocks), dim3(MIX_WAVE), 0, ctx->stream, S, count, mu, var, y, out);
    }
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
