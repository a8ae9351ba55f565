// What the batched chains over one box share (boxmala.hip, DESIGN I.19; boxhmc.hip, DESIGN I.20), every shared step written
// once: the arguments of a call, the layout of par and of a chain's state inside the workspace, the target and its gradient at
// the trial point, INIT, the commit of an accepted trial, the tally of a decision with the step's adaptation, the sample
// store, the hold of a chain that does not move, and on the host the argument checks and the launch.
// boxsmc.hip (DESIGN I.21) builds its tempered move on the lane, the commit, the tally, the hold and the argument checks.
//
// Q independent chains, each sampling x in lo <= x <= hi, D <= 64 columns, from
//   lp(x) = -1/2 sum_k w_k (ybar_k - f_k(x))^2 - 1/2 sum_d pv_d (x_d - pm_d)^2.
// One lane per chain, workgroups of one wave.  Every state field lies (field..., Q), chain fastest: the lanes of a wave read
// and write consecutive doubles.  The loops over D and K run over global memory -- a per-lane array with a runtime index
// would live in scratch.  No LDS, no cross-lane operation, no atomics: a chain's iterates are one fixed sequence of operations
// on its own inputs, whatever shares its wave.
// All three files are compiled with -ffp-contract=off (csrc/Makefile): every product is rounded before it enters a sum, every
// sum runs in index order, and the kernels use + - * / and comparisons alone, so they perform the operations of their numpy
// restatements (tests/boxmala_ref.py, whose target tests/boxhmc_ref.py inherits and tests/boxsmc_ref.py tempers) one for one.
// The operand order and the parentheses of every expression here are those roundings: they do not move.  Everything on the
// device is forced inline, as in wave.hpp: a kernel compiles to what it did with a copy of its own.
#pragma once
#include <math.h>

#include "common.hpp"

static_assert(DGPAMD_BOXMALA_OK == DGPAMD_BOXHMC_OK && DGPAMD_BOXMALA_NAN == DGPAMD_BOXHMC_NAN &&
                  DGPAMD_BOXMALA_COUNT == DGPAMD_BOXHMC_COUNT,
              "the two chain steps share their status values");
#define BOXCHAIN_OK DGPAMD_BOXMALA_OK
#define BOXCHAIN_NAN DGPAMD_BOXMALA_NAN

struct BoxchainArgs {
    int64_t Q;
    int D, K, first, last, adapt, slot;               // (last: boxhmc alone)
    double h0, hmin, hmax, up, down;
    const double *f, *J, *par, *z, *logu;
    double *ws, *x_trial, *h, *logr, *xs, *lps;
    int32_t *status, *n_prop, *n_acc;
};

// Chain q of a call: par, the chain's state inside the workspace, and its rows of the call's arrays
struct BoxchainLane {
    int64_t q, Q;
    int D, K;
    const double *w, *yb, *pv, *pm, *sc, *lo, *hi;    // par: w (K), ybar (K), pv (D), pm (D), s (D), lo (D), hi (D)
    double *X, *G, *GT, *LP;                          // x, g, g' (D x Q each) ... lp (Q) ...
    int32_t *FLAG;                                    // ... and one int32 (Q) behind the doubles
    double *xt;
    const double *fq, *Jq;
};

// The workspace holds NV vectors (D x Q doubles: x, g, g', then the kernel's own), NS scalars (Q doubles: lp, then the kernel's
// own) and the int32 flag (Q): boxmala 3 and 1, boxhmc 4 and 2.  0 for sizes the steps refuse.
template <int NV, int NS>
static size_t boxchain_workspace(int64_t Q, int D) {
    if (Q < 1 || Q > 0x7fffffffLL || D < 1 || D > DGPAMD_MAXD) return 0;
    return (size_t)Q * (8 * ((size_t)NV * D + NS) + 4);
}

// The part of a lane that the call's arguments fix: par and the chain's rows of f, J and x_trial
__device__ __forceinline__ BoxchainLane boxchain_lane_par(const BoxchainArgs &a, int64_t q) {
    BoxchainLane c;
    const int D = a.D, K = a.K;
    c.q = q, c.Q = a.Q, c.D = D, c.K = K;
    c.w = a.par, c.yb = c.w + K, c.pv = c.yb + K, c.pm = c.pv + D, c.sc = c.pm + D, c.lo = c.sc + D, c.hi = c.lo + D;
    c.xt = a.x_trial + q * D;
    c.fq = a.f + q * K, c.Jq = a.J + q * K * D;
    return c;
}
template <int NV, int NS>
__device__ __forceinline__ BoxchainLane boxchain_lane(const BoxchainArgs &a, int64_t q) {
    BoxchainLane c = boxchain_lane_par(a, q);
    c.X = a.ws + q, c.G = c.X + (int64_t)a.D * a.Q, c.GT = c.G + (int64_t)a.D * a.Q, c.LP = c.GT + (int64_t)(NV - 2) * a.D * a.Q;
    c.FLAG = (int32_t *)(a.ws + ((int64_t)NV * a.D + NS) * a.Q) + q;
    return c;
}
// the kernel's own fields: vector i >= 3, scalar i >= 1
__device__ __forceinline__ double *boxchain_vector(const BoxchainLane &c, int i) { return c.GT + (int64_t)(i - 2) * c.D * c.Q; }
__device__ __forceinline__ double *boxchain_scalar(const BoxchainLane &c, int i) { return c.LP + (int64_t)i * c.Q; }

// a column that keeps its x: it is left out of every sum over the free columns
__device__ __forceinline__ bool boxchain_fixed(const BoxchainLane &c, int d) { return c.sc[d] == 0.0 || c.lo[d] == c.hi[d]; }

// TARGET: lp' and, into the workspace, g' at the trial point; false if either is not finite.  An output with w_k = 0 and a
// column with pv_d = 0 are not read.  TEMPERED (boxsmc.hip, under prior(x) exp(beta ll(x))): ll' and lprior' come apart and
// g'_d = beta c_d - pv_d e_d, the likelihood's part times beta before the prior's.  Compile time: the chains gain no multiply.
template <bool TEMPERED>
__device__ __forceinline__ bool boxchain_target(const BoxchainLane &c, double beta, double &llt, double &lprt) {
    const int64_t Q = c.Q;
    const int D = c.D, K = c.K;
    double sa = 0.0, sb = 0.0;
    for (int k = 0; k < K; ++k) {
        const double wk = c.w[k];
        if (wk > 0.0) {
            const double r = c.yb[k] - c.fq[k];
            sa = sa + (wk * r) * r;
        }
    }
    for (int d = 0; d < D; ++d) {
        const double p = c.pv[d];
        if (p > 0.0) {
            const double e = c.xt[d] - c.pm[d];
            sb = sb + (p * e) * e;
        }
    }
    llt = TEMPERED ? -0.5 * sa : -0.5 * sa - 0.5 * sb;            // (untempered: lp', and lprt is not written)
    if (TEMPERED) lprt = -0.5 * sb;
    bool finite = isfinite(llt) && (!TEMPERED || isfinite(lprt));
    for (int d = 0; d < D; ++d) {
        double g = 0.0;
        for (int k = 0; k < K; ++k) {
            const double wk = c.w[k];
            if (wk > 0.0) g = g + (wk * (c.yb[k] - c.fq[k])) * c.Jq[k * D + d];
        }
        if (TEMPERED) g = beta * g;
        const double p = c.pv[d];
        if (p > 0.0) g = g - p * (c.xt[d] - c.pm[d]);
        c.GT[d * Q] = g;
        finite = finite && isfinite(g);
    }
    return finite;
}
__device__ __forceinline__ bool boxchain_target(const BoxchainLane &c, double &lpt) {
    return boxchain_target<false>(c, 1.0, lpt, lpt);
}

// (x, g, lp) <- the trial's
__device__ __forceinline__ void boxchain_commit(const BoxchainLane &c, double lpt) {
    for (int d = 0; d < c.D; ++d) c.X[d * c.Q] = c.xt[d], c.G[d * c.Q] = c.GT[d * c.Q];
    *c.LP = lpt;
}

// INIT: the state from the trial, the flag down, h <- h0, logr and the counts 0; the chain's status, true if it is OK
__device__ __forceinline__ bool boxchain_init(const BoxchainArgs &a, const BoxchainLane &c, double lpt, bool finite) {
    boxchain_commit(c, lpt);
    *c.FLAG = 0;
    a.h[c.q] = a.h0;
    a.logr[c.q] = 0.0;
    a.n_prop[c.q] = 0, a.n_acc[c.q] = 0;
    a.status[c.q] = finite ? BOXCHAIN_OK : BOXCHAIN_NAN;
    return finite;
}

// The tally of a decision made with the step hq: logr, the counts, and with adapt the step for the next proposal
__device__ __forceinline__ void boxchain_tally(const BoxchainArgs &a, const BoxchainLane &c, double hq, double lr, bool acc) {
    a.logr[c.q] = lr;
    a.n_prop[c.q] = a.n_prop[c.q] + 1;
    a.n_acc[c.q] = a.n_acc[c.q] + (acc ? 1 : 0);
    if (a.adapt) a.h[c.q] = fmin(fmax(hq * (acc ? a.up : a.down), a.hmin), a.hmax);
}

// STORE: slot >= 0: xs[slot, :, q] = x, lps[slot, q] = lp
__device__ __forceinline__ void boxchain_store(const BoxchainArgs &a, const BoxchainLane &c) {
    if (a.slot < 0) return;
    double *xs = a.xs + (int64_t)a.slot * c.D * c.Q + c.q;
    for (int d = 0; d < c.D; ++d) xs[d * c.Q] = c.X[d * c.Q];
    a.lps[(int64_t)a.slot * c.Q + c.q] = *c.LP;
}

// x_trial <- x: the walk evaluates a point of the box whose values are finite
__device__ __forceinline__ void boxchain_hold(const BoxchainLane &c) {
    for (int d = 0; d < c.D; ++d) c.xt[d] = c.X[d * c.Q];
}

// MALA's 0.5 qf - 0.5 qb of DECIDE: the trial was proposed from x with the step hq, and x would be from the trial with it
__device__ __forceinline__ double boxchain_mala_ratio(const BoxchainLane &c, double hq) {
    double qf = 0.0, qb = 0.0;
    for (int d = 0; d < c.D; ++d) {
        const double sd = c.sc[d];
        if (boxchain_fixed(c, d)) continue;
        const double e = (0.5 * (hq * hq)) * (sd * sd), hs = hq * sd, x = c.X[d * c.Q], t = c.xt[d];
        const double u = ((t - x) - e * c.G[d * c.Q]) / hs, v = ((x - t) - e * c.GT[d * c.Q]) / hs;
        qf = qf + u * u;
        qb = qb + v * v;
    }
    return 0.5 * qf - 0.5 * qb;
}

// MALA's PROPOSE: the next trial from x, g, the step and the call's normal draws; outside the box: flag up, the walk evaluates x
__device__ __forceinline__ void boxchain_mala_propose(const BoxchainArgs &a, const BoxchainLane &c) {
    const double hq = a.h[c.q];
    const double *zq = a.z + c.q * c.D;
    int flag = 0;
    for (int d = 0; d < c.D; ++d) {
        const double sd = c.sc[d], l = c.lo[d], u = c.hi[d], x = c.X[d * c.Q];
        double xp = x;
        if (!boxchain_fixed(c, d)) xp = (x + ((0.5 * (hq * hq)) * (sd * sd)) * c.G[d * c.Q]) + (hq * sd) * zq[d];
        if (!(xp >= l && xp <= u)) flag = 1;          // (a NaN is outside)
        c.xt[d] = xp;
    }
    if (flag) boxchain_hold(c);
    *c.FLAG = flag;
}

static bool positive_finite(double v) { return v > 0.0 && v <= 1.79769313486231570815e308; }

// The host side of a step before its launch: every refusal (under the name `who` of the entry point), then the arguments into a
// (boxsmc.hip launches a kernel with arguments of its own behind them)
static int boxchain_args(dgpamd_ctx *ctx, const char *who, BoxchainArgs &a, int64_t Q, int D, int K, const double *f,
                         const double *J, const double *par, const double *par_h, const double *z, const double *logu, double h0,
                         double hmin, double hmax, double up, double down, int adapt, int first, int last, int slot, int n_slots,
                         void *work, double *x_trial, double *h, double *logr, double *xs, double *lps, int32_t *status,
                         int32_t *n_prop, int32_t *n_acc) {
#define BOXCHAIN_BAD(msg)                                               \
    do {                                                                \
        snprintf(ctx->err, sizeof(ctx->err), "%s: %s", who, msg);       \
        return DGPAMD_BAD_ARG;                                          \
    } while (0)
    if (!ctx) return DGPAMD_BAD_ARG;
    if (Q < 1 || Q > 0x7fffffffLL) BOXCHAIN_BAD("need 1 <= Q < 2^31");
    if (D < 1 || D > DGPAMD_MAXD) BOXCHAIN_BAD("need 1 <= D <= DGPAMD_MAXD");
    if (K < 1) BOXCHAIN_BAD("need K >= 1");
    if (!f || !J || !par || !par_h || !z || !logu || !work || !x_trial || !h || !logr || !xs || !lps || !status || !n_prop || !n_acc)
        BOXCHAIN_BAD("null pointer");
    if (!positive_finite(h0) || !positive_finite(hmin) || !positive_finite(hmax) || !positive_finite(up) || !positive_finite(down))
        BOXCHAIN_BAD("h0, hmin, hmax, up and down must be positive and finite");
    if (hmin > hmax) BOXCHAIN_BAD("need hmin <= hmax");
    if (n_slots < 0 || slot < -1 || slot >= n_slots) BOXCHAIN_BAD("need -1 <= slot < n_slots");
    const double *w_h = par_h, *pv_h = par_h + 2 * K, *s_h = pv_h + 2 * D, *lo_h = s_h + D, *hi_h = lo_h + D;
    for (int k = 0; k < K; ++k)
        if (!(w_h[k] >= 0.0)) BOXCHAIN_BAD("every weight w must be a number >= 0");
    for (int i = 0; i < D; ++i) {
        if (!(pv_h[i] >= 0.0) || !(s_h[i] >= 0.0)) BOXCHAIN_BAD("every pv and s must be a number >= 0");
        if (!(lo_h[i] <= hi_h[i])) BOXCHAIN_BAD("every bound must be a number with lo <= hi");
    }
#undef BOXCHAIN_BAD
    a.Q = Q, a.D = D, a.K = K, a.first = first ? 1 : 0, a.last = last ? 1 : 0, a.adapt = adapt ? 1 : 0, a.slot = slot;
    a.h0 = h0, a.hmin = hmin, a.hmax = hmax, a.up = up, a.down = down;
    a.f = f, a.J = J, a.par = par, a.z = z, a.logu = logu;
    a.ws = (double *)work, a.x_trial = x_trial, a.h = h, a.logr = logr, a.xs = xs, a.lps = lps;
    a.status = status, a.n_prop = n_prop, a.n_acc = n_acc;
    return DGPAMD_OK;
}

// The host side of a step: the refusals, the arguments, the launch
static int boxchain_step(dgpamd_ctx *ctx, const char *who, void (*kernel)(BoxchainArgs), int64_t Q, int D, int K, const double *f,
                         const double *J, const double *par, const double *par_h, const double *z, const double *logu, double h0,
                         double hmin, double hmax, double up, double down, int adapt, int first, int last, int slot, int n_slots,
                         void *work, double *x_trial, double *h, double *logr, double *xs, double *lps, int32_t *status,
                         int32_t *n_prop, int32_t *n_acc) {
    BoxchainArgs a;
    const int rc = boxchain_args(ctx, who, a, Q, D, K, f, J, par, par_h, z, logu, h0, hmin, hmax, up, down, adapt, first, last, slot,
                                 n_slots, work, x_trial, h, logr, xs, lps, status, n_prop, n_acc);
    if (rc != DGPAMD_OK) return rc;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
