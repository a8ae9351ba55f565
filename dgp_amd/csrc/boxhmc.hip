// Batched Hamiltonian Monte Carlo chains over one box with reflecting walls, driven by reverse communication (DESIGN I.20),
// f64, for gfx950.
//
// Q independent chains, each sampling x in lo <= x <= hi, D <= 64 columns, from boxmala.hip's target
//   lp(x) = -1/2 sum_k w_k (ybar_k - f_k(x))^2 - 1/2 sum_d pv_d (x_d - pm_d)^2.
// A trajectory of L leapfrog steps takes L calls: each takes the walk's values (Q, K) and Jacobian (Q, K, D) at the trial
// points, kicks the momenta with the gradient there and drifts the positions to the next trial points, reflecting them at the
// walls (Neal 2011, 5.5.1: the potential is +inf outside the box); the L-th call (last) closes the trajectory with the energy
// test, adapts the step, stores a sample and starts the next trajectory from the caller's normal draws z.  Nothing goes to
// the host.  One lane per chain, workgroups of one wave.  Every state field lies (field..., Q), chain fastest: the lanes of a
// wave read and write consecutive doubles.  The loops over D and K run over global memory -- a per-lane array with a runtime
// index would live in scratch.  No LDS, no cross-lane operation, no atomics: a chain's iterates are one fixed sequence of
// operations on its own inputs, whatever shares its wave.
// The file is compiled with -ffp-contract=off (csrc/Makefile): every product is rounded before it enters a sum, every sum
// runs in index order, and the kernel uses + - * / and comparisons alone, so it performs the operations of its numpy
// restatement (tests/boxhmc_ref.py) one for one.
#include <math.h>

#include "common.hpp"

struct BoxhmcArgs {
    int64_t Q;
    int D, K, first, last, adapt, slot;
    double h0, hmin, hmax, up, down;
    const double *f, *J, *par, *z, *logu;
    double *ws, *x_trial, *h, *logr, *xs, *lps;
    int32_t *status, *n_prop, *n_acc;
};

// what a trajectory's `bad` flag holds
#define BOXHMC_WALL 1
#define BOXHMC_NONFINITE 2

static size_t boxhmc_ws_bytes(int64_t Q, int D) { return (size_t)Q * (8 * ((size_t)4 * D + 2) + 4); }

// DRIFT of one free column: y += hs p, then reflections at the walls, each negating p.  True if y ends outside [l, u] (a NaN
// is outside): the reflection cap was hit or y is not finite.
__device__ __forceinline__ bool boxhmc_drift(double &y, double &p, double hs, double l, double u) {
    y = y + hs * p;
    for (int r = 0; r < DGPAMD_BOXHMC_NREFL; ++r) {
        if (y > u)
            y = u - (y - u), p = -p;
        else if (y < l)
            y = l + (l - y), p = -p;
        else
            break;
    }
    return !(y >= l && y <= u);
}

__global__ __launch_bounds__(64) void boxhmc_step_kernel(BoxhmcArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Q) return;
    const int64_t Q = a.Q;
    const int D = a.D, K = a.K;
    // par: w (K), ybar (K), pv (D), pm (D), s (D), lo (D), hi (D)
    const double *w = a.par, *yb = w + K, *pv = yb + K, *pm = pv + D, *sc = pm + D, *lo = sc + D, *hi = lo + D;
    // the state of chain q inside the workspace; dgpamd_boxhmc_workspace is the sum of these fields
    double *X = a.ws + q, *G = X + (int64_t)D * Q, *GT = G + (int64_t)D * Q, *P = GT + (int64_t)D * Q, *LP = P + (int64_t)D * Q;
    double *H0 = LP + Q;
    int32_t *FLAG = (int32_t *)(a.ws + ((int64_t)4 * D + 2) * Q) + q;
    double *xt = a.x_trial + q * D;
    const double *fq = a.f + q * K, *Jq = a.J + q * K * D;
    bool live = a.first || a.status[q] == DGPAMD_BOXHMC_OK;
    bool start = false;

    if (live) {
        // TARGET: the target and its gradient at the trial point; an output with w_k = 0 and a column with pv_d = 0 are not read
        double sa = 0.0, sb = 0.0;
        for (int k = 0; k < K; ++k) {
            const double wk = w[k];
            if (wk > 0.0) {
                const double r = yb[k] - fq[k];
                sa = sa + (wk * r) * r;
            }
        }
        for (int d = 0; d < D; ++d) {
            const double p = pv[d];
            if (p > 0.0) {
                const double e = xt[d] - pm[d];
                sb = sb + (p * e) * e;
            }
        }
        const double lpt = -0.5 * sa - 0.5 * sb;
        bool finite = isfinite(lpt);
        for (int d = 0; d < D; ++d) {
            double c = 0.0;
            for (int k = 0; k < K; ++k) {
                const double wk = w[k];
                if (wk > 0.0) c = c + (wk * (yb[k] - fq[k])) * Jq[k * D + d];
            }
            const double p = pv[d];
            if (p > 0.0) c = c - p * (xt[d] - pm[d]);
            GT[d * Q] = c;
            finite = finite && isfinite(c);
        }
        if (a.first) {
            // INIT
            for (int d = 0; d < D; ++d) X[d * Q] = xt[d], G[d * Q] = GT[d * Q];
            *LP = lpt;
            a.h[q] = a.h0;
            a.logr[q] = 0.0;
            a.n_prop[q] = 0, a.n_acc[q] = 0;
            a.status[q] = finite ? DGPAMD_BOXHMC_OK : DGPAMD_BOXHMC_NAN;
            live = finite;
            start = true;
        } else {
            const double hq = a.h[q];                 // the step the trajectory started with: only DECIDE changes it
            int bad = *FLAG;
            if (!finite && bad == 0) bad = BOXHMC_NONFINITE;
            if (a.last) {
                // DECIDE
                double lr;
                if (bad == BOXHMC_WALL) {
                    lr = -INFINITY;                   // the reflection cap was hit: the trajectory is not reversible
                } else if (bad) {
                    lr = NAN;
                } else {
                    double ke = 0.0;
                    for (int d = 0; d < D; ++d) {
                        const double sd = sc[d];
                        if (sd == 0.0 || lo[d] == hi[d]) continue;
                        const double p = P[d * Q] + (0.5 * (hq * sd)) * GT[d * Q];
                        ke = ke + p * p;
                    }
                    lr = (lpt - 0.5 * ke) - *H0;
                }
                const bool acc = a.logu[q] < lr;      // (a NaN comparison is a rejection)
                if (acc) {
                    for (int d = 0; d < D; ++d) X[d * Q] = xt[d], G[d * Q] = GT[d * Q];
                    *LP = lpt;
                }
                a.logr[q] = lr;
                a.n_prop[q] = a.n_prop[q] + 1;
                a.n_acc[q] = a.n_acc[q] + (acc ? 1 : 0);
                if (a.adapt) a.h[q] = fmin(fmax(hq * (acc ? a.up : a.down), a.hmin), a.hmax);
                start = true;
            } else {
                // MID: a full kick with g', then DRIFT from the trial
                if (!bad) {
                    for (int d = 0; d < D; ++d) {
                        const double sd = sc[d], l = lo[d], u = hi[d];
                        if (sd == 0.0 || l == u) continue;
                        const double hs = hq * sd;
                        double p = P[d * Q] + hs * GT[d * Q], y = xt[d];
                        if (boxhmc_drift(y, p, hs, l, u)) bad = BOXHMC_WALL;
                        P[d * Q] = p;
                        xt[d] = y;
                    }
                }
                if (bad)
                    for (int d = 0; d < D; ++d) xt[d] = X[d * Q];
                *FLAG = bad;
            }
        }
    }
    if (a.slot >= 0) {
        double *xs = a.xs + (int64_t)a.slot * D * Q + q;
        for (int d = 0; d < D; ++d) xs[d * Q] = X[d * Q];
        a.lps[(int64_t)a.slot * Q + q] = *LP;
    }
    if (!live) {                                      // status NAN: the walk keeps evaluating the start
        for (int d = 0; d < D; ++d) xt[d] = X[d * Q];
        return;
    }
    if (!start) return;
    // START: fresh momenta, the energy at the start, a half kick with g, then DRIFT from x
    const double hq = a.h[q];
    const double *zq = a.z + q * D;
    int bad = 0;
    double ke = 0.0;
    for (int d = 0; d < D; ++d) {
        const double sd = sc[d], l = lo[d], u = hi[d];
        double y = X[d * Q], p = 0.0;
        if (!(sd == 0.0 || l == u)) {
            const double zd = zq[d], hs = hq * sd;
            ke = ke + zd * zd;
            p = zd + (0.5 * hs) * G[d * Q];
            if (boxhmc_drift(y, p, hs, l, u)) bad = BOXHMC_WALL;
        }
        P[d * Q] = p;
        xt[d] = y;
    }
    *H0 = *LP - 0.5 * ke;
    if (bad)
        for (int d = 0; d < D; ++d) xt[d] = X[d * Q];
    *FLAG = bad;
}

extern "C" size_t dgpamd_boxhmc_workspace(int64_t Q, int D) {
    if (Q < 1 || Q > 0x7fffffffLL || D < 1 || D > DGPAMD_MAXD) return 0;
    return boxhmc_ws_bytes(Q, D);
}

static bool positive_finite(double v) { return v > 0.0 && v <= 1.79769313486231570815e308; }

extern "C" int dgpamd_boxhmc_step(dgpamd_ctx *ctx, int64_t Q, int D, int K, const double *f, const double *J, const double *par,
                                  const double *par_h, const double *z, const double *logu, double h0, double hmin, double hmax,
                                  double up, double down, int adapt, int first, int last, int slot, int n_slots, void *work,
                                  double *x_trial, double *h, double *logr, double *xs, double *lps, int32_t *status,
                                  int32_t *n_prop, int32_t *n_acc) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (Q < 1 || Q > 0x7fffffffLL) BAD_ARG(ctx, "need 1 <= Q < 2^31");
    if (D < 1 || D > DGPAMD_MAXD) BAD_ARG(ctx, "need 1 <= D <= DGPAMD_MAXD");
    if (K < 1) BAD_ARG(ctx, "need K >= 1");
    if (!f || !J || !par || !par_h || !z || !logu || !work || !x_trial || !h || !logr || !xs || !lps || !status || !n_prop || !n_acc)
        BAD_ARG(ctx, "null pointer");
    if (!positive_finite(h0) || !positive_finite(hmin) || !positive_finite(hmax) || !positive_finite(up) || !positive_finite(down))
        BAD_ARG(ctx, "h0, hmin, hmax, up and down must be positive and finite");
    if (hmin > hmax) BAD_ARG(ctx, "need hmin <= hmax");
    if (n_slots < 0 || slot < -1 || slot >= n_slots) BAD_ARG(ctx, "need -1 <= slot < n_slots");
    const double *w_h = par_h, *pv_h = par_h + 2 * K, *s_h = pv_h + 2 * D, *lo_h = s_h + D, *hi_h = lo_h + D;
    for (int k = 0; k < K; ++k)
        if (!(w_h[k] >= 0.0)) BAD_ARG(ctx, "every weight w must be a number >= 0");
    for (int i = 0; i < D; ++i) {
        if (!(pv_h[i] >= 0.0) || !(s_h[i] >= 0.0)) BAD_ARG(ctx, "every pv and s must be a number >= 0");
        if (!(lo_h[i] <= hi_h[i])) BAD_ARG(ctx, "every bound must be a number with lo <= hi");
    }
    BoxhmcArgs a;
    a.Q = Q, a.D = D, a.K = K, a.first = first ? 1 : 0, a.last = last ? 1 : 0, a.adapt = adapt ? 1 : 0, a.slot = slot;
    a.h0 = h0, a.hmin = hmin, a.hmax = hmax, a.up = up, a.down = down;
    a.f = f, a.J = J, a.par = par, a.z = z, a.logu = logu;
    a.ws = (double *)work, a.x_trial = x_trial, a.h = h, a.logr = logr, a.xs = xs, a.lps = lps;
    a.status = status, a.n_prop = n_prop, a.n_acc = n_acc;
    hipLaunchKernelGGL(boxhmc_step_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
