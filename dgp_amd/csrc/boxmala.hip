// Batched Metropolis-adjusted Langevin chains over one box, driven by reverse communication (DESIGN I.19), f64, for gfx950.
//
// A call takes the walk's values (Q, K) and Jacobian (Q, K, D) at the trial points, decides every chain's pending proposal,
// adapts its step, stores a sample and writes the next trial points from the caller's normal draws z.  Nothing goes to the host.
// The target, the layout of par and of the workspace, the steps this kernel shares with boxhmc.hip and the roundings that
// hold it to its numpy restatement (tests/boxmala_ref.py) are boxchain.hpp's.  Its own: the log ratio of the two proposal
// densities, and PROPOSE.
#include "boxchain.hpp"

// 0.5 qf - 0.5 qb of DECIDE: the trial was proposed from x with the step hq, and x would be proposed from the trial with it
__device__ __forceinline__ double boxmala_proposal_ratio(const BoxchainLane &c, double hq) {
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

__global__ __launch_bounds__(64) void boxmala_step_kernel(BoxchainArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Q) return;
    const BoxchainLane c = boxchain_lane<3, 1>(a, q);       // x, g, g'; lp; the flag: the pending proposal left the box
    bool live = a.first || a.status[q] == BOXCHAIN_OK;

    if (live) {
        double lpt;
        const bool finite = boxchain_target(c, lpt);
        if (a.first) {
            live = boxchain_init(a, c, lpt, finite);
        } else {
            // DECIDE: the trial was proposed with the step h the chain still holds
            const double hq = a.h[q];
            double lr;
            bool acc = false;
            if (*c.FLAG) {
                lr = -INFINITY;                       // outside the box: target density zero
            } else if (!finite) {
                lr = NAN;
            } else {
                const double lq = boxmala_proposal_ratio(c, hq);      // (before lp is loaded: two VGPRs fewer across the loop)
                lr = (lpt - *c.LP) + lq;
                acc = a.logu[q] < lr;                 // (a NaN comparison is a rejection)
            }
            if (acc) boxchain_commit(c, lpt);
            boxchain_tally(a, c, hq, lr, acc);
        }
    }
    boxchain_store(a, c);
    if (!live) {                                      // status NAN: the walk keeps evaluating the start
        boxchain_hold(c);
        return;
    }
    // PROPOSE
    const double hq = a.h[q];
    const double *zq = a.z + q * c.D;
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

extern "C" size_t dgpamd_boxmala_workspace(int64_t Q, int D) { return boxchain_workspace<3, 1>(Q, D); }

extern "C" int dgpamd_boxmala_step(dgpamd_ctx *ctx, int64_t Q, int D, int K, const double *f, const double *J, const double *par,
                                   const double *par_h, const double *z, const double *logu, double h0, double hmin, double hmax,
                                   double up, double down, int adapt, int first, int slot, int n_slots, void *work,
                                   double *x_trial, double *h, double *logr, double *xs, double *lps, int32_t *status,
                                   int32_t *n_prop, int32_t *n_acc) {
    return boxchain_step(ctx, __func__, boxmala_step_kernel, Q, D, K, f, J, par, par_h, z, logu, h0, hmin, hmax, up, down, adapt,
                         first, 0, slot, n_slots, work, x_trial, h, logr, xs, lps, status, n_prop, n_acc);
}
