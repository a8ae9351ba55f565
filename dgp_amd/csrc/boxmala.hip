// Batched Metropolis-adjusted Langevin chains over one box, driven by reverse communication (DESIGN I.19), f64, for gfx950.
//
// A call takes the walk's values (Q, K) and Jacobian (Q, K, D) at the trial points, decides every chain's pending proposal,
// adapts its step, stores a sample and writes the next trial points from the caller's normal draws z.  Nothing goes to the host.
// The target, the layout of par and of the workspace, the steps this kernel shares with boxhmc.hip and the roundings that
// hold it to its numpy restatement (tests/boxmala_ref.py) are boxchain.hpp's, and so are the log ratio of the two proposal
// densities and PROPOSE, which boxsmc.hip's move shares.  Its own: the order of a call -- DECIDE, STORE, PROPOSE.
#include "boxchain.hpp"

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
                const double lq = boxchain_mala_ratio(c, hq);      // (before lp is loaded: two VGPRs fewer across the loop)
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
    boxchain_mala_propose(a, c);
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
