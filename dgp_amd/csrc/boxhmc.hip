// Batched Hamiltonian Monte Carlo chains over one box with reflecting walls, driven by reverse communication (DESIGN I.20),
// f64, for gfx950.
//
// A trajectory of L leapfrog steps takes L calls: each takes the walk's values (Q, K) and Jacobian (Q, K, D) at the trial
// points, kicks the momenta with the gradient there and drifts the positions to the next trial points, reflecting them at the
// walls (Neal 2011, 5.5.1: the potential is +inf outside the box); the L-th call (last) closes the trajectory with the energy
// test, adapts the step, stores a sample and starts the next trajectory from the caller's normal draws z.  Nothing goes to
// the host.  The target, the layout of par and of the workspace, the steps this kernel shares with boxmala.hip and the
// roundings that hold it to its numpy restatement (tests/boxhmc_ref.py) are boxchain.hpp's.  Its own: the momenta and the
// energy at a trajectory's start in the workspace, DRIFT, the `bad` flag, DECIDE's energy, MID and START.
#include "boxchain.hpp"

// what a trajectory's `bad` flag holds
#define BOXHMC_WALL 1
#define BOXHMC_NONFINITE 2

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

__global__ __launch_bounds__(64) void boxhmc_step_kernel(BoxchainArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Q) return;
    const BoxchainLane c = boxchain_lane<4, 2>(a, q);       // x, g, g', p; lp, H0; the flag: the trajectory's `bad`
    double *P = boxchain_vector(c, 3), *H0 = boxchain_scalar(c, 1);
    const int64_t Q = c.Q;
    const int D = c.D;
    bool live = a.first || a.status[q] == BOXCHAIN_OK;
    bool start = false, hold = false;

    if (live) {
        double lpt;
        const bool finite = boxchain_target(c, lpt);
        if (a.first) {
            live = boxchain_init(a, c, lpt, finite);
            start = true;
        } else {
            const double hq = a.h[q];                 // the step the trajectory started with: only DECIDE changes it
            int bad = *c.FLAG;
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
                        const double sd = c.sc[d];
                        if (boxchain_fixed(c, d)) continue;
                        const double p = P[d * Q] + (0.5 * (hq * sd)) * c.GT[d * Q];
                        ke = ke + p * p;
                    }
                    lr = (lpt - 0.5 * ke) - *H0;
                }
                const bool acc = a.logu[q] < lr;      // (a NaN comparison is a rejection)
                if (acc) boxchain_commit(c, lpt);
                boxchain_tally(a, c, hq, lr, acc);
                start = true;
            } else {
                // MID: a full kick with g', then DRIFT from the trial
                if (!bad) {
                    for (int d = 0; d < D; ++d) {
                        const double sd = c.sc[d], l = c.lo[d], u = c.hi[d];
                        if (boxchain_fixed(c, d)) continue;
                        const double hs = hq * sd;
                        double p = P[d * Q] + hs * c.GT[d * Q], y = c.xt[d];
                        if (boxhmc_drift(y, p, hs, l, u)) bad = BOXHMC_WALL;
                        P[d * Q] = p;
                        c.xt[d] = y;
                    }
                }
                *c.FLAG = bad;
                hold = bad != 0;                      // the rest of a bad trajectory evaluates x (held below, after STORE:
                                                      // a hold in here moves START's block behind MID's in the code object)
            }
        }
    }
    boxchain_store(a, c);
    if (!live || hold) {                              // (status NAN: the walk keeps evaluating the start)
        boxchain_hold(c);
        return;
    }
    if (!start) return;
    // START: fresh momenta, the energy at the start, a half kick with g, then DRIFT from x
    const double hq = a.h[q];
    const double *zq = a.z + q * D;
    int bad = 0;
    double ke = 0.0;
    for (int d = 0; d < D; ++d) {
        const double sd = c.sc[d], l = c.lo[d], u = c.hi[d];
        double y = c.X[d * Q], p = 0.0;
        if (!boxchain_fixed(c, d)) {
            const double zd = zq[d], hs = hq * sd;
            ke = ke + zd * zd;
            p = zd + (0.5 * hs) * c.G[d * Q];
            if (boxhmc_drift(y, p, hs, l, u)) bad = BOXHMC_WALL;
        }
        P[d * Q] = p;
        c.xt[d] = y;
    }
    *H0 = *c.LP - 0.5 * ke;
    if (bad) boxchain_hold(c);
    *c.FLAG = bad;
}

extern "C" size_t dgpamd_boxhmc_workspace(int64_t Q, int D) { return boxchain_workspace<4, 2>(Q, D); }

extern "C" int dgpamd_boxhmc_step(dgpamd_ctx *ctx, int64_t Q, int D, int K, const double *f, const double *J, const double *par,
                                  const double *par_h, const double *z, const double *logu, double h0, double hmin, double hmax,
                                  double up, double down, int adapt, int first, int last, int slot, int n_slots, void *work,
                                  double *x_trial, double *h, double *logr, double *xs, double *lps, int32_t *status,
                                  int32_t *n_prop, int32_t *n_acc) {
    return boxchain_step(ctx, __func__, boxhmc_step_kernel, Q, D, K, f, J, par, par_h, z, logu, h0, hmin, hmax, up, down, adapt,
                         first, last, slot, n_slots, work, x_trial, h, logr, xs, lps, status, n_prop, n_acc);
}
