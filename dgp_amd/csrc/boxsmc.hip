// Tempered sequential Monte Carlo over one box (DESIGN I.21), f64, for gfx950: the two device steps of calibrate_smc.
//
// P draws with R particles each, Q = P R lanes q = p R + r.  Draw p's particles sample
//   pi_beta(x)  proportional to  prior(x) exp(beta_p ll(x)),   ll(x) = -1/2 sum_k w_k (ybar_k - f_k(x))^2,
// and beta_p goes from 0 to 1 in steps that keep the effective sample size of the incremental weights.
//
// dgpamd_boxsmc_move: the MALA move under pi_beta, one lane per particle, on boxchain.hpp's lane, tempered target, commit,
// tally, hold, MALA proposal with its density ratio, and argument checks.  Its own: where the state lives -- the named tensors
// x (D x Q), ll and lprior (Q) that TEMPER and the caller read --, `first` as the start of a stage after the gather, which
// keeps the step h, `last`, and the tempered log ratio.  The file is compiled with -ffp-contract=off and the move uses + - * /
// and comparisons alone: it equals its numpy restatement (tests/boxsmc_ref.py) bit for bit.
//
// dgpamd_boxsmc_temper: one workgroup per draw, its R particles the parallelism: reweight, choose the step of beta by bisection
// on the effective sample size, add to the evidence, resample systematically, gather the ancestors into x_trial.  The
// workgroup, its reduction, the chunk scan, the gather, the size check and the launch are boxpop.hpp's, as for boxsus.hip.
//   Where the numbers live: d_i = m - ll_i (dead: -1) sits in LDS across the bisection, R doubles; every bisection step reads it
//   lane-strided and evaluates a_i = exp_negated(delta d_i) anew.  The final weights overwrite d in place and the scan reads
//   them in contiguous chunks.  ll is read from global memory once, x once in the gather.
//   LDS: 8 R bytes dynamic, 64 KB at the compiled maximum R = DGPAMD_BOXSMC_MAXR = 8192, plus 8.8 KB static (the partial sums
//   of the reductions and of the scan): under half of the CU's 160 KB.
//   What bounds it: latency, not throughput.  The bisection is BOXSMC_HALVINGS + 1 dependent rounds of (R / threads
//   exponentials, a cross-lane tree, one barrier, a sum over at most 16 wave totals); a draw is one workgroup, so P draws
//   occupy P of the 256 CUs.  The offspring loop of one dominant particle is R stores by one lane.
//   Determinism: boxpop.hpp's -- every sum runs lane-strided, then through boxpop_reduce, and the scan is boxpop_scan's.
#include "boxchain.hpp"
#include "boxpop.hpp"

static_assert(DGPAMD_BOXSMC_OK == BOXCHAIN_OK && DGPAMD_BOXSMC_NAN == BOXCHAIN_NAN, "a particle's status is a chain's");
#define BOXSMC_HALVINGS 52          // of the bracket [0, 1 - beta]: its width ends at one ulp of 1 - beta

struct BoxsmcArgs : BoxchainArgs {
    int64_t R;
    const double *beta;
    double *x, *ll, *lprior;
};

// Particle q: boxchain's lane over the workspace g, g' (D x Q each) and the int32 flag (Q), with x and ll the named tensors
__device__ __forceinline__ BoxchainLane boxsmc_lane(const BoxsmcArgs &a, int64_t q) {
    BoxchainLane c = boxchain_lane_par(a, q);
    c.X = a.x + q, c.G = a.ws + q, c.GT = c.G + (int64_t)a.D * a.Q, c.LP = a.ll + q;
    c.FLAG = (int32_t *)(a.ws + (int64_t)2 * a.D * a.Q) + q;
    return c;
}

__global__ __launch_bounds__(64) void boxsmc_move_kernel(BoxsmcArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Q) return;
    const BoxchainLane c = boxsmc_lane(a, q);
    const double beta = a.beta[q / a.R];
    bool live = a.first || a.status[q] == BOXCHAIN_OK;

    if (live) {
        double llt, lprt;
        const bool finite = boxchain_target<true>(c, beta, llt, lprt);
        if (a.first) {
            // INIT of a stage: the state from the trial under this beta; the step h stays what it was
            boxchain_commit(c, llt);
            a.lprior[q] = lprt;
            *c.FLAG = 0;
            a.logr[q] = 0.0;
            a.n_prop[q] = 0, a.n_acc[q] = 0;
            a.status[q] = finite ? BOXCHAIN_OK : BOXCHAIN_NAN;
            live = finite;
        } else {
            const double hq = a.h[q];
            double lr;
            bool acc = false;
            if (*c.FLAG) {
                lr = -INFINITY;                       // outside the box: target density zero
            } else if (!finite) {
                lr = NAN;
            } else {
                const double lq = boxchain_mala_ratio(c, hq);
                lr = ((beta * llt + lprt) - (beta * *c.LP + a.lprior[q])) + lq;
                acc = a.logu[q] < lr;                 // (a NaN comparison is a rejection)
            }
            if (acc) {
                boxchain_commit(c, llt);
                a.lprior[q] = lprt;
            }
            boxchain_tally(a, c, hq, lr, acc);
        }
    }
    if (!live || a.last) {                            // status NAN, or the stage ends: the walk evaluates x
        boxchain_hold(c);
        return;
    }
    boxchain_mala_propose(a, c);
}

// ------------------------------------------------------------------------------------------------------------------ TEMPER
struct BoxsmcTemperArgs {
    int64_t P;
    int R, D;
    double ess_frac;
    const double *ll, *x, *u;
    double *beta, *dbeta, *log_evidence, *stage_ess, *x_trial;
    int32_t *status, *anc, *running;
};

// The slot boundary ceil(R C - u) as an integer in 0 .. R (a NaN gives 0)
__device__ __forceinline__ int boxsmc_boundary(double C, double u, int R) {
    const double v = ceil((double)R * C - u);
    return v >= 0.0 ? (v <= (double)R ? (int)v : R) : 0;
}

__global__ __launch_bounds__(BOXPOP_THREADS) void boxsmc_temper_kernel(BoxsmcTemperArgs a) {
    extern __shared__ double dl[];                                // R: m - ll_i (dead: -1), then the weights a_i
    __shared__ double red[2][2][BOXPOP_WAVES];
    __shared__ double tot[BOXPOP_THREADS];
    __shared__ double wtot[BOXPOP_WAVES];
    const BoxpopThread th = boxpop_thread();
    const int t = th.t, NT = th.NT;
    const int R = a.R, D = a.D;
    const int64_t p = blockIdx.x, Q = a.P * R, q0 = p * R;
    const double *llp = a.ll + q0;
    int32_t *anc = a.anc + q0;
    const double beta = a.beta[p], full = 1.0 - beta;
    const bool ok = a.status[p] == DGPAMD_BOXSMC_OK;
    int turn = 0;

    // the largest live ll and the count of the live particles
    double m = -INFINITY, nlive = 0.0;
    for (int i = t; i < R; i += NT) {
        const double v = llp[i];
        if (isfinite(v)) m = fmax(m, v), nlive = nlive + 1.0;
    }
    {
        double cnt = nlive, none = 0.0;
        boxpop_reduce<BoxpopAdd, 2>(th, red[turn], cnt, none), turn ^= 1;
        nlive = cnt;
        boxpop_reduce<BoxpopMax, 2>(th, red[turn], m, none), turn ^= 1;
    }
    for (int i = t; i < R; i += NT) {
        const double v = llp[i];
        dl[i] = isfinite(v) ? m - v : -1.0;
    }

    // the step of beta: all of 1 - beta if that keeps ESS >= ess_frac R_live, else the lower end of the bisected bracket
    double delta = 0.0, S = 0.0, ess = NAN, beta_new = beta;
    if (ok && full > 0.0 && nlive > 0.0) {
        const double target = a.ess_frac * nlive;
        double lo = 0.0, hi = full;
        for (int it = 0; it <= BOXSMC_HALVINGS; ++it) {
            const double mid = it == 0 ? full : 0.5 * (lo + hi);
            double s1 = 0.0, s2 = 0.0;
            for (int i = t; i < R; i += NT) {
                const double d = dl[i], ai = d < 0.0 ? 0.0 : exp_negated(mid * d);
                s1 = s1 + ai;
                s2 = s2 + ai * ai;
            }
            boxpop_reduce<BoxpopAdd, 2>(th, red[turn], s1, s2), turn ^= 1;
            const double e = (s1 * s1) / s2;
            if (e >= target) {
                lo = mid, S = s1, ess = e;
                if (it == 0) break;
            } else {
                hi = mid;
            }
        }
        delta = lo;
        beta_new = delta == full ? 1.0 : beta + delta;
    }

    if (!(delta > 0.0)) {
        // a finished draw, a draw without a live particle, or no step that keeps the sample: the particles stay
        __syncthreads();
        if (t == 0) {
            a.dbeta[p] = 0.0;
            a.stage_ess[p] = NAN;
            if (ok && !(nlive > 0.0)) a.status[p] = DGPAMD_BOXSMC_NAN, a.log_evidence[p] = NAN;
            else if (ok && beta < 1.0) atomicAdd(a.running, 1);
        }
        boxpop_stay(th, R, D, Q, q0, a.x, a.x_trial, anc);
        return;
    }

    // the weights at delta, in place of d; the last particle with a positive weight
    double ilast = -1.0;
    for (int i = t; i < R; i += NT) {
        const double d = dl[i], ai = d < 0.0 ? 0.0 : exp_negated(delta * d);
        dl[i] = ai;
        if (ai > 0.0) ilast = (double)i;
    }
    {
        double none = 0.0;
        boxpop_reduce<BoxpopMax, 2>(th, red[turn], ilast, none), turn ^= 1;
    }
    if (t == 0) {
        a.beta[p] = beta_new;
        a.dbeta[p] = delta;
        a.stage_ess[p] = ess;
        a.log_evidence[p] = a.log_evidence[p] + (delta * m + log(S / (double)R));
        if (beta_new < 1.0) atomicAdd(a.running, 1);
    }

    // The inclusive scan C_i of a_i / S, monotone by construction: C_i = B + (L + run_i) on boxpop_scan's three levels
    const BoxpopScan<double> sc = boxpop_scan<false>(th, R, tot, wtot, [&](int i) { return dl[i] / S; });
    const int last = (int)ilast;

    // Systematic resampling: particle i gets the slots ceil(R C_{i-1} - u) .. ceil(R C_i - u) - 1; the first boundary is 0
    // and the one of the last weighted particle R, so every slot is written once whatever u holds
    const double u = a.u[p];
    int b0 = sc.i0 == 0 ? 0 : (sc.i0 - 1 >= last ? R : boxsmc_boundary(fmin(sc.B + sc.L, 1.0), u, R));
    double run = 0.0;
    for (int i = sc.i0; i < sc.i1; ++i) {
        run = run + dl[i] / S;
        const int b1 = i >= last ? R : boxsmc_boundary(fmin(sc.B + (sc.L + run), 1.0), u, R);
        for (int j = b0; j < b1; ++j) anc[j] = i;
        b0 = b1;
    }
    __syncthreads();
    boxpop_gather(th, R, D, Q, q0, a.x, a.x_trial, [&](int j) { return anc[j]; });
}

extern "C" size_t dgpamd_boxsmc_workspace(int64_t P, int64_t R, int D) {
    return boxpop_sizes(P, R, D) ? (size_t)(P * R) * (16 * (size_t)D + 4) : 0;
}

extern "C" int dgpamd_boxsmc_move(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, int K, const double *f, const double *J,
                                  const double *par, const double *par_h, const double *beta, const double *z, const double *logu,
                                  double hmin, double hmax, double up, double down, int adapt, int first, int last, void *work,
                                  double *x_trial, double *x, double *ll, double *lprior, double *h, double *logr, int32_t *status,
                                  int32_t *n_prop, int32_t *n_acc) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (!boxpop_sizes(P, R, 1)) BAD_ARG(ctx, "need P >= 1, 1 <= R <= DGPAMD_BOXSMC_MAXR and P R < 2^31");   // (D: the chains')
    if (!beta || !x || !ll || !lprior) BAD_ARG(ctx, "null pointer");
    BoxsmcArgs a;
    // (the step is the caller's: h0 is not used; no sample store)
    const int rc = boxchain_args(ctx, __func__, a, P * R, D, K, f, J, par, par_h, z, logu, 1.0, hmin, hmax, up, down, adapt, first,
                                 last, -1, 0, work, x_trial, h, logr, x, ll, status, n_prop, n_acc);
    if (rc != DGPAMD_OK) return rc;
    a.R = R, a.beta = beta, a.x = x, a.ll = ll, a.lprior = lprior;
    hipLaunchKernelGGL(boxsmc_move_kernel, dim3((unsigned)((a.Q + 63) / 64)), dim3(64), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_boxsmc_temper(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, double ess_frac, const double *ll,
                                    const double *x, const double *u, double *beta, double *dbeta, double *log_evidence,
                                    double *stage_ess, int32_t *status, int32_t *anc, double *x_trial, int32_t *running) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (!boxpop_sizes(P, R, D)) BAD_ARG(ctx, BOXPOP_SIZES("DGPAMD_BOXSMC_MAXR"));
    if (!(ess_frac > 0.0 && ess_frac < 1.0)) BAD_ARG(ctx, "need 0 < ess_frac < 1");
    if (!ll || !x || !u || !beta || !dbeta || !log_evidence || !stage_ess || !status || !anc || !x_trial || !running)
        BAD_ARG(ctx, "null pointer");
    BoxsmcTemperArgs a;
    a.P = P, a.R = (int)R, a.D = D, a.ess_frac = ess_frac;
    a.ll = ll, a.x = x, a.u = u, a.beta = beta, a.dbeta = dbeta, a.log_evidence = log_evidence, a.stage_ess = stage_ess;
    a.x_trial = x_trial, a.status = status, a.anc = anc, a.running = running;
    return boxpop_launch(ctx, boxsmc_temper_kernel, a, P, R, 8 * (size_t)R, running);
}
