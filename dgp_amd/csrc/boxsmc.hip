// Tempered sequential Monte Carlo over one box (DESIGN I.21), f64, for gfx950: the two device steps of calibrate_smc.
//
// P draws with R particles each, Q = P R lanes q = p R + r.  Draw p's particles sample
//   pi_beta(x)  proportional to  prior(x) exp(beta_p ll(x)),   ll(x) = -1/2 sum_k w_k (ybar_k - f_k(x))^2,
// and beta_p goes from 0 to 1 in steps that keep the effective sample size of the incremental weights.
//
// dgpamd_boxsmc_move: the MALA move under pi_beta, one lane per particle, on boxchain.hpp's lane layout, commit, tally, hold and
// argument checks.  Its own: the tempered target, which keeps ll and the prior part apart, the named state x (D x Q), ll and
// lprior (Q) that TEMPER and the caller read, `first` as the start of a stage after the gather, and `last`.  The proposal and
// its density ratio are MALA's (boxmala.hip holds them as its own; they are restated here because that file does not move).
// The file is compiled with -ffp-contract=off and the move uses + - * / and comparisons alone: it equals its numpy
// restatement (tests/boxsmc_ref.py) bit for bit.
//
// dgpamd_boxsmc_temper: one workgroup per draw, its R particles the parallelism: reweight, choose the step of beta by bisection
// on the effective sample size, add to the evidence, resample systematically, gather the ancestors into x_trial.
//   Where the numbers live: d_i = m - ll_i (dead: -1) sits in LDS across the bisection, R doubles; every bisection step reads it
//   lane-strided and evaluates a_i = exp_negated(delta d_i) anew.  The final weights overwrite d in place and the scan reads
//   them in contiguous chunks.  ll is read from global memory once, x once in the gather.
//   LDS: 8 R bytes dynamic, 64 KB at the compiled maximum R = DGPAMD_BOXSMC_MAXR = 8192, plus 8.8 KB static (the partial sums
//   of the reductions and of the scan): under half of the CU's 160 KB.
//   What bounds it: latency, not throughput.  The bisection is BOXSMC_HALVINGS + 1 dependent rounds of (R / threads
//   exponentials, a cross-lane tree, one barrier, a sum over at most 16 wave totals); a draw is one workgroup, so P draws
//   occupy P of the 256 CUs.  The offspring loop of one dominant particle is R stores by one lane.
//   Determinism: the threads of a draw are min(1024, R rounded up to 64), fixed by R; every sum runs lane-strided, then an
//   xor butterfly inside the wave (both partners add the same two numbers), then the wave totals in index order; the scan is
//   sequential inside a thread's chunk, over the lanes of a wave and over the waves.  Nothing depends on P or on the other
//   draws of the launch but the running count, an integer.
#include "boxchain.hpp"

static_assert(DGPAMD_BOXSMC_OK == BOXCHAIN_OK && DGPAMD_BOXSMC_NAN == BOXCHAIN_NAN, "a particle's status is a chain's");
#define BOXSMC_HALVINGS 52          // of the bracket [0, 1 - beta]: its width ends at one ulp of 1 - beta
#define BOXSMC_THREADS 1024

struct BoxsmcArgs : BoxchainArgs {
    int64_t R;
    const double *beta;
    double *x, *ll, *lprior;
};

// Particle q: boxchain's lane over the workspace g, g' (D x Q each) and the int32 flag (Q), with x and ll the named tensors
__device__ __forceinline__ BoxchainLane boxsmc_lane(const BoxsmcArgs &a, int64_t q) {
    BoxchainLane c;
    const int64_t Q = a.Q;
    const int D = a.D, K = a.K;
    c.q = q, c.Q = Q, c.D = D, c.K = K;
    c.w = a.par, c.yb = c.w + K, c.pv = c.yb + K, c.pm = c.pv + D, c.sc = c.pm + D, c.lo = c.sc + D, c.hi = c.lo + D;
    c.X = a.x + q, c.G = a.ws + q, c.GT = c.G + (int64_t)D * Q, c.LP = a.ll + q;
    c.FLAG = (int32_t *)(a.ws + (int64_t)2 * D * Q) + q;
    c.xt = a.x_trial + q * D;
    c.fq = a.f + q * K, c.Jq = a.J + q * K * D;
    return c;
}

static size_t boxsmc_workspace(int64_t P, int64_t R, int D) {
    if (P < 1 || R < 1 || R > DGPAMD_BOXSMC_MAXR || P > 0x7fffffffLL / R || D < 1 || D > DGPAMD_MAXD) return 0;
    return (size_t)(P * R) * (16 * (size_t)D + 4);
}

// TARGET under beta: ll' and lprior' at the trial point and, into the workspace, g'_d = beta c_d - pv_d e_d; false if any is
// not finite.  The sums are boxchain_target's, term for term; at beta = 1, ll' + lprior' and g' are its lp' and g'.
__device__ __forceinline__ bool boxsmc_target(const BoxchainLane &c, double beta, double &llt, double &lprt) {
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
    llt = -0.5 * sa, lprt = -0.5 * sb;
    bool finite = isfinite(llt) && isfinite(lprt);
    for (int d = 0; d < D; ++d) {
        double g = 0.0;
        for (int k = 0; k < K; ++k) {
            const double wk = c.w[k];
            if (wk > 0.0) g = g + (wk * (c.yb[k] - c.fq[k])) * c.Jq[k * D + d];
        }
        g = beta * g;
        const double p = c.pv[d];
        if (p > 0.0) g = g - p * (c.xt[d] - c.pm[d]);
        c.GT[d * Q] = g;
        finite = finite && isfinite(g);
    }
    return finite;
}

// 0.5 qf - 0.5 qb of DECIDE, as boxmala_proposal_ratio
__device__ __forceinline__ double boxsmc_proposal_ratio(const BoxchainLane &c, double hq) {
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

__global__ __launch_bounds__(64) void boxsmc_move_kernel(BoxsmcArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Q) return;
    const BoxchainLane c = boxsmc_lane(a, q);
    const double beta = a.beta[q / a.R];
    bool live = a.first || a.status[q] == BOXCHAIN_OK;

    if (live) {
        double llt, lprt;
        const bool finite = boxsmc_target(c, beta, llt, lprt);
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
                const double lq = boxsmc_proposal_ratio(c, hq);
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
    // PROPOSE, as boxmala's
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

// ------------------------------------------------------------------------------------------------------------------ TEMPER
struct BoxsmcTemperArgs {
    int64_t P;
    int R, D;
    double ess_frac;
    const double *ll, *x, *u;
    double *beta, *dbeta, *log_evidence, *stage_ess, *x_trial;
    int32_t *status, *anc, *running;
};

// (s1, s2) <- their sums over the workgroup, in every thread: the xor butterfly of the wave, then the NW wave totals in index
// order.  buf: one of the two halves of the scratch, used in turn, so that one barrier per call is enough.
__device__ __forceinline__ void boxsmc_sum2(double &s1, double &s2, double (*buf)[BOXSMC_THREADS / 64], int w, int lane, int NW) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s1 = s1 + __shfl_xor(s1, off, 64);
        s2 = s2 + __shfl_xor(s2, off, 64);
    }
    if (lane == 0) buf[0][w] = s1, buf[1][w] = s2;
    __syncthreads();
    s1 = buf[0][0], s2 = buf[1][0];
    for (int v = 1; v < NW; ++v) s1 = s1 + buf[0][v], s2 = s2 + buf[1][v];
}
// (m1, m2) <- their maxima over the workgroup, in every thread
__device__ __forceinline__ void boxsmc_max2(double &m1, double &m2, double (*buf)[BOXSMC_THREADS / 64], int w, int lane, int NW) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m1 = fmax(m1, __shfl_xor(m1, off, 64));
        m2 = fmax(m2, __shfl_xor(m2, off, 64));
    }
    if (lane == 0) buf[0][w] = m1, buf[1][w] = m2;
    __syncthreads();
    m1 = buf[0][0], m2 = buf[1][0];
    for (int v = 1; v < NW; ++v) m1 = fmax(m1, buf[0][v]), m2 = fmax(m2, buf[1][v]);
}

// The slot boundary ceil(R C - u) as an integer in 0 .. R (a NaN gives 0)
__device__ __forceinline__ int boxsmc_boundary(double C, double u, int R) {
    const double v = ceil((double)R * C - u);
    return v >= 0.0 ? (v <= (double)R ? (int)v : R) : 0;
}

__global__ __launch_bounds__(BOXSMC_THREADS) void boxsmc_temper_kernel(BoxsmcTemperArgs a) {
    extern __shared__ double dl[];                                // R: m - ll_i (dead: -1), then the weights a_i
    __shared__ double red[2][2][BOXSMC_THREADS / 64];
    __shared__ double tot[BOXSMC_THREADS];
    __shared__ double wtot[BOXSMC_THREADS / 64];
    const int t = threadIdx.x, NT = blockDim.x, lane = t & 63, w = t >> 6, NW = NT >> 6;
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
        boxsmc_sum2(cnt, none, red[turn], w, lane, NW), turn ^= 1;
        nlive = cnt;
        boxsmc_max2(m, none, red[turn], w, lane, NW), turn ^= 1;
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
            boxsmc_sum2(s1, s2, red[turn], w, lane, NW), turn ^= 1;
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
        for (int i = t; i < R; i += NT) anc[i] = i;
        for (int64_t e = t; e < (int64_t)R * D; e += NT) {
            const int64_t j = e / D, d = e - j * D;
            a.x_trial[(q0 + j) * D + d] = a.x[d * Q + q0 + j];
        }
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
        boxsmc_max2(ilast, none, red[turn], w, lane, NW), turn ^= 1;
    }
    if (t == 0) {
        a.beta[p] = beta_new;
        a.dbeta[p] = delta;
        a.stage_ess[p] = ess;
        a.log_evidence[p] = a.log_evidence[p] + (delta * m + log(S / (double)R));
        if (beta_new < 1.0) atomicAdd(a.running, 1);
    }

    // The inclusive scan C_i of a_i / S, monotone by construction: a thread sums its chunk in index order, a lane's offset L is
    // the sum of the totals of the lanes before it in its wave, one after the other, a wave's offset B likewise over the
    // waves, and C_i = B + (L + run_i): each level's last value is the next one's first offset, by the same additions.
    const int chunk = (R + NT - 1) / NT, i0 = min(t * chunk, R), i1 = min(i0 + chunk, R), last = (int)ilast;
    double run = 0.0;
    for (int i = i0; i < i1; ++i) run = run + dl[i] / S;
    tot[t] = run;
    __syncthreads();
    double L = 0.0;
    for (int j = 0; j < 63; ++j)
        if (j < lane) L = L + tot[w * 64 + j];
    if (lane == 63) wtot[w] = L + run;
    __syncthreads();
    double B = 0.0;
    for (int v = 0; v < w; ++v) B = B + wtot[v];

    // Systematic resampling: particle i gets the slots ceil(R C_{i-1} - u) .. ceil(R C_i - u) - 1; the first boundary is 0
    // and the one of the last weighted particle R, so every slot is written once whatever u holds
    const double u = a.u[p];
    int b0 = i0 == 0 ? 0 : (i0 - 1 >= last ? R : boxsmc_boundary(fmin(B + L, 1.0), u, R));
    run = 0.0;
    for (int i = i0; i < i1; ++i) {
        run = run + dl[i] / S;
        const int b1 = i >= last ? R : boxsmc_boundary(fmin(B + (L + run), 1.0), u, R);
        for (int j = b0; j < b1; ++j) anc[j] = i;
        b0 = b1;
    }
    __syncthreads();
    // GATHER: the particles are read from the move's state and written to the trial array
    for (int64_t e = t; e < (int64_t)R * D; e += NT) {
        const int64_t j = e / D, d = e - j * D;
        a.x_trial[(q0 + j) * D + d] = a.x[d * Q + q0 + anc[j]];
    }
}

extern "C" size_t dgpamd_boxsmc_workspace(int64_t P, int64_t R, int D) { return boxsmc_workspace(P, R, D); }

extern "C" int dgpamd_boxsmc_move(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, int K, const double *f, const double *J,
                                  const double *par, const double *par_h, const double *beta, const double *z, const double *logu,
                                  double hmin, double hmax, double up, double down, int adapt, int first, int last, void *work,
                                  double *x_trial, double *x, double *ll, double *lprior, double *h, double *logr, int32_t *status,
                                  int32_t *n_prop, int32_t *n_acc) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (P < 1 || R < 1 || R > DGPAMD_BOXSMC_MAXR || P > 0x7fffffffLL / R) BAD_ARG(ctx, "need P >= 1, 1 <= R <= DGPAMD_BOXSMC_MAXR and P R < 2^31");
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
    if (boxsmc_workspace(P, R, D) == 0)
        BAD_ARG(ctx, "need P >= 1, 1 <= R <= DGPAMD_BOXSMC_MAXR, P R < 2^31 and 1 <= D <= DGPAMD_MAXD");
    if (!(ess_frac > 0.0 && ess_frac < 1.0)) BAD_ARG(ctx, "need 0 < ess_frac < 1");
    if (!ll || !x || !u || !beta || !dbeta || !log_evidence || !stage_ess || !status || !anc || !x_trial || !running)
        BAD_ARG(ctx, "null pointer");
    BoxsmcTemperArgs a;
    a.P = P, a.R = (int)R, a.D = D, a.ess_frac = ess_frac;
    a.ll = ll, a.x = x, a.u = u, a.beta = beta, a.dbeta = dbeta, a.log_evidence = log_evidence, a.stage_ess = stage_ess;
    a.x_trial = x_trial, a.status = status, a.anc = anc, a.running = running;
    const size_t shm = 8 * (size_t)R;
    const int rc = set_lds(ctx, (const void *)boxsmc_temper_kernel, shm);
    if (rc != DGPAMD_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(running, 0, sizeof(int32_t), ctx->stream));
    const unsigned threads = (unsigned)(R >= BOXSMC_THREADS ? BOXSMC_THREADS : (R + 63) / 64 * 64);
    hipLaunchKernelGGL(boxsmc_temper_kernel, dim3((unsigned)P), dim3(threads), shm, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
