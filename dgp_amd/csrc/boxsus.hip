// Subset simulation over one box (DESIGN I.22), f64, for gfx950: the two device steps of failure_probability.
//
// P draws with R particles each, Q = P R lanes q = p R + r.  The event of draw p is F = {score >= 0},
//   score(x) = sign (f_output(x) - threshold) + 0.0        (the + 0.0 turns -0 into +0: f = threshold lies in F),
// and its probability under the prior on the box is the product of the conditional probabilities of a ladder of levels
// b_1 < b_2 < ... <= 0, each the n_s-th largest score of the particles that sample prior(x | score >= the level before).
//
// dgpamd_boxsus_move: the component-wise modified Metropolis move of Au and Beck (2001) inside {score >= level}, one lane per
// particle, one wave per workgroup.  From boxchain.hpp it takes the status values and positive_finite; the chains' lane, target,
// commit and tally are about a log-density with a gradient and a step per lane, none of which exists here, so the state is
// named tensors of this file's own and boxmala, boxhmc and boxsmc compile to what they did.  No LDS, no cross-lane operation, no
// atomics; the loops over D run over global memory.  The file is compiled with -ffp-contract=off and the move uses + - * and
// comparisons alone: it equals its numpy restatement (tests/boxsus_ref.py) bit for bit.
//
// dgpamd_boxsus_level: one workgroup per draw, its R particles the parallelism: the level, the survivors, the running product,
// the ancestors, the gather into x_trial and the survivors' spread per column.  The workgroup, its reduction, the chunk scan,
// the gather, the size check and the launch are boxpop.hpp's, as for boxsmc.hip's TEMPER.
//   Where the numbers live: the scores sit in LDS as order-preserving 64-bit keys (all bits of a negative double flipped, the
//   sign bit of a non-negative one; a NaN, a dead particle, is key 0, which no number has), 8 R bytes; the survivors' indices
//   in rank order behind them, 4 R bytes: 96 KB dynamic at the compiled maximum R = DGPAMD_BOXSUS_MAXR = 8192, plus 4.4 KB
//   static, of the CU's 160 KB.
//   The selection is a most-significant-bit-first radix select: 64 rounds, each an integer count over the thread's keys, a
//   butterfly inside the wave, one barrier and a sum over at most 16 wave totals.  Integer counts: no summation order to fix.
//   What bounds it: latency -- 65 + 2 D dependent rounds of a reduction with one barrier each; a draw is one workgroup.
//   Determinism: the threads of a draw are fixed by R; every loop that holds a barrier runs to a bound that is a constant,
//   R's or D's, and every barrier sits in control flow that the whole workgroup takes (the branches on done, on the live count
//   and on D are uniform).  The floating sums of sd run lane-strided, then through boxpop_reduce, as boxsmc_temper's.
#include "boxchain.hpp"
#include "boxpop.hpp"

static_assert(DGPAMD_BOXSUS_OK == BOXCHAIN_OK && DGPAMD_BOXSUS_NAN == BOXCHAIN_NAN, "a particle's status is a chain's");
#define BOXSUS_ZERO_KEY 0x8000000000000000ULL       // the key of +0.0

struct BoxsusMoveArgs {
    int64_t Q;
    int R, D, K, output, first, last;
    double sign, threshold;
    const double *f, *par, *level, *lam, *sd, *z, *logu;
    double *x_trial, *x, *score;
    int32_t *moved, *status, *n_prop, *n_acc;
};

__global__ __launch_bounds__(64) void boxsus_move_kernel(BoxsusMoveArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x, Q = a.Q;
    if (q >= Q) return;
    const int D = a.D;
    const int64_t p = q / a.R;
    const double *pv = a.par, *pm = pv + D, *lo = pm + D, *hi = lo + D;     // par: pv (D), pm (D), lo (D), hi (D)
    double *xt = a.x_trial + q * D, *X = a.x + q;
    // SCORE: the one output that is read
    const double st = a.sign * (a.f[q * a.K + a.output] - a.threshold) + 0.0;
    bool live;
    if (a.first) {
        // INIT of a stage: the state from the trial
        for (int d = 0; d < D; ++d) X[d * Q] = xt[d];
        a.score[q] = st;
        a.n_prop[q] = 0, a.n_acc[q] = 0;
        a.moved[q] = 0;
        live = !(st != st);
        a.status[q] = live ? BOXCHAIN_OK : BOXCHAIN_NAN;
    } else {
        live = a.status[q] == BOXCHAIN_OK;
        if (live) {
            // DECIDE: the trial stays inside the level set (a NaN comparison is a rejection)
            const bool acc = a.moved[q] != 0 && st >= a.level[p];
            if (acc) {
                for (int d = 0; d < D; ++d) X[d * Q] = xt[d];
                a.score[q] = st;
            }
            a.n_prop[q] = a.n_prop[q] + 1;
            a.n_acc[q] = a.n_acc[q] + (acc ? 1 : 0);
        }
    }
    if (!live || a.last) {                            // status NAN, or the stage ends: the walk evaluates x
        for (int d = 0; d < D; ++d) xt[d] = X[d * Q];
        return;
    }
    // PROPOSE: every free column on its own, kept inside the box with the probability of the prior's ratio
    const double lam = a.lam[p];
    const double *sdp = a.sd + p * D, *zq = a.z + q * D, *uq = a.logu + q * D;
    int moved = 0;
    for (int d = 0; d < D; ++d) {
        const double s = sdp[d], l = lo[d], u = hi[d], x = X[d * Q];
        double xp = x;
        if (!(s == 0.0 || l == u)) {
            const double c = x + (lam * s) * zq[d];
            bool keep = c >= l && c <= u;             // (a NaN is outside)
            const double pvd = pv[d];
            if (keep && pvd > 0.0) {
                const double et = c - pm[d], e = x - pm[d];
                keep = uq[d] < (-0.5 * (pvd * et)) * et - (-0.5 * (pvd * e)) * e;
            }
            if (keep) xp = c, moved = 1;
        }
        xt[d] = xp;
    }
    a.moved[q] = moved;
}

// ------------------------------------------------------------------------------------------------------------------- LEVEL
struct BoxsusLevelArgs {
    int64_t P;
    int R, D, n_s;
    double min_prob;
    const double *score, *x;
    double *prob, *level, *sd, *x_trial;
    int32_t *nsurv, *done, *status, *anc, *running;
};

__device__ __forceinline__ unsigned long long boxsus_key(double s) {
    if (s != s) return 0ULL;
    const unsigned long long b = (unsigned long long)__double_as_longlong(s + 0.0);
    return (b >> 63) ? ~b : (b | BOXSUS_ZERO_KEY);
}
__device__ __forceinline__ double boxsus_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k ^ BOXSUS_ZERO_KEY) : ~k));
}

__global__ __launch_bounds__(BOXPOP_THREADS) void boxsus_level_kernel(BoxsusLevelArgs a) {
    extern __shared__ unsigned long long key[];                   // R keys, then R int32: the survivors in rank order
    __shared__ int ibuf[2][BOXPOP_WAVES];
    __shared__ double dbuf[2][BOXPOP_WAVES];
    __shared__ int tot[BOXPOP_THREADS];
    const BoxpopThread th = boxpop_thread();
    const int t = th.t, NT = th.NT;
    const int R = a.R, D = a.D;
    int *surv = (int *)(key + R);
    const int64_t p = blockIdx.x, Q = a.P * R, q0 = p * R;
    int32_t *anc = a.anc + q0;
    int turn = 0;

    // (uniform: every thread reads done[p] before the barriers that precede thread 0's store to it)
    bool identity = a.done[p] != 0;
    int nlive = 0;
    if (!identity) {
        for (int i = t; i < R; i += NT) {
            const unsigned long long k = boxsus_key(a.score[q0 + i]);
            key[i] = k;
            nlive += k != 0ULL;
        }
        nlive = boxpop_reduce<BoxpopAdd>(th, &ibuf[turn], nlive), turn ^= 1;
        if (nlive == 0) {
            if (t == 0) a.status[p] = DGPAMD_BOXSUS_NAN, a.prob[p] = NAN, a.done[p] = 1, a.nsurv[p] = 0;
            identity = true;
        }
    }
    if (identity) {
        // a finished draw, or one without a live particle: the particles stay
        boxpop_stay(th, R, D, Q, q0, a.x, a.x_trial, anc);
        return;
    }

    // the k-th largest key, bit by bit from the top: of the keys that agree with the prefix above `bit`, c have the bit set
    int k = min(a.n_s, nlive);
    unsigned long long b = 0ULL;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long want = (b >> bit) | 1ULL;
        int c = 0;
        for (int i = t; i < R; i += NT) c += (key[i] >> bit) == want;
        c = boxpop_reduce<BoxpopAdd>(th, &ibuf[turn], c), turn ^= 1;
        if (c >= k) b |= 1ULL << bit;
        else k -= c;
    }
    const bool ends = b >= BOXSUS_ZERO_KEY;                      // b >= 0: the level is +0.0, the draw's final stage
    const unsigned long long lk = ends ? BOXSUS_ZERO_KEY : b;

    // the survivors' ranks in index order, on boxpop_scan's three levels (a dead key is 0 < lk); n_b is its total
    const BoxpopScan<int> sc = boxpop_scan<true>(th, R, tot, ibuf[turn], [&](int i) { return (int)(key[i] >= lk); });
    turn ^= 1;
    const int nb = sc.total;
    int rank = sc.B + sc.L;
    for (int i = sc.i0; i < sc.i1; ++i)
        if (key[i] >= lk) surv[rank++] = i;
    __syncthreads();

    // the running product and what the draw's stage is
    if (t == 0) {
        const double pr = a.prob[p] * ((double)nb / (double)R);
        a.prob[p] = pr;
        a.nsurv[p] = nb;
        a.level[p] = boxsus_unkey(lk);
        if (ends) {
            a.done[p] = 1;
        } else if (pr < a.min_prob) {
            a.done[p] = 1, a.status[p] = DGPAMD_BOXSUS_BELOW_MIN;
        } else {
            atomicAdd(a.running, 1);
        }
    }

    // ANCESTORS and GATHER: slot j gets the (j mod n_b)-th survivor
    for (int j = t; j < R; j += NT) anc[j] = surv[j % nb];
    boxpop_gather(th, R, D, Q, q0, a.x, a.x_trial, [&](int j) { return surv[j % nb]; });

    // the survivors' spread per column, two passes; a column whose value is 0 or not finite keeps what it had
    const double n = (double)nb;
    for (int d = 0; d < D; ++d) {
        const double *xd = a.x + (int64_t)d * Q + q0;
        double s = 0.0;
        for (int i = t; i < R; i += NT)
            if (key[i] >= lk) s = s + xd[i];
        const double mean = boxpop_reduce<BoxpopAdd>(th, &dbuf[0], s) / n;
        s = 0.0;
        for (int i = t; i < R; i += NT)
            if (key[i] >= lk) {
                const double e = xd[i] - mean;
                s = s + e * e;
            }
        const double v = sqrt(boxpop_reduce<BoxpopAdd>(th, &dbuf[1], s) / n);
        if (t == 0 && v > 0.0 && v <= 1.79769313486231570815e308) a.sd[p * D + d] = v;
    }
}

#define BOXSUS_SIZES BOXPOP_SIZES("DGPAMD_BOXSUS_MAXR")
extern "C" int dgpamd_boxsus_move(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, int K, int output, double sign, double threshold,
                                  const double *f, const double *par, const double *par_h, const double *level, const double *lam,
                                  const double *sd, const double *z, const double *logu, int first, int last, double *x_trial,
                                  double *x, double *score, int32_t *moved, int32_t *status, int32_t *n_prop, int32_t *n_acc) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (!boxpop_sizes(P, R, D)) BAD_ARG(ctx, BOXSUS_SIZES);
    if (K < 1 || output < 0 || output >= K) BAD_ARG(ctx, "need K >= 1 and 0 <= output < K");
    if (!(sign == 1.0 || sign == -1.0)) BAD_ARG(ctx, "sign must be +1 or -1");
    if (!(threshold >= -1.79769313486231570815e308 && threshold <= 1.79769313486231570815e308))
        BAD_ARG(ctx, "threshold must be finite");
    if (!f || !par || !par_h || !level || !lam || !sd || !z || !logu || !x_trial || !x || !score || !moved || !status || !n_prop ||
        !n_acc)
        BAD_ARG(ctx, "null pointer");
    const double *pv_h = par_h, *lo_h = par_h + 2 * D, *hi_h = lo_h + D;
    for (int i = 0; i < D; ++i) {
        if (!(pv_h[i] >= 0.0)) BAD_ARG(ctx, "every pv must be a number >= 0");
        if (!(lo_h[i] <= hi_h[i])) BAD_ARG(ctx, "every bound must be a number with lo <= hi");
    }
    BoxsusMoveArgs a;
    a.Q = P * R, a.R = (int)R, a.D = D, a.K = K, a.output = output, a.first = first ? 1 : 0, a.last = last ? 1 : 0;
    a.sign = sign, a.threshold = threshold;
    a.f = f, a.par = par, a.level = level, a.lam = lam, a.sd = sd, a.z = z, a.logu = logu;
    a.x_trial = x_trial, a.x = x, a.score = score, a.moved = moved, a.status = status, a.n_prop = n_prop, a.n_acc = n_acc;
    hipLaunchKernelGGL(boxsus_move_kernel, dim3((unsigned)((a.Q + 63) / 64)), dim3(64), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_boxsus_level(dgpamd_ctx *ctx, int64_t P, int64_t R, int D, int n_s, double min_prob, const double *score,
                                   const double *x, double *prob, double *level, int32_t *nsurv, int32_t *done, int32_t *status,
                                   int32_t *anc, double *x_trial, double *sd, int32_t *running) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (!boxpop_sizes(P, R, D)) BAD_ARG(ctx, BOXSUS_SIZES);
    if (n_s < 1 || n_s >= R) BAD_ARG(ctx, "need 1 <= n_s < R");
    if (!(min_prob >= 0.0 && min_prob < 1.0)) BAD_ARG(ctx, "need 0 <= min_prob < 1");
    if (!score || !x || !prob || !level || !nsurv || !done || !status || !anc || !x_trial || !sd || !running)
        BAD_ARG(ctx, "null pointer");
    BoxsusLevelArgs a;
    a.P = P, a.R = (int)R, a.D = D, a.n_s = n_s, a.min_prob = min_prob;
    a.score = score, a.x = x, a.prob = prob, a.level = level, a.sd = sd, a.x_trial = x_trial;
    a.nsurv = nsurv, a.done = done, a.status = status, a.anc = anc, a.running = running;
    return boxpop_launch(ctx, boxsus_level_kernel, a, P, R, 12 * (size_t)R, running);
}
