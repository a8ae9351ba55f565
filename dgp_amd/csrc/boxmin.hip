// Batched projected L-BFGS over one box, driven by reverse communication (DESIGN I.17), f64, for gfx950.
//
// Q independent problems min phi_q(x), lo <= x <= hi, D <= 64 columns.  A call takes phi and its gradient at the trial points
// -- column k of the walk's values (Q, K) and Jacobian (Q, K, D), times sign -- advances every problem's state machine by one
// transition and writes the next trial points.  Nothing goes to the host; the only atomic is the integer count of problems
// still running.
// One lane per problem, workgroups of one wave.  Every state field lies (field..., Q), problem fastest: the lanes of a wave read
// and write consecutive doubles.  The loops over D and over the stored pairs run over that global memory -- a per-lane array
// with a runtime index would live in scratch -- and the bound set of a point is one 64-bit mask in registers.  No cross-lane
// operation: a problem's iterates are one fixed sequence of operations on its own inputs, whatever shares its wave.
// The file is compiled with -ffp-contract=off (csrc/Makefile): every product is rounded before it enters a sum, and every sum
// runs in index order, so the kernel performs the operations of its numpy restatement (tests/boxmin_ref.py) one for one.
#include <math.h>

#include "common.hpp"

#define BOXMIN_ARMIJO 1e-4
#define BOXMIN_CURVATURE 1e-10
#define BOXMIN_HALVINGS 20
#define BOXMIN_MAXGROW 30

struct BoxminArgs {
    int64_t Q;
    int D, K, k, history, maxiter, max_eval, first;
    double sign, gtol, ftol;
    const double *f, *J, *lo, *hi;
    double *ws, *x_trial, *x, *fun;
    int32_t *status, *n_iter, *n_eval, *running;
};

// The state of problem q inside the workspace; dgpamd_boxmin_workspace is the sum of these fields.
struct BoxminState {
    double *X, *G, *Dv, *S, *Y, *RHO, *ALPHA, *F, *T;
    int32_t *HALV, *SD, *NP, *HEAD, *GROW;
    int64_t Q;
    __device__ BoxminState(double *ws, int64_t Q_, int D, int h, int64_t q) : Q(Q_) {
        X = ws + q;
        G = X + D * Q;
        Dv = G + D * Q;
        S = Dv + D * Q;
        Y = S + (int64_t)h * D * Q;
        RHO = Y + (int64_t)h * D * Q;
        ALPHA = RHO + h * Q;
        F = ALPHA + h * Q;
        T = F + Q;
        HALV = (int32_t *)(T + Q - q) + q;
        SD = HALV + Q;
        NP = SD + Q;
        HEAD = NP + Q;
        GROW = HEAD + Q;
    }
};

static size_t boxmin_ws_bytes(int64_t Q, int D, int h) {
    return (size_t)Q * (8 * ((size_t)3 * D + (size_t)2 * h * D + (size_t)2 * h + 2) + 20);
}

__device__ __forceinline__ double box_project(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// B = {i : (x_i <= lo_i and g_i > 0) or (x_i >= hi_i and g_i < 0) or lo_i == hi_i} as a mask
__device__ static uint64_t bound_set(const BoxminState &s, const BoxminArgs &a) {
    uint64_t bm = 0;
    for (int i = 0; i < a.D; ++i) {
        const double x = s.X[i * s.Q], g = s.G[i * s.Q], lo = a.lo[i], hi = a.hi[i];
        if ((x <= lo && g > 0.0) || (x >= hi && g < 0.0) || lo == hi) bm |= 1ull << i;
    }
    return bm;
}

// d = -pg, t = min(1, 1 / max|pg|) 2^grow
__device__ static void steepest(const BoxminState &s, const BoxminArgs &a, uint64_t bm) {
    double mx = 0.0;
    for (int i = 0; i < a.D; ++i) {
        const double pg = (bm >> i & 1) ? 0.0 : s.G[i * s.Q];
        s.Dv[i * s.Q] = -pg;
        mx = fmax(mx, fabs(pg));
    }
    *s.T = ldexp(fmin(1.0, 1.0 / mx), *s.GROW);
    *s.SD = 1;
}

// x_trial = P(x + t d)
__device__ static void emit(const BoxminState &s, const BoxminArgs &a, double *xt) {
    const double t = *s.T;
    for (int i = 0; i < a.D; ++i) xt[i] = box_project(s.X[i * s.Q] + t * s.Dv[i * s.Q], a.lo[i], a.hi[i]);
}

// DIRECTION after its convergence test: the two-loop recursion on the free components, the first step length, the trial
__device__ static void direction(const BoxminState &s, const BoxminArgs &a, double *xt) {
    const int64_t Q = s.Q;
    const int D = a.D, h = a.history, np = *s.NP, head = *s.HEAD;
    const uint64_t bm = bound_set(s, a);
    for (int i = 0; i < D; ++i) s.Dv[i * Q] = (bm >> i & 1) ? 0.0 : s.G[i * Q];
    double sy_new = 0.0;
    int newest = 0;
    for (int jj = np - 1; jj >= 0; --jj) {
        const int slot = (head + jj) % h;
        const double *Sj = s.S + (int64_t)slot * D * Q, *Yj = s.Y + (int64_t)slot * D * Q;
        double sy = 0.0;
        for (int i = 0; i < D; ++i) sy += (bm >> i & 1) ? 0.0 : Sj[i * Q] * Yj[i * Q];
        if (jj == np - 1) sy_new = sy, newest = slot;
        double rho = 0.0, al = 0.0;
        if (sy > 0.0) {
            rho = 1.0 / sy;
            double sq = 0.0;
            for (int i = 0; i < D; ++i) sq += (bm >> i & 1) ? 0.0 : Sj[i * Q] * s.Dv[i * Q];
            al = rho * sq;
            for (int i = 0; i < D; ++i)
                if (!(bm >> i & 1)) s.Dv[i * Q] = s.Dv[i * Q] - al * Yj[i * Q];
        }
        s.RHO[slot * Q] = rho;
        s.ALPHA[slot * Q] = al;
    }
    double gamma = 1.0;
    if (sy_new > 0.0) {
        const double *Yj = s.Y + (int64_t)newest * D * Q;
        double yy = 0.0;
        for (int i = 0; i < D; ++i) yy += (bm >> i & 1) ? 0.0 : Yj[i * Q] * Yj[i * Q];
        if (yy > 0.0) gamma = sy_new / yy;
    }
    for (int i = 0; i < D; ++i) s.Dv[i * Q] = gamma * s.Dv[i * Q];
    for (int jj = 0; jj < np; ++jj) {
        const int slot = (head + jj) % h;
        const double rho = s.RHO[slot * Q];
        if (!(rho > 0.0)) continue;
        const double *Sj = s.S + (int64_t)slot * D * Q, *Yj = s.Y + (int64_t)slot * D * Q;
        double yr = 0.0;
        for (int i = 0; i < D; ++i) yr += (bm >> i & 1) ? 0.0 : Yj[i * Q] * s.Dv[i * Q];
        const double c = s.ALPHA[slot * Q] - rho * yr;
        for (int i = 0; i < D; ++i)
            if (!(bm >> i & 1)) s.Dv[i * Q] = s.Dv[i * Q] + c * Sj[i * Q];
    }
    double slope = 0.0;
    for (int i = 0; i < D; ++i) {
        const bool bound = bm >> i & 1;
        const double d = bound ? 0.0 : -s.Dv[i * Q];
        s.Dv[i * Q] = d;
        slope += (bound ? 0.0 : s.G[i * Q]) * d;
    }
    if (np == 0 || !(slope < 0.0) || !isfinite(slope)) {
        steepest(s, a, bm);
    } else {
        *s.T = 1.0;
        *s.SD = 0;
    }
    *s.HALV = 0;
    emit(s, a, xt);
}

__global__ __launch_bounds__(64) void boxmin_step_kernel(BoxminArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= a.Q) return;
    if (!a.first && a.status[q] != DGPAMD_BOXMIN_RUNNING) return;   // finished: x_trial is x already
    const int64_t Q = a.Q;
    const int D = a.D;
    const BoxminState s(a.ws, Q, D, a.history, q);
    double *xt = a.x_trial + q * D;
    const double *gt = a.J + (q * a.K + a.k) * D;
    const double sign = a.sign;
    const double phi = sign * a.f[q * a.K + a.k];
    bool finite = isfinite(phi);
    for (int i = 0; i < D; ++i) finite = finite && isfinite(sign * gt[i]);
    int ne = a.first ? 1 : a.n_eval[q] + 1, ni = a.first ? 0 : a.n_iter[q];
    int done = DGPAMD_BOXMIN_RUNNING;
    bool moved = false;                       // (x, f, g) is new: the convergence tests apply
    double f_old = 0.0;

    if (a.first) {
        for (int i = 0; i < D; ++i) s.X[i * Q] = xt[i], s.G[i * Q] = sign * gt[i];
        *s.F = phi;
        *s.NP = 0, *s.HEAD = 0, *s.HALV = 0, *s.SD = 1, *s.GROW = 0;
        *s.T = 0.0;
        a.status[q] = DGPAMD_BOXMIN_RUNNING;
        if (!finite)
            done = DGPAMD_BOXMIN_NAN;
        else
            moved = true;                     // (INIT: the GTOL test alone applies)
    } else {
        double gd = 0.0;
        for (int i = 0; i < D; ++i) gd += s.G[i * Q] * (xt[i] - s.X[i * Q]);
        if (finite && phi <= *s.F + BOXMIN_ARMIJO * gd && gd < 0.0) {
            // ACCEPT
            double sy = 0.0, ss = 0.0, yy = 0.0;
            for (int i = 0; i < D; ++i) {
                const double dl = xt[i] - s.X[i * Q], y = sign * gt[i] - s.G[i * Q];
                sy += dl * y;
                ss += dl * dl;
                yy += y * y;
            }
            if (sy > BOXMIN_CURVATURE * (sqrt(ss) * sqrt(yy))) {
                const int h = a.history, np = *s.NP, head = *s.HEAD;
                const int slot = (head + np) % h;      // (a full ring: the oldest pair's slot)
                if (np < h)
                    *s.NP = np + 1;
                else
                    *s.HEAD = (head + 1) % h;
                double *Sj = s.S + (int64_t)slot * D * Q, *Yj = s.Y + (int64_t)slot * D * Q;
                for (int i = 0; i < D; ++i) Sj[i * Q] = xt[i] - s.X[i * Q], Yj[i * Q] = sign * gt[i] - s.G[i * Q];
                *s.GROW = 0;
            } else {
                *s.GROW = *s.HALV == 0 ? min(*s.GROW + 1, BOXMIN_MAXGROW) : 0;   // (no positive curvature seen: the next -pg step doubles)
            }
            f_old = *s.F;
            for (int i = 0; i < D; ++i) s.X[i * Q] = xt[i], s.G[i * Q] = sign * gt[i];
            *s.F = phi;
            ++ni;
            moved = true;
        } else if (ne >= a.max_eval) {
            done = DGPAMD_BOXMIN_MAXEVAL;
        } else if (*s.HALV >= BOXMIN_HALVINGS) {
            if (*s.SD) {
                done = DGPAMD_BOXMIN_LINESEARCH;
            } else {
                *s.NP = 0, *s.HEAD = 0, *s.HALV = 0, *s.GROW = 0;
                steepest(s, a, bound_set(s, a));
                emit(s, a, xt);
            }
        } else {
            *s.T = *s.T * 0.5;
            *s.HALV = *s.HALV + 1;
            emit(s, a, xt);
        }
    }
    if (moved) {
        double res = 0.0;
        for (int i = 0; i < D; ++i) {
            const double x = s.X[i * Q];
            res = fmax(res, fabs(box_project(x - s.G[i * Q], a.lo[i], a.hi[i]) - x));
        }
        if (res <= a.gtol)
            done = DGPAMD_BOXMIN_GTOL;
        else if (!a.first && f_old - phi <= a.ftol * fmax(fmax(fabs(f_old), fabs(phi)), 1.0))
            done = DGPAMD_BOXMIN_FTOL;
        else if (!a.first && ni >= a.maxiter)
            done = DGPAMD_BOXMIN_MAXITER;
        else if (ne >= a.max_eval)
            done = DGPAMD_BOXMIN_MAXEVAL;
        else
            direction(s, a, xt);
    }
    a.n_eval[q] = ne;
    a.n_iter[q] = ni;
    if (done != DGPAMD_BOXMIN_RUNNING) {
        for (int i = 0; i < D; ++i) {
            const double x = s.X[i * Q];
            xt[i] = x;
            a.x[q * D + i] = x;
        }
        a.fun[q] = sign * *s.F;
        a.status[q] = done;
        atomicSub(a.running, 1);
    }
}

__global__ void boxmin_count_kernel(int32_t *running, int32_t Q) { *running = Q; }

extern "C" size_t dgpamd_boxmin_workspace(int64_t Q, int D, int history) {
    if (Q < 1 || Q > 0x7fffffffLL || D < 1 || D > DGPAMD_MAXD || history < 1 || history > DGPAMD_BOXMIN_MAXHIST) return 0;
    return boxmin_ws_bytes(Q, D, history);
}

extern "C" int dgpamd_boxmin_step(dgpamd_ctx *ctx, int64_t Q, int D, int K, int k, double sign, const double *f, const double *J,
                                  const double *lo, const double *hi, const double *lo_h, const double *hi_h, int history,
                                  int maxiter, int max_eval, double gtol, double ftol, int first, void *work, double *x_trial,
                                  double *x, double *fun, int32_t *status, int32_t *n_iter, int32_t *n_eval, int32_t *running) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (Q < 1 || Q > 0x7fffffffLL) BAD_ARG(ctx, "need 1 <= Q < 2^31");
    if (D < 1 || D > DGPAMD_MAXD) BAD_ARG(ctx, "need 1 <= D <= DGPAMD_MAXD");
    if (K < 1 || k < 0 || k >= K) BAD_ARG(ctx, "need K >= 1 and 0 <= k < K");
    if (!(sign == 1.0 || sign == -1.0)) BAD_ARG(ctx, "sign must be +1 or -1");
    if (history < 1 || history > DGPAMD_BOXMIN_MAXHIST) BAD_ARG(ctx, "need 1 <= history <= DGPAMD_BOXMIN_MAXHIST");
    if (maxiter < 1 || max_eval < 1) BAD_ARG(ctx, "need maxiter >= 1 and max_eval >= 1");
    if (!(gtol >= 0.0) || !(ftol >= 0.0)) BAD_ARG(ctx, "the tolerances must be numbers >= 0");
    if (!f || !J || !lo || !hi || !lo_h || !hi_h || !work || !x_trial || !x || !fun || !status || !n_iter || !n_eval || !running)
        BAD_ARG(ctx, "null pointer");
    for (int i = 0; i < D; ++i)
        if (!(lo_h[i] <= hi_h[i])) BAD_ARG(ctx, "every bound must be a number with lo <= hi");
    BoxminArgs a;
    a.Q = Q, a.D = D, a.K = K, a.k = k, a.history = history, a.maxiter = maxiter, a.max_eval = max_eval, a.first = first ? 1 : 0;
    a.sign = sign, a.gtol = gtol, a.ftol = ftol;
    a.f = f, a.J = J, a.lo = lo, a.hi = hi;
    a.ws = (double *)work, a.x_trial = x_trial, a.x = x, a.fun = fun;
    a.status = status, a.n_iter = n_iter, a.n_eval = n_eval, a.running = running;
    if (first) {
        hipLaunchKernelGGL(boxmin_count_kernel, dim3(1), dim3(1), 0, ctx->stream, running, (int32_t)Q);
        LAUNCH_CHECK(ctx);
    }
    hipLaunchKernelGGL(boxmin_step_kernel, dim3((unsigned)((Q + 63) / 64)), dim3(64), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
