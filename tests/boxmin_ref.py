"""numpy restatement of dgpamd_boxmin_step (csrc/boxmin.hip, DESIGN I.17): a projected L-BFGS for min phi(x), lo <= x <= hi,
driven by reverse communication, one problem at a time.  Written from the text of DESIGN I.17, not from the kernel.

Machine(x0, lo, hi, ...) holds one problem: .trial is the point to evaluate; .step(phi, grad) takes the objective and its
gradient there, advances the state machine by one transition and leaves the next .trial (a finished problem: .trial = .x).
Every sum over the D columns or the stored pairs is taken in index order, one addition after the other (seqsum: numpy's cumsum
adds in order), and no product is fused into a sum: the kernel is compiled without contraction, so it performs the same
operations in the same order.

  INIT       (x, f, g) <- trial; phi or g not finite: NAN.  Then DIRECTION (after its GTOL test: MAXEVAL if max_eval is 1).
  DIRECTION  B = {i: (x_i <= lo_i and g_i > 0) or (x_i >= hi_i and g_i < 0) or lo_i == hi_i}; pg = g off B, 0 on B.
             max_i |P(x - g) - x| <= gtol: GTOL.
             d = -H pg by the two-loop recursion over the stored pairs, the components of B of q, s, y taken as zero, d = 0 on
             B; a pair whose s^T y over the free components is not positive is skipped; gamma = s^T y / y^T y of the newest
             pair over the free components (1 if that pair is skipped, or without pairs).
             No pair, or pg^T d >= 0 or not finite: d = -pg, t = min(1, 1 / max|pg|) 2^grow; else t = 1.  trial = P(x + t d).
             grow counts the accepted steps just before that stored no pair and needed no halving (at most 30): where the
             draw shows no positive curvature the steepest-descent steps double, so that a linear objective overshoots its
             corner and is projected onto it exactly, where steps of one fixed length can stop one rounding error short.
  SEARCH     delta = trial - x; accept if phi_t and g_t are finite and phi_t <= f + 1e-4 g^T delta and g^T delta < 0.
             Else: n_eval >= max_eval: MAXEVAL (x kept).  After 20 halvings: a quasi-Newton direction drops the pairs and
             restarts along -pg; along -pg: LINESEARCH (x kept).  Else t <- t / 2, trial = P(x + t d).
  ACCEPT     s = delta, y = g_t - g; the pair enters the ring if s^T y > 1e-10 |s| |y| (grow <- 0), else grow <- grow + 1 after
             a search without halvings and 0 after one with.  (x, f, g) <- trial, n_iter += 1.
             The DIRECTION test for GTOL comes first; then FTOL if f_old - f <= ftol max(|f_old|, |f|, 1); MAXITER at maxiter;
             MAXEVAL at max_eval; else the rest of DIRECTION.
"""
import math

import numpy as np

RUNNING, GTOL, FTOL, MAXITER, MAXEVAL, LINESEARCH, NAN = range(7)
STATUS = dict(running=RUNNING, gtol=GTOL, ftol=FTOL, maxiter=MAXITER, maxeval=MAXEVAL, linesearch=LINESEARCH, nan=NAN)
ARMIJO, CURVATURE, HALVINGS, MAXGROW = 1e-4, 1e-10, 20, 30


def workspace_bytes(Q, D, history):
    """dgpamd_boxmin_workspace: x, g, d (D each), the pairs (2 history D), rho and alpha (history each), f and t, as doubles,
    and five int32 (halvings, steepest flag, pairs, ring head, grow), per problem."""
    return Q * (8 * (3 * D + 2 * history * D + 2 * history + 2) + 20)


def seqsum(terms):
    """((t0 + t1) + t2) + ... starting from +0."""
    return float(np.cumsum(np.concatenate(([0.0], terms)))[-1])


def project(v, lo, hi):
    return np.fmin(np.fmax(v, lo), hi)


def kkt(x, g, lo, hi):
    """max_i |P(x - g) - x|."""
    return float(np.max(np.abs(project(x - g, lo, hi) - x)))


class Machine:
    def __init__(self, x0, lo, hi, history=6, maxiter=100, max_eval=None, gtol=1e-6, ftol=1e-12):
        self.lo, self.hi = np.asarray(lo, float), np.asarray(hi, float)
        self.history, self.maxiter, self.gtol, self.ftol = history, maxiter, gtol, ftol
        self.max_eval = 4 * maxiter + 20 if max_eval is None else max_eval
        self.trial = np.array(x0, float)
        self.first = True
        self.status, self.n_iter, self.n_eval = RUNNING, 0, 0
        self.S, self.Y = [], []           # oldest first
        self.x = self.trial.copy()
        self.f = np.nan
        self.grow, self.halvings = 0, 0
        self.accepted = []                # f at INIT and after every accepted step

    # ------------------------------------------------------------------
    def _bound(self):
        x, g = self.x, self.g
        return ((x <= self.lo) & (g > 0)) | ((x >= self.hi) & (g < 0)) | (self.lo == self.hi)

    def _finish(self, status):
        self.status = status
        self.trial = self.x.copy()

    def _steepest(self):
        pg = np.where(self._bound(), 0.0, self.g)
        self.d, self.sd = -pg, True
        self.t = math.ldexp(min(1.0, 1.0 / float(np.max(np.abs(pg)))), self.grow)

    def _emit(self):
        self.trial = project(self.x + self.t * self.d, self.lo, self.hi)

    def _direction(self):
        """DIRECTION after its GTOL test."""
        free = ~self._bound()
        pg = np.where(free, self.g, 0.0)
        q = pg.copy()
        rho, alpha = [0.0] * len(self.S), [0.0] * len(self.S)
        sy_new = 0.0
        for j in reversed(range(len(self.S))):
            s, y = self.S[j], self.Y[j]
            sy = seqsum(np.where(free, s * y, 0.0))
            if j == len(self.S) - 1:
                sy_new = sy
            if sy > 0.0:
                rho[j] = 1.0 / sy
                alpha[j] = rho[j] * seqsum(np.where(free, s * q, 0.0))
                q = np.where(free, q - alpha[j] * y, 0.0)
        gamma = 1.0
        if sy_new > 0.0:
            y = self.Y[-1]
            yy = seqsum(np.where(free, y * y, 0.0))
            if yy > 0.0:
                gamma = sy_new / yy
        r = gamma * q
        for j in range(len(self.S)):
            if rho[j] > 0.0:
                beta = rho[j] * seqsum(np.where(free, self.Y[j] * r, 0.0))
                r = np.where(free, r + (alpha[j] - beta) * self.S[j], 0.0)
        d = np.where(free, -r, 0.0)
        slope = seqsum(pg * d)
        if not self.S or not (slope < 0.0) or not np.isfinite(slope):
            self._steepest()
        else:
            self.d, self.sd, self.t = d, False, 1.0
        self.halvings = 0
        self._emit()

    # ------------------------------------------------------------------
    def step(self, phi, grad):
        if self.status != RUNNING:
            return
        phi, grad = float(phi), np.asarray(grad, float)
        self.n_eval += 1
        finite = bool(np.isfinite(phi) and np.all(np.isfinite(grad)))
        if self.first:
            self.first = False
            self.x, self.f, self.g = self.trial.copy(), phi, grad.copy()
            if not finite:
                return self._finish(NAN)
            self.accepted.append(phi)
            if kkt(self.x, self.g, self.lo, self.hi) <= self.gtol:
                return self._finish(GTOL)
            if self.n_eval >= self.max_eval:
                return self._finish(MAXEVAL)
            return self._direction()
        delta = self.trial - self.x
        gd = seqsum(self.g * delta)
        if finite and phi <= self.f + ARMIJO * gd and gd < 0.0:
            y = grad - self.g
            sy, ss, yy = seqsum(delta * y), seqsum(delta * delta), seqsum(y * y)
            if sy > CURVATURE * (np.sqrt(ss) * np.sqrt(yy)):
                self.S.append(delta)
                self.Y.append(y)
                if len(self.S) > self.history:
                    self.S.pop(0)
                    self.Y.pop(0)
                self.grow = 0
            else:
                self.grow = min(self.grow + 1, MAXGROW) if self.halvings == 0 else 0
            f_old = self.f
            self.x, self.f, self.g = self.trial.copy(), phi, grad.copy()
            self.n_iter += 1
            self.accepted.append(phi)
            if kkt(self.x, self.g, self.lo, self.hi) <= self.gtol:
                return self._finish(GTOL)
            if f_old - phi <= self.ftol * max(abs(f_old), abs(phi), 1.0):
                return self._finish(FTOL)
            if self.n_iter >= self.maxiter:
                return self._finish(MAXITER)
            if self.n_eval >= self.max_eval:
                return self._finish(MAXEVAL)
            return self._direction()
        if self.n_eval >= self.max_eval:
            return self._finish(MAXEVAL)
        if self.halvings >= HALVINGS:
            if self.sd:
                return self._finish(LINESEARCH)
            self.S, self.Y, self.grow = [], [], 0
            self._steepest()
            self.halvings = 0
            return self._emit()
        self.t *= 0.5
        self.halvings += 1
        self._emit()


def minimize(fun, x0, lo, hi, **kw):
    """Drive one Machine with fun(x) -> (phi, grad) to its end: a dict like scipy's result."""
    m = Machine(x0, lo, hi, **kw)
    while m.status == RUNNING:
        m.step(*fun(m.trial))
    return dict(x=m.x, fun=m.f, status=m.status, n_iter=m.n_iter, n_eval=m.n_eval, accepted=m.accepted)


# ---------------------------------------------------------------------- the reference and the objectives of the tests
def scipy_lbfgsb(fun, x0, lo, hi, gtol=1e-6):
    """scipy.optimize.minimize(method='L-BFGS-B') with pgtol = gtol and no other stopping rule, run to a point whose own
    projected-gradient residual is <= gtol.  scipy 1.15's L-BFGS-B can return 'RELATIVE REDUCTION OF F <= FACTR*EPSMCH' after
    a few steps at a point that is no Karush-Kuhn-Tucker point at all (residual 0.67 on one of the two-column quadratics
    with active bounds, whatever ftol, maxcor or maxls): it is then started again from where it stopped, at most ten times.
    The callers assert the residual of what this returns."""
    from scipy.optimize import minimize as scipy_minimize
    x = np.array(x0, float)
    for _ in range(10):
        x = scipy_minimize(fun, x, jac=True, method='L-BFGS-B', bounds=list(zip(lo, hi)),
                           options=dict(gtol=gtol, ftol=0.0, maxiter=2000, maxfun=20000)).x
        if kkt(x, fun(x)[1], lo, hi) <= gtol:
            break
    return x


def quadratic(D, seed, outside):
    """phi = (x - c)^T A (x - c) / 2 with the eigenvalues of A spread geometrically over [1, 100] (D = 1: A = [1]) on the box
    [-1, 1]^D; c inside the box, or with `outside` beyond it in every coordinate, so that bounds are active at the minimiser.
    Returns (fun, lo, hi, lambda_min)."""
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((D, D)))[0]
    lam = np.geomspace(1.0, 100.0, D) if D > 1 else np.ones(1)
    A = (U * lam) @ U.T
    A = 0.5 * (A + A.T)
    c = rng.uniform(1.2, 2.0, D) * rng.choice([-1.0, 1.0], D) if outside else rng.uniform(-0.5, 0.5, D)

    def fun(x):
        r = x - c
        Ar = A @ r
        return 0.5 * float(r @ Ar), Ar
    return fun, -np.ones(D), np.ones(D), float(lam[0])


def rosenbrock(x):
    a, b = 1.0 - x[0], x[1] - x[0] * x[0]
    return a * a + 100.0 * b * b, np.array([-2.0 * a - 400.0 * x[0] * b, 200.0 * b])


def linear(D, seed):
    """phi = c^T x, every c_i at least 0.5 in size, on [-2, 2]^D: the minimiser is the corner -2 sign(c)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.5, 2.0, D) * rng.choice([-1.0, 1.0], D)
    return (lambda x: (float(c @ x), c.copy())), -2.0 * np.ones(D), 2.0 * np.ones(D), c
