"""dgpamd_boxsmc_move and dgpamd_boxsmc_temper (csrc/boxsmc.hip, DESIGN I.21) restated in numpy from the text of
include/dgp_amd.h.  The move: elementwise over the particles, per particle the same operations in the same order on float64
numbers, so that the device's trials, decisions and steps can be compared with array_equal.  The tempering step: the same definitions with
numpy's exp and sequential sums -- the device sums in another (fixed) order and uses its own exponential, so it is held to
this by bounds, not by equality.  Also smc, the driver's schedule for one draw, and grid_evidence, the exact answer."""
import numpy as np

import boxmala_ref as M

OK, NAN, MAX_STAGES = 0, 1, 2
F = np.float64
XMAX = 707.5                  # exp_negated returns exactly 0 beyond it
HALVINGS = 52


# ------------------------------------------------------------------------------------------------------------------ TEMPER
def weights(ll, dbeta):
    """a_i = exp(-(dbeta (m - ll_i))), m the largest finite ll; 0 for a dead particle (ll not finite) and beyond XMAX.
    Any float type: the dtype of ll decides."""
    ll = np.asarray(ll)
    live = np.isfinite(ll)
    a = np.zeros(ll.shape, dtype=ll.dtype)
    if live.any():
        arg = ll.dtype.type(dbeta) * (ll[live].max() - ll[live])
        with np.errstate(under='ignore'):
            a[live] = np.where(arg > XMAX, 0.0, np.exp(-arg))
    return a


def ess(a):
    s = a.sum()
    return (s * s) / (a * a).sum()


def choose_dbeta(ll, beta, ess_frac):
    """The device's rule: 1 - beta if ESS(1 - beta) >= ess_frac R_live, else the lower end of [0, 1 - beta] after HALVINGS
    halvings.  0 without a live particle or at beta = 1."""
    ll = np.asarray(ll, dtype=F)
    n_live, full = np.isfinite(ll).sum(), F(1.0) - F(beta)
    if n_live == 0 or not full > 0.0:
        return F(0.0)
    target = F(ess_frac) * F(n_live)
    if ess(weights(ll, full)) >= target:
        return full
    lo, hi = F(0.0), full
    for _ in range(HALVINGS):
        mid = F(0.5) * (lo + hi)
        if ess(weights(ll, mid)) >= target:
            lo = mid
        else:
            hi = mid
    return lo


def boundaries(a, u):
    """R C_i - u before the ceiling, C the sequential cumsum of a / sum a, clamped to 1 and exactly 1 from the last
    particle of positive weight on."""
    a = np.asarray(a, dtype=F)
    R = len(a)
    C = np.minimum(np.cumsum(a / a.sum()), 1.0)
    C[np.nonzero(a > 0.0)[0][-1]:] = 1.0
    return F(R) * C - F(u)


def resample(a, u):
    """(anc (R,), offspring counts (R,)) of systematic resampling with the one uniform u."""
    R = len(a)
    b = np.concatenate([[0], np.clip(np.ceil(boundaries(a, u)), 0, R).astype(np.int64)])
    b[1 + np.nonzero(np.asarray(a) > 0.0)[0][-1]:] = R
    counts = np.diff(b)
    return np.repeat(np.arange(R), counts), counts


def temper(ll, beta, u, ess_frac, dbeta=None):
    """One draw's TEMPER: dict(dbeta, beta, increment (of log_evidence), ess, anc, status, running).  dbeta: evaluate at this
    step instead of the rule's (the device's own, in the tests)."""
    ll = np.asarray(ll, dtype=F)
    R = len(ll)
    live = np.isfinite(ll)
    if beta >= 1.0:
        return dict(dbeta=F(0.0), beta=F(beta), increment=F(0.0), ess=F(np.nan), anc=np.arange(R), status=OK, running=0)
    if not live.any():
        return dict(dbeta=F(0.0), beta=F(beta), increment=F(np.nan), ess=F(np.nan), anc=np.arange(R), status=NAN, running=0)
    d = choose_dbeta(ll, beta, ess_frac) if dbeta is None else F(dbeta)
    if not d > 0.0:
        return dict(dbeta=F(0.0), beta=F(beta), increment=F(0.0), ess=F(np.nan), anc=np.arange(R), status=OK, running=1)
    a = weights(ll, d)
    new = F(1.0) if d == F(1.0) - F(beta) else F(beta) + d
    return dict(dbeta=d, beta=new, increment=d * ll[live].max() + np.log(a.sum() / R), ess=ess(a), anc=resample(a, u)[0],
                status=OK, running=int(new < 1.0))


# -------------------------------------------------------------------------------------------------------------------- MOVE
class Particles:
    """Q particles, one array entry each.  Every operation is elementwise over the particles and the sums over the outputs
    and the columns are Python loops in index order: particle q's numbers are the kernel's, operation for operation.
    move(f (Q, K), J (Q, K, D), z (Q, D), logu (Q,), beta (Q,), ...) is one call of the move kernel: f and J are the values
    and the Jacobian at self.trial; afterwards self.trial holds the next points to evaluate.  The steps h are the caller's
    and no call resets them."""

    def __init__(self, x0, w, ybar, lo, hi, s, pv=None, pm=None, h0=0.1, hmin=1e-10, hmax=1e2):
        Q, D = np.shape(x0)
        self.w, self.ybar, self.lo, self.hi, self.s = (np.asarray(a, dtype=F) for a in (w, ybar, lo, hi, s))
        self.pv = np.zeros(D) if pv is None else np.asarray(pv, dtype=F)
        self.pm = np.zeros(D) if pm is None else np.asarray(pm, dtype=F)
        self.hmin, self.hmax = F(hmin), F(hmax)
        self.trial = np.array(x0, dtype=F)
        self.h = np.full(Q, h0, dtype=F)
        self.status = np.zeros(Q, dtype=np.int32)
        self.free = ~((self.s == 0.0) | (self.lo == self.hi))
        self.x, self.g = self.trial.copy(), np.zeros((Q, D))
        self.ll, self.lprior, self.logr = np.zeros(Q), np.zeros(Q), np.zeros(Q)
        self.flag = np.zeros(Q, dtype=bool)
        self.n_prop, self.n_acc = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)

    def target(self, x, f, J, beta):
        """(ll, lprior, g) at x under beta: boxmala_ref's sums, the likelihood's gradient times beta before the prior's."""
        Q, D = x.shape
        sa, sb = np.zeros(Q), np.zeros(Q)
        for k in range(len(self.w)):
            if self.w[k] > 0.0:
                r = self.ybar[k] - f[:, k]
                sa = sa + (self.w[k] * r) * r
        for d in range(D):
            if self.pv[d] > 0.0:
                e = x[:, d] - self.pm[d]
                sb = sb + (self.pv[d] * e) * e
        g = np.zeros((Q, D))
        for d in range(D):
            c = np.zeros(Q)
            for k in range(len(self.w)):
                if self.w[k] > 0.0:
                    c = c + (self.w[k] * (self.ybar[k] - f[:, k])) * J[:, k, d]
            c = beta * c
            if self.pv[d] > 0.0:
                c = c - self.pv[d] * (x[:, d] - self.pm[d])
            g[:, d] = c
        return F(-0.5) * sa, F(-0.5) * sb, g

    def move(self, f, J, z, logu, beta, first=False, last=False, adapt=False, up=1.0, down=1.0):
        with np.errstate(all='ignore'):
            self._move(np.asarray(f, dtype=F), np.asarray(J, dtype=F), np.asarray(z, dtype=F), np.asarray(logu, dtype=F),
                       np.asarray(beta, dtype=F), first, last, adapt, F(up), F(down))

    def _move(self, f, J, z, logu, beta, first, last, adapt, up, down):
        Q, D = self.trial.shape
        xt = self.trial
        live = np.ones(Q, dtype=bool) if first else self.status == OK
        llt, lprt, gt = self.target(xt, f, J, beta)
        finite = np.isfinite(llt) & np.isfinite(lprt) & np.all(np.isfinite(gt), 1)
        if first:
            self.x, self.g, self.ll, self.lprior = xt.copy(), gt, llt, lprt
            self.flag, self.logr = np.zeros(Q, dtype=bool), np.zeros(Q)
            self.n_prop, self.n_acc = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)
            self.status = np.where(finite, OK, NAN).astype(np.int32)
            live = finite
        else:
            h = self.h
            qf, qb = np.zeros(Q), np.zeros(Q)
            for d in range(D):
                if not self.free[d]:
                    continue
                sd = self.s[d]
                c, hs = (F(0.5) * (h * h)) * (sd * sd), h * sd
                u = ((xt[:, d] - self.x[:, d]) - c * self.g[:, d]) / hs
                v = ((self.x[:, d] - xt[:, d]) - c * gt[:, d]) / hs
                qf = qf + u * u
                qb = qb + v * v
            lr = ((beta * llt + lprt) - (beta * self.ll + self.lprior)) + (F(0.5) * qf - F(0.5) * qb)
            lr = np.where(self.flag, -np.inf, np.where(finite, lr, np.nan))
            acc = live & ~self.flag & finite & (logu < lr)
            self.x, self.g = np.where(acc[:, None], xt, self.x), np.where(acc[:, None], gt, self.g)
            self.ll, self.lprior = np.where(acc, llt, self.ll), np.where(acc, lprt, self.lprior)
            self.logr = np.where(live, lr, self.logr)
            self.n_prop = self.n_prop + live
            self.n_acc = self.n_acc + acc
            if adapt:
                self.h = np.where(live, np.minimum(np.maximum(h * np.where(acc, up, down), self.hmin), self.hmax), h)
        hold = ~live | last
        h, xp = self.h, self.x.copy()
        for d in range(D):
            if self.free[d]:
                sd = self.s[d]
                xp[:, d] = (self.x[:, d] + ((F(0.5) * (h * h)) * (sd * sd)) * self.g[:, d]) + (h * sd) * z[:, d]
        out = np.any(~((xp >= self.lo) & (xp <= self.hi)), 1)
        self.trial = np.where((hold | out)[:, None], self.x, xp)
        self.flag = np.where(hold, self.flag, out)


def smc(fun, x0, w, ybar, lo, hi, s, streams, stage_gain, n_moves=4, ess_frac=0.5, max_stages=100, pv=None, pm=None, h0=0.1, p=0,
        hmin=1e-10, hmax=1e2):
    """calibrate_smc's schedule for draw p of the streams (a calibrate.SmcStreams whose prior uniforms made x0 (R, D)),
    fun(x (R, D)) -> (f (R, K), J (R, K, D)): the evaluation of the prior particles, then per stage TEMPER, the start of the
    stage and n_moves decisions with the draw's step held fixed, and after the stage the step times
    stage_gain(stage, the stage's acceptance rate).  Returns dict(x (R, D), ll, log_evidence, betas, stage_ess, accept_rate,
    status, parts)."""
    R, D = x0.shape
    pt = Particles(x0, w, ybar, lo, hi, s, pv, pm, h0)
    pt.move(*fun(pt.trial), np.zeros((R, D)), np.zeros(R), np.zeros(R), first=True, last=True)
    beta, logz, betas, esss, rates, status = F(0.0), F(0.0), [], [], [], MAX_STAGES
    for stage in range(max_stages):
        u, z, logu = streams.stage(n_moves + 1)
        t = temper(pt.ll, beta, u[p], ess_frac)
        if t['status'] == NAN:
            status, logz = NAN, F(np.nan)
            break
        beta, logz = t['beta'], logz + t['increment'] if t['dbeta'] > 0.0 else logz
        betas.append(beta), esss.append(t['ess'])
        pt.trial = pt.x[t['anc']].copy()
        for i in range(n_moves + 1):
            pt.move(*fun(pt.trial), z[i, p], logu[i, p], np.full(R, beta), first=i == 0, last=i == n_moves)
        rates.append(pt.n_acc.sum() / max(pt.n_prop.sum(), 1))
        pt.h = np.minimum(np.maximum(pt.h * stage_gain(stage, rates[-1]), hmin), hmax)
        if not beta < 1.0:
            status = OK
            break
    return dict(x=pt.x, ll=pt.ll, log_evidence=logz, betas=betas, stage_ess=esss, accept_rate=rates, status=status, parts=pt)


# ------------------------------------------------------------------------------------------------------------- exact answers
def grid_evidence(f_on_grid, axes, ybar, w, pv=None, pm=None):
    """log of the integral of prior(x) exp(ll(x)) over the box spanned by axes (1 or 2 increasing grids that end on the
    bounds), prior the NORMALISED prior on the box, by the trapezoid rule; f_on_grid as in boxmala_ref.grid_posterior."""
    D = len(axes)
    mesh = np.meshgrid(*axes, indexing='ij')
    f = np.asarray(f_on_grid, dtype=F).reshape(mesh[0].shape + (-1,))
    seen = np.asarray(w) > 0.0
    ll = -0.5 * np.sum(np.asarray(w)[seen] * (np.asarray(ybar)[seen] - f[..., seen]) ** 2, -1)
    lprior = np.zeros(mesh[0].shape)
    if pv is not None:
        for d in range(D):
            if pv[d] > 0.0:
                lprior = lprior - 0.5 * pv[d] * (mesh[d] - pm[d]) ** 2
    wt = M._trapezoid(axes[0]) if D == 1 else np.outer(M._trapezoid(axes[0]), M._trapezoid(axes[1]))
    top = ll.max()
    return float(top + np.log(np.sum(np.exp(lprior + ll - top) * wt)) - np.log(np.sum(np.exp(lprior) * wt)))


def grid_mass(f_on_grid, axes, ybar, w, below, pv=None, pm=None):
    """The posterior mass of x_0 < below on the grid (below a grid point of axes[0])."""
    D = len(axes)
    mesh = np.meshgrid(*axes, indexing='ij')
    f = np.asarray(f_on_grid, dtype=F).reshape(mesh[0].shape + (-1,))
    seen = np.asarray(w) > 0.0
    lp = -0.5 * np.sum(np.asarray(w)[seen] * (np.asarray(ybar)[seen] - f[..., seen]) ** 2, -1)
    if pv is not None:
        for d in range(D):
            if pv[d] > 0.0:
                lp = lp - 0.5 * pv[d] * (mesh[d] - pm[d]) ** 2
    dens = np.exp(lp - lp.max())
    k = int(np.searchsorted(axes[0], below))
    assert axes[0][k] == below
    if D == 2:
        dens = dens @ M._trapezoid(axes[1])
    return float(np.sum(dens[:k + 1] * M._trapezoid(axes[0][:k + 1])) / np.sum(dens * M._trapezoid(axes[0])))
