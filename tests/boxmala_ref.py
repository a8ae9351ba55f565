"""dgpamd_boxmala_step (csrc/boxmala.hip, DESIGN I.19) restated in numpy, one chain at a time, written from the text of
include/dgp_amd.h: the same operations in the same order on float64 scalars, so that the device's decisions, steps and samples
can be compared with array_equal.  Also the exact answers the samplers are held to: grid_posterior (moments of a 1-D or 2-D
posterior by quadrature) and ar1_ess (the effective sample size of an AR(1) series)."""
import numpy as np

OK, NAN = 0, 1
F = np.float64


class Chain:
    """One chain.  step(f (K,), J (K, D), z (D,), logu, ...) is one call of the kernel for this chain: f and J are the
    values and the Jacobian at self.trial; afterwards self.trial is the next point to evaluate.  The first call is INIT."""

    def __init__(self, x0, w, ybar, lo, hi, s, pv=None, pm=None, h0=0.1, hmin=1e-10, hmax=1e2):
        D = len(x0)
        self.w, self.ybar, self.lo, self.hi, self.s = (np.asarray(a, dtype=F) for a in (w, ybar, lo, hi, s))
        self.pv = np.zeros(D) if pv is None else np.asarray(pv, dtype=F)
        self.pm = np.zeros(D) if pm is None else np.asarray(pm, dtype=F)
        self.h0, self.hmin, self.hmax = F(h0), F(hmin), F(hmax)
        self.trial = np.array(x0, dtype=F)
        self.started = False
        self.xs, self.lps, self.accepts = [], [], []

    def free(self, d):
        return not (self.s[d] == 0.0 or self.lo[d] == self.hi[d])

    def target(self, x, f, J):
        """(lp, g) at x: the sums in index order, every product rounded before it enters a sum."""
        D, K = len(x), len(self.w)
        sa, sb = F(0.0), F(0.0)
        for k in range(K):
            if self.w[k] > 0.0:
                r = self.ybar[k] - f[k]
                sa = sa + (self.w[k] * r) * r
        for d in range(D):
            if self.pv[d] > 0.0:
                e = x[d] - self.pm[d]
                sb = sb + (self.pv[d] * e) * e
        lp = F(-0.5) * sa - F(0.5) * sb
        g = np.zeros(D)
        for d in range(D):
            c = F(0.0)
            for k in range(K):
                if self.w[k] > 0.0:
                    c = c + (self.w[k] * (self.ybar[k] - f[k])) * J[k, d]
            if self.pv[d] > 0.0:
                c = c - self.pv[d] * (x[d] - self.pm[d])
            g[d] = c
        return lp, g

    def step(self, f, J, z, logu, adapt=False, up=1.0, down=1.0, save=False):
        with np.errstate(all='ignore'):
            self._step(np.asarray(f, dtype=F), np.asarray(J, dtype=F), np.asarray(z, dtype=F), F(logu), adapt, F(up), F(down), save)

    def _step(self, f, J, z, logu, adapt, up, down, save):
        D = len(self.trial)
        live = not self.started or self.status == OK
        if live:
            xt = self.trial
            lpt, gt = self.target(xt, f, J)
            finite = bool(np.isfinite(lpt) and np.all(np.isfinite(gt)))
            if not self.started:
                self.x, self.g, self.lp = xt.copy(), gt, lpt
                self.flag, self.h, self.logr, self.n_prop, self.n_acc = False, self.h0, F(0.0), 0, 0
                self.status = OK if finite else NAN
                self.started = True
                live = finite
            else:
                h, acc = self.h, False
                if self.flag:
                    lr = F(-np.inf)
                elif not finite:
                    lr = F(np.nan)
                else:
                    qf, qb = F(0.0), F(0.0)
                    for d in range(D):
                        if not self.free(d):
                            continue
                        sd = self.s[d]
                        c, hs = (F(0.5) * (h * h)) * (sd * sd), h * sd
                        u = ((xt[d] - self.x[d]) - c * self.g[d]) / hs
                        v = ((self.x[d] - xt[d]) - c * gt[d]) / hs
                        qf = qf + u * u
                        qb = qb + v * v
                    lr = (lpt - self.lp) + (F(0.5) * qf - F(0.5) * qb)
                    acc = bool(logu < lr)
                if acc:
                    self.x, self.g, self.lp = xt.copy(), gt, lpt
                self.logr = lr
                self.n_prop += 1
                self.n_acc += int(acc)
                self.accepts.append(acc)
                if adapt:
                    self.h = min(max(h * (up if acc else down), self.hmin), self.hmax)
        if save:
            self.xs.append(self.x.copy())
            self.lps.append(self.lp)
        if not live:
            self.trial = self.x.copy()
            return
        h, flag = self.h, False
        xp = self.x.copy()
        for d in range(D):
            if self.free(d):
                sd = self.s[d]
                xp[d] = (self.x[d] + ((F(0.5) * (h * h)) * (sd * sd)) * self.g[d]) + (h * sd) * z[d]
            if not (xp[d] >= self.lo[d] and xp[d] <= self.hi[d]):
                flag = True
        self.trial = self.x.copy() if flag else xp
        self.flag = flag


def sample(fun, x0, w, ybar, lo, hi, s, z, logu, warmup, thin, gain, pv=None, pm=None, h0=0.1):
    """calibrate's schedule for one chain, fun(x) -> (f (K,), J (K, D)): call 0 is INIT, calls 1 .. warmup adapt with
    (up, down) = gain(call - 1), every thin-th call after them is saved.  z (calls, D), logu (calls,).  Returns the Chain."""
    ch = Chain(x0, w, ybar, lo, hi, s, pv, pm, h0)
    for c in range(len(z)):
        f, J = fun(ch.trial)
        adapt, j = 1 <= c <= warmup, c - warmup
        up, down = gain(c - 1) if adapt else (1.0, 1.0)
        ch.step(f, J, z[c], logu[c], adapt, up, down, save=j >= 1 and j % thin == 0)
    return ch


def _trapezoid(axis):
    wt = np.zeros(len(axis))
    step = np.diff(axis)
    wt[:-1] += 0.5 * step
    wt[1:] += 0.5 * step
    return wt


def grid_posterior(f_on_grid, axes, ybar, w, pv=None, pm=None):
    """(mean (D,), covariance (D, D)) of the density proportional to exp(lp) on the box spanned by axes, a list of D = 1 or 2
    increasing 1-D grids that end on the bounds, by the trapezoid rule.  f_on_grid: (len(axes[0]), [len(axes[1]),] K), the
    function on the grid's points."""
    D = len(axes)
    mesh = np.meshgrid(*axes, indexing='ij')
    f = np.asarray(f_on_grid, dtype=F).reshape(mesh[0].shape + (-1,))
    seen = np.asarray(w) > 0.0
    lp = -0.5 * np.sum(np.asarray(w)[seen] * (np.asarray(ybar)[seen] - f[..., seen]) ** 2, -1)
    if pv is not None:
        for d in range(D):
            if pv[d] > 0.0:
                lp = lp - 0.5 * pv[d] * (mesh[d] - pm[d]) ** 2
    wt = _trapezoid(axes[0]) if D == 1 else np.outer(_trapezoid(axes[0]), _trapezoid(axes[1]))
    p = np.exp(lp - lp.max()) * wt
    p /= p.sum()
    mean = np.array([np.sum(p * m) for m in mesh])
    cov = np.array([[np.sum(p * (mesh[a] - mean[a]) * (mesh[b] - mean[b])) for b in range(D)] for a in range(D)])
    return mean, cov


def ar1_ess(rho, n):
    """The effective sample size of the mean of n steps of a stationary AR(1) series with coefficient rho, for large n."""
    return n * (1.0 - rho) / (1.0 + rho)
