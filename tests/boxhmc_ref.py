"""dgpamd_boxhmc_step (csrc/boxhmc.hip, DESIGN I.20) restated in numpy, one chain at a time, written from the text of
include/dgp_amd.h: the same operations in the same order on float64 scalars, so that the device's trial points, decisions,
steps and samples can be compared with array_equal.  The target is boxmala_ref's."""
import numpy as np

import boxmala_ref as M

OK, NAN = 0, 1
WALL, NONFINITE = 1, 2
NREFL = 8
F = np.float64


class Chain(M.Chain):
    """One chain.  step(f (K,), J (K, D), z (D,), logu, last, ...) is one call of the kernel for this chain: f and J are
    the values and the Jacobian at self.trial; afterwards self.trial is the next point to evaluate.  The first call is INIT.
    self.reflections counts the reflections of every drift, for the tests."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.reflections = 0

    def step(self, f, J, z, logu, last=True, adapt=False, up=1.0, down=1.0, save=False):
        with np.errstate(all='ignore'):
            self._hmc(np.asarray(f, dtype=F), np.asarray(J, dtype=F), np.asarray(z, dtype=F), F(logu), last, adapt, F(up), F(down), save)

    def drift(self, d, y, p, hs):
        """(y, p, outside) of column d."""
        l, u = self.lo[d], self.hi[d]
        y = y + hs * p
        for _ in range(NREFL):
            if y > u:
                y, p = u - (y - u), -p
            elif y < l:
                y, p = l + (l - y), -p
            else:
                break
            self.reflections += 1
        return y, p, not (y >= l and y <= u)

    def _hmc(self, f, J, z, logu, last, adapt, up, down, save):
        D = len(self.trial)
        live = not self.started or self.status == OK
        start = False
        if live:
            xt = self.trial
            lpt, gt = self.target(xt, f, J)
            finite = bool(np.isfinite(lpt) and np.all(np.isfinite(gt)))
            if not self.started:
                self.x, self.g, self.lp = xt.copy(), gt, lpt
                self.h, self.logr, self.n_prop, self.n_acc = self.h0, F(0.0), 0, 0
                self.p, self.bad, self.H0 = np.zeros(D), 0, F(0.0)
                self.status = OK if finite else NAN
                self.started = True
                live = finite
                start = True
            else:
                h, bad = self.h, self.bad
                if not finite and bad == 0:
                    bad = NONFINITE
                if last:
                    if bad == WALL:
                        lr = F(-np.inf)
                    elif bad:
                        lr = F(np.nan)
                    else:
                        ke = F(0.0)
                        for d in range(D):
                            if not self.free(d):
                                continue
                            p = self.p[d] + (F(0.5) * (h * self.s[d])) * gt[d]
                            ke = ke + p * p
                        lr = (lpt - F(0.5) * ke) - self.H0
                    acc = bool(logu < lr)
                    if acc:
                        self.x, self.g, self.lp = xt.copy(), gt, lpt
                    self.logr = lr
                    self.n_prop += 1
                    self.n_acc += int(acc)
                    self.accepts.append(acc)
                    if adapt:
                        self.h = min(max(h * (up if acc else down), self.hmin), self.hmax)
                    start = True
                else:
                    y = xt.copy()
                    if not bad:
                        for d in range(D):
                            if not self.free(d):
                                continue
                            hs = h * self.s[d]
                            y[d], self.p[d], out = self.drift(d, xt[d], self.p[d] + hs * gt[d], hs)
                            if out:
                                bad = WALL
                    self.trial = self.x.copy() if bad else y
                    self.bad = bad
        if save:
            self.xs.append(self.x.copy())
            self.lps.append(self.lp)
        if not live:
            self.trial = self.x.copy()
            return
        if not start:
            return
        h, bad, kz = self.h, 0, F(0.0)
        y = self.x.copy()
        for d in range(D):
            self.p[d] = F(0.0)
            if self.free(d):
                hs = h * self.s[d]
                kz = kz + z[d] * z[d]
                y[d], self.p[d], out = self.drift(d, self.x[d], z[d] + (F(0.5) * hs) * self.g[d], hs)
                if out:
                    bad = WALL
        self.H0 = self.lp - F(0.5) * kz
        self.trial = self.x.copy() if bad else y
        self.bad = bad


def sample(fun, x0, w, ybar, lo, hi, s, z, logu, lengths, warmup, thin, gain, pv=None, pm=None, h0=0.1):
    """calibrate's schedule of method='hmc' for one chain, fun(x) -> (f (K,), J (K, D)): iteration 0 is INIT; iteration
    i >= 1 takes lengths[i - 1] calls, the last of which decides with logu[i], adapts with gain(i - 1) while i <= warmup and
    starts the next trajectory from z[i]; every thin-th iteration after warm-up is saved.  z (iterations, D), logu
    (iterations,).  Returns the Chain; chain.calls counts its calls."""
    ch = Chain(x0, w, ybar, lo, hi, s, pv, pm, h0)
    ch.calls = 0
    for c in range(len(z)):
        adapt, j = 1 <= c <= warmup, c - warmup
        up, down = gain(c - 1) if adapt else (1.0, 1.0)
        L = 1 if c == 0 else int(lengths[c - 1])
        for l in range(1, L + 1):
            f, J = fun(ch.trial)
            ch.step(f, J, z[c], logu[c], l == L, adapt and l == L, up, down, save=l == L and j >= 1 and j % thin == 0)
            ch.calls += 1
    return ch
