"""The exact predictive distribution of an emulator at its test points (DESIGN I.15).

With N imputations the predictive distribution of a DGP emulator at a point is the equal-weight mixture of the N
Gaussians N(mu_s, var_s) the imputations predict -- skewed or bimodal wherever they disagree, and not the one Gaussian
that predict's two moments describe.  PredictiveMixture holds the per-imputation moments on the device and evaluates
the mixture itself there (csrc/mixture.hip): cdf, upper tail, log density, quantiles, central intervals and the CRPS.
Built by emulator.predict_dist / loo_dist, gp.predict_dist (one component) and lgp.predict_dist."""
import warnings

import numpy as np
import torch


def host_moments(ms, vs):
    """mu = mean_s mu_s, var = mean_s(mu_s^2 + v_s) - mu^2 over the leading axis on the host (emulation.py:846-847): lgp.predict's
    aggregation, and the moments of the mixtures lgp.predict_dist returns."""
    ms, vs = np.asarray(ms), np.asarray(vs)
    mu = ms.mean(0)
    return mu, (ms ** 2 + vs).mean(0) - mu ** 2


def check_points(x):
    """predict's refusal of a 1-d x, in its words."""
    if x.ndim == 1:
        raise Exception('The testing input has to be a numpy 2d-array')


class PredictiveMixture:
    """The mixtures (1/S) sum_s N(mu[s, i, k], var[s, i, k]) at M points with K outputs each.  mu, var: (S, M, K) float64
    device tensors (copied); a component with var <= 0 is a point mass.  Every method returns host numpy arrays.
    host_moments: mean() and var() by the host formula of lgp.predict instead of the device kernels of emulator.predict."""

    def __init__(self, engine, mu, var, host_moments=False):
        if mu.dim() != 3 or mu.shape != var.shape or mu.shape[0] < 1:
            raise ValueError('PredictiveMixture: mu and var must be (S, M, K) tensors of one shape, S >= 1')
        self.engine = engine
        self.mu = mu.to(dtype=torch.float64, copy=True).contiguous()
        self.variance = var.to(dtype=torch.float64, copy=True).contiguous()
        if bool(torch.isnan(self.mu).any()):
            raise ValueError('PredictiveMixture: NaN among the component means')
        self.S, self.M, self.K = (int(n) for n in mu.shape)
        self._host_moments = bool(host_moments)
        self._moments = None

    # ------------------------------------------------------------------ shapes
    def _flat(self):
        return self.mu.view(self.S, -1), self.variance.view(self.S, -1)

    def _thresholds(self, y, what):
        """y as Engine.mixture_eval takes it, and the shape of the result."""
        y = np.asarray(y, dtype=float)
        if y.shape == (self.M, self.K):
            return self.engine.tensor(y.reshape(-1, 1)), (self.M, self.K)
        if y.ndim == 3 and y.shape[:2] == (self.M, self.K) and y.shape[2] >= 1:
            return self.engine.tensor(y.reshape(self.M * self.K, -1)), y.shape
        if y.ndim == 1 and y.size >= 1:
            return self.engine.tensor(y), (self.M, self.K, y.size)
        raise Exception('%s: y has to be a numpy array of shape (%d, %d), (%d, %d, T) or (T,)' % (what, self.M, self.K, self.M, self.K))

    def _eval(self, what, y):
        yd, shape = self._thresholds(y, what)
        return self.engine.mixture_eval(what, *self._flat(), yd).cpu().numpy().reshape(shape)

    # ------------------------------------------------------------------ the distribution
    def mean(self):
        """mean_s mu_s, (M, K): predict's mean."""
        return self._two_moments()[0]

    def var(self):
        """mean_s(mu_s^2 + var_s) - mean^2, (M, K): predict's variance."""
        return self._two_moments()[1]

    def _two_moments(self):
        if self._moments is None:
            if self._host_moments:
                self._moments = host_moments(self.mu.cpu().numpy(), self.variance.cpu().numpy())
            else:   # (emulator._aggregate's calls: the same kernels in the same order, the same bits)
                e = self.engine
                s1, s2 = e.zeros(self.M, self.K), e.zeros(self.M, self.K)
                for s in range(self.S):
                    e.moments_accumulate(self.mu[s], self.variance[s], s1, s2)
                e.moments_finalize(self.S, s1, s2)
                self._moments = (s1.cpu().numpy(), s2.cpu().numpy())
        return self._moments

    def cdf(self, y):
        """P(Y <= y).  y (M, K) -> (M, K); (M, K, T) -> (M, K, T); 1-d (T,) thresholds shared by every point -> (M, K, T)."""
        return self._eval('cdf', y)

    def sf(self, y):
        """P(Y > y), summed from the components' upper tails (accurate where cdf rounds to 1).  Shapes as cdf."""
        return self._eval('sf', y)

    def logpdf(self, y):
        """The log of the mixture density (the log score is its negative); -inf where every component is a point mass.
        Shapes as cdf."""
        return self._eval('logpdf', y)

    def quantile(self, p):
        """inf{q : cdf(q) >= p}.  Scalar p in (0, 1) -> (M, K); 1-d p -> (M, K, T)."""
        p = np.asarray(p, dtype=float)
        if p.ndim > 1 or p.size < 1:
            raise Exception('quantile: p has to be a number or a 1-d array')
        if not np.all((p > 0.0) & (p < 1.0)):
            raise ValueError('quantile: p has to lie in (0, 1)')
        out, capped = self.engine.mixture_quantile(*self._flat(), p.reshape(-1))
        if capped:
            warnings.warn('quantile: %d results reached the iteration limit of the root search' % capped, RuntimeWarning)
        out = out.cpu().numpy()
        return out.reshape(self.M, self.K) if p.ndim == 0 else out.reshape(self.M, self.K, p.size)

    def interval(self, level=0.95):
        """The central interval of probability `level`: (lo, hi), each (M, K), the quantiles (1 -+ level) / 2."""
        if not 0.0 < level < 1.0:
            raise ValueError('interval: level has to lie in (0, 1)')
        q = self.quantile(np.array([0.5 * (1.0 - level), 0.5 * (1.0 + level)]))
        return q[..., 0], q[..., 1]

    def crps(self, y):
        """The continuous ranked probability score of the mixtures at the observations y (M, K) -> (M, K)."""
        y = np.asarray(y, dtype=float)
        if y.shape != (self.M, self.K):
            raise Exception('crps: y has to be a numpy array of shape (%d, %d)' % (self.M, self.K))
        return self.engine.mixture_crps(*self._flat(), self.engine.tensor(y.reshape(-1))).cpu().numpy().reshape(self.M, self.K)
