"""The predictive-mixture reference against itself, the public signatures and the library's symbols (no GPU)."""
import ctypes
import inspect
import os

import mpmath as mp
import numpy as np
import pytest

import mixture_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MU = [0.3, -1.2, 2.5, 0.9, 4.0]
VAR = [0.5, 2.0, 0.0, 0.01, 1.5]     # (a point mass among the components)


def test_crps_formula_is_the_integral_of_the_squared_cdf_error():
    """CRPS = int (F(t) - 1{t >= y})^2 dt, by Gauss-Legendre on the pieces between the kinks (y and the point mass)."""
    y = 1.1
    F = lambda t: R._exact_cdf(MU, VAR, t)
    g = lambda t: (F(t) - (1 if t >= y else 0)) ** 2
    integral = mp.quad(g, [-40, -5, 0.3, 0.9, y, 2.5, 4.0, 10, 40])
    assert abs(integral - R.crps(MU, VAR, y)) < mp.mpf(10) ** -25


def test_equal_components_are_one_gaussian():
    mu, var = [0.7] * 6, [2.3] * 6
    for y in (-3.0, 0.7, 5.5):
        assert abs(R.cdf(mu, var, y) - mp.ncdf(y, mu[0], mp.sqrt(mp.mpf(var[0])))) < mp.mpf(10) ** -45
        assert abs(R.sf(mu, var, y) + R.cdf(mu, var, y) - 1) < mp.mpf(10) ** -45
        assert abs(R.logpdf(mu, var, y) - mp.log(mp.npdf(y, mu[0], mp.sqrt(mp.mpf(var[0]))))) < mp.mpf(10) ** -45
        one = R.crps(mu[:1], var[:1], y)
        assert abs(R.crps(mu, var, y) - one) < mp.mpf(10) ** -45
        sd = mp.sqrt(mp.mpf(var[0]))
        z = (mp.mpf(y) - mu[0]) / sd
        closed = sd * (z * (2 * mp.ncdf(z) - 1) + 2 * mp.npdf(z) - 1 / mp.sqrt(mp.pi))   # (Gneiting & Raftery 2007, eq. 21)
        assert abs(one - closed) < mp.mpf(10) ** -45
    q = R.quantile(mu, var, 0.975)
    assert abs(q - (mu[0] + mp.sqrt(2) * mp.erfinv(0.95) * mp.sqrt(mp.mpf(var[0])))) < mp.mpf(10) ** -28


@pytest.mark.parametrize('p', [1e-6, 0.025, 0.2, 0.5, 0.9, 1 - 1e-6])
def test_the_components_own_quantiles_bracket_the_mixture_quantile(p):
    zp = mp.sqrt(2) * mp.erfinv(2 * mp.mpf(p) - 1)
    ends = [mp.mpf(m) + zp * mp.sqrt(mp.mpf(v)) for m, v in zip(MU, VAR)]
    lo, hi = min(ends), max(ends)
    q = R.quantile(MU, VAR, p)
    assert lo <= q <= hi
    assert R._exact_cdf(MU, VAR, hi) >= p
    tiny = mp.mpf(10) ** -20
    assert R._exact_cdf(MU, VAR, lo - tiny) <= p
    # the generalised inverse: F(q) >= p and F just below q is < p -- also when q is the point mass
    assert R._exact_cdf(MU, VAR, q) >= p and R._exact_cdf(MU, VAR, q - tiny) < p


def test_quantile_at_a_jump_is_the_point_mass():
    below = float(R._exact_cdf(MU, VAR, mp.mpf(2.5) - mp.mpf(10) ** -20))
    assert abs(R.quantile(MU, VAR, below + 0.1) - 2.5) < mp.mpf(10) ** -25


def test_bounds_are_positive_and_grow_with_the_constant():
    for y in (-2.0, 0.9, 2.5, 30.0):
        b = R.cdf_bound(MU, VAR, y)
        assert b > 0 and b < R.cdf_bound(MU, VAR, y, c=16.0) <= 2 * b     # (the summation term does not scale with C)
        assert R.crps_bound(MU, VAR, y) > 0 and R.logpdf_bound(MU, VAR, y) > 0
    ok, ratio, _ = R.quantile_check(MU, VAR, 0.3, float(R.quantile(MU, VAR, 0.3)))
    assert ok and ratio <= 1
    ok, _, _ = R.quantile_check(MU, VAR, 0.3, float(R.quantile(MU, VAR, 0.3)) + 1e-9)
    assert not ok


def test_numpy_formulas_agree_with_the_reference():
    mu, var = np.array(MU)[[0, 1, 3, 4], None], np.array(VAR)[[0, 1, 3, 4], None]
    y = np.array([0.4])
    assert abs(R.np_cdf(mu, var, y)[0] - float(R.cdf(mu[:, 0], var[:, 0], 0.4))) < 1e-15
    assert abs(R.np_crps(mu, var, y)[0] - float(R.crps(mu[:, 0], var[:, 0], 0.4))) < 1e-14


def test_public_signatures():
    from dgp_amd import emulator, gp, lgp
    from dgp_amd.mixture import PredictiveMixture
    sig = lambda f: str(inspect.signature(f))
    assert sig(emulator.predict_dist) == '(self, x, m=50)'
    assert sig(emulator.loo_dist) == '(self, X, m=30)'
    assert sig(gp.predict_dist) == '(self, x, m=50)'
    assert sig(lgp.predict_dist) == '(self, x, m=50)'
    assert sig(PredictiveMixture.interval) == '(self, level=0.95)'
    for name, want in (('mean', '(self)'), ('var', '(self)'), ('cdf', '(self, y)'), ('sf', '(self, y)'), ('logpdf', '(self, y)'),
                       ('quantile', '(self, p)'), ('crps', '(self, y)')):
        assert sig(getattr(PredictiveMixture, name)) == want


def test_library_has_the_three_entries():
    lib = ctypes.CDLL(os.path.join(ROOT, 'dgp_amd', 'libdgp_amd.so'))
    for name in ('dgpamd_mixture_eval', 'dgpamd_mixture_quantile', 'dgpamd_mixture_crps'):
        assert hasattr(lib, name), name
    from dgp_amd import _lib
    assert all(n in _lib.SIGNATURES for n in ('dgpamd_mixture_eval', 'dgpamd_mixture_quantile', 'dgpamd_mixture_crps'))


def test_entries_refuse_bad_arguments_without_a_context_or_a_launch():
    """A null context is refused first; the other host-side checks are exercised by tools/mixture_args_check.cpp."""
    from dgp_amd._lib import lib, BAD_ARG
    assert lib.dgpamd_mixture_eval(None, 0, 1, 0, 1, None, None, None, 0, None) == BAD_ARG
    assert lib.dgpamd_mixture_quantile(None, 1, 0, 1, None, None, None, None, 0, None, None) == BAD_ARG
    assert lib.dgpamd_mixture_crps(None, 1, 0, None, None, None, 0, None) == BAD_ARG
